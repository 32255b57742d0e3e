"""The surfel lifecycle under KEYFRAME sharding (bahip_context_set_keyframe_sharding): the batched creation, the merge batch by bound
keyframe index, deletion + radii and compaction.

A rank holds the whole cloud and the images of its own keyframes only (k % world == rank).  The image reads of a batch are dealt out
by owner and exchanged as zero-filled partials or integer counts (BAHIP_SUM_I64); the order-dependent rest -- the creation chain, the
merge decisions, the deletion decision -- runs on every rank.  So every rank ends with the unsharded call's bits.  Ranks are threads
on one GPU with the in-process loopback all-reduce of tests/test_gpu_keyframe_sharded_intrinsics.py."""
import ctypes as C
import time

import numpy as np
import pytest

from badslam_amd import capi, synthetic
from tests import common
from tests.test_gpu_keyframe_sharded_intrinsics import _bits, _run_ranks

pytestmark = pytest.mark.gpu

KEYFRAMES = 10
CREATE = [3, 5, 4, 7, 6, 9, 8]          # a creation batch in an order that crosses the ranks
MERGE = [2, 7, 4, 9, 0, 5, 3, 8]        # a merge batch: a permuted subset of the bound keyframes


def _scene():
    scene = common.small_scene(num_keyframes=KEYFRAMES, seed=41)
    rng = np.random.Generator(np.random.PCG64(17))
    poses = [T if k % 3 == 0 else synthetic.perturb_pose(rng, T, 0.01, 0.004) for k, T in enumerate(scene.poses_gt)]
    return scene, poses


def _frame_T_global_3x4(global_T_frame):
    """se3_device.h: se3_matrix3x4(se3_inverse(T)) operation for operation in binary32 -- the 12 coefficients bahip_set_keyframes keeps."""
    f = np.float32
    a = [f(v) for v in global_T_frame]
    q = [-a[0], -a[1], -a[2], a[3]]
    v = [a[4] * f(-1), a[5] * f(-1), a[6] * f(-1)]
    ux = f(2) * (q[1] * v[2] - q[2] * v[1])
    uy = f(2) * (q[2] * v[0] - q[0] * v[2])
    uz = f(2) * (q[0] * v[1] - q[1] * v[0])
    t = [v[0] + q[3] * ux + (q[1] * uz - q[2] * uy), v[1] + q[3] * uy + (q[2] * ux - q[0] * uz), v[2] + q[3] * uz + (q[0] * uy - q[1] * ux)]
    x, y, z, w = q
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([f(1) - (tyy + tzz), txy - twz, txz + twy, t[0], txy + twz, f(1) - (txx + tzz), tyz - twx, t[1],
                     txz - twy, tyz + twx, f(1) - (txx + tyy), t[2]], np.float32)


def _build(scene, poses, capacity=900000):
    g = common.build_gpu(scene, capacity, poses=poses, create_from=[0, 1, 2])   # (unsharded: the cloud every rank starts from)
    g.set_sum_classes(8)
    return g


def _state(g):
    g.ctx.synchronize()
    return dict(size=g.surfels_size, rows=g.surfel_buf.download()[:8, :g.surfels_size].copy().view(np.uint32))


def _stages(g, min_obs):
    """A filtered creation batch, a batch of one keyframe, a merge batch by index, deletion + radii, compaction."""
    out = {}
    with g.lifecycle_batch(keyframes=CREATE):
        out["new"] = g.create_surfels_for_keyframes([(k, None) for k in CREATE], filter_new_surfels=True, min_observation_count=min_obs)
    out["after_create"] = _state(g)
    with g.lifecycle_batch(keyframes=[1]):
        out["new_one"] = g.create_surfels_for_keyframes([(1, [0, 2, 5, 6, 9])], filter_new_surfels=True, min_observation_count=min_obs)
    out["after_create_one"] = _state(g)
    with g.lifecycle_batch(keyframes=MERGE):
        _, out["merged"] = g.merge_surfels_for_bound_keyframes(MERGE, merge_dist_factor=0.8)
    out["after_merge"] = _state(g)
    out["deleted"] = g.delete_surfels_and_update_radii(min_obs)
    out["after_delete"] = _state(g)
    n = g.surfels_size
    out["accum"] = g.surfel_buf.download()[8:11, :n].copy().view(np.uint32)       # observations, violations, minimum radius
    g.compact_surfels(with_active=False)
    out["after_compact"] = _state(g)
    return out


def _compare(got, ref, where):
    for key, value in ref.items():
        if isinstance(value, dict):
            assert got[key]["size"] == value["size"], (where, key)
            assert np.array_equal(got[key]["rows"], value["rows"]), (where, key, np.flatnonzero((got[key]["rows"] != value["rows"]).any(axis=0))[:10])
        elif isinstance(value, np.ndarray):
            assert np.array_equal(got[key], value), (where, key)
        else:
            assert got[key] == value, (where, key, got[key], value)


# ---- (1) stage by stage, against the unsharded context --------------------------------------------------------------------------
@pytest.mark.parametrize("min_obs", [2, 3])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_keyframe_shards_reproduce_the_unsharded_lifecycle_stages(world, min_obs):
    """Every rank ends every stage with the unsharded run's rows 0-7, size and counts (and deletion's accumulator rows); at world 2,
    rank 1 is handed its non-owned keyframes' frames with scrambled images, which the backend must not look at."""
    import torch
    torch.cuda.set_device(0)
    scene, poses = _scene()
    ref = _stages(_build(scene, poses), min_obs)
    assert ref["new"] > 100 and ref["merged"] > 0 and ref["deleted"] > 0, {k: ref[k] for k in ("new", "new_one", "merged", "deleted")}

    def rank_main(rank, hook):
        g = _build(scene, poses)
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, hook, None))
        g.set_keyframe_sharding(rank, world)
        if world == 2 and rank == 1:
            rng = np.random.Generator(np.random.PCG64(3))
            for k in range(0, KEYFRAMES, 2):                                   # rank 0's keyframes: scrambled, and handed over
                for which in ("depth", "normals", "radius"):
                    buf = g.keyframes[k][which]
                    buf.upload(rng.integers(0, 1 << 16, size=(buf.height, buf.width), dtype=np.uint16))
            g.kf_shard = (0, 1)                                                 # (bind_keyframes then passes every frame's pointers)
        calls = C.c_longlong()
        out = _stages(g, min_obs)
        capi.check(g.ctx.lib.bahip_exchange_stats(g.ctx.handle, C.byref(calls), None, 0))
        out["exchanges"] = calls.value
        out["keep"] = (hook, g)
        return out

    results, loop = _run_ranks(world, rank_main)
    for rank, r in enumerate(results):
        _compare(r, ref, rank)
    # candidates + filter counts + records + one occupancy row per keyframe after the first; the same for the batch of one without
    # the rows (records only if it has a candidate); counts + members of the merge; one of the deletion
    assert results[0]["exchanges"] == (3 + len(CREATE) - 1) + (2 + (ref["new_one"] > 0)) + 2 + 1, results[0]["exchanges"]


def test_keyframe_sharded_creation_respects_the_capacity():
    """A keyframe of the chain that does not fit creates nothing and raises the flag on every rank, the ones behind it go on."""
    import torch
    torch.cuda.set_device(0)
    scene, poses = _scene()
    probe = _build(scene, poses)
    with probe.lifecycle_batch(keyframes=CREATE):
        full = probe.create_surfels_for_keyframes([(k, None) for k in CREATE], filter_new_surfels=False)
    base = _build(scene, poses).surfels_size
    capacity = base + full // 2

    def run(g):
        with g.lifecycle_batch(keyframes=CREATE):
            created = g.create_surfels_for_keyframes([(k, None) for k in CREATE], filter_new_surfels=False)
        exceeded = g.ctx.lib.bahip_context_take_capacity_exceeded(g.ctx.handle)
        return dict(created=created, exceeded=exceeded, state=_state(g))

    ref = run(_build(scene, poses, capacity))
    assert ref["exceeded"] == 1 and 0 < ref["created"] < full

    def rank_main(rank, hook):
        g = _build(scene, poses, capacity)
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, hook, None))
        g.set_keyframe_sharding(rank, 4)
        out = run(g)
        out["keep"] = (hook, g)
        return out

    results, _ = _run_ranks(4, rank_main)
    for rank, r in enumerate(results):
        _compare(r, ref, rank)


# ---- (2) the by-index merge, unsharded, is the frame-based call ----------------------------------------------------------------
@pytest.mark.parametrize("order", [MERGE, list(range(KEYFRAMES)), [6]])
def test_merge_by_bound_index_is_the_frame_based_merge(order):
    scene, poses = _scene()
    outs = []
    for by_index in (False, True):
        g = _build(scene, poses)
        with g.lifecycle_batch(keyframes=CREATE):
            g.create_surfels_for_keyframes([(k, None) for k in CREATE], filter_new_surfels=True, min_observation_count=2)
        Fs = [_frame_T_global_3x4(g.keyframes[k]["pose"]) for k in order]
        with g.lifecycle_batch(keyframes=order):                                # (the frames' lists are found by these coefficients)
            if by_index:
                _, merged = g.merge_surfels_for_bound_keyframes(order, merge_dist_factor=0.8)
            else:
                _, merged = g.merge_surfels_for_keyframes(order, Fs, merge_dist_factor=0.8)
        outs.append((merged, _state(g), _merge_cells_batches()))
    assert outs[0][0] == outs[1][0] and (outs[0][0] > 0 or len(order) == 1)
    assert outs[0][1]["size"] == outs[1][1]["size"] and np.array_equal(outs[0][1]["rows"], outs[1][1]["rows"])
    assert outs[1][2] - outs[0][2] == 1                                         # both by cell lists: the frames' lists were found


def _merge_cells_batches():
    n = C.c_longlong()
    capi.check(capi.load().bahip_debug_merge_cells_batches(C.byref(n)))
    return int(n.value)


# ---- (3) DirectBA, eight ranks, configs[2]-shaped slice -----------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["alternating", "pcg", "joint"])
def test_eight_keyframe_shards_of_directba_with_surfel_updates_are_the_unsharded_call(scheme):
    """BundleAdjustment(do_surfel_updates = true, increase_ba_iteration_count = true) of eight DirectBA instances in lockstep on one GPU
    (SetKeyframeSharding(rank, 8), SetSumClasses(8); SetPCGSumClasses(8) for PCG; SetIntrinsicsSumClasses(8) and the intrinsics flags
    for the joint BA of configs[4]), on a slice of the configs[2] scene (640 x 480, 16 keyframes) with a third of its surfels missing,
    so that creation runs: every rank ends with the unsharded call's surfels, count, poses and statistics, bit for bit."""
    import torch
    from badslam_amd.directba import DirectBA
    from tests.test_gpu_scale_parity import _bench_scene
    torch.cuda.set_device(0)
    bench_ba, data, poses_gt, args = _bench_scene(width=640, height=480, keyframes=16, surfels=10 ** 9)
    frames = args.frames
    K, WORLD = bench_ba.keyframe_count(), 8
    start_poses = [bench_ba.keyframe_pose(k) for k in range(K)]
    bench_ba.close()
    data = np.ascontiguousarray(data[:, :data.shape[1] * 2 // 3])
    N = data.shape[1]
    cam = common.synthetic.test_camera(args.width, args.height)
    joint = scheme == "joint"
    call = dict(optimize_depth_intrinsics=joint, optimize_color_intrinsics=joint, do_surfel_updates=True, optimize_poses=True,
                optimize_geometry=True, min_iterations=1, max_iterations=1 if scheme == "alternating" else 2, use_pcg=scheme == "pcg",
                active_keyframe_window_start=0, active_keyframe_window_end=K - 1, increase_ba_iteration_count=True, pcg_max_inner_iterations=10)

    def build():
        rb = DirectBA(3 * N, 1.0 / 5000, 40.0, args.cell, args.width, args.height, cam, cam)
        for (raw, rgb), T in zip(frames, poses_gt):
            rb.AddKeyframe(raw, rgb, T)
        for k, T in enumerate(start_poses):
            rb.set_keyframe_pose(k, T)
        rb.upload_surfels(data)
        rb.set_ba_iteration_counts(1, 1)
        rb.SetSumClasses(8)
        rb.SetPCGSumClasses(8)
        rb.SetIntrinsicsSumClasses(8)
        if scheme == "pcg":
            rb.set_pcg_gauge_keyframe(0)
        return rb

    def outcome(rb, done):
        return dict(done=done, stats=rb.last_stats(), count=rb.surfel_count(), size=rb.surfels_size(),
                    poses=np.asarray([rb.keyframe_pose(k) for k in range(K)], np.float32), surfels=rb.download_surfels(8),
                    cameras=rb.cameras())

    rb = build()
    ref = outcome(rb, rb.BundleAdjustment(**call)[0])
    rb.close()
    assert ref["size"] != N, "the call changed nothing in the cloud"

    ranks = [build() for _ in range(WORLD)]

    def rank_main(rank, hook):
        rb = ranks[rank]
        capi.check(capi.load().bahip_context_set_allreduce(rb.backend_context().handle, hook, None))
        rb.SetKeyframeSharding(rank, WORLD)
        h = rb.backend_context().handle
        capi.check(capi.load().bahip_exchange_stats(h, None, None, 1))
        out = outcome(rb, rb.BundleAdjustment(**call)[0])
        calls, nbytes = C.c_longlong(), C.c_longlong()
        capi.check(capi.load().bahip_exchange_stats(h, C.byref(calls), C.byref(nbytes), 0))
        out["exchanges"] = (calls.value, nbytes.value)
        out["keep"] = hook
        return out

    t0 = time.perf_counter()
    results, loop = _run_ranks(WORLD, rank_main, timeout=1200)
    wall = time.perf_counter() - t0
    for rb in ranks:
        rb.close()
    calls, nbytes = results[0]["exchanges"]
    print(f"eight keyframe shards of DirectBA ({scheme}, surfel updates and end tasks, {N} surfels at the start, {ref['size']} at the end) "
          f"in loopback (one GPU, threads -- not a link measurement): {calls} exchanges, {nbytes / 1e6:.1f} MB per rank, {wall:.2f} s wall")
    for rank, r in enumerate(results):
        assert (r["done"], r["count"], r["size"]) == (ref["done"], ref["count"], ref["size"]), rank
        assert r["stats"] == ref["stats"], rank
        for key in ("poses", "surfels"):
            assert np.array_equal(_bits(r[key]), _bits(ref[key])), (rank, key)
        cams = [np.concatenate([np.asarray(x[0], np.float32), np.asarray(x[1], np.float32), [np.float32(x[2])]]) for x in (r["cameras"], ref["cameras"])]
        assert np.array_equal(_bits(cams[0]), _bits(cams[1])), rank


# ---- (4) robustness and refusals ----------------------------------------------------------------------------------------------
class _FailAt:
    """A hook that passes the first `ok` exchanges to the loopback and fails the next one."""

    def __init__(self, ok):
        self.ok, self.seen = ok, 0

    def wrap(self, inner):
        def _hook(ptr, count, dtype, stream, user):
            self.seen += 1
            if self.seen > self.ok:
                return 1
            return inner(ptr, count, dtype, stream, user)
        return capi.ALLREDUCE_FN(_hook)


@pytest.mark.parametrize("stage,ok", [("create", 0), ("create", 1), ("create", 2), ("create", 3), ("merge", 0), ("merge", 1), ("delete", 0)])
def test_a_failing_exchange_fails_the_stage_and_leaves_the_context_usable(stage, ok):
    """One rank alone (world 2, rank 0) with a hook that fails at a stage's (ok + 1)-th exchange: the call fails with the standard
    message; the context then runs the same stage unsharded with the unsharded bits (deletion: rows 0-7 untouched by the failure)."""
    import torch
    torch.cuda.set_device(0)
    scene, poses = _scene()

    def run(g):
        if stage == "create":
            with g.lifecycle_batch(keyframes=CREATE):
                n = g.create_surfels_for_keyframes([(k, None) for k in CREATE], filter_new_surfels=True, min_observation_count=2)
        elif stage == "merge":
            with g.lifecycle_batch(keyframes=MERGE):
                _, n = g.merge_surfels_for_bound_keyframes(MERGE, merge_dist_factor=0.8)
        else:
            n = g.delete_surfels_and_update_radii(2)
        return n, _state(g)

    ref = run(_build(scene, poses))
    g = _build(scene, poses)
    before = _state(g)
    fail = _FailAt(ok)
    hook = fail.wrap(lambda *a: 0)                                              # (the exchanges that pass change nothing: a lone rank)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, hook, None))
    g.set_keyframe_sharding(0, 2)
    with pytest.raises(RuntimeError, match="keyframe sharding: the exchange of "):
        run(g)
    assert fail.seen == ok + 1
    if stage == "delete":
        assert np.array_equal(_state(g)["rows"], before["rows"])
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, capi.ALLREDUCE_FN(), None))
    g.set_keyframe_sharding(0, 1)
    g.surfels_size, g.surfel_count = before["size"], before["size"]
    g.upload_surfels(before["rows"].view(np.float32), np.ones(before["size"], np.uint8))
    n, state = run(g)
    assert n == ref[0]
    assert state["size"] == ref[1]["size"] and np.array_equal(state["rows"], ref[1]["rows"])


def test_what_the_keyframe_sharded_lifecycle_refuses():
    import torch
    torch.cuda.set_device(0)
    scene, poses = _scene()
    g = _build(scene, poses)
    lib, h = g.ctx.lib, g.ctx.handle
    g.set_keyframe_sharding(1, 2)
    g.bind_keyframes()
    for call in (lambda: g.delete_surfels_and_update_radii(2),
                 lambda: g.create_surfels_for_keyframes([(3, None)], filter_new_surfels=True),
                 lambda: g.merge_surfels_for_bound_keyframes([3, 4])):
        with pytest.raises(RuntimeError, match="keyframe sharding needs an all-reduce hook or an RCCL communicator"):
            call()
    hook = capi.ALLREDUCE_FN(lambda *a: 1)                                      # (a refused call never reaches the exchange)
    capi.check(lib.bahip_context_set_allreduce(h, hook, None))
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.create_surfels_for_keyframe(3, filter_new_surfels=True)
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.determine_supporting_surfels(3, np.eye(4, dtype=np.float32)[:3].ravel(), merge=True)
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        capi.check(lib.bahip_assign_colors(h, C.byref(g.surfels_struct())))
    with g.lifecycle_batch(keyframes=MERGE):
        with pytest.raises(RuntimeError, match="keyframe sharding.*bahip_merge_surfels_for_bound_keyframes"):
            g.merge_surfels_for_keyframes([3], [np.eye(4, dtype=np.float32)[:3].ravel()])
    with pytest.raises(RuntimeError, match="keyframe sharding: bahip_merge_surfels_for_bound_keyframes needs an open lifecycle batch"):
        g.merge_surfels_for_bound_keyframes([3, 4])                             # outside a batch that knows its keyframes
    with g.lifecycle_batch(keyframes=[3, 4]):
        with pytest.raises(RuntimeError, match="keyframe sharding: bahip_merge_surfels_for_bound_keyframes needs an open lifecycle batch"):
            g.merge_surfels_for_bound_keyframes([3, 5])                         # keyframe 5 is not one of the batch's
