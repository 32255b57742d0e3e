"""The intrinsics step under KEYFRAME sharding (bahip_context_set_keyframe_sharding + bahip_context_set_intrinsics_sum_classes).

The 34 global sums of the step (A, b1, colour H, colour b) are defined over C keyframe classes: per surfel and class a binary32
chain over the class's keyframes (k % C == c) in ascending order, per 64-surfel tile and class the xor butterfly, then binary64
over all (tile, class) values (kernels_intrinsics.hip).  C = 1 (default) is the one chain over all keyframes of before.  A rank
that holds whole classes sweeps its own and the binary64 accumulators are summed over the ranks, so every rank ends with the bits
of the unsharded run with the same C.  The definition is pinned to the oracle: orc_intrinsics_accumulate over one class's keyframes
(the others passed as NULL, which the oracle skips) is exactly that class's chains."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

ITERATIONS = 3
DEPTH_OFFSET = (0.5, -0.6, 1.23, -2.17)
COLOR_OFFSET = (0.4, -0.3, 0.8, -0.6)


def _bits(values):
    return np.ascontiguousarray(np.asarray(values, np.float32)).view(np.uint32)


def _cam(c):
    return np.array([c.fx, c.fy, c.cx, c.cy], np.float32)


def _perturb(obj):
    for name, off in (("depth_cam", DEPTH_OFFSET), ("color_cam", COLOR_OFFSET)):
        cam = getattr(obj, name)
        cam.fx += off[0]; cam.fy += off[1]; cam.cx += off[2]; cam.cy += off[3]


class _Loopback:
    """Sum-all-reduce between host threads that share one device, in a fixed rank order (as tests/test_gpu_sharded_loopback.py)."""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.ptrs = [None] * world
        self.calls = 0

    def hook_for(self, rank):
        import torch
        from badslam_amd import capi, multigpu

        def _hook(device_ptr, count, dtype, _stream, _user):
            try:
                torch.cuda.synchronize()
                self.ptrs[rank] = (device_ptr, count, dtype)
                self.barrier.wait(timeout=120)
                if rank == 0:
                    views = [torch.as_tensor(multigpu._DevicePtrView(p, n, d), device="cuda") for p, n, d in self.ptrs]
                    total = views[0].clone()
                    for v in views[1:]:
                        total += v
                    for v in views:
                        v.copy_(total)
                    torch.cuda.synchronize()
                    self.calls += 1
                self.barrier.wait(timeout=120)
                return 0
            except Exception as e:   # noqa: BLE001 -- surfaces as a bahip error in the calling thread
                print("loopback all-reduce failed:", e, flush=True)
                self.barrier.abort()
                return 1

        return capi.ALLREDUCE_FN(_hook)


def _run_ranks(world, rank_main, timeout=600):
    loop = _Loopback(world)
    results, errors = [None] * world, []

    def main(rank):
        try:
            import torch
            torch.cuda.set_device(0)
            results[rank] = rank_main(rank, loop.hook_for(rank))
        except Exception as e:   # noqa: BLE001
            errors.append((rank, repr(e)))
            loop.barrier.abort()

    threads = [threading.Thread(target=main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not errors, errors
    assert all(r is not None for r in results)
    return results, loop


# ---- (a) the default is the definition of before -----------------------------------------------------------------------------
def test_class_count_set_back_to_one_is_the_default_step():
    """C = 4 and back to 1 on one context: the next step is bit for bit the step of a fresh context (cameras, a, cfactor)."""
    import torch
    torch.cuda.set_device(0)
    scene = common.small_scene(num_keyframes=5, seed=21)

    def step(g):
        _perturb(g)
        g.set_intrinsics()
        g.bind_keyframes()
        cc, dc, a = g.optimize_intrinsics(True, True)
        return _cam(cc), _cam(dc), np.float32(a), g.cfactor.download()

    fresh = step(common.build_gpu(scene, 400000))
    g = common.build_gpu(scene, 400000)
    g.set_intrinsics_sum_classes(4)
    g.set_intrinsics_sum_classes(1)
    toggled = step(g)
    assert np.count_nonzero(fresh[3]) > 0.5 * fresh[3].size
    for x, y in zip(fresh, toggled):
        assert np.array_equal(_bits(x), _bits(y))


# ---- (b) the class definition, held against the oracle -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def pinned_pair():
    """Oracle + GPU scenes with identical surfels, identically perturbed cameras and the same non-zero depth deformation (a and the
    cfactor cells: every term of the 5 x 5 block is non-zero), 9 keyframes (every class of C = 8 has one).  Returns the cfactor cells
    too: the GPU step updates them, each test uploads them again."""
    scene = common.small_scene(num_keyframes=9, seed=21)
    ba = common.build_oracle(scene, 600000)
    g = common.build_gpu(scene, 600000, create_from=[])
    data, active = common.oracle_surfels(ba)
    g.upload_surfels(data, np.ones_like(active))
    ba.active[:data.shape[1]] = 1
    for obj in (ba, g):
        _perturb(obj)
        obj.dp.a = 0.0125
    cfactor = np.random.Generator(np.random.PCG64(5)).uniform(-0.01, 0.01, ba.cfactor.shape).astype(np.float32)
    ba.cfactor[...] = cfactor
    g.set_intrinsics()
    g.bind_keyframes()
    return ba, g, cfactor


def _oracle_class_sums(ba, classes):
    """orc_intrinsics_accumulate once per class (the other classes' keyframes NULL), the per-class results added in binary64."""
    from oracle import binding as ob
    S = ba.cf_w * ba.cf_h
    glob, cells = np.zeros(34, np.float64), np.zeros((S, 8), np.float64)
    n = len(ba.keyframes)
    for c in range(classes):
        arr = (C.POINTER(ob.Keyframe) * n)()
        for k in range(n):
            if k % classes == c:
                arr[k] = C.pointer(ba.keyframes[k])
        part = np.zeros(34, np.float64)
        ba.L.orc_intrinsics_accumulate.restype = None
        ba.L.orc_intrinsics_accumulate(1, 1, arr, n, C.byref(ba.color_cam), C.byref(ba.depth_cam), C.byref(ba.dp), C.byref(ba.surfels),
                                       part.ctypes.data_as(C.POINTER(C.c_double)), cells.ctypes.data_as(C.POINTER(C.c_double)))
        glob += part
    return glob, cells


@pytest.mark.parametrize("classes", [1, 2, 8])
def test_class_sums_are_the_oracle_accumulators_per_class(pinned_pair, classes):
    ba, g, cfactor = pinned_pair
    g.set_intrinsics_sum_classes(classes)
    try:
        g.cfactor.upload(cfactor)                         # (the step updates the deformation cells; the oracle's stay)
        g.optimize_intrinsics(True, True, apply=False)
        got, got_cells = g.read_intrinsics_sums()
    finally:
        g.set_intrinsics_sum_classes(1)
    ref, ref_cells = _oracle_class_sums(ba, classes)
    assert np.array_equal(_bits(got), _bits(ref.astype(np.float32))), np.flatnonzero(_bits(got) != _bits(ref.astype(np.float32)))
    assert np.array_equal(_bits(got_cells), _bits(ref_cells.astype(np.float32)))
    assert np.count_nonzero(got) == 34
    assert np.count_nonzero(got_cells[:, 7]) > 0.5 * got_cells.shape[0]
    if classes == 1:
        plain, plain_cells = ba.intrinsics_accumulators(True, True)       # the binding's own call: all keyframes in one chain
        assert np.array_equal(_bits(got), _bits(plain.astype(np.float32)))
    else:
        one, _ = _oracle_class_sums(ba, 1)
        # the class count is part of the definition: the binary32 chains split in classes round differently (in the binary64 sums;
        # their rounding to binary32 may or may not show it)
        assert not np.array_equal(ref, one)


# ---- (c) loopback parity: keyframe shards vs the unsharded run with the same class counts ------------------------------------
@pytest.mark.parametrize("world,arithmetic", [(2, "exact"), (2, "fast"), (4, "exact"), (8, "exact"), (8, "fast")])
def test_keyframe_shards_with_intrinsics_reproduce_the_unsharded_run(world, arithmetic):
    """Three alternating iterations of geometry, poses and the depth + colour intrinsics step from perturbed cameras: every rank ends
    with the unsharded run's surfels (rows 0-7), active flags, poses, cameras, a and cfactor, bit for bit."""
    import torch
    from badslam_amd import capi
    torch.cuda.set_device(0)
    scene = common.small_scene(num_keyframes=7 if world < 8 else 11, seed=21)
    rng = np.random.Generator(np.random.PCG64(4))
    start_poses = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    classes = 8 if world == 8 else 4

    g = common.build_gpu(scene, 500000)
    data = g.download_surfels()
    data[2] += rng.uniform(0, 0.004, data.shape[1]).astype(np.float32)
    N = data.shape[1]

    def prepare(gr):
        gr.ctx.set_arithmetic(arithmetic)
        gr.set_sum_classes(classes)
        gr.set_intrinsics_sum_classes(classes)
        gr.upload_surfels(data, np.ones(N, np.uint8))
        for k, T in enumerate(start_poses):
            gr.keyframes[k]["pose"] = np.asarray(T, np.float32)
        _perturb(gr)
        gr.set_intrinsics()

    def run(gr):
        out = []
        for _ in range(ITERATIONS):
            for kf in gr.keyframes:
                kf["activation"] = capi.KF_ACTIVE
            gr.bind_keyframes()
            gr.update_surfel_activation()
            gr.optimize_geometry_iteration(True, True)
            poses, its, conv, rounds = gr.estimate_keyframe_poses(True, True)
            for k, kf in enumerate(gr.keyframes):
                kf["pose"] = poses[k].astype(np.float32)
            gr.bind_keyframes()
            gr.optimize_intrinsics(True, True)
            out.append((rounds, tuple(its)))
        return dict(out=out, surfels=gr.download_surfels()[:8], active=gr.active_buf.download().ravel()[:N].copy(),
                    poses=[kf["pose"].copy() for kf in gr.keyframes], color=_cam(gr.color_cam), depth=_cam(gr.depth_cam),
                    a=np.float32(gr.dp.a), cfactor=gr.cfactor.download())

    prepare(g)
    ref = run(g)

    def rank_main(rank, hook):
        gr = common.build_gpu(scene, 500000, create_from=[])
        prepare(gr)
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        gr.set_keyframe_sharding(rank, world)
        out = run(gr)
        out["keep"] = (hook, gr)
        return out

    results, loop = _run_ranks(world, rank_main)
    assert loop.calls >= 4 * ITERATIONS
    for r in results:
        assert r["out"] == ref["out"]
        for k in range(len(start_poses)):
            assert np.array_equal(ref["poses"][k], r["poses"][k]), (k, common.pose_error(ref["poses"][k], r["poses"][k]))
        assert np.array_equal(_bits(r["surfels"]), _bits(ref["surfels"]))
        assert np.array_equal(r["active"], ref["active"])
        for key in ("color", "depth", "a", "cfactor"):
            assert np.array_equal(_bits(r[key]), _bits(ref[key])), key
    # the steps did something: the cameras moved, the deformation field is populated
    perturbed = np.asarray(scene.camera, np.float64) + np.array(DEPTH_OFFSET)
    assert np.abs(ref["depth"] - perturbed.astype(np.float32)).max() > 0.02     # (the geometry step absorbs part of the offset)
    assert np.count_nonzero(ref["cfactor"]) > 0.5 * ref["cfactor"].size


# ---- (d) DirectBA on the configs[4] slice, eight keyframe shards ---------------------------------------------------------------
def test_c5_slice_eight_keyframe_shards_with_intrinsics_are_the_unsharded_call():
    """BASELINE configs[4] ("intrinsics + pose + surfel joint BA across 8 GPUs") sharded by keyframe: eight DirectBA instances in
    lockstep on one GPU, SetKeyframeSharding(rank, 8) with SetSumClasses(8) and SetIntrinsicsSumClasses(8), one BundleAdjustment
    iteration over geometry, poses, depth and colour intrinsics on the 1280 x 960, 20-keyframe slice.  Every rank ends with the
    unsharded call's poses, surfels, cameras, a and cfactor (same class counts), bit for bit.  The 8-class definition against the
    1-class one (everything else alike) is reported and held under a bound: measured on an MI355X, the two calls ended with the
    same bits (0 m, 0 px); the bound leaves room for binary32 rounding of the sums showing in the solves (1e-6 m, 1e-3 px)."""
    import torch
    from badslam_amd import capi, synthetic
    from badslam_amd.directba import DirectBA
    from tests.test_gpu_scale_parity import _bench_scene
    torch.cuda.set_device(0)
    bench_ba, data, poses_gt, args = _bench_scene(width=1280, height=960, keyframes=20, surfels=10 ** 9)
    frames = args.frames
    K, N, WORLD = bench_ba.keyframe_count(), data.shape[1], 8
    assert N > 1000000 and K == len(frames) == 20
    start_poses = [bench_ba.keyframe_pose(k) for k in range(K)]
    bench_ba.close()
    cam = synthetic.test_camera(args.width, args.height)
    depth_cam = cam.astype(np.float64) + np.array(DEPTH_OFFSET)
    color_cam = cam.astype(np.float64) + np.array(COLOR_OFFSET)
    call = dict(optimize_depth_intrinsics=True, optimize_color_intrinsics=True, do_surfel_updates=False, optimize_poses=True,
                optimize_geometry=True, min_iterations=1, max_iterations=1, active_keyframe_window_start=0, active_keyframe_window_end=K - 1,
                increase_ba_iteration_count=False)

    def build(intrinsics_classes):
        rb = DirectBA(N + 4096, 1.0 / 5000, 40.0, args.cell, args.width, args.height, cam, cam)
        for (raw, rgb), T in zip(frames, poses_gt):
            rb.AddKeyframe(raw, rgb, T)
        for k, T in enumerate(start_poses):
            rb.set_keyframe_pose(k, T)
        rb.upload_surfels(data)
        rb.set_cameras(color_cam, depth_cam, 0.0)
        rb.set_ba_iteration_counts(1, 1)                  # equal counters: no end-of-scheme tasks (fixed surfel set)
        rb.SetSumClasses(8)
        rb.SetIntrinsicsSumClasses(intrinsics_classes)
        return rb

    def outcome(rb, done):
        cc, dc, a = rb.cameras()
        return dict(done=done, poses=np.asarray([rb.keyframe_pose(k) for k in range(K)], np.float32), surfels=rb.download_surfels(8),
                    color=np.asarray(cc, np.float32), depth=np.asarray(dc, np.float32), a=np.float32(a), cfactor=rb.cfactor())

    refs = {}
    for classes in (8, 1):
        rb = build(classes)
        refs[classes] = outcome(rb, rb.BundleAdjustment(**call)[0])
        rb.close()
    ref = refs[8]
    assert ref["done"] == 1

    ranks = [build(8) for _ in range(WORLD)]

    def rank_main(rank, hook):
        rb = ranks[rank]
        capi.check(capi.load().bahip_context_set_allreduce(rb.backend_context().handle, hook, None))
        rb.SetKeyframeSharding(rank, WORLD)
        out = outcome(rb, rb.BundleAdjustment(**call)[0])
        out["keep"] = hook
        return out

    results, loop = _run_ranks(WORLD, rank_main, timeout=900)
    for rb in ranks:
        rb.close()
    for rank, r in enumerate(results):
        assert r["done"] == ref["done"], rank
        for key in ("poses", "surfels", "color", "depth", "a", "cfactor"):
            assert np.array_equal(_bits(r[key]), _bits(ref[key])), (rank, key)
    moved = np.abs(ref["depth"] - depth_cam.astype(np.float32)).max()
    assert moved > 0.1                                                            # the step did something

    # the 8-class definition against the 1-class one: how far one iteration's result moves
    one = refs[1]
    dpos = float(np.abs(ref["poses"][:, 4:].astype(np.float64) - one["poses"][:, 4:]).max())
    ddepth = np.abs(ref["depth"].astype(np.float64) - one["depth"])
    dcolor = np.abs(ref["color"].astype(np.float64) - one["color"])
    print(f"configs[4] slice, 8 classes vs 1 (one iteration, {N} surfels): |d position| <= {dpos:.3e} m, depth camera |d fx, fy, cx, cy| = "
          f"{np.array2string(ddepth, precision=3)} px, colour camera {np.array2string(dcolor, precision=3)} px, |d a| = {abs(float(ref['a']) - float(one['a'])):.3e}")
    assert dpos <= 1e-6
    assert ddepth.max() <= 1e-3 and dcolor.max() <= 1e-3


# ---- (e) what stays refused -------------------------------------------------------------------------------------------------
def test_what_keyframe_sharded_intrinsics_refuse():
    import torch
    from badslam_amd import capi
    torch.cuda.set_device(0)
    scene = common.small_scene(num_keyframes=3, seed=3)
    g = common.build_gpu(scene, 200000)
    lib, h = g.ctx.lib, g.ctx.handle
    for bad in (0, 3, 5, 16, -1):
        assert lib.bahip_context_set_intrinsics_sum_classes(h, bad) != 0 and b"1, 2, 4 or 8" in lib.bahip_last_error()
    for good in (1, 2, 4, 8):
        capi.check(lib.bahip_context_set_intrinsics_sum_classes(h, good))
    g.set_intrinsics_sum_classes(1)
    g.set_keyframe_sharding(1, 2)
    g.bind_keyframes()
    # no hook: nothing to exchange with
    with pytest.raises(RuntimeError, match="keyframe sharding needs an all-reduce hook or an RCCL communicator"):
        g.optimize_intrinsics(True, True)

    hook = capi.ALLREDUCE_FN(lambda *a: 1)                                      # (a refused call never reaches the exchange)
    capi.check(lib.bahip_context_set_allreduce(h, hook, None))
    # two ranks over one class
    with pytest.raises(RuntimeError, match="keyframe sharding.*bahip_context_set_intrinsics_sum_classes"):
        g.optimize_intrinsics(True, False)
    # eight ranks over four classes
    g.set_sum_classes(8)
    g.set_keyframe_sharding(0, 8)
    g.bind_keyframes()
    g.set_intrinsics_sum_classes(4)
    with pytest.raises(RuntimeError, match="keyframe sharding.*bahip_context_set_intrinsics_sum_classes"):
        g.optimize_intrinsics(False, True)
    # PCG and the lifecycle stay refused with enough classes too
    g.set_intrinsics_sum_classes(8)
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.pcg_iteration(optimize_depth_intrinsics=True, optimize_color_intrinsics=True)
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.update_surfel_normals()
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.delete_surfels_and_update_radii(1)
    capi.check(lib.bahip_context_set_allreduce(h, capi.ALLREDUCE_FN(), None))
    g.set_keyframe_sharding(0, 1)
    g.bind_keyframes()
    g.optimize_intrinsics(True, True)                                              # unsharded again: runs
