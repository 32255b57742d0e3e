"""The surfel lifecycle dealt over the ranks of a SURFEL partition (bahip_context_set_lifecycle_dealing, DirectBA::SetDistributedLifecycle).

Inside a whole-cloud phase of surfel sharding every rank holds the gathered cloud and every keyframe's images.  With the mode on, the
creation batch's and the merge batch's per-keyframe sweeps run on the keyframe's owner (bound index % world), deletion + radius update
on each rank's own surfel chunks, and what they computed is exchanged as integer sums; the creation chain, the merge decisions and
compaction run on every rank.  Every rank must end with the bits of the replicated run.  Ranks are threads on one GPU with the
in-process loopback all-reduce of tests/test_gpu_sharded_loopback.py."""
import ctypes as C
import threading

import numpy as np
import pytest

from badslam_amd import capi, multigpu
from tests import common
from tests.test_gpu_keyframe_sharded_lifecycle import CREATE, KEYFRAMES, MERGE, _scene
from tests.test_gpu_sharded_loopback import _Loopback

pytestmark = pytest.mark.gpu

CHUNK = 128                      # small chunks: the deletion's partition has a boundary every 128 surfels
CAPACITY = 900000


def _run_ranks(world, rank_main, timeout=900):
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


def _build(scene, poses):
    return common.build_gpu(scene, CAPACITY, poses=poses, create_from=[0, 1, 2])


def _enter_whole_cloud(g, rank, world):
    """What DirectBA's whole-cloud phase does: this rank's shard of the cloud out into a buffer of its own, then
    bahip_gather_surfel_shards back into g's buffers (the phase the dealt lifecycle goes by)."""
    from badslam_amd.lowlevel import DeviceBuffer2D
    rows = DeviceBuffer2D(g.ctx, capi.SURFEL_ATTRIBUTE_COUNT, CAPACITY, np.float32).clear(0)
    active = DeviceBuffer2D(g.ctx, 1, CAPACITY, np.uint8).clear(0)
    shard = capi.Surfels(rows.ptr, rows.pitch, active.ptr, 0, CAPACITY)
    cloud = g.surfels_struct()
    mine = C.c_uint32()
    capi.check(g.lib.bahip_extract_surfel_shard(g.ctx.handle, C.byref(cloud), rank, world, CHUNK, C.byref(shard), C.byref(mine)))
    shard.size = mine.value
    size, count = C.c_uint32(), C.c_uint32()
    capi.check(g.lib.bahip_gather_surfel_shards(g.ctx.handle, C.byref(shard), mine.value, rank, world, CHUNK, C.byref(cloud), C.byref(size),
                                                C.byref(count)))
    g.ctx.synchronize()
    assert size.value == g.surfels_size and count.value == g.surfels_size
    return rows, active, mine.value


def _exchanges(g):
    calls, nbytes = C.c_longlong(), C.c_longlong()
    capi.check(g.lib.bahip_exchange_stats(g.ctx.handle, C.byref(calls), C.byref(nbytes), 1))
    return calls.value, nbytes.value


def _state(g, planes=False):
    g.ctx.synchronize()
    out = dict(size=g.surfels_size, rows=g.surfel_buf.download()[:8, :g.surfels_size].copy().view(np.uint32))
    if planes:
        out["planes"] = np.stack([b.download()[:g.cf_h, :g.cf_w] for b in g.supporting])
    return out


def _stages(g, min_obs, create=CREATE):
    """A filtered creation batch, a batch of one keyframe, a merge batch by index, deletion + radii; exchanges per stage."""
    out = {}
    _exchanges(g)
    with g.lifecycle_batch(keyframes=create):
        out["new"] = g.create_surfels_for_keyframes([(k, None) for k in create], filter_new_surfels=True, min_observation_count=min_obs)
    out["after_create"] = _state(g, planes=True)
    out["x_create"] = _exchanges(g)
    with g.lifecycle_batch(keyframes=[1]):
        out["new_one"] = g.create_surfels_for_keyframes([(1, [0, 2, 5, 6, 9])], filter_new_surfels=True, min_observation_count=min_obs)
    out["after_create_one"] = _state(g, planes=True)
    out["x_create_one"] = _exchanges(g)
    with g.lifecycle_batch(keyframes=MERGE):
        _, out["merged"] = g.merge_surfels_for_bound_keyframes(MERGE, merge_dist_factor=0.8)
    out["after_merge"] = _state(g, planes=True)
    out["x_merge"] = _exchanges(g)
    out["deleted"] = g.delete_surfels_and_update_radii(min_obs)
    out["after_delete"] = _state(g)
    out["x_delete"] = _exchanges(g)
    return out


def _compare(got, ref, where):
    for key, value in ref.items():
        if key.startswith("x_"):
            continue
        if isinstance(value, dict):
            for part in value:
                assert np.array_equal(np.asarray(got[key][part]), np.asarray(value[part])), (where, key, part)
        else:
            assert got[key] == value, (where, key, got[key], value)


def _align(v):
    return (v + 255) & ~255


# ---- each stage against its replicated counterpart, on the gathered cloud ------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4, 8])
def test_dealt_lifecycle_stages_are_the_replicated_stages(world):
    """Every rank ends every stage with the replicated run's rows 0-7, sizes, counts and supporting planes; each rank swept only its
    owned keyframes in the creation / merge up-front kernels and only its own chunks in deletion; the exchanges are the header's."""
    import torch
    torch.cuda.set_device(0)
    scene, poses = _scene()
    min_obs = 2
    ref = _stages(_build(scene, poses), min_obs)
    assert ref["new"] > 100 and ref["merged"] > 0 and ref["deleted"] > 0
    assert all(ref[k] == (0, 0) for k in ("x_create", "x_create_one", "x_merge", "x_delete"))    # one context: no exchange

    def rank_main(rank, hook):
        g = _build(scene, poses)
        capi.check(g.lib.bahip_context_set_allreduce(g.ctx.handle, hook, None))
        g.set_lifecycle_dealing(True)
        keep = _enter_whole_cloud(g, rank, world)
        size_at_begin = g.surfels_size
        g.lifecycle_deal_stats(reset=True)
        out = _stages(g, min_obs)
        out["stats"] = g.lifecycle_deal_stats()
        out["size_at_begin"] = size_at_begin
        out["keep"] = keep
        return out

    results, _ = _run_ranks(world, rank_main)
    cells = ((scene.width - 1) // scene.cell + 1) * ((scene.height - 1) // scene.cell + 1)
    tile = 8 * scene.cell                                                    # the creation's padded pixel sequence (tile-major)
    px = -(-scene.width // tile) * -(-scene.height // tile) * tile * tile
    for rank, r in enumerate(results):
        _compare(r, ref, f"rank {rank}")
        owned_create = [k for k in CREATE[:-1] if k % world == rank]          # the chain's keyframes: all but the last
        owned_merge = [k for k in MERGE if k % world == rank]
        s = r["stats"]
        assert s[0] == len(owned_create) and s[1] == sum(k + 1 for k in owned_create), (rank, s)
        assert s[2] == len(owned_merge) and s[3] == sum(k + 1 for k in owned_merge), (rank, s)
        n_delete = ref["after_merge"]["size"]
        assert s[4] == multigpu.shard_chunks(n_delete, rank, world, chunk=CHUNK).size, (rank, s)
        assert s[5] == 3                                                        # creation batch, merge batch, deletion
        # the header's table: creation = candidates + filter counts + records, a batch of one keyframe none, merge two, deletion one
        # (s[6]: the candidates whose records went out, s[7]: the associated pairs whose cell members went out)
        n = len(CREATE) - 1
        candidates, pairs = s[6], s[7]
        assert candidates > 0 and pairs > 0, s
        records = 36 * ((candidates + 63) // 64 * 64)                         # the list's cell + 8 record rows, whole 64-column blocks
        assert r["x_create"] == (3, _align(n * cells) + _align(n * px) + _align(4 * n * cells) + _align(8 * n * cells) + records), (r["x_create"], s)
        assert r["x_create_one"] == (0, 0)
        even = lambda v: (v + 1) & ~1                                          # noqa: E731  (int64 words: an even number of 32-bit words)
        assert r["x_merge"] == (2, 4 * even(len(MERGE) * cells) + 12 * even(pairs)), (r["x_merge"], s)
        assert r["x_delete"] == (1, 8 * (n_delete + 1))
    assert sum(r["stats"][0] for r in results) == len(CREATE) - 1
    assert sum(r["stats"][2] for r in results) == len(MERGE)
    assert sum(r["stats"][4] for r in results) == ref["after_merge"]["size"]
    assert len({tuple(r["stats"][6:]) for r in results}) == 1                 # (the exchanged lists are the same on every rank)


def test_dealt_creation_batch_in_another_order_and_with_the_mode_off():
    """Reordered keyframe indices at world 2 (each rank's owned keyframes interleaved differently), against the replicated run; the
    same ranks with the mode off exchange nothing inside the phase, as before the mode existed."""
    import torch
    torch.cuda.set_device(0)
    scene, poses = _scene()
    order = [9, 4, 3, 8, 5, 6]
    ref = _stages(_build(scene, poses), 3, create=order)

    def rank_main(rank, hook, dealing):
        g = _build(scene, poses)
        capi.check(g.lib.bahip_context_set_allreduce(g.ctx.handle, hook, None))
        g.set_lifecycle_dealing(dealing)
        keep = _enter_whole_cloud(g, rank, 2)
        g.lifecycle_deal_stats(reset=True)
        out = _stages(g, 3, create=order)
        out["stats"], out["keep"] = g.lifecycle_deal_stats(), keep
        # the phase belongs to the gathered cloud: deletion on another buffer (this rank's shard) is not dealt and exchanges nothing
        rows, active, mine = keep
        shard = capi.Surfels(rows.ptr, rows.pitch, active.ptr, mine, CAPACITY)
        deleted = C.c_uint32()
        capi.check(g.lib.bahip_delete_surfels_and_update_radii(g.ctx.handle, 3, C.byref(shard), C.byref(deleted)))
        g.ctx.synchronize()
        out["other_buffer"] = (g.lifecycle_deal_stats(), _exchanges(g))
        return out

    on, _ = _run_ranks(2, lambda rank, hook: rank_main(rank, hook, True))
    off, _ = _run_ranks(2, lambda rank, hook: rank_main(rank, hook, False))
    for rank in range(2):
        _compare(on[rank], ref, f"on, rank {rank}")
        _compare(off[rank], ref, f"off, rank {rank}")
        assert on[rank]["stats"][0] == sum(1 for k in order[:-1] if k % 2 == rank)
        assert off[rank]["stats"] == [0] * 8
        assert on[rank]["other_buffer"] == ([0] * 8, (0, 0)) and off[rank]["other_buffer"] == ([0] * 8, (0, 0))
        assert all(off[rank][k] == (0, 0) for k in ("x_create", "x_create_one", "x_merge", "x_delete"))


# ---- refusals, world 1 ----------------------------------------------------------------------------------------------------------------
def test_dealing_is_refused_under_keyframe_sharding_and_a_no_op_at_world_one():
    import torch
    torch.cuda.set_device(0)
    scene, poses = _scene()
    g = _build(scene, poses)
    capi.check(g.lib.bahip_context_set_keyframe_sharding(g.ctx.handle, 0, 2))
    with pytest.raises(capi.BackendError, match="refused under keyframe sharding"):
        g.set_lifecycle_dealing(True)
    capi.check(g.lib.bahip_context_set_keyframe_sharding(g.ctx.handle, 0, 1))
    g.set_lifecycle_dealing(True)                                          # (the context is still usable)
    with pytest.raises(capi.BackendError, match="deals its own lifecycle"):
        capi.check(g.lib.bahip_context_set_keyframe_sharding(g.ctx.handle, 0, 2))

    ref = _stages(_build(scene, poses), 2)
    one = _build(scene, poses)
    one.set_lifecycle_dealing(True)
    _enter_whole_cloud(one, 0, 1)
    one.lifecycle_deal_stats(reset=True)
    got = _stages(one, 2)
    _compare(got, ref, "world 1")
    assert one.lifecycle_deal_stats() == [0] * 8


def test_directba_refuses_the_distributed_lifecycle_under_keyframe_sharding():
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=2, seed=5)
    ba = DirectBA(100000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    ba.SetDistributedLifecycle(True)
    ba.SetDistributedLifecycle(False)
    ba.SetKeyframeSharding(0, 2)
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        ba.SetDistributedLifecycle(True)


# ---- the drop-in call, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,use_pcg,fast", [(2, False, False), (4, False, False), (8, False, False), (2, True, False), (4, True, False),
                                                (8, True, False), (4, False, True)])
def test_distributed_lifecycle_bundle_adjustment_is_the_unsharded_run(world, use_pcg, fast):
    """Two DirectBA::BundleAdjustment(do_surfel_updates) calls of two iterations each from no surfels on `world` surfel shards with
    SetDistributedLifecycle(True): the union of the shards is the unsharded cloud (rows 0-7), the shard sizes the chunk-cyclic
    partition, the poses equal, bit for bit; every rank dealt (creation / merge keyframes and deletion surfels).  The fast case also
    optimises the intrinsics in the fast arithmetic flavour."""
    import torch
    from badslam_amd.directba import DirectBA
    torch.cuda.set_device(0)
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    chunk = 1024

    def build():
        ba = DirectBA(600000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
        for k in range(len(scene.depth)):
            ba.AddKeyframe(scene.depth[k], scene.rgb[k], start[k])
        ba.set_pcg_gauge_keyframe(0)
        if fast:
            ba.SetFastArithmetic(True)
        return ba

    def run(ba):
        sizes = []
        for _ in range(2):
            ba.BundleAdjustment(optimize_depth_intrinsics=fast, optimize_color_intrinsics=fast, do_surfel_updates=True, optimize_poses=True,
                                optimize_geometry=True, min_iterations=2, max_iterations=2, use_pcg=use_pcg, increase_ba_iteration_count=True)
            sizes.append(ba.surfels_size())
        return dict(sizes=sizes, surfels=ba.download_surfels(8), poses=[ba.keyframe_pose(k) for k in range(len(start))])

    ref = run(build())
    N = ref["surfels"].shape[1]
    assert N > 10000 and ref["sizes"][1] != ref["sizes"][0]

    def rank_main(rank, hook):
        ba = build()
        ctx = ba.backend_context()
        capi.check(ctx.lib.bahip_context_set_allreduce(ctx.handle, hook, None))
        ba.SetSurfelSharding(rank, world, chunk)
        ba.SetDistributedLifecycle(True)
        out = run(ba)
        stats = (C.c_longlong * 8)()
        capi.check(ctx.lib.bahip_debug_lifecycle_deal_stats(ctx.handle, stats, 0))
        out["stats"], out["keep"] = list(stats), (hook, ba)
        return out

    results, _ = _run_ranks(world, rank_main)
    for call in range(2):
        assert sum(r["sizes"][call] for r in results) == ref["sizes"][call]
    merged = np.zeros_like(ref["surfels"])
    for rank, r in enumerate(results):
        mine = multigpu.shard_chunks(N, rank, world, chunk=chunk)
        assert r["surfels"].shape[1] == mine.size
        merged[:, mine] = r["surfels"]
    assert np.array_equal(merged.view(np.uint32), ref["surfels"].view(np.uint32))
    for k in range(len(start)):
        for r in results:
            assert np.array_equal(r["poses"][k], ref["poses"][k]), k
    # creation dealt the chain's keyframes, merging and deletion took the dealt path on every rank
    assert sum(r["stats"][0] for r in results) >= len(start) - 1
    assert all(r["stats"][4] > 0 and r["stats"][5] >= 3 for r in results), [r["stats"] for r in results]
    assert sum(r["stats"][2] for r in results) > 0
