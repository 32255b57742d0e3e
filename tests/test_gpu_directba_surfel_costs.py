"""DirectBA::ComputeSurfelCosts (dba_compute_surfel_costs, DirectBA.compute_surfel_costs): the low-level call's bits on the object's
state, the planes of a cloud that creation, merging and compaction have gone over, and either sharding."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi, lowlevel, multigpu
from tests import common
from tests import surfel_costs as sc
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

CHUNK = 1024


def _lowlevel_planes(ba, use_depth=True, use_desc=True):
    """bahip_evaluate_surfel_costs on the object's bound scene and surfel buffer, the planes filled with 0xFF bytes first."""
    ba.BindScene()
    ctx, s = ba.backend_context(), ba.surfels_struct()
    n = int(s.surfels_size)
    names = [(name, np.float64) for name in sc.SUMS] + [(name, np.uint32) for name in sc.COUNTS]
    bufs = {name: lowlevel.DeviceBuffer2D(ctx, 1, max(1, n), dtype).clear(0xFF) for name, dtype in names}
    out = capi.SurfelCosts(*[bufs[name].ptr for name, _ in names])
    capi.check(ctx.lib.bahip_evaluate_surfel_costs(ctx.handle, int(use_depth), int(use_desc), C.byref(s), C.byref(out)))
    planes = {name: b.download()[0, :n].copy() for name, b in bufs.items()}
    for b in bufs.values():
        b.free()
    return planes


def _adjust(ba):
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)


def _scene():
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    return scene, [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]


def test_compute_surfel_costs_is_the_lowlevel_call_on_the_same_state():
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    got = ba.compute_surfel_costs()
    assert all(got[name].shape == (ba.surfels_size(),) for name in sc.PLANES) and ba.surfels_size() > 10000
    sc.assert_same_bits(got, _lowlevel_planes(ba), "after creation")
    total, _ = ba.compute_cost()
    sc.assert_consistent_with_cost(got, total, "after creation")


def test_after_surfel_updates_deleted_slots_are_zero_rows_and_the_planes_sum_to_the_cost():
    scene, start = _scene()
    ba = _build(scene, start)
    _adjust(ba)                                   # creation, merging, deletion, compaction
    got = ba.compute_surfel_costs()
    n = ba.surfels_size()
    assert all(got[name].shape == (n,) for name in sc.PLANES) and n > 10000
    sc.assert_same_bits(got, _lowlevel_planes(ba), "after BundleAdjustment")
    total, _ = ba.compute_cost()
    print("totals", sc.totals(got), total)
    sc.assert_consistent_with_cost(got, total, "after BundleAdjustment")
    # slots the lifecycle left deleted (NaN position) are zero rows; delete some more by hand, where there are terms
    data = ba.download_surfels(8)
    deleted = np.isnan(data[0])
    victims = np.flatnonzero(~deleted & (got["depth_residuals"] > 0))[5:600:7]
    assert victims.size > 50
    data[0, victims] = np.nan
    ba.upload_surfels(data)
    deleted[victims] = True
    again = ba.compute_surfel_costs()
    zeros = {name: np.zeros(int(deleted.sum()), a.dtype) for name, a in again.items()}
    sc.assert_same_bits(sc.take(again, deleted), zeros, "deleted slots")
    sc.assert_same_bits(sc.take(again, ~deleted), sc.take(got, ~deleted), "the other slots")
    total, _ = ba.compute_cost()
    sc.assert_consistent_with_cost(again, total, "after deleting by hand")


@pytest.mark.parametrize("sharding", ["surfel", "keyframe"])
def test_compute_surfel_costs_on_shards_gives_the_unsharded_rows(sharding):
    """Two ranks run the same BundleAdjustment call as the unsharded object (bit for bit: tests/test_gpu_directba_cost.py) and then
    ComputeSurfelCosts: under keyframe sharding every rank returns the unsharded planes, under surfel sharding the rows of its shard."""
    scene, start = _scene()
    ref_ba = _build(scene, start)
    _adjust(ref_ba)
    ref = ref_ba.compute_surfel_costs()
    N = ref_ba.surfels_size()
    assert sc.totals(ref)["depth_residuals"] > 10000

    def rank_main(rank, hook):
        ba = _build(scene, start)
        ctx = ba.backend_context()
        capi.check(ctx.lib.bahip_context_set_allreduce(ctx.handle, hook, None))
        if sharding == "surfel":
            ba.SetSurfelSharding(rank, 2, CHUNK)
        else:
            ba.SetKeyframeSharding(rank, 2)
        _adjust(ba)
        return dict(planes=ba.compute_surfel_costs(), keep=(hook, ba))

    results, _ = _run_ranks(2, rank_main)
    for rank, r in enumerate(results):
        expected = sc.take(ref, multigpu.shard_chunks(N, rank, 2, chunk=CHUNK)) if sharding == "surfel" else ref
        sc.assert_same_bits(r["planes"], expected, (sharding, rank))
