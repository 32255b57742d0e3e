"""DirectBA::ComputeCost (dba_compute_cost, DirectBA.compute_cost) under either sharding, and the Route-B shim's debug outputs of the
pose accumulation (badslam_amd/host/route_b/test_route_b_cost.cc)."""
import os
import subprocess

import numpy as np
import pytest

from badslam_amd import capi
from tests import common
from tests.test_gpu_cost import _key, _keys
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_b_debug_outputs_are_the_references_definition():
    binary = os.path.join(ROOT, "badslam_amd", "lib", "test_route_b_cost")
    assert os.path.exists(binary), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    proc = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0 and "ROUTE_B_COST_OK" in proc.stdout, (proc.stdout[-2000:], proc.stderr[-2000:])


def _build(scene, start):
    from badslam_amd.directba import DirectBA
    ba = DirectBA(600000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    for k in range(len(scene.depth)):
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], start[k])
    return ba


def _run(ba):
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)
    return _keys(ba.compute_cost())


@pytest.mark.parametrize("sharding", ["surfel", "keyframe"])
def test_directba_compute_cost_on_shards_is_the_unsharded_cost(sharding):
    """Two ranks run the same BundleAdjustment call as the unsharded object (bit for bit: tests/test_gpu_sharded_loopback.py and
    tests/test_gpu_keyframe_sharded_lifecycle.py) and then ComputeCost: every rank returns the unsharded object's bits."""
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    ref = _run(_build(scene, start))
    total, per = ref
    assert total[3] > 10000 and len(per) == len(start)
    assert sum(p[3] for p in per) == total[3] and sum(p[4] for p in per) == total[4]

    def rank_main(rank, hook):
        ba = _build(scene, start)
        ctx = ba.backend_context()
        capi.check(ctx.lib.bahip_context_set_allreduce(ctx.handle, hook, None))
        if sharding == "surfel":
            ba.SetSurfelSharding(rank, 2, 1024)
        else:
            ba.SetKeyframeSharding(rank, 2)
        return dict(cost=_run(ba), keep=(hook, ba))

    results, _ = _run_ranks(2, rank_main)
    for rank, r in enumerate(results):
        assert r["cost"] == ref, rank


def test_directba_compute_cost_is_indexed_by_keyframe_id():
    """Entries by keyframe id; a deleted keyframe's entry is zero and the others keep their values."""
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    total, per = ba.compute_cost()
    assert len(per) == 4 and all(p["depth_residuals"] > 0 for p in per)
    assert ba.L.dba_delete_keyframe(ba.h, 2) == 0
    total2, per2 = ba.compute_cost()
    assert per2[2] == dict(depth=0.0, descriptor_1=0.0, descriptor_2=0.0, depth_residuals=0, descriptor_pairs=0)
    for k in (0, 1, 3):
        assert _key(per2[k]) == _key(per[k]), k
    assert total2["depth_residuals"] == total["depth_residuals"] - per[2]["depth_residuals"]
