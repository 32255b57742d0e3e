"""The context owns its device and page-locked memory through the owning buffers of capi_buffers.h: every growing path is driven on a
small scene, then again on a cloud and a keyframe table large enough that every buffer has to be replaced, and after
bahip_context_destroy the library holds exactly the blocks and bytes it held before (bahip_debug_live_allocations).  A context that
dies must not take anything of another one with it."""
import ctypes as C
import dataclasses
import gc

import numpy as np
import pytest

from badslam_amd import capi, synthetic
from badslam_amd import lowlevel as ll
from tests import common

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, CAPACITY = 64, 48, 8192
CONTROL = (4.0, 0.5, 0.0, 1e6, 4)   # lambda_up, lambda_down, lambda_min, lambda_max, max_trials


@pytest.fixture(scope="module")
def world():
    """Three keyframes; the oracle's cloud of all three and, from it, what the oracle's pose phase gives for perturbed poses of
    the first two keyframes (over a fifth of the cloud) and of all three (over the whole cloud) -- computed once."""
    scene = common.small_scene(num_keyframes=3, width=WIDTH, height=HEIGHT, seed=7)
    rng = np.random.Generator(np.random.PCG64(1))
    perturbed = [synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    full, _ = common.oracle_surfels(common.build_oracle(scene, CAPACITY))
    clouds = {2: np.ascontiguousarray(full[:, ::5]), 3: full}
    assert clouds[3].shape[1] >= 4 * clouds[2].shape[1] >= 4 * 64
    expected = {}
    for K, cloud in clouds.items():
        ba = common.build_oracle(_first(scene, K), CAPACITY, create_from=[])
        n = cloud.shape[1]
        ba.surfel_data[:, :n] = cloud
        ba.surfels.surfels_size = ba.surfels.surfel_count = n
        for k in range(K):
            ba.set_pose(k, perturbed[k])
        ba.update_surfel_activation()
        ba.optimize_geometry_iteration()
        expected[K] = [ba.estimate_frame_pose(k, perturbed[k])[0].to_array() for k in range(K)]
    return scene, perturbed, clouds, expected


def _first(scene, K):
    return dataclasses.replace(scene, poses_gt=scene.poses_gt[:K], depth=scene.depth[:K], rgb=scene.rgb[:K])


def _baseline():
    gc.collect()   # (what earlier tests left to the collector goes now, not in the middle of the count)
    return ll.live_allocations()


def _pose_phase(g, perturbed):
    """smoke()'s pass from the perturbed poses: activation, geometry step, pose phase."""
    for k, kf in enumerate(g.keyframes):
        kf["pose"] = np.asarray(perturbed[k], np.float32)
    g.bind_keyframes()
    g.update_surfel_activation()
    g.optimize_geometry_iteration(True, True)
    return g.estimate_keyframe_poses(True, True)[0]


def _drive(g, cloud, perturbed):
    """Every path of the C boundary that grows a buffer of the context, once.  Returns the poses of the plain pose phase."""
    lib, h, K = g.lib, g.ctx.handle, len(g.keyframes)
    g.upload_surfels(cloud, np.zeros(cloud.shape[1], np.uint8))
    poses = _pose_phase(g, perturbed)                                     # activation, geometry step, pose phase
    g.estimate_keyframe_poses_controlled([1e-3] * K, CONTROL)              # the controlled pose phase
    g.optimize_intrinsics(True, True, apply=False)                         # the intrinsics step with depth
    g.cfactor.clear(0)                                                     # (it writes the depth deformation in place: the scene stays the oracle's)
    g.bind_keyframes()
    g.pcg_iteration()
    g.pcg_iteration(windowed=True)
    g.pcg_iteration_controlled(1e-3, CONTROL)
    g.bind_keyframes()
    g.evaluate_cost()
    # one call of the device-driven loop
    lists = [[j for j in range(K) if j != k] for k in range(K)]
    offsets = np.zeros(K + 1, np.int32)
    offsets[1:] = np.cumsum([len(l) for l in lists])
    indices = np.asarray([j for l in lists for j in l], np.int32)
    window = np.ones(K, np.uint8)
    capi.check(lib.bahip_set_covisibility(h, offsets.ctypes.data_as(C.POINTER(C.c_int)), indices.ctypes.data_as(C.POINTER(C.c_int)), K))
    capi.check(lib.bahip_set_activation_window(h, window.ctypes.data_as(C.POINTER(C.c_uint8)), K))
    opt = capi.AlternatingOptions(1, 1, 1, 1, g.surfels_size, 2, 2)
    s = g.surfels_struct()
    out_poses, activation = (C.c_float * (7 * K))(), (C.c_int * K)()
    handled, done, converged, rounds, steps, stuck = (C.c_int() for _ in range(6))
    capi.check(lib.bahip_alternating_iterations(h, C.byref(opt), C.byref(s), out_poses, activation, C.byref(handled), C.byref(done),
                                                C.byref(converged), C.byref(rounds), C.byref(steps), C.byref(stuck)))
    assert handled.value == 1 and done.value == 2
    # the lifecycle: merge batches by cell lists and pipelined, creation batches as a chain and keyframe by keyframe, a single
    # creation with the outlier filter, deletion, compaction, the spatial sort
    everyone = list(range(K))
    try:
        for cells in (1, 0):
            capi.check(lib.bahip_debug_set_merge_cells(cells))
            with g.lifecycle_batch(keyframes=everyone):
                g.merge_surfels_for_bound_keyframes(everyone)
        for chain in (1, 0):
            capi.check(lib.bahip_debug_set_creation_chain(chain))
            with g.lifecycle_batch(keyframes=everyone):
                g.create_surfels_for_keyframes([(k, None) for k in everyone], filter_new_surfels=True)
    finally:
        capi.check(lib.bahip_debug_set_merge_cells(1))
        capi.check(lib.bahip_debug_set_creation_chain(1))
    g.create_surfels_for_keyframe(0, filter_new_surfels=True)
    g.delete_surfels_and_update_radii(2)
    g.compact_surfels()
    g.sort_surfels_spatially()
    g.ctx.synchronize()
    return poses


def test_a_destroyed_context_gives_back_every_block(world):
    scene, perturbed, clouds, expected = world
    base = _baseline()
    g = common.build_gpu(_first(scene, 2), CAPACITY, create_from=[])
    _drive(g, clouds[2], perturbed)
    small = ll.live_allocations()
    assert small[0] > base[0] and small[1] > base[1]                       # (the count is not vacuous)
    g.add_keyframe(scene.depth[2], scene.rgb[2], scene.poses_gt[2])
    poses = _drive(g, clouds[3], perturbed)                                # every buffer sized by the cloud or the table is replaced
    grown = ll.live_allocations()
    assert grown[1] > small[1]
    for k in range(3):                                                     # ... and what the grown buffers give is still the oracle's
        err = common.pose_error(expected[3][k], poses[k])
        assert np.abs(err).max() < 1e-5, f"keyframe {k}: pose differs from the oracle by {err}"
    g.ctx.close()
    assert ll.live_allocations() == base


def test_the_first_pass_matches_the_oracle_too(world):
    scene, perturbed, clouds, expected = world
    g = common.build_gpu(_first(scene, 2), CAPACITY, create_from=[])
    g.upload_surfels(clouds[2], np.zeros(clouds[2].shape[1], np.uint8))
    poses = _pose_phase(g, perturbed)
    for k in range(2):
        err = common.pose_error(expected[2][k], poses[k])
        assert np.abs(err).max() < 1e-5, f"keyframe {k}: pose differs from the oracle by {err}"
    g.ctx.close()


def test_a_context_destroyed_right_after_creation_gives_back_every_block():
    base = _baseline()
    ctx = ll.Context()
    created = ll.live_allocations()
    assert created[0] > base[0] and created[1] > base[1]
    ctx.close()
    assert ll.live_allocations() == base


def test_destroying_one_context_leaves_the_other_alone(world):
    scene, perturbed, clouds, expected = world
    base = _baseline()
    first = common.build_gpu(scene, CAPACITY, create_from=[])
    second = common.build_gpu(scene, CAPACITY, create_from=[])
    assert first.ctx.handle.value != second.ctx.handle.value
    for g in (first, second):
        _drive(g, clouds[3], perturbed)
        g.upload_surfels(clouds[3], np.zeros(clouds[3].shape[1], np.uint8))
    before = np.asarray(_pose_phase(second, perturbed), np.float32)
    second.upload_surfels(clouds[3], np.zeros(clouds[3].shape[1], np.uint8))   # (the geometry step moved the surfels)
    both = ll.live_allocations()
    first.ctx.close()
    alone = ll.live_allocations()
    assert base[0] < alone[0] < both[0] and base[1] < alone[1] < both[1]
    after = np.asarray(_pose_phase(second, perturbed), np.float32)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    second.ctx.close()
    assert ll.live_allocations() == base
