"""The fused route of the geometry step (kernels_surfel.hip: geometry_fused_kernel + geometry_fixup_kernel; launch shape 6 of
bahip_debug_set_launch_shapes): one walk over a tile's candidates with the old normals gives the sums of the normals pass and of the
position pass; a surfel whose packed normal does not change is solved from the walk's sums, a tile with at least T changed surfels runs
its position pass again in the kernel, and fewer changed surfels are left to the fix-up launch (windows of W tiles, 64 surfels at a
time).  Whatever T and W, the step must give the classic step's bits.

Exact flavour: bit for bit against the CPU oracle after each of four successive steps -- tests/test_cpu_geometry_fused_census.py pins
how many normals change in each of them on these clouds, so that all three routes are taken.  Both flavours: against the classic
one- and four-wavefront shapes, per step and over five BundleAdjustment iterations.  The depth-only selection has no fused kernel and
runs the classic one-wavefront kernel under shape 6."""
import ctypes as C
import gc

import numpy as np
import pytest

from badslam_amd import capi
from badslam_amd import lowlevel as ll
from oracle import binding as ob
from tests import common
from tests.test_gpu_geometry_parked_state import (KEYFRAME_COUNTS, LATE_KEYFRAMES, LOOKING_AWAY, MAX_KEYFRAMES, SELECTIONS, SURFEL_COUNTS,
                                                  _bundle_adjustment, _cloud, _first_keyframes)
from tests.test_gpu_geometry_parked_state import ba_inputs   # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

STEPS = 4
FUSED = 6                                     # the launch shape
SETTINGS = ((1, 0), (8, 0), (65, 0), (8, 2), (65, 2))   # (threshold T, window W; 0 = default): W plays no part at T = 1
THRESHOLDS = (1, 8, 65)


def _shapes(tile_waves):
    capi.check(capi.load().bahip_debug_set_launch_shapes(tile_waves, 0))


def _fused(threshold, window):
    capi.check(capi.load().bahip_debug_set_geometry_fused(threshold, window))


def _stats(g):
    """tiles held, tiles run again, tiles with deferred surfels, deferred surfels -- of the last step that took the fused route"""
    out = (C.c_longlong * 4)()
    capi.check(g.lib.bahip_debug_geometry_fused_stats(g.ctx.handle, out))
    return tuple(int(v) for v in out)


def _restore(g=None):
    _shapes(0)
    _fused(0, 0)
    ob.lib().orc_set_sum_classes(4)
    if g is not None:
        g.set_sum_classes(4)
        g.ctx.set_arithmetic("exact")


@pytest.fixture(scope="module")
def scene():
    return common.small_scene(num_keyframes=MAX_KEYFRAMES, width=160, height=120, seed=21, translation_range=0.3, rotation_range=0.15)


@pytest.fixture(scope="module")
def pairs(scene):
    """keyframes -> (oracle, GPU scene, the cloud of keyframe 0): built once per keyframe count, shared by every test"""
    built = {}

    def get(count):
        if count not in built:
            cut = _first_keyframes(scene, count)
            ba = common.build_oracle(cut, 8192, create_from=[0])
            g = common.build_gpu(cut, 8192, create_from=[])
            built[count] = (ba, g, common.oracle_surfels(ba)[0])
        return built[count]
    return get


def _oracle_steps(ba, cloud, use_depth, use_desc, steps=STEPS):
    """[(the eight caller-visible rows, the flags the step's activation decided)] after each of `steps` successive steps"""
    n = cloud.shape[1]
    ba.use_depth, ba.use_desc = int(use_depth), int(use_desc)
    ba.surfel_data[:, :n] = cloud
    ba.active[:n] = 0
    ba.surfels.surfels_size = ba.surfels.surfel_count = n
    out = []
    for _ in range(steps):
        ba.update_surfel_activation()
        flags = ba.active[:n].copy()
        ba.optimize_geometry_iteration()
        out.append((ba.surfel_data[:8, :n].copy(), flags))
    return out


def _gpu_steps(g, cloud, use_depth, use_desc, in_sweep, given=None, steps=STEPS, after_step=None):
    """The same on the GPU.  in_sweep: the flags are decided inside the sweep (from all-zero flags); else given[step] are uploaded in
    front of each step, with the rows the previous step left."""
    n = cloud.shape[1]
    out = []
    rows = cloud
    if in_sweep:
        g.upload_surfels(cloud, np.zeros(n, np.uint8))
    for step in range(steps):
        if in_sweep:
            g.update_activation_and_optimize_geometry(use_depth, use_desc)
        else:
            g.upload_surfels(rows, given[step])
            g.optimize_geometry_iteration(use_depth, use_desc)
        rows = g.download_surfels().copy()
        out.append((rows[:8].copy(), g.active_buf.download()[0, :n].copy()))
        if after_step:
            after_step(step)
    return out


def _assert_same(got, ref, case):
    for step, ((rows, flags), (ref_rows, ref_flags)) in enumerate(zip(got, ref)):
        assert np.array_equal(flags, ref_flags), (case, step)
        assert np.array_equal(rows.view(np.uint32), ref_rows.view(np.uint32)), (case, step)


@pytest.mark.parametrize("classes", [4, 8])
@pytest.mark.parametrize("keyframes", KEYFRAME_COUNTS)
def test_exact_flavour_gives_the_oracles_four_steps(pairs, keyframes, classes, request):
    ba, g, data = pairs(keyframes)
    request.addfinalizer(lambda: _restore(g))
    g.ctx.set_arithmetic("exact")
    g.set_sum_classes(classes)
    ob.lib().orc_set_sum_classes(classes)
    _shapes(FUSED)
    g.bind_keyframes()
    moved = 0
    for count in SURFEL_COUNTS:
        cloud, deleted = _cloud(data, count)
        for use_depth, use_desc in SELECTIONS:
            ref = _oracle_steps(ba, cloud, use_depth, use_desc)
            assert not any(flags[deleted].any() for _, flags in ref)
            for threshold, window in (SETTINGS if use_desc else SETTINGS[:1]):     # (depth only: the classic kernel, once)
                _fused(threshold, window)
                for in_sweep in (True, False):
                    got = _gpu_steps(g, cloud, use_depth, use_desc, in_sweep, [flags for _, flags in ref])
                    _assert_same(got, ref, (count, use_depth, use_desc, threshold, window, in_sweep))
            moved += int(np.count_nonzero(ref[-1][0][2] != cloud[2]))
    assert moved > 0


@pytest.mark.parametrize("keyframes", [5, 257])
def test_exact_flavour_gives_the_oracles_four_steps_on_the_whole_cloud(pairs, keyframes, request):
    """4524 surfels: 71 tiles, a second, partial fix-up window at the default of 64 tiles"""
    ba, g, data = pairs(keyframes)
    request.addfinalizer(lambda: _restore(g))
    g.ctx.set_arithmetic("exact")
    _shapes(FUSED)
    g.bind_keyframes()
    assert data.shape[1] > 64 * 64
    ref = _oracle_steps(ba, data, True, True)
    deferred = 0

    def count(step):
        nonlocal deferred
        deferred += _stats(g)[3]
    for threshold, window in SETTINGS:
        _fused(threshold, window)
        got = _gpu_steps(g, data, True, True, True, after_step=count)
        _assert_same(got, ref, (threshold, window))
    assert deferred > 64


LATE_COUNTS = (65, 193)


@pytest.fixture(scope="module")
def late_pair():
    """(oracle, GPU scene, the cloud of keyframe 0) with 1040 keyframes of 64 x 48 pixels: from keyframe 1024 on the position pass run
    again tests the chunks itself instead of replaying the walk's masks, and the fix-up tests every chunk"""
    from badslam_amd import se3
    scene = common.small_scene(num_keyframes=LATE_KEYFRAMES, width=64, height=48, seed=22, translation_range=0.3, rotation_range=0.15)
    away = se3.exp([0, 0, 0, 0, np.pi, 0])
    for k in LOOKING_AWAY:
        scene.poses_gt[k] = se3.mul(scene.poses_gt[k], away)
    ba = common.build_oracle(scene, 8192, create_from=[0])
    g = common.build_gpu(scene, 8192, create_from=[])
    return ba, g, common.oracle_surfels(ba)[0]


def test_keyframes_beyond_the_replayed_masks_exact_flavour_gives_the_oracles_four_steps(late_pair, request):
    ba, g, data = late_pair
    request.addfinalizer(lambda: _restore(g))
    g.ctx.set_arithmetic("exact")
    _shapes(FUSED)
    g.bind_keyframes()
    routes = np.zeros(4, np.int64)

    def count(step):
        routes[:] += _stats(g)
    for n in LATE_COUNTS:
        cloud, deleted = _cloud(data, n)
        for use_depth, use_desc in SELECTIONS:
            ref = _oracle_steps(ba, cloud, use_depth, use_desc)
            assert ref[0][1].any()
            for threshold in (THRESHOLDS if use_desc else THRESHOLDS[:1]):
                _fused(threshold, 0)
                got = _gpu_steps(g, cloud, use_depth, use_desc, True, after_step=count if use_desc else None)
                _assert_same(got, ref, (n, use_depth, use_desc, threshold))
    assert routes[1] > 0 and routes[3] > 0, routes      # tiles ran again and surfels were deferred on this scene too


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
@pytest.mark.parametrize("keyframes", KEYFRAME_COUNTS)
def test_fused_route_gives_the_classic_shapes_bits_per_step(pairs, keyframes, arithmetic, request):
    """Both flavours against the classic one- and four-wavefront shapes (in the fast flavour there is no oracle)."""
    ba, g, data = pairs(keyframes)
    request.addfinalizer(lambda: _restore(g))
    g.ctx.set_arithmetic(arithmetic)
    g.bind_keyframes()
    for classes in (4, 8):
        g.set_sum_classes(classes)
        for count in (65, 193):
            cloud, deleted = _cloud(data, count)
            for use_depth, use_desc in SELECTIONS:
                _shapes(4)
                ref = _gpu_steps(g, cloud, use_depth, use_desc, True)
                given = [flags for _, flags in ref]
                _shapes(1)
                _assert_same(_gpu_steps(g, cloud, use_depth, use_desc, True), ref, (classes, count, use_depth, use_desc, "shape 1"))
                _shapes(FUSED)
                for threshold in (THRESHOLDS if use_desc else THRESHOLDS[:1]):
                    _fused(threshold, 0)
                    for in_sweep in (True, False):
                        got = _gpu_steps(g, cloud, use_depth, use_desc, in_sweep, given)
                        _assert_same(got, ref, (classes, count, use_depth, use_desc, threshold, in_sweep))


@pytest.mark.parametrize("cloud", ["whole cloud", "193 surfels with a deleted tile"])
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_five_bundle_adjustment_iterations_end_with_the_classic_shapes_bits(ba_inputs, fast, cloud, request):   # noqa: F811
    scene, perturbed, surfels = ba_inputs
    if cloud != "whole cloud":
        surfels = surfels[:, ::max(1, surfels.shape[1] // 193)][:, :193].copy()
        surfels[0, 64:128] = np.nan
        surfels[0, [5, 17, 40, 62]] = np.nan
    request.addfinalizer(_restore)
    runs = {}
    for shape in (4, 1):
        _shapes(shape)
        runs[shape] = _bundle_adjustment(scene, perturbed, surfels, fast)
    _shapes(FUSED)
    for threshold in THRESHOLDS:
        _fused(threshold, 0)
        runs[threshold + 100] = _bundle_adjustment(scene, perturbed, surfels, fast)
    assert runs[4][0] == 5
    for key, (done, poses, rows) in runs.items():
        assert done == 5, key
        assert np.array_equal(poses.view(np.uint32), runs[4][1].view(np.uint32)), key
        assert np.array_equal(rows.view(np.uint32), runs[4][2].view(np.uint32)), key


def test_the_three_routes_are_taken_and_counted(pairs, request):
    """The census of tests/test_cpu_geometry_fused_census.py, seen through bahip_debug_geometry_fused_stats: on the 193-surfel cloud
    with 5 keyframes 25 / 0 / 63 / 1 normals change per tile in step 1, 1 / 0 / 2 / 0 in step 2, none in steps 3 and 4; with 257
    keyframes 60 / 0 / 64 / 1, then 5 / 0 / 4 / 0."""
    ba, g, data = pairs(5)
    request.addfinalizer(lambda: _restore(g))
    g.ctx.set_arithmetic("exact")
    g.bind_keyframes()
    cloud, _ = _cloud(data, 193)
    seen = []
    _shapes(FUSED)
    _fused(8, 0)
    _gpu_steps(g, cloud, True, True, True, after_step=lambda step: seen.append(_stats(g)))
    assert seen == [(1, 2, 1, 1), (2, 0, 2, 3), (4, 0, 0, 0), (4, 0, 0, 0)]
    seen.clear()
    _fused(1, 0)         # every changed tile runs again in the kernel: nothing is deferred
    _gpu_steps(g, cloud, True, True, True, after_step=lambda step: seen.append(_stats(g)))
    assert seen == [(1, 3, 0, 0), (2, 2, 0, 0), (4, 0, 0, 0), (4, 0, 0, 0)]
    # the classic shapes, and the heuristic on a cloud this small, leave the route alone: the numbers stay those of the last fused step
    last = (1, 3, 0, 0)
    _gpu_steps(g, cloud, True, True, True, steps=1)
    assert _stats(g) == last
    for shape in (1, 4, 0):
        _shapes(shape)
        _gpu_steps(g, cloud, True, True, True, steps=2)
        assert _stats(g) == last, shape
    # the depth-only step has no fused kernel
    _shapes(FUSED)
    _gpu_steps(g, cloud, True, False, True, steps=2)
    assert _stats(g) == last
    # everything deferred: 125 surfels of one window, i.e. two groups of 64 in the fix-up
    ba, g257, data = pairs(257)
    g257.ctx.set_arithmetic("exact")
    g257.bind_keyframes()
    _fused(65, 0)
    seen.clear()
    _gpu_steps(g257, cloud, True, True, True, after_step=lambda step: seen.append(_stats(g257)))
    assert seen == [(1, 0, 3, 125), (2, 0, 2, 9), (4, 0, 0, 0), (4, 0, 0, 0)]


def test_no_allocation_remains_after_the_calls(scene):
    gc.collect()
    base = ll.live_allocations()
    g = common.build_gpu(_first_keyframes(scene, 5), 8192, create_from=[0])
    data = g.download_surfels().copy()
    held = ll.live_allocations()
    try:
        _shapes(FUSED)
        g.update_activation_and_optimize_geometry(True, True)
        g.ctx.synchronize()
        with_route = ll.live_allocations()
        assert with_route[0] > held[0]                       # the deferred words and the route bytes, for the cloud's capacity
        for _ in range(3):
            g.update_activation_and_optimize_geometry(True, True)
        g.upload_surfels(data[:, :193], np.zeros(193, np.uint8))
        g.optimize_geometry_iteration(True, True)
        assert _stats(g)[0] + _stats(g)[1] + _stats(g)[2] == 4
        assert ll.live_allocations() == with_route           # nothing is allocated from step to step
    finally:
        _restore(g)
    g.ctx.close()
    assert ll.live_allocations() == base


def test_without_forcing_a_large_cloud_takes_the_route_from_the_sixth_iteration_of_a_call():
    """ba_launch.h: kGeometryFusedAfter.  A bench-like scene of 9 400 tiles (the one-wavefront shape's size): a call of five iterations
    never takes the route, a call of eight takes it in iterations 6-8 -- and ends with the classic kernel's bits."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    argv, sys.argv = sys.argv, ["bench.py", "--keyframes", "24", "--surfels", "600000"]
    try:
        args = bench.parse_args()
    finally:
        sys.argv = argv
    ba, data, _ = bench.build_scene(args, lambda m: None)
    tiles = (data.shape[1] + 63) // 64
    assert tiles >= 8192
    ctx = ba.backend_context()
    poses = [ba.keyframe_pose(k) for k in range(args.keyframes)]

    def run(iterations):
        ba.upload_surfels(data)
        for k, T in enumerate(poses):
            ba.set_keyframe_pose(k, T)
        ba.set_ba_iteration_counts(1, 1)
        done, _ = ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, min_iterations=iterations,
                                      max_iterations=iterations, active_keyframe_window_start=0,
                                      active_keyframe_window_end=args.keyframes - 1, increase_ba_iteration_count=False)
        assert done == iterations
        out = (C.c_longlong * 4)()
        capi.check(ctx.lib.bahip_debug_geometry_fused_stats(ctx.handle, out))
        return ba.download_surfels(rows=8), np.asarray([ba.keyframe_pose(k) for k in range(args.keyframes)], np.float32), tuple(out)

    try:
        _, _, stats = run(5)
        assert stats == (0, 0, 0, 0)
        rows, end_poses, stats = run(8)
        assert sum(stats[:3]) == tiles and stats[0] > 0
        _shapes(1)
        ref_rows, ref_poses, unchanged = run(8)
        assert unchanged == stats
        assert np.array_equal(rows.view(np.uint32), ref_rows.view(np.uint32))
        assert np.array_equal(end_poses.view(np.uint32), ref_poses.view(np.uint32))
    finally:
        _restore()
