"""The one-wavefront geometry kernel keeps its cold per-lane state in LDS (kernels_surfel.hip: ParkSlot; DESIGN.md section 3, "five
wavefronts per SIMD"): what a lane parks must come back as the word it stored, at the shapes where a parked block can go wrong --
a partial last tile, a tile made entirely of deleted (NaN) surfels, which returns before anything is parked, deleted lanes among
live ones, one keyframe, a second 64-keyframe chunk per class, both numbers of sum classes, and 1040 keyframes: from keyframe 1024 on
(four sum classes) the position pass no longer replays the normals pass's candidate masks but tests the chunk itself, on the parked
bounding sphere.

Exact flavour: bit for bit against the CPU oracle's geometry step, through the harness of tests/test_gpu_kernels_vs_oracle.py.
Both flavours: the one-wavefront shape against the four-wavefront shape, which parks nothing and whose code is the parent's --
per geometry step on the same small clouds, and over five BundleAdjustment iterations (poses and surfel rows as uint32, as
tests/test_gpu_device_loop.py::test_the_hybrid_shape_of_the_geometry_step_is_the_other_shapes)."""
import copy

import numpy as np
import pytest

from badslam_amd import capi, synthetic
from oracle import binding as ob
from tests import common

pytestmark = pytest.mark.gpu

SURFEL_COUNTS = (1, 63, 64, 65, 193)
KEYFRAME_COUNTS = (1, 5, 257)          # 257: class 0 of four holds 65 keyframes, a second chunk of 64
SELECTIONS = ((True, False), (True, True), (False, True))   # (use_depth, use_desc)
MAX_KEYFRAMES = max(KEYFRAME_COUNTS)


@pytest.fixture(scope="module")
def scene():
    # small images: 257 keyframes are preprocessed twice (oracle and GPU); the poses stay close, so that most keyframes see the cloud
    return common.small_scene(num_keyframes=MAX_KEYFRAMES, width=160, height=120, seed=21, translation_range=0.3, rotation_range=0.15)


def _first_keyframes(scene, count):
    cut = copy.copy(scene)
    cut.depth, cut.rgb, cut.poses_gt = scene.depth[:count], scene.rgb[:count], scene.poses_gt[:count]
    return cut


@pytest.fixture(scope="module")
def pairs(scene):
    """keyframes -> (oracle, GPU scene, the cloud of keyframe 0): built once per keyframe count, shared by every test"""
    built = {}

    def get(count):
        if count not in built:
            cut = _first_keyframes(scene, count)
            ba = common.build_oracle(cut, 8192, create_from=[0])
            g = common.build_gpu(cut, 8192, create_from=[])
            data, _ = common.oracle_surfels(ba)
            assert data.shape[1] >= max(SURFEL_COUNTS)
            built[count] = (ba, g, data)
        return built[count]
    return get


def _cloud(data, count):
    """The first `count` surfels, moved off the surface and detuned; tile 1 (64..127) deleted as a whole where it exists, and a few
    lanes of tile 0 deleted among live ones."""
    rng = np.random.Generator(np.random.PCG64(100 + count))
    cloud = data[:, :count].copy()
    cloud[2] += rng.uniform(0, 0.004, count).astype(np.float32)
    cloud[6] += 3.0
    deleted = np.zeros(count, bool)
    deleted[64:128] = True
    if count >= 63:
        deleted[[5, 17, 40, 62]] = True
    cloud[0, deleted] = np.nan
    return cloud, deleted


def _oracle_step(ba, cloud, use_depth, use_desc):
    n = cloud.shape[1]
    ba.use_depth, ba.use_desc = int(use_depth), int(use_desc)
    ba.surfel_data[:, :n] = cloud
    ba.active[:n] = 0
    ba.surfels.surfels_size = ba.surfels.surfel_count = n
    ba.update_surfel_activation()
    flags = ba.active[:n].copy()
    ba.optimize_geometry_iteration()
    return ba.surfel_data[:8, :n].copy(), flags


def _gpu_step(g, cloud, use_depth, use_desc, in_sweep, flags):
    """One geometry step; in_sweep: the activation flags are decided inside the sweep (from all-zero flags), else given."""
    n = cloud.shape[1]
    if in_sweep:
        g.upload_surfels(cloud, np.zeros(n, np.uint8))
        g.update_activation_and_optimize_geometry(use_depth, use_desc)
    else:
        g.upload_surfels(cloud, flags)
        g.optimize_geometry_iteration(use_depth, use_desc)
    return g.download_surfels()[:8].copy(), g.active_buf.download()[0, :n].copy()


def _shapes(g, tile_waves):
    capi.check(g.ctx.lib.bahip_debug_set_launch_shapes(tile_waves, 0))


@pytest.mark.parametrize("classes", [4, 8])
@pytest.mark.parametrize("keyframes", KEYFRAME_COUNTS)
def test_exact_flavour_gives_the_oracles_geometry_step(pairs, keyframes, classes, request):
    ba, g, data = pairs(keyframes)
    g.ctx.set_arithmetic("exact")
    g.set_sum_classes(classes)
    ob.lib().orc_set_sum_classes(classes)
    _shapes(g, 1)

    def restore():
        _shapes(g, 0)
        g.set_sum_classes(4)
        ob.lib().orc_set_sum_classes(4)
    request.addfinalizer(restore)
    g.bind_keyframes()
    moved = 0
    for count in SURFEL_COUNTS:
        cloud, deleted = _cloud(data, count)
        for use_depth, use_desc in SELECTIONS:
            ref, ref_flags = _oracle_step(ba, cloud, use_depth, use_desc)
            assert not ref_flags[deleted].any()
            for in_sweep in (True, False):
                got, flags = _gpu_step(g, cloud, use_depth, use_desc, in_sweep, ref_flags)
                case = (count, use_depth, use_desc, in_sweep)
                assert np.array_equal(flags, ref_flags), case
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), case
            live = ref_flags.astype(bool)
            moved += int(np.count_nonzero(ref[2, live] != cloud[2, live]))
            # a deleted surfel is left as it is: NaN x, every other word untouched
            assert np.array_equal(ref[1:, deleted].view(np.uint32), cloud[1:8, deleted].view(np.uint32))
    assert moved > 0     # the steps did something


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
@pytest.mark.parametrize("keyframes", KEYFRAME_COUNTS)
def test_one_wavefront_shape_gives_the_four_wavefront_shapes_bits(pairs, keyframes, arithmetic, request):
    """The reference here is the four-wavefront shape: code this kernel's parked state does not reach (in the fast flavour there is
    no oracle to hold it to)."""
    ba, g, data = pairs(keyframes)
    g.ctx.set_arithmetic(arithmetic)

    def restore():
        _shapes(g, 0)
        g.set_sum_classes(4)
        g.ctx.set_arithmetic("exact")
    request.addfinalizer(restore)
    g.bind_keyframes()
    for classes in (4, 8):
        g.set_sum_classes(classes)
        for count in SURFEL_COUNTS:
            cloud, deleted = _cloud(data, count)
            for use_depth, use_desc in SELECTIONS:
                given = None
                for in_sweep in (True, False):
                    case = (classes, count, use_depth, use_desc, in_sweep)
                    _shapes(g, 4)
                    ref, ref_flags = _gpu_step(g, cloud, use_depth, use_desc, in_sweep, given)
                    _shapes(g, 1)
                    got, flags = _gpu_step(g, cloud, use_depth, use_desc, in_sweep, given)
                    assert np.array_equal(flags, ref_flags), case
                    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), case
                    assert not ref_flags[deleted].any() and (count == 1 or ref_flags.any()), case
                    given = ref_flags       # the flags the sweep decided, for the step that takes them as they are


# ---- beyond the replayed masks: the position pass tests a chunk of keyframes itself only from chunk kMaskChunks = 4 of a class on, i.e.
# from keyframe 1024 at four sum classes; there it reads the parked bounding sphere and recomputes the norms of the frustum planes --------
LATE_KEYFRAMES = 1040                       # 16 keyframes in the fifth chunks: four per class
LATE_FIRST = 1024
LOOKING_AWAY = (1025, 1030, 1035)           # turned by pi about y: the sphere test must reject them, the others it must keep


@pytest.fixture(scope="module")
def late_pair():
    """(oracle, GPU scene, the cloud of keyframe 0, the scene) with 1040 keyframes of 64 x 48 pixels, built once"""
    from badslam_amd import se3
    scene = common.small_scene(num_keyframes=LATE_KEYFRAMES, width=64, height=48, seed=22, translation_range=0.3, rotation_range=0.15)
    away = se3.exp([0, 0, 0, 0, np.pi, 0])
    for k in LOOKING_AWAY:
        scene.poses_gt[k] = se3.mul(scene.poses_gt[k], away)
    ba = common.build_oracle(scene, 8192, create_from=[0])
    g = common.build_gpu(scene, 8192, create_from=[])
    data, _ = common.oracle_surfels(ba)
    assert data.shape[1] >= max(SURFEL_COUNTS)
    return ba, g, data, scene


def test_keyframes_beyond_the_replayed_masks_exact_flavour_gives_the_oracles_step(late_pair, request):
    from badslam_amd import se3
    ba, g, data, scene = late_pair
    g.ctx.set_arithmetic("exact")
    g.set_sum_classes(4)
    ob.lib().orc_set_sum_classes(4)
    _shapes(g, 1)
    request.addfinalizer(lambda: _shapes(g, 0))
    g.bind_keyframes()
    for count in (65, 193):
        cloud, deleted = _cloud(data, count)
        for use_depth, use_desc in SELECTIONS:
            ref, ref_flags = _oracle_step(ba, cloud, use_depth, use_desc)
            assert ref_flags.any() and not ref_flags[deleted].any()
            for in_sweep in (True, False):
                got, flags = _gpu_step(g, cloud, use_depth, use_desc, in_sweep, ref_flags)
                case = (count, use_depth, use_desc, in_sweep)
                assert np.array_equal(flags, ref_flags), case
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), case
    # the keyframes from 1024 on are part of that result: with them turned away the oracle's step ends elsewhere, so a sphere test
    # that wrongly rejected them could not have given the bits above
    away = se3.exp([0, 0, 0, 0, np.pi, 0])
    try:
        for k in range(LATE_FIRST, LATE_KEYFRAMES):
            if k not in LOOKING_AWAY:
                ba.set_pose(k, se3.mul(scene.poses_gt[k], away))
        without, _ = _oracle_step(ba, cloud, True, True)
    finally:
        for k in range(LATE_FIRST, LATE_KEYFRAMES):
            ba.set_pose(k, scene.poses_gt[k])
    full, _ = _oracle_step(ba, cloud, True, True)
    assert np.count_nonzero(full.view(np.uint32) != without.view(np.uint32)) > 100


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
def test_keyframes_beyond_the_replayed_masks_one_wavefront_shape_gives_the_four_wavefront_shapes_bits(late_pair, arithmetic, request):
    ba, g, data, scene = late_pair
    g.ctx.set_arithmetic(arithmetic)
    g.set_sum_classes(4)

    def restore():
        _shapes(g, 0)
        g.ctx.set_arithmetic("exact")
    request.addfinalizer(restore)
    g.bind_keyframes()
    for count in (65, 193):
        cloud, deleted = _cloud(data, count)
        for use_depth, use_desc in SELECTIONS:
            given = None
            for in_sweep in (True, False):
                case = (count, use_depth, use_desc, in_sweep)
                _shapes(g, 4)
                ref, ref_flags = _gpu_step(g, cloud, use_depth, use_desc, in_sweep, given)
                _shapes(g, 1)
                got, flags = _gpu_step(g, cloud, use_depth, use_desc, in_sweep, given)
                assert np.array_equal(flags, ref_flags), case
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), case
                assert ref_flags.any() and not ref_flags[deleted].any(), case
                given = ref_flags


def _bundle_adjustment(scene, perturbed, surfels, fast):
    from badslam_amd.directba import DirectBA
    ba = DirectBA(600000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    ba.SetFastArithmetic(fast)
    for k in range(len(scene.depth)):
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], scene.poses_gt[k])
    ba.upload_surfels(surfels)
    for k, T in enumerate(perturbed):
        ba.set_keyframe_pose(k, T)
    ba.set_ba_iteration_counts(1, 1)      # no end tasks: the surfel set and its order stay
    done, _ = ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, increase_ba_iteration_count=False,
                                  min_iterations=5, max_iterations=5)
    poses = np.asarray([ba.keyframe_pose(k) for k in range(len(perturbed))], np.float32)
    return done, poses, ba.download_surfels(8)


@pytest.fixture(scope="module")
def ba_inputs():
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=6, seed=33)
    rng = np.random.Generator(np.random.PCG64(4))
    perturbed = [synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    ba = DirectBA(600000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    for k in range(len(scene.depth)):
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], scene.poses_gt[k])
    for k in range(len(scene.depth)):
        ba.CreateSurfelsForKeyframe(k, filter_new_surfels=False)
    surfels = ba.download_surfels(8)
    rng = np.random.Generator(np.random.PCG64(5))
    surfels[2] += rng.uniform(0, 0.004, surfels.shape[1]).astype(np.float32)
    return scene, perturbed, surfels


@pytest.mark.parametrize("cloud", ["whole cloud", "193 surfels with a deleted tile"])
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_five_bundle_adjustment_iterations_end_with_the_four_wavefront_shapes_bits(ba_inputs, fast, cloud):
    scene, perturbed, surfels = ba_inputs
    if cloud != "whole cloud":
        surfels = surfels[:, ::max(1, surfels.shape[1] // 193)][:, :193].copy()
        surfels[0, 64:128] = np.nan
        surfels[0, [5, 17, 40, 62]] = np.nan
    lib = capi.load()
    runs = {}
    try:
        for shape in (4, 1):
            capi.check(lib.bahip_debug_set_launch_shapes(shape, 0))
            runs[shape] = _bundle_adjustment(scene, perturbed, surfels, fast)
    finally:
        capi.check(lib.bahip_debug_set_launch_shapes(0, 0))
    assert runs[1][0] == runs[4][0] == 5
    assert np.array_equal(runs[1][1].view(np.uint32), runs[4][1].view(np.uint32))
    assert np.array_equal(runs[1][2].view(np.uint32), runs[4][2].view(np.uint32))
    live = surfels[0] == surfels[0]
    assert np.any(runs[1][2][:3, live] != surfels[:3, live])      # the iterations moved the cloud
