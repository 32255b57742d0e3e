"""DirectBA::ComputeReducedCameraSystem and ::ComputePoseCovariances (dba_reduced_camera_system, dba_pose_covariances,
DirectBA.reduced_camera_system, DirectBA.pose_covariances) against the C-ABI call on the state the object holds -- after creation, and
after a BundleAdjustment with surfel updates --, the covariances against numpy.linalg.inv of the same returned words with the gauge rows
removed, the refusals, and `ba_tum --pose_information_file`: the file it writes against the state it saved.

The covariances against numpy.linalg.inv: the largest |difference| over the largest |word| of the inverse, measured on the three
scenes below (four keyframes after creation, six after a BundleAdjustment, the runner's four), is MEASURED_DIFFERENCE = 1.85e-14
(3.4e-15, 4.3e-15 and 1.84e-14; the condition numbers of the three reduced systems are 160 .. 360); the bound is 16 x that."""
import ctypes as C
import math

import numpy as np
import pytest

from badslam_amd import capi, lowlevel
from tests import common, state_file, tum_writer
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_tum_pipeline import BIN, _run

pytestmark = pytest.mark.gpu

FILL = 0xA5
MEASURED_DIFFERENCE = 1.85e-14
COVARIANCE_BOUND = 16 * MEASURED_DIFFERENCE


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _lowlevel_system(ba, K, marginalise=True):
    """bahip_reduced_camera_system on the object's own context (bound by the object's last call) and surfel buffer, the words prefilled."""
    ctx = ba.backend_context()
    n = 6 * K
    bufs = [lowlevel.DeviceBuffer2D(ctx, 1, size, np.float64).clear(FILL) for size in (n * n, n, 36 * K, n)]
    s = ba.surfels_struct()
    stats = (C.c_uint64 * 6)()
    capi.check(ctx.lib.bahip_reduced_camera_system(ctx.handle, 1, 1, int(marginalise), C.byref(s),          # (the object's residual switches: both on)
                                                   bufs[0].ptr, n, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, stats))
    ctx.synchronize()
    S, g, A, b = (buf.download()[0].copy() for buf in bufs)
    for buf in bufs:
        buf.free()
    return S.reshape(n, n), g, A.reshape(K, 6, 6), b.reshape(K, 6), [int(v) for v in stats]


def _check_against_the_lowlevel_call(ba, what, ids_expected):
    got = ba.reduced_camera_system()
    K = len(ids_expected)
    assert got["keyframe_ids"] == ids_expected and got["S"].shape == (6 * K, 6 * K)
    S, g, A, b, stats = _lowlevel_system(ba, K)
    for name, mine, theirs in (("S", got["S"], S), ("g", got["g"], g), ("A", got["A"], A), ("b", got["b"], b)):
        assert np.array_equal(_bits(mine), _bits(theirs)), (what, name)
    assert list(got["stats"].values()) == stats and got["stats"]["invalid"] == 0 and got["stats"]["pairs_visited"] > 0, what
    assert np.array_equal(_bits(got["S"]), _bits(got["S"].T))
    plain = ba.reduced_camera_system(marginalise=False)
    assert np.array_equal(_bits(plain["A"]), _bits(got["A"])) and np.array_equal(_bits(plain["g"]), _bits(got["b"].reshape(-1)))
    for k in range(K):
        assert np.array_equal(_bits(plain["S"][6 * k:6 * k + 6, 6 * k:6 * k + 6]), _bits(got["A"][k]))
    return got


def _covariance_difference(ba, system, gauge, what):
    """pose_covariances against numpy.linalg.inv of the returned S without the gauge rows: the largest difference over the largest word."""
    ids = system["keyframe_ids"]
    rest = [k for k in ids if k != gauge]
    pairs = [(rest[0], rest[-1]), (rest[-1], rest[0]), (rest[1], rest[1])]
    got_ids, marginal, cross = ba.pose_covariances(gauge, pairs)
    assert got_ids == rest and marginal.shape == (len(rest), 6, 6) and cross.shape == (3, 6, 6)
    keep = np.concatenate([np.arange(6 * ids.index(k), 6 * ids.index(k) + 6) for k in rest])
    reduced = system["S"][np.ix_(keep, keep)]
    inverse = np.linalg.inv(reduced)
    scale = np.abs(inverse).max()
    block = lambda i, j: inverse[6 * rest.index(i):6 * rest.index(i) + 6, 6 * rest.index(j):6 * rest.index(j) + 6]          # noqa: E731
    difference = max(max(np.abs(marginal[q] - block(k, k)).max() for q, k in enumerate(rest)),
                     max(np.abs(cross[q] - block(i, j)).max() for q, (i, j) in enumerate(pairs))) / scale
    print(what, "covariances against numpy.linalg.inv: largest difference over the largest word", difference, "condition number", np.linalg.cond(reduced),
          "standard deviations of the first remaining keyframe", np.sqrt(np.diag(marginal[0])).tolist())
    assert np.array_equal(cross[0], cross[1].T) and np.array_equal(cross[2], marginal[1])
    assert all((np.diag(m) > 0).all() and np.array_equal(m, m.T) for m in marginal)
    assert difference <= COVARIANCE_BOUND, (what, difference)
    return difference


def test_the_host_class_is_the_lowlevel_call_after_creation_and_skips_a_deleted_keyframe():
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    assert ba.surfels_size() > 10000
    full = _check_against_the_lowlevel_call(ba, "after creation", [0, 1, 2, 3])
    _covariance_difference(ba, full, 0, "after creation, gauge 0")
    _covariance_difference(ba, full, 2, "after creation, gauge 2")
    # refusals by name, nothing raised but the reason
    for gauge, pairs, reason in ((7, (), "gauge keyframe 7 does not exist"), (0, [(0, 1)], "names the gauge keyframe"), (0, [(1, 9)], "does not exist")):
        with pytest.raises(ValueError, match=reason):
            ba.pose_covariances(gauge, pairs)
    assert ba.L.dba_delete_keyframe(ba.h, 2) == 0
    left = _check_against_the_lowlevel_call(ba, "keyframe 2 deleted", [0, 1, 3])
    assert left["S"].shape == (18, 18)
    # the flat C view: too few rows are refused with the number needed, nothing else written
    rows = C.c_int(-1)
    words = np.full(36 * 4, np.nan)
    assert ba.L.dba_reduced_camera_system(ba.h, ba.stream, 1, 2, words.ctypes.data, words.ctypes.data, None, None, None, None, C.byref(rows)) != 0
    assert rows.value == 3 and np.isnan(words).all()


def test_a_keyframe_that_sees_nothing_is_a_pivot_that_is_not_positive():
    scene = common.small_scene(num_keyframes=3, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(3):
        ba.CreateSurfelsForKeyframe(k)
    away = np.array(scene.poses_gt[0], np.float32).copy()
    away[4:7] += 100.0                                       # a hundred metres off: it is paired with no surfel
    assert ba.AddKeyframe(scene.depth[0], scene.rgb[0], away) == 3
    system = ba.reduced_camera_system()
    assert not system["S"][18:].any() and not system["A"][3].any()
    with pytest.raises(ValueError, match=r"pivot 12 \(keyframe 3, unknown 0\) is not positive"):
        ba.pose_covariances(0)
    ids, marginal, _ = ba.pose_covariances(3)                # with that keyframe as the gauge the rest is determined
    assert ids == [0, 1, 2] and (np.diagonal(marginal, axis1=1, axis2=2) > 0).all()


def test_the_host_class_after_a_bundle_adjustment_with_surfel_updates():
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    ba = _build(scene, start)
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)
    assert ba.surfels_size() > 10000
    system = _check_against_the_lowlevel_call(ba, "after BundleAdjustment", list(range(6)))
    _covariance_difference(ba, system, 0, "after BundleAdjustment, gauge 0")


def test_ba_tum_writes_the_pose_information_of_the_final_state(tmp_path):
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=4, width=320, height=240, seed=7)
    rng = np.random.Generator(np.random.PCG64(8))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    state = str(tmp_path / "final.state")
    written = tmp_path / "pose_information.txt"
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "out"), "--cell", "2", "--max_depth", "8", "--iterations", "2", "--save_state", state,
                "--pose_information_file", str(written), "--pose_information_gauge", "1"])
    s = state_file.read_state(state)
    assert len(s["keyframes"]) == 4 and s["surfels_size"] > 10000
    w, h = s["depth_camera"]["width"], s["depth_camera"]["height"]
    # the saved state again (as tests/test_gpu_directba_observed_covisibility.py rebuilds it)
    ba = DirectBA(s["surfels_size"] + 64, s["raw_to_float_depth"], s["baseline_fx"], s["sparse_surfel_cell_size"], w, h,
                  s["color_camera"]["parameters"], s["depth_camera"]["parameters"])
    scale = np.float32(s["raw_to_float_depth"])
    for kf in s["keyframes"]:
        depth = scene.depth[kf["frame_index"]].copy()
        depth[depth == 65535] = 0
        filtered = lowlevel.bilateral_filtering_and_depth_cutoff(ba.backend_context(), depth, 1.5, 0.005, 2.0, int(np.float32(8.0) / scale), float(scale))
        assert ba.AddKeyframe(filtered, scene.rgb[kf["frame_index"]], s["frame_poses"][kf["frame_index"]]) == kf["id"]
    ba.upload_surfels(s["surfels"])
    system = ba.reduced_camera_system()
    ids = system["keyframe_ids"]
    _covariance_difference(ba, system, 1, "the runner's state, gauge 1")
    rest, marginal, _ = ba.pose_covariances(1)
    lines = [line.split() for line in open(written).read().splitlines()]
    assert len(lines) == 3 + 6 and [int(line[0]) for line in lines[:3]] == rest == [0, 2, 3]
    for q, line in enumerate(lines[:3]):
        assert [float(v) for v in line[1:]] == [math.sqrt(marginal[q][i, i]) for i in range(6)], q
    expected = [(ids[i], ids[j]) for i in range(4) for j in range(i + 1, 4)]
    assert [(int(line[0]), int(line[1])) for line in lines[3:]] == expected
    for line, (a, b) in zip(lines[3:], expected):
        block = system["S"][6 * ids.index(a):6 * ids.index(a) + 6, 6 * ids.index(b):6 * ids.index(b) + 6]
        squares = 0.0
        for value in block.reshape(-1):
            squares += float(value) * float(value)
        assert float(line[2]) == math.sqrt(squares) > 0, (a, b)
    assert f"wrote the pose information of 4 keyframe(s) (gauge keyframe 1) to {written}: {system['stats']['list_entries']} list entries" in log
