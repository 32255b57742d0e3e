"""DirectBA::ComputeKeyframeRedundancy, FindRedundantKeyframes and CullRedundantKeyframes (dba_keyframe_redundancy,
dba_find_redundant_keyframes, dba_cull_redundant_keyframes and the Python wrappers): the table against the C-ABI call on the state the
object holds -- after creation, with a deleted keyframe, and after a BundleAdjustment with surfel updates --, the find rule and the
greedy cull against the model of tests/keyframe_redundancy.py on a scene of duplicated views whose census
tests/test_cpu_keyframe_redundancy.py asserts, and the runner: `ba_tum --redundancy_file` against the table of the state it saved,
`--cull_redundant_keyframes` against the keyframes of the state it saved, and a run without either option beside one with the file:
the same bytes in every other output.  Equalities throughout."""
import ctypes as C
import os

import numpy as np
import pytest

from badslam_amd import capi, lowlevel
from tests import common, state_file, tum_writer
from tests import keyframe_redundancy as kr
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_tum_pipeline import BIN, _run

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _lowlevel_table(ba, K, bins):
    """bahip_keyframe_observer_histogram on the object's own context (bound by the object's last call) and surfel buffer, the words
    prefilled."""
    ctx = ba.backend_context()
    buf = lowlevel.DeviceBuffer2D(ctx, 1, K * bins, np.uint32).clear(FILL)
    s = ba.surfels_struct()
    capi.check(ctx.lib.bahip_keyframe_observer_histogram(ctx.handle, C.byref(s), bins, buf.ptr, bins))
    ctx.synchronize()
    out = buf.download().reshape(K, bins).copy()
    buf.free()
    return out


def _check_against_the_lowlevel_call(ba, what, ids_expected, bins=16):
    ids, hist = ba.keyframe_redundancy(bins)
    print(what, ids, hist.tolist())
    K = len(ids_expected)
    assert ids == ids_expected and hist.shape == (K, bins) and hist.dtype == np.uint32
    assert np.array_equal(hist, _lowlevel_table(ba, K, bins)), what
    _, per = ba.compute_cost()
    assert [per[k]["depth_residuals"] for k in ids] == hist.sum(axis=1).tolist() and (hist.sum(axis=1) > 1000).all()
    _, counts = ba.observed_covisibility()
    assert np.diag(counts).tolist() == hist.sum(axis=1).tolist()
    lengths = np.bincount(np.diff(ba.surfel_observations()["first"].astype(np.int64)), minlength=bins + 1)
    assert [int(v) for v in hist.sum(axis=0)[:bins - 1]] == [(j + 1) * int(lengths[j + 1]) for j in range(bins - 1)]
    return hist


def test_the_host_class_is_the_lowlevel_call_after_creation_and_skips_a_deleted_keyframe():
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    assert ba.surfels_size() > 10000
    full = _check_against_the_lowlevel_call(ba, "after creation", [0, 1, 2, 3])
    _check_against_the_lowlevel_call(ba, "after creation, 3 bins", [0, 1, 2, 3], bins=3)
    assert ba.L.dba_delete_keyframe(ba.h, 2) == 0
    left = _check_against_the_lowlevel_call(ba, "keyframe 2 deleted", [0, 1, 3])
    assert left.sum() < full.sum() and np.array_equal(left.sum(axis=1), full.sum(axis=1)[[0, 1, 3]])     # the other rows keep their totals
    assert left[:, 3].sum() == 0 and left[:, 0].sum() >= full[[0, 1, 3], 0].sum()                        # and lose an observer
    # the flat C view: too few rows are refused with the number needed, nothing else written
    rows = C.c_int(-1)
    words = np.full(2 * 16, 0xA5A5A5A5, np.uint32)
    assert ba.L.dba_keyframe_redundancy(ba.h, ba.stream, 16, 2, words.ctypes.data, None, C.byref(rows)) != 0
    assert rows.value == 3 and (words == 0xA5A5A5A5).all()
    assert ba.L.dba_keyframe_redundancy(ba.h, ba.stream, 65, 4, words.ctypes.data, None, C.byref(rows)) != 0 and (words == 0xA5A5A5A5).all()


def test_the_host_class_after_a_bundle_adjustment_with_surfel_updates():
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    ba = _build(scene, start)
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)
    assert ba.surfels_size() > 10000
    _check_against_the_lowlevel_call(ba, "after BundleAdjustment", list(range(6)))


def _duplicated_views():
    """The object in the state of kr.duplicated_views(): its twelve keyframes and the oracle's surfels."""
    from badslam_amd.directba import DirectBA
    scene, images, poses, orc, A = kr.duplicated_views()
    ba = DirectBA(100000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    for image, T in zip(images, poses):
        ba.AddKeyframe(scene.depth[image], scene.rgb[image], T)
    data, _ = common.oracle_surfels(orc)
    ba.upload_surfels(data[:8])
    return ba, A


def test_find_and_cull_follow_the_models_greedy_sequence():
    m, f = kr.CULL_RULE
    ba, A = _duplicated_views()
    K = kr.DUPLICATED_VIEWS
    ids, hist = ba.keyframe_redundancy()
    assert ids == list(range(K)) and np.array_equal(hist.astype(np.int64), kr.table(A, 16))
    for rule in ((m, f), (3, 0.9), (0, 1.0), (15, 0.0), (9, 0.65)):
        assert ba.find_redundant_keyframes(*rule) == kr.find(kr.table(A, 16), *rule), rule
    assert ba.find_redundant_keyframes(m, f, bins=8) == kr.find(kr.table(A, 8), m, f)
    assert ba.keyframe_count() == K and ba.keyframe_redundancy()[0] == list(range(K))       # finding deletes nothing
    # stopped by max_deletions, then by the rule: together the model's sequence
    expected, by_rule = kr.cull(A, m, f, K, 1)
    assert len(expected) >= 2 and by_rule
    assert ba.cull_redundant_keyframes(m, f, 2, protect_newest=1) == expected[:2]
    assert ba.keyframe_redundancy()[0] == [k for k in range(K) if k not in expected[:2]]
    assert ba.cull_redundant_keyframes(m, f, K, protect_newest=1) == expected[2:]
    left = [k for k in range(K) if k not in expected]
    ids, hist = ba.keyframe_redundancy()
    assert ids == left and 0 in left and K - 1 in left                                       # the protected keyframes survive
    assert np.array_equal(hist.astype(np.int64), kr.table(A[left], 16))
    assert ba.cull_redundant_keyframes(m, f, K, protect_newest=1) == []
    # more of the newest protected: another sequence; nothing protects the first but its place
    ba, A = _duplicated_views()
    expected = kr.cull(A, m, f, K, 3)[0]
    assert ba.cull_redundant_keyframes(m, f, K, protect_newest=3) == expected and not set(expected) & {0, 9, 10, 11}
    ba, A = _duplicated_views()
    expected = kr.cull(A, 0, 0.0, K, 0)[0]
    assert expected == list(range(1, K)) and ba.cull_redundant_keyframes(0, 0.0, K, protect_newest=0) == expected
    assert ba.keyframe_redundancy()[0] == [0]
    # the flat C view refuses a rule its sixteen bins cannot state
    n = C.c_int(-1)
    out = (C.c_int * K)()
    assert ba.L.dba_cull_redundant_keyframes(ba.h, ba.stream, 16, 0.5, K, 0, K, out, C.byref(n)) != 0 and n.value == -1
    assert ba.L.dba_find_redundant_keyframes(ba.h, ba.stream, 8, 0.5, 8, K, out, C.byref(n)) != 0 and n.value == -1


def _read_table(path):
    return [[int(v) for v in line.split()] for line in open(path).read().splitlines()]


def test_ba_tum_writes_the_keyframe_redundancy_of_the_final_state_and_changes_nothing_else(tmp_path):
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=4, width=320, height=240, seed=7)
    rng = np.random.Generator(np.random.PCG64(8))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    state = str(tmp_path / "final.state")
    written = tmp_path / "redundancy.txt"
    base = ["--cell", "2", "--max_depth", "8", "--iterations", "2"]
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "out")] + base + ["--save_state", state, "--redundancy_file", str(written),
                                                                                  "--redundancy_bins", "6"])
    assert f"wrote the keyframe redundancy of 4 keyframe(s) (6 bins) to {written}" in log
    s = state_file.read_state(state)
    assert len(s["keyframes"]) == 4 and s["surfels_size"] > 10000
    w, h = s["depth_camera"]["width"], s["depth_camera"]["height"]
    # the saved state again: the surfels, and the keyframes through the runner's preprocessing (its defaults, --max_depth 8) at the saved poses
    ba = DirectBA(s["surfels_size"] + 64, s["raw_to_float_depth"], s["baseline_fx"], s["sparse_surfel_cell_size"], w, h,
                  s["color_camera"]["parameters"], s["depth_camera"]["parameters"])
    scale = np.float32(s["raw_to_float_depth"])
    for kf in s["keyframes"]:
        depth = scene.depth[kf["frame_index"]].copy()
        depth[depth == 65535] = 0                                                       # as tum_writer stores "no measurement"
        filtered = lowlevel.bilateral_filtering_and_depth_cutoff(ba.backend_context(), depth, 1.5, 0.005, 2.0, int(np.float32(8.0) / scale), float(scale))
        assert ba.AddKeyframe(filtered, scene.rgb[kf["frame_index"]], s["frame_poses"][kf["frame_index"]]) == kf["id"]
    ba.upload_surfels(s["surfels"])
    ids, hist = ba.keyframe_redundancy(6)
    assert ids == [kf["id"] for kf in s["keyframes"]] and hist.sum() > 10000
    assert _read_table(written) == [[i, int(row.sum())] + row.tolist() for i, row in zip(ids, hist)]
    # the default number of bins, from the loaded state
    again = tmp_path / "again.txt"
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "again"), "--cell", "2", "--max_depth", "8", "--iterations", "0", "--load_state", state,
                "--redundancy_file", str(again)])
    ids, hist = ba.keyframe_redundancy(16)
    assert _read_table(again) == [[i, int(row.sum())] + row.tolist() for i, row in zip(ids, hist)]
    # a run without the new options: no word of them on the output, and every other file of the run above, byte for byte
    plain_state = str(tmp_path / "plain.state")
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "plain")] + base + ["--save_state", plain_state])
    assert "redundan" not in log and "culled" not in log
    assert open(plain_state, "rb").read() == open(state, "rb").read()
    for suffix in (".poses.txt", ".depth_intrinsics.txt", ".color_intrinsics.txt", ".deformation.txt", ".ply"):
        assert open(str(tmp_path / "plain") + suffix, "rb").read() == open(str(tmp_path / "out") + suffix, "rb").read(), suffix
    # options the runner refuses
    import subprocess
    for bad in (["--redundancy_bins", "65"], ["--cull_redundant_keyframes", "2"], ["--cull_redundant_keyframes", "16,0.5"],
                ["--cull_redundant_keyframes", "2,0.5", "--incremental"]):
        assert subprocess.run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "bad")] + base + bad, capture_output=True, timeout=600).returncode == 2, bad


def test_ba_tum_culls_redundant_keyframes_before_the_final_ba_call(tmp_path):
    scene = common.small_scene(num_keyframes=6, width=320, height=240, seed=4)
    rng = np.random.Generator(np.random.PCG64(6))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    state = str(tmp_path / "culled.state")
    table = tmp_path / "redundancy.txt"
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "out"), "--cell", "2", "--max_depth", "8", "--iterations", "2", "--save_state", state,
                "--cull_redundant_keyframes", "1,0.5", "--redundancy_file", str(table)])
    line, = [text for text in log.splitlines() if text.startswith("culled ")]
    print(line)
    deleted = [int(v) for v in line.split(":")[1].split()]
    assert line.startswith(f"culled {len(deleted)} redundant keyframe(s) (at least 0.5 of the surfels with 1 or more other observers):")
    assert len(deleted) >= 1 and len(set(deleted)) == len(deleted) and 0 not in deleted and 5 not in deleted
    assert log.index("culled ") < log.index("BA call 2")  and log.index("BA call 1") < log.index("culled ")
    s = state_file.read_state(state)
    left = [k for k in range(6) if k not in deleted]
    assert [kf["id"] if kf else None for kf in s["keyframes"]] == [k if k in left else None for k in range(6)]
    rows = _read_table(table)
    assert [row[0] for row in rows] == left and all(row[1] == sum(row[2:]) and len(row) == 18 for row in rows)
    assert os.path.getsize(str(tmp_path / "out") + ".ply") > 0
