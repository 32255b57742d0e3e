"""DirectBA::ComputeSurfelObservations (dba_surfel_observations, DirectBA.surfel_observations) against the C-ABI call on the state the
object holds -- after creation, with a deleted keyframe (keyframe_ids skip it), and after a BundleAdjustment with surfel updates
(merging, deletion, compaction, the spatial reorder) --, and `ba_tum --observations_file`: the file it writes against the table of the
state it saved.  Equalities throughout; the payload planes are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi, lowlevel
from tests import common, state_file, tum_writer
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_tum_pipeline import BIN, _run

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _lowlevel_table(ba):
    """bahip_surfel_observations on the object's own context (bound by the object's last call) and surfel buffer: a count-only call, then
    the fill into prefilled planes of exactly P entries."""
    ctx = ba.backend_context()
    s = ba.surfels_struct()
    n = int(s.surfels_size)
    pairs = C.c_uint64()
    first = lowlevel.DeviceBuffer2D(ctx, 1, n + 1, np.uint32).clear(FILL)
    capi.check(ctx.lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(capi.Observations(first.ptr, None, None, None, 0)), C.byref(pairs)))
    P = int(pairs.value)
    ks = lowlevel.DeviceBuffer2D(ctx, 1, max(1, P), np.uint16).clear(FILL)
    depth = lowlevel.DeviceBuffer2D(ctx, 1, max(1, P), np.float32).clear(FILL)
    desc = lowlevel.DeviceBuffer2D(ctx, 1, max(1, 2 * P), np.float32).clear(FILL)
    capi.check(ctx.lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(capi.Observations(first.ptr, ks.ptr, depth.ptr, desc.ptr, P)), C.byref(pairs)))
    assert pairs.value == P
    out = dict(first=first.download()[0].copy(), keyframes=ks.download()[0, :P].copy(), depth_raw=depth.download()[0, :P].copy(),
               descriptor_raw=desc.download()[0, :2 * P].reshape(P, 2).copy())
    for b in (first, ks, depth, desc):
        b.free()
    return out


def _check_against_the_lowlevel_call(ba, what, ids_expected):
    got = ba.surfel_observations(residuals=True)
    plain = ba.surfel_observations()
    expected = _lowlevel_table(ba)
    P = len(expected["keyframes"])
    print(what, got["keyframe_ids"], "pairs", P, "lengths", np.bincount(np.diff(got["first"].astype(np.int64))).tolist())
    assert got["keyframe_ids"] == ids_expected == plain["keyframe_ids"] and set(plain) == {"keyframe_ids", "first", "keyframes"}
    assert got["first"].dtype == np.uint32 and got["keyframes"].dtype == np.uint16 and len(got["first"]) == ba.surfels_size() + 1
    assert P > 10000 and got["first"][-1] == P
    for name in ("first", "keyframes"):
        assert np.array_equal(got[name], expected[name]) and np.array_equal(plain[name], expected[name]), (what, name)
    for name in ("depth_raw", "descriptor_raw"):
        assert got[name].dtype == np.float32 and np.array_equal(got[name].view(np.uint32), expected[name].view(np.uint32)), (what, name)
    _, per = ba.compute_cost()
    assert [per[k]["depth_residuals"] for k in ids_expected] == np.bincount(got["keyframes"], minlength=len(ids_expected)).tolist()
    return got


def test_the_host_class_is_the_lowlevel_call_after_creation_and_skips_a_deleted_keyframe():
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    assert ba.surfels_size() > 10000
    full = _check_against_the_lowlevel_call(ba, "after creation", [0, 1, 2, 3])
    assert ba.L.dba_delete_keyframe(ba.h, 2) == 0
    left = _check_against_the_lowlevel_call(ba, "keyframe 2 deleted", [0, 1, 3])
    # the lists without keyframe 2, the bound indices renumbered
    keep = full["keyframes"] != 2
    surfel_of = np.repeat(np.arange(len(full["first"]) - 1), np.diff(full["first"].astype(np.int64)))
    assert np.array_equal(np.array([0, 1, 3])[left["keyframes"]], full["keyframes"][keep])
    assert np.array_equal(np.diff(left["first"].astype(np.int64)), np.bincount(surfel_of[keep], minlength=len(full["first"]) - 1))
    assert np.array_equal(left["depth_raw"].view(np.uint32), full["depth_raw"][keep].view(np.uint32))
    # the flat C view: too little room is refused with the sizes needed, nothing else written
    pairs, K = C.c_uint64(), C.c_int(-1)
    words = np.full(ba.surfels_size() + 1, 0xA5A5A5A5, np.uint32)
    ks = np.full(8, 0xA5A5, np.uint16)
    assert ba.L.dba_surfel_observations(ba.h, ba.stream, ba.surfels_size(), 8, 3, words.ctypes.data, ks.ctypes.data, None, None, None,
                                        C.byref(pairs), C.byref(K)) != 0
    assert pairs.value == len(left["keyframes"]) and K.value == 3 and (words == 0xA5A5A5A5).all() and (ks == 0xA5A5).all()


def test_the_host_class_after_a_bundle_adjustment_with_surfel_updates():
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    ba = _build(scene, start)
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)
    assert ba.surfels_size() > 10000
    _check_against_the_lowlevel_call(ba, "after BundleAdjustment", list(range(6)))


def test_ba_tum_writes_the_observation_lists_of_the_final_state(tmp_path):
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=4, width=320, height=240, seed=7)
    rng = np.random.Generator(np.random.PCG64(8))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    state = str(tmp_path / "final.state")
    written = tmp_path / "observations.txt"
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "out"), "--cell", "2", "--max_depth", "8", "--iterations", "2", "--save_state", state,
                "--observations_file", str(written)])
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
    t = ba.surfel_observations()
    ids = t["keyframe_ids"]
    first = t["first"].astype(np.int64)
    lengths = np.diff(first)
    assert ids == [kf["id"] for kf in s["keyframes"]] and len(t["keyframes"]) > 10000

    def check(path, log):
        lines = [[int(v) for v in line.split()] for line in open(path).read().splitlines()]
        assert [line[0] for line in lines] == np.flatnonzero(lengths).tolist()
        for line in lines:
            i = line[0]
            assert line[1] == lengths[i] == len(line) - 2, i
            assert line[2:] == [ids[k] for k in t["keyframes"][first[i]:first[i + 1]]], i
        histogram = " ".join(f"{c}:{v}" for c, v in enumerate(np.bincount(lengths)))
        below = int(np.count_nonzero(lengths == 1))
        assert (f"wrote the observation lists of {len(lengths)} surfel(s) to {path}: {len(t['keyframes'])} pair(s), list lengths {histogram}, "
                f"{below} observed surfel(s) below min_observation_count 2") in log

    check(written, log)
    # the same file from the loaded state
    again = tmp_path / "again.txt"
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "again"), "--cell", "2", "--max_depth", "8", "--iterations", "0", "--load_state", state,
                "--observations_file", str(again)])
    check(again, log)
    assert open(again).read() == open(written).read()
