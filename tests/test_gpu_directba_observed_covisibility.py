"""DirectBA::ComputeObservedCovisibility (dba_observed_covisibility, DirectBA.observed_covisibility) against the C-ABI call on the state
the object holds -- after creation, and after a BundleAdjustment with surfel updates (merging, deletion, compaction, the spatial
reorder) --, with a deleted keyframe, and `ba_tum --covisibility_file`: the file it writes against the matrix and the lists of the state it
saved."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi, lowlevel
from tests import common, state_file, tum_writer
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_tum_pipeline import BIN, _run

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _lowlevel_matrix(ba, K):
    """bahip_observed_covisibility on the object's own context (bound by the object's last call) and surfel buffer, the words prefilled."""
    ctx = ba.backend_context()
    buf = lowlevel.DeviceBuffer2D(ctx, 1, K * K, np.uint32).clear(FILL)
    s = ba.surfels_struct()
    capi.check(ctx.lib.bahip_observed_covisibility(ctx.handle, C.byref(s), buf.ptr, K))
    ctx.synchronize()
    out = buf.download().reshape(K, K).copy()
    buf.free()
    return out


def _check_against_the_lowlevel_call(ba, what, ids_expected):
    ids, counts = ba.observed_covisibility()
    print(what, ids, counts.tolist())
    K = len(ids_expected)
    assert ids == ids_expected and counts.shape == (K, K) and counts.dtype == np.uint32
    assert np.array_equal(counts, _lowlevel_matrix(ba, K)), what
    assert np.array_equal(counts, counts.T) and (np.diag(counts) > 1000).all() and (counts > 0).all()
    _, per = ba.compute_cost()
    assert [per[k]["depth_residuals"] for k in ids] == np.diag(counts).tolist()
    return counts


def test_the_host_class_is_the_lowlevel_call_after_creation_and_skips_a_deleted_keyframe():
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    assert ba.surfels_size() > 10000
    full = _check_against_the_lowlevel_call(ba, "after creation", [0, 1, 2, 3])
    assert ba.L.dba_delete_keyframe(ba.h, 2) == 0
    left = _check_against_the_lowlevel_call(ba, "keyframe 2 deleted", [0, 1, 3])
    assert np.array_equal(left, full[np.ix_([0, 1, 3], [0, 1, 3])])
    # the flat C view: too few rows are refused with the number needed, nothing else written
    rows = C.c_int(-1)
    words = np.full(4, 0xA5A5A5A5, np.uint32)
    assert ba.L.dba_observed_covisibility(ba.h, ba.stream, 2, words.ctypes.data, None, C.byref(rows)) != 0
    assert rows.value == 3 and (words == 0xA5A5A5A5).all()


def test_the_host_class_after_a_bundle_adjustment_with_surfel_updates():
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    ba = _build(scene, start)
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)
    assert ba.surfels_size() > 10000
    _check_against_the_lowlevel_call(ba, "after BundleAdjustment", list(range(6)))


def test_ba_tum_writes_the_observed_covisibility_of_the_final_state(tmp_path):
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=4, width=320, height=240, seed=7)
    rng = np.random.Generator(np.random.PCG64(8))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    state = str(tmp_path / "final.state")
    written = tmp_path / "covisibility.txt"
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "out"), "--cell", "2", "--max_depth", "8", "--iterations", "2", "--save_state", state,
                "--covisibility_file", str(written)])
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
    ids, counts = ba.observed_covisibility()
    lists = {k: set(ba.keyframe_covisibility(k)) for k in ids}
    assert ids == [kf["id"] for kf in s["keyframes"]] and (counts > 0).all()

    def check(path, log):
        lines = [[int(v) for v in line.split()] for line in open(path).read().splitlines()]
        assert all(len(line) == 4 for line in lines)
        assert [(a, b) for a, b, _, _ in lines] == [(ids[i], ids[j]) for i in range(len(ids)) for j in range(i, len(ids))]
        shared = listed_without = unlisted = 0
        for a, b, count, frustum in lines:
            i, j = ids.index(a), ids.index(b)
            assert count == counts[i, j] == counts[j, i], (a, b)
            assert frustum == int(b in lists[a]), (a, b)
            if a != b:
                shared += count > 0
                listed_without += bool(frustum) and count == 0
                unlisted += (not frustum) and count > 0
        assert (f"wrote the observed co-visibility of {len(ids)} keyframe(s) to {path}: {shared} pair(s) share surfels, {listed_without} pair(s) of the "
                f"lists share none, {unlisted} sharing pair(s) are in no list") in log
        assert shared == 6

    check(written, log)
    # the same file from the loaded state
    again = tmp_path / "again.txt"
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "again"), "--cell", "2", "--max_depth", "8", "--iterations", "0", "--load_state", state,
                "--covisibility_file", str(again)])
    check(again, log)
    assert open(again).read() == open(written).read()
