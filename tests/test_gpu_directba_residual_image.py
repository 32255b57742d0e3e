"""DirectBA::KeyframeResidualImage / FrameResidualImage (dba_keyframe_residual_image, DirectBA.keyframe_residual_image) against the
low-level call on the same state -- after creation, and after a BundleAdjustment with surfel updates (merging, deletion, compaction,
the spatial reorder) -- and `ba_tum --residual_dir`: the files it writes against residual images of the state it saved."""
import os

import numpy as np
import pytest

from badslam_amd import capi, lowlevel
from tests import common, state_file, tum_writer
from tests import residual_image as ri
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_directba_render_view import _read_pnm
from tests.test_gpu_tum_pipeline import BIN, _run

pytestmark = pytest.mark.gpu


def _lowlevel_image(ba, k, frame_T_global, select, index_base=0):
    """bahip_frame_residual_image on the object's surfel buffer and keyframe k's images (with the packed planes the keyframe maintains)
    through its own context, the planes filled with 0xA5 bytes first."""
    return lowlevel.frame_residual_image(ba.backend_context(), ba.keyframe_frame(k), frame_T_global, ba.surfels_struct(), ba.width, ba.height,
                                         select=select, index_base=index_base, prefill=0xA5)


def _check_against_the_lowlevel_call(ba, what):
    last = ba.keyframe_count() - 1
    for select in (capi.RESIDUAL_BEST, capi.RESIDUAL_WORST):
        for k in (0, last):
            got = ba.keyframe_residual_image(k, select=select)                          # KeyframeResidualImage
            frame = got.pop("frame_T_global")
            explained = int(np.count_nonzero(got["index"] != ri.EMPTY_INDEX))
            print(what, "keyframe", k, "select", select, "explained", explained, "pairs", int(got["pairs"].sum()))
            assert explained > 5000 and int(got["index"][got["index"] != ri.EMPTY_INDEX].max()) < ba.surfels_size()
            assert int(got["pairs"].sum()) >= explained and np.count_nonzero(got["pairs"] > 1) > 10
            ri.assert_same_bits(got, _lowlevel_image(ba, k, frame, select), (what, "keyframe", k, select))
            # FrameResidualImage: the same images at a neighbour's pose, with an index offset
            other = ba.keyframe_pose(last - 1 if k == last else 1)
            free = ba.keyframe_residual_image(k, global_T_frame=other, select=select, index_base=1000)
            other_frame = free.pop("frame_T_global")
            assert not np.array_equal(other_frame, frame)
            ri.assert_same_bits(free, _lowlevel_image(ba, k, other_frame, select, 1000), (what, "another pose", k, select))
            assert not np.array_equal(free["pairs"], got["pairs"])
        own = ba.keyframe_residual_image(1, global_T_frame=ba.keyframe_pose(1), select=select)
        keyframe = ba.keyframe_residual_image(1, select=select)
        assert np.array_equal(own.pop("frame_T_global"), keyframe.pop("frame_T_global"))
        ri.assert_same_bits(own, keyframe, "FrameResidualImage at the keyframe's own pose")


def test_residual_images_are_the_lowlevel_call_on_the_same_state_after_creation():
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    assert ba.surfels_size() > 10000
    _check_against_the_lowlevel_call(ba, "after creation")


def test_residual_images_after_a_bundle_adjustment_with_surfel_updates():
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    ba = _build(scene, start)
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)
    assert ba.surfels_size() > 10000
    _check_against_the_lowlevel_call(ba, "after BundleAdjustment")


def _expected_files(image):
    """The stated rules: depth file 0 = no pair, else clamp(32768 + (int)floorf(raw * 1024 + 0.5f), 1, 65535) in binary32; pairs file
    min(pairs, 255); the summary's explained pixels, pairs, pixels with 2+ pairs, mean and RMS of the winners' raw in binary64, row-major."""
    covered = image["index"] != ri.EMPTY_INDEX
    raw = image["depth_residual"]
    scaled = np.floor(raw * np.float32(1024) + np.float32(0.5)).astype(np.float32)
    depth = np.where(covered, np.clip(32768 + scaled.astype(np.int64), 1, 65535), 0).astype(np.uint16)
    pairs = np.minimum(image["pairs"], 255).astype(np.uint8)
    mean = rms = 0.0
    winners = [float(v) for v in raw[covered]]                                         # row-major
    if winners:
        total = total_sq = 0.0
        for v in winners:
            total += v
            total_sq += v * v
        mean, rms = total / len(winners), float(np.sqrt(total_sq / len(winners)))
    return depth, pairs, (int(covered.sum()), int(image["pairs"].sum(dtype=np.int64)), int(np.count_nonzero(image["pairs"] >= 2)), mean, rms)


def test_ba_tum_writes_residual_images_of_the_final_state(tmp_path):
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=4, width=320, height=240, seed=7)
    rng = np.random.Generator(np.random.PCG64(8))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    images = tmp_path / "residuals"
    images.mkdir()
    state = str(tmp_path / "final.state")
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "out"), "--cell", "2", "--max_depth", "8", "--iterations", "2", "--save_state", state,
                "--residual_dir", str(images)])
    assert "wrote 4 residual image(s) (best pair per pixel)" in log
    assert sorted(os.listdir(images)) == sorted([f"residual_{k:06d}_{kind}" for k in range(4) for kind in ("depth.pgm", "pairs.pgm")] + ["residuals.txt"])
    s = state_file.read_state(state)
    assert len(s["keyframes"]) == 4 and s["surfels_size"] > 10000
    w, h = s["depth_camera"]["width"], s["depth_camera"]["height"]
    assert (w, h) == (320, 240) and s["a"] == 0 and not s["cfactor"].any()               # (no --intrinsics: the depth deformation is untouched)
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

    def check(directory, select):
        lines = [line.split() for line in open(directory / "residuals.txt").read().splitlines()]
        assert [int(line[0]) for line in lines] == [kf["id"] for kf in s["keyframes"]] and all(len(line) == 6 for line in lines)
        multi = []
        for kf, line in zip(s["keyframes"], lines):
            image = ba.keyframe_residual_image(kf["id"], select=select)
            depth, pairs, summary = _expected_files(image)
            kind, pw, ph, top, pixels = _read_pnm(str(directory / f"residual_{kf['id']:06d}_depth.pgm"))
            assert (kind, pw, ph, top) == ("P5", w, h, 65535) and len(pixels) == 2 * w * h
            assert np.array_equal(np.frombuffer(pixels, ">u2").reshape(h, w), depth)
            kind, pw, ph, top, pixels = _read_pnm(str(directory / f"residual_{kf['id']:06d}_pairs.pgm"))
            assert (kind, pw, ph, top) == ("P5", w, h, 255) and len(pixels) == w * h
            assert np.array_equal(np.frombuffer(pixels, np.uint8).reshape(h, w), pairs)
            # (cell 2: one surfel per 2 x 2 pixels, so a frame's pairs explain about a quarter of its pixels, not more)
            # a converged map has few pixels with two pairs (measured: 22 on keyframe 0, 2 on keyframe 1); one shows that the files count them
            assert summary[0] > 0.125 * w * h and summary[1] >= summary[0] + summary[2] and 1 < depth[depth > 0].min() and depth.max() < 65535
            multi.append(summary[2])
            assert (int(line[1]), int(line[2]), int(line[3])) == summary[:3]
            assert (float(line[4]), float(line[5])) == summary[3:]                       # 17 digits: the binary64 values themselves
            print("keyframe", kf["id"], "select", select, summary)
        assert sum(multi) >= 1
    check(images, capi.RESIDUAL_BEST)
    # the worst pair per pixel through the option, on the loaded state
    worst = tmp_path / "worst"
    worst.mkdir()
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "again"), "--cell", "2", "--max_depth", "8", "--iterations", "0", "--load_state", state,
                "--residual_dir", str(worst), "--residual_select", "worst"])
    assert "wrote 4 residual image(s) (worst pair per pixel)" in log
    check(worst, capi.RESIDUAL_WORST)
