"""Frame ingestion at a pyramid level through the whole chain: `ba_tum --pyramid_level_for_depth / --pyramid_level_for_color /
--median_filter_and_densify_iterations` on a synthetic TUM directory at 2W x 2H against `ba_tum` at level 0 on a directory that holds
the images the plain model (tests/frame_ingest.py) makes of them, with the scaled calibration -- every output file byte for byte.  The
intrinsics are dyadic (fx = 60, pixel-corner cx = 79.5, cy = 59.5 at 160 x 120), so halving them and the text round trip of
calibration.txt are exact.  Then the refused options, the state file at a pyramid level, and Scene.add_frame."""
import os
import subprocess
import types

import numpy as np
import pytest

from badslam_amd import lowlevel as ll
from tests import common, frame_ingest as fi, tum_writer

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "badslam_amd", "lib", "ba_tum")
FULL_W, FULL_H, KEYFRAMES = 160, 120, 4
OPTIONS = ["--cell", "2", "--max_depth", "8"]
OUTPUTS = (".poses.txt", ".ply", ".depth_intrinsics.txt", ".color_intrinsics.txt", ".deformation.txt")
REFUSAL = "Simultaneous downscaling and median filtering of depth maps is not implemented."


@pytest.fixture(scope="module")
def full():
    """The full-resolution sequence: raw depth with 0 = no measurement, made noisy and holey so that the median rules have even counts,
    ties and zeros to work on; colour; perturbed start poses."""
    scene = common.small_scene(num_keyframes=KEYFRAMES, width=FULL_W, height=FULL_H, seed=4)
    assert all(float(v) * 4 == int(float(v) * 4) for v in scene.camera)                      # dyadic: exact under halving
    rng = np.random.Generator(np.random.PCG64(21))
    depth = []
    for d in scene.depth:
        raw = np.where(d == 65535, 0, d).astype(np.int64)
        raw = np.where(raw > 0, raw + rng.integers(-6, 7, raw.shape), 0)
        raw = np.where(rng.random(raw.shape) < 0.12, 0, raw)
        depth.append(np.clip(raw, 0, 65534).astype(np.uint16))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    return types.SimpleNamespace(scene=scene, depth=depth, rgb=list(scene.rgb), camera=scene.camera, initial=initial)


def _write(folder, depth, rgb, camera, initial):
    os.makedirs(folder, exist_ok=True)
    as_scene = types.SimpleNamespace(depth=depth, rgb=rgb, camera=np.asarray(camera, np.float32))
    return tum_writer.write_dataset(folder, as_scene, {"initial.txt": initial})


def _run(folder, out, extra, expect=0):
    proc = subprocess.run([BIN, folder, "initial.txt", out] + OPTIONS + extra, capture_output=True, text=True, timeout=300)
    print(proc.stdout[-2000:])
    print(proc.stderr[-2000:])
    assert proc.returncode == expect, proc.returncode
    return proc


def _same_outputs(a, b, suffixes=OUTPUTS):
    for suffix in suffixes:
        blob_a, blob_b = open(a + suffix, "rb").read(), open(b + suffix, "rb").read()
        assert len(blob_a) > 0 and blob_a == blob_b, suffix


def _no_outputs(out):
    return not any(os.path.exists(out + suffix) for suffix in OUTPUTS)


@pytest.fixture(scope="module")
def half(full):
    """What the model makes of the full sequence at level 1, and the camera that goes with it."""
    camera, w, h = fi.scaled_camera(full.camera, FULL_W, FULL_H, 1)
    assert (w, h) == (80, 60)
    depth = [fi.downscale_depth_median(d, w, h) for d in full.depth]
    rgb = [fi.downscale_rgb_half(c, 1) for c in full.rgb]
    return types.SimpleNamespace(depth=depth, rgb=rgb, camera=camera)


def test_level_1_equals_level_0_on_the_models_half_size_directory(tmp_path, full, half):
    assert os.path.exists(BIN), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    a, b = str(tmp_path / "full"), str(tmp_path / "half")
    _write(a, full.depth, full.rgb, full.camera, full.initial)
    _write(b, half.depth, half.rgb, half.camera, full.initial)
    log = _run(a, a + "/out", ["--iterations", "2", "--pyramid_level_for_depth", "1", "--pyramid_level_for_color", "1"]).stdout
    assert "BA resolution: depth 80 x 60 (pyramid level 1), colour 80 x 60 (pyramid level 1)" in log
    log = _run(b, b + "/out", ["--iterations", "2"]).stdout
    assert "BA resolution: depth 80 x 60 (pyramid level 0), colour 80 x 60 (pyramid level 0)" in log
    _same_outputs(a + "/out", b + "/out")
    # the calibration written is the BA cameras': the halved one, cx and cy in the pixel-centre convention
    got = [float(v) for v in open(a + "/out.depth_intrinsics.txt").read().split()]
    assert got == [30.0, 30.0, 39.25, 29.25]
    assert int(open(a + "/out.ply", "rb").read().split(b"element vertex ")[1].split()[0]) > 500


def test_depth_level_1_with_colour_level_0(tmp_path, full, half):
    """`ba_tum` reads one calibration and takes both cameras' size from the first colour image, so a comparison run cannot have a depth
    camera of its own size: the run at levels (1, 0) is held to its resolution and its calibration files, and the keyframes it would
    build are compared through Scene.add_frame -- the same three device calls in the same order -- with a Scene of the two cameras."""
    a = str(tmp_path / "full")
    _write(a, full.depth, full.rgb, full.camera, full.initial)
    log = _run(a, a + "/out", ["--iterations", "2", "--pyramid_level_for_depth", "1", "--pyramid_level_for_color", "0"]).stdout
    assert "BA resolution: depth 80 x 60 (pyramid level 1), colour 160 x 120 (pyramid level 0)" in log
    assert [float(v) for v in open(a + "/out.depth_intrinsics.txt").read().split()] == [30.0, 30.0, 39.25, 29.25]
    assert [float(v) for v in open(a + "/out.color_intrinsics.txt").read().split()] == [60.0, 60.0, 79.0, 59.0]
    assert int(open(a + "/out.ply", "rb").read().split(b"element vertex ")[1].split()[0]) > 500
    _compare_scenes(full, half, 1, 0)


def test_two_median_iterations_equal_the_models_filtered_directory(tmp_path, full):
    # at level 0 the size is free: the left upper quarter of the frames, with the camera as it is
    depth = [np.ascontiguousarray(d[:60, :80]) for d in full.depth]
    rgb = [np.ascontiguousarray(c[:60, :80]) for c in full.rgb]
    filtered = [fi.median_filter_and_densify(d, 2) for d in depth]
    assert sum(int(np.count_nonzero((d == 0) & (f != 0))) for d, f in zip(depth, filtered)) > 100          # holes were filled
    a, b = str(tmp_path / "raw"), str(tmp_path / "filtered")
    _write(a, depth, rgb, full.camera, full.initial)
    _write(b, filtered, rgb, full.camera, full.initial)
    _run(a, a + "/out", ["--iterations", "2", "--median_filter_and_densify_iterations", "2"])
    _run(b, b + "/out", ["--iterations", "2"])
    _same_outputs(a + "/out", b + "/out")
    _run(a, a + "/plain", ["--iterations", "2"])
    assert open(a + "/plain.ply", "rb").read() != open(a + "/out.ply", "rb").read()                         # the option does something


def test_an_odd_number_of_median_iterations(tmp_path, full):
    """One and three iterations leave the filtered depth in the other image of the host's ping-pong pair."""
    depth = [np.ascontiguousarray(d[:60, :80]) for d in full.depth[:2]]
    rgb = [np.ascontiguousarray(c[:60, :80]) for c in full.rgb[:2]]
    a = str(tmp_path / "raw")
    _write(a, depth, rgb, full.camera, full.initial[:2])
    for iterations in (1, 3):
        b = str(tmp_path / ("filtered%d" % iterations))
        _write(b, [fi.median_filter_and_densify(d, iterations) for d in depth], rgb, full.camera, full.initial[:2])
        _run(a, a + "/out%d" % iterations, ["--iterations", "1", "--median_filter_and_densify_iterations", str(iterations)])
        _run(b, b + "/out", ["--iterations", "1"])
        _same_outputs(a + "/out%d" % iterations, b + "/out")


def test_refused_options(tmp_path, full):
    a = str(tmp_path / "full")
    _write(a, full.depth[:2], full.rgb[:2], full.camera, full.initial[:2])
    proc = _run(a, a + "/both", ["--pyramid_level_for_depth", "1", "--median_filter_and_densify_iterations", "1"], expect=2)
    assert REFUSAL in proc.stderr and _no_outputs(a + "/both")
    for option in ("--pyramid_level_for_depth", "--pyramid_level_for_color"):
        proc = _run(a, a + "/four", [option, "4"], expect=2)
        assert "must be in 0 .. 3" in proc.stderr and _no_outputs(a + "/four")
        proc = _run(a, a + "/minus", [option, "-1"], expect=2)
        assert "must be in 0 .. 3" in proc.stderr and _no_outputs(a + "/minus")


def test_state_file_round_trip_at_a_pyramid_level(tmp_path, full, half):
    a, b = str(tmp_path / "full"), str(tmp_path / "half")
    _write(a, full.depth, full.rgb, full.camera, full.initial)
    _write(b, half.depth, half.rgb, half.camera, full.initial)
    level = ["--pyramid_level_for_depth", "1", "--pyramid_level_for_color", "1"]
    state, again = a + "/a.state", a + "/b.state"
    _run(a, a + "/saved", ["--iterations", "1"] + level + ["--save_state", state])
    log = _run(a, a + "/loaded", ["--iterations", "0"] + level + ["--load_state", state, "--save_state", again]).stdout
    assert "loaded" in log and "%d keyframes" % KEYFRAMES in log
    assert open(state, "rb").read() == open(again, "rb").read()
    # the keyframes rebuilt from the full-size frames at level 1 are the model's: one more BA call from the state gives, byte for byte,
    # what it gives on the model's half-size directory at level 0 (where the state's cameras fit as they are)
    _run(a, a + "/resumed", ["--iterations", "1"] + level + ["--load_state", state])
    _run(b, b + "/resumed", ["--iterations", "1", "--load_state", state])
    _same_outputs(a + "/resumed", b + "/resumed")
    # at level 0 the stored cameras do not have the live cameras' size: refused cleanly
    proc = _run(a, a + "/level0", ["--iterations", "0", "--load_state", state], expect=1)
    assert "cannot load state" in proc.stderr and "size does not match" in proc.stderr and _no_outputs(a + "/level0")


def _planes(g, k):
    kf = g.keyframes[k]
    return [kf[name].download() for name in ("depth", "normals", "radius", "color")] + [kf["min_depth"], kf["max_depth"]]


def _compare_scenes(full, half, level_depth, level_color):
    scene = full.scene
    ctx = ll.Context()
    try:
        depth_cam = ll.scaled_camera(ll.make_camera(full.camera, FULL_W, FULL_H), level_depth)
        color_cam = ll.scaled_camera(ll.make_camera(full.camera, FULL_W, FULL_H), level_color)
        bilateral = (1.5, 0.005, 2.0, int(8.0 / scene.raw_to_float_depth))
        for use_bilateral in (False, True):
            g = ll.Scene(ctx, 1000, scene.raw_to_float_depth, scene.baseline_fx, 2, color_cam, depth_cam)
            m = ll.Scene(ctx, 1000, scene.raw_to_float_depth, scene.baseline_fx, 2, color_cam, depth_cam)
            for k in range(2):
                depth = half.depth[k] if level_depth else full.depth[k]
                rgb = half.rgb[k] if level_color else full.rgb[k]
                if use_bilateral:
                    depth = ll.bilateral_filtering_and_depth_cutoff(ctx, depth, *bilateral[:3], bilateral[3], scene.raw_to_float_depth)
                g.add_frame(full.depth[k], full.rgb[k], scene.poses_gt[k], level_depth, level_color, 0, bilateral if use_bilateral else None)
                m.add_keyframe(depth, rgb, scene.poses_gt[k])
                got, want = _planes(g, k), _planes(m, k)
                for name, x, y in zip(("depth", "normals", "radius", "color"), got, want):
                    assert x.shape == y.shape and np.array_equal(x, y), (use_bilateral, k, name)
                assert got[4:] == want[4:], (use_bilateral, k, got[4:], want[4:])
                if use_bilateral:
                    assert np.count_nonzero(got[0] != 65535) > 1000                          # real keyframes, not empty ones
    finally:
        ctx.close()


def test_scene_add_frame_at_levels_1_1(full, half):
    _compare_scenes(full, half, 1, 1)


def test_scene_add_frame_with_median_iterations_and_refusals(full):
    scene = full.scene
    ctx = ll.Context()
    try:
        cam = ll.make_camera(full.camera, FULL_W, FULL_H)
        g = ll.Scene(ctx, 1000, scene.raw_to_float_depth, scene.baseline_fx, 2, cam, cam)
        m = ll.Scene(ctx, 1000, scene.raw_to_float_depth, scene.baseline_fx, 2, cam, cam)
        g.add_frame(full.depth[0], full.rgb[0], scene.poses_gt[0], median_iterations=1)
        m.add_keyframe(ll.median_filter_and_densify(ctx, full.depth[0], 1), full.rgb[0], scene.poses_gt[0])
        for x, y in zip(_planes(g, 0), _planes(m, 0)):
            assert np.array_equal(x, y)
        with pytest.raises(ValueError, match="not implemented"):
            g.add_frame(full.depth[0], full.rgb[0], scene.poses_gt[0], 1, 1, 1)
        with pytest.raises(ValueError):
            g.add_frame(full.depth[0], full.rgb[0], scene.poses_gt[0], 4, 0)
        with pytest.raises(ValueError, match="depth camera"):
            g.add_frame(full.depth[0], full.rgb[0], scene.poses_gt[0], 1, 0)                 # the scene's cameras are the full ones
        assert len(g.keyframes) == 1
    finally:
        ctx.close()
