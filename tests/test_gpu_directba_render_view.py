"""DirectBA::RenderSurfels / RenderKeyframeView (dba_render_surfels, DirectBA.render_surfels) against the low-level call on the same
state -- after creation, and after a BundleAdjustment with surfel updates (merging, deletion, compaction, the spatial reorder) -- and
`ba_tum --render_dir`: the files it writes against a render of the state it saved."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from badslam_amd import capi, lowlevel
from tests import common, state_file, tum_writer
from tests import render_view as rv
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_tum_pipeline import BIN, _run

pytestmark = pytest.mark.gpu

PLANES = (("depth", np.float32, 1), ("index", np.uint32, 1), ("normal", np.float32, 3), ("color", np.uint8, 4))


def _lowlevel_view(ba, view, frame_T_global, options):
    """bahip_render_surfels on the object's surfel buffer through its own context, the planes filled with 0xFF bytes first."""
    ctx, s = ba.backend_context(), ba.surfels_struct()
    w, h = view.width, view.height
    bufs = {name: lowlevel.DeviceBuffer2D(ctx, 1, w * h, dtype, channels).clear(0xFF) for name, dtype, channels in PLANES}
    out = capi.RenderOut(None, *[bufs[name].ptr for name, _, _ in PLANES])
    F = (C.c_float * 12)(*[float(v) for v in frame_T_global])
    capi.check(ctx.lib.bahip_render_surfels(ctx.handle, C.byref(s), C.byref(view), F, C.byref(options), C.byref(out)))
    planes = {name: bufs[name].download()[0].reshape((h, w) if channels == 1 else (h, w, channels)).copy() for name, _, channels in PLANES}
    for b in bufs.values():
        b.free()
    return planes


def _check_against_the_lowlevel_call(ba, scene, what):
    depth_view = lowlevel.make_camera(scene.camera, scene.width, scene.height)
    other = rv.scaled_camera(rv.camera(scene.camera, scene.width, scene.height), 97, 61)
    other_view = lowlevel.make_camera([other.fx, other.fy, other.cx, other.cy], other.width, other.height)
    for options in (capi.RenderOptions(), capi.RenderOptions(mode=capi.RENDER_POINT), capi.RenderOptions(max_radius_px=9, radius_factor=1.5, cull_backfaces=0)):
        for k in (0, ba.keyframe_count() - 1):
            got = ba.render_surfels(keyframe=k, options=options)                       # RenderKeyframeView
            frame = got.pop("frame_T_global")
            covered = int(np.count_nonzero(got["index"] != rv.EMPTY_INDEX))
            print(what, "keyframe", k, "mode", options.mode, "covered", covered)
            assert covered > 5000 and int(got["index"][got["index"] != rv.EMPTY_INDEX].max()) < ba.surfels_size()
            rv.assert_same_planes(got, _lowlevel_view(ba, depth_view, frame, options), (what, "keyframe view", k, options.mode))
            free = ba.render_surfels(view_camera=[other.fx, other.fy, other.cx, other.cy], width=other.width, height=other.height,
                                     global_T_frame=ba.keyframe_pose(k), options=options)   # RenderSurfels: another camera, the same pose
            assert np.array_equal(free.pop("frame_T_global"), frame)
            assert free["depth"].shape == (61, 97) and np.count_nonzero(free["index"] != rv.EMPTY_INDEX) > 500
            rv.assert_same_planes(free, _lowlevel_view(ba, other_view, frame, options), (what, "free view", k, options.mode))


def test_render_surfels_is_the_lowlevel_call_on_the_same_state_after_creation():
    scene = common.small_scene(num_keyframes=4, seed=23)
    ba = _build(scene, scene.poses_gt)
    for k in range(4):
        ba.CreateSurfelsForKeyframe(k)
    assert ba.surfels_size() > 10000
    _check_against_the_lowlevel_call(ba, scene, "after creation")


def test_render_surfels_after_a_bundle_adjustment_with_surfel_updates():
    scene = common.small_scene(num_keyframes=6, seed=17)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    ba = _build(scene, start)
    ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=2, max_iterations=2,
                        use_pcg=False, increase_ba_iteration_count=True)
    assert ba.surfels_size() > 10000
    _check_against_the_lowlevel_call(ba, scene, "after BundleAdjustment")


def _read_pnm(path):
    blob = open(path, "rb").read()
    m = re.match(rb"(P[56])\n(\d+) (\d+)\n(\d+)\n", blob)
    assert m, blob[:32]
    return m.group(1).decode(), int(m.group(2)), int(m.group(3)), int(m.group(4)), blob[m.end():]


def test_ba_tum_writes_one_pair_of_views_per_keyframe_that_are_renders_of_the_final_state(tmp_path):
    from badslam_amd.directba import DirectBA
    scene = common.small_scene(num_keyframes=4, width=320, height=240, seed=7)
    rng = np.random.Generator(np.random.PCG64(8))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    views = tmp_path / "views"
    views.mkdir()
    state = str(tmp_path / "final.state")
    log = _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "out"), "--cell", "2", "--max_depth", "8", "--iterations", "2", "--save_state", state,
                "--render_dir", str(views), "--render_max_radius", "3", "--render_radius_factor", "1.25"])
    assert "wrote 4 rendered view(s) (discs, at most 3 px)" in log
    assert sorted(os.listdir(views)) == sorted(f"render_{k:06d}_{kind}" for k in range(4) for kind in ("color.ppm", "depth.pgm"))
    s = state_file.read_state(state)
    assert len(s["keyframes"]) == 4 and s["surfels_size"] > 10000
    w, h = s["depth_camera"]["width"], s["depth_camera"]["height"]
    assert (w, h) == (320, 240)
    ba = DirectBA(s["surfels_size"] + 64, s["raw_to_float_depth"], s["baseline_fx"], s["sparse_surfel_cell_size"], w, h,
                  s["color_camera"]["parameters"], s["depth_camera"]["parameters"])
    ba.upload_surfels(s["surfels"])
    options = capi.RenderOptions(max_radius_px=3, radius_factor=1.25)
    for kf in s["keyframes"]:
        kind, pw, ph, top, pixels = _read_pnm(str(views / f"render_{kf['id']:06d}_depth.pgm"))
        assert (kind, pw, ph, top) == ("P5", w, h, 65535) and len(pixels) == 2 * w * h
        ckind, cw, ch, ctop, cpixels = _read_pnm(str(views / f"render_{kf['id']:06d}_color.ppm"))
        assert (ckind, cw, ch, ctop) == ("P6", w, h, 255) and len(cpixels) == 3 * w * h
        out = ba.render_surfels(view_camera=s["depth_camera"]["parameters"], width=w, height=h, global_T_frame=s["frame_poses"][kf["frame_index"]],
                                options=options)
        covered = out["index"] != rv.EMPTY_INDEX
        assert covered.sum() > 0.5 * w * h
        # the stated rule, in binary32: min(65534, (int)(depth / raw_to_float_depth + 0.5f)), 0 where no surfel is seen
        units = out["depth"] / np.float32(s["raw_to_float_depth"]) + np.float32(0.5)
        expected = np.where(covered, np.where(units >= np.float32(65534), 65534, np.trunc(units)), 0).astype(np.uint16)
        assert np.array_equal(np.frombuffer(pixels, ">u2").reshape(h, w), expected)
        assert expected[covered].min() > 0 and expected.max() < 65534
        assert np.array_equal(np.frombuffer(cpixels, np.uint8).reshape(h, w, 3), np.where(covered[..., None], out["color"][..., :3], 0))
    # point mode through the options, on the loaded state
    _run([BIN, str(tmp_path), "initial.txt", str(tmp_path / "again"), "--cell", "2", "--max_depth", "8", "--iterations", "0", "--load_state", state,
          "--render_dir", str(views), "--render_mode", "point"])
    kind, pw, ph, top, pixels = _read_pnm(str(views / "render_000000_depth.pgm"))
    point = ba.render_surfels(view_camera=s["depth_camera"]["parameters"], width=w, height=h, global_T_frame=s["frame_poses"][s["keyframes"][0]["frame_index"]],
                              options=capi.RenderOptions(mode=capi.RENDER_POINT))
    assert np.array_equal(np.frombuffer(pixels, ">u2").reshape(h, w) > 0, point["index"] != rv.EMPTY_INDEX)
