"""Rendered views of the surfel map on the GPU (bahip_render_surfels; kernels_render.hip, DESIGN.md section 3, "Rendered views of the
map") against the plain model of tests/render_view.py: all five planes -- key, depth, index, normal, colour -- BIT FOR BIT, no pixel
left out, on the scenes `tiny` and `crop_small` of tests/two_cameras.py in their perturbed state.  Every call's output planes are
filled with 0xFF bytes first: an entry the call did not write shows.  tests/test_cpu_render_view.py holds the model to the oracle and
shows that these scenes give it occlusions, box clipping, disc misses and back faces to decide."""
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll
from tests import render_view as rv
from tests import two_cameras as tcam

pytestmark = pytest.mark.gpu

_WORLD = {}
# waves, workgroups
SHAPES = [(1, 1), (8, 0), (4, 37), (2, 5), (1, 1000), (8, 1), (3, 2), (5, 7), (7, 0), (2, 100000)]


def _world(name):
    """(scene, an oracle nobody changes, its surfel rows, a GPU scene in the oracle's state that every test leaves as it found it)."""
    if name not in _WORLD:
        tc = tcam.build_scene(name)
        ba = tcam.build_oracle(tc)
        _WORLD[name] = (tc, ba, rv.oracle_surfels(ba), tcam.build_gpu(tc, ba))
    return _WORLD[name]


def _fresh(name="tiny"):
    """A GPU scene of its own in the scene's state (for the tests that upload other surfels or change the context)."""
    tc, ba, _, _ = _world(name)
    return tcam.build_gpu(tc, ba)


def _opt(**kw):
    return capi.RenderOptions(**kw)


def _render(g, cam, frame, opt=None, planes=None):
    view = ll.make_camera([cam.fx, cam.fy, cam.cx, cam.cy], cam.width, cam.height)
    return g.render_surfels(view, frame, opt, planes=planes, prefill=0xFF)


def _depth_cam(ba):
    return rv.camera(ba.depth_cam, 0, 0)


def _check(g, surfels, cam, frame, opt, what):
    expected = rv.render(surfels, cam, frame, opt)
    rv.assert_same_planes(_render(g, cam, frame, opt), expected, what)
    return expected


def _upload(g, data):
    g.upload_surfels(np.ascontiguousarray(data), np.ones(data.shape[1], np.uint8))


def _past_the_edge(ba):
    """Keyframe 1's frame turned by 25 degrees: part of the image looks past the cloud's edge."""
    return rv.turned_frame(rv.oracle_frame(ba, 1), 25.0)


# ---- model parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,radius", [(rv.POINT, 0), (rv.DISC, 1), (rv.DISC, 4), (rv.DISC, 16)])
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_planes_are_the_models_bits(name, mode, radius):
    tc, ba, surfels, g = _world(name)
    expected = _check(g, surfels, _depth_cam(ba), rv.oracle_frame(ba, 0), _opt(mode=mode, max_radius_px=radius), (name, mode, radius))
    covered = int(np.count_nonzero(expected["index"] != rv.EMPTY_INDEX))
    multi = int(np.count_nonzero(expected["stats"]["candidates"] > 1))
    print(name, mode, radius, "covered", covered, "multi-candidate", multi)
    assert covered >= 500 and multi >= 10


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_radius_factor_culling_and_a_depth_range_that_cuts_through_the_scene(name):
    tc, ba, surfels, g = _world(name)
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    depth = rv.render(surfels, cam, frame, _opt())["depth"]
    lo, hi = np.quantile(depth[depth > 0], [0.3, 0.7])
    assert lo < hi
    for factor in (1.0, 1.5):
        for cull in (1, 0):
            for limits in ((0.0, float("inf")), (float(lo), float(hi))):
                opt = _opt(radius_factor=factor, cull_backfaces=cull, min_depth=limits[0], max_depth=limits[1])
                expected = _check(g, surfels, cam, frame, opt, (name, factor, cull, limits))
                seen = expected["depth"][expected["depth"] > 0]
                assert seen.size > 100 and seen.min() >= np.float32(limits[0]) and seen.max() <= np.float32(limits[1])
    cut = rv.render(surfels, cam, frame, _opt(min_depth=float(lo), max_depth=float(hi)))
    assert np.count_nonzero(cut["depth"] > 0) < np.count_nonzero(depth > 0)              # the range removed something


@pytest.mark.parametrize("mode", [rv.POINT, rv.DISC])
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_a_keyframe_pose_and_a_pose_that_looks_past_the_clouds_edge(name, mode):
    tc, ba, surfels, g = _world(name)
    cam = _depth_cam(ba)
    for what, frame in (("keyframe 2", rv.oracle_frame(ba, 2)), ("past the edge", _past_the_edge(ba)), ("from behind", rv.turned_frame(rv.oracle_frame(ba, 0), 180.0, (0, 0, 5.0)))):
        for cull in (1, 0):
            expected = _check(g, surfels, cam, frame, _opt(mode=mode, cull_backfaces=cull), (name, what, mode, cull))
            covered = expected["index"] != rv.EMPTY_INDEX
            print(name, what, mode, cull, "covered", int(covered.sum()), {k: v for k, v in expected["stats"].items() if isinstance(v, int)})
            edge = cam.width // 8
            if what == "past the edge":
                assert covered.any() and (not covered[:, :edge].any() or not covered[:, -edge:].any()), (name, what)
            if what == "from behind":
                assert covered.any() == (cull == 0), (name, what, cull)


# ---- view shapes --------------------------------------------------------------------------------------------------------------------------
def test_a_view_camera_that_is_not_the_depth_camera():
    tc, ba, surfels, g = _world("tiny")
    cam = rv.camera(tc.color_camera, tc.color_width, tc.color_height)
    assert (cam.width, cam.height) == (53, 38)
    for mode in (rv.POINT, rv.DISC):
        expected = _check(g, surfels, cam, rv.oracle_frame(ba, 0), _opt(mode=mode), ("colour camera", mode))
        assert np.count_nonzero(expected["index"] != rv.EMPTY_INDEX) > 300


@pytest.mark.parametrize("width,height", [(1, 1), (7, 5), (65, 3)])
def test_small_and_odd_views(width, height):
    tc, ba, surfels, g = _world("tiny")
    cam = rv.scaled_camera(_depth_cam(ba), width, height)
    for mode, radius in ((rv.POINT, 0), (rv.DISC, 4), (rv.DISC, 16)):
        expected = _check(g, surfels, cam, rv.oracle_frame(ba, 0), _opt(mode=mode, max_radius_px=radius), (width, height, mode, radius))
        print(width, height, mode, radius, "covered", int(np.count_nonzero(expected["index"] != rv.EMPTY_INDEX)), "most candidates", int(expected["stats"]["candidates"].max()))
        if mode == rv.POINT:                       # many surfels meet in these few pixels (a disc rarely holds a pixel centre of such a view)
            assert expected["stats"]["candidates"].max() > 4 and np.count_nonzero(expected["index"] != rv.EMPTY_INDEX) >= 1


# ---- surfel buffer shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1142])
def test_the_first_n_surfels(n):
    tc, ba, surfels, _ = _world("tiny")
    assert surfels.shape[1] == 1142
    g = _fresh()
    _upload(g, surfels[:, :n])
    for mode in (rv.POINT, rv.DISC):
        expected = _check(g, surfels[:, :n], _depth_cam(ba), rv.oracle_frame(ba, 0), _opt(mode=mode), (n, mode))
        if n == 0:
            assert np.all(expected["key"] == rv.EMPTY_KEY) and np.all(expected["depth"].view(np.uint32) == 0)
            assert np.all(expected["index"] == rv.EMPTY_INDEX) and not expected["normal"].any() and not expected["color"].any()


def test_deleted_surfels_degenerate_radii_and_a_surfel_behind_the_camera():
    tc, ba, surfels, _ = _world("tiny")
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    whole = rv.render(surfels, cam, frame, _opt())
    winners = np.unique(whole["index"][whole["index"] != rv.EMPTY_INDEX]).astype(np.int64)
    data = surfels.copy()
    gone = np.zeros(data.shape[1], bool)
    gone[winners[3::9]] = True                        # deleted surfels (NaN x) spread through the tiles, all of them winners somewhere
    gone[192:256] = True                              # and tile 3 as a whole
    data[0, gone] = np.nan
    data[1, winners[1]] = np.inf                      # a non-finite y
    for victim, value in zip(winners[[2, 40, 80]], (0.0, np.nan, np.inf)):
        assert not gone[victim]
        data[4, victim] = value                       # r^2 = 0, NaN, +inf
    behind = int(winners[100])
    R = frame.reshape(3, 4)[:, :3].astype(np.float64)
    data[:3, behind] -= (2.0 * whole["depth"].max() * R[2]).astype(np.float32)      # moved back along the view axis: local.z < 0
    assert len({int(winners[1]), int(winners[2]), int(winners[40]), int(winners[80]), behind}) == 5 and not gone[behind]
    g = _fresh()
    _upload(g, data)
    for mode in (rv.POINT, rv.DISC):
        for cull in (1, 0):
            expected = _check(g, data, cam, frame, _opt(mode=mode, cull_backfaces=cull), ("degenerate", mode, cull))
            seen = set(np.unique(expected["index"]).tolist())
            assert not seen & set(np.flatnonzero(gone).tolist()) and behind not in seen and int(winners[1]) not in seen
            if mode == rv.DISC:                       # (point mode never reads r^2)
                assert not seen & {int(winners[2]), int(winners[40]), int(winners[80])}


# ---- NULL planes --------------------------------------------------------------------------------------------------------------------------
def test_every_plane_may_be_null():
    tc, ba, surfels, g = _world("tiny")
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    expected = rv.render(surfels, cam, frame, _opt())
    for missing in rv.PLANES:
        wanted = [name for name in rv.PLANES if name != missing]
        got = _render(g, cam, frame, _opt(), planes=wanted)
        assert sorted(got) == sorted(wanted)
        rv.assert_same_planes(got, expected, ("without", missing))
    rv.assert_same_planes(_render(g, cam, frame, _opt(), planes=["key"]), expected, "key alone")
    depth, index = ll.split_render_key(expected["key"])
    assert np.array_equal(depth.view(np.uint32), expected["depth"].view(np.uint32)) and np.array_equal(index, expected["index"])
    rv.assert_same_planes(_render(g, cam, frame, _opt()), expected, "all planes again")


# ---- invariance ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_same_bits_for_ten_launch_shapes_and_from_consecutive_calls(name):
    tc, ba, surfels, g = _world(name)
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    lib = capi.load()
    for opt in (_opt(mode=rv.POINT), _opt(max_radius_px=16)):
        expected = rv.render(surfels, cam, frame, opt)
        rv.assert_same_planes(_render(g, cam, frame, opt), expected, "first call")
        rv.assert_same_planes(_render(g, cam, frame, opt), expected, "second call")
        try:
            for waves, workgroups in SHAPES:
                capi.check(lib.bahip_debug_set_render_shape(waves, workgroups))
                rv.assert_same_planes(_render(g, cam, frame, opt), expected, (waves, workgroups))
        finally:
            capi.check(lib.bahip_debug_set_render_shape(0, 0))
    with pytest.raises(capi.BackendError, match="bahip_debug_set_render_shape"):
        capi.check(lib.bahip_debug_set_render_shape(9, 0))


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_a_surfel_permutation_keeps_the_depth_and_permutes_the_index(name):
    tc, ba, surfels, _ = _world(name)
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    g = _fresh(name)
    n = surfels.shape[1]
    perm = np.random.Generator(np.random.PCG64(8)).permutation(n)           # new position j holds old surfel perm[j]
    _upload(g, surfels[:, perm])
    old_to_new = np.empty(n, np.int64)
    old_to_new[perm] = np.arange(n)
    for opt in (_opt(mode=rv.POINT), _opt()):
        ref = rv.render(surfels, cam, frame, opt)
        got = _render(g, cam, frame, opt)
        rv.assert_same_planes(got, rv.render(surfels[:, perm], cam, frame, opt), "the permuted cloud's own model")
        assert np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32))
        decided = (ref["index"] != rv.EMPTY_INDEX) & ~ref["stats"]["tie"]
        assert decided.sum() > 500
        assert np.array_equal(got["index"][decided], old_to_new[ref["index"][decided]].astype(np.uint32))
        assert np.array_equal(got["index"] == rv.EMPTY_INDEX, ref["index"] == rv.EMPTY_INDEX)
        print(name, opt.mode, "ties", int(ref["stats"]["tie"].sum()))


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_minimum_of_two_shards_key_planes_is_the_whole_render(name):
    tc, ba, surfels, _ = _world(name)
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    n = surfels.shape[1]
    half = n // 2
    g = _fresh(name)
    for mode in (rv.POINT, rv.DISC):
        whole = rv.render(surfels, cam, frame, _opt(mode=mode))
        keys = []
        for begin, end in ((0, half), (half, n)):
            _upload(g, surfels[:, begin:end])
            part = _render(g, cam, frame, _opt(mode=mode, index_base=begin))
            rv.assert_same_planes(part, rv.render(surfels[:, begin:end], cam, frame, _opt(mode=mode, index_base=begin)), (mode, begin))
            keys.append(part["key"])
        assert np.array_equal(np.minimum(keys[0], keys[1]), whole["key"])
        depth, index = ll.split_render_key(np.minimum(keys[0], keys[1]))
        assert np.array_equal(depth.view(np.uint32), whole["depth"].view(np.uint32)) and np.array_equal(index, whole["index"])


# ---- refused calls ------------------------------------------------------------------------------------------------------------------------
def test_an_index_base_that_would_overflow_fails_with_an_error_string():
    tc, ba, surfels, g = _world("tiny")
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    n = surfels.shape[1]
    with pytest.raises(capi.BackendError, match="index_base"):
        _render(g, cam, frame, _opt(index_base=0xFFFFFFFF - n))
    top = 0xFFFFFFFF - n - 1                                                     # the largest base that fits
    expected = _check(g, surfels, cam, frame, _opt(index_base=top), "the largest index_base")
    assert int(expected["index"][expected["index"] != rv.EMPTY_INDEX].max()) <= 0xFFFFFFFE


def test_every_rejected_option_fails_with_an_error_string_and_leaves_the_context_usable():
    tc, ba, surfels, g = _world("tiny")
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    expected = rv.render(surfels, cam, frame, _opt())

    def sized(width, height):
        return rv.camera([cam.fx, cam.fy, cam.cx, cam.cy], width, height)
    bad = [("width", sized(0, 45), _opt()), ("height", sized(70, 0), _opt()), ("width", sized(-3, 45), _opt()),
           ("2\\^26", sized(1 << 13, (1 << 13) + 1), _opt()),
           ("max_radius_px", cam, _opt(max_radius_px=-1)), ("max_radius_px", cam, _opt(max_radius_px=17)),
           ("radius_factor", cam, _opt(radius_factor=0.0)), ("radius_factor", cam, _opt(radius_factor=-1.0)),
           ("radius_factor", cam, _opt(radius_factor=float("nan"))), ("min_depth > max_depth", cam, _opt(min_depth=2.0, max_depth=1.0)),
           ("mode", cam, _opt(mode=2))]
    for pattern, view, opt in bad:
        with pytest.raises(capi.BackendError, match=pattern):
            _render(g, view, frame, opt, planes=["key"] if view is not cam else None)
        rv.assert_same_planes(_render(g, cam, frame, _opt()), expected, ("after the refused call", pattern))


# ---- the fast flavour, allocations ----------------------------------------------------------------------------------------------------------
def test_the_fast_flavour_renders_the_exact_flavours_planes():
    tc, ba, surfels, _ = _world("crop_small")
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    g = _fresh("crop_small")
    g.ctx.set_arithmetic("fast")
    try:
        assert g.ctx.arithmetic == "fast"
        for opt in (_opt(mode=rv.POINT), _opt(max_radius_px=16, radius_factor=1.5)):
            _check(g, surfels, cam, frame, opt, ("fast", opt.mode))
    finally:
        g.ctx.set_arithmetic("exact")


def test_a_destroyed_context_gives_back_the_key_plane():
    tc, ba, surfels, _ = _world("tiny")
    gc.collect()
    base = ll.live_allocations()
    g = _fresh()
    before = ll.live_allocations()
    cam, frame = _depth_cam(ba), rv.oracle_frame(ba, 0)
    _check(g, surfels, cam, frame, _opt(), "small view")
    small = ll.live_allocations()
    assert small[0] == before[0] + 1 and small[1] == before[1] + 8 * cam.width * cam.height      # the key plane, and nothing else
    _check(g, surfels, rv.scaled_camera(cam, 2 * cam.width, 2 * cam.height), frame, _opt(), "a larger view: the plane is replaced")
    grown = ll.live_allocations()
    assert grown[0] == small[0] and grown[1] == before[1] + 32 * cam.width * cam.height
    _check(g, surfels, cam, frame, _opt(), "the small view in the grown plane")
    assert ll.live_allocations() == grown
    g.ctx.close()
    assert ll.live_allocations() == base
