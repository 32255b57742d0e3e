"""Residual images on the GPU (bahip_frame_residual_image; kernels_residual_image.hip, DESIGN.md section 3, "Residual images") against the
plain model of tests/residual_image.py -- the oracle's per-pair words grouped by pixel: all seven planes BIT FOR BIT, no pixel left
out, on the scenes `tiny` and `crop_small` of tests/two_cameras.py in their perturbed state, every keyframe, both selects.  Every
call's output planes are filled with 0xA5 bytes first: an entry the call did not write shows (0xFF bytes would hide an unwritten empty
pixel).  tests/test_cpu_residual_image.py shows that these scenes have pixels with several pairs, winners that are not the lowest
index, colour-invalid winners and no ties."""
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll
from tests import render_view as rv
from tests import residual_image as ri
from tests import two_cameras as tcam

pytestmark = pytest.mark.gpu

_WORLD = {}
_SCRATCH = {}
SELECTS = (ri.BEST, ri.WORST)
FILL = 0xA5


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


def _pairs(name, data, k, frame=None):
    """The oracle's pair words of the surfel rows `data` against keyframe k of the scene (a second oracle whose surfels are replaced)."""
    if name not in _SCRATCH:
        _SCRATCH[name] = tcam.build_oracle(tcam.build_scene(name))
    ba = _SCRATCH[name]
    n = data.shape[1]
    ba.surfel_data[:data.shape[0], :n] = data
    ba.surfels.surfels_size = n
    return ri.from_oracle(ba, k, frame)


def _size(ba):
    return int(ba.depth_cam.width), int(ba.depth_cam.height)


def _model(name, data, k, frame=None, select=ri.BEST, index_base=0):
    w, h = _size(_world(name)[1])
    return ri.image(_pairs(name, data, k, frame), w, h, select, index_base)


def _image(g, k, frame, select=ri.BEST, index_base=0, planes=None, size=None):
    return g.residual_image(k, frame, select=select, index_base=index_base, planes=planes, prefill=FILL, size=size)


def _upload(g, data, active=None):
    g.upload_surfels(np.ascontiguousarray(data), np.ones(data.shape[1], np.uint8) if active is None else active)


def _displaced(ba, k):
    """Keyframe k's frame turned by 0.2 degrees and shifted by 3 mm: not the keyframe's own pose, near enough to associate."""
    return rv.turned_frame(rv.oracle_frame(ba, k), 0.2, (0.003, -0.002, 0.001))


# ---- model parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_planes_are_the_models_bits_on_every_keyframe_under_both_selects(name):
    tc, ba, surfels, g = _world(name)
    for k in range(len(ba.keyframes)):
        frame = rv.oracle_frame(ba, k)
        pairs = _pairs(name, surfels, k)
        for select in SELECTS:
            expected = ri.image(pairs, *_size(ba), select)
            ri.assert_same_bits(_image(g, k, frame, select), expected, (name, k, select))
            print(name, "keyframe", k, "select", select, expected["stats"])
            assert expected["stats"]["explained"] >= 500 and expected["stats"]["multi"] >= 5
    # best and worst differ exactly where a pixel has pairs of different magnitude
    best, worst = _image(g, 1, rv.oracle_frame(ba, 1), ri.BEST), _image(g, 1, rv.oracle_frame(ba, 1), ri.WORST)
    assert np.array_equal(best["pairs"], worst["pairs"])
    assert np.array_equal(best["index"] != worst["index"], best["pairs"] > 1)             # (no ties on these scenes)


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_a_displaced_pose(name):
    tc, ba, surfels, g = _world(name)
    for k in (0, 2):
        frame = _displaced(ba, k)
        own = _model(name, surfels, k)
        for select in SELECTS:
            expected = _model(name, surfels, k, frame, select)
            ri.assert_same_bits(_image(g, k, frame, select), expected, (name, k, select))
            assert expected["stats"]["pairs"] >= 300
        assert not np.array_equal(expected["pairs"], own["pairs"])


# ---- against the library's own calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_winners_words_are_the_per_pair_hooks(name):
    tc, ba, surfels, g = _world(name)
    for k, frame in ((1, rv.oracle_frame(ba, 1)), (3, _displaced(ba, 3))):
        for select in SELECTS:
            img = _image(g, k, frame, select, index_base=1000)
            ys, xs = np.nonzero(img["index"] != ri.EMPTY_INDEX)
            assert ys.size >= 500
            words = g.evaluate_pairs(k, img["index"][ys, xs] - np.uint32(1000), frame)
            u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731
            assert np.all(words[:, 0] == 1) and np.array_equal(words[:, 1], xs.astype(np.float32)) and np.array_equal(words[:, 2], ys.astype(np.float32))
            assert np.array_equal(words[:, 3], img["color_valid"][ys, xs].astype(np.float32))
            assert np.array_equal(u(words[:, 5]), u(img["depth_residual"][ys, xs])) and np.array_equal(u(words[:, 7]), u(img["inv_stddev"][ys, xs]))
            assert np.array_equal(u(words[:, 14:16]), u(img["desc_residual"][ys, xs]))       # the hook leaves +0.0 where the colour pixel is invalid
            assert np.count_nonzero(words[:, 3] == 0) >= 20


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_pairs_sum_to_the_frame_costs_depth_residuals(name):
    tc, ba, surfels, g = _world(name)
    for k, frame in ((0, rv.oracle_frame(ba, 0)), (2, _displaced(ba, 2))):
        cost = g.evaluate_frame_cost(k, frame, use_depth=True, use_desc=False)
        pairs = _image(g, k, frame, planes=["pairs"])["pairs"]
        assert int(pairs.sum(dtype=np.int64)) == cost["depth_residuals"] and cost["depth_residuals"] >= 300


# ---- invariance ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_same_bits_for_nine_launch_shapes_and_from_consecutive_calls(name):
    tc, ba, surfels, g = _world(name)
    frame = rv.oracle_frame(ba, 1)
    lib = capi.load()
    for select in SELECTS:
        expected = _model(name, surfels, 1, select=select)
        ri.assert_same_bits(_image(g, 1, frame, select), expected, "first call")
        ri.assert_same_bits(_image(g, 1, frame, select), expected, "second call")
        try:
            for waves in (1, 2, 8):
                for workgroups in (1, 2, 100000):
                    capi.check(lib.bahip_debug_set_residual_image_shape(waves, workgroups))
                    ri.assert_same_bits(_image(g, 1, frame, select), expected, (waves, workgroups))
        finally:
            capi.check(lib.bahip_debug_set_residual_image_shape(0, 0))
    with pytest.raises(capi.BackendError, match="bahip_debug_set_residual_image_shape"):
        capi.check(lib.bahip_debug_set_residual_image_shape(9, 0))
    with pytest.raises(capi.BackendError, match="bahip_debug_set_residual_image_shape"):
        capi.check(lib.bahip_debug_set_residual_image_shape(1, -1))


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_a_surfel_permutation_permutes_the_index_and_nothing_else(name):
    tc, ba, surfels, _ = _world(name)
    frame = rv.oracle_frame(ba, 1)
    g = _fresh(name)
    n = surfels.shape[1]
    perm = np.random.Generator(np.random.PCG64(8)).permutation(n)           # new position j holds old surfel perm[j]
    _upload(g, surfels[:, perm])
    old_to_new = np.empty(n, np.int64)
    old_to_new[perm] = np.arange(n)
    for select in SELECTS:
        ref = _model(name, surfels, 1, select=select)
        assert ref["stats"]["ties"] == 0                                    # (tests/test_cpu_residual_image.py: none on these scenes)
        got = _image(g, 1, frame, select)
        covered = ref["index"] != ri.EMPTY_INDEX
        assert np.array_equal(got["index"] != ri.EMPTY_INDEX, covered)
        assert np.array_equal(got["index"][covered], old_to_new[ref["index"][covered]].astype(np.uint32))
        assert np.array_equal(got["key"] >> np.uint64(32), ref["key"] >> np.uint64(32))
        for plane in ("pairs", "depth_residual", "inv_stddev", "desc_residual", "color_valid"):
            ri.assert_same_bits({plane: got[plane]}, {plane: ref[plane]}, (select, plane))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1142])
def test_the_first_n_surfels(n):
    tc, ba, surfels, g = _world("tiny")
    assert surfels.shape[1] == 1142
    frame = rv.oracle_frame(ba, 1)
    for select in SELECTS:
        expected = _model("tiny", surfels[:, :n], 1, select=select)
        ri.assert_same_bits(_image(g, 1, frame, select, size=n), expected, (n, select))
        if n == 0:
            assert np.all(expected["key"] == ri.EMPTY_KEY) and not expected["pairs"].any() and np.all(expected["index"] == ri.EMPTY_INDEX)
            assert not any(np.ascontiguousarray(expected[p]).view(np.uint32).any() for p in ri.FLOAT_PLANES)
        else:
            assert int(expected["index"][expected["index"] != ri.EMPTY_INDEX].max(initial=0)) < n


def test_deleted_surfels_never_win_and_are_not_counted():
    tc, ba, surfels, _ = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    whole = _model("tiny", surfels, 1)
    winners = np.unique(whole["index"][whole["index"] != ri.EMPTY_INDEX]).astype(np.int64)
    data = surfels.copy()
    gone = np.zeros(data.shape[1], bool)
    gone[winners[3::9]] = True                        # deleted surfels (NaN x) spread through the tiles, all of them winners somewhere
    gone[192:256] = True                              # and tile 3 as a whole
    data[0, gone] = np.nan
    g = _fresh()
    _upload(g, data)
    for select in SELECTS:
        expected = _model("tiny", data, 1, select=select)
        got = _image(g, 1, frame, select)
        ri.assert_same_bits(got, expected, ("deleted", select))
        assert not set(np.unique(got["index"]).tolist()) & set(np.flatnonzero(gone).tolist())
        pairs = _pairs("tiny", surfels, 1)
        assert int(got["pairs"].sum()) == int(np.count_nonzero(pairs["associated"] & ~gone)) < int(whole["pairs"].sum())


def test_activation_flags_change_nothing():
    tc, ba, surfels, _ = _world("tiny")
    frame = rv.oracle_frame(ba, 2)
    g = _fresh()
    n = surfels.shape[1]
    expected = _model("tiny", surfels, 2)
    for active in (np.zeros(n, np.uint8), np.ones(n, np.uint8), (np.arange(n) % 3 == 0).astype(np.uint8)):
        _upload(g, surfels, active)
        ri.assert_same_bits(_image(g, 2, frame), expected, int(active.sum()))


# ---- ties and NaN -------------------------------------------------------------------------------------------------------------------------
def test_an_exact_copy_raises_the_count_and_loses_to_the_lower_index():
    tc, ba, surfels, _ = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    whole = _model("tiny", surfels, 1)
    ys, xs = np.nonzero(whole["pairs"] == 1)
    y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
    original = int(whole["index"][y, x])
    n = surfels.shape[1]
    data = np.concatenate([surfels, surfels[:, original:original + 1]], axis=1)
    g = _fresh()
    _upload(g, data)
    for select in SELECTS:
        expected = _model("tiny", data, 1, select=select)
        got = _image(g, 1, frame, select)
        ri.assert_same_bits(got, expected, ("copy", select))
        assert got["pairs"][y, x] == 2 and got["index"][y, x] == original and n not in got["index"]
        assert expected["stats"]["ties"] == 1
        delta = got["pairs"].astype(np.int64) - whole["pairs"].astype(np.int64)
        assert delta[y, x] == 1 and np.count_nonzero(delta) == 1
    # the copy first: the copy wins, with the same words
    _upload(g, np.concatenate([surfels[:, original:original + 1], surfels], axis=1))
    for select in SELECTS:
        got = _image(g, 1, frame, select)
        assert got["pairs"][y, x] == 2 and got["index"][y, x] == 0
        assert got["depth_residual"][y, x].view(np.uint32) == whole["depth_residual"][y, x].view(np.uint32)


def test_a_nan_descriptor_gives_nan_descriptor_residuals_and_leaves_the_depth_planes():
    tc, ba, surfels, _ = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    whole = _model("tiny", surfels, 1)
    ys, xs = np.nonzero(whole["color_valid"] == 1)
    y, x = int(ys[len(ys) // 3]), int(xs[len(xs) // 3])
    victim = int(whole["index"][y, x])
    data = surfels.copy()
    data[6, victim] = np.nan
    g = _fresh()
    _upload(g, data)
    got = _image(g, 1, frame)
    ri.assert_same_bits(got, _model("tiny", data, 1), "NaN descriptor")
    assert np.isnan(got["desc_residual"][y, x, 0]) and np.isfinite(got["desc_residual"][y, x, 1]) and got["color_valid"][y, x] == 1
    for plane in ("key", "pairs", "index", "depth_residual", "inv_stddev", "color_valid"):
        ri.assert_same_bits({plane: got[plane]}, {plane: whole[plane]}, plane)
    assert int(np.isnan(got["desc_residual"]).sum()) == int(np.count_nonzero(whole["index"] == victim))


# ---- planes -------------------------------------------------------------------------------------------------------------------------------
def test_any_plane_may_be_null_and_every_given_plane_is_overwritten():
    tc, ba, surfels, g = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    for select in SELECTS:
        expected = _model("tiny", surfels, 1, select=select)
        for missing in ri.PLANES:
            wanted = [name for name in ri.PLANES if name != missing]
            got = _image(g, 1, frame, select, planes=wanted)
            assert sorted(got) == sorted(wanted)
            ri.assert_same_bits(got, expected, ("without", missing))
        for wanted in (["key"], ["pairs"], ["index"], ["depth_residual"], ["desc_residual"], ["color_valid"], ["inv_stddev", "color_valid"],
                       ["key", "depth_residual"], ["pairs", "desc_residual"]):
            ri.assert_same_bits(_image(g, 1, frame, select, planes=wanted), expected, wanted)
        magnitude, index = ll.split_residual_key(expected["key"], select)
        assert np.array_equal(index, expected["index"])
        assert np.array_equal(magnitude.view(np.uint32), np.abs(expected["depth_residual"]).view(np.uint32))
        ri.assert_same_bits(_image(g, 1, frame, select), expected, "all planes again")
    assert _image(g, 1, frame, planes=[]) == {}                                # nothing asked for: the call still succeeds


# ---- refused calls ------------------------------------------------------------------------------------------------------------------------
def _untouched(planes):
    return planes and all(np.all(np.ascontiguousarray(p).view(np.uint8) == FILL) for p in planes.values())


def test_refused_calls_write_nothing_and_leave_the_context_usable():
    tc, ba, surfels, g = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    expected = _model("tiny", surfels, 1)
    n = surfels.shape[1]
    for pattern, kw in (("select", dict(select=2)), ("select", dict(select=-1)), ("index_base", dict(index_base=0xFFFFFFFF - n)),
                        ("index_base", dict(index_base=0xFFFFFFFF))):
        with pytest.raises(capi.BackendError, match=pattern) as refused:
            _image(g, 1, frame, **kw)
        assert _untouched(refused.value.planes), pattern
        ri.assert_same_bits(_image(g, 1, frame), expected, ("after the refused call", pattern))
    w, h = _size(ba)
    with pytest.raises(capi.BackendError, match="bad arguments") as refused:
        ll.frame_residual_image(g.ctx, None, frame, g.surfels_struct(), w, h, prefill=FILL)
    assert _untouched(refused.value.planes)
    top = 0xFFFFFFFF - n - 1                                                    # the largest base that fits
    at_top = _model("tiny", surfels, 1, index_base=top)
    ri.assert_same_bits(_image(g, 1, frame, index_base=top), at_top, "the largest index_base")
    assert int(at_top["index"][at_top["index"] != ri.EMPTY_INDEX].max()) <= 0xFFFFFFFE


def test_a_context_without_intrinsics_refuses():
    tc, ba, surfels, g = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    bare = ll.Context()
    try:
        with pytest.raises(capi.BackendError, match="bahip_set_intrinsics") as refused:
            ll.frame_residual_image(bare, g.frame_struct(1), frame, g.surfels_struct(), *_size(ba), prefill=FILL)
        assert _untouched(refused.value.planes)
    finally:
        bare.close()
    ri.assert_same_bits(_image(g, 1, frame), _model("tiny", surfels, 1), "the scene's own context afterwards")


# ---- shards, the fast flavour, allocations ------------------------------------------------------------------------------------------------
def test_two_shards_composite_to_the_unsharded_planes():
    tc, ba, surfels, _ = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    n = surfels.shape[1]
    cut = 500                                          # not a multiple of 64
    g = _fresh()
    for select in SELECTS:
        whole = _model("tiny", surfels, 1, select=select, index_base=7)
        parts = []
        for begin, end in ((0, cut), (cut, n)):
            _upload(g, surfels[:, begin:end])
            part = _image(g, 1, frame, select, index_base=7 + begin)
            ri.assert_same_bits(part, _model("tiny", surfels[:, begin:end], 1, select=select, index_base=7 + begin), (select, begin))
            parts.append(part)
        ri.assert_same_bits(ri.composite(parts), whole, ("composited", select))
        assert np.count_nonzero((parts[0]["pairs"] > 0) & (parts[1]["pairs"] > 0)) >= 1          # pixels both shards explain


def test_the_fast_flavour_gives_the_exact_flavours_planes():
    tc, ba, surfels, _ = _world("crop_small")
    g = _fresh("crop_small")
    g.ctx.set_arithmetic("fast")
    try:
        assert g.ctx.arithmetic == "fast"
        for select in SELECTS:
            ri.assert_same_bits(_image(g, 1, rv.oracle_frame(ba, 1), select), _model("crop_small", surfels, 1, select=select), ("fast", select))
    finally:
        g.ctx.set_arithmetic("exact")


def test_repeated_calls_allocate_nothing_and_a_destroyed_context_gives_everything_back():
    tc, ba, surfels, _ = _world("tiny")
    frame = rv.oracle_frame(ba, 1)
    gc.collect()
    base = ll.live_allocations()
    g = _fresh()
    _image(g, 1, frame)                                # all planes given: the frame's packed planes are the only thing the context needs
    _image(g, 1, frame, planes=["index"])              # key and pairs are the context's own now
    held = ll.live_allocations()
    w, h = _size(ba)
    assert held[1] >= base[1] + 12 * w * h
    for _ in range(3):
        for select in SELECTS:
            _image(g, 1, frame, select)
            _image(g, 2, frame, select, planes=["index", "desc_residual"])
            _image(g, 0, frame, select, planes=["key", "depth_residual"])
    assert ll.live_allocations() == held
    g.ctx.close()
    assert ll.live_allocations() == base
