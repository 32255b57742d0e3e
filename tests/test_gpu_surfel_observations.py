"""Observation lists on the GPU (bahip_surfel_observations; kernels_observations.hip): surfel_first, keyframes,
depth_raw and descriptor_raw against the model of tests/surfel_observations.py -- the oracle's `associated` flags in compressed rows and
the oracle's pair words -- on the scenes and worlds whose census tests/test_cpu_surfel_observations.py asserts.  Every comparison is an
equality; the payload planes are compared as bit patterns.  Launch shape, tile order, fill form, staging window, surfel order within
what the definition allows, sharding and the arithmetic flavour must not move a word."""
import ctypes as C
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll, synthetic
from oracle import binding as ob
from tests import observed_covisibility as oc
from tests import surfel_observations as so
from tests import tile_cull
from tests import two_cameras

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL_WORDS = {"surfel_first": 0xA5A5A5A5, "keyframes": 0xA5A5, "depth_raw": 0xA5A5A5A5, "descriptor_raw": 0xA5A5A5A5}
DIRECT, STAGED = -1, -2            # stage_entries of bahip_debug_set_observations_shape: the two fill forms (staged: the default window)
FORMS = (DIRECT, STAGED)
_CACHE = {}


def _shape(waves=0, workgroups=0, stage_entries=0, tile_order=-1, pair_limit=0):
    capi.check(capi.load().bahip_debug_set_observations_shape(waves, workgroups, stage_entries, tile_order, pair_limit))


def _scene(name):
    """(oracle, A, table, a GPU scene in the oracle's state that every test leaves as it found it) of a scene of tests/two_cameras.py."""
    if name not in _CACHE:
        tc, ba, A, t = so.scene(name)
        _CACHE[name] = (ba, A, t, two_cameras.build_gpu(tc, ba))
    return _CACHE[name]


def _world(name):
    if name not in _CACHE:
        w, ba, A, t = so.world(name)
        _CACHE[name] = (ba, A, t, tile_cull.build_gpu(w, ba))
    return _CACHE[name]


def _untouched(plane, name, start=0):
    return (so.words(plane[start:]) == FILL_WORDS[name]).all() if name != "keyframes" else (plane[start:] == FILL_WORDS[name]).all()


def _check(g, t, what, **kw):
    """One call with every plane prefilled and 37 entries of room to spare: the model's words, and nothing beyond them."""
    got = g.surfel_observations(capacity=t["pairs"] + 37, prefill=FILL, **kw)
    so.assert_same(got, t, what)
    for name in ("keyframes", "depth_raw", "descriptor_raw"):
        if name in got:
            assert len(got[name]) == t["pairs"] + 37 and _untouched(got[name], name, t["pairs"]), (what, name)
    return got


def _both_forms(g, t, what):
    try:
        for form in FORMS:
            _shape(stage_entries=form)
            got = _check(g, t, (what, form))
    finally:
        _shape()
    return got


def _cross_checks(g, ba, got, K):
    """The same table through the library's other reductions, on the same state."""
    P = got["pairs"]
    first, ks = got["surfel_first"], got["keyframes"][:P]
    assert np.array_equal(so.lengths(first), g.evaluate_surfel_costs(True, False, planes=["depth_residuals"])["depth_residuals"])
    _, per = g.evaluate_cost(True, False)
    assert np.bincount(ks, minlength=K).tolist() == [c["depth_residuals"] for c in per]
    A = so.dense(first, ks, K)
    assert np.array_equal(oc.matrix(A), g.observed_covisibility().astype(np.int64))
    # depth_raw of sampled pairs: the raw word of the per-pair hook
    surfel_of = np.repeat(np.arange(len(first) - 1), so.lengths(first))
    sample = np.random.Generator(np.random.PCG64(3)).choice(P, size=min(P, 400), replace=False)
    for k in range(K):
        mine = sample[ks[sample] == k]
        if not len(mine):
            continue
        words = g.evaluate_pairs(k, surfel_of[mine].astype(np.uint32), list(ba.keyframes[k].frame_T_global))
        assert (words[:, 0] == 1).all()
        assert np.array_equal(np.ascontiguousarray(words[:, 5]).view(np.uint32), so.words(got["depth_raw"][mine])), k


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_table_is_the_model_on_the_scenes(name):
    ba, A, t, g = _scene(name)
    got = _both_forms(g, t, name)
    assert (so.words(got["descriptor_raw"][:t["pairs"]]) == so.NAN_WORD).any()          # pairs whose colour pixel is not valid
    _cross_checks(g, ba, got, A.shape[0])


@pytest.mark.parametrize("name", ["centred", "neg_fy", "off_image"])
def test_the_table_is_the_model_on_the_edge_worlds(name):
    ba, A, t, g = _world(name)
    got = _both_forms(g, t, name)
    assert t["pairs"] > 1000 and (so.per_tile(t["surfel_first"]) == 0).any()
    _cross_checks(g, ba, got, A.shape[0])


def _seventy():
    """70 keyframes on tiny's cloud: the four images in turn at perturbed poses; oracle and GPU scene in the same state."""
    if "seventy" not in _CACHE:
        tc, ba4, _, _ = so.scene("tiny")
        scene = tc.scene
        rng = np.random.Generator(np.random.PCG64(70))
        poses = [synthetic.perturb_pose(rng, tc.poses[k % 4]) for k in range(70)]
        color = lambda make: make(tc.color_camera, tc.color_width, tc.color_height)           # noqa: E731
        depth = lambda make: make(scene.camera, scene.width, scene.height)                    # noqa: E731
        ba = ob.OracleBA(tc.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, color(ob.make_camera), depth(ob.make_camera))
        g = ll.Scene(ll.Context(), tc.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, color(ll.make_camera), depth(ll.make_camera))
        for k, T in enumerate(poses):
            ba.add_keyframe(scene.depth[k % 4], scene.rgb[k % 4], T)
            g.add_keyframe(scene.depth[k % 4], scene.rgb[k % 4], T)
        n = ba4.surfels_size
        ba.surfel_data[:, :n] = ba4.surfel_data[:, :n]
        ba.surfels.surfels_size, ba.surfels.surfel_count = n, ba4.surfels.surfel_count
        ba.active[:n] = 1
        two_cameras.sync_gpu(g, ba)
        A = oc.associated_matrix(ba)
        _CACHE["seventy"] = (ba, A, so.table(ba, A), g)
    return _CACHE["seventy"]


def test_seventy_keyframes_cross_the_candidate_chunk_and_the_windows_many_times():
    ba, A, t, g = _seventy()
    lengths = so.lengths(t["surfel_first"])
    assert A.shape[0] == 70 and A[64:].any(axis=1).all() and lengths.max() > 64, lengths.max()
    assert so.per_tile(t["surfel_first"]).max() > 1024          # tiles larger than the default window as well
    reference = _both_forms(g, t, "70 keyframes")
    try:
        for window in (1, 2, 64):
            _shape(stage_entries=window)
            for residuals in ((), ("depth_raw", "descriptor_raw")):
                so.assert_same(g.surfel_observations(capacity=t["pairs"], prefill=FILL, residuals=residuals), t, ("70 keyframes", window, residuals))
    finally:
        _shape()
    assert np.array_equal(reference["keyframes"][:t["pairs"]], t["keyframes"])


LATE_FILLERS = 1032            # keyframes that look away, ahead of the world's eight (as tests/test_gpu_tile_cull.py places them)


def test_late_keyframes_behind_1032_that_look_away():
    w, ba, A, t = so.world("centred")
    poses = [w.poses[7]] * LATE_FILLERS + list(w.poses)
    images = [w.images[7]] * LATE_FILLERS + list(w.images)
    n = 64 * 64 - 11                                        # a prefix of 64 tiles that ends inside one
    g = tile_cull.build_gpu(w, poses=poses, images=images, capacity=n + 64)
    g.set_intrinsics()
    g.upload_surfels(w.surfels[:, :n], np.ones(n, np.uint8))
    assert not A[7, :n].any() and A[:6, :n].any(axis=1).all()
    expected = so.take(t, 0, n)
    expected["keyframes"] = (expected["keyframes"].astype(np.uint32) + LATE_FILLERS).astype(np.uint16)      # the fillers are keyframe 7 again: no pair
    assert expected["pairs"] > 1000 and expected["keyframes"].min() >= 1024
    _both_forms(g, expected, "late keyframes")


def test_both_fill_forms_and_every_window_give_the_same_bytes():
    ba, A, t, g = _scene("tiny")
    assert so.per_tile(t["surfel_first"]).min() == 76          # every tile holds more pairs than the small windows
    planes = ("keyframes", "depth_raw", "descriptor_raw")
    _shape(stage_entries=DIRECT)
    try:
        reference = g.surfel_observations(capacity=t["pairs"] + 5, prefill=FILL)
        so.assert_same(reference, t, "direct")
        for window in (1, 2, 64, STAGED, 4096):
            for waves in (1, 8):
                _shape(waves=waves, stage_entries=window)
                got = g.surfel_observations(capacity=t["pairs"] + 5, prefill=FILL)
                for name in planes:
                    assert np.array_equal(so.words(got[name]), so.words(reference[name])), (window, waves, name)
                assert np.array_equal(got["surfel_first"], reference["surfel_first"])
        lib = capi.load()
        for bad in ((9, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, -3, 0, 0), (0, 0, 4097, 0, 0), (0, 0, 0, 2, 0)):
            assert lib.bahip_debug_set_observations_shape(*bad) != 0 and b"bahip_debug_set_observations_shape" in lib.bahip_last_error()
        for bad in (2, 4, 5, 6, 8, -1):
            assert lib.bahip_debug_set_observations_stages(bad) != 0 and b"bahip_debug_set_observations_stages" in lib.bahip_last_error()
    finally:
        _shape()


def test_launch_shapes_and_tile_orders_give_the_same_words():
    ba, A, t, g = _scene("crop_small")
    poses = [kf["pose"].copy() for kf in g.keyframes]
    g.estimate_keyframe_poses(True, True)                   # a pose phase over the table leaves the heavy-first run order behind
    for kf, T in zip(g.keyframes, poses):
        kf["pose"] = T
    g.bind_keyframes()
    try:
        for waves, workgroups in [(1, 1), (2, 7), (3, 0), (4, 1), (5, 7), (6, 100000), (7, 1), (8, 7), (8, 0), (1, 100000)]:
            for order in (0, 1):
                for form in (DIRECT, 100):                  # (a window of 100 entries: most tiles here hold more)
                    _shape(waves, workgroups, form, order)
                    so.assert_same(g.surfel_observations(capacity=t["pairs"], prefill=FILL), t, (waves, workgroups, order, form))
    finally:
        _shape()


@pytest.mark.parametrize("form", FORMS)
def test_prefixes_with_ragged_and_exactly_full_last_tiles(form):
    ba, A, t, g = _scene("tiny")
    n = A.shape[1]
    _shape(stage_entries=form)
    try:
        for size in (0, 1, 63, 64, 65, 128, n):
            got = g.surfel_observations(size=size, capacity=t["pairs"], prefill=FILL)
            expected = so.take(t, 0, size)
            so.assert_same(got, expected, size)
            assert len(got["surfel_first"]) == size + 1
            for name in ("keyframes", "depth_raw", "descriptor_raw"):
                assert _untouched(got[name], name, expected["pairs"]), (size, name)
    finally:
        _shape()


@pytest.mark.parametrize("form", FORMS)
def test_invariances_and_edge_clouds(request, form):
    ba, A, t, g = _scene("tiny")
    tc = so.scene("tiny")[0]
    request.addfinalizer(lambda: (_shape(), two_cameras.sync_gpu(g, ba)))
    _shape(stage_entries=form)
    data = g.download_surfels().copy()
    n = data.shape[1]
    # a surfel permutation: lists move with their surfels and nothing changes inside them
    perm = np.random.Generator(np.random.PCG64(5)).permutation(n)
    g.upload_surfels(np.ascontiguousarray(data[:, perm]), np.ones(n, np.uint8))
    so.assert_same(g.surfel_observations(prefill=FILL), so.permuted(t, perm), "permuted")
    # deleted surfels (NaN x), in runs and alone: empty lists, their neighbours' offsets right
    dead = np.zeros(n, bool)
    dead[[0, 5, 63, 64, 65, n - 1]] = True
    dead[192:331] = True                                    # two whole tiles and a part of the next
    killed = data.copy()
    killed[0, dead] = np.nan
    g.upload_surfels(killed, np.ones(n, np.uint8))
    expected = so.table(ba, A & ~dead[None, :])
    assert expected["pairs"] < t["pairs"] and (so.per_tile(expected["surfel_first"]) == 0).sum() == 2
    so.assert_same(g.surfel_observations(prefill=FILL), expected, "deleted")
    # every surfel deleted: an all-zero prefix
    killed[0, :] = np.nan
    g.upload_surfels(killed, np.ones(n, np.uint8))
    got = g.surfel_observations(capacity=9, prefill=FILL)
    assert got["pairs"] == 0 and not got["surfel_first"].any() and _untouched(got["keyframes"], "keyframes")
    # activation flags of surfels and keyframes cleared: nothing changes
    g.upload_surfels(data, np.zeros(n, np.uint8))
    for kf in g.keyframes:
        kf["activation"] = ob.KF_INACTIVE
    g.bind_keyframes()
    so.assert_same(g.surfel_observations(prefill=FILL), t, "flags cleared")
    # a keyframe permutation and a single bound keyframe: the rows of A the binding names
    keyframes = list(g.keyframes)
    try:
        order = [2, 0, 3, 1]
        g.keyframes = [keyframes[k] for k in order]
        g.bind_keyframes()
        so.assert_same(g.surfel_observations(prefill=FILL), so.table(ba, A[order], order), "keyframes permuted")
        g.keyframes = [keyframes[3]]
        g.bind_keyframes()
        so.assert_same(g.surfel_observations(prefill=FILL), so.table(ba, A[3:4], [3]), "one keyframe")
    finally:
        g.keyframes = keyframes
        g.bind_keyframes()


def test_the_protocol_of_counting_sizing_and_filling():
    ba, A, t, g = _scene("tiny")
    P = t["pairs"]
    names = ("keyframes", "depth_raw", "descriptor_raw")
    # a count-only call: surfel_first and P
    got = g.surfel_observations(capacity=0, prefill=FILL, keyframes=False, residuals=())
    assert got["pairs"] == P and np.array_equal(got["surfel_first"], t["surfel_first"]) and set(got) == {"pairs", "surfel_first"}
    # capacity = P fills the planes; the sizing call of the wrapper does the same
    so.assert_same(g.surfel_observations(capacity=P, prefill=FILL), t, "capacity P")
    so.assert_same(g.surfel_observations(prefill=FILL), t, "sized by a count-only call")
    for form in FORMS:
        _shape(stage_entries=form)
        try:
            # capacity = P - 1: not a byte of a plane is touched, surfel_first and P are right, the call succeeds
            got = g.surfel_observations(capacity=P - 1, prefill=FILL)
            assert got["pairs"] == P and np.array_equal(got["surfel_first"], t["surfel_first"])
            for name in names:
                assert len(got[name]) == P - 1 and _untouched(got[name], name), name
            # a larger plane: the words beyond P are untouched
            got = g.surfel_observations(capacity=P + 100, prefill=FILL)
            so.assert_same(got, t, "capacity P + 100")
            for name in names:
                assert len(got[name]) == P + 100 and _untouched(got[name], name, P), name
            # NULL payload planes in every combination
            for residuals in ((), ("depth_raw",), ("descriptor_raw",), ("depth_raw", "descriptor_raw")):
                got = g.surfel_observations(capacity=P, prefill=FILL, residuals=residuals)
                assert set(got) == {"pairs", "surfel_first", "keyframes"} | set(residuals)
                so.assert_same(got, t, residuals)
        finally:
            _shape()
    # a pair limit below P fails the call and writes no plane
    _shape(pair_limit=P - 1)
    try:
        with pytest.raises(capi.BackendError, match="pair limit") as refused:
            g.surfel_observations(capacity=P, prefill=FILL)
        for name in ("surfel_first",) + names:
            assert _untouched(refused.value.arrays[name], name), name
        _shape(pair_limit=P)
        so.assert_same(g.surfel_observations(capacity=P, prefill=FILL), t, "pair limit P")
    finally:
        _shape()
    so.assert_same(g.surfel_observations(capacity=P, prefill=FILL), t, "after the refusals")


def test_refusals_write_nothing_and_leave_the_context_usable():
    ba, A, t, g = _scene("tiny")
    lib = capi.load()
    P, n = t["pairs"], A.shape[1]
    first = ll.DeviceBuffer2D(g.ctx, 1, n + 1, np.uint32).clear(FILL)
    ks = ll.DeviceBuffer2D(g.ctx, 1, P, np.uint16).clear(FILL)
    depth = ll.DeviceBuffer2D(g.ctx, 1, P, np.float32).clear(FILL)
    s = g.surfels_struct()
    pairs = C.c_uint64(77)
    out = capi.Observations(first.ptr, ks.ptr, depth.ptr, None, P)

    def intact():
        g.ctx.synchronize()
        return (first.download() == 0xA5A5A5A5).all() and (ks.download() == 0xA5A5).all() and (depth.download().view(np.uint32) == 0xA5A5A5A5).all() \
            and pairs.value == 77

    no_first = capi.Observations(None, ks.ptr, depth.ptr, None, P)
    payload_only = capi.Observations(first.ptr, None, depth.ptr, None, P)
    for args in ((None, C.byref(s), C.byref(out), C.byref(pairs)), (g.ctx.handle, None, C.byref(out), C.byref(pairs)),
                 (g.ctx.handle, C.byref(s), None, C.byref(pairs)), (g.ctx.handle, C.byref(s), C.byref(out), None),
                 (g.ctx.handle, C.byref(s), C.byref(no_first), C.byref(pairs)), (g.ctx.handle, C.byref(s), C.byref(payload_only), C.byref(pairs))):
        assert lib.bahip_surfel_observations(*args) != 0
        assert b"bahip_surfel_observations" in lib.bahip_last_error()
        assert intact()
    with pytest.raises(capi.BackendError, match="without keyframes") as refused:
        g.surfel_observations(capacity=P, prefill=FILL, keyframes=False, residuals=("descriptor_raw",))
    assert _untouched(refused.value.arrays["surfel_first"], "surfel_first") and _untouched(refused.value.arrays["descriptor_raw"], "descriptor_raw")
    # keyframe sharding
    g.set_keyframe_sharding(0, 2)
    try:
        assert lib.bahip_surfel_observations(g.ctx.handle, C.byref(s), C.byref(out), C.byref(pairs)) != 0
        assert b"keyframe sharding" in lib.bahip_last_error() and intact()
    finally:
        g.set_keyframe_sharding(0, 1)
        g.bind_keyframes()
    # a context without intrinsics
    bare = ll.Context()
    assert lib.bahip_surfel_observations(bare.handle, C.byref(s), C.byref(out), C.byref(pairs)) != 0
    assert b"bahip_set_intrinsics" in lib.bahip_last_error()
    bare.synchronize()
    assert intact()
    bare.close()
    # no keyframe bound: an all-zero surfel_first and P = 0, no plane touched
    keyframes = g.keyframes
    g.keyframes = []
    g.bind_keyframes()
    try:
        capi.check(lib.bahip_surfel_observations(g.ctx.handle, C.byref(s), C.byref(out), C.byref(pairs)))
        assert pairs.value == 0 and not first.download().any()
        assert (ks.download() == 0xA5A5).all() and (depth.download().view(np.uint32) == 0xA5A5A5A5).all()
    finally:
        g.keyframes = keyframes
        g.bind_keyframes()
    # a good call follows
    capi.check(lib.bahip_surfel_observations(g.ctx.handle, C.byref(s), C.byref(out), C.byref(pairs)))
    assert pairs.value == P and np.array_equal(first.download()[0], t["surfel_first"]) and np.array_equal(ks.download()[0], t["keyframes"])
    assert np.array_equal(depth.download()[0].view(np.uint32), t["depth_raw"])
    for b in (first, ks, depth):
        b.free()


def _shard_bounds(n, world):
    chunk = 64 * -(-n // (64 * world)) - 64 * (world - 1)   # the last shard is larger, none ends where the cloud does
    return [r * chunk for r in range(world)] + [n]


@pytest.mark.parametrize("world", [2, 3])
def test_the_tables_of_surfel_shards_concatenate_to_the_unsharded_table(request, world):
    ba, A, t, g = _scene("tiny")
    request.addfinalizer(lambda: two_cameras.sync_gpu(g, ba))
    data = g.download_surfels().copy()
    bounds = _shard_bounds(data.shape[1], world)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        g.upload_surfels(np.ascontiguousarray(data[:, lo:hi]), np.ones(hi - lo, np.uint8))
        got = g.surfel_observations(prefill=FILL)
        so.assert_same(got, so.take(t, lo, hi), (lo, hi))
        parts.append(got)
    offsets = np.cumsum([0] + [p["pairs"] for p in parts])
    first = np.concatenate([p["surfel_first"][:-1].astype(np.int64) + o for p, o in zip(parts, offsets)] + [offsets[-1:]])
    assert np.array_equal(first, t["surfel_first"].astype(np.int64))
    for name in ("keyframes", "depth_raw", "descriptor_raw"):
        assert np.array_equal(so.words(np.concatenate([p[name] for p in parts])), so.words(t[name])), name


def test_a_fast_flavour_context_gives_the_exact_bytes():
    ba, A, t, g = _world("off_image")
    g.ctx.set_arithmetic("fast")
    g.set_intrinsics()
    try:
        assert g.ctx.arithmetic == "fast"
        _both_forms(g, t, "fast flavour")
    finally:
        g.ctx.set_arithmetic("exact")
        g.set_intrinsics()
    _check(g, t, "exact again")


def test_no_allocation_is_left_behind():
    lib = capi.load()
    tc, ba, A, t = so.scene("tiny")
    gc.collect()
    before = ll.live_allocations(lib)
    g = two_cameras.build_gpu(tc, ba)
    try:
        for form in FORMS:
            _shape(stage_entries=form)
            so.assert_same(g.surfel_observations(prefill=FILL), t, form)
            g.surfel_observations(size=100, capacity=3)
    finally:
        _shape()
    held = ll.live_allocations(lib)
    for form in FORMS:                                      # repeated calls allocate nothing
        g.surfel_observations(prefill=FILL)
    assert ll.live_allocations(lib) == held
    g.ctx.close()
    print("allocations", before, held, ll.live_allocations(lib))
    assert held[0] >= before[0] + 3 and ll.live_allocations(lib) == before
