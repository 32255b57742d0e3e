"""The reduced camera system on the GPU (bahip_reduced_camera_system; kernels_rcs.hip): S, g, A, b and the
statistics against MODEL32 of tests/reduced_camera_system.py, bit for bit, on the scenes whose census
tests/test_cpu_reduced_camera_system.py asserts (`tiny` and `crop_small` are the scenes whose colour camera differs from the depth
one: tests/two_cameras.py).  Launch shape, tile order, list capacity, sharding and arithmetic flavour must not move a bit."""
import ctypes as C
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll, synthetic
from oracle import binding as ob
from tests import reduced_camera_system as rcs
from tests import tile_cull
from tests import two_cameras
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL_WORD = np.uint64(0xA5A5A5A5A5A5A5A5)
SELECTIONS = [(True, False), (True, True), (False, True)]
_CACHE = {}


def _shape(waves=0, workgroups=0, list_capacity=0, tile_order=-1):
    capi.check(capi.load().bahip_debug_set_rcs_shape(waves, workgroups, list_capacity, tile_order))


def _scene(name):
    """(Words, a GPU scene in the oracle's state that every test leaves as it found it) of a scene of tests/two_cameras.py."""
    if name not in _CACHE:
        tc, ba, words = rcs.scene(name)
        _CACHE[name] = (words, two_cameras.build_gpu(tc, ba))
    return _CACHE[name]


def _world(name):
    if name not in _CACHE:
        w, ba, words = rcs.world(name)
        _CACHE[name] = (words, tile_cull.build_gpu(w, ba))
    return _CACHE[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, model, what):
    n = model.S.shape[0]
    for name, mine, theirs in (("S", got["S"][:, :n], model.S), ("g", got["g"], model.g), ("A", got["A"], model.A), ("b", got["b"], model.b)):
        if mine is None:
            continue
        where = np.argwhere(_bits(mine) != _bits(theirs))
        assert len(where) == 0, (what, name, len(where), where[:5], np.asarray(mine)[tuple(where[0])], np.asarray(theirs)[tuple(where[0])])
    assert got["stats"] == model.stats, (what, got["stats"], model.stats)


def _check(g, words, use_depth=True, use_desc=True, what="", capacity=rcs.DEFAULT_LIST_CAPACITY, size=None):
    got = g.reduced_camera_system(use_depth, use_desc, prefill=FILL, size=size)
    model = rcs.model32(words if size is None else words.take(slice(0, size)), use_depth, use_desc, capacity=capacity)
    print(what, (use_depth, use_desc), got["stats"])
    _same(got, model, (what, use_depth, use_desc))
    return got


@pytest.mark.parametrize("use_depth,use_desc", SELECTIONS)
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_system_is_the_model_on_the_scenes(name, use_depth, use_desc):
    words, g = _scene(name)
    got = _check(g, words, use_depth, use_desc, name)
    K = words.K
    assert got["stats"]["invalid"] == 0 and got["stats"]["pairs_visited"] > got["stats"]["list_entries"]
    blocks = np.abs(got["S"]).reshape(K, 6, K, 6).max(axis=(1, 3))
    assert (blocks > 0).all()


@pytest.mark.parametrize("name", ["centred", "neg_fy", "off_image"])
def test_the_system_is_the_model_on_the_edge_worlds(name):
    words, g = _world(name)
    got = _check(g, words, True, True, name)
    K = words.K
    blocks = np.abs(got["S"]).reshape(K, 6, K, 6).max(axis=(1, 3))
    counts = g.observed_covisibility()
    assert np.array_equal(blocks == 0, counts == 0)          # zero exactly where no surfel is shared
    assert blocks[6, 6] > 0 and (name != "centred" or not (blocks[7].any() or blocks[:, 7].any()))
    _check(g, words, True, False, name)


def _seventy():
    """70 keyframes on tiny's cloud (as tests/test_gpu_observed_covisibility.py builds them): tiles hold more entries than the list."""
    if "seventy" not in _CACHE:
        tc, ba4, _ = rcs.scene("tiny")
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
        ba.cfactor[:] = ba4.cfactor
        two_cameras.sync_gpu(g, ba)
        _CACHE["seventy"] = (rcs.oracle_words(ba), g)
    return _CACHE["seventy"]


def test_seventy_keyframes_walk_their_tiles_in_passes():
    words, g = _seventy()
    per_tile = tile_cull.per_tile(words.associated).sum(axis=1)
    assert words.K == 70 and int((per_tile > 64).sum()) >= 4
    got = _check(g, words, True, True, "70 keyframes")
    assert got["stats"]["overflow_tiles"] == int((per_tile > rcs.DEFAULT_LIST_CAPACITY).sum()) > 0
    assert np.array_equal(_bits(got["S"]), _bits(got["S"].T))


LATE_FILLERS = 1032            # keyframes that look away, ahead of the world's eight


def test_late_keyframes_behind_1032_that_look_away():
    w, ba, words = rcs.world("centred")
    poses = [w.poses[7]] * LATE_FILLERS + list(w.poses)
    images = [w.images[7]] * LATE_FILLERS + list(w.images)
    n = 64 * 64 - 11                                        # a prefix of 64 tiles that ends inside one
    g = tile_cull.build_gpu(w, poses=poses, images=images, capacity=n + 64)
    g.set_intrinsics()
    g.upload_surfels(w.surfels[:, :n], np.ones(n, np.uint8))
    assert not words.associated[7, :n].any()                 # the fillers are keyframe 7 again: they see nothing
    model = rcs.model32(words.take(slice(0, n)), True, True)
    got = g.reduced_camera_system(True, True, prefill=FILL)
    first = 6 * LATE_FILLERS
    assert got["S"].shape == (first + 48, first + 48)
    assert np.array_equal(_bits(got["S"][first:, first:]), _bits(model.S)) and np.array_equal(_bits(got["g"][first:]), _bits(model.g))
    assert np.array_equal(_bits(got["A"][LATE_FILLERS:]), _bits(model.A))
    assert np.count_nonzero(got["S"]) == np.count_nonzero(model.S) and not got["g"][:first].any()
    assert not _bits(got["S"][:first]).any() and not _bits(got["S"][:, :first]).any()          # +0.0 everywhere else
    assert got["stats"] == model.stats


def test_list_capacities_give_the_same_bits_and_reach_the_overflow_path():
    words, g = _scene("tiny")
    assert tile_cull.per_tile(words.associated).sum(axis=1).max() == 4
    reference = _check(g, words, True, True, "default capacity")
    assert reference["stats"]["overflow_tiles"] == 0
    lib = capi.load()
    try:
        for capacity in (1, 2, 16):
            capi.check(lib.bahip_debug_set_rcs_list_capacity(capacity))
            got = _check(g, words, True, True, f"capacity {capacity}", capacity=capacity)
            assert np.array_equal(_bits(got["S"]), _bits(reference["S"])) and np.array_equal(_bits(got["g"]), _bits(reference["g"]))
            assert (got["stats"]["overflow_tiles"] > 0) == (capacity < 4)
            _check(g, words, True, False, f"capacity {capacity}", capacity=capacity)
        for bad in ((5, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 33, 0), (0, 0, 0, 2), (4, 0, 32, 0)):
            assert lib.bahip_debug_set_rcs_shape(*bad) != 0 and b"bahip_debug_set_rcs_shape" in lib.bahip_last_error()
    finally:
        _shape()


def test_launch_shapes_and_tile_orders_give_the_same_bits():
    words, g = _scene("crop_small")
    poses = [kf["pose"].copy() for kf in g.keyframes]
    g.estimate_keyframe_poses(True, True)                   # a pose phase over the table leaves the heavy-first run order behind
    for kf, T in zip(g.keyframes, poses):
        kf["pose"] = T
    g.bind_keyframes()
    reference = _check(g, words, True, True, "crop_small, default shape")
    try:
        for waves, workgroups in [(1, 1), (2, 7), (3, 0), (4, 1), (1, 7), (2, 100000), (3, 1), (4, 7), (4, 0), (1, 100000)]:
            for order in (0, 1):
                _shape(waves, workgroups, 3, order)         # (and a list of three entries: most tiles here have four)
                got = g.reduced_camera_system(True, True, prefill=FILL, planes=False)
                assert np.array_equal(_bits(got["S"]), _bits(reference["S"])) and np.array_equal(_bits(got["g"]), _bits(reference["g"])), (waves, workgroups, order)
                assert got["stats"]["overflow_tiles"] > 0 and got["stats"]["pairs_visited"] == reference["stats"]["pairs_visited"]
            _shape(waves, workgroups, 0, 1)
            got = g.reduced_camera_system(True, True, prefill=FILL, planes=False)
            assert np.array_equal(_bits(got["S"]), _bits(reference["S"])) and got["stats"] == reference["stats"], (waves, workgroups)
    finally:
        _shape()


def test_prefixes_deleted_surfels_and_cleared_flags(request):
    words, g = _scene("tiny")
    tc, ba, _ = rcs.scene("tiny")
    request.addfinalizer(lambda: two_cameras.sync_gpu(g, ba))
    reference = _check(g, words, True, True, "tiny")
    n = words.n
    for size in (0, 1, 63, 64, 65, n):
        got = _check(g, words, True, True, f"prefix {size}", size=size)
        if size == 0:
            assert not _bits(got["S"]).any() and not any(got["stats"].values())
    # every surfel shared by keyframes 2 and 3 deleted (NaN x): their block is zero, the words are the model's without those surfels
    data = g.download_surfels().copy()
    shared = words.associated[2] & words.associated[3]
    assert shared.sum() > 100
    dead = data.copy()
    dead[0, shared] = np.nan
    g.upload_surfels(dead, np.ones(n, np.uint8))
    keep = np.flatnonzero(~shared)
    blanked = words.take(slice(0, n))
    for name in ("associated", "color", "Jpose", "Jp1", "Jp2") + rcs.Words.FIELDS:
        getattr(blanked, name)[:, shared] = 0
    got = g.reduced_camera_system(True, True, prefill=FILL)
    _same(got, rcs.model32(blanked, True, True), "deleted surfels")
    assert not got["S"][12:18, 18:24].any() and not got["S"][18:24, 12:18].any() and len(keep)
    # activation flags of surfels and keyframes cleared: nothing changes
    g.upload_surfels(data, np.zeros(n, np.uint8))
    for kf in g.keyframes:
        kf["activation"] = ob.KF_INACTIVE
    g.bind_keyframes()
    got = g.reduced_camera_system(True, True, prefill=FILL)
    for name in ("S", "g", "A", "b"):
        assert np.array_equal(_bits(got[name]), _bits(reference[name])), name


@pytest.mark.parametrize("use_depth,use_desc", SELECTIONS)
def test_identities(use_depth, use_desc):
    words, g = _scene("tiny")
    K = words.K
    got = g.reduced_camera_system(use_depth, use_desc, prefill=FILL)
    plain = g.reduced_camera_system(use_depth, use_desc, marginalise=False, prefill=FILL)
    # marginalise = 0: the block diagonal of the pose equations, which the pose-sum entry point rounds to binary32
    assert np.array_equal(_bits(plain["A"]), _bits(got["A"])) and np.array_equal(_bits(plain["g"]), _bits(got["b"].reshape(-1)))
    assert plain["stats"] == dict.fromkeys(ll.Scene.RCS_STATS, 0)
    for k in range(K):
        assert np.array_equal(_bits(plain["S"][6 * k:6 * k + 6, 6 * k:6 * k + 6]), _bits(got["A"][k]))
        off = plain["S"][6 * k:6 * k + 6].copy()
        off[:, 6 * k:6 * k + 6] = 0
        assert not _bits(off).any()
        F = tile_cull.frame_T_global(g.keyframes[k]["pose"]).reshape(-1)
        H, b = g.accumulate_pose_coeffs(k, use_depth, use_desc, F)
        upper = np.array([got["A"][k][i, j] for i, j in rcs.UPPER])
        assert np.array_equal(upper.astype(np.float32), H.astype(np.float32)) and np.array_equal(got["b"][k].astype(np.float32), b.astype(np.float32)), k
        assert (np.diag(got["A"][k] - got["S"][6 * k:6 * k + 6, 6 * k:6 * k + 6]) >= 0).all()
    assert np.array_equal(_bits(got["S"]), _bits(got["S"].T))
    blocks = np.abs(got["S"]).reshape(K, 6, K, 6).max(axis=(1, 3))
    assert np.array_equal(blocks == 0, g.observed_covisibility() == 0)


def test_null_planes_and_a_wider_pitch_leave_the_foreign_words_alone():
    words, g = _scene("tiny")
    n = 6 * words.K
    reference = g.reduced_camera_system(True, True, prefill=FILL)
    got = g.reduced_camera_system(True, True, prefill=FILL, pitch=n + 5, planes=False)
    assert got["S"].shape == (n, n + 5) and got["A"] is None
    assert np.array_equal(_bits(got["S"][:, :n]), _bits(reference["S"])) and (_bits(got["S"][:, n:]) == FILL_WORD).all()
    assert np.array_equal(_bits(got["g"]), _bits(reference["g"])) and got["stats"] == reference["stats"]


def test_refusals_write_nothing_and_leave_the_context_usable():
    words, g = _scene("tiny")
    lib = capi.load()
    n = 6 * words.K
    reference = g.reduced_camera_system(True, True, prefill=FILL)
    S = ll.DeviceBuffer2D(g.ctx, 1, n * n, np.float64).clear(FILL)
    gv = ll.DeviceBuffer2D(g.ctx, 1, n, np.float64).clear(FILL)
    s = g.surfels_struct()

    def intact():
        g.ctx.synchronize()
        return (S.download().view(np.uint64) == FILL_WORD).all() and (gv.download().view(np.uint64) == FILL_WORD).all()

    h, sp = g.ctx.handle, C.byref(s)
    for args in ((None, 1, 1, 1, sp, S.ptr, n, gv.ptr), (h, 1, 1, 1, None, S.ptr, n, gv.ptr), (h, 1, 1, 1, sp, None, n, gv.ptr),
                 (h, 1, 1, 1, sp, S.ptr, n, None), (h, 0, 0, 1, sp, S.ptr, n, gv.ptr), (h, 1, 1, 1, sp, S.ptr, n - 1, gv.ptr)):
        assert lib.bahip_reduced_camera_system(*args, None, None, None) != 0
        assert b"bahip_reduced_camera_system" in lib.bahip_last_error()
        assert intact()
    with pytest.raises(capi.BackendError, match="pitch_doubles") as refused:
        g.reduced_camera_system(True, True, pitch=n - 1, prefill=FILL)
    assert all((a.view(np.uint64) == FILL_WORD).all() for a in refused.value.arrays)
    # keyframe sharding
    g.set_keyframe_sharding(0, 2)
    try:
        assert lib.bahip_reduced_camera_system(h, 1, 1, 1, sp, S.ptr, n, gv.ptr, None, None, None) != 0
        assert b"keyframe sharding" in lib.bahip_last_error() and intact()
    finally:
        g.set_keyframe_sharding(0, 1)
        g.bind_keyframes()
    # no keyframe bound
    keyframes = g.keyframes
    g.keyframes = []
    g.bind_keyframes()
    try:
        assert lib.bahip_reduced_camera_system(h, 1, 1, 1, sp, S.ptr, n, gv.ptr, None, None, None) != 0
        assert b"no keyframe is bound" in lib.bahip_last_error() and intact()
    finally:
        g.keyframes = keyframes
        g.bind_keyframes()
    # a context without intrinsics
    bare = ll.Context()
    assert lib.bahip_reduced_camera_system(bare.handle, 1, 1, 1, sp, S.ptr, n, gv.ptr, None, None, None) != 0
    bare.close()
    assert intact()
    # a good call follows
    capi.check(lib.bahip_reduced_camera_system(h, 1, 1, 1, sp, S.ptr, n, gv.ptr, None, None, None))
    g.ctx.synchronize()
    assert np.array_equal(S.download().reshape(n, n).view(np.uint64), _bits(reference["S"]))
    S.free()
    gv.free()


def _shard_bounds(n, world):
    chunk = 64 * -(-n // (64 * world)) - 64 * (world - 1)   # the last shard is larger, none ends where the cloud does
    return [r * chunk for r in range(world)] + [n]


@pytest.mark.parametrize("world", [2, 3])
def test_surfel_shards_end_with_the_unsharded_bits_on_every_rank(world):
    words, g = _scene("tiny")
    tc, ba, _ = rcs.scene("tiny")
    reference = g.reduced_camera_system(True, True, prefill=FILL)
    data = g.download_surfels().copy()
    bounds = _shard_bounds(data.shape[1], world)
    summed, shards = rcs.sum_over_shards(words, bounds, use_depth=True, use_desc=True)
    _same(reference, summed, "the model's sum over the shards")

    def rank_main(rank, hook):
        gr = two_cameras.build_gpu(tc, ba)
        lo, hi = bounds[rank], bounds[rank + 1]
        gr.upload_surfels(np.ascontiguousarray(data[:, lo:hi]), np.ones(hi - lo, np.uint8))
        alone = gr.reduced_camera_system(True, True, prefill=FILL)          # without a hook: the shard's own system
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        together = gr.reduced_camera_system(True, True, prefill=FILL, pitch=6 * words.K + 3)
        return dict(alone=alone, together=together, keep=(hook, gr))

    results, loop = _run_ranks(world, rank_main)
    assert loop.calls == 1
    for rank, r in enumerate(results):
        _same(r["alone"], shards[rank], f"rank {rank} alone")
        _same(r["together"], summed, f"rank {rank} with the hook")
        assert (_bits(r["together"]["S"][:, 6 * words.K:]) == FILL_WORD).all(), rank


def test_a_failing_exchange_fails_by_name_and_writes_nothing():
    words, g = _scene("tiny")
    reference = g.reduced_camera_system(True, True, prefill=FILL)
    failing = capi.ALLREDUCE_FN(lambda *_: 1)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, failing, None))
    try:
        with pytest.raises(capi.BackendError, match="reduced camera system: the sum of the limbs over the ranks") as refused:
            g.reduced_camera_system(True, True, prefill=FILL)
        assert all((a.view(np.uint64) == FILL_WORD).all() for a in refused.value.arrays)
    finally:
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
    assert np.array_equal(_bits(g.reduced_camera_system(True, True, prefill=FILL)["S"]), _bits(reference["S"]))


def test_a_fast_flavour_context_gives_the_exact_bits():
    words, g = _world("off_image")
    reference = g.reduced_camera_system(True, True, prefill=FILL)
    g.ctx.set_arithmetic("fast")
    g.set_intrinsics()
    try:
        assert g.ctx.arithmetic == "fast"
        got = g.reduced_camera_system(True, True, prefill=FILL)
    finally:
        g.ctx.set_arithmetic("exact")
        g.set_intrinsics()
    for name in ("S", "g", "A", "b"):
        assert np.array_equal(_bits(got[name]), _bits(reference[name])), name
    assert got["stats"] == reference["stats"]


def test_no_allocation_is_left_behind():
    words, g = _scene("tiny")
    lib = capi.load()
    g.reduced_camera_system(True, True, prefill=FILL)
    gc.collect()
    before = ll.live_allocations(lib)
    try:
        for capacity in (0, 1):
            _shape(list_capacity=capacity)
            g.reduced_camera_system(True, True, prefill=FILL)
            g.reduced_camera_system(True, False, size=100, pitch=6 * words.K + 9, prefill=FILL, marginalise=capacity == 0)
    finally:
        _shape()
    gc.collect()
    assert ll.live_allocations(lib) == before
