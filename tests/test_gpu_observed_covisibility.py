"""Observed co-visibility on the GPU (bahip_observed_covisibility; kernels_covisibility.hip): the K x K words against
the model of tests/observed_covisibility.py -- A @ A.T of the oracle's per-pair `associated` flags -- on the scenes and worlds whose
census tests/test_cpu_observed_covisibility.py asserts.  All results are integers: every comparison is an equality.  The census of the
call (list entries, atomic adds, tiles on the overflow path) is held to the model's counts as well; launch shape, tile order, list
capacity, surfel order, sharding and arithmetic flavour must not move a word."""
import ctypes as C
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll, synthetic
from oracle import binding as ob
from tests import observed_covisibility as oc
from tests import tile_cull
from tests import two_cameras
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL_WORD = 0xA5A5A5A5
_CACHE = {}


def _shape(waves=0, workgroups=0, list_capacity=0, tile_order=-1):
    capi.check(capi.load().bahip_debug_set_covisibility_shape(waves, workgroups, list_capacity, tile_order))


def _scene(name):
    """(A, a GPU scene in the oracle's state that every test leaves as it found it) of a scene of tests/two_cameras.py."""
    if name not in _CACHE:
        tc, ba, A = oc.scene(name)
        _CACHE[name] = (A, two_cameras.build_gpu(tc, ba))
    return _CACHE[name]


def _world(name):
    if name not in _CACHE:
        w = tile_cull.world(name)
        _CACHE[name] = (oc.world_matrix(name), tile_cull.build_gpu(w, tile_cull.build_oracle(w)))
    return _CACHE[name]


def _pairs_that_meet(A):
    """sum over the tiles of the pairs i <= j whose masks share a surfel: the atomic adds of a sweep that sums one triangle and adds
    nothing for a pair of masks that do not meet."""
    A = np.asarray(A, bool)
    K, n = A.shape
    total = 0
    for lo in range(0, n, 64):
        t = A[:, lo:lo + 64].astype(np.int64)
        total += int(np.count_nonzero(np.triu(t @ t.T)))
    return total


def _check(g, A, what, capacity=128):
    """One call with the words prefilled: the model's matrix, the diagonal of the cost sweep, the census."""
    K = A.shape[0]
    got = g.observed_covisibility(prefill=FILL)
    expected = oc.matrix(A)
    assert got.dtype == np.uint32 and got.shape == (K, K)
    assert np.array_equal(got.astype(np.int64), expected), (what, np.argwhere(got != expected)[:10])
    census = g.covisibility_census()
    counts = oc.tile_counts(A)
    print(what, "census", census, "ceiling", oc.atomic_ceiling(A), "largest tile", int(counts.max()) if len(counts) else 0)
    assert census[0] == oc.entries(A), what
    assert census[1] <= oc.atomic_ceiling(A), what          # one atomic per pair, triangle and tile at most
    assert census[1] == _pairs_that_meet(A), what
    assert census[2] == int((counts > capacity).sum()), what
    return got


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_matrix_is_the_model_on_the_scenes(name):
    A, g = _scene(name)
    got = _check(g, A, name)
    assert got[~np.eye(4, dtype=bool)].min() > 0
    _, per = g.evaluate_cost(True, False)
    assert [c["depth_residuals"] for c in per] == np.diag(got).tolist()
    _, per = g.evaluate_cost(True, True)
    assert [c["depth_residuals"] for c in per] == np.diag(got).tolist()


@pytest.mark.parametrize("name", ["centred", "neg_fy", "off_image"])
def test_the_matrix_is_the_model_on_the_edge_worlds(name):
    A, g = _world(name)
    got = _check(g, A, name)
    assert got[6, 6] > 0 and (name != "centred" or not (got[7].any() or got[:, 7].any()))   # the keyframe that looks away
    _, per = g.evaluate_cost(True, False)
    assert [c["depth_residuals"] for c in per] == np.diag(got).tolist()


def _seventy():
    """70 keyframes on tiny's cloud: the four images in turn at perturbed poses; oracle and GPU scene in the same state."""
    if "seventy" not in _CACHE:
        tc, ba4, _ = oc.scene("tiny")
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
        _CACHE["seventy"] = (oc.associated_matrix(ba), g)
    return _CACHE["seventy"]


def test_seventy_keyframes_fill_a_second_chunk_and_lists_of_more_than_64_entries():
    A, g = _seventy()
    counts = oc.tile_counts(A)
    assert A.shape[0] == 70 and A[64:].any(axis=1).all() and int((counts > 64).sum()) >= 4, np.bincount(counts).tolist()
    reference = _check(g, A, "70 keyframes")
    try:
        for capacity in (1, 2, 16, 64):
            _shape(list_capacity=capacity)
            got = _check(g, A, f"70 keyframes, capacity {capacity}", capacity=capacity)
            assert np.array_equal(got, reference) and g.covisibility_census()[2] > 0
    finally:
        _shape()


LATE_FILLERS = 1032            # keyframes that look away, ahead of the world's eight (as tests/test_gpu_tile_cull.py places them)


def test_late_keyframes_behind_1032_that_look_away():
    w = tile_cull.world("centred")
    poses = [w.poses[7]] * LATE_FILLERS + list(w.poses)
    images = [w.images[7]] * LATE_FILLERS + list(w.images)
    n = 64 * 64 - 11                                        # a prefix of 64 tiles that ends inside one
    g = tile_cull.build_gpu(w, poses=poses, images=images, capacity=n + 64)
    g.set_intrinsics()
    g.upload_surfels(w.surfels[:, :n], np.ones(n, np.uint8))
    flags = oc.world_matrix("centred")[:, :n]
    assert not flags[7].any() and flags[:6].any(axis=1).all()       # (keyframe 6 stands close: it sees none of the first tiles)
    A = np.concatenate([np.repeat(flags[7:8], LATE_FILLERS, axis=0), flags])       # the fillers are keyframe 7 again: its row
    K = LATE_FILLERS + 8
    got = g.observed_covisibility(prefill=FILL)
    assert got.shape == (K, K)
    block = got[LATE_FILLERS:, LATE_FILLERS:]
    assert np.array_equal(block.astype(np.int64), oc.matrix(flags)) and block[:6, :6].all()
    blanked = got.copy()
    blanked[LATE_FILLERS:, LATE_FILLERS:] = 0
    assert not blanked.any()
    assert g.covisibility_census()[0] == oc.entries(A)


def test_list_capacities_give_the_same_words_and_reach_the_overflow_path():
    A, g = _scene("tiny")
    assert oc.tile_counts(A).max() == 4
    reference = _check(g, A, "default capacity")
    assert g.covisibility_census()[2] == 0
    try:
        for capacity in (1, 2, 16):
            _shape(list_capacity=capacity)
            got = _check(g, A, f"capacity {capacity}", capacity=capacity)
            assert np.array_equal(got, reference)
            assert (g.covisibility_census()[2] > 0) == (capacity < 4)
        lib = capi.load()
        for bad in ((9, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 513, 0), (0, 0, 0, 2)):
            assert lib.bahip_debug_set_covisibility_shape(*bad) != 0 and b"bahip_debug_set_covisibility_shape" in lib.bahip_last_error()
    finally:
        _shape()


def test_launch_shapes_and_tile_orders_give_the_same_words():
    A, g = _scene("crop_small")
    poses = [kf["pose"].copy() for kf in g.keyframes]
    g.estimate_keyframe_poses(True, True)                   # a pose phase over the table leaves the heavy-first run order behind
    for kf, T in zip(g.keyframes, poses):
        kf["pose"] = T
    g.bind_keyframes()
    reference = _check(g, A, "crop_small, default shape")
    try:
        for waves, workgroups in [(1, 1), (2, 7), (3, 0), (4, 1), (5, 7), (6, 100000), (7, 1), (8, 7), (8, 0), (1, 100000)]:
            for order in (0, 1):
                _shape(waves, workgroups, 3, order)         # (and a list of three entries: most tiles here have four)
                got = g.observed_covisibility(prefill=FILL)
                assert np.array_equal(got, reference), (waves, workgroups, order)
                _shape(waves, workgroups, 0, order)
                got = g.observed_covisibility(prefill=FILL)
                assert np.array_equal(got, reference), (waves, workgroups, order)
    finally:
        _shape()


def test_invariances_and_edge_clouds(request):
    A, g = _scene("tiny")
    tc, ba, _ = oc.scene("tiny")
    request.addfinalizer(lambda: two_cameras.sync_gpu(g, ba))
    reference = _check(g, A, "tiny")
    data = g.download_surfels().copy()
    n = data.shape[1]
    # a surfel permutation: the same matrix
    perm = np.random.Generator(np.random.PCG64(5)).permutation(n)
    g.upload_surfels(np.ascontiguousarray(data[:, perm]), np.ones(n, np.uint8))
    assert np.array_equal(g.observed_covisibility(prefill=FILL), reference)
    g.upload_surfels(data, np.ones(n, np.uint8))
    # a keyframe permutation: the permuted matrix
    keyframes = list(g.keyframes)
    order = [2, 0, 3, 1]
    g.keyframes = [keyframes[k] for k in order]
    g.bind_keyframes()
    assert np.array_equal(g.observed_covisibility(prefill=FILL), reference[np.ix_(order, order)])
    # one bound keyframe: a 1 x 1 matrix
    g.keyframes = [keyframes[3]]
    g.bind_keyframes()
    assert g.observed_covisibility(prefill=FILL).tolist() == [[int(reference[3, 3])]]
    g.keyframes = keyframes
    g.bind_keyframes()
    # a prefix that ends inside a tile, and an empty cloud
    size = 7 * 64 + 29
    assert np.array_equal(g.observed_covisibility(size=size, prefill=FILL).astype(np.int64), oc.matrix(A[:, :size]))
    assert g.covisibility_census()[0] == oc.entries(A[:, :size])
    assert not g.observed_covisibility(size=0, prefill=FILL).any() and g.covisibility_census() == [0, 0, 0]
    # every surfel shared by keyframes 2 and 3 deleted (NaN x): they share nothing, the other words are the model's
    shared = A[2] & A[3]
    assert shared.sum() > 100 and (A[2] & ~shared).any() and (A[3] & ~shared).any()
    dead = data.copy()
    dead[0, shared] = np.nan
    g.upload_surfels(dead, np.ones(n, np.uint8))
    got = g.observed_covisibility(prefill=FILL)
    assert got[2, 3] == 0 and got[3, 2] == 0 and got[2, 2] > 0 and got[3, 3] > 0
    assert np.array_equal(got.astype(np.int64), oc.matrix(A & ~shared[None, :]))
    # activation flags of surfels and keyframes cleared: nothing changes
    g.upload_surfels(data, np.zeros(n, np.uint8))
    for kf in g.keyframes:
        kf["activation"] = ob.KF_INACTIVE
    g.bind_keyframes()
    assert np.array_equal(g.observed_covisibility(prefill=FILL), reference)


def test_a_matrix_inside_a_wider_buffer_leaves_the_foreign_words_alone():
    A, g = _scene("tiny")
    K = A.shape[0]
    got = g.observed_covisibility(pitch=K + 5, prefill=FILL)
    assert got.shape == (K, K + 5)
    assert np.array_equal(got[:, :K].astype(np.int64), oc.matrix(A))
    assert (got[:, K:] == FILL_WORD).all()


def test_refusals_write_nothing_and_leave_the_context_usable():
    A, g = _scene("tiny")
    lib = capi.load()
    K = A.shape[0]
    reference = g.observed_covisibility(prefill=FILL)
    buf = ll.DeviceBuffer2D(g.ctx, 1, K * K, np.uint32).clear(FILL)
    s = g.surfels_struct()

    def intact():
        g.ctx.synchronize()
        return (buf.download() == FILL_WORD).all()

    for args in ((None, C.byref(s), buf.ptr, K), (g.ctx.handle, None, buf.ptr, K), (g.ctx.handle, C.byref(s), None, K),
                 (g.ctx.handle, C.byref(s), buf.ptr, K - 1)):
        assert lib.bahip_observed_covisibility(*args) != 0
        assert b"bahip_observed_covisibility" in lib.bahip_last_error()
        assert intact()
    with pytest.raises(capi.BackendError, match="pitch_words") as refused:
        g.observed_covisibility(pitch=K - 1, prefill=FILL)
    assert (refused.value.arrays == FILL_WORD).all()
    # keyframe sharding
    g.set_keyframe_sharding(0, 2)
    try:
        assert lib.bahip_observed_covisibility(g.ctx.handle, C.byref(s), buf.ptr, K) != 0
        assert b"keyframe sharding" in lib.bahip_last_error() and intact()
    finally:
        g.set_keyframe_sharding(0, 1)
        g.bind_keyframes()
    # a context without intrinsics
    bare = ll.Context()
    bare_buf = ll.DeviceBuffer2D(bare, 1, K * K, np.uint32).clear(FILL)
    assert lib.bahip_observed_covisibility(bare.handle, C.byref(s), bare_buf.ptr, K) != 0
    assert b"bahip_set_intrinsics" in lib.bahip_last_error()
    bare.synchronize()
    assert (bare_buf.download() == FILL_WORD).all()
    bare_buf.free()
    bare.close()
    # no keyframe bound: succeeds and writes nothing
    keyframes = g.keyframes
    g.keyframes = []
    g.bind_keyframes()
    try:
        capi.check(lib.bahip_observed_covisibility(g.ctx.handle, C.byref(s), buf.ptr, 0))
        assert intact()
    finally:
        g.keyframes = keyframes
        g.bind_keyframes()
    # a good call follows
    capi.check(lib.bahip_observed_covisibility(g.ctx.handle, C.byref(s), buf.ptr, K))
    g.ctx.synchronize()
    assert np.array_equal(buf.download().reshape(K, K), reference)
    buf.free()


def _shard_bounds(n, world):
    chunk = 64 * -(-n // (64 * world)) - 64 * (world - 1)   # the last shard is larger, none ends where the cloud does
    return [r * chunk for r in range(world)] + [n]


@pytest.mark.parametrize("world", [2, 3])
def test_surfel_shards_end_with_the_unsharded_words_on_every_rank(world):
    A, g = _scene("tiny")
    tc, ba, _ = oc.scene("tiny")
    reference = g.observed_covisibility(prefill=FILL)
    data = g.download_surfels().copy()
    bounds = _shard_bounds(data.shape[1], world)
    assert np.array_equal(oc.sum_over_shards(A, bounds), reference.astype(np.int64))

    def rank_main(rank, hook):
        gr = two_cameras.build_gpu(tc, ba)
        lo, hi = bounds[rank], bounds[rank + 1]
        gr.upload_surfels(np.ascontiguousarray(data[:, lo:hi]), np.ones(hi - lo, np.uint8))
        alone = gr.observed_covisibility(prefill=FILL)      # without a hook: the shard's own matrix
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        summed = gr.observed_covisibility(pitch=A.shape[0] + 3, prefill=FILL)
        return dict(alone=alone, summed=summed, keep=(hook, gr))

    results, loop = _run_ranks(world, rank_main)
    assert loop.calls == 1
    for rank, r in enumerate(results):
        lo, hi = bounds[rank], bounds[rank + 1]
        assert np.array_equal(r["alone"].astype(np.int64), oc.matrix(A[:, lo:hi])), rank
        assert np.array_equal(r["summed"][:, :A.shape[0]], reference), rank
        assert (r["summed"][:, A.shape[0]:] == FILL_WORD).all(), rank
    assert np.array_equal(sum(r["alone"].astype(np.int64) for r in results), reference.astype(np.int64))


def test_a_failing_exchange_fails_the_call_only():
    A, g = _scene("tiny")
    reference = g.observed_covisibility(prefill=FILL)
    failing = capi.ALLREDUCE_FN(lambda *_: 1)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, failing, None))
    try:
        with pytest.raises(capi.BackendError, match="counts over the ranks") as refused:
            g.observed_covisibility(prefill=FILL)
        assert (refused.value.arrays == FILL_WORD).all()
    finally:
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
    assert np.array_equal(g.observed_covisibility(prefill=FILL), reference)


def test_a_fast_flavour_context_gives_the_exact_words():
    A, g = _world("off_image")
    reference = g.observed_covisibility(prefill=FILL)
    g.ctx.set_arithmetic("fast")
    g.set_intrinsics()
    try:
        assert g.ctx.arithmetic == "fast"
        assert np.array_equal(g.observed_covisibility(prefill=FILL), reference)
    finally:
        g.ctx.set_arithmetic("exact")
        g.set_intrinsics()
    assert np.array_equal(g.observed_covisibility(prefill=FILL), reference)


def test_no_allocation_is_left_behind():
    A, g = _scene("tiny")
    lib = capi.load()
    g.observed_covisibility(prefill=FILL)                   # (the context's census words exist from its first call on)
    gc.collect()
    before = ll.live_allocations(lib)
    try:
        for capacity in (0, 1):
            _shape(list_capacity=capacity)
            g.observed_covisibility(prefill=FILL)
            g.observed_covisibility(size=100, pitch=9, prefill=FILL)
            g.covisibility_census()
    finally:
        _shape()
    gc.collect()
    assert ll.live_allocations(lib) == before
