"""Keyframe redundancy on the GPU (bahip_keyframe_observer_histogram; kernels_redundancy.hip): the K x B words
against the model of tests/keyframe_redundancy.py -- per keyframe its surfels by the number of other observers, from the oracle's
per-pair `associated` flags -- on the scenes and worlds whose census tests/test_cpu_keyframe_redundancy.py asserts.  All results are
integers: every comparison is an equality.  The census of the call (list entries, atomic adds, tiles traversed a second time) is held
to the model's counts as well; launch shape, tile order, list capacity, surfel order, sharding and arithmetic flavour must not move a
word."""
import ctypes as C
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll
from oracle import binding as ob
from tests import keyframe_redundancy as kr
from tests import observed_covisibility as oc
from tests import tile_cull
from tests import two_cameras
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks
from tests.test_gpu_observed_covisibility import LATE_FILLERS, _scene, _seventy, _shard_bounds, _world

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL_WORD = 0xA5A5A5A5
DEFAULT_CAPACITY = 128
BINS = 16


def _shape(waves=0, workgroups=0, list_capacity=0, tile_order=-1):
    capi.check(capi.load().bahip_debug_set_redundancy_shape(waves, workgroups, list_capacity, tile_order))


def _check(g, A, what, bins=BINS, capacity=DEFAULT_CAPACITY, size=None):
    """One call with the words prefilled: the model's table and the census."""
    A = A if size is None else A[:, :size]
    K = A.shape[0]
    got = g.keyframe_observer_histogram(bins, prefill=FILL, size=size)
    expected = kr.table(A, bins)
    assert got.dtype == np.uint32 and got.shape == (K, bins)
    assert np.array_equal(got.astype(np.int64), expected), (what, np.argwhere(got != expected)[:10])
    census = g.redundancy_census()
    print(what, "bins", bins, "census", census, "ceiling", kr.atomic_ceiling(A, bins))
    assert census[0] == oc.entries(A), what
    assert census[1] <= kr.atomic_ceiling(A, bins), what          # one atomic per entry and bin present in its mask at most
    assert census[1] == kr.nonzero_cells(A, bins), what
    assert census[2] == kr.second_traversals(A, capacity), what
    return got


@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_table_is_the_model_on_the_scenes(name):
    A, g = _scene(name)
    got = _check(g, A, name)
    # the row sums: the cost sweep's pair counts and the diagonal of the observed co-visibility; the column sums: the list lengths
    _, per = g.evaluate_cost(True, False)
    assert [c["depth_residuals"] for c in per] == got.sum(axis=1).tolist()
    assert np.diag(g.observed_covisibility()).tolist() == got.sum(axis=1).tolist()
    lists = g.surfel_observations(residuals=())
    lengths = np.bincount(np.diff(lists["surfel_first"].astype(np.int64)), minlength=BINS + 1)
    assert [int(v) for v in got.sum(axis=0)[:BINS - 1]] == [(j + 1) * int(lengths[j + 1]) for j in range(BINS - 1)]
    if name == "tiny":
        assert got.sum(axis=0)[:4].tolist() == [210, 372, 231, 2676]


@pytest.mark.parametrize("name", ["centred", "neg_fy", "off_image"])
def test_the_table_is_the_model_on_the_edge_worlds(name):
    A, g = _world(name)
    got = _check(g, A, name)
    assert got[6].any() and (name != "centred" or not got[7].any())       # the keyframe that looks away
    _, per = g.evaluate_cost(True, False)
    assert [c["depth_residuals"] for c in per] == got.sum(axis=1).tolist()


@pytest.mark.parametrize("bins", [1, 2, 16, 64])
def test_every_number_of_bins_and_a_wider_pitch(bins):
    A, g = _world("centred")              # surfels seen by 1 .. 7 keyframes: clipped at 2, exact at 16 and 64
    _check(g, A, "centred", bins=bins)
    K = A.shape[0]
    got = g.keyframe_observer_histogram(bins, prefill=FILL, pitch=bins + 5)
    assert got.shape == (K, bins + 5)
    assert np.array_equal(got[:, :bins].astype(np.int64), kr.table(A, bins))
    assert (got[:, bins:] == FILL_WORD).all()


def test_seventy_keyframes_reach_the_clip_and_the_second_traversal():
    A, g = _seventy()
    assert np.array_equal(A, kr.seventy_matrix())
    assert A.sum(axis=0).max() - 1 >= 64 and int((oc.tile_counts(A) > 64).sum()) >= 4       # the clip at B = 64; lists of more than 64
    reference = _check(g, A, "70 keyframes", bins=64)
    assert (reference[:, 63] > 0).all()
    assert g.redundancy_census()[2] == 0
    try:
        for capacity in (1, 2, 16, 64):
            _shape(list_capacity=capacity)
            got = _check(g, A, f"70 keyframes, capacity {capacity}", bins=64, capacity=capacity)
            assert np.array_equal(got, reference) and g.redundancy_census()[2] > 0
            assert np.array_equal(_check(g, A, f"70 keyframes, 16 bins, capacity {capacity}", capacity=capacity)[:, :15], reference[:, :15])
    finally:
        _shape()


def test_late_keyframes_behind_1032_that_look_away():
    w = tile_cull.world("centred")
    poses = [w.poses[7]] * LATE_FILLERS + list(w.poses)
    images = [w.images[7]] * LATE_FILLERS + list(w.images)
    n = 64 * 64 - 11                                        # a prefix of 64 tiles that ends inside one
    g = tile_cull.build_gpu(w, poses=poses, images=images, capacity=n + 64)
    g.set_intrinsics()
    g.upload_surfels(w.surfels[:, :n], np.ones(n, np.uint8))
    flags = oc.world_matrix("centred")[:, :n]
    assert not flags[7].any() and flags[:6].any(axis=1).all()
    A = np.concatenate([np.repeat(flags[7:8], LATE_FILLERS, axis=0), flags])       # the fillers are keyframe 7 again: its row
    K = LATE_FILLERS + 8
    got = g.keyframe_observer_histogram(BINS, prefill=FILL)
    assert got.shape == (K, BINS)
    assert np.array_equal(got[LATE_FILLERS:].astype(np.int64), kr.table(flags, BINS)) and got[LATE_FILLERS:LATE_FILLERS + 6].any(axis=1).all()
    assert not got[:LATE_FILLERS].any()
    census = g.redundancy_census()
    assert census[0] == oc.entries(A) and census[1] == kr.nonzero_cells(flags, BINS) and census[2] == 0


def test_list_capacities_give_the_same_words_and_reach_the_second_traversal():
    A, g = _scene("tiny")
    assert oc.tile_counts(A).max() == 4
    reference = _check(g, A, "default capacity")
    assert g.redundancy_census()[2] == 0
    try:
        for capacity in (1, 2, 3, 4, 16):
            _shape(list_capacity=capacity)
            got = _check(g, A, f"capacity {capacity}", capacity=capacity)
            assert np.array_equal(got, reference)
            assert (g.redundancy_census()[2] > 0) == (capacity < 4)
        lib = capi.load()
        for bad in ((9, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 449, 0), (0, 0, 0, 2)):
            assert lib.bahip_debug_set_redundancy_shape(*bad) != 0 and b"bahip_debug_set_redundancy_shape" in lib.bahip_last_error()
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
                got = g.keyframe_observer_histogram(BINS, prefill=FILL)
                assert np.array_equal(got, reference), (waves, workgroups, order)
                _shape(waves, workgroups, 0, order)
                got = g.keyframe_observer_histogram(BINS, prefill=FILL)
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
    # a surfel permutation: the same table
    perm = np.random.Generator(np.random.PCG64(5)).permutation(n)
    g.upload_surfels(np.ascontiguousarray(data[:, perm]), np.ones(n, np.uint8))
    assert np.array_equal(g.keyframe_observer_histogram(BINS, prefill=FILL), reference)
    g.upload_surfels(data, np.ones(n, np.uint8))
    # a keyframe permutation: the permuted rows
    keyframes = list(g.keyframes)
    order = [2, 0, 3, 1]
    g.keyframes = [keyframes[k] for k in order]
    g.bind_keyframes()
    assert np.array_equal(g.keyframe_observer_histogram(BINS, prefill=FILL), reference[order])
    # one bound keyframe: everything it sees, seen by nobody else
    g.keyframes = [keyframes[3]]
    g.bind_keyframes()
    assert g.keyframe_observer_histogram(3, prefill=FILL).tolist() == [[int(reference[3].sum()), 0, 0]]
    g.keyframes = keyframes
    g.bind_keyframes()
    # prefixes: none, one surfel, around a tile's end, all
    for size in (0, 1, 63, 64, 65, n):
        _check(g, A, f"prefix {size}", size=size)
    assert not g.keyframe_observer_histogram(BINS, prefill=FILL, size=0).any() and g.redundancy_census() == [0, 0, 0]
    # a buffer with capacity above surfels_size, garbage beyond the size
    assert g.capacity > n
    full = g.surfel_buf.download().copy()
    junk = full.copy()
    junk[:, n:] = junk[:, :1]                               # copies of surfel 0 beyond the size: they must not be counted
    g.surfel_buf.upload(junk)
    assert np.array_equal(g.keyframe_observer_histogram(BINS, prefill=FILL), reference)
    g.surfel_buf.upload(full)
    # every surfel shared by keyframes 2 and 3 deleted (NaN x): the model without them
    shared = A[2] & A[3]
    assert shared.sum() > 100 and (A[2] & ~shared).any() and (A[3] & ~shared).any()
    dead = data.copy()
    dead[0, shared] = np.nan
    g.upload_surfels(dead, np.ones(n, np.uint8))
    got = g.keyframe_observer_histogram(BINS, prefill=FILL)
    assert np.array_equal(got.astype(np.int64), kr.table(A & ~shared[None, :], BINS)) and not np.array_equal(got, reference)
    # activation flags of surfels and keyframes cleared: nothing changes
    g.upload_surfels(data, np.zeros(n, np.uint8))
    for kf in g.keyframes:
        kf["activation"] = ob.KF_INACTIVE
    g.bind_keyframes()
    assert np.array_equal(g.keyframe_observer_histogram(BINS, prefill=FILL), reference)


def test_refusals_write_nothing_and_leave_the_context_usable():
    A, g = _scene("tiny")
    lib = capi.load()
    K = A.shape[0]
    reference = g.keyframe_observer_histogram(BINS, prefill=FILL)
    buf = ll.DeviceBuffer2D(g.ctx, 1, K * BINS, np.uint32).clear(FILL)
    s = g.surfels_struct()

    def intact():
        g.ctx.synchronize()
        return (buf.download() == FILL_WORD).all()

    for args in ((None, C.byref(s), BINS, buf.ptr, BINS), (g.ctx.handle, None, BINS, buf.ptr, BINS), (g.ctx.handle, C.byref(s), BINS, None, BINS),
                 (g.ctx.handle, C.byref(s), 0, buf.ptr, BINS), (g.ctx.handle, C.byref(s), -1, buf.ptr, BINS), (g.ctx.handle, C.byref(s), 65, buf.ptr, 65),
                 (g.ctx.handle, C.byref(s), BINS, buf.ptr, BINS - 1)):
        assert lib.bahip_keyframe_observer_histogram(*args) != 0
        assert b"bahip_keyframe_observer_histogram" in lib.bahip_last_error()
        assert intact()
    with pytest.raises(capi.BackendError, match="pitch_words") as refused:
        g.keyframe_observer_histogram(BINS, prefill=FILL, pitch=BINS - 1)
    assert (refused.value.arrays == FILL_WORD).all()
    with pytest.raises(capi.BackendError, match="bins outside") as refused:
        g.keyframe_observer_histogram(65, prefill=FILL)
    assert (refused.value.arrays == FILL_WORD).all()
    # keyframe sharding
    g.set_keyframe_sharding(0, 2)
    try:
        assert lib.bahip_keyframe_observer_histogram(g.ctx.handle, C.byref(s), BINS, buf.ptr, BINS) != 0
        assert b"keyframe sharding" in lib.bahip_last_error() and intact()
    finally:
        g.set_keyframe_sharding(0, 1)
        g.bind_keyframes()
    # a context without intrinsics
    bare = ll.Context()
    bare_buf = ll.DeviceBuffer2D(bare, 1, K * BINS, np.uint32).clear(FILL)
    assert lib.bahip_keyframe_observer_histogram(bare.handle, C.byref(s), BINS, bare_buf.ptr, BINS) != 0
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
        capi.check(lib.bahip_keyframe_observer_histogram(g.ctx.handle, C.byref(s), BINS, buf.ptr, BINS))
        assert intact()
    finally:
        g.keyframes = keyframes
        g.bind_keyframes()
    # a good call follows
    capi.check(lib.bahip_keyframe_observer_histogram(g.ctx.handle, C.byref(s), BINS, buf.ptr, BINS))
    g.ctx.synchronize()
    assert np.array_equal(buf.download().reshape(K, BINS), reference)
    buf.free()


@pytest.mark.parametrize("world", [2, 3])
def test_surfel_shards_end_with_the_unsharded_words_on_every_rank(world):
    A, g = _scene("tiny")
    tc, ba, _ = oc.scene("tiny")
    reference = g.keyframe_observer_histogram(BINS, prefill=FILL)
    data = g.download_surfels().copy()
    bounds = _shard_bounds(data.shape[1], world)
    assert np.array_equal(kr.sum_over_shards(A, bounds, BINS), reference.astype(np.int64))

    def rank_main(rank, hook):
        gr = two_cameras.build_gpu(tc, ba)
        lo, hi = bounds[rank], bounds[rank + 1]
        gr.upload_surfels(np.ascontiguousarray(data[:, lo:hi]), np.ones(hi - lo, np.uint8))
        alone = gr.keyframe_observer_histogram(BINS, prefill=FILL)      # without a hook: the shard's own table
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        summed = gr.keyframe_observer_histogram(BINS, prefill=FILL, pitch=BINS + 3)
        return dict(alone=alone, summed=summed, keep=(hook, gr))

    results, loop = _run_ranks(world, rank_main)
    assert loop.calls == 1
    for rank, r in enumerate(results):
        lo, hi = bounds[rank], bounds[rank + 1]
        assert np.array_equal(r["alone"].astype(np.int64), kr.table(A[:, lo:hi], BINS)), rank
        assert np.array_equal(r["summed"][:, :BINS], reference), rank
        assert (r["summed"][:, BINS:] == FILL_WORD).all(), rank
    assert np.array_equal(sum(r["alone"].astype(np.int64) for r in results), reference.astype(np.int64))


def test_a_failing_exchange_fails_the_call_only():
    A, g = _scene("tiny")
    reference = g.keyframe_observer_histogram(BINS, prefill=FILL)
    failing = capi.ALLREDUCE_FN(lambda *_: 1)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, failing, None))
    try:
        with pytest.raises(capi.BackendError, match="table over the ranks") as refused:
            g.keyframe_observer_histogram(BINS, prefill=FILL)
        assert (refused.value.arrays == FILL_WORD).all()
    finally:
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
    assert np.array_equal(g.keyframe_observer_histogram(BINS, prefill=FILL), reference)


def test_a_fast_flavour_context_gives_the_exact_words():
    A, g = _world("off_image")
    reference = g.keyframe_observer_histogram(BINS, prefill=FILL)
    g.ctx.set_arithmetic("fast")
    g.set_intrinsics()
    try:
        assert g.ctx.arithmetic == "fast"
        assert np.array_equal(g.keyframe_observer_histogram(BINS, prefill=FILL), reference)
    finally:
        g.ctx.set_arithmetic("exact")
        g.set_intrinsics()
    assert np.array_equal(g.keyframe_observer_histogram(BINS, prefill=FILL), reference)


def test_no_allocation_is_left_behind():
    A, g = _scene("tiny")
    lib = capi.load()
    g.keyframe_observer_histogram(BINS, prefill=FILL)       # (the context's census words exist from its first call on)
    gc.collect()
    before = ll.live_allocations(lib)
    try:
        for capacity in (0, 1):
            _shape(list_capacity=capacity)
            g.keyframe_observer_histogram(BINS, prefill=FILL)
            g.keyframe_observer_histogram(64, prefill=FILL, size=100, pitch=70)
            g.redundancy_census()
    finally:
        _shape()
    gc.collect()
    assert ll.live_allocations(lib) == before
