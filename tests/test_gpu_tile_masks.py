"""The tile mask table on one context (kernels_tile_masks.hip; DESIGN.md section 3, "The tile mask table"): on route 1 of
bahip_debug_set_observed_structure_route the observed co-visibility, the keyframe redundancy and the observation lists are computed
from the table on an unsharded context too.  The table read back is the model's (tests/tile_masks.py, from the oracle's flags), and
the three calls give, word for word, what their own kernels give on route 0 -- over launch shapes, tile orders, prefixes, deleted
surfels, cleared activation flags, a wider pitch, two surfel shards and a fast-flavour context.  All comparisons are equalities of
integers or of bit patterns."""
import ctypes as C
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll
from oracle import binding as ob
from tests import keyframe_redundancy as kr
from tests import observed_covisibility as oc
from tests import surfel_observations as so
from tests import tile_cull
from tests import tile_masks as tm
from tests import two_cameras
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks
from tests.test_gpu_observed_covisibility import LATE_FILLERS, _scene, _seventy, _shard_bounds, _world

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL_WORD = 0xA5A5A5A5
BINS = 16


@pytest.fixture(autouse=True)
def _default_route_afterwards():
    yield
    ll.set_observed_structure_route(0)
    ll.set_tile_mask_shape()


def _three(g, size=None, bins=BINS):
    """The three calls on the route that is set: the matrix, the histogram, the lists with every plane."""
    return dict(matrix=g.observed_covisibility(prefill=FILL, size=size), histogram=g.keyframe_observer_histogram(bins, prefill=FILL, size=size),
                lists=g.surfel_observations(prefill=FILL, size=size))


def _same(a, b, what):
    assert np.array_equal(a["matrix"], b["matrix"]), what
    assert np.array_equal(a["histogram"], b["histogram"]), what
    so.assert_same(a["lists"], {k: (so.words(v) if k in ("depth_raw", "descriptor_raw") else v) for k, v in b["lists"].items()}, what)
    P = b["lists"]["pairs"]
    for name in ("keyframes", "depth_raw", "descriptor_raw"):          # beyond P nothing is touched on either route
        assert np.array_equal(so.words(a["lists"][name])[P:] if name != "keyframes" else a["lists"][name][P:],
                              so.words(b["lists"][name])[P:] if name != "keyframes" else b["lists"][name][P:]), (what, name)


def _both_routes(g, what, size=None, bins=BINS):
    ll.set_observed_structure_route(0)
    direct = _three(g, size, bins)
    ll.set_observed_structure_route(1)
    table = _three(g, size, bins)
    _same(table, direct, what)
    return direct


def _check_table(g, A, what, size=None):
    """After a call on route 1: the table read back is the model's, and the statistics are its numbers."""
    A = A if size is None else A[:, :size]
    first, ks, ms = g.tile_masks(size)
    want = tm.table(A)
    assert np.array_equal(first, want[0]) and np.array_equal(ks, want[1]) and np.array_equal(ms, want[2]), what
    stats = g.tile_mask_stats()
    E, T = len(want[1]), len(want[0]) - 1
    assert stats[0] == E and stats[1] == E and stats[2] == 0 and stats[3] == T, (what, stats)
    return want, stats


@pytest.mark.parametrize("name", ["tiny", "crop_small", "centred", "neg_fy", "off_image"])
def test_the_table_is_the_model_and_the_three_calls_are_those_of_route_0(name):
    A, g = _scene(name) if name in ("tiny", "crop_small") else _world(name)
    K, n = A.shape
    direct = _both_routes(g, name)
    assert np.array_equal(direct["matrix"].astype(np.int64), oc.matrix(A)) and direct["lists"]["pairs"] == int(A.sum()) > 0
    ll.set_observed_structure_route(1)
    g.observed_covisibility(prefill=FILL)
    want, stats = _check_table(g, A, name)
    assert stats[4] == tm.covisibility_adds(want) and stats[5] == 0
    assert g.covisibility_census() == [len(want[1]), stats[4], 0]
    g.keyframe_observer_histogram(BINS, prefill=FILL)
    want, stats = _check_table(g, A, name)
    assert stats[4] == kr.nonzero_cells(A, BINS) and g.redundancy_census() == [len(want[1]), stats[4], 0]
    lists = g.surfel_observations(prefill=FILL)
    want, stats = _check_table(g, A, name)
    assert stats[4] == 0 and stats[5] == 3 * lists["pairs"]          # one depth word and two descriptor words per pair, NaN pairs included
    only_depth = g.surfel_observations(prefill=FILL, residuals=("depth_raw",))
    assert g.tile_mask_stats()[5] == only_depth["pairs"]


def test_seventy_keyframes_fill_tiles_of_seventy_entries():
    A, g = _seventy()
    assert int(oc.tile_counts(A).max()) == 70
    _both_routes(g, "70 keyframes", bins=64)
    _check_table(g, A, "70 keyframes")


def test_late_keyframes_behind_1032_that_look_away():
    w = tile_cull.world("centred")
    poses = [w.poses[7]] * LATE_FILLERS + list(w.poses)
    images = [w.images[7]] * LATE_FILLERS + list(w.images)
    n = 64 * 64 - 11                                        # a prefix of 64 tiles that ends inside one
    g = tile_cull.build_gpu(w, poses=poses, images=images, capacity=n + 64)
    g.set_intrinsics()
    g.upload_surfels(w.surfels[:, :n], np.ones(n, np.uint8))
    flags = oc.world_matrix("centred")[:, :n]
    A = np.concatenate([np.repeat(flags[7:8], LATE_FILLERS, axis=0), flags])
    assert not A[:LATE_FILLERS].any()
    _both_routes(g, "late keyframes")
    want, _ = _check_table(g, A, "late keyframes")
    assert int(want[1].min()) >= LATE_FILLERS


def test_launch_shapes_and_tile_orders_give_the_same_words():
    A, g = _scene("crop_small")
    poses = [kf["pose"].copy() for kf in g.keyframes]
    g.estimate_keyframe_poses(True, True)                   # a pose phase over the table leaves the heavy-first run order behind
    for kf, T in zip(g.keyframes, poses):
        kf["pose"] = T
    g.bind_keyframes()
    ll.set_observed_structure_route(0)
    reference = _three(g)
    ll.set_observed_structure_route(1)
    for waves, workgroups in [(1, 1), (2, 7), (3, 0), (5, 100000), (8, 7), (8, 0)]:
        for order in (0, 1):
            ll.set_tile_mask_shape(waves, workgroups, order)
            _same(_three(g), reference, (waves, workgroups, order))
            _check_table(g, A, (waves, workgroups, order))
    lib = capi.load()
    for bad in ((9, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, 2, 0, 0), (0, 0, -2, 0, 0)):
        assert lib.bahip_debug_set_tile_mask_shape(*bad) != 0 and b"bahip_debug_set_tile_mask_shape" in lib.bahip_last_error()
    assert lib.bahip_debug_set_observed_structure_route(2) != 0 and b"bahip_debug_set_observed_structure_route" in lib.bahip_last_error()


def test_prefixes_edge_clouds_and_a_wider_pitch(request):
    A, g = _scene("tiny")
    tc, ba, _ = oc.scene("tiny")
    request.addfinalizer(lambda: two_cameras.sync_gpu(g, ba))
    K, n = A.shape
    for size in (0, 1, 63, 64, 65, n):
        _both_routes(g, f"prefix {size}", size=size)
        if size:
            _check_table(g, A, f"prefix {size}", size=size)
    # a wider pitch: the words beyond the row are not touched
    ll.set_observed_structure_route(1)
    got = g.observed_covisibility(prefill=FILL, pitch=K + 3)
    assert np.array_equal(got[:, :K].astype(np.int64), oc.matrix(A)) and (got[:, K:] == FILL_WORD).all()
    got = g.keyframe_observer_histogram(BINS, prefill=FILL, pitch=BINS + 5)
    assert np.array_equal(got[:, :BINS].astype(np.int64), kr.table(A, BINS)) and (got[:, BINS:] == FILL_WORD).all()
    # deleted (NaN) surfels
    data = g.download_surfels().copy()
    shared = A[2] & A[3]
    dead = data.copy()
    dead[0, shared] = np.nan
    g.upload_surfels(dead, np.ones(n, np.uint8))
    _both_routes(g, "deleted surfels")
    _check_table(g, A & ~shared[None, :], "deleted surfels")
    # activation flags of surfels and keyframes cleared: nothing changes
    g.upload_surfels(data, np.zeros(n, np.uint8))
    for kf in g.keyframes:
        kf["activation"] = ob.KF_INACTIVE
    g.bind_keyframes()
    _both_routes(g, "cleared activation flags")
    _check_table(g, A, "cleared activation flags")


def test_the_count_then_fill_protocol_and_the_pair_limit():
    A, g = _scene("tiny")
    P = int(A.sum())
    ll.set_observed_structure_route(1)
    count_only = g.surfel_observations(prefill=FILL, residuals=(), keyframes=False, capacity=0)
    assert count_only["pairs"] == P and np.array_equal(count_only["surfel_first"], so.csr(A)[0])
    short = g.surfel_observations(prefill=FILL, capacity=P - 1)
    assert short["pairs"] == P
    for name in ("keyframes", "depth_raw", "descriptor_raw"):
        assert (short[name].view(np.uint8) == FILL).all(), name
    lib = capi.load()
    capi.check(lib.bahip_debug_set_observations_shape(0, 0, 0, -1, P - 1))
    try:
        with pytest.raises(capi.BackendError, match="more than the pair limit") as refused:
            g.surfel_observations(prefill=FILL, capacity=P)
        for name, plane in refused.value.arrays.items():
            assert (plane.view(np.uint8) == FILL).all(), name
    finally:
        capi.check(lib.bahip_debug_set_observations_shape(0, 0, 0, -1, 0))


def test_two_surfel_shards_sum_to_the_unsharded_words():
    A, g = _scene("tiny")
    tc, ba, _ = oc.scene("tiny")
    ll.set_observed_structure_route(0)
    reference = _three(g)
    data = g.download_surfels().copy()
    bounds = _shard_bounds(data.shape[1], 2)
    ll.set_observed_structure_route(1)

    def rank_main(rank, hook):
        gr = two_cameras.build_gpu(tc, ba)
        lo, hi = bounds[rank], bounds[rank + 1]
        gr.upload_surfels(np.ascontiguousarray(data[:, lo:hi]), np.ones(hi - lo, np.uint8))
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        res = _three(gr)
        res["table"] = gr.tile_masks()
        return dict(res=res, keep=(hook, gr))

    results, loop = _run_ranks(2, rank_main)
    assert loop.calls == 2                                  # the matrix and the histogram: the surfel shards' sums, no table exchange
    whole = so.table(ba, A)
    for rank, r in enumerate(results):
        lo, hi = bounds[rank], bounds[rank + 1]
        assert np.array_equal(r["res"]["matrix"], reference["matrix"]) and np.array_equal(r["res"]["histogram"], reference["histogram"]), rank
        so.assert_same(r["res"]["lists"], so.take(whole, lo, hi), rank)
        want = tm.table(A[:, lo:hi])
        assert all(np.array_equal(x, y) for x, y in zip(r["res"]["table"], want)), rank


def test_a_fast_flavour_context_gives_the_exact_words():
    A, g = _world("off_image")
    ll.set_observed_structure_route(0)
    reference = _three(g)
    g.ctx.set_arithmetic("fast")
    g.set_intrinsics()
    try:
        ll.set_observed_structure_route(1)
        _same(_three(g), reference, "fast flavour")
        _check_table(g, A, "fast flavour")
    finally:
        g.ctx.set_arithmetic("exact")
        g.set_intrinsics()


def test_refusals_write_nothing_and_no_allocation_is_left_behind():
    A, g = _scene("tiny")
    lib = capi.load()
    K = A.shape[0]
    ll.set_observed_structure_route(1)
    s = g.surfels_struct()
    buf = ll.DeviceBuffer2D(g.ctx, 1, K * BINS, np.uint32).clear(FILL)

    def intact():
        g.ctx.synchronize()
        return (buf.download() == FILL_WORD).all()

    assert lib.bahip_keyframe_observer_histogram(g.ctx.handle, C.byref(s), BINS, buf.ptr, BINS - 1) != 0 and intact()
    assert lib.bahip_observed_covisibility(g.ctx.handle, C.byref(s), buf.ptr, K - 1) != 0 and intact()
    g.set_keyframe_sharding(0, 2)                           # keyframe sharding without a transport
    try:
        assert lib.bahip_keyframe_observer_histogram(g.ctx.handle, C.byref(s), BINS, buf.ptr, BINS) != 0
        assert b"keyframe sharding" in lib.bahip_last_error() and intact()
        assert lib.bahip_observed_covisibility(g.ctx.handle, C.byref(s), buf.ptr, K) != 0
        assert b"keyframe sharding" in lib.bahip_last_error() and intact()
    finally:
        g.set_keyframe_sharding(0, 1)
        g.bind_keyframes()
    buf.free()
    ll.set_observed_structure_route(0)
    g.observed_covisibility()
    with pytest.raises(capi.BackendError, match="built no table"):
        g.tile_masks()
    ll.set_observed_structure_route(1)
    _three(g)                                               # (the context's buffers exist from its first calls on)
    gc.collect()
    before = ll.live_allocations(lib)
    for _ in range(2):
        _three(g)
        _three(g, size=100)
        g.tile_masks(100)
        g.tile_mask_stats()
    gc.collect()
    assert ll.live_allocations(lib) == before
