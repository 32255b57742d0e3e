"""The observed structure under KEYFRAME sharding (bahip_context_set_keyframe_sharding): bahip_observed_covisibility,
bahip_keyframe_observer_histogram and bahip_surfel_observations build the tile mask table (kernels_tile_masks.hip; DESIGN.md section 3,
"The tile mask table") from every rank's own keyframes and reduce it; every rank must end with the words of the unsharded call.  The
ranks are host threads that share one device and sum through the in-process loopback of tests/test_gpu_keyframe_sharded_intrinsics.py;
the images of the keyframes a rank does not own are scrambled before binding, so that reading one shows.  The census of what these
scenes exercise -- entries per rank, tiles the merge reorders, lists that interleave the ranks -- is asserted on the CPU in
tests/test_cpu_tile_masks.py.  All comparisons are equalities of integers or of bit patterns."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll
from tests import keyframe_redundancy as kr
from tests import observed_covisibility as oc
from tests import surfel_observations as so
from tests import tile_cull
from tests import tile_masks as tm
from tests import two_cameras
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks
from tests.test_gpu_observed_covisibility import _scene, _seventy, _world

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL_WORD = 0xA5A5A5A5
BINS = (1, 16, 64)


@pytest.fixture(autouse=True)
def _defaults_afterwards():
    yield
    ll.set_tile_mask_shape()
    capi.check(capi.load().bahip_debug_set_observations_shape(0, 0, 0, -1, 0))


@functools.lru_cache(maxsize=None)
def _seventy_oracle():
    return kr.seventy_oracle()


def _fresh(name):
    """A GPU scene of its own in the state of the cached one."""
    if name == "tiny":
        tc, ba, _ = oc.scene("tiny")
        return two_cameras.build_gpu(tc, ba)
    if name == "seventy":
        tc, _, _ = oc.scene("tiny")
        scene = tc.scene
        g = ll.Scene(ll.Context(), tc.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell,
                     ll.make_camera(tc.color_camera, tc.color_width, tc.color_height), ll.make_camera(scene.camera, scene.width, scene.height))
        for k, T in enumerate(kr.seventy_poses()):
            g.add_keyframe(scene.depth[k % 4], scene.rgb[k % 4], T)
        return two_cameras.sync_gpu(g, _seventy_oracle())
    w = tile_cull.world(name)
    return tile_cull.build_gpu(w, tile_cull.build_oracle(w))


def _reference(name):
    A, g = _seventy() if name == "seventy" else _scene(name) if name == "tiny" else _world(name)
    if name == "seventy":
        assert np.array_equal(A, kr.seventy_matrix())
    return A, dict(matrix=g.observed_covisibility(), histograms={b: g.keyframe_observer_histogram(b) for b in BINS}, lists=g.surfel_observations())


def _shard(gr, rank, world, hook, seed=3):
    """The scene as rank `rank` of `world` holds it: the transport, the partition, the other ranks' images scrambled and handed over."""
    capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
    if world == 8:
        gr.set_sum_classes(8)
    gr.set_keyframe_sharding(rank, world)
    rng = np.random.Generator(np.random.PCG64(seed + rank))
    for k in range(len(gr.keyframes)):
        if k % world != rank:
            for which in ("depth", "normals", "radius"):
                buf = gr.keyframes[k][which]
                buf.upload(rng.integers(0, 1 << 16, size=(buf.height, buf.width), dtype=np.uint16))
    gr.kf_shard = (0, 1)                                       # (bind_keyframes then passes every frame's pointers)
    gr.bind_keyframes()
    return gr


def _calls(gr):
    """The three calls of one rank, each with the table and the statistics it left."""
    out = dict(histograms={}, tables=[], stats=[])

    def note():
        out["tables"].append(gr.tile_masks())
        out["stats"].append(gr.tile_mask_stats())

    out["matrix"] = gr.observed_covisibility(prefill=FILL)
    note()
    out["census"] = gr.covisibility_census()
    for b in BINS:
        out["histograms"][b] = gr.keyframe_observer_histogram(b, prefill=FILL, pitch=b + 3)
        note()
    out["lists"] = gr.surfel_observations(prefill=FILL)
    note()
    return out


def _assert_lists(got, ref, what):
    so.assert_same(got, {k: (so.words(v) if k in ("depth_raw", "descriptor_raw") else v) for k, v in ref.items()}, what)


def _check_rank(r, rank, world, A, ref):
    K, n = A.shape
    want = tm.table(A)
    E, T, P = len(want[1]), len(want[0]) - 1, int(A.sum())
    assert np.array_equal(r["matrix"], ref["matrix"]), rank
    for b in BINS:
        assert np.array_equal(r["histograms"][b][:, :b], ref["histograms"][b]) and (r["histograms"][b][:, b:] == FILL_WORD).all(), (rank, b)
    _assert_lists(r["lists"], ref["lists"], rank)
    for table in r["tables"]:
        assert all(np.array_equal(x, y) for x, y in zip(table, want)), rank
    listed = tm.listed(A, world)[rank]
    dealt = tm.dealt_tiles(T, rank, world)
    for i, stats in enumerate(r["stats"]):
        assert stats[0] == listed and stats[1] == E, (rank, i, stats)
    matrix_stats, lists_stats = r["stats"][0], r["stats"][-1]
    assert matrix_stats[2] == tm.reduction_exchanges(E) and matrix_stats[3] == len(dealt), (rank, matrix_stats)
    assert matrix_stats[4] == tm.covisibility_adds(want, dealt) and r["census"] == [E, matrix_stats[4], 0], (rank, matrix_stats)
    for stats in r["stats"][1:-1]:
        assert stats[2] == tm.reduction_exchanges(E) and stats[3] == len(dealt), (rank, stats)
    assert lists_stats[2] == tm.observation_exchanges(E, P, P) and lists_stats[3] == T, (rank, lists_stats)
    own = A[tm.owned(K, rank, world)]
    assert lists_stats[5] == 3 * int(own.sum()), (rank, lists_stats)          # the payload of its own keyframes only
    return matrix_stats


def _run(name, world, arithmetic=None):
    A, ref = _reference(name)
    want = tm.table(A)
    E, T, P = len(want[1]), len(want[0]) - 1, int(A.sum())

    def rank_main(rank, hook):
        gr = _fresh(name)
        if arithmetic:
            gr.ctx.set_arithmetic(arithmetic)
            gr.set_intrinsics()
        _shard(gr, rank, world, hook)
        out = _calls(gr)
        out["keep"] = (hook, gr)
        return out

    results, loop = _run_ranks(world, rank_main)
    stats = [_check_rank(r, rank, world, A, ref) for rank, r in enumerate(results)]
    assert sum(s[0] for s in stats) == E and sum(s[3] for s in stats) == T
    # the matrix, three histograms, the count-only call of the lists and their fill
    assert loop.calls == 4 * tm.reduction_exchanges(E) + tm.table_exchanges(E) + tm.observation_exchanges(E, P, P)
    return A, results


@pytest.mark.parametrize("name", ["tiny", "centred"])
@pytest.mark.parametrize("world", [2, 4])
def test_every_rank_ends_with_the_unsharded_words(name, world):
    _run(name, world)


@pytest.mark.parametrize("name", ["tiny", "centred", "seventy"])
def test_eight_ranks(name):
    A, results = _run(name, 8)
    if name == "tiny":                                         # four keyframes: ranks 4 .. 7 own none and join every exchange
        assert [r["stats"][0][0] for r in results][4:] == [0, 0, 0, 0]


def test_a_fast_flavour_context_gives_the_exact_words():
    _run("tiny", 2, arithmetic="fast")


def test_one_keyframe_on_two_ranks():
    tc, ba, A4 = oc.scene("tiny")
    A = A4[3:4]
    expected = so.table(ba, A, keyframes=[3])

    def rank_main(rank, hook):
        gr = two_cameras.build_gpu(tc, ba)
        gr.keyframes = [gr.keyframes[3]]
        _shard(gr, rank, 2, hook)
        out = _calls(gr)
        out["keep"] = (hook, gr)
        return out

    results, _ = _run_ranks(2, rank_main)
    for rank, r in enumerate(results):
        assert np.array_equal(r["matrix"].astype(np.int64), oc.matrix(A)), rank
        for b in BINS:
            assert np.array_equal(r["histograms"][b][:, :b].astype(np.int64), kr.table(A, b)), (rank, b)
        so.assert_same(r["lists"], expected, rank)
        assert r["stats"][0][0] == (len(tm.table(A)[1]) if rank == 0 else 0)


def _tiny_pair(body, **shape):
    """body(gr, rank) on the two ranks of tiny; returns (A, results, exchanges)."""
    A, _ = _scene("tiny")

    def rank_main(rank, hook):
        gr = _shard(_fresh("tiny"), rank, 2, hook)
        out = body(gr, rank)
        out["keep"] = (hook, gr)
        return out

    ll.set_tile_mask_shape(**shape)
    try:
        results, loop = _run_ranks(2, rank_main)
    finally:
        ll.set_tile_mask_shape()
    return A, results, loop.calls


@pytest.mark.parametrize("entry_slice,payload_slice", [(1, 0), (7, 1000), (0, 333)])
def test_the_exchanges_follow_the_slices(entry_slice, payload_slice):
    _, ref = _reference("tiny")

    def body(gr, rank):
        return dict(matrix=gr.observed_covisibility(prefill=FILL), lists=gr.surfel_observations(prefill=FILL))

    A, results, calls = _tiny_pair(body, entry_slice=entry_slice, payload_slice=payload_slice)
    E, P = len(tm.table(A)[1]), int(A.sum())
    assert (E, P) == (72, 3489)
    slices = dict(entry_slice=entry_slice or tm.DEFAULT_ENTRY_SLICE, payload_slice=payload_slice or tm.DEFAULT_PAYLOAD_SLICE)
    assert calls == tm.reduction_exchanges(E, slices["entry_slice"]) + tm.table_exchanges(E, slices["entry_slice"]) + \
        tm.observation_exchanges(E, P, P, **slices)
    for rank, r in enumerate(results):
        assert np.array_equal(r["matrix"], ref["matrix"]), rank
        _assert_lists(r["lists"], ref["lists"], rank)


def test_the_count_then_fill_protocol_and_the_pair_limit():
    _, ref = _reference("tiny")
    P = ref["lists"]["pairs"]

    def body(gr, rank):
        out = dict(count_only=gr.surfel_observations(prefill=FILL, residuals=(), keyframes=False, capacity=0),
                   short=gr.surfel_observations(prefill=FILL, capacity=P - 1),
                   no_payload=gr.surfel_observations(prefill=FILL, capacity=P + 5, residuals=()))
        return out

    def limited(gr, rank):
        try:
            gr.surfel_observations(prefill=FILL, capacity=P)
            return dict(limit=None)
        except capi.BackendError as e:
            return dict(limit=(str(e), e.arrays))

    A, results, calls = _tiny_pair(body)
    E = len(tm.table(A)[1])
    assert calls == 3 * tm.table_exchanges(E)                  # no call of these exchanges a payload
    capi.check(capi.load().bahip_debug_set_observations_shape(0, 0, 0, -1, P - 1))          # (process-wide: set before the ranks start)
    _, limited_results, calls = _tiny_pair(limited)
    assert calls == tm.table_exchanges(E)                      # P is global: every rank fails alike, after the table
    for r, extra in zip(results, limited_results):
        r.update(limit=extra["limit"])
    for rank, r in enumerate(results):
        assert r["count_only"]["pairs"] == P and np.array_equal(r["count_only"]["surfel_first"], ref["lists"]["surfel_first"]), rank
        assert r["short"]["pairs"] == P, rank
        for name in ("keyframes", "depth_raw", "descriptor_raw"):
            assert (r["short"][name].view(np.uint8) == FILL).all(), (rank, name)
        assert np.array_equal(r["no_payload"]["keyframes"][:P], ref["lists"]["keyframes"]), rank
        assert (r["no_payload"]["keyframes"][P:].view(np.uint8) == FILL).all(), rank
        text, arrays = r["limit"]
        assert "more than the pair limit" in text and all((a.view(np.uint8) == FILL).all() for a in arrays.values()), rank


def test_a_failing_exchange_fails_the_call_only_and_nothing_is_left_behind():
    """Rank 0 of 2 alone, with a hook that adds nothing (as if the other rank listed nothing) and fails at one position."""
    g = _fresh("tiny")
    lib = g.ctx.lib
    state = dict(calls=0, fail_at=-1)

    def hook(_ptr, _count, _dtype, _stream, _user):
        state["calls"] += 1
        return 1 if state["calls"] - 1 == state["fail_at"] else 0

    keep = capi.ALLREDUCE_FN(hook)
    capi.check(lib.bahip_context_set_allreduce(g.ctx.handle, keep, None))
    g.set_keyframe_sharding(0, 2)
    g.bind_keyframes()

    def good():
        state.update(calls=0, fail_at=-1)
        return dict(matrix=g.observed_covisibility(prefill=FILL), histogram=g.keyframe_observer_histogram(16, prefill=FILL),
                    lists=g.surfel_observations(prefill=FILL))

    try:
        reference = good()
        assert reference["matrix"][0, 0] > 0 and not reference["matrix"][1].any()          # its own keyframes, its own tiles
        gc.collect()
        before = ll.live_allocations(lib)
        named = {"matrix": ("tile mask counts", "tile mask entries", "co-visibility words"),
                 "histogram": ("tile mask counts", "tile mask entries", "observer histogram words"),
                 "lists": ("tile mask counts", "tile mask entries", "observation payload", "observation payload")}
        call = {"matrix": lambda: g.observed_covisibility(prefill=FILL), "histogram": lambda: g.keyframe_observer_histogram(16, prefill=FILL),
                "lists": lambda: g.surfel_observations(prefill=FILL, capacity=reference["lists"]["pairs"])}
        for which, names in named.items():
            for position, name in enumerate(names):
                state.update(calls=0, fail_at=position)
                with pytest.raises(capi.BackendError, match=name) as refused:
                    call[which]()
                assert state["calls"] == position + 1, (which, position)
                if which != "lists":
                    assert (refused.value.arrays == FILL_WORD).all(), (which, position)
                again = good()
                assert np.array_equal(again["matrix"], reference["matrix"]) and np.array_equal(again["histogram"], reference["histogram"])
                _assert_lists(again["lists"], reference["lists"], (which, position))
        gc.collect()
        assert ll.live_allocations(lib) == before
    finally:
        g.set_keyframe_sharding(0, 1)
        capi.check(lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
