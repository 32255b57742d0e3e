"""The value of the BA objective per surfel on the GPU (bahip_evaluate_surfel_costs; kernels_surfel_cost.hip, DESIGN.md section 3, "The
objective per surfel").

Definition: for every surfel the depth terms 1 * TukeyCost(raw, 10) and -- where the colour pixel is valid -- the two descriptor terms
1e-2 * HuberCost(raw, 10) over every bound keyframe the production rule associates it with; each of the three sums the exact sum of its
binary32 terms rounded once to binary64, plus the two counts.  So the planes are checked BIT FOR BIT against the CPU model of
tests/surfel_costs.py (the oracle's per-pair words, the robust costs in binary32, math.fsum per surfel; tests/test_cpu_surfel_costs.py
holds that model to the oracle's total), against bahip_evaluate_cost, and must not move with the launch shape, the tile order, the
surfel order, the keyframe order or the sharding.  Scenes: tests/two_cameras.py (colour camera != depth camera: colour-invalid pairs and
border samples inside the tiles).  Every call's output planes are filled with 0xFF bytes first: an entry the call did not write shows."""
import ctypes as C
import math

import numpy as np
import pytest

from badslam_amd import capi, multigpu
from tests import surfel_costs as sc
from tests import two_cameras as tcam
from tests.test_gpu_cost import _pair_terms
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

_WORLD = {}
SHAPES = [(1, 1, 0), (8, 0, 1), (4, 37, 0), (2, 5, 1), (1, 1000, 1), (8, 0, 0), (4, 37, 1), (2, 5, 0), (1, 1, 1), (1, 1000, 0)]   # waves, workgroups, tile order


def _world(name):
    """(scene, an oracle nobody changes, its pair words, a GPU scene in the oracle's state that every test leaves as it found it)."""
    if name not in _WORLD:
        tc = tcam.build_scene(name)
        ba = tcam.build_oracle(tc)
        _WORLD[name] = (tc, ba, sc.oracle_pair_words(ba), tcam.build_gpu(tc, ba))
    return _WORLD[name]


def _fresh_tiny():
    """A GPU scene of its own in tiny's state (for the tests that upload other surfels or change the context)."""
    tc, ba, _, _ = _world("tiny")
    return tcam.build_gpu(tc, ba)


def _eval(g, use_depth=True, use_desc=True, planes=None):
    return g.evaluate_surfel_costs(use_depth, use_desc, planes=planes, prefill=0xFF)


def _set_shape(waves=0, workgroups=0, slice_surfels=0, tile_order=-1):
    capi.check(capi.load().bahip_debug_set_surfel_cost_shape(waves, workgroups, slice_surfels, tile_order))


def _reference(name, use_depth=True, use_desc=True):
    key = ("ref", name, use_depth, use_desc)
    if key not in _WORLD:
        _WORLD[key] = _eval(_world(name)[3], use_depth, use_desc)
    return _WORLD[key]


def _zero_rows(n):
    out = {name: np.zeros(n, np.float64) for name in sc.SUMS}
    out.update({name: np.zeros(n, np.uint32) for name in sc.COUNTS})
    return out


def _with_keyframes(g, keyframes):
    """Binds the given subset / order of g's keyframes; returns the list to restore."""
    kept = g.keyframes
    g.keyframes = list(keyframes)
    g.bind_keyframes()
    return kept


# ---- (1) the oracle's bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_depth,use_desc", sc.KINDS)
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_planes_are_the_cpu_models_bits(name, use_depth, use_desc):
    tc, ba, words, g = _world(name)
    got = _eval(g, use_depth, use_desc)
    expected = sc.model(words, use_depth, use_desc)
    t = sc.totals(expected)
    assert t["depth_residuals"] + t["descriptor_pairs"] > 1000, t
    assert (t["depth_residuals"] > 0) == use_depth and (t["descriptor_pairs"] > 0) == use_desc, t
    sc.assert_same_bits(got, expected, (name, use_depth, use_desc))


# ---- (2) consistency with bahip_evaluate_cost -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_depth,use_desc", sc.KINDS)
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_planes_sum_to_the_cost_in_total_and_per_keyframe(name, use_depth, use_desc):
    tc, ba, words, g = _world(name)
    total, per = g.evaluate_cost(use_depth, use_desc)
    print("total", total, sc.totals(_reference(name, use_depth, use_desc)))
    sc.assert_consistent_with_cost(_reference(name, use_depth, use_desc), total, (name, "total"))
    all_keyframes = g.keyframes
    try:
        for k, kf in enumerate(all_keyframes):
            _with_keyframes(g, [kf])
            planes = _eval(g, use_depth, use_desc)
            print("keyframe", k, per[k], sc.totals(planes))
            sc.assert_consistent_with_cost(planes, per[k], (name, k))
            sc.assert_same_bits(planes, sc.model(words[k:k + 1], use_depth, use_desc), (name, "only keyframe", k))
    finally:
        _with_keyframes(g, all_keyframes)


# ---- (3) edge shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1142])
def test_the_first_n_surfels_give_the_prefix(n):
    ref = _reference("tiny")
    g = _fresh_tiny()
    data = g.download_surfels().copy()
    assert data.shape[1] == 1142
    g.upload_surfels(np.ascontiguousarray(data[:, :n]), np.ones(n, np.uint8))
    sc.assert_same_bits(_eval(g), sc.take(ref, slice(0, n)), n)


def test_deleted_surfels_and_a_deleted_tile_give_zero_rows_and_touch_nothing_else():
    ref = _reference("tiny")
    g = _fresh_tiny()
    data = g.download_surfels().copy()
    gone = np.zeros(data.shape[1], bool)
    gone[100] = True                  # one surfel inside tile 1
    gone[192:256] = True              # tile 3 as a whole
    assert ref["depth_residuals"][100] > 0 and np.count_nonzero(ref["depth_residuals"][192:256]) > 32
    data[0, gone] = np.nan
    g.upload_surfels(data, np.ones(data.shape[1], np.uint8))
    got = _eval(g)
    sc.assert_same_bits(sc.take(got, gone), _zero_rows(int(gone.sum())), "deleted rows")
    sc.assert_same_bits(sc.take(got, ~gone), sc.take(ref, ~gone), "the other rows")


def test_a_nan_descriptor_poisons_exactly_its_own_row():
    tc, ba, words, _ = _world("tiny")
    ref = _reference("tiny")
    g = _fresh_tiny()
    data = g.download_surfels().copy()
    K = len(g.keyframes)
    pairs = ref["descriptor_pairs"]
    victim = int(np.flatnonzero((pairs >= 1) & (pairs < K))[0])          # seen by some keyframes, not by all
    data[capi.SURFEL_DESCRIPTOR1, victim] = np.nan
    g.upload_surfels(data, np.ones(data.shape[1], np.uint8))
    got = _eval(g)
    assert all(math.isnan(got[name][victim]) for name in sc.SUMS), [got[name][victim] for name in sc.SUMS]
    expected = {name: a.copy() for name, a in ref.items()}
    for name in sc.SUMS:
        expected[name][victim] = np.nan                                 # the counts still count: the model's
    sc.assert_same_bits(got, expected, "poisoned row")
    assert got["depth_residuals"][victim] == sc.model(words, True, True)["depth_residuals"][victim] > 0


def test_a_null_plane_is_skipped_and_the_others_are_written():
    _, _, _, g = _world("tiny")
    ref = _reference("tiny")
    for wanted in (["depth", "descriptor_pairs"], ["descriptor_1", "descriptor_2", "depth_residuals"], ["descriptor_2"]):
        got = _eval(g, planes=wanted)
        assert sorted(got) == sorted(wanted)
        sc.assert_same_bits(got, {name: ref[name] for name in wanted}, wanted)
    sc.assert_same_bits(_eval(g), ref, "all planes again")


def test_one_bound_keyframe():
    tc, ba, words, g = _world("tiny")
    all_keyframes = g.keyframes
    try:
        _with_keyframes(g, [all_keyframes[2]])
        got = _eval(g)
    finally:
        _with_keyframes(g, all_keyframes)
    expected = sc.model(words[2:3], True, True)
    assert sc.census(expected, 1)["none"] > 100          # surfels no bound keyframe sees: zero rows, written
    sc.assert_same_bits(got, expected, "keyframe 2 alone")


def test_no_surfels_no_keyframes_and_no_residual_type_give_zeros():
    g = _fresh_tiny()
    n = g.surfels_size
    assert all(_eval(g, False, False)[name].shape == (n,) for name in sc.PLANES)
    sc.assert_same_bits(_eval(g, False, False), _zero_rows(n), "both switches off")
    all_keyframes = g.keyframes
    _with_keyframes(g, [])
    sc.assert_same_bits(_eval(g), _zero_rows(n), "no bound keyframe")
    _with_keyframes(g, all_keyframes)
    data = g.download_surfels().copy()
    g.upload_surfels(np.ascontiguousarray(data[:, :0]), np.ones(0, np.uint8))
    got = _eval(g)
    assert all(got[name].shape == (0,) for name in sc.PLANES), {name: a.shape for name, a in got.items()}


# ---- (4) invariance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_same_bits_across_calls_shapes_and_tile_orders(name):
    tc, ba, words, _ = _world(name)
    ref = _reference(name)
    g = tcam.build_gpu(tc, ba)
    poses = [kf["pose"].copy() for kf in g.keyframes]
    g.estimate_keyframe_poses(True, True)        # a pose phase over the table leaves the heavy-first run order behind
    for kf, T in zip(g.keyframes, poses):
        kf["pose"] = T
    g.bind_keyframes()
    sc.assert_same_bits(_eval(g), ref, "after a pose phase")
    sc.assert_same_bits(_eval(g), ref, "again")
    try:
        for waves, workgroups, tile_order in SHAPES:
            _set_shape(waves, workgroups, 0, tile_order)
            sc.assert_same_bits(_eval(g), ref, (waves, workgroups, tile_order))
    finally:
        _set_shape()


def test_permuted_surfels_permute_the_planes():
    ref = _reference("tiny")
    g = _fresh_tiny()
    data = g.download_surfels().copy()
    perm = np.random.Generator(np.random.PCG64(8)).permutation(data.shape[1])
    g.upload_surfels(np.ascontiguousarray(data[:, perm]), np.ones(data.shape[1], np.uint8))
    sc.assert_same_bits(_eval(g), sc.take(ref, perm), "permuted")


def test_the_keyframe_order_does_not_matter():
    _, _, _, g = _world("tiny")
    ref = _reference("tiny")
    all_keyframes = g.keyframes
    order = [int(k) for k in np.random.Generator(np.random.PCG64(5)).permutation(len(all_keyframes))]
    assert order != sorted(order)
    try:
        _with_keyframes(g, all_keyframes[::-1])
        sc.assert_same_bits(_eval(g), ref, "reversed")
        _with_keyframes(g, [all_keyframes[k] for k in order])
        sc.assert_same_bits(_eval(g), ref, order)
    finally:
        _with_keyframes(g, all_keyframes)


def test_moving_one_surfel_changes_its_row_only():
    ref = _reference("tiny")
    g = _fresh_tiny()
    data = g.download_surfels().copy()
    victim = int(np.flatnonzero(ref["depth_residuals"] == len(g.keyframes))[7])
    normal = tcam._unpack_normal10(np.ascontiguousarray(data[3, victim:victim + 1]).view(np.uint32))[:, 0]
    data[0:3, victim] += (0.05 * normal).astype(np.float32)          # 5 cm along its normal
    g.upload_surfels(data, np.ones(data.shape[1], np.uint8))
    got = _eval(g)
    others = np.arange(data.shape[1]) != victim
    sc.assert_same_bits(sc.take(got, others), sc.take(ref, others), "the other rows")
    mine, before = sc.bits(sc.take(got, ~others)), sc.bits(sc.take(ref, ~others))
    assert any(a[0] != b[0] for a, b in zip(mine, before)), (victim, mine, before)


# ---- (5) the fast flavour -----------------------------------------------------------------------------------------------------------------
def test_the_fast_flavour_is_deterministic_and_close_to_the_exact_one():
    tc, ba, words, _ = _world("crop_small")
    exact = _reference("crop_small")
    g = tcam.build_gpu(tc, ba)
    g.ctx.set_arithmetic("fast")
    try:
        fast = _eval(g)
        sc.assert_same_bits(_eval(g), fast, "fast again")
        for waves, workgroups, tile_order in SHAPES[:5]:
            _set_shape(waves, workgroups, 0, tile_order)
            sc.assert_same_bits(_eval(g), fast, ("fast", waves, workgroups, tile_order))
    finally:
        _set_shape()
        g.ctx.set_arithmetic("exact")
    sc.assert_same_bits(_eval(g), exact, "back to exact")
    # The rule of tests/test_gpu_cost.py::test_the_fast_flavour_is_deterministic_and_close_to_the_exact_one on the sums over the surfels:
    # the flavours may decide a few associations differently (at most 1e-3 of the pairs); those pairs, counted from the per-pair hook
    # of both flavours, are the only slack beyond 1e-5 relative -- each moves a sum by at most its largest term.
    e, f = sc.totals(exact), sc.totals(fast)
    ex, fa = _pair_terms(g, False), _pair_terms(g, True)
    depth_flips = sum(int(np.count_nonzero(a[0] != b[0])) for a, b in zip(ex, fa))
    desc_flips = sum(int(np.count_nonzero(a[1] != b[1])) for a, b in zip(ex, fa))
    desc_max = max(max(a[2], b[2]) for a, b in zip(ex, fa))
    print("flips", depth_flips, desc_flips, "exact", e, "fast", f)
    assert depth_flips <= 1e-3 * e["depth_residuals"] and desc_flips <= 1e-3 * e["descriptor_pairs"], (depth_flips, desc_flips)
    assert abs(f["depth_residuals"] - e["depth_residuals"]) <= depth_flips
    assert abs(f["descriptor_pairs"] - e["descriptor_pairs"]) <= desc_flips
    for n, slack in (("depth", depth_flips * 100.0 / 6.0), ("descriptor_1", desc_flips * desc_max), ("descriptor_2", desc_flips * desc_max)):
        assert abs(f[n] - e[n]) <= 1e-5 * abs(e[n]) + slack, (n, f[n], e[n], slack)


# ---- (6) surfel sharding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,count", [(2, 1142), (8, 7 * 64)])
def test_surfel_shards_give_their_rows_and_exchange_nothing(world, count):
    """Chunks of 64 surfels dealt over the ranks.  Eight ranks share the first 7 x 64 surfels: the last rank's shard is empty."""
    tc, ba, words, _ = _world("tiny")
    g = _fresh_tiny()
    data = g.download_surfels().copy()[:, :count]
    g.upload_surfels(np.ascontiguousarray(data), np.ones(count, np.uint8))
    ref = _eval(g)
    sc.assert_same_bits(ref, sc.take(_reference("tiny"), slice(0, count)), "the cloud the ranks share")

    def rank_main(rank, hook):
        gr = tcam.build_gpu(tc, ba)
        mine = multigpu.shard_chunks(count, rank, world, chunk=64)
        gr.upload_surfels(np.ascontiguousarray(data[:, mine]), np.ones(mine.size, np.uint8))
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        return dict(mine=mine, planes=_eval(gr), keep=(hook, gr))

    results, loop = _run_ranks(world, rank_main)
    sizes = [int(r["mine"].size) for r in results]
    assert sum(sizes) == count and min(sizes[:-1]) > 0, sizes
    if world == 8:
        assert sizes[-1] == 0, sizes
    for rank, r in enumerate(results):
        sc.assert_same_bits(r["planes"], sc.take(ref, r["mine"]), rank)
    assert loop.calls == 0


# ---- (7) keyframe sharding ----------------------------------------------------------------------------------------------------------------
def _keyframe_sharded(world, slice_surfels):
    tc, ba, words, _ = _world("tiny")
    ref = _reference("tiny")

    def rank_main(rank, hook):
        gr = tcam.build_gpu(tc, ba)
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        gr.set_keyframe_sharding(rank, world)
        rng = np.random.Generator(np.random.PCG64(3 + rank))
        for k in range(len(gr.keyframes)):                        # other ranks' keyframes: scrambled images, and handed over
            if k % world != rank:
                for which in ("depth", "normals", "radius"):
                    buf = gr.keyframes[k][which]
                    buf.upload(rng.integers(0, 1 << 16, size=(buf.height, buf.width), dtype=np.uint16))
        gr.kf_shard = (0, 1)                                       # (bind_keyframes then passes every frame's pointers)
        gr.bind_keyframes()
        return dict(planes=_eval(gr), depth_only=_eval(gr, True, False, planes=["depth", "depth_residuals"]), keep=(hook, gr))

    _set_shape(0, 0, slice_surfels, -1)
    try:
        results, loop = _run_ranks(world, rank_main)
    finally:
        _set_shape()
    for rank, r in enumerate(results):
        sc.assert_same_bits(r["planes"], ref, rank)
        sc.assert_same_bits(r["depth_only"], {n: _reference("tiny", True, False)[n] for n in ("depth", "depth_residuals")}, rank)
    return loop.calls


@pytest.mark.parametrize("world", [2, 4])
def test_keyframe_shards_give_the_unsharded_bits_with_one_exchange(world):
    assert _keyframe_sharded(world, 0) == 2                        # two calls per rank, the default slice: one exchange each


def test_keyframe_shards_exchange_once_per_slice():
    assert _keyframe_sharded(2, 256) == 2 * 5                      # 1 142 surfels in slices of 256: five exchanges per call


def test_a_failing_exchange_fails_the_call_and_leaves_the_context_usable():
    ref = _reference("tiny")
    g = _fresh_tiny()
    failing = capi.ALLREDUCE_FN(lambda *_: 1)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, failing, None))
    g.set_keyframe_sharding(0, 2)
    g.kf_shard = (0, 1)
    g.bind_keyframes()
    try:
        with pytest.raises(capi.BackendError, match="surfel cost rows over the ranks"):
            _eval(g)
    finally:
        g.set_keyframe_sharding(0, 1)
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
        g.bind_keyframes()
    sc.assert_same_bits(_eval(g), ref, "after the failed call")
