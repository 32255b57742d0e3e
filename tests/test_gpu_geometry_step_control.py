"""The geometry phase of the alternating scheme under step control on the GPU (bahip_optimize_geometry_iteration_controlled;
kernels_geometry_trial.hip, DESIGN.md section 3, "Step control of the geometry phase").

Held to: the plain step at lambda 0 (flags, normals, words, and the per-surfel sums through the numpy restatement of the solve); a
controlled step played by hand through entry points that existed before (tests/geometry_step_control.py: by_hand), word for word; the
property the control exists for -- no surfel's cost rises; and the bits it must not touch.  Scene states T0 / T2 of `tiny` (1 142
surfels): tests/test_cpu_geometry_step_control.py holds the conditions under which they exercise anything.  Every call's outcome
buffer is filled with 0xEE bytes first: an entry the call did not write shows."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi, multigpu
from tests import geometry_step_control as gsc
from tests import surfel_costs as sc
from tests import two_cameras as tcam
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

ROWS = list(gsc.ROWS)
_CACHE = {}


def _gpu():
    """A GPU scene of its own with tiny's keyframes bound at the perturbed poses (the oracle's state T0)."""
    if "oracle" not in _CACHE:
        _CACHE["oracle"] = gsc.oracle_state("T0")
    return tcam.build_gpu(gsc.scene(), _CACHE["oracle"])


def _shared_gpu():
    if "gpu" not in _CACHE:
        _CACHE["gpu"] = _gpu()
    return _CACHE["gpu"]


def _words(rows):
    return np.ascontiguousarray(np.asarray(rows, np.float32)[ROWS]).view(np.uint32)


def _bits(rows):
    return np.ascontiguousarray(rows, np.float32).view(np.uint32)


def _call(g, rows, flags, ctl=None, use_depth=True, use_desc=True, activation="all", **kw):
    """Uploads the state, runs one controlled step; dict(rows (17, N), flags, outcome, stats)."""
    n = rows.shape[1]
    g.upload_surfels(rows, flags)
    outcome, stats = g.optimize_geometry_controlled(use_depth, use_desc, ctl, n if activation == "all" else activation, **kw)
    return dict(rows=g.download_surfels().copy(), flags=g.active_buf.download()[0, :n].copy(), outcome=outcome, stats=stats)


def _check_stats(res, max_trials=4):
    o, s = res["outcome"], res["stats"]
    assert not np.any(o == 0xEE), "an outcome entry was not written"
    assert set(np.unique(o).tolist()) <= set(range(0, max_trials + 1)) | {255}, np.unique(o)
    assert s["candidates"] == int(np.count_nonzero(o != 0)), (s, np.bincount(o))
    assert s["accepted"] == int(np.count_nonzero((o >= 1) & (o <= 254))) and s["restored"] == int(np.count_nonzero(o == 255)), s
    assert s["candidates"] == s["accepted"] + s["restored"], s
    assert 1 <= s["trials"] <= max_trials, s
    # every candidate is rejected once per trial it stayed open in
    t = s["trials"]
    rejections = int(sum(int(v) - 1 for v in o[(o >= 1) & (o <= 254)])) + t * s["restored"]
    assert s["rejected_cost"] + s["rejected_pairs"] == rejections, (s, rejections)


def _same(a, b, what=""):
    """Two results of _call equal word for word (rows, flags, outcome, stats)."""
    bad = np.argwhere(_bits(a["rows"]) != _bits(b["rows"]))
    assert bad.size == 0, (what, "rows", bad[:5].tolist())
    assert np.array_equal(a["flags"], b["flags"]), (what, "flags")
    assert np.array_equal(a["outcome"], b["outcome"]), (what, "outcome", np.flatnonzero(a["outcome"] != b["outcome"])[:5])
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])


def _reference(state, use_depth=True, use_desc=True, activation="all"):
    """The default-control result on state T0 / T2 (cached; do not change)."""
    key = ("ref", state, use_depth, use_desc, activation)
    if key not in _CACHE:
        rows, flags = gsc.state_arrays(state)
        _CACHE[key] = _call(_shared_gpu(), rows, flags, None, use_depth, use_desc, activation)
        _check_stats(_CACHE[key])
    return _CACHE[key]


def _s1_costs(g, rows, res, use_depth=True, use_desc=True):
    """c0 of a call: the cost of the pre-call rows with the post-call normal row (and flags, which the cost ignores)."""
    s1 = np.array(rows, np.float32)
    s1[3] = res["rows"][3]
    g.upload_surfels(s1, res["flags"])
    return g.evaluate_surfel_costs(use_depth, use_desc)


# ---- (1) lambda 0 is the plain step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_depth,use_desc", sc.KINDS)
@pytest.mark.parametrize("state", ["T0", "T2"])
def test_lambda_zero_is_the_plain_step(state, use_depth, use_desc):
    rows, flags = gsc.state_arrays(state)
    n = rows.shape[1]
    g = _shared_gpu()
    plain_rows, plain_flags = gsc.plain_step(g, rows, flags, use_depth, use_desc, n)
    res = _call(g, rows, flags, gsc.control(lambda_initial=0.0, max_trials=1, guard_pairs=0), use_depth, use_desc)
    _check_stats(res, 1)
    assert np.array_equal(res["flags"], plain_flags)
    assert np.array_equal(_bits(res["rows"][3]), _bits(plain_rows[3])), "normals"
    o = res["outcome"]
    kept = o == 1
    print(state, use_depth, use_desc, "outcomes", np.bincount(o, minlength=256)[[0, 1, 255]], res["stats"])
    assert kept.sum() >= 300 and set(np.unique(o).tolist()) <= {0, 1, 255}, np.bincount(o)
    assert np.array_equal(_words(res["rows"])[:, kept], _words(plain_rows)[:, kept]), "accepted surfels carry the plain step's words"
    assert np.array_equal(_words(res["rows"])[:, ~kept], _words(rows)[:, ~kept]), "every other surfel carries its old words"
    others = [r for r in range(rows.shape[0]) if r not in ROWS and r != 3]
    assert np.array_equal(_bits(res["rows"][others]), _bits(rows[others]))
    # the sums and the restated solve, pinned to the oracle-tested path
    sums = g.read_geometry_sums(8 if use_desc else 2)
    live = ((plain_flags & 1) != 0) & ~np.isnan(rows[0])
    cand = gsc.damped_solve(sums, _words(rows), gsc.unpack_normal10(_bits(plain_rows[3])), 0.0, use_desc)
    bad = np.flatnonzero((cand != _words(plain_rows)).any(axis=0) & live)
    assert bad.size == 0, (bad[:5], cand[:, bad[:2]], _words(plain_rows)[:, bad[:2]])
    assert live.sum() >= 1000 and (o[~live] == 0).all()


# ---- (2) the call is the by-hand sequence ---------------------------------------------------------------------------------------------------------
def _against_by_hand(g, rows, flags, ctl=None, use_depth=True, use_desc=True, activation="all"):
    n = rows.shape[1]
    res = _call(g, rows, flags, ctl, use_depth, use_desc, activation)
    sums = g.read_geometry_sums(8 if use_desc else 2)
    act = n if activation == "all" else (None if activation == -1 else activation)
    hand_rows, hand_flags, hand_outcome, hand_stats = gsc.by_hand(g, rows, flags, sums, gsc.control(**(ctl or {})), use_depth, use_desc, act)
    _same(res, dict(rows=hand_rows, flags=hand_flags, outcome=hand_outcome, stats=hand_stats), "by hand")
    return res


def test_the_call_is_the_by_hand_sequence_on_t2():
    """Measured on T2 with the default control, the real damped ladder 0, 1, 4, 16: outcome 0: 63 surfels, 1: 961, 2: 51, 3: 23, 4: 16,
    255 (restored): 28; 257 rejections by the cost test, none by the pair guard; total 4756.34 -> 4661.23 (a scaled-step estimate
    made before the kernel existed gave 961 / 38 / 30 / 17 accepted, 33 restored, 4661.20).  The counts are printed; each of the
    outcomes 1, 2, 3 and 255 must hold at least 5 surfels."""
    rows, flags = gsc.state_arrays("T2")
    res = _against_by_hand(_gpu(), rows, flags)
    _check_stats(res)
    hist = np.bincount(res["outcome"], minlength=256)
    print("T2 outcomes 0..4, 255:", hist[:5].tolist(), int(hist[255]), res["stats"])
    assert all(hist[v] >= 5 for v in (1, 2, 3, 255)), hist[[1, 2, 3, 4, 255]]


def test_the_call_is_the_by_hand_sequence_on_t0_and_the_guard_rejects():
    """Measured on T0: outcome 1: 1 132 surfels, 2: 5, 3: 3, 4: 1, 255: 1; 9 rejections by the cost test, 9 by the pair guard alone."""
    rows, flags = gsc.state_arrays("T0")
    res = _against_by_hand(_gpu(), rows, flags)
    _check_stats(res)
    print("T0 outcomes 0..4, 255:", np.bincount(res["outcome"], minlength=256)[[0, 1, 2, 3, 4, 255]].tolist(), res["stats"])
    assert res["stats"]["rejected_pairs"] >= 1, res["stats"]
    _same(res, _reference("T0"), "the shared reference")


@pytest.mark.parametrize("use_depth,use_desc", [(True, False), (False, True)])
def test_the_call_is_the_by_hand_sequence_for_one_residual_type(use_depth, use_desc):
    rows, flags = gsc.state_arrays("T2")
    res = _against_by_hand(_gpu(), rows, flags, dict(lambda_initial=0.5, lambda_up=3.0, lambda_min=0.25, max_trials=3), use_depth, use_desc)
    _check_stats(res, 3)
    assert res["stats"]["accepted"] >= 300, res["stats"]


# ---- (3) no surfel's cost rises ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["exact", "fast"])
@pytest.mark.parametrize("state", ["T0", "T2"])
def test_no_surfels_cost_rises(state, flavour):
    rows, flags = gsc.state_arrays(state)
    g = _gpu()
    g.ctx.set_arithmetic(flavour)
    try:
        res = _call(g, rows, flags)
        _check_stats(res)
        c0 = _s1_costs(g, rows, res)
        g.upload_surfels(res["rows"], res["flags"])
        c1 = g.evaluate_surfel_costs()
    finally:
        g.ctx.set_arithmetic("exact")
    f0, f1, o = gsc.objective(c0), gsc.objective(c1), res["outcome"]
    assert np.isfinite(f0).all() and np.isfinite(f1).all()
    untouched = (o == 0) | (o == 255)
    print(state, flavour, "total", float(f0.sum()), "->", float(f1.sum()), res["stats"])
    assert (f1 <= f0).all(), np.flatnonzero(f1 > f0)[:5]
    assert np.array_equal(f1[untouched], f0[untouched]) and (f1[~untouched] < f0[~untouched]).all()
    sc.assert_same_bits(sc.take(c1, untouched), sc.take(c0, untouched), "restored and untouched rows")
    for name in sc.COUNTS:      # the guard is on: no pair is lost
        assert (c1[name] >= c0[name]).all(), (name, np.flatnonzero(c1[name] < c0[name])[:5])
    assert (~untouched).sum() >= 500


def test_without_the_guard_pairs_may_go_but_no_cost_rises():
    rows, flags = gsc.state_arrays("T0")
    g = _gpu()
    res = _call(g, rows, flags, dict(guard_pairs=0))
    _check_stats(res)
    assert res["stats"]["rejected_pairs"] == 0
    c0 = _s1_costs(g, rows, res)
    g.upload_surfels(res["rows"], res["flags"])
    c1 = g.evaluate_surfel_costs()
    assert (gsc.objective(c1) <= gsc.objective(c0)).all()
    lost = (c1["depth_residuals"] < c0["depth_residuals"]) | (c1["descriptor_pairs"] < c0["descriptor_pairs"])
    assert lost.sum() >= 1                          # what the guard of the default control keeps from happening (5 by the CPU census)


# ---- (4) restored means every bit -------------------------------------------------------------------------------------------------------------------
def test_restored_and_untouched_surfels_keep_every_bit_and_nothing_else_is_written():
    rows, flags = gsc.state_arrays("T2")
    n = rows.shape[1]
    g = _gpu()
    rng = np.random.Generator(np.random.PCG64(11))
    full = rng.integers(0, 1 << 32, size=(capi.SURFEL_ATTRIBUTE_COUNT, g.capacity), dtype=np.uint64).astype(np.uint32)
    full[:8, :n] = _bits(rows[:8])                       # rows 8 .. 16 (scratch) and everything past surfels_size: random words
    active = rng.integers(0, 256, size=(1, g.capacity), dtype=np.uint64).astype(np.uint8)
    active[0, :n] = flags
    g.surfel_buf.upload(full.view(np.float32))
    g.active_buf.upload(active)
    g.surfels_size = g.surfel_count = n
    outcome, stats = g.optimize_geometry_controlled(True, True, None, n)
    after = g.surfel_buf.download().view(np.uint32)
    after_active = g.active_buf.download()
    ref = _reference("T2")
    assert np.array_equal(after[:8, :n], _bits(ref["rows"][:8])) and np.array_equal(after_active[0, :n], ref["flags"])
    assert np.array_equal(outcome, ref["outcome"]) and stats == ref["stats"]
    assert np.array_equal(after[:, n:], full[:, n:]) and np.array_equal(after_active[0, n:], active[0, n:]), "past surfels_size"
    assert np.array_equal(after[[4, 5]], full[[4, 5]]) and np.array_equal(after[8:], full[8:]), "rows 4, 5 and the scratch rows"
    still = (outcome == 0) | (outcome == 255)
    assert (outcome == 255).sum() >= 5 and (outcome == 0).sum() >= 5
    assert np.array_equal(after[ROWS][:, :n][:, still], full[ROWS][:, :n][:, still])


# ---- (5) edges --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1142])
def test_the_first_n_surfels_give_the_prefix(n):
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    res = _call(_shared_gpu(), np.ascontiguousarray(rows[:, :n]), flags[:n])
    _check_stats(res)
    assert np.array_equal(_bits(res["rows"]), _bits(ref["rows"][:, :n])) and np.array_equal(res["outcome"], ref["outcome"][:n])
    assert np.array_equal(res["flags"], ref["flags"][:n])


def test_deleted_surfels_and_a_deleted_tile_are_untouched():
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    gone = np.zeros(rows.shape[1], bool)
    gone[100] = True
    gone[192:256] = True
    assert np.count_nonzero(ref["outcome"][gone]) > 32
    mine = rows.copy()
    mine[0, gone] = np.nan
    res = _call(_shared_gpu(), mine, flags)
    _check_stats(res)
    assert (res["outcome"][gone] == 0).all() and (res["flags"][gone] & 1 == 0).all()
    assert np.array_equal(_bits(res["rows"][:, gone]), _bits(mine[:, gone]))
    assert np.array_equal(_bits(res["rows"][:, ~gone]), _bits(ref["rows"][:, ~gone])) and np.array_equal(res["outcome"][~gone], ref["outcome"][~gone])


def test_an_inactive_surfel_is_untouched_when_the_flags_are_kept():
    rows, flags = gsc.state_arrays("T2")
    assert (flags & 1).sum() >= 1000
    ref = _reference("T2", activation=-1)
    off = np.zeros(rows.shape[1], bool)
    moved = np.flatnonzero(ref["outcome"] != 0)
    off[[moved[5], moved[moved >= 64][0], moved[-1]]] = True          # surfels the reference call moved or tried to move
    mine = flags.copy()
    mine[off] = 0
    res = _call(_shared_gpu(), rows, mine, activation=-1)
    _check_stats(res)
    assert (res["outcome"][off] == 0).all() and (res["flags"][off] == 0).all()
    assert np.array_equal(_bits(res["rows"][:, off]), _bits(rows[:, off])), "not even the normal of an inactive surfel moves"
    assert np.array_equal(_bits(res["rows"][:, ~off]), _bits(ref["rows"][:, ~off])) and np.array_equal(res["outcome"][~off], ref["outcome"][~off])
    # and with the flags decided by the call they are active again: the reference of the whole range
    _same(_call(_shared_gpu(), rows, mine), _reference("T2"), "flags decided by the call")


def test_an_inactive_keyframe_is_not_swept_for_the_sums_but_counts_in_the_cost():
    rows, flags = gsc.state_arrays("T2")
    g = _gpu()
    g.keyframes[3]["activation"] = capi.KF_INACTIVE
    g.bind_keyframes()
    res = _against_by_hand(g, rows, flags)
    _check_stats(res)
    assert res["stats"]["accepted"] >= 300
    assert not np.array_equal(res["outcome"], _reference("T2")["outcome"])
    # the cost the decisions were taken from is the cost over all four keyframes
    total, per = g.evaluate_cost()
    assert per[3]["depth_residuals"] > 0
    sc.assert_consistent_with_cost(g.evaluate_surfel_costs(), total, "all bound keyframes")


def test_one_bound_keyframe():
    rows, flags = gsc.state_arrays("T2")
    g = _gpu()
    g.keyframes = [g.keyframes[2]]
    g.bind_keyframes()
    res = _against_by_hand(g, rows, flags)
    _check_stats(res)
    assert res["stats"]["candidates"] >= 100 and (res["outcome"] == 0).sum() >= 100


def test_no_bound_keyframe_gives_outcome_zero_everywhere():
    rows, flags = gsc.state_arrays("T2")
    g = _gpu()
    g.keyframes = []
    g.bind_keyframes()
    res = _call(g, rows, flags, activation=-1)
    assert (res["outcome"] == 0).all() and np.array_equal(_bits(res["rows"]), _bits(rows)) and np.array_equal(res["flags"], flags)
    assert [res["stats"][k] for k in ("candidates", "accepted", "restored", "rejected_cost", "rejected_pairs")] == [0] * 5
    res = _call(g, rows, flags)                          # the flags decided: no keyframe sees anything
    assert (res["outcome"] == 0).all() and np.array_equal(_bits(res["rows"]), _bits(rows)) and (res["flags"] & 1 == 0).all()


def test_a_nan_descriptor_ends_restored_and_no_other_surfel_is_touched():
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    g = _shared_gpu()
    g.upload_surfels(rows, flags)
    pairs = g.evaluate_surfel_costs()["descriptor_pairs"]
    victim = int(np.flatnonzero((pairs >= 1) & (ref["outcome"] != 0))[3])
    mine = rows.copy()
    mine[6, victim] = np.nan
    res = _call(g, mine, flags)
    _check_stats(res)
    others = np.arange(rows.shape[1]) != victim
    assert res["outcome"][victim] == 255
    assert np.array_equal(_bits(res["rows"][ROWS, victim]), _bits(mine[ROWS, victim]))
    assert np.array_equal(_bits(res["rows"][:, others]), _bits(ref["rows"][:, others])) and np.array_equal(res["outcome"][others], ref["outcome"][others])
    assert res["stats"]["rejected_cost"] >= 4


def test_outcome_and_stats_may_be_null():
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    g = _shared_gpu()
    for want_outcome, want_stats in ((False, False), (True, False), (False, True)):
        res = _call(g, rows, flags, want_outcome=want_outcome, want_stats=want_stats)
        assert np.array_equal(_bits(res["rows"]), _bits(ref["rows"])) and np.array_equal(res["flags"], ref["flags"])
        assert (res["outcome"] is None) == (not want_outcome) and (res["stats"] is None) == (not want_stats)
        if want_outcome:
            assert np.array_equal(res["outcome"], ref["outcome"])
        if want_stats:
            assert res["stats"] == ref["stats"]


def test_bad_arguments_are_refused_and_the_context_stays_usable():
    rows, flags = gsc.state_arrays("T2")
    g = _gpu()
    nan, inf = float("nan"), float("inf")
    bad = [dict(lambda_initial=-1.0), dict(lambda_initial=nan), dict(lambda_initial=inf), dict(lambda_up=1.0), dict(lambda_up=inf),
           dict(lambda_up=nan), dict(lambda_min=0.0), dict(lambda_min=nan), dict(lambda_min=2.0, lambda_max=1.0), dict(lambda_max=inf),
           dict(max_trials=0), dict(max_trials=-3), dict(max_trials=255)]
    for fields in bad:
        g.upload_surfels(rows, flags)
        with pytest.raises(capi.BackendError, match="bahip_optimize_geometry_iteration_controlled"):
            g.optimize_geometry_controlled(True, True, fields, rows.shape[1])
        assert np.array_equal(_bits(g.download_surfels()), _bits(rows)), fields
    with pytest.raises(capi.BackendError, match="at least one residual type"):
        g.optimize_geometry_controlled(False, False, None, rows.shape[1])
    with pytest.raises(capi.BackendError, match="activation range"):
        g.optimize_geometry_controlled(True, True, None, rows.shape[1] + 1)
    with pytest.raises(capi.BackendError, match="activation range"):
        g.optimize_geometry_controlled(True, True, None, -2)
    _same(_call(g, rows, flags), _reference("T2"), "after the refusals")
    fresh = _gpu()
    with pytest.raises(capi.BackendError, match="no controlled geometry step"):
        fresh.read_geometry_sums(8)


# ---- (6) invariance -----------------------------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_move_with_the_cost_sweeps_shape_or_the_tile_order():
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    g = _gpu()
    lib = capi.load()
    g.upload_surfels(rows, flags)
    poses = [kf["pose"].copy() for kf in g.keyframes]
    g.estimate_keyframe_poses(True, True)        # a pose phase over the table leaves the heavy-first run order behind
    for kf, T in zip(g.keyframes, poses):
        kf["pose"] = T
    g.bind_keyframes()
    _same(_call(g, rows, flags), ref, "after a pose phase")
    try:
        for waves, workgroups, tile_order in [(8, 0, 1), (4, 37, 0), (2, 5, 1), (1, 1, 0)]:
            capi.check(lib.bahip_debug_set_surfel_cost_shape(waves, workgroups, 0, tile_order))
            _same(_call(g, rows, flags), ref, (waves, workgroups, tile_order))
        capi.check(lib.bahip_debug_set_surfel_cost_shape(0, 0, 0, -1))
        capi.check(lib.bahip_debug_set_tile_order(0))
        _same(_call(g, rows, flags), ref, "buffer order")
    finally:
        capi.check(lib.bahip_debug_set_surfel_cost_shape(0, 0, 0, -1))
        capi.check(lib.bahip_debug_set_tile_order(1))


def test_permuted_surfels_permute_rows_and_outcomes():
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    perm = np.random.Generator(np.random.PCG64(8)).permutation(rows.shape[1])
    res = _call(_shared_gpu(), np.ascontiguousarray(rows[:, perm]), flags[perm])
    assert np.array_equal(_bits(res["rows"]), _bits(ref["rows"][:, perm])) and np.array_equal(res["outcome"], ref["outcome"][perm])
    assert np.array_equal(res["flags"], ref["flags"][perm]) and res["stats"] == ref["stats"]


# ---- (7) sharding -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
def test_keyframe_shards_end_with_the_unsharded_rows_outcomes_and_stats(world):
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    _gpu()                                                       # (the oracle of the cache is built on this thread)

    def rank_main(rank, hook):
        gr = _gpu()
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
        res = _call(gr, rows, flags)
        res["keep"] = (hook, gr)
        return res

    results, loop = _run_ranks(world, rank_main)
    for rank, r in enumerate(results):
        _same(r, ref, rank)
    # two exchanges for the sums, one per cost sweep (the slice holds the whole cloud): c0 and one per trial
    assert loop.calls == 2 + 1 + ref["stats"]["trials"], (loop.calls, ref["stats"])


def test_surfel_shards_give_the_unsharded_slices_and_exchange_nothing():
    rows, flags = gsc.state_arrays("T2")
    ref = _reference("T2")
    n, world = rows.shape[1], 2
    _gpu()

    def rank_main(rank, hook):
        gr = _gpu()
        mine = multigpu.shard_chunks(n, rank, world, chunk=64)
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        res = _call(gr, np.ascontiguousarray(rows[:, mine]), flags[mine])
        _check_stats(res)
        res.update(mine=mine, keep=(hook, gr))
        return res

    results, loop = _run_ranks(world, rank_main)
    assert sum(int(r["mine"].size) for r in results) == n
    for rank, r in enumerate(results):
        mine = r["mine"]
        assert np.array_equal(_bits(r["rows"]), _bits(ref["rows"][:, mine])), rank
        assert np.array_equal(r["outcome"], ref["outcome"][mine]) and np.array_equal(r["flags"], ref["flags"][mine]), rank
    assert loop.calls == 0


@pytest.mark.parametrize("fail_at", [0, 1, 2, 3, 4])
def test_a_failing_exchange_fails_the_call_puts_the_saved_words_back_and_the_next_call_succeeds(fail_at):
    """Exchanges of a call at world 2: 0 and 1 carry the sums, 2 the cost before, 3 and 4 the costs of trials 0 and 1 -- inside the
    loop, where candidates are in the rows when the exchange fails."""
    rows, flags = gsc.state_arrays("T2")
    g = _gpu()
    calls = []

    def hook(buf, count, dtype, stream, user):                     # a lone rank of two: its own words are the sum
        calls.append(count)
        return 1 if len(calls) - 1 == fail_at else 0

    failing = capi.ALLREDUCE_FN(hook)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, failing, None))
    g.set_keyframe_sharding(0, 2)
    g.kf_shard = (0, 1)
    g.bind_keyframes()
    try:
        g.upload_surfels(rows, flags)
        with pytest.raises(capi.BackendError):
            g.optimize_geometry_controlled(True, True, None, rows.shape[1])
        assert len(calls) == fail_at + 1
        after = g.download_surfels()
        assert np.array_equal(_words(after), _words(rows)), "the saved words are back"
        others = [r for r in range(rows.shape[0]) if r not in ROWS and r != 3]
        assert np.array_equal(_bits(after[others]), _bits(rows[others]))
    finally:
        g.set_keyframe_sharding(0, 1)
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
        g.bind_keyframes()
    _same(_call(g, rows, flags), _reference("T2"), "after the failed call")
