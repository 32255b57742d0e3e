"""The parts of the geometry phase's step control that need no GPU (tests/geometry_step_control.py): the ladder arithmetic, the decide
rule on hand-made rows, and the census conditions on the oracle that make the GPU tests meaningful.  (The numpy solve at lambda 0 is
held to the plain step on the GPU, where the per-surfel sums come from: tests/test_gpu_geometry_step_control.py.)"""
import numpy as np

from tests import geometry_step_control as gsc

F32 = np.float32


# ---- the ladder ---------------------------------------------------------------------------------------------------------------------------
def test_the_default_ladder_is_0_1_4_16():
    assert [float(v) for v in gsc.ladder(gsc.DEFAULTS)] == [0.0, 1.0, 4.0, 16.0]
    assert all(isinstance(v, np.float32) for v in gsc.ladder(gsc.DEFAULTS))


def test_the_ladder_clamps_to_min_and_max_in_binary32():
    # 0.1f * 3 is not 0.3f: every rung is the binary32 product of the rung before
    got = gsc.ladder(gsc.control(lambda_initial=0.1, lambda_up=3.0, lambda_min=0.05, lambda_max=2.5, max_trials=6))
    expected = [F32(0.1)]
    for _ in range(5):
        expected.append(min(max(F32(expected[-1] * F32(3.0)), F32(0.05)), F32(2.5)))
    assert [v.tobytes() for v in got] == [v.tobytes() for v in expected]
    assert float(got[1]) != 0.1 * 3 and float(got[-1]) == 2.5 and float(got[-2]) == 2.5
    # from 0 the first non-zero rung is lambda_min; a small positive start is lifted to it as well
    assert [float(v) for v in gsc.ladder(gsc.control(lambda_min=0.5, max_trials=3))] == [0.0, 0.5, 2.0]
    assert [float(v) for v in gsc.ladder(gsc.control(lambda_initial=1e-3, lambda_min=0.5, max_trials=2))] == [float(F32(1e-3)), 0.5]
    # an overflowing product ends at lambda_max
    top = gsc.ladder(gsc.control(lambda_initial=3e38, lambda_up=4.0, lambda_max=3.2e38, max_trials=2))
    assert float(top[1]) == float(F32(3.2e38))
    assert len(gsc.ladder(gsc.control(max_trials=1))) == 1


# ---- the decide rule ------------------------------------------------------------------------------------------------------------------------
def _planes(rows):
    """rows: (depth, descriptor_1, descriptor_2, depth_residuals, descriptor_pairs) per surfel."""
    a = np.array(rows, np.float64)
    return dict(depth=a[:, 0].copy(), descriptor_1=a[:, 1].copy(), descriptor_2=a[:, 2].copy(),
                depth_residuals=a[:, 3].astype(np.uint32), descriptor_pairs=a[:, 4].astype(np.uint32))


def test_the_decide_rule_on_hand_made_rows():
    nan, inf = float("nan"), float("inf")
    #              c0                        c1                         candidate x     guard on: accepted, lost   guard off: accepted
    cases = [
        ((5.0, 1.0, 1.0, 3, 3), (4.0, 1.0, 1.0, 3, 3), 1.0, (True, False), True),        # lower cost, same pairs
        ((5.0, 1.0, 1.0, 3, 3), (5.0, 1.0, 1.0, 3, 3), 1.0, (False, False), False),      # equal cost: not lower
        ((5.0, 1.0, 1.0, 3, 3), (6.0, 1.0, 1.0, 3, 3), 1.0, (False, False), False),      # higher cost
        ((5.0, 1.0, 1.0, 3, 3), (nan, 1.0, 1.0, 3, 3), 1.0, (False, False), False),      # NaN cost after
        ((5.0, 1.0, 1.0, 3, 3), (1.0, 1.0, -inf, 3, 3), 1.0, (False, False), False),     # -inf is lower but not finite
        ((nan, 1.0, 1.0, 3, 3), (1.0, 1.0, 1.0, 3, 3), 1.0, (False, False), False),      # NaN cost before: nothing is lower than it
        ((5.0, 1.0, 1.0, 3, 3), (1.0, 1.0, 1.0, 2, 3), 1.0, (False, True), True),        # lost a depth residual
        ((5.0, 1.0, 1.0, 3, 3), (1.0, 1.0, 1.0, 3, 2), 1.0, (False, True), True),        # lost a descriptor pair
        ((5.0, 1.0, 1.0, 3, 3), (1.0, 1.0, 1.0, 4, 2), 1.0, (False, True), True),        # gained one, lost the other
        ((5.0, 1.0, 1.0, 3, 3), (6.9, 0.0, 0.0, 4, 4), 1.0, (True, False), True),        # gained pairs and still lower
        ((5.0, 1.0, 1.0, 3, 3), (9.0, 1.0, 1.0, 2, 3), 1.0, (False, False), False),      # lost a pair AND higher: the cost test rejects
        ((5.0, 1.0, 1.0, 3, 3), (0.0, 0.0, 0.0, 0, 0), nan, (False, False), False),      # NaN position: reads as deleted, cost 0
        ((5.0, 1.0, 1.0, 3, 3), (1.0, 1.0, 1.0, 3, 3), inf, (False, False), False),      # infinite candidate word
    ]
    c0, c1 = _planes([c[0] for c in cases]), _planes([c[1] for c in cases])
    cand = np.zeros((5, len(cases)), F32)
    cand[0] = [c[2] for c in cases]
    words = cand.view(np.uint32)
    accepted, lost = gsc.decide(words, c0, c1, 1)
    assert [(bool(a), bool(b)) for a, b in zip(accepted, lost)] == [c[3] for c in cases]
    accepted, lost = gsc.decide(words, c0, c1, 0)
    assert [bool(a) for a in accepted] == [c[4] for c in cases] and not lost.any()
    # a non-finite word in any of the five rows rejects
    for row in range(5):
        cand = np.zeros((5, 1), F32)
        cand[row, 0] = nan
        assert not gsc.decide(cand.view(np.uint32), _planes([cases[0][0]]), _planes([cases[0][1]]), 0)[0][0], row


def test_the_objective_is_added_in_the_stated_order():
    # (depth + descriptor_1) + descriptor_2 in binary64: the other order rounds differently on these values
    p = _planes([(1.0, 2.0 ** -53, 2.0 ** -53, 0, 0)])
    assert gsc.objective(p)[0] == 1.0 and 1.0 + (2.0 ** -53 + 2.0 ** -53) != 1.0


# ---- the solve, where no sums are needed ---------------------------------------------------------------------------------------------------
def test_zero_sums_move_nothing_and_the_gate_of_the_depth_only_solve_holds():
    words = np.array([[1.0], [2.0], [3.0], [10.0], [-20.0]], F32).view(np.uint32)
    normal = np.array([[0.0], [0.0], [1.0]], F32)
    for lam in (0.0, 1.0, 16.0):
        assert (gsc.damped_solve(np.zeros((8, 1), F32), words, normal, lam, True) == words).all()
        assert (gsc.damped_solve(np.zeros((2, 1), F32), words, normal, lam, False) == words).all()
        assert (gsc.damped_solve(np.array([[1e-6], [5.0]], F32), words, normal, lam, False) == words).all()      # H > 1e-6f fails
    # depth-only: t = -b / (H + lambda * H) along the normal
    for lam, expected_z in ((0.0, 3.0 - 0.5), (1.0, 3.0 - 0.25), (3.0, 3.0 - 0.125)):
        got = gsc.damped_solve(np.array([[2.0], [1.0]], F32), words, normal, lam, False).view(F32)
        assert got[:, 0].tolist() == [1.0, 2.0, expected_z, 10.0, -20.0], (lam, got)
    # a NaN descriptor: every candidate word the solve writes is non-finite or clamped; the position is NaN
    nan_words = words.copy()
    nan_words[3, 0] = np.array([np.nan], F32).view(np.uint32)[0]
    sums = np.full((8, 1), np.nan, F32)
    got = gsc.damped_solve(sums, nan_words, normal, 0.0, True).view(F32)
    assert np.isnan(got[0:3, 0]).all()


def test_unpack_normal10_gives_unit_vectors_and_its_fma_rounds_once():
    words = np.array([511 | (0 << 10) | (0 << 20), (1024 - 511) | (300 << 10) | ((1024 - 7) << 20), 1 | (1 << 10) | (1 << 20)], np.uint32)
    n = gsc.unpack_normal10(words)
    assert n.dtype == np.float32 and n[:, 0].tolist() == [1.0, 0.0, 0.0]
    assert np.allclose((n.astype(np.float64) ** 2).sum(axis=0), 1.0, atol=3e-7)
    assert n[0, 1] < 0 < n[1, 1] and n[2, 1] < 0
    # the exact rounding helper: a sum that float64 would round twice
    a, c = F32(1 + 2.0 ** -23), F32(2.0 ** -60)
    assert gsc._fma32(a, a, c) == F32(1 + 2.0 ** -22)                                            # 1 + 2^-22 + 2^-46 + 2^-60
    from fractions import Fraction
    assert gsc._round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == F32(1.0)                       # a tie goes to even
    assert gsc._round_f32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80)) == F32(1 + 2.0 ** -23)   # just above the tie: float64 alone would lose it


# ---- the census conditions on the oracle ---------------------------------------------------------------------------------------------------
def test_on_t2_the_plain_step_raises_the_cost_of_many_surfels_and_lowers_many():
    """Measured: 1 079 moved, 961 lowered, 101 raised (the third plain step on tiny)."""
    census = gsc.plain_step_census(gsc.oracle_state("T2"))
    print(census)
    assert census["raised"] >= 50 and census["lowered"] >= 500, census


def test_on_t0_a_surfel_lowers_its_cost_by_losing_a_pair():
    """Measured: 5 of 1 142 (the first plain step on tiny): what the pair guard is for."""
    census = gsc.plain_step_census(gsc.oracle_state("T0"))
    print(census)
    assert census["lowered_losing_a_pair"] >= 1, census
