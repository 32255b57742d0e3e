"""Step control of the intrinsics step on the CPU (no GPU needed): the binary32 model of tests/intrinsics_step_control.py against the
oracle, the ladder and the argument checks, and the census of states the GPU tests (tests/test_gpu_intrinsics_step_control.py) stand on.

The model is trustworthy because at lambda = 0, fed with the oracle's accumulators rounded to binary32, it gives orc_optimize_intrinsics'
cameras, a and cfactor image bit for bit.  The census is taken with it and the oracle's cost (orc_evaluate_cost):
  state R   crop_small after 4 plain steps: the plain step raises the cost (6.5e-5 relative), the rung lambda = 1 lowers it;
  state H   small21 after 9 plain steps: the plain step raises the cost (7.4e-6 relative) and none of the default ladder's rungs 0, 1, 4,
            16 lowers it.  (small21 after 5 plain steps, where a float64 model holds, is not such a state in binary32: lambda = 4 lowers
            the cost by 1.7e-7 relative there.  profiles/intrinsics_step_control_ladder.json records the search.)
  tiny      the first steps fall at lambda = 0."""
import numpy as np
import pytest

from tests import intrinsics_step_control as isc

STATE_R = ("crop_small", 4)
STATE_H = ("small21", 9)
MIN_RISE = 1e-6          # relative: the GPU total agrees with the oracle's to 1e-9, so the two cannot disagree on the sign
MIN_MARGIN = 1e-8        # relative, for the damped rungs of state H: ten times that agreement


build = isc.build_oracle


def _bits(values):
    return np.ascontiguousarray(np.asarray(values, np.float32)).view(np.uint32)


@pytest.mark.parametrize("optimize_depth,optimize_color", [(True, False), (False, True), (True, True)], ids=["depth", "colour", "both"])
@pytest.mark.parametrize("name", ["small21", "tiny", "crop_small"])
def test_the_model_at_lambda_0_gives_the_oracles_step_bit_for_bit(name, optimize_depth, optimize_color):
    ba = build(name)
    for step in range(2):   # (the second step starts from a != 0 and a cfactor image that is not the scene's)
        saved = isc.oracle_state(ba)
        glob, cells = isc.oracle_sums(ba, optimize_depth, optimize_color)
        assert cells.shape == (ba.cfactor.size, 8)
        got = isc.damped_step(glob, cells, 0.0, saved["depth_cam"], saved["color_cam"], saved["a"], saved["cfactor"], optimize_depth, optimize_color)
        cc, dc, a = ba.optimize_intrinsics(optimize_depth, optimize_color)
        assert np.array_equal(_bits(got["depth_cam"]), _bits(isc.camera_of(dc))), (name, step)
        assert np.array_equal(_bits(got["color_cam"]), _bits(isc.camera_of(cc))), (name, step)
        assert _bits(got["a"]) == _bits(a), (name, step)
        assert np.array_equal(_bits(got["cfactor"]), _bits(ba.cfactor).reshape(-1)), (name, step)
        if optimize_depth:
            assert np.any(got["x1"] != 0) and np.any(got["cfactor"] != saved["cfactor"].reshape(-1))
        if optimize_color:
            assert np.any(got["xc"] != 0)


def test_tiny_has_a_partial_last_wavefront_of_cells():
    ba = build("tiny")
    assert ba.cfactor.size == 805 and 805 % 64 != 0


def test_the_ladder():
    c = isc.control()
    assert [float(v) for v in isc.rungs(c, 0.0)] == [0.0, 1.0, 4.0, 16.0]
    assert float(isc.up(c, 0.0)) == 1.0 and float(isc.up(c, 1.0)) == 4.0 and float(isc.up(c, 4096.0)) == 1e4 and float(isc.up(c, 1e4)) == 1e4
    assert float(isc.down(c, 16.0)) == 4.0 and float(isc.down(c, 4.0)) == 1.0 and float(isc.down(c, 1.0)) == 0.0 and float(isc.down(c, 0.0)) == 0.0
    # a rejection at lambda_max ends the ladder; max_trials cuts it
    assert [float(v) for v in isc.rungs(c, 1e4)] == [1e4]
    assert [float(v) for v in isc.rungs(c, 4096.0)] == [4096.0, 1e4]
    assert [float(v) for v in isc.rungs(isc.control(max_trials=1), 0.0)] == [0.0]
    # binary32: up and down are single roundings of the product / quotient
    odd = isc.control(lambda_first=0.3, lambda_up=3.0)
    assert isc.up(odd, 0.0) == np.float32(0.3) and isc.up(odd, np.float32(0.3)) == np.float32(0.3) * np.float32(3.0)
    assert isc.down(odd, np.float32(0.3)) == 0.0       # 0.1 < lambda_first
    assert isc.down(odd, np.float32(2.7)) == np.float32(2.7) / np.float32(3.0)


def test_the_argument_checks():
    assert isc.control_ok(isc.control())
    for bad in (dict(lambda_first=0.0), dict(lambda_first=-1.0), dict(lambda_up=1.0), dict(lambda_up=0.5), dict(lambda_first=2.0, lambda_max=1.0),
                dict(lambda_first=float("nan")), dict(lambda_up=float("inf")), dict(lambda_max=float("inf")), dict(lambda_max=float("nan")),
                dict(max_trials=0)):
        assert not isc.control_ok(isc.control(**bad)), bad
    assert isc.control_ok(isc.control(lambda_first=5.0, lambda_max=5.0))


def test_the_accept_rule():
    assert isc.accepts(2.0, 1.0) and not isc.accepts(1.0, 1.0) and not isc.accepts(1.0, 2.0)
    assert not isc.accepts(1.0, float("nan")) and not isc.accepts(1.0, float("-inf")) and not isc.accepts(float("nan"), 1.0)
    assert isc.objective(dict(depth=1e16, descriptor_1=1.0, descriptor_2=1.0)) == (1e16 + 1.0) + 1.0


def _rung_costs(ba):
    """(cost before, [cost of the damped step at every default rung]) of the oracle's state, which is left as it was."""
    saved = isc.oracle_state(ba)
    before = ba.evaluate_cost()[0]
    sums = isc.oracle_sums(ba)
    costs = [isc.oracle_trial(ba, sums, saved, lam)[0] for lam in isc.rungs(isc.control(), 0.0)]
    isc.oracle_put(ba, saved)
    return before, costs


def test_census_state_r():
    name, steps = STATE_R
    ba = build(name, steps)
    before, costs = _rung_costs(ba)
    assert (costs[0] - before) / before > MIN_RISE, (before, costs)
    assert min(costs[1:]) < before and (before - min(costs[1:])) / before > MIN_RISE, (before, costs)
    got = isc.oracle_controlled_step(ba, 0.0)
    assert got["accepted"] and got["trials"] == 2 and got["lambda_accepted"] == 1.0 and got["lam"] == 0.0
    # (the oracle's cost is a threaded binary64 sum: two evaluations of one state agree to its last bits, not bit for bit)
    assert got["cost_after"] == pytest.approx(costs[1], rel=1e-12) and ba.evaluate_cost()[0] == pytest.approx(costs[1], rel=1e-12)


def test_census_state_h():
    name, steps = STATE_H
    ba = build(name, steps)
    before, costs = _rung_costs(ba)
    assert (costs[0] - before) / before > MIN_RISE, (before, costs)
    assert all((c - before) / before > MIN_MARGIN for c in costs), (before, costs)
    saved = isc.oracle_state(ba)
    got = isc.oracle_controlled_step(ba, 0.0)
    assert not got["accepted"] and got["trials"] == 4 and got["lam"] == 64.0 and got["cost_after"] == got["cost_before"]
    assert got["cost_before"] == pytest.approx(before, rel=1e-12)
    after = isc.oracle_state(ba)
    for key in saved:
        assert np.array_equal(_bits(saved[key]), _bits(after[key])), key


def test_census_tiny_falls_at_lambda_0():
    ba = build("tiny")
    lam = 0.0
    for step in range(4):
        got = isc.oracle_controlled_step(ba, lam)
        assert got["accepted"] and got["trials"] == 1 and got["lambda_accepted"] == 0.0 and got["lam"] == 0.0, (step, got)
        assert got["cost_after"] < got["cost_before"]
        lam = got["lam"]


def test_no_controlled_step_raises_the_cost_and_crop_small_ends_below_the_plain_sequence():
    plain = build("crop_small", 8).evaluate_cost()[0]
    ba = build("crop_small")
    lam, cost = 0.0, ba.evaluate_cost()[0]
    for _ in range(8):
        got = isc.oracle_controlled_step(ba, lam)
        assert got["cost_before"] == pytest.approx(cost, rel=1e-12) and got["cost_after"] <= got["cost_before"]
        assert ba.evaluate_cost()[0] == pytest.approx(got["cost_after"], rel=1e-12)
        lam, cost = got["lam"], got["cost_after"]
    assert cost <= plain, (cost, plain)
