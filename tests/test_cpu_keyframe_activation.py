"""The keyframe activation state machine on the CPU: the plain model of tests/keyframe_activation.py against the oracle
(oracle/oracle_ba.c: determine_covisible_active, the window handling and the moved rule), rule by rule, and the conditions that make the
scenarios S1-S4 worth comparing the HIP backend with (tests/test_gpu_keyframe_activation.py): conditions, not measurements -- a
scenario that fails one is to be changed, not the condition.  No GPU."""
import numpy as np
import pytest

from tests import keyframe_activation as ka

A, C, I = ka.ACTIVE, ka.COVISIBLE, ka.INACTIVE


def test_the_rules_on_small_lists():
    covis = [[1], [0, 2], [1, 3, 3, 3], [], [4, 0]]
    assert ka.window_rule([0, 1, 1, 0, 0]) == [I, A, A, I, I]
    # sources are the keyframes that are kActive BEFORE the step: 0 wakes 1, and 1 -- now co-visible -- wakes nobody
    assert ka.propagation_rule([A, I, I, I, I], covis) == [A, C, I, I, I]
    # duplicates and self-references change nothing; a co-visible or active target stays what it is; an empty row wakes nobody
    assert ka.propagation_rule([I, C, A, A, A], covis) == [C, C, A, A, A]
    assert ka.propagation_rule([I, I, I, A, I], covis) == [I, I, I, A, I]
    assert ka.pose_phase_rule([A, C, I, A, C], [1, 1, 1, 0, 0]) == ([A, A, I, I, I], 3)


@pytest.fixture(scope="module")
def traces():
    return {name: ka.oracle_trace(ka.scenario(name)) for name in ("S1", "S2")}


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_model_reproduces_the_oracle_iteration_by_iteration(traces, name):
    sc, trace = ka.scenario(name), traces[name]
    state = list(sc.activation)
    for n, it in enumerate(trace):
        assert it["at_pose"] == state, n
        # what the oracle shows of its pose phase: a keyframe it skipped keeps its pose bits; one it estimated moved or did not by
        # is_scale1_pose_converged of log(old^-1 new)
        for k in range(sc.num_keyframes):
            if state[k] == I:
                assert not it["changed"][k] and it["steps"][k] == 0, (n, k)
            else:
                assert it["steps"][k] >= 1, (n, k)
            if it["moved"][k]:
                assert it["changed"][k], (n, k)
        after_pose, num_converged = ka.pose_phase_rule(state, it["moved"])
        assert it["converged"] == int(num_converged == sc.num_keyframes), n
        state = after_pose if it["converged"] else ka.propagation_rule(after_pose, sc.covis)
        assert it["after"] == state, (n, it["after"], state)


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_one_call_is_the_iterations_one_by_one(traces, name):
    sc, trace = ka.scenario(name), traces[name]
    orc = ka.build_oracle(sc)
    stats = orc.bundle_adjustment(min_iterations=1, max_iterations=sc.max_iterations, window_start=-1, window_end=-1,
                                  increase_ba_iteration_count=False)
    assert (stats.iterations_done, stats.converged) == (len(trace), trace[-1]["converged"])
    assert stats.pose_gn_steps_total == sum(it["gn_steps"] for it in trace)
    assert ka.oracle_state(orc) == trace[-1]["after"]
    assert np.array_equal(ka.bits(ka.oracle_poses(orc)), ka.bits(trace[-1]["poses"]))
    assert np.array_equal(ka.bits(orc.surfel_data[:8, :orc.surfels_size]), ka.bits(trace[-1]["surfels"]))


def _assert_deactivation_is_not_vacuous(sc, trace):
    # ends by convergence, after at least two iterations and before the limit
    assert trace[-1]["converged"] == 1 and 2 <= len(trace) < sc.max_iterations, len(trace)
    # an iteration after which all three states are present at once
    assert any(set(it["after"]) == {A, C, I} for it in trace), [it["after"] for it in trace]
    # a keyframe that is kInactive at the pose phase, stays kInactive and keeps its pose bits
    assert any(it["at_pose"][k] == I and it["after"][k] == I and not it["changed"][k] for it in trace for k in range(sc.num_keyframes))
    # a propagation with a kInactive keyframe it does not wake and one it does
    woken = left = False
    for it in trace:
        if it["converged"]:
            continue
        after_pose, _ = ka.pose_phase_rule(it["at_pose"], it["moved"])
        woken_here = [k for k in range(sc.num_keyframes) if after_pose[k] == I and it["after"][k] == C]
        left_here = [k for k in range(sc.num_keyframes) if after_pose[k] == I and it["after"][k] == I]
        woken, left = woken or bool(woken_here), left or bool(left_here)
    assert woken and left


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_deactivation_scenarios_are_not_vacuous(traces, name):
    _assert_deactivation_is_not_vacuous(ka.scenario(name), traces[name])


def _s3():
    sc = ka.scenario("S3")
    orc = ka.build_oracle(sc)
    before = ka.oracle_poses(orc)
    stats = orc.bundle_adjustment(min_iterations=1, max_iterations=sc.max_iterations, window_start=sc.window[0], window_end=sc.window[1],
                                  increase_ba_iteration_count=False)
    return sc, orc, before, stats


def test_partial_fixed_window_model_and_conditions():
    sc, orc, before, stats = _s3()
    K = sc.num_keyframes
    after = ka.oracle_poses(orc)
    assert (stats.iterations_done, stats.converged) == (3, 0)
    # the top of every iteration: window rule + propagation, whatever the pose phase left -- so every iteration's pose phase meets
    at_pose = ka.propagation_rule(ka.window_rule(ka.window_flags(sc.window, K)), sc.covis)
    assert at_pose == [I, C, A, A, C, I, I, I]
    changed = [int(not np.array_equal(ka.bits(before[k]), ka.bits(after[k]))) for k in range(K)]
    # the co-visible keyframes 1 and 4 are solved too; everything outside keeps every bit
    assert changed == [0, 1, 1, 1, 1, 0, 0, 0]
    # the last iteration's pose phase and the propagation behind it (the loop did not converge): from the moved flags of that phase
    orc2 = ka.build_oracle(sc)
    orc2.bundle_adjustment(min_iterations=1, max_iterations=2, window_start=sc.window[0], window_end=sc.window[1], increase_ba_iteration_count=False)
    mid = ka.oracle_poses(orc2)
    moved = [ka.oracle_moved(mid[k], after[k]) if at_pose[k] != I else 0 for k in range(K)]
    after_pose, num_converged = ka.pose_phase_rule(at_pose, moved)
    assert num_converged < K
    assert ka.oracle_state(orc) == ka.propagation_rule(after_pose, sc.covis)
    # conditions: 6 and 7 end kInactive (nothing wakes them), the loop did not end by convergence, all three states at the end
    final = ka.oracle_state(orc)
    assert final[6] == I and final[7] == I and set(final) == {A, C, I}, final


def _s4(orc=None, sc=None):
    sc = sc or ka.scenario("S4")
    orc = orc or ka.build_oracle(sc)
    orc.spatial_sort_cell = 0.02
    out = []
    for _ in range(2):
        stats = orc.bundle_adjustment(do_surfel_updates=True, min_iterations=1, max_iterations=sc.max_iterations, window_start=-1, window_end=-1,
                                      increase_ba_iteration_count=True)
        out.append((stats.iterations_done, stats.converged, orc.surfels_size,
                    [(kf.last_active_in_ba_iteration, kf.last_covis_in_ba_iteration) for kf in orc.keyframes]))
    return out


def test_surfel_updates_under_deactivation_conditions():
    first, second = _s4()
    assert first[1] == 1 and 2 <= first[0] < 10, first
    assert first[2] > 5000
    # a created-for mark differs between keyframes: some were met co-visible by a creation loop, some never
    assert len(set(first[3])) > 1, first[3]
    assert second[0] == 1 and second[1] == 1 and second[2] == first[2], second


# ---- the scenes of the DirectBA-level comparison (co-visibility lists from the host's frustum test) -----------------------------------
@pytest.mark.parametrize("name", ["S1", "S3"])
def test_host_frustum_lists_are_incomplete(tmp_path, name):
    sc = ka.host_scenario(name)
    lists = ka.frustum_lists(sc.scene, ka.build_oracle(sc), tmp_path)
    assert lists == ka.HOST_COVIS[ka.HOST_TRANSLATION_RANGE[name]]
    K = sc.num_keyframes
    missing = [(j, k) for j in range(K) for k in range(j + 1, K) if k not in lists[j]]
    assert len(missing) >= 1 and all(j in lists[k] for j in range(K) for k in lists[j]), missing       # incomplete, symmetric
    # the scenarios' own scene has complete lists: that is why these are wider
    narrow = ka.scenario(name)
    assert ka.frustum_lists(narrow.scene, ka.build_oracle(narrow), tmp_path) == [[j for j in range(K) if j != k] for k in range(K)]


def test_deactivation_under_the_host_lists_is_not_vacuous():
    sc = ka.host_scenario("S1")
    _assert_deactivation_is_not_vacuous(sc, ka.oracle_trace(sc))


def test_partial_fixed_window_under_the_host_lists_conditions():
    """The window (2, 3) under the host's lists: keyframes stay kInactive through every pose phase and keep their pose bits, some of them
    to the end (one that the window's keyframes never list, but a keyframe that moved does, is woken by the last propagation only);
    converged == 0; all three states at the end."""
    sc = ka.host_scenario("S3")
    K = sc.num_keyframes
    orc = ka.build_oracle(sc)
    before = ka.oracle_poses(orc)
    stats = orc.bundle_adjustment(min_iterations=1, max_iterations=sc.max_iterations, window_start=sc.window[0], window_end=sc.window[1],
                                  increase_ba_iteration_count=False)
    after, final = ka.oracle_poses(orc), ka.oracle_state(orc)
    assert (stats.iterations_done, stats.converged) == (3, 0)
    at_pose = ka.propagation_rule(ka.window_rule(ka.window_flags(sc.window, K)), sc.covis)
    assert set(at_pose) == {A, C, I}, at_pose
    changed = [int(not np.array_equal(ka.bits(before[k]), ka.bits(after[k]))) for k in range(K)]
    assert changed == [int(s != I) for s in at_pose], (changed, at_pose)      # solved: the window and what it wakes; the rest keeps every bit
    assert set(final) == {A, C, I}, final
    ends_inactive = [k for k in range(K) if final[k] == I]
    assert ends_inactive and all(at_pose[k] == I and not changed[k] for k in ends_inactive), (final, at_pose, changed)
    # ... and one that was kInactive at the pose phases is woken by the propagation that follows the last one
    assert any(at_pose[k] == I and final[k] == C for k in range(K)), (at_pose, final)


def test_surfel_updates_under_the_host_lists_conditions():
    sc = ka.host_scenario("S4")
    first, second = _s4(ka.build_oracle(sc), sc)
    assert first[1] == 1 and 2 <= first[0] < 10 and first[2] > 5000 and len(set(first[3])) > 1, first
    assert second[0] == 1 and second[1] == 1 and second[2] == first[2], second
