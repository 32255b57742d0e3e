"""DirectBA::SetPoseStepControl: with the switch off a BundleAdjustment call is what it was before the switch existed, bit for bit; with
it on no keyframe's cost rises across a pose phase, the statistics add up, the damping factors are carried across calls, and keyframe
sharding refuses it."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f(c):
    return (c["depth"] + c["descriptor_1"]) + c["descriptor_2"]


def _build(scene, start):
    from badslam_amd.directba import DirectBA
    ba = DirectBA(600000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    for k in range(len(start)):
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], start[k])
    return ba


@pytest.fixture(scope="module")
def setup():
    """small_scene(5 keyframes, seed 21), poses perturbed by 2 cm / 8 mrad, surfels created from keyframes 0 and 3 (computed once)."""
    scene = common.small_scene(num_keyframes=5, seed=21)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.02, 0.008) for T in scene.poses_gt]
    ba = _build(scene, start)
    for k in (0, 3):
        ba.CreateSurfelsForKeyframe(k)
    return scene, start, ba.download_surfels()


def _fresh(setup):
    scene, start, data = setup
    ba = _build(scene, start)
    ba.upload_surfels(data)
    return ba


def _alternating(ba, iterations, geometry=True):
    return ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=geometry, min_iterations=iterations,
                               max_iterations=iterations, use_pcg=False, increase_ba_iteration_count=False)


def test_with_the_switch_off_nothing_changes(setup):
    plain, switched = _fresh(setup), _fresh(setup)
    switched.SetPoseStepControl(True)
    switched.SetPoseStepControl(None)
    _alternating(plain, 3)
    _alternating(switched, 3)
    assert plain.last_stats() == switched.last_stats() and switched.pose_step_stats()[:2] == (0, 0)
    assert np.array_equal(_bits(plain.download_surfels()), _bits(switched.download_surfels()))
    for k in range(plain.keyframe_count()):
        assert np.array_equal(_bits(plain.keyframe_pose(k)), _bits(switched.keyframe_pose(k))), k
    # and the switch does take another path
    controlled = _fresh(setup)
    controlled.SetPoseStepControl(True)
    _alternating(controlled, 3)
    assert controlled.pose_step_stats()[0] > 0
    assert any(not np.array_equal(_bits(plain.keyframe_pose(k)), _bits(controlled.keyframe_pose(k))) for k in range(plain.keyframe_count()))


def test_no_keyframes_cost_rises_across_a_pose_phase(setup):
    """Iterations of poses only (the surfels frozen, so that a keyframe's cost changes in its pose phase alone), one per call to see every
    phase -- after a call of no iterations has run the pending end-of-scheme tasks, which do change surfels --, then three in one call
    (whose phases cannot be told apart from outside: its endpoints are compared); the statistics of a call add up."""
    ba = _fresh(setup)
    ba.SetPoseStepControl(True, lambda_initial=0.25)
    K = ba.keyframe_count()
    # the first call with increase_ba_iteration_count = false runs the end-of-scheme tasks (deletion, radius update, compaction) ahead of
    # its iterations: a call of no iterations gets them out of the way, so that the surfels are frozen from here on
    _alternating(ba, 0, geometry=False)
    assert all(ba.pose_step_stats(k)[2] == 0.25 for k in range(K))
    costs = [[_f(c) for c in ba.compute_cost()[1]]]
    for _ in range(3):
        _alternating(ba, 1, geometry=False)
        costs.append([_f(c) for c in ba.compute_cost()[1]])
        trials, rejected, _ = ba.pose_step_stats()
        steps = ba.last_stats()["pose_steps"]
        assert trials == steps + rejected and 0 <= rejected <= trials, (trials, rejected, steps)
    for before, after in zip(costs, costs[1:]):
        assert all(a <= b for a, b in zip(after, before)), (before, after)
    assert any(a < b for a, b in zip(costs[1], costs[0]))
    start = [_f(c) for c in ba.compute_cost()[1]]
    _alternating(ba, 3, geometry=False)
    end = [_f(c) for c in ba.compute_cost()[1]]
    assert all(a <= b for a, b in zip(end, start)), (start, end)
    # with the geometry step in the loop the call still runs through the stage functions and reports its trials
    full = _fresh(setup)
    full.SetPoseStepControl(True)
    _alternating(full, 2)
    trials, rejected, _ = full.pose_step_stats()
    assert trials == full.last_stats()["pose_steps"] + rejected and trials > 0


def test_lambda_persists_across_calls(setup):
    """Every call starts each keyframe from the factor the call before left.  With lambda_initial = 2^-2, lambda_up = 2^2, lambda_down =
    2^-1 and bounds that are never reached (at most 4 rejections in a row, at most BAHIP_MAX_POSE_ITERATIONS accepted steps per phase)
    every factor is a power of two, and over a call  sum_k log2 lambda_k  changes by exactly  2 * rejected - accepted  -- counted from the
    factors stored after the call before, not from lambda_initial.  The two differ as soon as an earlier call has moved a factor."""
    ba = _fresh(setup)
    ba.SetPoseStepControl(True, lambda_initial=0.25, lambda_up=4.0, lambda_down=0.5, lambda_min=0.0, lambda_max=2.0 ** 100, max_trials=4)
    K = ba.keyframe_count()
    _alternating(ba, 0, geometry=False)

    def log2_sum():
        values = [np.float32(ba.pose_step_stats(k)[2]) for k in range(K)]
        exponents = [np.frexp(v)[1] - 1 for v in values]
        assert all(np.ldexp(np.float32(1), e) == v for v, e in zip(values, exponents)), values   # powers of two
        return int(sum(exponents))

    sums, moves = [log2_sum()], []
    assert sums[0] == -2 * K
    for call in range(3):
        _alternating(ba, 1 + call % 2, geometry=False)   # one, two, one iteration(s)
        trials, rejected, _ = ba.pose_step_stats()
        accepted = ba.last_stats()["pose_steps"]
        assert trials == accepted + rejected
        moves.append(2 * rejected - accepted)
        sums.append(log2_sum())
        print("call", call, "trials", trials, "rejected", rejected, "accepted", accepted, "sum log2 lambda", sums[-2], "->", sums[-1])
        assert sums[-1] == sums[-2] + moves[-1], (call, sums, moves)
    # (the factors did move away from lambda_initial, so a call that restarted from it would not have met the sums above)
    assert any(ba.pose_step_stats(k)[2] != 0.25 for k in range(K))


def test_keyframe_sharding_refuses_it(setup):
    ba = _fresh(setup)
    ba.SetKeyframeSharding(0, 2)
    assert ba.L.dba_set_pose_step_control(ba.h, 1, 1e-3, 10.0, 0.33, 0.0, 1e6, 4) == 1
    with pytest.raises(RuntimeError):
        ba.SetPoseStepControl(True)
    ba.SetKeyframeSharding(0, 1)
    ba.SetPoseStepControl(True)
    with pytest.raises(RuntimeError):
        ba.SetPoseStepControl(True, max_trials=0)
