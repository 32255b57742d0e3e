"""DirectBA::SetPCGStepControl: BundleAdjustment(use_pcg=True) under step control does not raise ComputeCost, reports its trials, carries
the damping factor across calls, and with the control off is the plain PCG host path bit for bit."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scalar(c):
    return (c["depth"] + c["descriptor_1"]) + c["descriptor_2"]


def _build(scene, start):
    from badslam_amd.directba import DirectBA
    ba = DirectBA(600000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    for k in range(len(start)):
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], start[k])
    return ba


def _scene(sigma_t, sigma_r, num_keyframes=5, seed=17):
    scene = common.small_scene(num_keyframes=num_keyframes, seed=seed)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, sigma_t, sigma_r) for T in scene.poses_gt]
    ba = _build(scene, start)
    for k in (0, 3):
        ba.CreateSurfelsForKeyframe(k)
    return scene, start, ba.download_surfels()


def _pcg(ba, iterations):
    ba.set_pcg_gauge_keyframe(1)
    return ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, min_iterations=iterations,
                               max_iterations=iterations, use_pcg=True, increase_ba_iteration_count=False)


@pytest.mark.parametrize("sigmas", [(0.005, 0.002), (0.08, 0.032)])
def test_the_cost_does_not_rise_under_step_control(sigmas):
    scene, start, data = _scene(*sigmas)
    ba = _build(scene, start)
    ba.upload_surfels(data)
    ba.SetPCGStepControl(True)
    assert ba.pcg_step_stats()[0] == np.float32(1e-3)
    before, _ = ba.compute_cost(per_keyframe=False)
    _pcg(ba, 4)
    after, _ = ba.compute_cost(per_keyframe=False)
    lam, trials, rejected = ba.pcg_step_stats()
    print(sigmas, _scalar(before), _scalar(after), lam, trials, rejected)
    assert _scalar(after) <= _scalar(before)
    assert 1 <= trials <= 4 * 6 and 0 <= rejected <= trials
    if rejected < trials:
        assert _scalar(after) < _scalar(before)
    # the factor is carried into the next call
    _pcg(ba, 1)
    again, _ = ba.compute_cost(per_keyframe=False)
    assert _scalar(again) <= _scalar(after)


def test_with_the_control_off_the_call_is_the_plain_pcg_path():
    scene, start, data = _scene(0.005, 0.002)
    plain = _build(scene, start)
    plain.upload_surfels(data)
    switched = _build(scene, start)
    switched.upload_surfels(data)
    switched.SetPCGStepControl(True)
    switched.SetPCGStepControl(None)
    _pcg(plain, 3)
    _pcg(switched, 3)
    assert plain.last_stats() == switched.last_stats() and switched.pcg_step_stats()[1:] == (0, 0)
    assert np.array_equal(_bits(plain.download_surfels()), _bits(switched.download_surfels()))
    for k in range(len(start)):
        assert np.array_equal(_bits(plain.keyframe_pose(k)), _bits(switched.keyframe_pose(k))), k
    # and step control does take another path: its first step is damped
    controlled = _build(scene, start)
    controlled.upload_surfels(data)
    controlled.SetPCGStepControl(True)
    _pcg(controlled, 3)
    assert not np.array_equal(_bits(plain.download_surfels()), _bits(controlled.download_surfels()))


def test_values_out_of_range_are_refused():
    scene, start, _ = _scene(0.005, 0.002)
    ba = _build(scene, start)
    with pytest.raises(RuntimeError):
        ba.SetPCGStepControl(True, max_trials=0)
    with pytest.raises(RuntimeError):
        ba.SetPCGStepControl(True, lambda_up=0.5)
    ba.SetPCGStepControl(True, lambda_initial=0.5)
    assert ba.pcg_step_stats()[0] == 0.5
