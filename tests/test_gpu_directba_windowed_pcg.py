"""DirectBA::SetWindowedPCG: BundleAdjustment(use_pcg=True) with deleted keyframes and with a fixed active keyframe window
(bahip_pcg_iteration_windowed), and with the switch off (the reference's refusals: window ignored, nothing done while a keyframe is
deleted)."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _build(scene, start, ids):
    from badslam_amd.directba import DirectBA
    ba = DirectBA(600000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    for k in ids:
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], start[k])
    return ba


def _scene(num_keyframes=6, seed=17):
    scene = common.small_scene(num_keyframes=num_keyframes, seed=seed)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    return scene, start


def _surfels(scene, start):
    ba = _build(scene, start, range(len(start)))
    for k in (0, 3):
        ba.CreateSurfelsForKeyframe(k)
    return ba.download_surfels()


def _pcg(ba, window=(-1, -1), gauge=None, **kw):
    if gauge is not None:
        ba.set_pcg_gauge_keyframe(gauge)
    args = dict(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=2, use_pcg=True,
                active_keyframe_window_start=window[0], active_keyframe_window_end=window[1], increase_ba_iteration_count=False)
    args.update(kw)
    return ba.BundleAdjustment(**args)


@pytest.mark.parametrize("window", [None, "window"])
def test_deleted_keyframes_are_skipped(window):
    """Scene A: 6 keyframes, id 2 deleted.  Scene B: the same without that keyframe, the same surfels.  With the switch on both give
    the same poses (by id) and surfels; with it off A does nothing."""
    scene, start = _scene()
    data = _surfels(scene, start)
    a = _build(scene, start, range(6))
    a.upload_surfels(data)
    assert a.L.dba_delete_keyframe(a.h, 2) == 0
    b = _build(scene, start, [0, 1, 3, 4, 5])
    b.upload_surfels(data)
    b_of_a = {0: 0, 1: 1, 3: 2, 4: 3, 5: 4}

    off_before = [a.keyframe_pose(k) for k in b_of_a]
    done, _ = _pcg(a, gauge=3)
    assert done == 0
    assert all(np.array_equal(a.keyframe_pose(k), p) for k, p in zip(b_of_a, off_before))
    assert np.array_equal(_bits(a.download_surfels()), _bits(data))

    a.SetWindowedPCG(True)
    b.SetWindowedPCG(True)
    wa, wb = ((3, 5), (2, 4)) if window else ((-1, -1), (-1, -1))
    da, _ = _pcg(a, wa, gauge=3)
    db, _ = _pcg(b, wb, gauge=2)
    assert da == db > 0
    for ka, kb in b_of_a.items():
        assert np.array_equal(a.keyframe_pose(ka), b.keyframe_pose(kb)), ka
    assert np.array_equal(_bits(a.download_surfels()), _bits(b.download_surfels()))
    if window:
        assert all(np.array_equal(a.keyframe_pose(k), p) for k, p in zip((0, 1), off_before[:2]))


def test_the_window_is_honoured():
    """Perturbed poses of the window's keyframes move towards the ground truth; every pose outside the window keeps its bits.  With the
    switch off the same call is today's whole-map call."""
    scene, _ = _scene()
    rng = np.random.Generator(np.random.PCG64(4))
    start = [np.asarray(T) for T in scene.poses_gt]
    start[3] = common.synthetic.perturb_pose(rng, scene.poses_gt[3], 0.01, 0.002)
    data = _surfels(scene, [np.asarray(T) for T in scene.poses_gt])

    def fresh():
        ba = _build(scene, start, range(6))
        ba.upload_surfels(data)
        return ba

    ba = fresh()
    ba.SetWindowedPCG(True)
    before = [ba.keyframe_pose(k) for k in range(6)]
    _pcg(ba, (2, 3), gauge=2, max_iterations=4)
    for k in (0, 1, 4, 5):
        assert np.array_equal(ba.keyframe_pose(k), before[k]), k
    for k in (3,):   # (2 sits at the ground truth: fixed as the gauge, or an unknown that stays there)
        err_before = np.abs(common.pose_error(before[k], scene.poses_gt[k]))
        err_after = np.abs(common.pose_error(ba.keyframe_pose(k), scene.poses_gt[k]))
        # back to the ground truth: every component of log(T^-1 T_gt) below 1e-3 (the single-plane closed-loop tests reach 1e-6 on
        # dense exact surfels; here the surfels are the sparse cells of two keyframes)
        assert err_before.max() > 2e-3 and err_after.max() < 1e-3, (k, err_before, err_after)

    off, whole = fresh(), fresh()
    _pcg(off, (2, 3), gauge=2)
    _pcg(whole, (-1, -1), gauge=2)
    for k in range(6):
        assert np.array_equal(off.keyframe_pose(k), whole.keyframe_pose(k)), k
    assert np.array_equal(_bits(off.download_surfels()), _bits(whole.download_surfels()))


def test_windowed_surfel_updates_create_for_the_windows_keyframes_only():
    """A windowed BundleAdjustment(use_pcg, do_surfel_updates, increase_ba_iteration_count) runs its creation batch for the window's
    kActive keyframes only: the same keyframes as the alternating scheme's first creation batch for the same window (both mark them with
    last_active_in_ba_iteration, the co-visible ones with last_covis_in_ba_iteration), no others.  Whole-map PCG creates for all.  And the
    windowed call gives the same bits twice."""
    scene, start = _scene()
    window = (1, 2)
    alt = _build(scene, start, range(6))
    alt.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=1,
                         use_pcg=False, active_keyframe_window_start=window[0], active_keyframe_window_end=window[1],
                         increase_ba_iteration_count=True)
    whole = _build(scene, start, range(6))
    whole.SetWindowedPCG(True)
    _pcg(whole, gauge=1, max_iterations=1, do_surfel_updates=True, increase_ba_iteration_count=True)
    runs = []
    for _ in range(2):
        ba = _build(scene, start, range(6))
        ba.SetWindowedPCG(True)
        _pcg(ba, window, gauge=1, max_iterations=1, do_surfel_updates=True, increase_ba_iteration_count=True)
        runs.append(([ba.keyframe_pose(k) for k in range(6)], ba.download_surfels(), ba.surfel_count(),
                     [ba.keyframe_ba_iterations(k) for k in range(6)]))
    marks = runs[0][3]
    assert [a for a, _ in marks] == [0 if window[0] <= k <= window[1] else -1 for k in range(6)], marks
    assert marks == [alt.keyframe_ba_iterations(k) for k in range(6)]
    assert [whole.keyframe_ba_iterations(k)[0] for k in range(6)] == [0] * 6
    assert 0 < runs[0][2] < whole.surfel_count()
    assert runs[0][3] == runs[1][3]
    assert runs[0][2] == runs[1][2] > 0
    for k in range(6):
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
