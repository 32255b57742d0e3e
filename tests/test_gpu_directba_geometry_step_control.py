"""DirectBA::SetGeometryStepControl (dba_set_geometry_step_control, DirectBA.SetGeometryStepControl): with the control on, both geometry
calls of the alternating scheme are bahip_optimize_geometry_iteration_controlled -- the C-ABI sequence on the same state, bit for bit --,
the accessors add up, the default (off) leaves the existing path with its device-driven loop, and the control runs under keyframe
sharding."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi
from tests import common
from tests import geometry_step_control as gsc
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

ROWS = 17


def _scene():
    scene = common.small_scene(num_keyframes=4, seed=23)
    rng = np.random.Generator(np.random.PCG64(9))
    return scene, [common.synthetic.perturb_pose(rng, T, 0.004, 0.001) for T in scene.poses_gt]


def _prepared(window, scene=None, start=None):
    """An object whose surfels were created at perturbed poses, after one BundleAdjustment call that optimises nothing: the end tasks
    have run, the window's activations are in the Keyframe objects, and the flags are what the loop leaves for this window."""
    if scene is None:
        scene, start = _scene()
    ba = _build(scene, start)
    for k in range(len(scene.depth)):
        ba.CreateSurfelsForKeyframe(k)
    _adjust(ba, window, geometry=False, iterations=1)
    return ba


def _adjust(ba, window, geometry=True, iterations=3, poses=False):
    ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=poses, optimize_geometry=geometry, min_iterations=iterations,
                        max_iterations=iterations, use_pcg=False, active_keyframe_window_start=window[0],
                        active_keyframe_window_end=window[1], increase_ba_iteration_count=False)


def _flags(ba, upload=None):
    ctx, s = ba.backend_context(), ba.surfels_struct()
    n = int(s.surfels_size)
    if upload is not None:
        a = np.ascontiguousarray(upload, np.uint8)
        capi.check(ctx.lib.bahip_memcpy_2d(ctx.handle, s.active, n, a.ctypes.data, n, n, 1, 1))
        return None
    out = np.empty(n, np.uint8)
    capi.check(ctx.lib.bahip_memcpy_2d(ctx.handle, out.ctypes.data, n, s.active, n, n, 1, 2))
    return out


def _state(ba):
    return ba.download_surfels(ROWS).copy(), _flags(ba)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lowlevel_sequence(ba, full_window, iterations=3, control=None):
    """The calls BundleAdjustment(optimize_poses=false, optimize_geometry=true) makes with the control on, through the C ABI."""
    ba.BindScene()
    ctx, s = ba.backend_context(), ba.surfels_struct()
    n = int(s.surfels_size)
    fields = gsc.control(**(control or {}))
    ctl = capi.GeometryStepControl(fields["lambda_initial"], fields["lambda_up"], fields["lambda_min"], fields["lambda_max"],
                                   fields["max_trials"], fields["guard_pairs"])
    totals = dict.fromkeys(gsc.STATS, 0)
    for _ in range(iterations):
        if not full_window:
            _flags(ba, np.ones(n, np.uint8))
        else:
            _flags(ba, np.zeros(n, np.uint8))        # (the loop clears the flags once; the call decides all of them anyway)
        stats = capi.GeometryStepStats()
        capi.check(ctx.lib.bahip_optimize_geometry_iteration_controlled(ctx.handle, 1, 1, C.byref(ctl), C.byref(s), n if full_window else -1,
                                                                        None, C.byref(stats)))
        for name in gsc.STATS:
            totals[name] += int(getattr(stats, name))
    ctx.synchronize()
    return totals


@pytest.mark.parametrize("window", [(0, 3), (1, 2)])
def test_bundle_adjustment_with_the_control_is_the_c_abi_sequence(window):
    full_window = window == (0, 3)
    ba = _prepared(window)
    rows0, flags0 = _state(ba)
    assert rows0.shape[1] > 10000
    ba.SetGeometryStepControl(True)
    _adjust(ba, window)
    rows_a, flags_a = _state(ba)
    got = ba.geometry_step_stats()
    # the same state again, through the C ABI
    ba.upload_surfels(rows0)
    _flags(ba, flags0)
    totals = _lowlevel_sequence(ba, full_window)
    rows_b, flags_b = _state(ba)
    assert np.array_equal(_bits(rows_a), _bits(rows_b)) and np.array_equal(flags_a, flags_b)
    moved = (_bits(rows_a[list(gsc.ROWS)]) != _bits(rows0[list(gsc.ROWS)])).any(axis=0)
    print(window, "stats", got, "moved", int(moved.sum()), "of", rows0.shape[1])
    assert moved.sum() > 5000
    # the accessors add up, and are the sums of the calls' stats
    candidates, accepted, restored, trials = got
    assert candidates == accepted + restored and accepted > 5000 and restored >= 1
    assert (candidates, accepted, restored, trials) == (totals["candidates"], totals["accepted"], totals["restored"], totals["trials"])
    assert 3 <= trials <= 3 * 4
    # the plain path from the same state moves other bits: the control is what ran
    ba.SetGeometryStepControl(None)
    ba.upload_surfels(rows0)
    _flags(ba, flags0)
    _adjust(ba, window)
    assert ba.geometry_step_stats() == (0, 0, 0, 0)
    assert not np.array_equal(_bits(ba.download_surfels(ROWS)), _bits(rows_a))


def test_no_surfels_cost_rises_over_a_controlled_call():
    ba = _prepared((0, 3))
    rows0, _ = _state(ba)
    before = ba.compute_surfel_costs()
    ba.SetGeometryStepControl(dict(max_trials=3), lambda_min=2.0)
    _adjust(ba, (0, 3), iterations=1)
    after = ba.compute_surfel_costs()
    rows1, _ = _state(ba)
    # (the normals update is not part of the trial: the cost before is taken with the new normal row)
    s1 = rows0.copy()
    s1[3] = rows1[3]
    ba.upload_surfels(s1)
    c0 = ba.compute_surfel_costs()
    f0, f1 = gsc.objective(c0), gsc.objective(after)
    assert (f1 <= f0).all() and (f1 < f0).sum() > 5000
    for name in ("depth_residuals", "descriptor_pairs"):
        assert (after[name] >= c0[name]).all()
    print("total", float(gsc.objective(before).sum()), "->", float(f0.sum()), "(normals) ->", float(f1.sum()))


def test_off_is_the_default_and_takes_the_device_loop_and_on_skips_it():
    lib = capi.load()

    def loop_calls():
        handled, declined = C.c_longlong(), C.c_longlong()
        capi.check(lib.bahip_debug_alternating_loop_calls(C.byref(handled), C.byref(declined)))
        return handled.value, declined.value

    ba = _prepared((0, 3))
    rows0, flags0 = _state(ba)
    before = loop_calls()
    _adjust(ba, (0, 3), poses=True, iterations=2)                     # the default: off
    after_off = loop_calls()
    assert after_off[0] == before[0] + 1 and after_off[1] == before[1], (before, after_off)
    assert ba.geometry_step_stats() == (0, 0, 0, 0)
    rows_off = ba.download_surfels(ROWS)
    ba.SetGeometryStepControl(True)
    ba.upload_surfels(rows0)
    _flags(ba, flags0)
    _adjust(ba, (0, 3), poses=True, iterations=2)
    assert loop_calls() == after_off, "the device-driven loop was asked although the control is on"
    candidates, accepted, restored, trials = ba.geometry_step_stats()
    assert candidates == accepted + restored and accepted > 5000 and 2 <= trials <= 8
    assert not np.array_equal(_bits(ba.download_surfels(ROWS)), _bits(rows_off))
    ba.SetGeometryStepControl(False)
    _adjust(ba, (0, 3), poses=True, iterations=1)
    assert loop_calls()[0] == after_off[0] + 1


def test_values_out_of_range_are_refused_by_the_wrapper_and_the_c_view():
    scene, start = _scene()
    ba = _build(scene, start)
    for fields in (dict(lambda_up=1.0), dict(lambda_min=0.0), dict(lambda_initial=-1.0), dict(max_trials=0), dict(max_trials=255),
                   dict(lambda_min=3.0, lambda_max=2.0), dict(lambda_max=float("inf"))):
        with pytest.raises(RuntimeError, match="SetGeometryStepControl"):
            ba.SetGeometryStepControl(fields)
    assert ba.L.dba_set_geometry_step_control(ba.h, 1, 0.0, 4.0, 1.0, 1e4, 4, 1) == 0
    assert ba.L.dba_set_geometry_step_control(ba.h, 1, 0.0, 0.5, 1.0, 1e4, 4, 1) == 1
    assert ba.L.dba_set_geometry_step_control(ba.h, 0, 0.0, 0.0, 0.0, 0.0, 0, 0) == 0
    assert ba.geometry_step_stats() == (0, 0, 0, 0)


def test_the_control_runs_under_keyframe_sharding_with_the_unsharded_bits():
    scene, start = _scene()
    ref = _prepared((0, 3), scene, start)
    ref.SetGeometryStepControl(True)
    _adjust(ref, (0, 3), iterations=2)
    ref_rows, ref_flags = _state(ref)
    ref_stats = ref.geometry_step_stats()

    def rank_main(rank, hook):
        ba = _prepared((0, 3), scene, start)
        ctx = ba.backend_context()
        capi.check(ctx.lib.bahip_context_set_allreduce(ctx.handle, hook, None))
        ba.SetKeyframeSharding(rank, 2)
        ba.SetGeometryStepControl(True)
        _adjust(ba, (0, 3), iterations=2)
        rows, flags = _state(ba)
        return dict(rows=rows, flags=flags, stats=ba.geometry_step_stats(), keep=(hook, ba))

    results, loop = _run_ranks(2, rank_main)
    for rank, r in enumerate(results):
        assert np.array_equal(_bits(r["rows"]), _bits(ref_rows)) and np.array_equal(r["flags"], ref_flags), rank
        assert r["stats"] == ref_stats, (rank, r["stats"], ref_stats)
    assert loop.calls > 0
