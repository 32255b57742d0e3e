"""DirectBA::SetIntrinsicsStepControl (dba_set_intrinsics_step_control, DirectBA.SetIntrinsicsStepControl): with the control on, the
intrinsics step of the alternating scheme is bahip_optimize_intrinsics_controlled -- the C-ABI sequence on the same state, bit for bit,
with the damping factor carried from step to step --, the accessors add up, the intrinsics-updated callback fires after accepted steps
only, the default (off) is the plain path, the control runs under surfel sharding, and `ba_tum --intrinsics_step_control` runs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from badslam_amd import capi
from tests import common, tum_writer
from tests import intrinsics_step_control as isc
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "badslam_amd", "lib", "ba_tum")
DEPTH_OFFSET = np.array([0.5, -0.6, 1.23, -2.17])
COLOR_OFFSET = np.array([0.4, -0.3, 0.8, -0.6])
ITERATIONS = 8


def _scene():
    return common.small_scene(num_keyframes=5, seed=21)


def _prepared(scene=None, rows=None):
    """An object with small21's keyframes at ground truth and its surfels [or `rows`], after one BundleAdjustment call that optimises
    nothing (the end tasks have run: later calls start from the buffer as it is), and then both cameras moved off the truth."""
    scene = scene or _scene()
    ba = _build(scene, scene.poses_gt)
    for k in range(len(scene.depth)):
        ba.CreateSurfelsForKeyframe(k)
    _adjust(ba, iterations=1, depth=False, color=False)
    if rows is not None:
        ba.upload_surfels(rows)
    ba.set_cameras(np.asarray(scene.camera, np.float64) + COLOR_OFFSET, np.asarray(scene.camera, np.float64) + DEPTH_OFFSET, 0.0)
    return ba


def _adjust(ba, iterations=ITERATIONS, depth=True, color=True):
    ba.BundleAdjustment(optimize_depth_intrinsics=depth, optimize_color_intrinsics=color, do_surfel_updates=False, optimize_poses=False,
                        optimize_geometry=False, min_iterations=iterations, max_iterations=iterations, use_pcg=False,
                        increase_ba_iteration_count=False)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _state(ba):
    cc, dc, a = ba.cameras()
    return dict(color_cam=cc, depth_cam=dc, a=a, cfactor=ba.cfactor())


def _same(a, b, what=""):
    for key in ("color_cam", "depth_cam", "a", "cfactor"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (what, key)


def _lowlevel_sequence(ba, iterations=ITERATIONS, control=None, lam=0.0):
    """The calls BundleAdjustment(optimize_poses=false, optimize_geometry=false, intrinsics on) makes with the control on, through the
    C ABI: per iteration the activation update, then the controlled step -- the damping factor and, since nothing else touches the
    state, the cost carried from step to step.  Returns the per-step results."""
    ba.BindScene()
    ctx, s = ba.backend_context(), ba.surfels_struct()
    fields = isc.control(**(control or {}))
    ctl = capi.IntrinsicsStepControl(fields["lambda_first"], fields["lambda_up"], fields["lambda_max"], fields["max_trials"])
    lam_io, cost, steps = C.c_float(lam), None, []
    for _ in range(iterations):
        capi.check(ctx.lib.bahip_update_surfel_activation(ctx.handle, C.byref(s), int(s.surfels_size)))
        cc, dc, a = capi.Camera(), capi.Camera(), C.c_float()
        before, after = (capi.Cost() if cost is None else cost), capi.Cost()
        trials, accepted, lam_accepted = C.c_int(), C.c_int(), C.c_float()
        capi.check(ctx.lib.bahip_optimize_intrinsics_controlled(ctx.handle, 1, 1, 1, 1, C.byref(ctl), C.byref(s), C.byref(lam_io), C.byref(cc),
                                                                C.byref(dc), C.byref(a), int(cost is not None), C.byref(before), C.byref(after),
                                                                C.byref(trials), C.byref(accepted), C.byref(lam_accepted)))
        steps.append(dict(trials=trials.value, accepted=accepted.value, lambda_accepted=lam_accepted.value, lam=lam_io.value,
                          before=isc.objective(dict(depth=before.depth, descriptor_1=before.descriptor_1, descriptor_2=before.descriptor_2)),
                          after=isc.objective(dict(depth=after.depth, descriptor_1=after.descriptor_1, descriptor_2=after.descriptor_2)),
                          color_cam=isc.camera_of(cc), depth_cam=isc.camera_of(dc), a=np.float32(a.value)))
        cost = after
        if accepted.value:      # (what BundleAdjustment does with an accepted step: the object follows the context)
            ba.set_cameras(isc.camera_of(cc), isc.camera_of(dc), a.value)
    ctx.synchronize()
    return steps


def test_bundle_adjustment_with_the_control_is_the_c_abi_sequence_and_the_accessors_add_up():
    scene = _scene()
    ba = _prepared(scene)
    calls = []
    ba.SetIntrinsicsUpdatedCallback(lambda: calls.append(ba.cameras()[1].copy()))
    ba.SetIntrinsicsStepControl(True)
    start = _state(ba)
    _adjust(ba)
    got = _state(ba)
    trials, accepted, lam_accepted, lam_next = ba.intrinsics_step_stats()
    total_drop, smallest_drop = ba.intrinsics_step_drops()
    # the same state again, through the C ABI
    hand = _prepared(scene)
    steps = _lowlevel_sequence(hand)
    last = [st for st in steps if st["accepted"]][-1]
    _same(got, dict(color_cam=last["color_cam"], depth_cam=last["depth_cam"], a=last["a"], cfactor=hand.cfactor()), "C ABI")
    assert trials == sum(st["trials"] for st in steps) and accepted == sum(st["accepted"] for st in steps)
    assert lam_accepted == last["lambda_accepted"] and lam_next == steps[-1]["lam"]
    print("steps", [(st["trials"], st["accepted"], st["lambda_accepted"]) for st in steps], "drop", total_drop, smallest_drop)
    assert ITERATIONS <= trials <= 4 * ITERATIONS and 4 <= accepted <= ITERATIONS
    assert all(st["after"] < st["before"] for st in steps if st["accepted"]) and all(st["after"] == st["before"] for st in steps if not st["accepted"])
    assert smallest_drop > 0 and total_drop == pytest.approx(sum(st["before"] - st["after"] for st in steps), rel=1e-12)
    # the callback fired after the accepted steps only, each time with the cameras of that step in the object
    assert len(calls) == accepted
    for seen, st in zip(calls, [st for st in steps if st["accepted"]]):
        assert np.array_equal(_bits(seen), _bits(st["depth_cam"]))
    assert not np.array_equal(_bits(got["depth_cam"]), _bits(start["depth_cam"])) and np.count_nonzero(got["cfactor"]) > 0.5 * got["cfactor"].size
    # the damping factor persists across calls
    _adjust(ba, iterations=1)
    more = _lowlevel_sequence(hand, iterations=1, lam=lam_next)
    assert ba.intrinsics_step_stats()[0] == more[0]["trials"] and ba.intrinsics_step_stats()[3] == more[0]["lam"]
    # the plain path from the same start ends elsewhere: the control is what ran
    plain = _prepared(scene)
    _adjust(plain)
    assert plain.intrinsics_step_stats()[:2] == (0, 0)
    if trials > ITERATIONS:
        assert not np.array_equal(_bits(_state(plain)["cfactor"]), _bits(got["cfactor"]))


def test_a_rejected_ladder_changes_nothing_and_the_callback_stays_silent():
    scene = _scene()
    ba = _prepared(scene)
    rows = ba.download_surfels(17).copy()
    rows[6, rows.shape[1] // 2] = np.nan            # a NaN descriptor: the objective is not finite, every trial is rejected
    ba.upload_surfels(rows)
    calls = []
    ba.SetIntrinsicsUpdatedCallback(lambda: calls.append(1))
    ba.SetIntrinsicsStepControl(True)
    start = _state(ba)
    _adjust(ba, iterations=2)
    _same(_state(ba), start)
    trials, accepted, lam_accepted, lam_next = ba.intrinsics_step_stats()
    # 0, 1, 4, 16 rejected -> 64; 64, 256, 1024, 4096 rejected -> 1e4
    assert (trials, accepted, lam_accepted) == (8, 0, -1.0) and lam_next == 1e4 and calls == []
    assert ba.intrinsics_step_drops() == (0.0, 0.0)


def test_off_is_the_default_and_switching_it_off_again_gives_the_plain_calls_bits():
    scene = _scene()
    never, toggled, hand = _prepared(scene), _prepared(scene), _prepared(scene)
    assert toggled.intrinsics_step_stats() == (0, 0, -1.0, 0.0)
    toggled.SetIntrinsicsStepControl(True)
    toggled.SetIntrinsicsStepControl(False)
    calls = []
    never.SetIntrinsicsUpdatedCallback(lambda: calls.append(1))
    for ba in (never, toggled):
        _adjust(ba, iterations=3)
        assert ba.intrinsics_step_stats() == (0, 0, -1.0, 0.0)
    assert len(calls) == 3      # the plain step applies every update
    _same(_state(never), _state(toggled))
    # ... which are the plain C-ABI calls: activation update, bahip_optimize_intrinsics, bahip_set_intrinsics
    hand.BindScene()
    ctx, s = hand.backend_context(), hand.surfels_struct()
    cc, dc, a = capi.Camera(), capi.Camera(), C.c_float()
    for _ in range(3):
        capi.check(ctx.lib.bahip_update_surfel_activation(ctx.handle, C.byref(s), int(s.surfels_size)))
        capi.check(ctx.lib.bahip_optimize_intrinsics(ctx.handle, 1, 1, C.byref(s), C.byref(cc), C.byref(dc), C.byref(a)))
        hand.set_cameras(isc.camera_of(cc), isc.camera_of(dc), a.value)
        hand.BindScene()
    _same(_state(never), dict(color_cam=isc.camera_of(cc), depth_cam=isc.camera_of(dc), a=a.value, cfactor=hand.cfactor()), "plain C ABI")


def test_values_out_of_range_are_refused_by_the_wrapper_and_the_c_view():
    scene = _scene()
    ba = _build(scene, scene.poses_gt)
    for fields in (dict(lambda_up=1.0), dict(lambda_first=0.0), dict(lambda_first=-1.0), dict(max_trials=0), dict(lambda_first=3.0, lambda_max=2.0),
                   dict(lambda_max=float("inf")), dict(lambda_up=float("nan"))):
        assert not isc.control_ok(isc.control(**fields))
        with pytest.raises(RuntimeError, match="SetIntrinsicsStepControl"):
            ba.SetIntrinsicsStepControl(fields)
    assert ba.L.dba_set_intrinsics_step_control(ba.h, 1, 1.0, 4.0, 1e4, 4) == 0
    assert ba.L.dba_set_intrinsics_step_control(ba.h, 1, 1.0, 0.5, 1e4, 4) == 1
    assert ba.L.dba_set_intrinsics_step_control(ba.h, 0, 0.0, 0.0, 0.0, 0) == 0
    assert ba.intrinsics_step_stats() == (0, 0, -1.0, 0.0)


def test_the_control_runs_under_surfel_sharding_with_one_gpus_decisions_and_bits():
    """Two ranks run the same BundleAdjustment call as the unsharded object -- surfel updates, geometry, poses and the controlled
    intrinsics step -- and end with its cameras, a, cfactor image and accessors."""
    scene = _scene()
    rng = np.random.Generator(np.random.PCG64(9))
    start = [common.synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]

    def run(ba):
        ba.set_cameras(np.asarray(scene.camera, np.float64) + COLOR_OFFSET, np.asarray(scene.camera, np.float64) + DEPTH_OFFSET, 0.0)
        ba.SetIntrinsicsStepControl(True)
        ba.BundleAdjustment(optimize_depth_intrinsics=True, optimize_color_intrinsics=True, do_surfel_updates=True, optimize_poses=True,
                            optimize_geometry=True, min_iterations=4, max_iterations=4, use_pcg=False, increase_ba_iteration_count=True)
        return dict(state=_state(ba), stats=ba.intrinsics_step_stats(), drops=ba.intrinsics_step_drops())

    ref = run(_build(scene, start))

    def rank_main(rank, hook):
        ba = _build(scene, start)
        ctx = ba.backend_context()
        capi.check(ctx.lib.bahip_context_set_allreduce(ctx.handle, hook, None))
        ba.SetSurfelSharding(rank, 2, 1024)
        out = run(ba)
        out["keep"] = (hook, ba)
        return out

    results, loop = _run_ranks(2, rank_main)
    for rank, r in enumerate(results):
        _same(r["state"], ref["state"], rank)
        assert r["stats"] == ref["stats"] and r["drops"] == ref["drops"], (rank, r["stats"], ref["stats"])
    print("stats", ref["stats"], "drops", ref["drops"])
    assert loop.calls > 0 and ref["stats"][1] >= 2 and ref["drops"][1] > 0


def test_ba_tum_with_the_control_runs_and_no_accepted_step_raises_the_objective(tmp_path):
    assert os.path.exists(BIN), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    scene = common.small_scene(num_keyframes=4, width=320, height=240, seed=4)
    rng = np.random.Generator(np.random.PCG64(6))
    initial = [common.synthetic.perturb_pose(rng, T) for T in scene.poses_gt]
    tum_writer.write_dataset(str(tmp_path), scene, {"initial.txt": initial})
    base = [BIN, str(tmp_path), "initial.txt", str(tmp_path / "result"), "--cell", "2", "--iterations", "3", "--max_depth", "8"]
    for refused in (["--intrinsics_step_control"], ["--intrinsics_step_control", "--intrinsics", "--pcg"]):
        proc = subprocess.run(base + refused, capture_output=True, text=True, timeout=120)
        assert proc.returncode == 2 and "--intrinsics_step_control needs --intrinsics" in proc.stderr
    proc = subprocess.run(base + ["--intrinsics", "--intrinsics_step_control"], capture_output=True, text=True, timeout=300)
    print(proc.stdout[-3000:])
    print(proc.stderr[-3000:])
    assert proc.returncode == 0
    lines = re.findall(r"intrinsics step control: (\d+) trial\(s\), (\d+) accepted step\(s\), last accepted lambda (\S+), next lambda (\S+), "
                       r"objective lowered by (\S+) \(smallest drop (\S+)\)", proc.stdout)
    assert len(lines) == 3
    for trials, accepted, _, _, drop, smallest in lines:
        assert int(trials) >= 1 and int(trials) >= int(accepted)
        if int(accepted):
            assert float(smallest) > 0 and float(drop) >= float(smallest)
        else:
            assert float(drop) == 0 and float(smallest) == 0
    assert sum(int(line[1]) for line in lines) >= 1
    assert os.path.exists(str(tmp_path / "result") + ".depth_intrinsics.txt")
