#!/usr/bin/env python3
"""Times step control of the pose phase (DirectBA.SetPoseStepControl, bahip_estimate_keyframe_poses_controlled) on the bench scene, built
the way bench.py builds it (same arguments: configs[2] by default).

Kernel times come from the backend's stage timers (hipEvent pairs on its stream; stage 2 = the sweep of a pose round, which is the plain
accumulate launch with the control off -- the code of before this feature, compiled to the same gfx950 instructions -- and the fused sweep
with it on), taken over a call of ONE iteration of poses only (surfels frozen).  `ms_per_round`: all sweep launches of the phase over its
rounds (round 0 of the controlled phase included, which takes no step).  `ms_cost_sweep`: one DirectBA.ComputeCost call, host clock
around a call that ends synchronised (one sweep over all keyframes plus its resolution).  The aim: a fused round cheaper than a plain
round plus a cost sweep.
`alternating`: ms per BundleAdjustment iteration (geometry + poses, three per call, host clock) with the control off and on; off takes the
device-driven loop, on the stage functions.  Prints one JSON line and writes it to profiles/pose_step_control_eval.json."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from badslam_amd import capi
    repeats = int(os.environ.get("POSE_STEP_CONTROL_REPEATS", "4"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    K = args.keyframes
    poses = [ba.keyframe_pose(k) for k in range(K)]
    lib = capi.load()
    handle = C.c_void_p(ba.L.dba_backend_context(ba.h))

    def reset():
        ba.upload_surfels(data)
        for k in range(K):
            ba.set_keyframe_pose(k, poses[k])

    def call(iterations, geometry):
        t0 = time.perf_counter()
        ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=geometry, min_iterations=iterations,
                            max_iterations=iterations, use_pcg=False, increase_ba_iteration_count=False)
        return (time.perf_counter() - t0) * 1e3

    def sweep_timer():
        ms, n = C.c_float(), C.c_int()
        capi.check(lib.bahip_last_stage_time_ms(handle, 2, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def pose_phase(control):
        """One iteration of poses only under the stage timers: (ms of all sweeps, launches, rounds, (candidates, rejected))."""
        reset()
        ba.SetPoseStepControl(control)
        capi.check(lib.bahip_set_profiling(handle, 2))
        call(1, False)
        total, launches = sweep_timer()
        rounds = ba.last_stats()["pose_rounds"]
        stats = ba.pose_step_stats()[:2]
        capi.check(lib.bahip_set_profiling(handle, 0))
        return total, launches, rounds, stats

    rows = {"plain": [], "controlled": []}
    cost, alt = [], {"off": [], "on": []}
    for rep in range(repeats + 1):   # the first round warms up
        p = pose_phase(None)
        c = pose_phase(True)
        reset()
        ba.SetPoseStepControl(None)
        t0 = time.perf_counter()
        ba.compute_cost(per_keyframe=True)
        e = (time.perf_counter() - t0) * 1e3
        reset()
        ba.SetPoseStepControl(None)
        off = call(3, True) / 3.0
        reset()
        ba.SetPoseStepControl(True)
        on = call(3, True) / 3.0
        on_stats = ba.pose_step_stats()[:2]
        if rep:
            rows["plain"].append(p)
            rows["controlled"].append(c)
            cost.append(e)
            alt["off"].append(off)
            alt["on"].append((on, on_stats))
    ba.SetPoseStepControl(None)
    mean = lambda v: sum(v) / len(v) if v else None   # noqa: E731

    def summary(which):
        r = rows[which]
        return dict(ms_all_sweeps=mean([x[0] for x in r]), launches=mean([x[1] for x in r]), rounds=mean([x[2] for x in r]),
                    ms_per_round=mean([x[0] / max(1, x[2]) for x in r]), trials_and_rejected=[list(x[3]) for x in r])

    out = dict(keyframes=K, surfels=int(data.shape[1]), repeats=repeats, plain=summary("plain"), controlled=summary("controlled"),
               ms_cost_sweep=mean(cost), spread_cost_sweep=[min(cost), max(cost)],
               alternating=dict(ms_per_iteration_off=mean(alt["off"]), ms_per_iteration_on=mean([m for m, _ in alt["on"]]),
                                spread_off=[min(alt["off"]), max(alt["off"])], spread_on=[min(m for m, _ in alt["on"]), max(m for m, _ in alt["on"])],
                                trials_and_rejected_on=[list(s) for _, s in alt["on"]]))
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_step_control_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
