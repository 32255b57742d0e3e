#!/usr/bin/env python3
"""Times step control of the PCG scheme (DirectBA.SetPCGStepControl, bahip_pcg_iteration_controlled) on the bench scene, built the way
bench.py builds it (same arguments: configs[2] by default), against the plain PCG outer iteration.  Each figure is ms per
BundleAdjustment(use_pcg=True) call of one outer iteration (binding, normals, the solve, the write-back), host clock around a call that
ends synchronised, alternating plain and controlled calls from the same surfels and poses.  The split of a controlled iteration:
`cost` is one DirectBA.ComputeCost call timed alone (a controlled iteration makes two), `iteration` the plain call, and `snapshot_by_subtraction`
what is left of an accepted controlled call (controlled - plain - 2 x cost: the snapshot kernel, the host copy of the keyframe table
and the buffer bookkeeping; a difference of host-clock means, so it can come out below zero when it is smaller than their noise).  `restore` is the extra time of a call whose single trial (max_trials = 1) was rejected over an accepted one -- reported only when
such a call occurred on this scene, else null: not measured.  `three_iterations`: the same comparison for calls of three outer iterations, where the
second and third controlled iterations take their cost_before from the one before.  Prints one JSON line and writes it to profiles/pcg_step_control_eval.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    repeats = int(os.environ.get("PCG_STEP_CONTROL_REPEATS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    K = args.keyframes
    poses = [ba.keyframe_pose(k) for k in range(K)]
    ba.set_pcg_gauge_keyframe(0)

    def reset():
        ba.upload_surfels(data)
        for k in range(K):
            ba.set_keyframe_pose(k, poses[k])

    def call(iterations=1):
        t0 = time.perf_counter()
        ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, min_iterations=iterations,
                            max_iterations=iterations, use_pcg=True, increase_ba_iteration_count=False)
        return (time.perf_counter() - t0) * 1e3

    plain, controlled, rejected, cost, steps = [], [], [], [], {"plain": [], "controlled": []}
    plain3, controlled3 = [], []   # calls of three outer iterations: the second and third take their cost_before from the one before
    for rep in range(repeats + 1):   # the first round warms up
        reset()
        ba.SetPCGStepControl(None)
        ms = call()
        if rep:
            plain.append(ms)
            steps["plain"].append(ba.last_stats()["pcg_inner_steps"])
        reset()
        ba.SetPCGStepControl(True, max_trials=1)
        ms = call()
        _, trials, undone = ba.pcg_step_stats()
        if rep:
            (rejected if undone else controlled).append(ms)
            steps["controlled"].append(ba.last_stats()["pcg_inner_steps"])
        reset()
        ba.SetPCGStepControl(None)
        ms = call(3)
        if rep:
            plain3.append(ms)
        reset()
        ba.SetPCGStepControl(True)
        ms = call(3)
        if rep:
            controlled3.append((ms, ba.pcg_step_stats()[1:]))
        t0 = time.perf_counter()
        ba.compute_cost(per_keyframe=False)
        if rep:
            cost.append((time.perf_counter() - t0) * 1e3)
    ba.SetPCGStepControl(None)
    mean = lambda v: sum(v) / len(v) if v else None   # noqa: E731
    p, c, r, e = mean(plain), mean(controlled), mean(rejected), mean(cost)
    out = dict(keyframes=K, surfels=int(data.shape[1]), repeats=repeats, inner_steps=steps,
               ms_plain_outer_iteration=p, ms_controlled_outer_iteration_accepted=c, ms_controlled_outer_iteration_rejected=r,
               accepted_calls=len(controlled), rejected_calls=len(rejected), spread_plain=[min(plain), max(plain)],
               spread_controlled=[min(controlled), max(controlled)] if controlled else None,
               split=dict(iteration=p, cost=e, snapshot_by_subtraction=(c - p - 2 * e) if c is not None else None,
                          restore=(r - c) if (r is not None and c is not None) else None),
               overhead_of_an_accepted_step_ms=(c - p) if c is not None else None,
               overhead_of_an_accepted_step_percent=(100.0 * (c - p) / p) if c is not None else None,
               ms_per_inner_step_plain=p / max(1.0, mean(steps["plain"])),
               three_iterations=dict(ms_plain=mean(plain3), ms_controlled=mean([m for m, _ in controlled3]),
                                     trials_and_undone=[list(t) for _, t in controlled3],
                                     overhead_per_outer_iteration_ms=(mean([m for m, _ in controlled3]) - mean(plain3)) / 3.0))
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pcg_step_control_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
