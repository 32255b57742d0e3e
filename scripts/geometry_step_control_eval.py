#!/usr/bin/env python3
"""Times the geometry phase under step control (bahip_optimize_geometry_iteration_controlled) against the plain geometry step on the
bench scene, built the way bench.py builds it (same arguments: configs[2] by default), from the perturbed surfels bench.py times on --
both from the same state, in the same process.  Per arithmetic flavour:
  plain_ms            bahip_update_activation_and_optimize_geometry, then a wait for the stream
  controlled_ms       the controlled step with the default control (DirectBA::GeometryStepControl), outcome and stats asked for
  split_ms            the same call with a wait after every part (bahip_debug_geometry_trial_timing): phases 1-2, the cost sweeps,
                      snapshot + solve + decide launches, the per-trial read-backs; their sum exceeds controlled_ms by the extra waits
  outcomes            how many surfels ended with outcome 0, 1 .. max_trials, 255
  stats               bahip_geometry_step_stats of the call
  cost_start / cost_plain / cost_controlled   ComputeCost's scalar (depth + descriptor_1 + descriptor_2) of the state, after a plain
                      step and after a controlled step
Prints one JSON line and writes it to profiles/geometry_step_control_eval.json."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from badslam_amd import capi, lowlevel
    evals = int(os.environ.get("GEOMETRY_STEP_EVALS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ctx = ba.backend_context()
    lib = ctx.lib
    control = capi.GeometryStepControl(0.0, 4.0, 1.0, 1e4, 4, 1)

    def reset():
        ba.upload_surfels(data)
        ba.BindScene()
        ctx.synchronize()
        return ba.surfels_struct()

    def scalar():
        total, _ = ba.compute_cost(per_keyframe=False)
        return (total["depth"] + total["descriptor_1"]) + total["descriptor_2"]

    def timed(call):
        ms = []
        for _ in range(evals + 1):
            s = reset()
            t0 = time.perf_counter()
            call(s)
            ctx.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms[1:]))           # (the first one warms up)

    n = int(reset().surfels_size)
    outcome = lowlevel.DeviceBuffer2D(ctx, 1, n, np.uint8)
    stats = capi.GeometryStepStats()
    plain = lambda s: capi.check(lib.bahip_update_activation_and_optimize_geometry(ctx.handle, 1, 1, C.byref(s), n))   # noqa: E731
    controlled = lambda s: capi.check(lib.bahip_optimize_geometry_iteration_controlled(   # noqa: E731
        ctx.handle, 1, 1, C.byref(control), C.byref(s), n, outcome.ptr, C.byref(stats)))

    results = {}
    for arithmetic in ("exact", "fast"):
        ba.SetFastArithmetic(arithmetic == "fast")
        reset()
        row = dict(cost_start=scalar())
        row["plain_ms"] = timed(plain)
        row["cost_plain"] = scalar()
        row["controlled_ms"] = timed(controlled)
        row["cost_controlled"] = scalar()
        hist = np.bincount(outcome.download()[0, :n], minlength=256)
        row["outcomes"] = {str(v): int(hist[v]) for v in (0, 1, 2, 3, 4, 255)}
        row["stats"] = {name: int(getattr(stats, name)) for name, _ in capi.GeometryStepStats._fields_}
        parts = (C.c_double * 4)()
        capi.check(lib.bahip_debug_geometry_trial_timing(ctx.handle, 1, None))
        try:
            split = []
            for _ in range(evals):
                controlled(reset())
                capi.check(lib.bahip_debug_geometry_trial_timing(ctx.handle, 1, parts))
                split.append(list(parts))
        finally:
            capi.check(lib.bahip_debug_geometry_trial_timing(ctx.handle, 0, None))
        med = np.median(np.array(split), axis=0)
        row["split_ms"] = dict(phases_1_2=float(med[0]), cost_sweeps=float(med[1]), solve_and_decide=float(med[2]), host_waits=float(med[3]))
        row["cost_sweeps_per_call"] = 1 + row["stats"]["trials"]
        results[arithmetic] = row
        log(f"{arithmetic}: {row}")
    ba.SetFastArithmetic(False)
    line = json.dumps(dict(keyframes=args.keyframes, surfels=n, evaluations=evals, **results))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "geometry_step_control_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
