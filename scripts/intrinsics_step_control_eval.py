#!/usr/bin/env python3
"""Times the intrinsics step under step control (bahip_optimize_intrinsics_controlled) against the plain intrinsics step on the bench
scene, built the way bench.py builds it (same arguments: configs[2] by default), from the perturbed surfels bench.py times on, the
cameras as the scene has them, a = 0 and a cleared cfactor image -- both from the same state, in the same process.  Depth and colour
intrinsics, both residual types.  Per arithmetic flavour:
  plain_ms            bahip_optimize_intrinsics, then a wait for the stream (median of the evaluations after one warm-up)
  controlled_ms       the controlled step with the default control (DirectBA::IntrinsicsStepControl) starting at lambda = 0
  split_ms            the same call with a wait after every part (bahip_debug_intrinsics_trial_timing): the sweep, the cost sweeps (the
                      cost before and one per trial), Schur complement + solves + back-substitution (+ restore after a rejection), and
                      the waits for the per-trial read-backs; their sum exceeds controlled_ms by the extra waits
  trials / accepted / lambda_accepted     of that call
  sequence            eight controlled steps in a row, lambda carried over: trials and accepted rung per step (rungs beyond 0 show what
                      a rejection costs on this scene: one more Schur complement, solve, back-substitution, restore and cost sweep)
  cost_start / cost_plain / cost_controlled   the objective (depth + descriptor_1 + descriptor_2) of the state, after the plain step
                      (its cameras put into the context) and after the controlled step
Prints one JSON line and writes it to profiles/intrinsics_step_control_eval.json."""
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
    from badslam_amd import capi
    evals = int(os.environ.get("INTRINSICS_STEP_EVALS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ctx = ba.backend_context()
    lib = ctx.lib
    control = capi.IntrinsicsStepControl(1.0, 4.0, 1e4, 4)
    start_cameras = ba.cameras()

    def reset():
        ba.upload_surfels(data)
        ba.set_cameras(start_cameras[0], start_cameras[1], 0.0)
        ba.L.dba_clear_cfactor(ba.h, ba.stream)
        ba.BindScene()
        ctx.synchronize()
        return ba.surfels_struct()

    def scalar():
        total, _ = ba.compute_cost(per_keyframe=False)
        return (total["depth"] + total["descriptor_1"]) + total["descriptor_2"]

    out = dict(cc=capi.Camera(), dc=capi.Camera(), a=C.c_float(), lam=C.c_float(), before=capi.Cost(), after=capi.Cost(), trials=C.c_int(),
               accepted=C.c_int(), lam_accepted=C.c_float())

    def plain(s):
        capi.check(lib.bahip_optimize_intrinsics(ctx.handle, 1, 1, C.byref(s), C.byref(out["cc"]), C.byref(out["dc"]), C.byref(out["a"])))

    def controlled(s, lam=0.0):
        out["lam"].value = lam
        capi.check(lib.bahip_optimize_intrinsics_controlled(ctx.handle, 1, 1, 1, 1, C.byref(control), C.byref(s), C.byref(out["lam"]),
                                                            C.byref(out["cc"]), C.byref(out["dc"]), C.byref(out["a"]), 0, C.byref(out["before"]),
                                                            C.byref(out["after"]), C.byref(out["trials"]), C.byref(out["accepted"]),
                                                            C.byref(out["lam_accepted"])))

    def timed(call):
        ms = []
        for _ in range(evals + 1):
            s = reset()
            t0 = time.perf_counter()
            call(s)
            ctx.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms[1:]))           # (the first one warms up)

    cam = lambda c: [c.fx, c.fy, c.cx, c.cy]      # noqa: E731
    results = {}
    for arithmetic in ("exact", "fast"):
        ba.SetFastArithmetic(arithmetic == "fast")
        reset()
        row = dict(cost_start=scalar())
        row["plain_ms"] = timed(plain)
        ba.set_cameras(cam(out["cc"]), cam(out["dc"]), out["a"].value)      # (the plain step leaves the new intrinsics to the caller)
        ba.BindScene()
        row["cost_plain"] = scalar()
        row["controlled_ms"] = timed(controlled)
        row.update(trials=out["trials"].value, accepted=out["accepted"].value, lambda_accepted=out["lam_accepted"].value)
        row["cost_controlled"] = (out["after"].depth + out["after"].descriptor_1) + out["after"].descriptor_2
        parts = (C.c_double * 4)()
        capi.check(lib.bahip_debug_intrinsics_trial_timing(ctx.handle, 1, None))
        try:
            split = []
            for _ in range(evals):
                controlled(reset())
                capi.check(lib.bahip_debug_intrinsics_trial_timing(ctx.handle, 1, parts))
                split.append(list(parts))
        finally:
            capi.check(lib.bahip_debug_intrinsics_trial_timing(ctx.handle, 0, None))
        med = np.median(np.array(split), axis=0)
        row["split_ms"] = dict(sweep=float(med[0]), cost_sweeps=float(med[1]), solve_and_back_substitution=float(med[2]), host_waits=float(med[3]))
        row["cost_sweeps_per_call"] = 1 + row["trials"]
        # eight steps in a row (the context keeps what an accepted step leaves; the object's own cameras are not needed for this)
        s, lam, sequence = reset(), 0.0, []
        for _ in range(8):
            t0 = time.perf_counter()
            controlled(s, lam)
            ms = (time.perf_counter() - t0) * 1e3
            lam = out["lam"].value
            sequence.append(dict(trials=out["trials"].value, accepted=out["lam_accepted"].value if out["accepted"].value else None, ms=ms,
                                 cost=(out["after"].depth + out["after"].descriptor_1) + out["after"].descriptor_2))
        row["sequence"] = sequence
        results[arithmetic] = row
        log(f"{arithmetic}: {row}")
    ba.SetFastArithmetic(False)
    line = json.dumps(dict(keyframes=args.keyframes, surfels=int(data.shape[1]), evaluations=evals, **results))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "intrinsics_step_control_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
