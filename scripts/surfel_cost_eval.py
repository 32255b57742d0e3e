#!/usr/bin/env python3
"""Times the evaluation of the BA objective per surfel (bahip_evaluate_surfel_costs: the sweep of kernels_surfel_cost.hip) on the bench
scene, built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times on, in both
arithmetic flavours -- and, in the same process on the same state, DirectBA.compute_cost (the cost sweep of kernels_cost.hip: the same
traversal with a contended sink).  Per flavour:
  sweep_ms        bahip_evaluate_surfel_costs into device planes allocated up front, then a wait for the stream: the sweep itself
  call_ms         DirectBA.compute_surfel_costs: scene binding, the sweep, 32 bytes per surfel read back into host arrays
  cost_ms         bahip_evaluate_cost (total only) on the same bound scene: the cost sweep, the resolution of its rows, one wait
  cost_call_ms    DirectBA.compute_cost(per_keyframe=False): the same with the scene binding
  sweep_over_cost sweep_ms / cost_ms
and `shapes`: sweep_ms for other launch shapes (wavefronts per workgroup, workgroups per compute unit; the first is the default).
The sums of the planes are checked against the cost's counts before anything is timed.  Prints one JSON line and writes it to
profiles/surfel_cost_eval.json."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 11), (2, 5), (4, 2), (8, 1), (2, 2), (1, 5)]    # (wavefronts per workgroup, workgroups per compute unit)


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    evals = int(os.environ.get("SURFEL_COST_EVALS", "20"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    ba.BindScene()
    ctx, s = ba.backend_context(), ba.surfels_struct()
    n = int(s.surfels_size)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    planes = [lowlevel.DeviceBuffer2D(ctx, 1, n, dtype) for dtype in (np.float64, np.float64, np.float64, np.uint32, np.uint32)]
    out = capi.SurfelCosts(*[p.ptr for p in planes])

    def sweep_ms():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(evals):
            capi.check(ctx.lib.bahip_evaluate_surfel_costs(ctx.handle, 1, 1, C.byref(s), C.byref(out)))
        ctx.synchronize()
        return (time.perf_counter() - t0) / evals * 1e3

    def timed(call):
        t0 = time.perf_counter()
        for _ in range(evals):
            call()
        return (time.perf_counter() - t0) / evals * 1e3

    results = {}
    for arithmetic in ("exact", "fast"):
        ba.SetFastArithmetic(arithmetic == "fast")
        total, _ = ba.compute_cost(per_keyframe=False)   # warm-up, and what the planes must sum to
        got = ba.compute_surfel_costs()
        assert int(got["depth_residuals"].astype(np.uint64).sum()) == total["depth_residuals"], (arithmetic, total)
        assert int(got["descriptor_pairs"].astype(np.uint64).sum()) == total["descriptor_pairs"], (arithmetic, total)
        ba.BindScene()
        sweep_ms()
        cost = capi.Cost()
        evaluate_cost = lambda: capi.check(ctx.lib.bahip_evaluate_cost(ctx.handle, 1, 1, C.byref(s), C.byref(cost), None))   # noqa: E731
        evaluate_cost()
        row = dict(sweep_ms=sweep_ms(), cost_ms=timed(evaluate_cost), call_ms=timed(ba.compute_surfel_costs),
                   cost_call_ms=timed(lambda: ba.compute_cost(per_keyframe=False)), pairs=total["depth_residuals"], descriptor_pairs=total["descriptor_pairs"])
        row["sweep_over_cost"] = row["sweep_ms"] / row["cost_ms"]
        row["pairs_per_s"] = row["pairs"] / (row["sweep_ms"] * 1e-3)
        shapes = {}
        ba.BindScene()
        try:
            for waves, per_unit in SHAPES:
                capi.check(ctx.lib.bahip_debug_set_surfel_cost_shape(waves, per_unit * units, 0, -1))
                sweep_ms()
                shapes[f"{waves}x{per_unit}"] = sweep_ms()
        finally:
            capi.check(ctx.lib.bahip_debug_set_surfel_cost_shape(0, 0, 0, -1))
        row["shapes"] = shapes
        results[arithmetic] = row
        log(f"{arithmetic}: {row}")
    ba.SetFastArithmetic(False)
    line = json.dumps(dict(keyframes=args.keyframes, surfels=n, evaluations=evals, compute_units=units, **results))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "surfel_cost_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
