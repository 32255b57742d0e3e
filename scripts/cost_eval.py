#!/usr/bin/env python3
"""Times the evaluation of the BA objective (DirectBA.compute_cost: the cost sweep of kernels_cost.hip, exact sums, per keyframe) on
the bench scene, built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times
on.  Prints one JSON line: ms per evaluation (the whole call, scene binding and read-back included), associated surfel-keyframe pairs
per second, and the cost itself.  The CPU cost-evaluation path bench.py reports as cpu_baseline is the comparison."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    evals = int(os.environ.get("COST_EVALS", "20"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    results = {}
    for arithmetic in ("exact", "fast"):
        ba.SetFastArithmetic(arithmetic == "fast")
        total, _ = ba.compute_cost()   # warm-up
        t0 = time.perf_counter()
        for _ in range(evals):
            total, _ = ba.compute_cost(per_keyframe=False)
        ms = (time.perf_counter() - t0) / evals * 1e3
        results[arithmetic] = dict(ms_per_evaluation=ms, pairs=total["depth_residuals"],
                                   pairs_per_s=total["depth_residuals"] / (ms * 1e-3), cost=total)
    ba.SetFastArithmetic(False)
    print(json.dumps(dict(keyframes=args.keyframes, surfels=int(data.shape[1]), evaluations=evals, **results)), flush=True)


if __name__ == "__main__":
    main()
