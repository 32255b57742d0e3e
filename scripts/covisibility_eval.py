#!/usr/bin/env python3
"""Times the observed co-visibility (bahip_observed_covisibility: the clear and sweep kernels of kernels_covisibility.hip) on the bench
scene, built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times on.
  call_ms          the median of `rounds` windows of `calls` queued calls into a device matrix allocated up front, one wait per window
  clear_ms, traversal_ms, pair_ms
                   by difference of three timed windows that launch clear / clear + traversal (the lists are built, no atomic) / all
                   (bahip_debug_set_covisibility_stages); the windows alternate `rounds` times and the medians are taken
  census           (tile, keyframe) entries with a non-zero mask, atomic adds issued, tiles on the overflow path
  atomics_per_us   atomic adds issued / pair_ms: the effective rate of the 32-bit add onto the K x K words
  shapes           call_ms for other launch shapes (wavefronts per workgroup x workgroups per compute unit), default list capacity
In the same process on the same state, the yardstick: cost_depth_ms, bahip_evaluate_cost(use_depth = 1, use_desc = 0) -- the same
traversal with the cost sweep's sink; it waits for the stream itself and reads its sums back, so a call is timed as it is -- and
cost_both_ms with both terms.  ratio = call_ms / cost_depth_ms.  Prints one JSON line and writes it to profiles/covisibility_eval.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4, 7), (8, 2), (8, 4), (2, 14), (1, 28), (4, 4))


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    calls = int(os.environ.get("COVISIBILITY_EVALS", "200"))
    rounds = int(os.environ.get("COVISIBILITY_ROUNDS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    ids, reference = ba.observed_covisibility()                 # also leaves the object's keyframes bound in its context
    ctx, s = ba.backend_context(), ba.surfels_struct()
    lib = ctx.lib
    K, n = len(ids), int(s.surfels_size)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    counts = lowlevel.DeviceBuffer2D(ctx, 1, K * K, np.uint32)

    def window():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_observed_covisibility(ctx.handle, C.byref(s), counts.ptr, K))
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    def census():
        out = (C.c_uint64 * 3)()
        capi.check(lib.bahip_debug_covisibility_census(ctx.handle, out))
        return [int(v) for v in out]

    try:
        window()                                                # warm-up
        assert np.array_equal(counts.download().reshape(K, K), reference)
        words = census()
        timed = {1: [], 3: [], 7: []}
        for _ in range(rounds):
            for stages in (1, 3, 7):
                capi.check(lib.bahip_debug_set_covisibility_stages(stages))
                timed[stages].append(window())
        capi.check(lib.bahip_debug_set_covisibility_stages(0))
        clear, clear_traversal, whole = (statistics.median(timed[k]) for k in (1, 3, 7))
        shapes = {}
        for waves, per_unit in SHAPES:
            capi.check(lib.bahip_debug_set_covisibility_shape(waves, per_unit * units, 0, -1))
            window()
            assert np.array_equal(counts.download().reshape(K, K), reference), (waves, per_unit)
            shapes[f"{waves}x{per_unit}"] = statistics.median(window() for _ in range(3))
            log(f"shape {waves} x {per_unit} per unit: {shapes[f'{waves}x{per_unit}']:.4f} ms")
    finally:
        capi.check(lib.bahip_debug_set_covisibility_stages(0))
        capi.check(lib.bahip_debug_set_covisibility_shape(0, 0, 0, -1))

    def cost_window(use_desc):
        total = capi.Cost()
        cost_calls = max(1, calls // 4)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(cost_calls):
            capi.check(lib.bahip_evaluate_cost(ctx.handle, 1, int(use_desc), C.byref(s), C.byref(total), None))
        ctx.synchronize()
        return (time.perf_counter() - t0) / cost_calls * 1e3, int(total.depth_residuals)
    cost_window(False)
    depth_only = [cost_window(False) for _ in range(rounds)]
    both = [cost_window(True) for _ in range(rounds)]
    assert depth_only[0][1] == int(np.trace(reference.astype(np.int64)))            # the same pairs
    cost_depth = statistics.median(t for t, _ in depth_only)
    pair_ms = whole - clear_traversal
    tri = reference[np.triu_indices(K, 1)]
    line = json.dumps(dict(keyframes=K, surfels=n, calls_per_window=calls, rounds=rounds, compute_units=units, call_ms=whole,
                           call_ms_spread=[min(timed[7]), max(timed[7])], clear_ms=clear, traversal_ms=clear_traversal - clear, pair_ms=pair_ms,
                           census=dict(entries=words[0], atomics=words[1], overflow_tiles=words[2]),
                           atomics_per_us=(words[1] / (pair_ms * 1e3)) if pair_ms > 0 else None, shapes=shapes,
                           cost_depth_ms=cost_depth, cost_both_ms=statistics.median(t for t, _ in both), ratio=whole / cost_depth,
                           pairs=int(np.trace(reference.astype(np.int64))), keyframe_pairs_sharing=int(np.count_nonzero(tri)),
                           keyframe_pairs=int(tri.size), largest_shared=int(tri.max()) if tri.size else 0))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "covisibility_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
