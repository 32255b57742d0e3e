#!/usr/bin/env python3
"""Times the reduced camera system (bahip_reduced_camera_system: the pose sweep, the surfel stage of kernels_rcs.hip, the resolve kernel)
on the bench scene, built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times on.
  call_ms          the median of `rounds` windows of `calls` calls into device planes allocated up front; a call allocates and frees its
                   block of sums and waits for the stream itself, so a call is timed as it is
  pose_ms, factor_ms, pair_ms, resolve_ms
                   by difference of four timed windows that launch the pose sums / + the factor traversal / + the pair stage / all
                   (bahip_debug_set_rcs_stages); the windows alternate `rounds` times and the medians are taken
  stats            list entries, pairs of entries visited, 64-bit limb adds due, degenerate surfels, tiles on the overflow path, invalid
  atomics_per_ns   limb adds / pair_ms
  shapes           call_ms for other launch shapes: wavefronts per workgroup x workgroups per compute unit x list capacity
In the same process on the same state: covisibility_ms (bahip_observed_covisibility, queued calls) and, last because it moves the state,
pcg_iteration_ms, one BundleAdjustment(use_pcg=True) call of one outer iteration.  Prints one JSON line and writes it to
profiles/reduced_camera_system_eval.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 8, 8), (1, 4, 8), (1, 4, 16), (1, 2, 16), (1, 1, 32), (2, 4, 8), (2, 2, 16), (4, 2, 8), (1, 8, 4))
STATS = ("list_entries", "pairs_visited", "atomics_issued", "degenerate_surfels", "overflow_tiles", "invalid")


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    calls = int(os.environ.get("RCS_EVALS", "5"))
    rounds = int(os.environ.get("RCS_ROUNDS", "3"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    ids, covisibility = ba.observed_covisibility()              # also leaves the object's keyframes bound in its context
    ctx, s = ba.backend_context(), ba.surfels_struct()
    lib = ctx.lib
    K, n = len(ids), int(s.surfels_size)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    S = lowlevel.DeviceBuffer2D(ctx, 1, 36 * K * K, np.float64)
    g = lowlevel.DeviceBuffer2D(ctx, 1, 6 * K, np.float64)
    stats = (C.c_uint64 * 6)()

    def window(count=calls):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            capi.check(lib.bahip_reduced_camera_system(ctx.handle, 1, 1, 1, C.byref(s), S.ptr, 6 * K, g.ptr, None, None, stats))
        ctx.synchronize()
        return (time.perf_counter() - t0) / count * 1e3

    try:
        first = window(1)                                       # warm-up
        reference = S.download().reshape(6 * K, 6 * K).copy()
        words = dict(zip(STATS, (int(v) for v in stats)))
        log(f"first call {first:.1f} ms, {words}")
        assert np.array_equal(reference, reference.T) and words["invalid"] == 0
        blocks = np.abs(reference).reshape(K, 6, K, 6).max(axis=(1, 3))
        assert np.array_equal(blocks == 0, covisibility == 0)
        timed = {1: [], 3: [], 7: [], 15: []}
        for _ in range(rounds):
            for stages in timed:
                capi.check(lib.bahip_debug_set_rcs_stages(stages))
                timed[stages].append(window())
        capi.check(lib.bahip_debug_set_rcs_stages(0))
        pose, factor, pairs, whole = (statistics.median(timed[k]) for k in (1, 3, 7, 15))
        shapes = {}
        for waves, per_unit, capacity in SHAPES:
            capi.check(lib.bahip_debug_set_rcs_shape(waves, per_unit * units, capacity, -1))
            window(1)
            assert np.array_equal(S.download().reshape(6 * K, 6 * K), reference), (waves, per_unit, capacity)
            name = f"{waves}x{per_unit}x{capacity}"
            shapes[name] = dict(call_ms=statistics.median(window(2) for _ in range(2)), overflow_tiles=int(stats[4]))
            log(f"shape {name}: {shapes[name]}")
    finally:
        capi.check(lib.bahip_debug_set_rcs_stages(0))
        capi.check(lib.bahip_debug_set_rcs_shape(0, 0, 0, -1))

    counts = lowlevel.DeviceBuffer2D(ctx, 1, K * K, np.uint32)

    def covisibility_window():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            capi.check(lib.bahip_observed_covisibility(ctx.handle, C.byref(s), counts.ptr, K))
        ctx.synchronize()
        return (time.perf_counter() - t0) / 50 * 1e3
    covisibility_window()
    covisibility_ms = statistics.median(covisibility_window() for _ in range(rounds))

    ba.set_pcg_gauge_keyframe(0)

    def pcg_iteration():
        ctx.synchronize()
        t0 = time.perf_counter()
        ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=1, use_pcg=True,
                            increase_ba_iteration_count=False)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3
    pcg_iteration()
    pcg_ms = statistics.median(pcg_iteration() for _ in range(3))

    pair_ms = pairs - factor
    tri = blocks[np.triu_indices(K, 1)]
    line = json.dumps(dict(keyframes=K, surfels=n, calls_per_window=calls, rounds=rounds, compute_units=units, call_ms=whole,
                           call_ms_spread=[min(timed[15]), max(timed[15])], pose_ms=pose, factor_ms=factor - pose, pair_ms=pair_ms, resolve_ms=whole - pairs,
                           stats=words, atomics_per_ns=(words["atomics_issued"] / (pair_ms * 1e6)) if pair_ms > 0 else None, shapes=shapes,
                           covisibility_ms=covisibility_ms, pcg_iteration_ms=pcg_ms, keyframe_pairs_coupled=int(np.count_nonzero(tri)), keyframe_pairs=int(tri.size),
                           sums_megabytes=(K * 56 + 6 + K * (K + 1) // 2 * 72 + K * 12) * 8 / 1e6))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "reduced_camera_system_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
