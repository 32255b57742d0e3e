#!/usr/bin/env python3
"""Times the observation lists (bahip_surfel_observations: the count and fill sweeps of kernels_observations.hip and the scan between
them) on the bench scene, built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py
times on.  The call waits for the stream itself (it reads P back after the count and waits again at its end), so a call is timed as it
is: the host clock around `calls` calls into device planes allocated up front.
  cases            keyframes only / with depth_raw / with depth_raw and descriptor_raw
  forms            the direct fill and the staged fill with several windows (entries per wavefront x wavefronts per workgroup, then
                   workgroups per compute unit where not 4); a window the 64 KB of LDS cannot hold is made smaller by the launcher
  call_ms, count_ms, scan_ms, fill_ms
                   by difference of three timed windows that launch count / count + scan / all (bahip_debug_set_observations_stages);
                   the windows alternate `rounds` times and the medians are taken
  bytes            what a call writes: surfel_first and the P entries of the planes asked for
  fill_gb_per_s    the planes' bytes / fill_ms: the effective store rate of the fill (it also traverses every pair again)
Every form's planes are compared with the direct form's before they are timed.  In the same process on the same state, the yardsticks:
surfel_costs_depth_ms, bahip_evaluate_surfel_costs(use_depth = 1, use_desc = 0), and covisibility_ms, bahip_observed_covisibility (queued
calls and one wait per window, as scripts/covisibility_eval.py times it).  Prints one JSON line and writes it to
profiles/surfel_observations_eval.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("keyframes", ()), ("depth", ("depth_raw",)), ("depth_descriptor", ("depth_raw", "descriptor_raw")))
# name, stage_entries of the shape hook, wavefronts per workgroup, workgroups per compute unit (0 = default)
FORMS = (("direct", -1, 8, 4), ("direct_4x4", -1, 4, 4), ("staged_256x8", 256, 8, 4), ("staged_512x4", 512, 4, 4), ("staged_768x4", 768, 4, 4),
         ("staged_1024x4", 1024, 4, 4), ("staged_1024x4_2", 1024, 4, 2), ("staged_1024x4_8", 1024, 4, 8), ("staged_1024x8", 1024, 8, 4),
         ("staged_2048x2", 2048, 2, 4))
ENTRY_BYTES = {"keyframes": 2, "depth_raw": 4, "descriptor_raw": 8}


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    calls = int(os.environ.get("OBSERVATIONS_EVALS", "20"))
    rounds = int(os.environ.get("OBSERVATIONS_ROUNDS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    ids, covis = ba.observed_covisibility()                     # also leaves the object's keyframes bound in its context
    ctx, s = ba.backend_context(), ba.surfels_struct()
    lib = ctx.lib
    K, n = len(ids), int(s.surfels_size)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = C.c_uint64(0)
    first = lowlevel.DeviceBuffer2D(ctx, 1, n + 1, np.uint32)
    capi.check(lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(capi.Observations(first.ptr, None, None, None, 0)), C.byref(pairs)))
    P = int(pairs.value)
    assert P == int(np.trace(covis.astype(np.int64)))           # the same pairs
    lengths = np.diff(first.download()[0].astype(np.int64))
    log(f"{K} keyframes, {n} surfels, {P} pairs")
    planes = {"keyframes": lowlevel.DeviceBuffer2D(ctx, 1, P, np.uint16), "depth_raw": lowlevel.DeviceBuffer2D(ctx, 1, P, np.float32),
              "descriptor_raw": lowlevel.DeviceBuffer2D(ctx, 1, 2 * P, np.float32)}

    def out_for(residuals):
        return capi.Observations(first.ptr, planes["keyframes"].ptr, *[planes[name].ptr if name in residuals else None
                                                                     for name in ("depth_raw", "descriptor_raw")], P)

    def window(out):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(out), C.byref(pairs)))
        ctx.synchronize()
        assert pairs.value == P
        return (time.perf_counter() - t0) / calls * 1e3

    def snapshot(residuals):
        return {name: planes[name].download()[0].view(np.uint32 if name != "keyframes" else np.uint16).copy() for name in ("keyframes",) + residuals}

    results = {}
    try:
        for case, residuals in CASES:
            out = out_for(residuals)
            nbytes = P * sum(ENTRY_BYTES[name] for name in ("keyframes",) + residuals)
            reference = None
            results[case] = dict(bytes=4 * (n + 1) + nbytes, forms={})
            for form, stage_entries, waves, per_unit in FORMS:
                capi.check(lib.bahip_debug_set_observations_shape(waves, per_unit * units, stage_entries, -1, 0))
                for b in planes.values():
                    b.clear(0xA5)
                window(out)                                     # warm-up
                got = snapshot(residuals)
                if reference is None:
                    reference = got
                for name in got:
                    assert np.array_equal(got[name], reference[name]), (case, form, name)
                timed = {1: [], 3: [], 7: []}
                for _ in range(rounds):
                    for stages in (1, 3, 7):
                        capi.check(lib.bahip_debug_set_observations_stages(stages))
                        timed[stages].append(window(out))
                capi.check(lib.bahip_debug_set_observations_stages(0))
                count, count_scan, whole = (statistics.median(timed[k]) for k in (1, 3, 7))
                fill = whole - count_scan
                results[case]["forms"][form] = dict(call_ms=whole, call_ms_spread=[min(timed[7]), max(timed[7])], count_ms=count,
                                                    scan_ms=count_scan - count, fill_ms=fill,
                                                    fill_gb_per_s=(nbytes / (fill * 1e6)) if fill > 0 else None)
                log(f"{case} {form}: call {whole:.3f} ms = count {count:.3f} + scan {count_scan - count:.3f} + fill {fill:.3f}")
    finally:
        capi.check(lib.bahip_debug_set_observations_stages(0))
        capi.check(lib.bahip_debug_set_observations_shape(0, 0, 0, -1, 0))

    # the yardsticks, in the same process on the same state
    cost_planes = [lowlevel.DeviceBuffer2D(ctx, 1, max(1, n), dtype) for _, dtype in lowlevel.Scene.SURFEL_COST_PLANES]
    costs = capi.SurfelCosts(*[b.ptr for b in cost_planes])

    def surfel_cost_window():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_evaluate_surfel_costs(ctx.handle, 1, 0, C.byref(s), C.byref(costs)))
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3
    surfel_cost_window()
    surfel_costs_ms = statistics.median(surfel_cost_window() for _ in range(rounds))
    assert np.array_equal(cost_planes[3].download()[0, :n].astype(np.int64), lengths)       # the same pairs per surfel
    counts = lowlevel.DeviceBuffer2D(ctx, 1, K * K, np.uint32)

    def covis_window():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_observed_covisibility(ctx.handle, C.byref(s), counts.ptr, K))
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3
    covis_window()
    covisibility_ms = statistics.median(covis_window() for _ in range(rounds))

    line = json.dumps(dict(keyframes=K, surfels=n, pairs=P, calls_per_window=calls, rounds=rounds, compute_units=units,
                           list_lengths=dict(mean=float(lengths.mean()), max=int(lengths.max()), empty=int((lengths == 0).sum())),
                           cases=results, surfel_costs_depth_ms=surfel_costs_ms, covisibility_ms=covisibility_ms))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "surfel_observations_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
