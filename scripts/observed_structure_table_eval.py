#!/usr/bin/env python3
"""Times the three calls of the observed structure -- bahip_observed_covisibility, bahip_keyframe_observer_histogram (16 bins) and
bahip_surfel_observations (keyframes plane alone, and with both payload planes) -- on the tile mask table (route 1 of
bahip_debug_set_observed_structure_route: kernels_tile_masks.hip) against their own kernels (route 0), in one process on the bench scene,
built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times on.
  route0_ms, route1_ms  the median of `rounds` windows of `calls` calls into device memory allocated up front, the host clock around the
                        window, closed by a wait; the windows of the two routes alternate
  count_ms, fill_ms, merge_ms, consumer_ms
                        of route 1, by difference of four timed windows that launch the count sweep (with the scan and the read-back of
                        E) / + the fill sweep / + the merge / all (bahip_debug_set_tile_mask_stages), alternating, medians
  entries, pairs        E of the table and P of the lists
  world8_bytes          what every exchange of a keyframe-sharded call at 8 ranks would move, COMPUTED from E, P, T and K, not measured
Route 1's words are asserted equal to route 0's.  Not measured: the keyframe-sharded path on real links (one process here; the RCCL
path goes through the same reduce_over_ranks), kernel time alone.  Prints one JSON line and writes it to
profiles/observed_structure_table_eval.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = 16
STAGES = (1, 3, 7, 15)
ENTRY_SLICE, PAYLOAD_SLICE = 1600000, 4000000


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    calls = int(os.environ.get("TABLE_EVALS", "50"))
    rounds = int(os.environ.get("TABLE_ROUNDS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    ids, reference_hist = ba.keyframe_redundancy(BINS)          # also leaves the object's keyframes bound in its context
    ctx, s = ba.backend_context(), ba.surfels_struct()
    lib = ctx.lib
    K, n = len(ids), int(s.surfels_size)
    T = (n + 63) // 64
    units = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = int(reference_hist.astype(np.int64).sum())
    matrix = lowlevel.DeviceBuffer2D(ctx, 1, K * K, np.uint32)
    hist = lowlevel.DeviceBuffer2D(ctx, 1, K * BINS, np.uint32)
    first = lowlevel.DeviceBuffer2D(ctx, 1, n + 1, np.uint32)
    ks = lowlevel.DeviceBuffer2D(ctx, 1, max(1, pairs), np.uint16)
    depth = lowlevel.DeviceBuffer2D(ctx, 1, max(1, pairs), np.float32)
    desc = lowlevel.DeviceBuffer2D(ctx, 1, 2 * max(1, pairs), np.float32)
    found = C.c_uint64()
    lists = capi.Observations(first.ptr, ks.ptr, None, None, pairs)
    lists_payload = capi.Observations(first.ptr, ks.ptr, depth.ptr, desc.ptr, pairs)
    what = {
        "covisibility": (lambda: lib.bahip_observed_covisibility(ctx.handle, C.byref(s), matrix.ptr, K), lambda: [matrix.download()[0].copy()]),
        "histogram": (lambda: lib.bahip_keyframe_observer_histogram(ctx.handle, C.byref(s), BINS, hist.ptr, BINS), lambda: [hist.download()[0].copy()]),
        "lists": (lambda: lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(lists), C.byref(found)),
                  lambda: [first.download()[0].copy(), ks.download()[0].copy()]),
        "lists_with_payload": (lambda: lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(lists_payload), C.byref(found)),
                               lambda: [first.download()[0].copy(), ks.download()[0].copy(), depth.download()[0].view(np.uint32).copy(),
                                        desc.download()[0].view(np.uint32).copy()]),
    }

    def window(call, count):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            capi.check(call())
        ctx.synchronize()
        return (time.perf_counter() - t0) / count * 1e3

    out = {}
    entries = None
    try:
        for name, (call, read) in what.items():
            count = calls if name != "lists_with_payload" else max(1, calls // 5)
            results = {}
            for route in (0, 1):
                lowlevel.set_observed_structure_route(route)
                window(call, 2)                                  # warm-up
                ctx.synchronize()
                results[route] = read()
            assert all(np.array_equal(a, b) for a, b in zip(results[0], results[1])), name
            stats = (C.c_uint64 * 6)()
            capi.check(lib.bahip_debug_tile_mask_stats(ctx.handle, stats))
            entries = int(stats[1])
            timed = {0: [], 1: []}
            for _ in range(rounds):
                for route in (0, 1):
                    lowlevel.set_observed_structure_route(route)
                    timed[route].append(window(call, count))
            lowlevel.set_observed_structure_route(1)
            staged = {k: [] for k in STAGES}
            for _ in range(rounds):
                for stages in STAGES:
                    capi.check(lib.bahip_debug_set_tile_mask_stages(stages))
                    staged[stages].append(window(call, count))
            capi.check(lib.bahip_debug_set_tile_mask_stages(0))
            c, cf, cfm, whole = (statistics.median(staged[k]) for k in STAGES)
            out[name] = dict(route0_ms=statistics.median(timed[0]), route1_ms=statistics.median(timed[1]),
                             route0_ms_spread=[min(timed[0]), max(timed[0])], route1_ms_spread=[min(timed[1]), max(timed[1])],
                             count_ms=c, fill_ms=cf - c, merge_ms=cfm - cf, consumer_ms=whole - cfm, atomics=int(stats[4]),
                             payload_words=int(stats[5]))
            out[name]["route1_over_route0"] = out[name]["route1_ms"] / out[name]["route0_ms"]
            log(f"{name}: {out[name]}")
    finally:
        capi.check(lib.bahip_debug_set_tile_mask_stages(0))
        lowlevel.set_observed_structure_route(0)

    world = 8
    slices = lambda words, size: -(-words // size)              # noqa: E731
    world8 = dict(tile_mask_counts=T * ((world + 3) // 4) * 8, tile_mask_entries=(entries + (entries + 3) // 4) * 8,
                  tile_mask_entry_exchanges=slices(entries, ENTRY_SLICE), covisibility_words=K * K * 8, observer_histogram_words=K * BINS * 8,
                  observation_payload_depth=(pairs + 1) // 2 * 8, observation_payload_descriptor=pairs * 8,
                  observation_payload_exchanges=slices(pairs, PAYLOAD_SLICE) + slices(2 * pairs, PAYLOAD_SLICE))
    line = json.dumps(dict(keyframes=K, surfels=n, tiles=T, entries=entries, pairs=pairs, bins=BINS, calls_per_window=calls, rounds=rounds,
                           compute_units=units, calls=out, world8_bytes_computed_not_measured=world8,
                           not_measured=["the keyframe-sharded path on real links (RCCL goes through the same reduce_over_ranks)",
                                         "kernel time alone"]))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "observed_structure_table_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
