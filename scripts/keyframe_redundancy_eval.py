#!/usr/bin/env python3
"""Times the keyframe redundancy (bahip_keyframe_observer_histogram: the clear and sweep kernels of kernels_redundancy.hip) on the bench
scene, built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times on, for 16
and for 64 bins.
  call_ms          the median of `rounds` windows of `calls` calls into a device table allocated up front; the call waits for the stream
                   itself, so a window is `calls` launches and `calls` waits, closed by one more wait
  clear_ms, traversal_ms, attribution_ms
                   by difference of three timed windows that launch clear / clear + traversal (the counts and the lists are built, no
                   atomic, no second traversal) / all (bahip_debug_set_redundancy_stages); the windows alternate `rounds` times and
                   the medians are taken
  census           (tile, keyframe) entries with a non-zero mask, atomic adds issued, tiles traversed a second time
  shapes           call_ms (16 bins) for other launch shapes (wavefronts per workgroup x workgroups per compute unit)
In the same process on the same state: covisibility_ms, bahip_observed_covisibility (queued calls, one wait per window);
cost_depth_ms, bahip_evaluate_cost(use_depth = 1, use_desc = 0), which waits and reads its sums back; and alternative_ms, what a user
has without this call: bahip_surfel_observations with the keyframes plane alone into planes allocated up front, the read-back of the
offsets and the indices, and a numpy reduction to the same table (split into device_ms, readback_ms and numpy_ms) -- its table is
asserted equal.  Prints one JSON line and writes it to profiles/keyframe_redundancy_eval.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4, 7), (8, 2), (8, 4), (2, 14), (4, 4))
BINS = (16, 64)


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    calls = int(os.environ.get("REDUNDANCY_EVALS", "100"))
    rounds = int(os.environ.get("REDUNDANCY_ROUNDS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    reference = {}
    for bins in BINS:
        ids, reference[bins] = ba.keyframe_redundancy(bins)     # also leaves the object's keyframes bound in its context
    ctx, s = ba.backend_context(), ba.surfels_struct()
    lib = ctx.lib
    K, n = len(ids), int(s.surfels_size)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    hist = lowlevel.DeviceBuffer2D(ctx, 1, K * max(BINS), np.uint32)

    def window(bins):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_keyframe_observer_histogram(ctx.handle, C.byref(s), bins, hist.ptr, bins))
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    def census():
        out = (C.c_uint64 * 3)()
        capi.check(lib.bahip_debug_redundancy_census(ctx.handle, out))
        return [int(v) for v in out]

    per_bins, shapes = {}, {}
    try:
        for bins in BINS:
            window(bins)                                        # warm-up
            assert np.array_equal(hist.download()[0, :K * bins].reshape(K, bins), reference[bins])
            words = census()
            timed = {1: [], 3: [], 7: []}
            for _ in range(rounds):
                for stages in (1, 3, 7):
                    capi.check(lib.bahip_debug_set_redundancy_stages(stages))
                    timed[stages].append(window(bins))
            capi.check(lib.bahip_debug_set_redundancy_stages(0))
            clear, clear_traversal, whole = (statistics.median(timed[k]) for k in (1, 3, 7))
            attribution = whole - clear_traversal
            per_bins[str(bins)] = dict(call_ms=whole, call_ms_spread=[min(timed[7]), max(timed[7])], clear_ms=clear,
                                       traversal_ms=clear_traversal - clear, attribution_ms=attribution,
                                       census=dict(entries=words[0], atomics=words[1], second_traversal_tiles=words[2]),
                                       atomics_per_us=(words[1] / (attribution * 1e3)) if attribution > 0 else None)
            log(f"{bins} bins: {per_bins[str(bins)]}")
        for waves, per_unit in SHAPES:
            capi.check(lib.bahip_debug_set_redundancy_shape(waves, per_unit * units, 0, -1))
            window(16)
            assert np.array_equal(hist.download()[0, :K * 16].reshape(K, 16), reference[16]), (waves, per_unit)
            shapes[f"{waves}x{per_unit}"] = statistics.median(window(16) for _ in range(3))
            log(f"shape {waves} x {per_unit} per unit: {shapes[f'{waves}x{per_unit}']:.4f} ms")
    finally:
        capi.check(lib.bahip_debug_set_redundancy_stages(0))
        capi.check(lib.bahip_debug_set_redundancy_shape(0, 0, 0, -1))

    # the yardsticks, in the same process on the same state
    counts = lowlevel.DeviceBuffer2D(ctx, 1, K * K, np.uint32)

    def covisibility_window():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_observed_covisibility(ctx.handle, C.byref(s), counts.ptr, K))
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    def cost_window():
        total = capi.Cost()
        cost_calls = max(1, calls // 4)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(cost_calls):
            capi.check(lib.bahip_evaluate_cost(ctx.handle, 1, 0, C.byref(s), C.byref(total), None))
        ctx.synchronize()
        return (time.perf_counter() - t0) / cost_calls * 1e3, int(total.depth_residuals)

    covisibility_window()
    cost_window()
    covisibility, cost = [], []
    for _ in range(rounds):
        covisibility.append(covisibility_window())
        cost.append(cost_window())
    pairs = int(reference[16].astype(np.int64).sum())
    assert cost[0][1] == pairs                                  # the same pairs

    # the alternative: the observation lists, read back and reduced on the host
    first = lowlevel.DeviceBuffer2D(ctx, 1, n + 1, np.uint32)
    found = C.c_uint64()
    capi.check(lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(capi.Observations(first.ptr, None, None, None, 0)), C.byref(found)))
    ctx.synchronize()
    assert int(found.value) == pairs
    ks = lowlevel.DeviceBuffer2D(ctx, 1, max(1, pairs), np.uint16)
    planes = capi.Observations(first.ptr, ks.ptr, None, None, pairs)

    def alternative(bins):
        ctx.synchronize()
        t0 = time.perf_counter()
        capi.check(lib.bahip_surfel_observations(ctx.handle, C.byref(s), C.byref(planes), C.byref(found)))
        ctx.synchronize()
        t1 = time.perf_counter()
        offsets = first.download()[0].astype(np.int64)
        indices = ks.download()[0, :pairs]
        t2 = time.perf_counter()
        lengths = np.diff(offsets)
        of_pair = np.repeat(np.minimum(lengths - 1, bins - 1), lengths)
        table = np.bincount(indices.astype(np.int64) * bins + of_pair, minlength=K * bins).reshape(K, bins)
        t3 = time.perf_counter()
        assert np.array_equal(table, reference[bins].astype(np.int64))
        return (t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3

    alternative(16)
    alt = {str(bins): [alternative(bins) for _ in range(3)] for bins in BINS}
    alt = {bins: dict(zip(("alternative_ms", "device_ms", "readback_ms", "numpy_ms"), (statistics.median(v) for v in zip(*runs))))
           for bins, runs in alt.items()}
    for bins in BINS:
        per_bins[str(bins)].update(alt[str(bins)])
        per_bins[str(bins)]["speedup_over_alternative"] = alt[str(bins)]["alternative_ms"] / per_bins[str(bins)]["call_ms"]
    line = json.dumps(dict(keyframes=K, surfels=n, pairs=pairs, calls_per_window=calls, rounds=rounds, compute_units=units, bins=per_bins,
                           shapes_16_bins=shapes, attribution_shape="cells (entry, present bin), bins fastest", lds_private_table="not tried",
                           covisibility_ms=statistics.median(covisibility), cost_depth_ms=statistics.median(t for t, _ in cost),
                           ratio_to_covisibility=per_bins["16"]["call_ms"] / statistics.median(covisibility),
                           ratio_to_cost_depth=per_bins["16"]["call_ms"] / statistics.median(t for t, _ in cost),
                           surfels_only_one_keyframe_sees=int(reference[16][:, 0].sum()),
                           not_measured=["kernel time alone", "the sharded path", "small list capacities on this scene"]))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "keyframe_redundancy_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
