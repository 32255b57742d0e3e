#!/usr/bin/env python3
"""Times the windowed PCG scheme (DirectBA.SetWindowedPCG, bahip_pcg_iteration_windowed) on the bench scene, built the way bench.py
builds it (same arguments: configs[2] by default), against the whole-map PCG iteration.  For the whole map and for windows of 16 and
50 keyframes at the start and in the middle of the sequence it reports ms per outer iteration (one BundleAdjustment(use_pcg=True)
call of one iteration: binding, window and surfel activation, normals, the solve and the write-back) and per inner step (that time
over the inner steps taken), with the swept keyframes and the 64-surfel tiles the window's sweeps ran over.  Prints one JSON line and
writes it to profiles/pcg_window_eval.json."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from badslam_amd import capi
    repeats = int(os.environ.get("PCG_WINDOW_REPEATS", "3"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    K = args.keyframes
    mid = K // 2
    cases = [("whole_map", -1, -1, False)]
    for size in (16, 50):
        cases.append((f"window{size}_start", 0, size - 1, True))
        cases.append((f"window{size}_middle", mid - size // 2, mid - size // 2 + size - 1, True))
    ctx = ba.backend_context()
    ba.set_pcg_gauge_keyframe(0)
    results = {}
    for name, start, end, windowed in cases:
        ba.SetWindowedPCG(windowed)
        times, steps = [], []
        for rep in range(repeats + 1):   # the first call warms up
            ba.upload_surfels(data)
            t0 = time.perf_counter()
            ba.BundleAdjustment(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=1,
                                use_pcg=True, active_keyframe_window_start=start, active_keyframe_window_end=end,
                                increase_ba_iteration_count=False)
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                times.append(ms)
                steps.append(ba.last_stats()["pcg_inner_steps"])   # (reset by every BundleAdjustment call)
        row = dict(window=[start, end], ms_per_outer_iteration=sum(times) / len(times), inner_steps=steps,
                   ms_per_inner_step=sum(times) / max(1, sum(steps)))
        if windowed:
            sk, tiles = C.c_int(), C.c_uint32()
            capi.check(ctx.lib.bahip_pcg_window_size(ctx.handle, C.byref(sk), C.byref(tiles)))
            row.update(swept_keyframes=sk.value, tiles=tiles.value)
        else:
            row.update(swept_keyframes=K, tiles=-(-int(data.shape[1]) // 64))
        results[name] = row
        log(f"{name}: {row}")
    out = dict(keyframes=K, surfels=int(data.shape[1]), repeats=repeats, **results)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pcg_window_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
