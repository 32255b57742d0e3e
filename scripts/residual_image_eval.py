#!/usr/bin/env python3
"""Times a residual image (bahip_frame_residual_image: the clear, sweep and resolve kernels of kernels_residual_image.hip) on the bench
scene, built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times on; the frame
is keyframe 0 at its own pose.  Per select (best, worst) and per set of planes (all seven; the depth planes only, which leaves the
descriptors out of the resolve):
  call_ms          the whole call into device planes allocated up front, then a wait for the stream
  clear_ms, sweep_ms, resolve_ms
                   by difference of three timed windows that launch clear / clear + sweep / all three
                   (bahip_debug_set_residual_image_stages); the windows alternate `rounds` times and the medians are taken.  A call is
                   three short launches: at these sizes the differences hold launch gaps as well as kernel time
  pairs, explained, multi
                   the sum of the pairs plane, the pixels with a pair, the pixels with two or more
In the same process, for scale: frame_cost_depth_ms and frame_cost_ms, bahip_evaluate_frame_cost for the same frame with the depth
term alone and with both terms -- the existing call that walks the same pairs; it waits for the stream itself and reads its sums back,
so a call is timed as it is.  Prints one JSON line and writes it to profiles/residual_image_eval.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANE_SETS = {"all_planes": None, "depth_planes": ("key", "pairs", "index", "depth_residual", "inv_stddev")}


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    calls = int(os.environ.get("RESIDUAL_EVALS", "1000"))
    rounds = int(os.environ.get("RESIDUAL_ROUNDS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    first = ba.keyframe_residual_image(0)                       # also leaves the object's intrinsics set in its context
    ctx, s = ba.backend_context(), ba.surfels_struct()
    lib = ctx.lib
    n = int(s.surfels_size)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    W, H = ba.width, ba.height
    F = (C.c_float * 12)(*[float(v) for v in first["frame_T_global"]])
    frame = ba.keyframe_frame(0)
    planes = {name: lowlevel.DeviceBuffer2D(ctx, 1, W * H, dtype, channels) for name, dtype, channels in lowlevel.RESIDUAL_IMAGE_PLANES}

    def window(opt, out):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_frame_residual_image(ctx.handle, C.byref(frame), F, C.byref(s), C.byref(opt), C.byref(out)))
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    results = {}
    try:
        for select_name, select in (("best", capi.RESIDUAL_BEST), ("worst", capi.RESIDUAL_WORST)):
            opt = capi.ResidualImageOptions(select)
            for set_name, wanted in PLANE_SETS.items():
                out = capi.ResidualImageOut(*[planes[name].ptr if wanted is None or name in wanted else None
                                              for name, _, _ in lowlevel.RESIDUAL_IMAGE_PLANES])
                window(opt, out)                                                  # warm-up of this configuration's kernels
                pairs = planes["pairs"].download()[0, :W * H]
                index = planes["index"].download()[0, :W * H]
                assert np.array_equal(index.reshape(H, W), ba.keyframe_residual_image(0, select=select)["index"]), (select_name, set_name)
                timed = {1: [], 3: [], 7: []}
                for _ in range(rounds):
                    for stages in (1, 3, 7):
                        capi.check(lib.bahip_debug_set_residual_image_stages(stages))
                        timed[stages].append(window(opt, out))
                capi.check(lib.bahip_debug_set_residual_image_stages(0))
                clear, clear_sweep, whole = (statistics.median(timed[k]) for k in (1, 3, 7))
                r = dict(call_ms=whole, clear_ms=clear, sweep_ms=clear_sweep - clear, resolve_ms=whole - clear_sweep,
                         call_ms_spread=[min(timed[7]), max(timed[7])], pairs=int(pairs.sum(dtype=np.int64)),
                         explained=int(np.count_nonzero(index != 0xFFFFFFFF)), multi=int(np.count_nonzero(pairs >= 2)))
                results[f"{select_name}_{set_name}"] = r
                log(f"{select_name} {set_name}: {r}")
    finally:
        capi.check(lib.bahip_debug_set_residual_image_stages(0))

    def cost_window(use_desc):
        cost = capi.Cost()
        cost_calls = max(1, calls // 10)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(cost_calls):
            capi.check(lib.bahip_evaluate_frame_cost(ctx.handle, 1, int(use_desc), C.byref(frame), F, C.byref(s), C.byref(cost)))
        ctx.synchronize()
        return (time.perf_counter() - t0) / cost_calls * 1e3, int(cost.depth_residuals)
    cost_window(False)
    depth_only = [cost_window(False) for _ in range(rounds)]
    both = [cost_window(True) for _ in range(rounds)]
    assert depth_only[0][1] == results["best_all_planes"]["pairs"]                # the same pairs
    line = json.dumps(dict(keyframes=args.keyframes, surfels=n, width=W, height=H, calls_per_window=calls, rounds=rounds, compute_units=units,
                           frame_cost_depth_ms=statistics.median(t for t, _ in depth_only), frame_cost_ms=statistics.median(t for t, _ in both),
                           frame_cost_depth_residuals=depth_only[0][1], **results))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "residual_image_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
