#!/usr/bin/env python3
"""Times a rendered view of the map (bahip_render_surfels: the clear, splat and resolve kernels of kernels_render.hip) on the bench scene,
built the way bench.py builds it (same arguments: configs[2] by default), with the perturbed surfels bench.py times on; the view is
keyframe 0 through the depth camera.  Per configuration -- point mode, disc mode at max_radius_px 2, 4 and 8, and discs of four times
the radius in a box of 16 px (many atomics per surfel: the configuration that says most about the atomic itself):
  call_ms          the whole call into device planes allocated up front, then a wait for the stream
  clear_ms, splat_ms, resolve_ms
                   by difference of three timed windows that launch clear / clear + splat / all three (bahip_debug_set_render_stages);
                   the windows alternate `rounds` times and the medians are taken.  A call is three short launches: at these sizes
                   the differences hold launch gaps as well as kernel time
  tests, atomics, covered
                   the counting splat of bahip_debug_render_census: candidate tests, candidates that contributed a key (one atomic
                   each), covered pixels
  tests_per_surfel, umin_bytes_per_s
                   tests / surfels; 8 bytes per atomic over splat_ms (a lower bound of the rate: splat_ms also reads every surfel) --
                   beside the 1.3e12 bytes/s of added bytes the microarchitecture notes give for 32-bit float adds that arrive as
                   whole 256-byte wave-instructions.  A lane per surfel scatters its atomics over rows of the plane: the shape those
                   notes measured 17 times slower than the contiguous one.
For scale: sweep_ms of profiles/surfel_cost_eval.json, the per-surfel cost sweep over the same buffer.  Prints one JSON line and writes
it to profiles/render_eval.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("point", 0, 0, 1.0), ("disc_r2", 1, 2, 1.0), ("disc_r4", 1, 4, 1.0), ("disc_r8", 1, 8, 1.0), ("disc_r16_factor4", 1, 16, 4.0)]
FLOAT_ADD_BYTES_PER_S = 1.3e12


def main():
    import bench
    import torch
    from badslam_amd import capi, lowlevel
    calls = int(os.environ.get("RENDER_EVALS", "1000"))
    rounds = int(os.environ.get("RENDER_ROUNDS", "5"))
    args = bench.parse_args()
    log = lambda msg: print(msg, file=sys.stderr, flush=True)   # noqa: E731
    ba, data, _ = bench.build_scene(args, log)
    ba.upload_surfels(data)
    ctx, s = ba.backend_context(), ba.surfels_struct()
    lib = ctx.lib
    n = int(s.surfels_size)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    _, depth_camera, _ = ba.cameras()
    W, H = ba.width, ba.height
    view = lowlevel.make_camera(depth_camera, W, H)
    frame = ba.render_surfels(keyframe=0, options=capi.RenderOptions(mode=capi.RENDER_POINT))["frame_T_global"]
    F = (C.c_float * 12)(*[float(v) for v in frame])
    shapes = (("key", np.uint64, 1), ("depth", np.float32, 1), ("index", np.uint32, 1), ("normal", np.float32, 3), ("color", np.uint8, 4))
    planes = {name: lowlevel.DeviceBuffer2D(ctx, 1, W * H, dtype, channels) for name, dtype, channels in shapes}
    out = capi.RenderOut(*[planes[name].ptr for name, _, _ in shapes])

    def window(opt):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(lib.bahip_render_surfels(ctx.handle, C.byref(s), C.byref(view), F, C.byref(opt), C.byref(out)))
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    results = {}
    try:
        for name, mode, radius, factor in CONFIGS:
            opt = capi.RenderOptions(mode=mode, max_radius_px=radius, radius_factor=factor)
            window(opt)                                                      # warm-up of this configuration's kernels
            counts = (C.c_ulonglong * 3)()
            capi.check(lib.bahip_debug_render_census(ctx.handle, C.byref(s), C.byref(view), F, C.byref(opt), counts))
            index = planes["index"].download()
            assert int(np.count_nonzero(index != 0xFFFFFFFF)) == int(counts[2]), name       # the planes and the census agree
            timed = {1: [], 3: [], 7: []}
            for _ in range(rounds):
                for stages in (1, 3, 7):
                    capi.check(lib.bahip_debug_set_render_stages(stages))
                    timed[stages].append(window(opt))
            capi.check(lib.bahip_debug_set_render_stages(0))
            clear, clear_splat, whole = (statistics.median(timed[k]) for k in (1, 3, 7))
            r = dict(call_ms=whole, clear_ms=clear, splat_ms=clear_splat - clear, resolve_ms=whole - clear_splat,
                     call_ms_spread=[min(timed[7]), max(timed[7])], tests=int(counts[0]), atomics=int(counts[1]), covered=int(counts[2]))
            r["tests_per_surfel"] = r["tests"] / n
            r["umin_bytes_per_s"] = 8.0 * r["atomics"] / (r["splat_ms"] * 1e-3) if r["splat_ms"] > 0 else None
            results[name] = r
            log(f"{name}: {r}")
    finally:
        capi.check(lib.bahip_debug_set_render_stages(0))
    reference_sweep = None
    try:
        reference_sweep = json.load(open(os.path.join(ROOT, "profiles", "surfel_cost_eval.json")))["exact"]["sweep_ms"]
    except (OSError, KeyError, ValueError):
        pass
    line = json.dumps(dict(keyframes=args.keyframes, surfels=n, width=W, height=H, calls_per_window=calls, rounds=rounds, compute_units=units,
                           float_add_bytes_per_s=FLOAT_ADD_BYTES_PER_S, surfel_cost_sweep_ms=reference_sweep, **results))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "render_eval.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
