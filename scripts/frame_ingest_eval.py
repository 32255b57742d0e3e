#!/usr/bin/env python3
"""Times frame ingestion at a pyramid level (kernels_ingest.hip) on a 1280 x 960 frame, each call into device images allocated up front:
  median_iteration_ms    bahip_median_filter_and_densify, one iteration at 1280 x 960
  depth_downscale_ms     bahip_downscale_depth_median, 1280 x 960 -> 640 x 480 (blocks of 2 x 2)
  rgb_level_1_ms         bahip_downscale_rgb_half, 1280 x 960 at level 1
  bilateral_ms           for scale: the existing bahip_bilateral_filtering_and_depth_cutoff at 1280 x 960 with the defaults of
                         PreprocessConfig (sigma_xy 1.5, radius factor 2, sigma_inv_depth 0.005)
The depth image is a smooth surface in TUM units with noise and 10 % holes; the colour image is random.  Each figure is the median of
`rounds` windows of `calls` calls between two waits for the stream, so it holds the launch as well as the kernel.  Before timing, each
result is compared with the plain model of tests/frame_ingest.py on a 64-row band of the frame.  Prints one JSON line and writes it to
profiles/frame_ingest_eval.json."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1280, 960


def main():
    from badslam_amd import capi, lowlevel as ll
    from tests import frame_ingest as fi
    calls = int(os.environ.get("INGEST_EVALS", "5000"))
    rounds = int(os.environ.get("INGEST_ROUNDS", "5"))
    rng = np.random.Generator(np.random.PCG64(1))
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (9000 + 2500 * np.sin(xx / 97.0) * np.cos(yy / 71.0) + rng.integers(-8, 9, (H, W))).astype(np.int64)
    depth = np.where(rng.random((H, W)) < 0.1, 0, depth).astype(np.uint16)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    ctx = ll.Context()
    lib, h = ctx.lib, ctx.handle
    d_in = ll.DeviceBuffer2D(ctx, H, W, np.uint16).upload(depth)
    d_out = ll.DeviceBuffer2D(ctx, H, W, np.uint16)
    d_half = ll.DeviceBuffer2D(ctx, H // 2, W // 2, np.uint16)
    c_in = ll.DeviceBuffer2D(ctx, H, W, np.uint8, 3).upload(rgb)
    c_half = ll.DeviceBuffer2D(ctx, H // 2, W // 2, np.uint8, 3)
    calls_by_name = {
        "median_iteration_ms": lambda: lib.bahip_median_filter_and_densify(h, d_in.ptr, d_in.pitch, d_out.ptr, d_out.pitch, W, H),
        "depth_downscale_ms": lambda: lib.bahip_downscale_depth_median(h, d_in.ptr, d_in.pitch, W, H, d_half.ptr, d_half.pitch, W // 2, H // 2),
        "rgb_level_1_ms": lambda: lib.bahip_downscale_rgb_half(h, c_in.ptr, c_in.pitch, W, H, 1, c_half.ptr, c_half.pitch),
        "bilateral_ms": lambda: lib.bahip_bilateral_filtering_and_depth_cutoff(h, 1.5, 0.005, 2.0, 15000, 1.0 / 5000, d_in.ptr, d_in.pitch,
                                                                               d_out.ptr, d_out.pitch, W, H),
    }
    # what is timed is what the model says: a band of the frame (the model is plain Python)
    band = slice(448, 512)
    capi.check(calls_by_name["median_iteration_ms"]())
    assert np.array_equal(d_out.download()[band][1:-1], fi.median_filter_and_densify(depth[band])[1:-1])
    capi.check(calls_by_name["depth_downscale_ms"]())
    assert np.array_equal(d_half.download()[band.start // 2:band.stop // 2], fi.downscale_depth_median(depth[band], W // 2, 32))
    capi.check(calls_by_name["rgb_level_1_ms"]())
    assert np.array_equal(c_half.download()[band.start // 2:band.stop // 2], fi.downscale_rgb_half(rgb[band], 1))

    def window(call):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            capi.check(call())
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    results = {}
    for name, call in calls_by_name.items():
        window(call)                                                          # warm-up
        timed = [window(call) for _ in range(rounds)]
        results[name] = statistics.median(timed)
        results[name.replace("_ms", "_ms_spread")] = [min(timed), max(timed)]
        print(f"{name}: {results[name]:.4f} ms (min {min(timed):.4f}, max {max(timed):.4f})", file=sys.stderr, flush=True)
    line = json.dumps(dict(width=W, height=H, calls_per_window=calls, rounds=rounds, holes=float(np.mean(depth == 0)), **results))
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "frame_ingest_eval.json"), "w") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
