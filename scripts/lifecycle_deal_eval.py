#!/usr/bin/env python3
"""The drop-in call under surfel sharding with the lifecycle replicated and dealt (DirectBA.SetDistributedLifecycle).

Runs BundleAdjustment(do_surfel_updates=True, ten iterations, full window) from no surfels on G in-process ranks on ONE GPU (threads,
one DirectBA each on a HIP stream of its own, the loopback all-reduce of tests/test_gpu_sharded_loopback.py), for G = 1, 2, 4 and 8,
with the mode off and on.  The first call from no surfels creates surfels keyframe by keyframe (no lifecycle batch knows tiles of an
empty cloud), so its creation is not dealt in either mode; merging and deletion are.  Per rank it reports the exchanges (bahip_exchange_stats: calls and bytes), what the rank swept of the dealt phases
(bahip_debug_lifecycle_deal_stats) and the wall time of the call; every rank's cloud and poses are checked against G = 1.

--trace: the same runs once more under `rocprofv3 --kernel-trace` in a child process of their own, and the kernel time of the lifecycle
phases (creation, merging, deletion, compaction, gather / extract, spatial sort) summed per stream from its kernel trace.  The runs are
sequential and every rank creates a new stream, so the streams, in the order their first lifecycle kernel started, are assigned to the
runs in order, `world` streams per run.  The ranks share one GPU, so these are kernel times, not a scaling measurement; real links are not measured.

Writes profiles/lifecycle_deal_eval.json (and profiles/lifecycle_deal_kernels.json with --trace)."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIFECYCLE_KERNELS = ("create_", "merge_", "supporting_", "delete_", "compact_", "lifecycle_", "shard_to_cloud", "cloud_to_shard", "sort_keys",
                     "gather_rows", "scatter_rows")


def parse_args():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--keyframes", type=int, default=16)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--iterations", type=int, default=10)
    p.add_argument("--chunk", type=int, default=4096)
    p.add_argument("--worlds", default="1,2,4,8")
    p.add_argument("--trace", action="store_true", help="also run once under rocprofv3 --kernel-trace and split the lifecycle kernel time by stream")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lifecycle_deal_eval.json"))
    return p.parse_args()


def run(args):
    import torch
    from badslam_amd import capi, multigpu, synthetic
    from badslam_amd.directba import DirectBA
    from tests.test_gpu_sharded_loopback import _Loopback
    torch.cuda.set_device(0)
    scene = synthetic.make_scene(args.keyframes, args.width, args.height, seed=3, cell=2, translation_range=1.0, rotation_range=0.4)
    rng = np.random.Generator(np.random.PCG64(9))
    start = [synthetic.perturb_pose(rng, T, 0.002, 0.0005) for T in scene.poses_gt]
    capacity = (args.width * args.height // 4 * args.keyframes + 4095) // 4096 * 4096

    def build(stream):
        ba = DirectBA(capacity, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera,
                      stream=stream)
        for k in range(len(scene.depth)):
            ba.AddKeyframe(scene.depth[k], scene.rgb[k], start[k])
        ba.set_pcg_gauge_keyframe(0)
        return ba

    def call(ba):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ba.BundleAdjustment(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=args.iterations,
                            max_iterations=args.iterations, increase_ba_iteration_count=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    runs, reference = [], None
    for world in [int(w) for w in args.worlds.split(",")]:
        for dealing in ((False,) if world == 1 else (False, True)):
            loop = _Loopback(world) if world > 1 else None
            out, errors = [None] * world, []

            def rank_main(rank):
                try:
                    torch.cuda.set_device(0)
                    handle = C.c_void_p()                             # a new HIP stream of this rank's own (never a pooled one)
                    capi.check(capi.load().bahip_stream_create(C.byref(handle)))
                    stream = handle.value
                    ba = build(stream)
                    ctx = ba.backend_context()
                    hook = None
                    if world > 1:
                        hook = loop.hook_for(rank)
                        capi.check(ctx.lib.bahip_context_set_allreduce(ctx.handle, hook, None))
                        ba.SetSurfelSharding(rank, world, args.chunk)
                    ba.SetDistributedLifecycle(dealing)
                    capi.check(ctx.lib.bahip_exchange_stats(ctx.handle, None, None, 1))
                    wall = call(ba)
                    calls, nbytes = C.c_longlong(), C.c_longlong()
                    capi.check(ctx.lib.bahip_exchange_stats(ctx.handle, C.byref(calls), C.byref(nbytes), 1))
                    stats = (C.c_longlong * 8)()
                    capi.check(ctx.lib.bahip_debug_lifecycle_deal_stats(ctx.handle, stats, 1))
                    out[rank] = dict(rank=rank, wall_ms=round(wall * 1e3, 2), exchange_calls=calls.value, exchange_bytes=nbytes.value,
                                     deal_stats=list(stats), surfels=ba.download_surfels(8), poses=[ba.keyframe_pose(k) for k in range(len(start))],
                                     keep=(hook, ba, stream))
                except Exception as e:   # noqa: BLE001
                    errors.append((rank, repr(e)))
                    if loop:
                        loop.barrier.abort()

            threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            if errors:
                raise RuntimeError(errors)
            total = sum(r["surfels"].shape[1] for r in out)
            cloud = np.zeros((8, total), np.float32)
            for r in out:
                cloud[:, multigpu.shard_chunks(total, r["rank"], world, chunk=args.chunk)] = r["surfels"]
            if reference is None:
                reference = (cloud, out[0]["poses"])
            same = bool(np.array_equal(cloud.view(np.uint32), reference[0].view(np.uint32)) and
                        all(np.array_equal(a, b) for r in out for a, b in zip(r["poses"], reference[1])))
            runs.append(dict(world=world, dealing=dealing, surfels=total, bits_equal_to_world_1=same,
                             ranks=[{k: v for k, v in r.items() if k not in ("surfels", "poses", "keep")} for r in out]))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    return dict(scene=dict(keyframes=args.keyframes, width=args.width, height=args.height, iterations=args.iterations, chunk=args.chunk),
                deal_stats_fields=["creation keyframes swept", "sum of their index + 1", "merge keyframes swept", "sum of their index + 1",
                                   "deletion surfels swept", "dealt calls", "creation candidates exchanged", "merge pairs exchanged"], runs=runs)


def trace(args):
    """One run under rocprofv3 --kernel-trace (a child process): lifecycle kernel time per stream, in the order the streams appear."""
    d = tempfile.mkdtemp(prefix="lifecycle_deal_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "trace", "--", sys.executable, os.path.abspath(__file__),
           "--keyframes", str(args.keyframes), "--width", str(args.width), "--height", str(args.height), "--iterations", str(args.iterations),
           "--chunk", str(args.chunk), "--worlds", args.worlds, "--out", os.path.join(d, "run.json")]
    subprocess.run(cmd, check=True, timeout=3000)
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"no kernel trace under {d}")
    rows = list(csv.DictReader(open(files[0])))
    stream_key = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
    per_stream, order = {}, []
    for row in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = row["Kernel_Name"]
        short = name.split("(")[0].split("::")[-1].split("<")[0]
        if not any(short.startswith(p) for p in LIFECYCLE_KERNELS):
            continue
        sid = row[stream_key]
        if sid not in per_stream:
            per_stream[sid] = {}
            order.append(sid)
        ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        per_stream[sid][short] = per_stream[sid].get(short, 0) + ns
    def summary(sid):
        kernels = per_stream[sid]
        return dict(stream=sid, lifecycle_kernel_ms=round(sum(kernels.values()) / 1e6, 3),
                    by_kernel_ms={k: round(v / 1e6, 3) for k, v in sorted(kernels.items())})

    # the null stream (id 0) belongs to no rank: what runs there (buffer set-up before a DirectBA has its stream) is listed apart
    default = [summary(sid) for sid in order if sid == "0"]
    order = [sid for sid in order if sid != "0"]
    sequence = [(w, d) for w in [int(w) for w in args.worlds.split(",")] for d in ((False,) if w == 1 else (False, True))]
    if len(order) != sum(w for w, _ in sequence):
        return dict(grouped_by=stream_key, note=f"{len(order)} rank streams in the trace for {sum(w for w, _ in sequence)} ranks: not assigned to runs",
                    default_stream=default, streams=[summary(sid) for sid in order])
    runs, at = [], 0
    for world, dealing in sequence:
        ranks = []
        for sid in order[at:at + world]:
            ranks.append(summary(sid))
        at += world
        runs.append(dict(world=world, dealing=dealing, max_rank_lifecycle_kernel_ms=max(r["lifecycle_kernel_ms"] for r in ranks), ranks=ranks))
    return dict(grouped_by=stream_key, note="one stream per rank; the ranks of a run in the order their first lifecycle kernel started (not "
                "necessarily rank order); the ranks share one GPU, so their kernels overlap and slow each other", default_stream=default, runs=runs)


def main():
    args = parse_args()
    result = run(args)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(dict(runs=[(r["world"], r["dealing"], r["bits_equal_to_world_1"]) for r in result["runs"]])))
    if args.trace:
        kernels = trace(args)
        with open(os.path.join(os.path.dirname(args.out), "lifecycle_deal_kernels.json"), "w") as f:
            json.dump(kernels, f, indent=1)


if __name__ == "__main__":
    main()
