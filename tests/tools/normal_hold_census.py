#!/usr/bin/env python3
"""(Under tests/tools/ because nothing under scripts/ may import the oracle: tests/test_cpu_boundary.py.)

How often does a geometry step change a surfel's packed normal?  A CPU script over the oracle (no GPU): bench.py's scene recipe at
--keyframes K (same camera, planes, pose distribution over an area scaled to the keyframe count, unfiltered creation from every
keyframe, Morton sort at 2 cm, the bench's perturbation of poses and surfels), then one bundle_adjustment(min = max = 1) per
iteration with word 3 of every surfel row compared before and after.

Per iteration it prints the share of surfels whose word changed, the share of 64-surfel tiles (buffer order) with at least one and with
at least --threshold changes, and the histogram of changes per tile.  This is what the geometry step's fused route lives on
(kernels_surfel.hip: geometry_step, kFused): a surfel whose word holds is solved from the one walk, a tile with at least `threshold`
changes runs its position pass again, the others leave their changed surfels to the fix-up launch.

Note on bench.py: its timed region is iterations warmup + 1 .. warmup + steps FROM THE START STATE (the pre-pass is followed by a
reset), i.e. iterations 4 .. 23 of this table at the defaults."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--keyframes", type=int, default=12)
    p.add_argument("--iterations", type=int, default=24)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--cell", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--threshold", type=int, default=8)
    args = p.parse_args()

    from badslam_amd import se3, synthetic
    from oracle import binding as ob
    t0 = time.time()
    rng = np.random.Generator(np.random.PCG64(args.seed))
    cam = synthetic.test_camera(args.width, args.height)
    T0 = se3.exp([0.01, 0.02, 0.03, 0.004, 0.005, 0.006])
    # bench.py at "all the surfels the keyframes create": the area follows the keyframe count, so that the observations per surfel
    # are those of its defaults (200 keyframes over 17.3 m x 13 m)
    ext = np.array([17.3, 13.0, 0.6])
    ext[:2] *= np.sqrt(args.keyframes / 200.0)
    planes = synthetic.random_planes(rng, 20, slope=0.05)
    cells = ((args.width - 1) // args.cell + 1) * ((args.height - 1) // args.cell + 1)
    poses_gt = []
    for _ in range(args.keyframes):
        xi = np.concatenate([ext * (rng.random(3) - 0.5), 0.6 * (rng.random(3) - 0.5)])
        poses_gt.append(se3.mul(T0, se3.exp(xi)))
    ocam = ob.make_camera(cam, args.width, args.height)
    ocam2 = ob.make_camera(cam, args.width, args.height)
    ba = ob.OracleBA(args.keyframes * cells + 1024, 1.0 / 5000, 40.0, args.cell, ocam, ocam2, use_depth_residuals=True,
                     use_descriptor_residuals=True)
    for T, (raw, rgb) in zip(poses_gt, synthetic.render_many(poses_gt, planes, cam, args.width, args.height, 1.0 / 5000, 1)):
        ba.add_keyframe(raw, rgb, T)
    for k in range(args.keyframes):
        ba.create_surfels_for_keyframe(k, filter_new_surfels=False)
    ba.sort_surfels_spatially(0.02)
    n = ba.surfels_size
    prng = np.random.Generator(np.random.PCG64(args.seed + 1))
    for k in range(args.keyframes):
        ba.set_pose(k, synthetic.perturb_pose(prng, poses_gt[k]))
    ba.surfel_data[2, :n] += prng.uniform(0, 0.005, n).astype(np.float32)
    tiles = (n + 63) // 64
    print(f"{args.keyframes} keyframes {args.width} x {args.height}, cell {args.cell}: {n} surfels in {tiles} tiles "
          f"(scene built in {time.time() - t0:.0f} s)", flush=True)
    print("iteration  surfels changed  tiles with >= 1  tiles with >= %d   changes per tile: 0 | 1 | 2-3 | 4-7 | 8-15 | 16-31 | 32-64" % args.threshold)
    edges = [0, 1, 2, 4, 8, 16, 32, 65]
    for it in range(1, args.iterations + 1):
        before = ba.surfel_data[3, :n].view(np.uint32).copy()
        ba.bundle_adjustment(min_iterations=1, max_iterations=1, increase_ba_iteration_count=False)
        changed = np.zeros(tiles * 64, bool)
        changed[:n] = ba.surfel_data[3, :n].view(np.uint32) != before
        per_tile = changed.reshape(tiles, 64).sum(axis=1)
        hist = np.histogram(per_tile, bins=edges)[0]
        print("%9d  %14.2f%%  %14.1f%%  %15.1f%%   %s" % (it, 100.0 * changed.sum() / n, 100.0 * np.count_nonzero(per_tile) / tiles,
                                                       100.0 * np.count_nonzero(per_tile >= args.threshold) / tiles,
                                                       " | ".join("%d" % h for h in hist)), flush=True)


if __name__ == "__main__":
    main()
