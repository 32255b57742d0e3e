"""The model of the keyframe redundancy (bahip_keyframe_observer_histogram; DESIGN.md section 3, "Keyframe redundancy") for
tests/test_cpu_keyframe_redundancy.py, tests/test_gpu_keyframe_redundancy.py and tests/test_gpu_directba_keyframe_redundancy.py.
A plain module: no fixtures, no conftest.

MODEL.  A is the K x N 0/1 matrix of tests/observed_covisibility.py (the oracle's per-pair `associated` flags; a surfel with a NaN
position has no pair).  c_s = the column sums; a surfel with A[k][s] = 1 has o = c_s - 1 other observers; hist[k][j] = the number of s
with A[k][s] = 1 and min(o, B - 1) = j.  The sweep keeps one (keyframe, mask) entry per tile of 64 surfels and keyframe with an
associated surfel (oc.tile_counts, oc.entries) and issues one atomic add per entry and bin among the entry's surfels.  The find rule and
the greedy cull are stated on tables and on A: deleting a keyframe removes its row.  All integers: every comparison is an equality."""
import functools

import numpy as np

from badslam_amd import synthetic
from oracle import binding as ob
from tests import observed_covisibility as oc


def bins_of(A, bins):
    """Per surfel min(c_s - 1, bins - 1); -1 for a surfel nobody sees: (N,) int64."""
    A = np.asarray(A, bool)
    c = A.sum(axis=0, dtype=np.int64) if A.shape[0] else np.zeros(A.shape[1], np.int64)
    return np.where(c > 0, np.minimum(c - 1, bins - 1), -1)


def table(A, bins):
    """hist (K, bins) int64."""
    A = np.asarray(A, bool)
    assert 1 <= bins <= 64
    b = bins_of(A, bins)
    hist = np.zeros((A.shape[0], bins), np.int64)
    for k in range(A.shape[0]):
        hist[k] = np.bincount(b[A[k]], minlength=bins)
    return hist


def atomic_ceiling(A, bins):
    """sum over (tile, entry) of the distinct bins among the entry's surfels: one atomic per entry and bin present in its mask."""
    A = np.asarray(A, bool)
    b = bins_of(A, bins)
    total = 0
    for lo in range(0, A.shape[1], 64):
        for row in A[:, lo:lo + 64]:
            total += len(set(b[lo:lo + 64][row].tolist()))
    return total


def nonzero_cells(A, bins):
    """sum over the tiles of the non-zero words of the tile's own table: the atomic adds of a sweep that adds nothing for an empty cell."""
    A = np.asarray(A, bool)
    b = bins_of(A, bins)
    total = 0
    for lo in range(0, A.shape[1], 64):
        t, tb = A[:, lo:lo + 64], b[lo:lo + 64]
        cells = np.zeros((A.shape[0], bins), np.int64)
        for k in range(A.shape[0]):
            cells[k] = np.bincount(tb[t[k]], minlength=bins)
        total += int(np.count_nonzero(cells))
    return total


def second_traversals(A, capacity):
    """Tiles with more entries than a list of `capacity` holds."""
    return int((oc.tile_counts(A) > capacity).sum())


def sum_over_shards(A, bounds, bins):
    """The sum of the tables of the surfel shards [bounds[r], bounds[r + 1]) -- the words every rank of a surfel partition ends with."""
    A = np.asarray(A)
    return sum((table(A[:, lo:hi], bins) for lo, hi in zip(bounds[:-1], bounds[1:])), np.zeros((A.shape[0], bins), np.int64))


def find(hist, min_other_observers, min_fraction, ids=None):
    """The find rule on a table: the ids (default: the row numbers) of the rows with total > 0 and (double)covered >= min_fraction *
    (double)total, most redundant first by the exact cross products, ties to the lower id."""
    hist = np.asarray(hist).astype(np.int64)
    assert 0 <= min_other_observers <= hist.shape[1] - 1
    ids = list(range(hist.shape[0])) if ids is None else [int(i) for i in ids]
    rows = []
    for i, row in zip(ids, hist):
        total, covered = int(row.sum()), int(row[min_other_observers:].sum())
        if total > 0 and float(covered) >= float(min_fraction) * float(total):
            rows.append((i, covered, total))

    def order(a, b):
        ab, ba = a[1] * b[2], b[1] * a[2]
        return (ba > ab) - (ba < ab) if ab != ba else (a[0] > b[0]) - (a[0] < b[0])

    return [r[0] for r in sorted(rows, key=functools.cmp_to_key(order))]


def cull(A, min_other_observers, min_fraction, max_deletions, protect_newest, ids=None, bins=16):
    """The greedy cull on A (rows = the existing keyframes in order, `ids` their ids): per round the table of the remaining rows, the
    first of find() that is neither the first remaining row nor among the protect_newest last ones is deleted.  Returns (deleted ids
    in order, stopped by the rule: no candidate was left when it ended)."""
    A = np.asarray(A, bool)
    ids = list(range(A.shape[0])) if ids is None else [int(i) for i in ids]
    deleted = []
    while len(deleted) < max_deletions:
        order = find(table(A, bins), min_other_observers, min_fraction, ids)
        allowed = [i for i in order if ids.index(i) != 0 and ids.index(i) < len(ids) - max(0, protect_newest)]
        if not allowed:
            return deleted, True
        at = ids.index(allowed[0])
        deleted.append(ids.pop(at))
        A = np.delete(A, at, axis=0)
    order = find(table(A, bins), min_other_observers, min_fraction, ids)
    return deleted, not [i for i in order if ids.index(i) != 0 and ids.index(i) < len(ids) - max(0, protect_newest)]


SEVENTY = 70


def seventy_poses():
    """The poses of the 70 keyframes of tests/test_gpu_observed_covisibility.py::_seventy: tiny's four images in turn at perturbed poses."""
    tc, _, _ = oc.scene("tiny")
    rng = np.random.Generator(np.random.PCG64(70))
    return [synthetic.perturb_pose(rng, tc.poses[k % 4]) for k in range(SEVENTY)]


def seventy_oracle(poses=None, images=None):
    """An oracle with tiny's cloud and the keyframes (images[k] of tiny's four, poses[k]); default: the 70 of seventy_poses()."""
    tc, ba4, _ = oc.scene("tiny")
    scene = tc.scene
    poses = seventy_poses() if poses is None else poses
    images = [k % 4 for k in range(len(poses))] if images is None else images
    ba = ob.OracleBA(tc.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell,
                     ob.make_camera(tc.color_camera, tc.color_width, tc.color_height), ob.make_camera(scene.camera, scene.width, scene.height))
    for image, T in zip(images, poses):
        ba.add_keyframe(scene.depth[image], scene.rgb[image], T)
    n = ba4.surfels_size
    ba.surfel_data[:, :n] = ba4.surfel_data[:, :n]
    ba.surfels.surfels_size, ba.surfels.surfel_count = n, ba4.surfels.surfel_count
    ba.active[:n] = 1
    return ba


@functools.lru_cache(maxsize=None)
def seventy_matrix():
    """A of the 70 keyframes (built once; nobody changes it)."""
    return oc.associated_matrix(seventy_oracle())


DUPLICATED_VIEWS = 12
CULL_RULE = (7, 0.6)             # (min_other_observers, min_fraction) of the cull tests on duplicated_views()


@functools.lru_cache(maxsize=None)
def duplicated_views():
    """A scene for the cull: the four views of a small synthetic scene three times over -- as they are, then twice at perturbed poses --
    on the surfels created from the first four.  (scene, images, poses, oracle, A); built once, nobody changes it."""
    from tests import common
    scene = common.small_scene(num_keyframes=4, width=160, height=120, seed=23)
    rng = np.random.Generator(np.random.PCG64(12))
    images = [k % 4 for k in range(DUPLICATED_VIEWS)]
    poses = [scene.poses_gt[k] if k < 4 else synthetic.perturb_pose(rng, scene.poses_gt[k % 4]) for k in range(DUPLICATED_VIEWS)]
    ba = ob.OracleBA(100000, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, ob.make_camera(scene.camera, scene.width, scene.height),
                     ob.make_camera(scene.camera, scene.width, scene.height))
    for image, T in zip(images, poses):
        ba.add_keyframe(scene.depth[image], scene.rgb[image], T)
    for k in range(4):
        ba.create_surfels_for_keyframe(k, filter_new_surfels=False)
    return scene, images, poses, ba, oc.associated_matrix(ba)
