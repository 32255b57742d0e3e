"""The model of the observed co-visibility (bahip_observed_covisibility; DESIGN.md section 3, "Observed co-visibility") for
tests/test_cpu_observed_covisibility.py, tests/test_gpu_observed_covisibility.py and tests/test_gpu_directba_observed_covisibility.py.
A plain module: no fixtures, no conftest.

MODEL.  A is the K x N 0/1 matrix of the oracle's per-pair `associated` flags (OracleBA.evaluate_pairs, as
tests/surfel_costs.py::oracle_pair_words and tests/tile_cull.py::pairs read them; a surfel with a NaN position has no pair).  The
matrix is A @ A.T in int64: entry (i, j) counts the surfels associated with both keyframes, the diagonal a keyframe's own pairs.  The
sweep keeps one (keyframe, mask) entry per tile of 64 surfels and keyframe with an associated surfel: their number is
tile_cull.per_tile(A).sum(), and a tile with c entries may issue at most c (c + 1) atomic adds (one per ordered pair of entries, the
diagonal once: c^2, below the ceiling of one atomic per pair and triangle).  All integers: every comparison is an equality."""
import functools

import numpy as np

from oracle import binding as ob
from tests import tile_cull, two_cameras


def associated_matrix(ba, keyframes=None, size=None):
    """The oracle's `associated` flag of every (keyframe, surfel): (K, size) bool, keyframes all or the listed ones, surfels [0, size)."""
    n = ba.surfels_size if size is None else int(size)
    ks = list(range(len(ba.keyframes))) if keyframes is None else list(keyframes)
    x = ba.surfel_data[0, :n]
    live = np.flatnonzero(x == x).astype(np.uint32)
    word = ob.OracleBA.PAIR_FIELDS["associated"][0]
    A = np.zeros((len(ks), n), bool)
    for row, k in enumerate(ks):
        if len(live):
            A[row, live] = ba.evaluate_pairs(k, live).view(np.int32)[:, word] == 1
    return A


def matrix(A):
    """A @ A.T in int64."""
    a = np.asarray(A).astype(np.int64)
    return a @ a.T


def tile_counts(A):
    """Per tile of 64 surfels the keyframes with an associated surfel in it: (T,) int64."""
    A = np.asarray(A, bool)
    if A.shape[1] == 0:
        return np.zeros(0, np.int64)
    return tile_cull.per_tile(A).sum(axis=1).astype(np.int64)


def entries(A):
    """(tile, keyframe) entries with a non-zero mask."""
    return int(tile_counts(A).sum())


def atomic_ceiling(A):
    """sum over the tiles of c (c + 1): what one atomic per pair, triangle and tile allows."""
    c = tile_counts(A)
    return int((c * (c + 1)).sum())


def sum_over_shards(A, bounds):
    """The sum of the matrices of the surfel shards [bounds[r], bounds[r + 1]) -- the words every rank of a surfel partition ends with."""
    A = np.asarray(A)
    return sum((matrix(A[:, lo:hi]) for lo, hi in zip(bounds[:-1], bounds[1:])), np.zeros((A.shape[0], A.shape[0]), np.int64))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(TwoCameraScene, oracle, A) of a scene of tests/two_cameras.py in its perturbed state (built once per process; nobody changes it)."""
    tc = two_cameras.build_scene(name)
    ba = two_cameras.build_oracle(tc)
    return tc, ba, associated_matrix(ba)


def world_matrix(name):
    """A of a world of tests/tile_cull.py: its oracle's flags."""
    return tile_cull.pairs(name).associated
