"""The model of the observation lists (bahip_surfel_observations; DESIGN.md section 3, "Observation lists") for
tests/test_cpu_surfel_observations.py, tests/test_gpu_surfel_observations.py and tests/test_gpu_directba_surfel_observations.py.
A plain module: no fixtures, no conftest.

MODEL.  A is the K x N 0/1 matrix of tests/observed_covisibility.py (the oracle's per-pair `associated` flags; a surfel with a NaN
position has no pair).  The table is A in compressed rows by surfel: surfel_first = the exclusive prefix sum of A's column sums
(N + 1 uint32 words, the last one P), keyframes = per surfel the row indices of its ones, ascending (P uint16 words).  The payload, entry
for entry, is the oracle's pair record (OracleBA.evaluate_pairs, as tests/surfel_costs.py::oracle_pair_words reads it): the word of
depth_residual, and the two words of desc_residual where color_valid is 1, else 0x7fc00000 twice.  All comparisons are equalities of
integer words (the payload planes are compared as uint32 bit patterns)."""
import functools

import numpy as np

from oracle import binding as ob
from tests import observed_covisibility as oc
from tests import tile_cull

NAN_WORD = 0x7fc00000


def csr(A):
    """A (K, N) 0/1 -> (surfel_first (N + 1,) uint32, keyframes (P,) uint16): per surfel its keyframes, ascending."""
    A = np.asarray(A, bool)
    K, n = A.shape
    assert K < 65536
    counts = A.sum(axis=0, dtype=np.int64) if K else np.zeros(n, np.int64)
    first = np.concatenate([[0], np.cumsum(counts)])
    assert first[-1] < 2 ** 32
    s, k = np.nonzero(A.T)                              # row-major over (surfel, keyframe): by surfel, then keyframe ascending
    return first.astype(np.uint32), k.astype(np.uint16)


def dense(surfel_first, keyframes, K):
    """The inverse: (K, N) bool from the compressed rows (asserts what makes them well formed)."""
    first = np.asarray(surfel_first).astype(np.int64)
    ks = np.asarray(keyframes).astype(np.int64)
    n = len(first) - 1
    assert first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] == len(ks), (first[:4], first[-1], len(ks))
    assert ((ks >= 0) & (ks < max(K, 1))).all() or len(ks) == 0
    s = np.repeat(np.arange(n), np.diff(first))
    A = np.zeros((K, n), bool)
    A[ks, s] = True
    assert int(A.sum()) == len(ks), "a keyframe twice in one list"
    inner = np.flatnonzero(np.diff(ks) <= 0) + 1          # where k does not ascend, a new list must begin
    assert np.isin(inner, first).all(), "a list that does not ascend"
    return A


def raw_words(ba, A, keyframes=None):
    """(depth (P,) uint32, descriptor (P, 2) uint32): the oracle's words of the pairs of A (rows = `keyframes` of the oracle, all by
    default), in the table's order."""
    A = np.asarray(A, bool)
    K, n = A.shape
    ks = list(range(len(ba.keyframes))) if keyframes is None else list(keyframes)
    assert len(ks) == K
    off = ob.OracleBA.PAIR_FIELDS
    first, _ = csr(A)
    P = int(first[-1])
    depth = np.zeros(P, np.uint32)
    desc = np.full((P, 2), NAN_WORD, np.uint32)
    slot = first[:-1].astype(np.int64) + np.cumsum(A, axis=0) - A          # (K, N): where the pair (k, s) stands
    for row, k in enumerate(ks):
        idx = np.flatnonzero(A[row]).astype(np.uint32)
        if not len(idx):
            continue
        words = ba.evaluate_pairs(k, idx)
        assert (words[:, off["associated"][0]] == 1).all()
        at = slot[row, idx]
        depth[at] = words[:, off["depth_residual"][0]]
        valid = words[:, off["color_valid"][0]] == 1
        d0 = off["desc_residual"][0]
        desc[at[valid]] = words[valid][:, d0:d0 + 2]
    return depth, desc


def table(ba, A, keyframes=None):
    """The whole table: dict of pairs, surfel_first, keyframes, depth_raw, descriptor_raw (the payload as uint32 words)."""
    first, ks = csr(A)
    depth, desc = raw_words(ba, A, keyframes)
    return dict(pairs=int(first[-1]), surfel_first=first, keyframes=ks, depth_raw=depth, descriptor_raw=desc)


def take(t, lo, hi):
    """The table of the surfels [lo, hi): what a call over that shard returns."""
    first = t["surfel_first"].astype(np.int64)
    a, b = int(first[lo]), int(first[hi])
    return dict(pairs=b - a, surfel_first=(first[lo:hi + 1] - a).astype(np.uint32), keyframes=t["keyframes"][a:b], depth_raw=t["depth_raw"][a:b],
                descriptor_raw=t["descriptor_raw"][a:b])


def permuted(t, perm):
    """The table of the cloud whose surfel i is surfel perm[i] of t's: lists move with their surfels."""
    first = t["surfel_first"].astype(np.int64)
    lengths = np.diff(first)[perm]
    new_first = np.concatenate([[0], np.cumsum(lengths)])
    src = np.concatenate([np.arange(first[p], first[p + 1]) for p in perm]) if len(perm) else np.zeros(0, np.int64)
    src = src.astype(np.int64)
    return dict(pairs=t["pairs"], surfel_first=new_first.astype(np.uint32), keyframes=t["keyframes"][src], depth_raw=t["depth_raw"][src],
                descriptor_raw=t["descriptor_raw"][src])


def words(plane):
    """A payload plane as uint32 bit patterns (float32 from the device, or the model's uint32)."""
    a = np.ascontiguousarray(plane)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


def assert_same(got, expected, what="", planes=("keyframes", "depth_raw", "descriptor_raw")):
    """pairs, surfel_first and the first P entries of every plane of `planes` that `got` holds, word for word."""
    P = expected["pairs"]
    assert got["pairs"] == P, (what, got["pairs"], P)
    assert got["surfel_first"].dtype == np.uint32 and np.array_equal(got["surfel_first"], expected["surfel_first"]), \
        (what, np.flatnonzero(got["surfel_first"] != expected["surfel_first"])[:5])
    for name in planes:
        if name not in got:
            continue
        a, b = words(got[name][:P]) if name != "keyframes" else got[name][:P], expected[name]
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist())


def lengths(first):
    return np.diff(np.asarray(first).astype(np.int64))


def gaps(first, keyframes):
    """Lists that skip a keyframe: not a contiguous run of indices."""
    first = np.asarray(first).astype(np.int64)
    ks = np.asarray(keyframes).astype(np.int64)
    n = np.diff(first)
    has = n > 0
    span = np.zeros(len(n), np.int64)
    span[has] = ks[first[1:][has] - 1] - ks[first[:-1][has]] + 1
    return int(np.count_nonzero(span > n))


def per_tile(first):
    """Pairs per tile of 64 surfels."""
    first = np.asarray(first).astype(np.int64)
    n = len(first) - 1
    edges = np.minimum(np.arange(0, n + 64, 64), n)
    return np.diff(first[edges])


@functools.lru_cache(maxsize=None)
def scene(name):
    """(TwoCameraScene, oracle, A, table) of a scene of tests/two_cameras.py in its perturbed state (built once; nobody changes it)."""
    tc, ba, A = oc.scene(name)
    return tc, ba, A, table(ba, A)


@functools.lru_cache(maxsize=None)
def world(name):
    """(world, oracle, A, table) of a world of tests/tile_cull.py."""
    w = tile_cull.world(name)
    ba = tile_cull.build_oracle(w)
    A = oc.world_matrix(name)
    return w, ba, A, table(ba, A)
