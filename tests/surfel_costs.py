"""A CPU model of the bundle-adjustment objective per surfel ("The objective per surfel") for
tests/test_cpu_surfel_costs.py, tests/test_gpu_surfel_costs.py and tests/test_gpu_directba_surfel_costs.py, and the helpers they
share.  A plain module: no fixtures, no conftest.

The model: per (surfel, keyframe) pair the ORACLE's evaluate_pairs words (oracle.binding.OracleBA.PAIR_FIELDS: associated, color_valid,
depth_residual, desc_residual); the robust costs in binary32, operation for operation as tests/test_gpu_cost.py spells them
(_tukey_cost, _huber_cost), here vectorised in numpy float32 (numpy rounds every elementwise operation to binary32 and contracts
nothing); per surfel math.fsum of the terms of all keyframes -- the exact sum rounded once to binary64.  A surfel with a non-finite term
has three NaN sums and keeps its counts."""
import math

import numpy as np

from oracle import binding as ob

F32 = np.float32
KINDS = [(True, True), (True, False), (False, True)]
SUMS = ("depth", "descriptor_1", "descriptor_2")
COUNTS = ("depth_residuals", "descriptor_pairs")
PLANES = SUMS + COUNTS
REL = 2.0 ** -51     # fsum of the per-surfel sums against a total: three roundings of 2^-53 relative, all terms >= 0


def tukey_cost(r):
    """tests/test_gpu_cost.py::_tukey_cost on an array: 1 * tukey_residual(r, 10) in binary32."""
    r = np.asarray(r, F32)
    k, c = F32(10), F32(1) / F32(6)
    with np.errstate(invalid="ignore", over="ignore"):
        q = r * F32(0.1)
        t = F32(1) - q * q
        inside = F32(1) * (c * k * k * (F32(1) - t * t * t))
        outside = F32(1) * (c * k * k)
        return np.where(np.abs(r) < k, inside, outside).astype(F32)


def huber_cost(r):
    """tests/test_gpu_cost.py::_huber_cost on an array: 1 * 1e-2 * huber_residual(r, 10) in binary32."""
    r = np.asarray(r, F32)
    k = F32(10)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(r)
        h = np.where(a < k, F32(0.5) * r * r, k * (a - F32(0.5) * k)).astype(F32)
        return ((F32(1) * F32(1e-2)) * h).astype(F32)


def oracle_pair_words(ba, keyframes=None):
    """Per keyframe (all, or the listed ones) the oracle's (surfels_size, 37) pair words."""
    idx = np.arange(ba.surfels_size, dtype=np.uint32)
    return [ba.evaluate_pairs(k, idx) for k in (range(len(ba.keyframes)) if keyframes is None else keyframes)]


def pair_terms(words):
    """One keyframe's words -> (associated, with a descriptor pair, depth terms, descriptor-1 terms, descriptor-2 terms), the terms
    binary32 and meaningful under their mask."""
    off = ob.OracleBA.PAIR_FIELDS
    associated = words[:, off["associated"][0]] == 1
    paired = associated & (words[:, off["color_valid"][0]] == 1)
    depth = tukey_cost(np.ascontiguousarray(words[:, off["depth_residual"][0]]).view(F32))
    d0 = off["desc_residual"][0]
    desc1 = huber_cost(np.ascontiguousarray(words[:, d0]).view(F32))
    desc2 = huber_cost(np.ascontiguousarray(words[:, d0 + 1]).view(F32))
    return associated, paired, depth, desc1, desc2


def model(per_keyframe_words, use_depth, use_desc, size=None):
    """The five planes (dict of numpy arrays: float64 sums, uint32 counts) from the pair words of the bound keyframes."""
    n = (per_keyframe_words[0].shape[0] if per_keyframe_words else 0) if size is None else size
    terms = [[[] for _ in range(n)] for _ in SUMS]
    counts = {name: np.zeros(n, np.uint32) for name in COUNTS}
    for words in per_keyframe_words:
        associated, paired, depth, desc1, desc2 = pair_terms(words[:n])
        if use_depth:
            counts["depth_residuals"] += associated
            for i in np.flatnonzero(associated):
                terms[0][i].append(float(depth[i]))
        if use_desc:
            counts["descriptor_pairs"] += paired
            for i in np.flatnonzero(paired):
                terms[1][i].append(float(desc1[i]))
                terms[2][i].append(float(desc2[i]))
    out = {name: np.zeros(n, np.float64) for name in SUMS}
    for i in range(n):
        mine = [terms[c][i] for c in range(3)]
        if all(math.isfinite(v) for t in mine for v in t):
            for name, t in zip(SUMS, mine):
                out[name][i] = math.fsum(t)
        else:
            for name in SUMS:
                out[name][i] = math.nan
    out.update(counts)
    return out


def bits(planes):
    """The planes as a tuple of integer arrays: the words of the binary64 sums (every NaN as one word) and the counts."""
    res = []
    for name in PLANES:
        if name not in planes:
            continue
        a = np.ascontiguousarray(planes[name])
        if name in SUMS:
            assert a.dtype == np.float64, (name, a.dtype)
            w = a.view(np.uint64).copy()
            w[np.isnan(a)] = np.uint64(0x7ff8000000000000)
            res.append(w)
        else:
            assert a.dtype == np.uint32, (name, a.dtype)
            res.append(a.astype(np.uint64))
    return tuple(res)


def assert_same_bits(got, expected, what=""):
    """Every plane equal word for word (+0.0 is not -0.0; NaN equals NaN); names the first rows that differ."""
    assert set(got) == set(expected), (what, sorted(got), sorted(expected))
    for name, a, b in zip([n for n in PLANES if n in got], bits(got), bits(expected)):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, name, int(bad.size), [(int(i), got[name][i], expected[name][i]) for i in bad[:5]])


def take(planes, index):
    """planes[index] on every plane (a prefix, a permutation, a shard)."""
    return {name: np.ascontiguousarray(a[index]) for name, a in planes.items()}


def totals(planes):
    """math.fsum of the three sums and the integer sums of the two counts."""
    out = {name: math.fsum(map(float, planes[name])) for name in SUMS}
    out.update({name: int(planes[name].astype(np.uint64).sum()) for name in COUNTS})
    return out


def assert_consistent_with_cost(planes, cost, what=""):
    """Check 2 of the definition: count sums equal the cost's counts, fsum of each plane within 2^-51 relative of the cost's sum."""
    t = totals(planes)
    for name in COUNTS:
        assert t[name] == cost[name], (what, name, t[name], cost[name])
    for name in SUMS:
        assert abs(t[name] - cost[name]) <= REL * abs(cost[name]), (what, name, t[name], cost[name])


def census(planes, keyframes):
    """How many surfels have no term, are seen by all `keyframes`, and have a depth term but no descriptor pair."""
    d, p = planes["depth_residuals"], planes["descriptor_pairs"]
    return dict(none=int(np.count_nonzero((d == 0) & (p == 0))), by_all=int(np.count_nonzero(d == keyframes)),
                depth_only=int(np.count_nonzero((d > 0) & (p == 0))))
