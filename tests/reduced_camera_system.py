"""The model of the reduced camera system (bahip_reduced_camera_system; DESIGN.md section 3, "The reduced camera system") for
tests/test_cpu_reduced_camera_system.py and tests/test_gpu_reduced_camera_system.py.  A plain module: no fixtures, no conftest.

MODEL32 states the definition operation for operation in numpy binary32 (one rounding per operation; `fma` is the exact fused
multiply-add of tests/render_view.py), from the oracle's per-pair words (OracleBA.evaluate_pairs: residuals, weights, pose and
surfel Jacobians).  Per surfel, over its associated keyframes in ascending order, the eight sums of the geometry step, C = sums + 1e-6
on the diagonal, the in-place Cholesky factor L and z = L^-1 c; per pair E (6 x m) and Y = E L^-T by forward substitution; per tile of
64 surfels the fixed tree (tile_tree_sum, the restatement of orc_tile_tree_sum over many tiles at once) of the lane products, split
into the two fixed-point limbs (pose_limbs: orc_pose_limbs over arrays) and added as integers; A and b are the pose equations with
the same definition (orc_accumulate_pose_coeffs_fixed, restated from the pair words so that prefixes, shards and hand-made pairs
have them too).  S_kl = delta_kl A_k - M_kl and g_k = b_k - v_k in binary64 from the resolved sums.  Every comparison of the GPU
with MODEL32 is an equality of bits.

REFERENCE64 is the same system in binary64 from the same pair words: per surfel the 3 x 3 (1 x 1) block is inverted with numpy, so
it shares no rounding with MODEL32 beyond the words themselves; it also gives, per word of S, the sum of the magnitudes of its
terms, which scales the bound of tests/test_cpu_reduced_camera_system.py."""
import functools

import numpy as np

from oracle import binding as ob
from tests import tile_cull, two_cameras
from tests.render_view import fma

F = np.float32
ATOMICS_PER_ENTRY, ATOMICS_PER_PAIR, ATOMICS_PER_DIAGONAL_PAIR = 12, 72, 42
DEFAULT_LIST_CAPACITY = 8
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]          # the row-major upper triangle of the pose equations


# ---- the fixed tree and the fixed point, over arrays ----------------------------------------------------------------------------------
def tile_tree_sum(x):
    """orc_tile_tree_sum over the last axis (64 lanes) of a binary32 array."""
    x = np.asarray(x, F)
    v = x.reshape(x.shape[:-1] + (8, 8))                 # v[..., m, c] = lane c + 8 m
    with np.errstate(invalid="ignore", over="ignore"):
        s04, s26, s15, s37 = v[..., 0, :] + v[..., 4, :], v[..., 2, :] + v[..., 6, :], v[..., 1, :] + v[..., 5, :], v[..., 3, :] + v[..., 7, :]
        A = (s04 + s26) + (s15 + s37)
        b0, b1, b2, b3 = A[..., 0] + A[..., 7], A[..., 1] + A[..., 6], A[..., 2] + A[..., 5], A[..., 3] + A[..., 4]
        return (b0 + b2) + (b1 + b3)


def pose_limbs(v):
    """orc_pose_limbs over a binary32 array: (lo, hi, valid) -- the multiples of 2^-32 and of 1, int64."""
    bits = np.asarray(v, F).view(np.uint32).astype(np.int64)
    e, m = (bits >> 23) & 0xff, bits & 0x7fffff
    m = np.where(e != 0, m | 0x800000, m)
    e = np.where(e != 0, e, 1)
    s = e - 118
    valid = s <= 60
    lo, hi = np.zeros(bits.shape, np.int64), np.zeros(bits.shape, np.int64)
    big = valid & (s >= 32)
    hi = np.where(big, m << np.clip(s - 32, 0, 28), hi)
    mid = valid & (s >= 0) & (s < 32)
    w = m << np.clip(s, 0, 31)
    lo = np.where(mid, w & 0xffffffff, lo)
    hi = np.where(mid, w >> 32, hi)
    small = valid & (s < 0) & (s >= -25)
    sh = np.clip(-s, 1, 25)
    q, rem, half = m >> sh, m & ((1 << sh) - 1), 1 << (sh - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    lo = np.where(small, q, lo)
    neg = (bits >> 31) != 0
    return np.where(neg, -lo, lo), np.where(neg, -hi, hi), valid


def limbs_value(lo, hi):
    """orc_pose_limbs_value over int64 arrays."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    return (hi + (lo >> 32)).astype(np.float64) + (lo & 0xffffffff).astype(np.float64) * 2.0 ** -32


class Limbs:
    """A table of fixed-point sums: add tile totals (binary32, first axis = tiles, `use` = the tiles that count), read values."""

    def __init__(self, shape):
        self.lo, self.hi, self.invalid = np.zeros(shape, np.int64), np.zeros(shape, np.int64), False

    def add(self, index, totals, use):
        lo, hi, valid = pose_limbs(totals)
        take = valid & use.reshape((-1,) + (1,) * (totals.ndim - 1))
        self.invalid = self.invalid or bool((~valid & use.reshape((-1,) + (1,) * (totals.ndim - 1))).any())
        self.lo[index] += np.where(take, lo, 0).sum(axis=0)
        self.hi[index] += np.where(take, hi, 0).sum(axis=0)

    def values(self):
        if (np.abs(self.hi) >= 2 ** 62).any():
            self.invalid = True
        return limbs_value(self.lo, self.hi)


# ---- the pair words ------------------------------------------------------------------------------------------------------------------
class Words:
    """Per (keyframe, surfel): associated, color (the colour pixel is valid), and the binary32 words raw, w, Jgeom, Jpose[6], raw1,
    raw2, w1, w2, Jg1, Jg2, Jp1[6], Jp2[6] -- zeros where the pair is not associated."""
    FIELDS = ("raw", "w", "Jgeom", "raw1", "raw2", "w1", "w2", "Jg1", "Jg2")

    def __init__(self, K, n):
        self.K, self.n = K, n
        self.associated, self.color = np.zeros((K, n), bool), np.zeros((K, n), bool)
        for name in self.FIELDS:
            setattr(self, name, np.zeros((K, n), F))
        self.Jpose, self.Jp1, self.Jp2 = (np.zeros((K, n, 6), F) for _ in range(3))

    def take(self, surfels, keyframes=None):
        """The words of a subset of the surfels (a slice or an index array) and keyframes."""
        ks = np.arange(self.K) if keyframes is None else np.asarray(keyframes)
        idx = np.arange(self.n)[surfels]
        out = Words(len(ks), len(idx))
        for name in ("associated", "color", "Jpose", "Jp1", "Jp2") + self.FIELDS:
            setattr(out, name, getattr(self, name)[np.ix_(ks, idx)])
        return out


def oracle_words(ba, keyframes=None):
    """The Words of an oracle's current state: every live surfel against every keyframe (or the listed ones)."""
    n = ba.surfels_size
    ks = list(range(len(ba.keyframes))) if keyframes is None else list(keyframes)
    x = ba.surfel_data[0, :n]
    live = np.flatnonzero(x == x).astype(np.uint32)
    w = Words(len(ks), n)
    field = ob.OracleBA.PAIR_FIELDS
    for row, k in enumerate(ks):
        if not len(live):
            continue
        raw = ba.evaluate_pairs(k, live)
        ints, floats = raw.view(np.int32), raw.view(F)
        get = lambda name: floats[:, field[name][0]:field[name][0] + field[name][1]]          # noqa: E731
        a = ints[:, field["associated"][0]] == 1
        c = a & (ints[:, field["color_valid"][0]] == 1)
        w.associated[row, live], w.color[row, live] = a, c
        zero = lambda v, keep: np.where(keep.reshape((-1,) + (1,) * (v.ndim - 1)), v, F(0))          # noqa: E731
        w.raw[row, live], w.w[row, live] = zero(get("depth_residual")[:, 0], a), zero(get("depth_weight")[:, 0], a)
        w.Jgeom[row, live], w.Jpose[row, live] = zero(get("depth_jac_surfel")[:, 0], a), zero(get("depth_jac_pose"), a)
        w.raw1[row, live], w.raw2[row, live] = zero(get("desc_residual")[:, 0], c), zero(get("desc_residual")[:, 1], c)
        w.w1[row, live], w.w2[row, live] = zero(get("desc_weight")[:, 0], c), zero(get("desc_weight")[:, 1], c)
        w.Jg1[row, live], w.Jg2[row, live] = zero(get("desc_jac_surfel")[:, 0], c), zero(get("desc_jac_surfel")[:, 1], c)
        w.Jp1[row, live], w.Jp2[row, live] = zero(get("desc_jac_pose")[:, :6], c), zero(get("desc_jac_pose")[:, 6:], c)
    return w


# ---- MODEL32 -----------------------------------------------------------------------------------------------------------------------
def factor32(w, use_depth, use_desc):
    """Per surfel the factor (L00, L10, L20, L11, L21, L22), z (3) and whether it is degenerate."""
    n = w.n
    a0, a1, a2, a3, a5, a6, a7, a8 = (np.zeros(n, F) for _ in range(8))
    jd = F(-1)
    with np.errstate(all="ignore"):
        for k in range(w.K):
            if use_depth:
                on = w.associated[k]
                a0 = np.where(on, fma(w.w[k] * w.Jgeom[k], w.Jgeom[k], a0), a0)
                a6 = np.where(on, fma(w.w[k] * w.raw[k], w.Jgeom[k], a6), a6)
            if use_desc:
                on = w.color[k]
                wr1, wr2 = w.w1[k] * w.raw1[k], w.w2[k] * w.raw2[k]
                a0 = np.where(on, fma(w.w2[k] * w.Jg2[k], w.Jg2[k], fma(w.w1[k] * w.Jg1[k], w.Jg1[k], a0)), a0)
                a1 = np.where(on, a1 + w.w1[k] * w.Jg1[k] * jd, a1)
                a3 = np.where(on, a3 + w.w1[k] * jd * jd, a3)
                a6 = np.where(on, fma(wr2, w.Jg2[k], fma(wr1, w.Jg1[k], a6)), a6)
                a7 = np.where(on, a7 + wr1 * jd, a7)
                a2 = np.where(on, a2 + w.w2[k] * w.Jg2[k] * jd, a2)
                a5 = np.where(on, a5 + w.w2[k] * jd * jd, a5)
                a8 = np.where(on, a8 + wr2 * jd, a8)
        eps = F(1e-6)
        H00 = np.sqrt(a0 + eps)
        z0 = a6 / H00
        if use_desc:
            H01 = a1 / H00
            H11 = np.sqrt((a3 + eps) - H01 * H01)
            H02 = a2 / H00
            H12 = (F(0) - H02 * H01) / H11
            H22 = np.sqrt(((a5 + eps) - H02 * H02) - H12 * H12)
            z1 = (a7 - H01 * z0) / H11
            z2 = ((a8 - H02 * z0) - H12 * z1) / H22
        else:
            H01 = H02 = H12 = np.zeros(n, F)
            H11 = H22 = np.ones(n, F)
            z1 = z2 = np.zeros(n, F)
        L = np.stack([H00, H01, H02, H11, H12, H22], axis=1).astype(F)
        sound = np.isfinite(L).all(axis=1) & (H00 > 0) & (H11 > 0) & (H22 > 0)
    return L, np.stack([z0, z1, z2], axis=1).astype(F), ~sound


def pair_E32(w, k, use_depth, use_desc):
    """E of keyframe k's pairs: (n, 6, m) binary32, zeros where there is no pair."""
    m = 3 if use_desc else 1
    E = np.zeros((w.n, 6, m), F)
    with np.errstate(all="ignore"):
        for i in range(6):
            e0 = (w.w[k] * w.Jgeom[k]) * w.Jpose[k, :, i] if use_depth else np.zeros(w.n, F)
            e0 = np.where(w.associated[k], e0, F(0))
            if use_desc:
                on = w.color[k]
                e0 = np.where(on, fma(w.w2[k] * w.Jg2[k], w.Jp2[k, :, i], fma(w.w1[k] * w.Jg1[k], w.Jp1[k, :, i], e0)), e0)
                E[:, i, 1] = np.where(on, -(w.w1[k] * w.Jp1[k, :, i]), F(0))
                E[:, i, 2] = np.where(on, -(w.w2[k] * w.Jp2[k, :, i]), F(0))
            E[:, i, 0] = e0
    return E


def pair_Y32(E, L, keep):
    """Y = E L^-T row by row; zeros where `keep` is false."""
    m = E.shape[2]
    Y = np.zeros(E.shape, F)
    H00, H01, H02, H11, H12, H22 = (L[:, c][:, None] for c in range(6))
    with np.errstate(all="ignore"):
        y0 = E[:, :, 0] / H00
        Y[:, :, 0] = y0
        if m == 3:
            y1 = (E[:, :, 1] - H01 * y0) / H11
            Y[:, :, 1] = y1
            Y[:, :, 2] = ((E[:, :, 2] - H02 * y0) - H12 * y1) / H22
    Y[~keep] = 0
    return Y


def _chain(x, y):
    """mad(x2, y2, mad(x1, y1, x0 y0)) over the last axis (m = 3), x0 y0 for m = 1."""
    with np.errstate(all="ignore"):
        p = x[..., 0] * y[..., 0]
        if x.shape[-1] == 3:
            p = fma(x[..., 2], y[..., 2], fma(x[..., 1], y[..., 1], p))
    return p.astype(F)


def _tiles(a):
    """(n, ...) -> (T, 64, ...), padded with zeros."""
    n = a.shape[0]
    t = (n + 63) // 64
    out = np.zeros((t * 64,) + a.shape[1:], a.dtype)
    out[:n] = a
    return out.reshape((t, 64) + a.shape[1:])


def pose_equations32(w, use_depth, use_desc):
    """The pose sums of every keyframe with the definition of orc_accumulate_pose_coeffs_fixed: Limbs of shape (K, 27)."""
    sums = Limbs((w.K, 27))
    for k in range(w.K):
        acc = np.zeros((w.n, 27), F)
        residuals = []
        if use_depth:
            residuals.append((w.associated[k], w.raw[k], w.w[k], w.Jpose[k]))
        if use_desc:
            residuals += [(w.color[k], w.raw1[k], w.w1[k], w.Jp1[k]), (w.color[k], w.raw2[k], w.w2[k], w.Jp2[k])]
        with np.errstate(all="ignore"):
            for on, raw, wt, J in residuals:
                for q, (i, j) in enumerate(UPPER):
                    acc[:, q] = np.where(on, fma(wt * J[:, i], J[:, j], acc[:, q]), acc[:, q])
                for i in range(6):
                    acc[:, 21 + i] = np.where(on, fma(wt * raw, J[:, i], acc[:, 21 + i]), acc[:, 21 + i])
        any_pair = _tiles(w.associated[k]).any(axis=1)
        sums.add(k, tile_tree_sum(np.moveaxis(_tiles(acc), 1, -1)), any_pair)
    return sums


class System:
    """What a call returns: S, g, A, b (binary64), stats, and the integer tables they are resolved from."""


def model32(w, use_depth=True, use_desc=True, marginalise=True, capacity=DEFAULT_LIST_CAPACITY, tables=None):
    """The reduced camera system of the words; tables: the (pose, blocks, v) Limbs and counts of other shards to add before resolving."""
    K, n = w.K, w.n
    pose = pose_equations32(w, use_depth, use_desc)
    blocks, v = Limbs((K, K, 6, 6)), Limbs((K, 6))
    counts = dict(list_entries=0, pairs_visited=0, atomics_issued=0, degenerate_surfels=0, overflow_tiles=0)
    if marginalise and n:
        L, z, degenerate = factor32(w, use_depth, use_desc)
        counts["degenerate_surfels"] = int(degenerate.sum())
        masks = {k: _tiles(w.associated[k]) for k in range(K) if w.associated[k].any()}
        Y = {k: _tiles(pair_Y32(pair_E32(w, k, use_depth, use_desc), L, w.associated[k] & ~degenerate)) for k in masks}
        zt = _tiles(z[:, :Y[next(iter(Y))].shape[-1]]) if Y else None
        per_tile = tile_cull.per_tile(w.associated).sum(axis=1)
        counts["list_entries"] = int(per_tile.sum())
        counts["overflow_tiles"] = int((per_tile > capacity).sum())
        upper = np.triu(np.ones((6, 6), bool))
        for b in masks:
            listed = masks[b].any(axis=1)
            v.add(b, tile_tree_sum(np.moveaxis(_chain(Y[b], zt[:, :, None, :]), 1, -1)), listed)
            for a in masks:
                if a > b:
                    continue
                meet = (masks[a] & masks[b]).any(axis=1)
                if not meet.any():
                    continue
                P = _chain(Y[b][:, :, :, None, :], Y[a][:, :, None, :, :])          # (T, 64, 6, 6): row i of b, column j of a
                totals = tile_tree_sum(np.moveaxis(P, 1, -1))
                if a == b:
                    totals = np.where(upper, totals, F(0))
                blocks.add((b, a), totals, meet)
                counts["pairs_visited"] += int(meet.sum())
                counts["atomics_issued"] += int(meet.sum()) * (ATOMICS_PER_DIAGONAL_PAIR if a == b else ATOMICS_PER_PAIR)
        counts["atomics_issued"] += ATOMICS_PER_ENTRY * counts["list_entries"]
    for other in tables or []:
        for mine, theirs in zip((pose, blocks, v), other.tables):
            mine.lo += theirs.lo
            mine.hi += theirs.hi
            mine.invalid = mine.invalid or theirs.invalid
        for name in counts:
            counts[name] += other.stats[name]
    return resolve(pose, blocks, v, counts)


def resolve(pose, blocks, v, counts):
    K = pose.lo.shape[0]
    out = System()
    out.tables = (pose, blocks, v)
    values = pose.values()
    A = np.zeros((K, 6, 6))
    for q, (i, j) in enumerate(UPPER):
        A[:, i, j] = A[:, j, i] = values[:, q]
    out.A, out.b = A, values[:, 21:27].copy()
    M = blocks.values()
    for k in range(K):                                   # the diagonal blocks are summed over i <= j
        M[k, k] = np.triu(M[k, k]) + np.triu(M[k, k], 1).T
        for l in range(k + 1, K):
            M[k, l] = M[l, k].T
    S = np.zeros((6 * K, 6 * K))
    for k in range(K):
        for l in range(K):
            S[6 * k:6 * k + 6, 6 * l:6 * l + 6] = (A[k] if k == l else 0.0) - M[k, l]
    out.S, out.g = S, (out.b - v.values()).reshape(-1)
    out.stats = dict(counts, invalid=int(pose.invalid or blocks.invalid or v.invalid))
    return out


def sum_over_shards(w, bounds, **kw):
    """The system every rank of a surfel partition [bounds[r], bounds[r + 1]) ends with: the shards' integer tables added."""
    shards = [model32(w.take(slice(lo, hi)), **kw) for lo, hi in zip(bounds[:-1], bounds[1:])]
    return model32(w.take(slice(0, 0)), tables=shards, **kw), shards


# ---- REFERENCE64 -------------------------------------------------------------------------------------------------------------------
def reference64(w, use_depth=True, use_desc=True, fixed=None):
    """(S, g, magnitude) in binary64 from the same words; `fixed`: surfels that are not eliminated (MODEL32's degenerate ones).
    magnitude[r, c] = the sum of the magnitudes of the terms of S[r, c]."""
    K, n, m = w.K, w.n, 3 if use_desc else 1
    d = lambda a: np.asarray(a, np.float64)          # noqa: E731
    A, Aabs, b = np.zeros((K, 6, 6)), np.zeros((K, 6, 6)), np.zeros((K, 6))
    E = np.zeros((K, n, 6, m))
    C, c = np.zeros((n, m, m)), np.zeros((n, m))
    for k in range(K):
        residuals = []
        if use_depth:
            js = np.zeros((n, m))
            js[:, 0] = d(w.Jgeom[k])
            residuals.append((w.associated[k], d(w.raw[k]), d(w.w[k]), d(w.Jpose[k]), js))
        if use_desc:
            for which, (raw, wt, Jp, Jg) in enumerate(((w.raw1, w.w1, w.Jp1, w.Jg1), (w.raw2, w.w2, w.Jp2, w.Jg2))):
                js = np.zeros((n, 3))
                js[:, 0], js[:, 1 + which] = d(Jg[k]), -1.0
                residuals.append((w.color[k], d(raw[k]), d(wt[k]), d(Jp[k]), js))
        for on, raw, wt, Jp, js in residuals:
            wt, raw = np.where(on, wt, 0.0), np.where(on, raw, 0.0)
            terms = wt[:, None, None] * Jp[:, :, None] * Jp[:, None, :]
            A[k] += terms.sum(axis=0)
            Aabs[k] += np.abs(terms).sum(axis=0)
            b[k] += ((wt * raw)[:, None] * Jp).sum(axis=0)
            E[k] += wt[:, None, None] * Jp[:, :, None] * js[:, None, :]
            C += wt[:, None, None] * js[:, :, None] * js[:, None, :]
            c += (wt * raw)[:, None] * js
    C += 1e-6 * np.eye(m)
    keep = np.ones(n, bool) if fixed is None else ~np.asarray(fixed, bool)
    Lc = np.linalg.cholesky(C[keep])
    Li = np.linalg.inv(Lc)                               # (n', m, m)
    Y = np.einsum("ksim,snm->ksin", E[:, keep], Li)      # Y = E L^-T
    zz = np.einsum("snm,sm->sn", Li, c[keep])
    M = np.einsum("ksic,lsjc->kilj", Y, Y)
    Mabs = np.einsum("ksic,lsjc->kilj", np.abs(Y), np.abs(Y))
    S, mag = -M.reshape(6 * K, 6 * K), Mabs.reshape(6 * K, 6 * K)
    g = (b - np.einsum("ksic,sc->ki", Y, zz)).reshape(-1)
    for k in range(K):
        S[6 * k:6 * k + 6, 6 * k:6 * k + 6] += A[k]
        mag[6 * k:6 * k + 6, 6 * k:6 * k + 6] += Aabs[k]
    return S, g, mag


def block_ratio(S32, S64, magnitude):
    """Per 6 x 6 block the largest |S32 - S64| over 2^-24 times the block's largest term sum: (K, K)."""
    K = S32.shape[0] // 6
    diff = np.abs(S32 - S64).reshape(K, 6, K, 6).max(axis=(1, 3))
    scale = magnitude.reshape(K, 6, K, 6).max(axis=(1, 3))
    return np.where(scale > 0, diff / (2.0 ** -24 * np.where(scale > 0, scale, 1.0)), np.where(diff > 0, np.inf, 0.0))


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """(TwoCameraScene, oracle, Words) of a scene of tests/two_cameras.py in its perturbed state (built once per process)."""
    tc = two_cameras.build_scene(name)
    ba = two_cameras.build_oracle(tc)
    return tc, ba, oracle_words(ba)


@functools.lru_cache(maxsize=None)
def world(name):
    """(World, oracle, Words) of a world of tests/tile_cull.py."""
    w = tile_cull.world(name)
    ba = tile_cull.build_oracle(w)
    return w, ba, oracle_words(ba)
