"""The model of the reduced camera system (tests/reduced_camera_system.py) on the CPU: its restatements of the oracle's tile tree,
fixed point and pose sums against the oracle itself, hand-made cases, MODEL32 against the binary64 elimination, and the census that
makes tests/test_gpu_reduced_camera_system.py meaningful.

MODEL32 against REFERENCE64, per 6 x 6 block: |S32 - S64| <= C * 2^-24 * (the block's largest sum of term magnitudes).  The largest
ratio measured here, over `tiny` and `crop_small` and the selections (1, 0), (1, 1), (0, 1), is MEASURED_RATIO = 1.84 (crop_small,
descriptors only: 1.836; tiny, descriptors only: 1.433; the four cases with the depth term lie between 0.058 and 0.388);
C = 4 x that = BOUND_C = 7.36."""
import numpy as np
import pytest

from oracle import binding as ob
from tests import observed_covisibility as oc
from tests import reduced_camera_system as rcs

F = np.float32
SELECTIONS = [(True, False), (True, True), (False, True)]
MEASURED_RATIO = 1.84
BOUND_C = 4 * MEASURED_RATIO


def test_the_tree_and_the_fixed_point_are_the_oracles():
    L = ob.lib()
    import ctypes as C
    L.orc_tile_tree_sum.restype = C.c_float
    rng = np.random.Generator(np.random.PCG64(11))
    x = (rng.standard_normal((200, 64)) * 10.0 ** rng.integers(-6, 7, (200, 64))).astype(F)
    mine = rcs.tile_tree_sum(x)
    for row, got in zip(x, mine):
        assert L.orc_tile_tree_sum((C.c_float * 64)(*row.tolist())) == got
    values = np.concatenate([x.reshape(-1)[:3000], np.array([0, -0.0, 1e-12, -3e-10, 2.0 ** -33, 3 * 2.0 ** -33, 2.0 ** 51, -2.0 ** 52, np.inf, np.nan, 1e-45,
                                                             4.6e15, -1.5 * 2.0 ** -32, 2.5 * 2.0 ** -32, 2.0 ** 31, 2.0 ** 32 + 512], F)])
    lo, hi, valid = rcs.pose_limbs(values)
    out = (C.c_longlong * 2)()
    for v, l, h, ok in zip(values, lo, hi, valid):
        assert bool(L.orc_pose_limbs(C.c_float(float(v)), out)) == bool(ok), v
        if ok:
            assert (out[0], out[1]) == (int(l), int(h)), v
    some = np.array([[5, -3], [-7, 2], [2 ** 40 + 17, -(2 ** 50)], [-(2 ** 33) - 1, 9]], np.int64)
    assert np.array_equal(rcs.limbs_value(some[:, 0], some[:, 1]), ob.OracleBA.pose_limbs_value(some))


@pytest.mark.parametrize("use_depth,use_desc", SELECTIONS)
def test_the_models_pose_equations_are_the_oracles(use_depth, use_desc):
    tc, ba, words = rcs.scene("tiny")
    pose = rcs.pose_equations32(words, use_depth, use_desc)
    saved = ba.use_depth, ba.use_desc
    try:
        ba.use_depth, ba.use_desc = int(use_depth), int(use_desc)
        for k in range(words.K):
            fixed = ba.accumulate_pose_coeffs_fixed(k)
            assert np.array_equal(fixed[:, 0], pose.lo[k]) and np.array_equal(fixed[:, 1], pose.hi[k]), k
        assert not ba.pose_sum_invalid() and not pose.invalid
    finally:
        ba.use_depth, ba.use_desc = saved


def _hand(K, n):
    w = rcs.Words(K, n)
    return w


def test_one_surfel_seen_by_two_keyframes_worked_by_hand():
    w = _hand(2, 1)
    p = np.array([[1, 2, 0, -1, 3, 0.5], [2, -1, 1, 0, 0.25, 4]], F)
    r = np.array([0.5, -0.25], F)
    w.associated[:] = True
    w.w[:] = 1
    w.Jgeom[:] = -2
    w.raw[:, 0] = r
    w.Jpose[:, 0] = p
    out = rcs.model32(w, True, False)
    c = float(F(8) + F(1e-6))                           # C as binary32 holds it
    for k in range(2):
        assert np.array_equal(out.A[k], np.outer(p[k], p[k])) and np.array_equal(out.b[k], r[k] * p[k])
        for l in range(2):
            expected = (np.outer(p[k], p[k]) if k == l else 0.0) - 4.0 * np.outer(p[k], p[l]) / c
            got = out.S[6 * k:6 * k + 6, 6 * l:6 * l + 6]
            assert np.allclose(got, expected, rtol=0, atol=4e-6 * np.abs(np.outer(p[k], p[l])).max()), (k, l)
        v = p[k] * 4.0 * (r[0] + r[1]) / c
        assert np.allclose(out.g[6 * k:6 * k + 6], out.b[k] - v, rtol=0, atol=1e-6)
    assert np.array_equal(out.S, out.S.T)
    # the surfel carries all the information along p0 + p1 that the two keyframes share: S is singular there up to the 1e-6
    assert out.stats == dict(list_entries=2, pairs_visited=3, atomics_issued=2 * 12 + 72 + 2 * 42, degenerate_surfels=0, overflow_tiles=0, invalid=0)
    plain = rcs.model32(w, True, False, marginalise=False)
    assert np.array_equal(plain.S[:6, :6], out.A[0]) and not plain.S[:6, 6:].any() and np.array_equal(plain.g, out.b.reshape(-1))
    assert plain.stats["list_entries"] == 0


def test_a_surfel_seen_by_one_keyframe_gives_a_diagonal_term_only():
    w = _hand(2, 1)
    w.associated[0] = w.color[0] = True
    w.w[0], w.Jgeom[0], w.raw[0] = 1, -3, 0.5
    w.w1[0], w.w2[0], w.Jg1[0], w.Jg2[0], w.raw1[0], w.raw2[0] = 0.01, 0.01, 2, -1, 3, -2
    w.Jpose[0, 0], w.Jp1[0, 0], w.Jp2[0, 0] = [1, 0, 2, 0, 1, 0], [0, 1, 0, 3, 0, 1], [2, 2, 0, 0, 1, 1]
    for use_depth, use_desc in SELECTIONS:
        out = rcs.model32(w, use_depth, use_desc)
        assert not out.S[:6, 6:].any() and not out.S[6:, :].any() and not out.g[6:].any()
        M = out.A[0] - out.S[:6, :6]
        assert (np.diag(M) > 0).sum() >= 3 and np.array_equal(M, M.T)
        assert np.linalg.eigvalsh(out.S[:6, :6]).min() > -1e-6          # eliminating a surfel cannot add information
        assert out.stats["pairs_visited"] == 1 and out.stats["atomics_issued"] == 12 + 42
        S64, g64, mag = rcs.reference64(w, use_depth, use_desc)
        assert rcs.block_ratio(out.S, S64, mag).max() < 16


def test_a_degenerate_surfel_is_counted_and_held_fixed():
    w = _hand(2, 2)
    w.associated[:] = w.color[:] = True
    w.w[:], w.Jgeom[:], w.raw[:] = 1, -2, 0.5
    w.w1[:], w.w2[:], w.Jg1[:], w.Jg2[:], w.raw1[:], w.raw2[:] = 0.01, 0.01, 2, -1, 3, -2
    w.Jpose[:], w.Jp1[:], w.Jp2[:] = [1, 0, 2, 0, 1, 0], [0, 1, 0, 3, 0, 1], [2, 2, 0, 0, 1, 1]
    sound = rcs.model32(w.take(slice(0, 1)), True, True)
    w.Jg1[:, 1] = 1e25                                       # a0 overflows: the factor of surfel 1 is not finite; A does not hold Jg1
    out = rcs.model32(w, True, True)
    assert out.stats["degenerate_surfels"] == 1 and out.stats["invalid"] == 0 and out.stats["pairs_visited"] == 3
    assert np.array_equal(out.A, 2 * sound.A) and np.array_equal(out.b, 2 * sound.b)          # it contributes to A and b
    assert np.array_equal(out.A[0] - out.S[:6, :6], sound.A[0] - sound.S[:6, :6])             # ... and is not eliminated
    assert np.array_equal(out.S[6:, :6], sound.S[6:, :6])
    assert rcs.model32(w, True, False).stats["degenerate_surfels"] == 0                       # (depth only does not read Jg1)


@pytest.mark.parametrize("use_depth,use_desc", SELECTIONS)
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_model32_against_the_binary64_elimination(name, use_depth, use_desc):
    tc, ba, words = rcs.scene(name)
    out = rcs.model32(words, use_depth, use_desc)
    _, _, degenerate = rcs.factor32(words, use_depth, use_desc)
    S64, g64, mag = rcs.reference64(words, use_depth, use_desc, fixed=degenerate)
    ratio = rcs.block_ratio(out.S, S64, mag)
    gscale = np.abs(g64).max()
    print(name, (use_depth, use_desc), "largest block ratio", float(ratio.max()), "g: largest difference over the largest word",
          float(np.abs(out.g - g64).max() / gscale), "degenerate", int(degenerate.sum()))
    assert out.stats["invalid"] == 0
    assert ratio.max() <= BOUND_C, ratio
    assert np.array_equal(out.S, out.S.T)
    # the smallest eigenvalue of the binary64 S: non-negative up to the bound
    smallest = np.linalg.eigvalsh(S64).min()
    assert smallest >= -BOUND_C * 2.0 ** -24 * mag.max(), smallest
    for k in range(words.K):
        assert (np.diag(out.A[k] - out.S[6 * k:6 * k + 6, 6 * k:6 * k + 6]) >= 0).all(), k


def test_census_every_block_of_tiny_is_non_zero_and_zero_blocks_follow_the_covisibility():
    tc, ba, words = rcs.scene("tiny")
    out = rcs.model32(words, True, True)
    K = words.K
    blocks = np.abs(out.S).reshape(K, 6, K, 6).max(axis=(1, 3))
    assert K == 4 and (blocks > 0).all()
    assert np.array_equal(words.associated, oc.scene("tiny")[2])
    w, ba, words = rcs.world("centred")
    out = rcs.model32(words, True, True)
    K = words.K
    blocks = np.abs(out.S).reshape(K, 6, K, 6).max(axis=(1, 3))
    counts = oc.matrix(words.associated)
    assert np.array_equal(blocks == 0, counts == 0)
    assert not blocks[7].any() and not blocks[:, 7].any() and blocks[6, 6] > 0          # row 7: the keyframe that looks away
    assert out.stats["list_entries"] == oc.entries(words.associated)


def test_shards_sum_to_the_whole():
    tc, ba, words = rcs.scene("tiny")
    whole = rcs.model32(words, True, True)
    n = words.n
    bounds = [0, 64 * 5, 64 * 11, n]
    summed, shards = rcs.sum_over_shards(words, bounds, use_depth=True, use_desc=True)
    assert np.array_equal(summed.S, whole.S) and np.array_equal(summed.g, whole.g) and summed.stats == whole.stats
    assert not np.array_equal(shards[0].S, whole.S)
