"""The model of the observation lists (tests/surfel_observations.py) on hand-made association matrices, and the census of the scenes
and worlds the GPU tests run on (tests/test_gpu_surfel_observations.py): the figures below were computed from the oracle and are
asserted, so that a changed fixture is noticed and the GPU tests keep meaning something -- lists of every length, lists that skip a
keyframe, tiles with more pairs than the small staging windows and tiles with none, ragged last tiles."""
import numpy as np
import pytest

from tests import observed_covisibility as oc
from tests import surfel_costs as sc
from tests import surfel_observations as so


def _round_trip(A):
    A = np.asarray(A, bool)
    first, ks = so.csr(A)
    assert first.dtype == np.uint32 and ks.dtype == np.uint16 and len(first) == A.shape[1] + 1 and first[0] == 0 and first[-1] == len(ks) == A.sum()
    assert np.array_equal(so.dense(first, ks, A.shape[0]), A)
    return first.tolist(), ks.tolist()


def test_an_empty_cloud_and_no_keyframes():
    assert _round_trip(np.zeros((3, 0), bool)) == ([0], [])
    assert _round_trip(np.zeros((0, 5), bool)) == ([0] * 6, [])
    assert so.per_tile(np.zeros(1, np.uint32)).tolist() == [] and so.per_tile(np.zeros(6, np.uint32)).tolist() == [0]


def test_one_pair():
    A = np.zeros((4, 70), bool)
    A[2, 65] = True
    first, ks = _round_trip(A)
    assert first == [0] * 66 + [1] * 5 and ks == [2]
    assert so.per_tile(np.array(first)).tolist() == [0, 1] and so.gaps(first, ks) == 0


def test_a_surfel_seen_by_all_keyframes():
    A = np.zeros((5, 3), bool)
    A[:, 1] = True
    A[3, 2] = True
    first, ks = _round_trip(A)
    assert first == [0, 0, 5, 6] and ks == [0, 1, 2, 3, 4, 3]
    assert so.lengths(first).tolist() == [0, 5, 1]


def test_a_nan_surfel_between_live_ones_and_lists_with_gaps():
    A = np.array([[1, 0, 1, 1], [0, 0, 1, 0], [1, 0, 1, 1]], bool)        # surfel 1 is dead: an empty list, its neighbours' offsets right
    first, ks = _round_trip(A)
    assert first == [0, 2, 2, 5, 7] and ks == [0, 2, 0, 1, 2, 0, 2]
    assert so.gaps(first, ks) == 2                                          # surfels 0 and 3 skip keyframe 1
    t = dict(pairs=7, surfel_first=np.array(first, np.uint32), keyframes=np.array(ks, np.uint16), depth_raw=np.arange(7, dtype=np.uint32),
             descriptor_raw=np.arange(14, dtype=np.uint32).reshape(7, 2))
    part = so.take(t, 1, 3)
    assert part["surfel_first"].tolist() == [0, 0, 3] and part["keyframes"].tolist() == [0, 1, 2] and part["depth_raw"].tolist() == [2, 3, 4]
    moved = so.permuted(t, np.array([3, 2, 1, 0]))
    assert moved["surfel_first"].tolist() == [0, 2, 5, 5, 7] and moved["keyframes"].tolist() == [0, 2, 0, 1, 2, 0, 2]
    assert moved["depth_raw"].tolist() == [5, 6, 2, 3, 4, 0, 1] and moved["descriptor_raw"][0].tolist() == [10, 11]
    with pytest.raises(AssertionError):
        so.dense([0, 2], [1, 1], 3)                                         # a keyframe twice
    with pytest.raises(AssertionError):
        so.dense([0, 2], [2, 1], 3)                                         # not ascending


def _reductions(ba, A, t):
    """The table reduces to what the other units report."""
    first, ks = t["surfel_first"], t["keyframes"]
    K = A.shape[0]
    back = so.dense(first, ks, K)
    assert np.array_equal(back, A)
    C = oc.matrix(A)
    assert np.array_equal(np.bincount(ks, minlength=K), np.diag(C))                       # column sums: the co-visibility model's diagonal
    assert np.array_equal(oc.matrix(back), C)                                             # A A^T rebuilt from the compressed rows
    counts = sum(sc.pair_terms(w)[0].astype(np.int64) for w in sc.oracle_pair_words(ba))  # the per-surfel depth counts
    assert np.array_equal(so.lengths(first), counts)


@pytest.mark.parametrize("name,surfels,last,pairs,histogram,gapped,tile_range", [
    ("tiny", 1142, 54, 3489, [0, 210, 186, 77, 669], 151, (76, 256)),
    ("crop_small", 31057, 17, 96191, [217, 5442, 4449, 1945, 19004], 3677, None)])
def test_census_of_the_scenes(name, surfels, last, pairs, histogram, gapped, tile_range):
    tc, ba, A, t = so.scene(name)
    first, ks = t["surfel_first"], t["keyframes"]
    tiles = so.per_tile(first)
    print(name, "pairs", t["pairs"], "lengths", np.bincount(so.lengths(first)).tolist(), "gaps", so.gaps(first, ks), "tiles", len(tiles), tiles.min(),
          tiles.max())
    assert A.shape == (4, surfels) and (surfels - 1) % 64 + 1 == last and len(tiles) == -(-surfels // 64)
    assert t["pairs"] == pairs
    assert np.bincount(so.lengths(first), minlength=5).tolist() == histogram
    assert so.gaps(first, ks) == gapped
    if tile_range:
        assert len(tiles) == 18 and (int(tiles.min()), int(tiles.max())) == tile_range
    _reductions(ba, A, t)
    # the payload: one depth word per pair, finite; descriptor words NaN exactly where the colour pixel is not valid
    depth = t["depth_raw"].view(np.float32)
    assert np.isfinite(depth).all()
    nan = t["descriptor_raw"] == so.NAN_WORD
    assert (nan[:, 0] == nan[:, 1]).all() and np.isfinite(t["descriptor_raw"].view(np.float32)[~nan[:, 0]]).all()


def test_census_of_the_world_centred():
    w, ba, A, t = so.world("centred")
    first, ks = t["surfel_first"], t["keyframes"]
    tiles = so.per_tile(first)
    print("centred pairs", t["pairs"], "lengths", np.bincount(so.lengths(first)).tolist(), "largest tile", tiles.max(), "empty tiles", int((tiles == 0).sum()))
    assert t["pairs"] == 13411
    assert set(range(8)) <= set(so.lengths(first).tolist())
    assert (tiles == 0).any() and tiles.max() == 448
    _reductions(ba, A, t)
