"""The model of the observed co-visibility (tests/observed_covisibility.py) on hand-made association matrices, and the census of the
scenes and worlds the GPU tests run on (tests/test_gpu_observed_covisibility.py): the counts below were computed from the oracle and are
asserted, so that a changed fixture is noticed and the GPU tests keep meaning something -- shared surfels between every pair, tiles with
seven entries and with none, a keyframe that shares nothing."""
import numpy as np
import pytest

from tests import observed_covisibility as oc
from tests import tile_cull


def _A(rows):
    return np.array(rows, bool)


def test_an_empty_cloud_and_no_keyframes():
    assert oc.matrix(np.zeros((3, 0), bool)).tolist() == [[0] * 3] * 3
    assert oc.entries(np.zeros((3, 0), bool)) == 0 and oc.atomic_ceiling(np.zeros((3, 0), bool)) == 0
    assert oc.matrix(np.zeros((0, 5), bool)).shape == (0, 0)


def test_one_surfel_seen_by_all():
    A = np.zeros((5, 70), bool)
    A[:, 3] = True
    assert np.array_equal(oc.matrix(A), np.ones((5, 5), np.int64))
    assert oc.tile_counts(A).tolist() == [5, 0] and oc.entries(A) == 5 and oc.atomic_ceiling(A) == 30


def test_disjoint_keyframes():
    A = np.zeros((3, 30), bool)
    A[0, :10], A[1, 10:17], A[2, 17:] = True, True, True
    assert np.array_equal(oc.matrix(A), np.diag([10, 7, 13]))
    assert oc.entries(A) == 3


def test_a_tile_boundary_at_64():
    A = np.zeros((2, 130), bool)
    A[0, 60:70] = True                      # four surfels of tile 0, six of tile 1
    A[1, 63:65] = True                      # one on each side
    A[1, 129] = True                        # and the ragged last tile
    assert oc.matrix(A).tolist() == [[10, 2], [2, 3]]
    assert oc.tile_counts(A).tolist() == [2, 2, 1] and oc.entries(A) == 5
    assert np.array_equal(oc.sum_over_shards(A, [0, 64, 128, 130]), oc.matrix(A))
    assert np.array_equal(oc.sum_over_shards(A, [0, 61, 130]), oc.matrix(A))       # shards need not end on tiles


def _identities(A, C):
    d = np.diag(C)
    assert np.array_equal(C, C.T)
    assert np.array_equal(d, np.asarray(A).sum(axis=1))                             # the oracle's pair count per keyframe
    assert (C <= np.minimum(d[:, None], d[None, :])).all()


@pytest.mark.parametrize("name,diagonal", [("tiny", [913, 930, 705, 941]), ("crop_small", [24633, 25792, 19943, 25823])])
def test_census_of_the_scenes(name, diagonal):
    tc, ba, A = oc.scene(name)
    C = oc.matrix(A)
    print(name, C.tolist(), "entries", oc.entries(A), "tiles", len(oc.tile_counts(A)))
    _identities(A, C)
    assert np.diag(C).tolist() == diagonal
    off = C[~np.eye(4, dtype=bool)]
    assert off.min() > 0
    if name == "tiny":
        assert (off.min(), off.max()) == (673, 790)
        assert oc.tile_counts(A).max() == 4              # four list entries at most: the default list never overflows here


def test_census_of_the_world_centred():
    A = oc.world_matrix("centred")
    C = oc.matrix(A)
    counts = oc.tile_counts(A)
    print(C.tolist(), "entries", oc.entries(A), "tiles", len(counts), np.bincount(counts).tolist())
    _identities(A, C)
    assert A.shape == (8, 23589) and len(counts) == 369  # 368 tiles and a ragged one of 37
    assert oc.entries(A) == int(tile_cull.per_tile(A).sum()) > 1000
    assert not C[7].any() and not C[:, 7].any()          # the keyframe that looks away shares nothing
    assert C[6, 6] == 727 and C[0, 2] == 1700
    assert int((counts == 7).sum()) == 64 and int((counts == 0).sum()) == 18
    seen_by = A.sum(axis=0)
    assert set(range(1, 8)) <= set(seen_by.tolist())     # surfels seen by 1 .. 7 keyframes


def test_census_of_the_world_narrow():
    A = oc.world_matrix("narrow")
    C = oc.matrix(A)
    print(C.tolist())
    _identities(A, C)
    assert not C[7].any()
    assert C[6, :7].tolist() == [577] * 7
