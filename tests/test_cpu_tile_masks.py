"""The model of the tile mask table (tests/tile_masks.py) on hand-made matrices and against the models of the three reductions
(tests/observed_covisibility.py, tests/keyframe_redundancy.py, tests/surfel_observations.py) on the scenes the GPU tests run, and the
census that makes those GPU tests mean something: how many entries every rank lists, how many tiles the merge has to reorder, how
many lists interleave the ranks -- re-counted here from the oracle's flags and asserted."""
import numpy as np
import pytest

from tests import keyframe_redundancy as kr
from tests import observed_covisibility as oc
from tests import surfel_observations as so
from tests import tile_cull
from tests import tile_masks as tm


def _matrix(name):
    return oc.scene(name)[2] if name in ("tiny", "crop_small") else oc.world_matrix(name)


def _check_all(A, bins=(1, 16, 64)):
    A = np.asarray(A, bool)
    K, n = A.shape
    tab = tm.table(A)
    assert np.array_equal(tm.dense(tab, K, n), A)
    assert len(tab[1]) == oc.entries(A)
    assert np.array_equal(tm.covisibility(tab, K), oc.matrix(A))
    for b in bins:
        assert np.array_equal(tm.histogram(tab, K, n, b), kr.table(A, b))
    first, ks = tm.observations(tab, n)
    want_first, want_ks = so.csr(A)
    assert np.array_equal(first, want_first) and np.array_equal(ks, want_ks)
    for world in (1, 2, 4, 8):
        parts = [tm.partial(A, r, world) for r in range(world)]
        assert sum(len(p[1]) for p in parts) == len(tab[1])
        rm = tm.rank_major(A, world)
        assert np.array_equal(rm[0], tab[0])
        for t in range(len(tab[0]) - 1):          # the canonical layout is the rank-major one, sorted by keyframe inside each tile
            lo, hi = int(tab[0][t]), int(tab[0][t + 1])
            order = np.argsort(rm[1][lo:hi], kind="stable")
            assert np.array_equal(rm[1][lo:hi][order], tab[1][lo:hi]) and np.array_equal(rm[2][lo:hi][order], tab[2][lo:hi])
    return tab


def test_hand_made_matrices():
    empty = tm.table(np.zeros((3, 100), bool))
    assert empty[0].tolist() == [0, 0, 0] and len(empty[1]) == 0 and len(empty[2]) == 0
    assert tm.table(np.zeros((0, 0), bool))[0].tolist() == [0]
    one = np.zeros((3, 130), bool)
    one[1, 65] = True
    first, ks, ms = tm.table(one)
    assert first.tolist() == [0, 0, 1, 1] and ks.tolist() == [1] and ms.tolist() == [2]
    _check_all(one)
    for n in (64, 65):
        A = np.ones((2, n), bool)
        first, ks, ms = _check_all(A)
        assert first.tolist() == ([0, 2] if n == 64 else [0, 2, 4]) and int(ms[0]) == 2 ** 64 - 1 and (n == 64 or int(ms[-1]) == 1)
    rng = np.random.Generator(np.random.PCG64(3))
    _check_all(rng.random((1, 200)) < 0.5)                   # K = 1
    A = rng.random((5, 300)) < 0.3
    A[2] = False                                             # a keyframe nobody owns entries of
    tab = _check_all(A)
    assert 2 not in tab[1].tolist() and tm.listed(A, 4)[2] == 0
    assert tm.partial(A, 1, 4)[1].tolist() == [1] * len(tm.partial(A, 1, 4)[1])


def test_the_exchange_counts():
    assert tm.table_exchanges(0) == 1 and tm.table_exchanges(1) == 2 and tm.table_exchanges(72, 7) == 1 + 11 and tm.table_exchanges(72, 72) == 2
    assert tm.reduction_exchanges(72) == 3 and tm.reduction_exchanges(0) == 2 and tm.reduction_exchanges(72, 1) == 74
    assert tm.observation_exchanges(72, 3489, 3489) == 2 + 1 + 1
    assert tm.observation_exchanges(72, 3489, 3489, payload_slice=1000) == 2 + 4 + 7
    assert tm.observation_exchanges(72, 3489, 3488) == 2 and tm.observation_exchanges(72, 3489, 3489, keyframes=False) == 2
    assert tm.observation_exchanges(72, 3489, 3489, descriptor=False) == 3 and tm.observation_exchanges(0, 0, 0) == 1


@pytest.mark.parametrize("name", ["tiny", "crop_small", "centred"])
def test_the_reductions_of_the_table_are_the_models(name):
    _check_all(_matrix(name), bins=(1, 16))


def test_census_tiny():
    A = _matrix("tiny")
    tab = tm.table(A)
    assert A.shape[0] == 4 and len(tab[0]) - 1 == 18 and len(tab[1]) == 72 and int(A.sum()) == 3489
    assert tm.listed(A, 2) == [36, 36] and tm.tiles_to_reorder(A, 2) == 18 and tm.interleaving_lists(A, 2) == 704
    assert tm.listed(A, 4) == [18, 18, 18, 18] and tm.tiles_to_reorder(A, 4) == 0          # one keyframe per rank: no merge to test
    assert tm.listed(A, 8)[4:] == [0, 0, 0, 0]


def test_census_crop_small():
    A = _matrix("crop_small")
    tab = tm.table(A)
    assert len(tab[0]) - 1 == 486 and len(tab[1]) == 1665
    assert tm.listed(A, 2) == [788, 877] and tm.tiles_to_reorder(A, 2) == 374


def test_census_centred():
    A = _matrix("centred")
    tab = tm.table(A)
    assert len(tab[0]) - 1 == 369 and len(tab[1]) == 1256
    assert tm.listed(A, 2) == [677, 579] and tm.tiles_to_reorder(A, 2) == 150 and tm.interleaving_lists(A, 2) == 1538
    assert tm.listed(A, 4) == [405, 400, 272, 179] and tm.tiles_to_reorder(A, 4) == 178 and tm.interleaving_lists(A, 4) == 1934
    assert tm.listed(A, 8)[6:] == [83, 0]


def test_census_off_image():
    assert tm.listed(_matrix("off_image"), 8)[7] == 1


def test_census_seventy_keyframes():
    A = kr.seventy_matrix()
    counts = oc.tile_counts(A)
    assert A.shape[0] == 70 and int(counts.max()) == 70          # tiles of 70 entries: more than one chunk of the merge
    assert min(tm.listed(A, 8)) > 0 and tm.tiles_to_reorder(A, 8) == len(counts)
