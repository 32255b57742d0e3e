"""The model of the keyframe redundancy (tests/keyframe_redundancy.py) on hand-made association matrices, and the census of the scenes
and worlds the GPU tests run on (tests/test_gpu_keyframe_redundancy.py, tests/test_gpu_directba_keyframe_redundancy.py): the counts
below were computed from the oracle and are asserted, so that a changed fixture is noticed and the GPU tests keep meaning something --
surfels with every number of observers, a keyframe that sees nothing, a clip that is reached, tiles that overflow the list, a cull that
deletes several keyframes and stops by its rule."""
import numpy as np

from tests import keyframe_redundancy as kr
from tests import observed_covisibility as oc
from tests import surfel_observations as so


def _A(rows):
    return np.array(rows, bool)


def _identities(A, bins):
    """What the definition gives: row sums = the diagonal of A A^T, column j < B - 1 sums to (j + 1) x #{c_s = j + 1}, the list lengths
    of the observation-list model, column 0 the surfels only k sees."""
    A = np.asarray(A, bool)
    hist = kr.table(A, bins)
    assert (hist >= 0).all()
    assert np.array_equal(hist.sum(axis=1), np.diag(oc.matrix(A)))
    first, _ = so.csr(A)
    with_length = np.bincount(so.lengths(first), minlength=bins + 1)
    for j in range(bins - 1):
        assert hist[:, j].sum() == (j + 1) * with_length[j + 1], j
    assert hist[:, bins - 1].sum() == sum(c * n for c, n in enumerate(with_length) if c >= bins)
    alone = A & (A.sum(axis=0) == 1)[None, :]
    if bins > 1:
        assert np.array_equal(hist[:, 0], alone.sum(axis=1))
    assert kr.atomic_ceiling(A, bins) == kr.nonzero_cells(A, bins) <= oc.entries(A) * min(bins, 64)
    return hist


def test_one_keyframe():
    A = _A([[1, 0, 1, 1]])
    assert kr.table(A, 4).tolist() == [[3, 0, 0, 0]]
    assert kr.table(A, 1).tolist() == [[3]]
    assert kr.table(np.zeros((1, 0), bool), 3).tolist() == [[0, 0, 0]]
    assert kr.table(np.zeros((0, 5), bool), 3).shape == (0, 3)
    _identities(A, 4)


def test_a_surfel_nobody_sees_and_one_seen_by_all():
    A = np.zeros((5, 70), bool)
    A[:, 3] = True                          # seen by all five: four other observers
    A[1, 66] = True                         # seen by one, in the second tile; every other surfel by nobody
    hist = _identities(A, 8)
    assert hist[:, 4].tolist() == [1] * 5 and hist[1, 0] == 1 and hist.sum() == 6
    assert oc.tile_counts(A).tolist() == [5, 1] and kr.nonzero_cells(A, 8) == 6
    assert kr.bins_of(A, 8)[[0, 3, 66]].tolist() == [-1, 4, 0]


def test_one_bin_holds_everything():
    A = _A([[1, 1, 0, 1], [1, 0, 0, 1], [1, 1, 0, 0]])
    assert kr.table(A, 1).tolist() == [[3], [2], [2]]
    _identities(A, 1)


def test_the_clip_below_at_and_above_the_largest_count():
    A = np.zeros((4, 10), bool)
    A[:, 0] = True                          # o = 3, the largest
    A[:3, 1] = True                         # o = 2
    A[0, 2] = True                          # o = 0
    assert kr.table(A, 3).tolist() == [[1, 0, 2], [0, 0, 2], [0, 0, 2], [0, 0, 1]]             # B - 1 = 2 < 3: clipped
    assert kr.table(A, 4).tolist() == [[1, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]]   # B - 1 = 3: the last bin is exact
    assert kr.table(A, 5).tolist() == [[1, 0, 1, 1, 0], [0, 0, 1, 1, 0], [0, 0, 1, 1, 0], [0, 0, 0, 1, 0]]
    for bins in (1, 2, 3, 4, 5, 64):
        _identities(A, bins)


def test_a_tile_boundary_and_the_sum_over_shards():
    A = np.zeros((2, 130), bool)
    A[0, 60:70] = True
    A[1, 63:65] = True
    A[1, 129] = True
    hist = _identities(A, 4)
    assert hist.tolist() == [[8, 2, 0, 0], [1, 2, 0, 0]]
    assert kr.nonzero_cells(A, 4) == 2 + 2 + 1 + 1 + 1      # tile 0: both bins for both keyframes; tile 1: two and one; tile 2: one
    assert np.array_equal(kr.sum_over_shards(A, [0, 64, 128, 130], 4), hist)
    assert np.array_equal(kr.sum_over_shards(A, [0, 61, 130], 4), hist)   # shards need not end on tiles
    assert kr.second_traversals(A, 1) == 2 and kr.second_traversals(A, 2) == 0


def test_the_find_rule_orders_by_the_exact_ratio_and_breaks_ties_by_id():
    hist = np.array([[1, 1, 2],             # covered (>= 1) 3 of 4
                     [2, 0, 6],             # 6 of 8: the same ratio, a higher row
                     [0, 0, 5],             # 5 of 5
                     [9, 1, 0],             # 1 of 10: does not qualify at 0.5
                     [0, 0, 0]])            # sees nothing: never qualifies
    assert kr.find(hist, 1, 0.5) == [2, 0, 1]
    assert kr.find(hist, 1, 0.5, ids=[7, 5, 3, 2, 1]) == [3, 5, 7]                     # the tie goes to the lower id
    assert kr.find(hist, 1, 0.75) == [2, 0, 1] and kr.find(hist, 1, 0.76) == [2]      # >=: 0.75 * 4 = 3 qualifies
    assert kr.find(hist, 0, 1.0) == [0, 1, 2, 3] and kr.find(hist, 2, 0.0) == [2, 1, 0, 3]
    # 1 - 1 / (2^31 - 1) against 1 - 1 / (2^31 - 1.5): ratios that a binary64 division does not tell apart (a tie would go to id 4)
    big = np.array([[1, 2 ** 31 - 2], [2, 2 ** 32 - 5]], np.int64)
    assert big[0, 1] / big[0].sum() == big[1, 1] / big[1].sum()
    assert kr.find(big, 1, 0.5, ids=[9, 4]) == [9, 4]


def test_a_cull_recomputes_the_table_after_every_deletion():
    """A deletion lowers the observer counts of the deleted keyframe's surfels and leaves every total alone, so it can only take
    candidates away: no keyframe qualifies after a deletion that did not qualify before it.  What the recomputation changes is the
    reverse, and that is the case here -- rows 1 and 2 are duplicates covered by each other alone, both qualify at first, and the
    second deletion is not the second of the first list but a keyframe further down it, which qualifies before and after."""
    A = np.zeros((6, 12), bool)
    A[0, :] = True                          # the first keyframe sees everything (never deleted)
    A[1, 0:4] = True
    A[2, 0:4] = True                        # 1 and 2: the same four surfels, two other observers each
    A[3, 4:10] = True
    A[4, 4:10] = True
    A[5, 4:12] = True                       # 3, 4, 5 share six surfels (three others), 5 has two more (one other)
    first = kr.find(kr.table(A, 16), 2, 1.0)
    assert first == [1, 2, 3, 4]
    deleted, by_rule = kr.cull(A, 2, 1.0, 10, 0)
    assert deleted == [1, 3, 4] and by_rule                 # after 1 is gone 2 no longer qualifies; 3 and 4 go, then 5 is left with one other
    assert kr.cull(A, 2, 1.0, 1, 0) == ([1], False)         # stopped by max_deletions: a candidate was left
    assert kr.cull(A, 0, 0.0, 10, 2) == ([1, 2, 3], True)   # everything qualifies: all but the first and the two newest
    assert kr.cull(A, 0, 0.0, 10, 0, ids=[3, 4, 6, 8, 9, 11]) == ([4, 6, 8, 9, 11], True)
    assert kr.cull(A, 2, 1.0, 10, 5) == ([], True)


def test_census_of_tiny():
    tc, ba, A = oc.scene("tiny")
    hist = _identities(A, 16)
    first, _ = so.csr(A)
    assert np.bincount(so.lengths(first)).tolist() == [0, 210, 186, 77, 669]              # STATE.md, "Observation lists"
    for bins in (4, 5, 16, 64):
        h = kr.table(A, bins)
        assert h.sum(axis=0)[:4].tolist() == [210, 372, 231, 2676] and not h[:, 4:].any()
        assert h.sum(axis=1).tolist() == [913, 930, 705, 941]
    assert kr.table(A, 2).sum(axis=0).tolist() == [210, 372 + 231 + 2676]
    assert hist[:, :4].tolist() == [[43, 156, 45, 669], [78, 107, 76, 669], [0, 0, 36, 669], [89, 109, 74, 669]]
    assert oc.entries(A) == 72 and kr.nonzero_cells(A, 16) == 139 and oc.tile_counts(A).max() == 4


def test_census_of_the_world_centred():
    A = oc.world_matrix("centred")
    hist = _identities(A, 16)
    seen_by = A.sum(axis=0)
    assert np.bincount(seen_by).tolist() == [19579, 1031, 660, 684, 465, 398, 246, 526]   # surfels seen by 1 .. 7 keyframes
    assert not hist[7].any() and hist[:7].any(axis=1).all()                                 # the keyframe that looks away
    assert (hist[:7, :7] > 0).sum() > 40 and not hist[:, 7:].any()
    assert hist[6].tolist()[:7] == [0, 0, 0, 11, 92, 98, 526]


def test_census_of_the_seventy_keyframes():
    A = kr.seventy_matrix()
    counts = oc.tile_counts(A)
    seen_by = A.sum(axis=0)
    print(np.bincount(seen_by).tolist(), np.bincount(counts).tolist())
    assert A.shape[0] == 70 and int((counts > 64).sum()) >= 4                              # lists of more than 64 entries
    assert seen_by.max() == 70 and int((seen_by >= 65).sum()) > 600                        # o >= 64: the clip at B = 64 is reached
    hist = _identities(A, 64)
    assert (hist[:, 63] > 0).all() and kr.table(A, 64)[:, 63].sum() == int(seen_by[seen_by >= 64].sum())
    _identities(A, 16)
    assert [kr.second_traversals(A, c) for c in (1, 2, 16, 64, 128)] == [18, 18, 18, int((counts > 64).sum()), 0]


def test_census_of_the_duplicated_views():
    scene, images, poses, ba, A = kr.duplicated_views()
    m, f = kr.CULL_RULE
    assert A.shape[0] == kr.DUPLICATED_VIEWS and A.shape[1] > 5000
    _identities(A, 16)
    first = kr.find(kr.table(A, 16), m, f)
    deleted, by_rule = kr.cull(A, m, f, kr.DUPLICATED_VIEWS, 1)
    print(first, deleted)
    assert deleted == [10, 2, 7, 3, 6] and by_rule          # at least two, and stopped by the rule
    assert first[:3] == [10, 2, 6] and 11 in first          # not the first list's order: the table is computed again; 11 is protected
    assert kr.cull(A, m, f, 2, 1) == ([10, 2], False)
    assert kr.cull(A, m, f, kr.DUPLICATED_VIEWS, 3)[0] == [2, 6, 7, 3]
