"""The model of a residual image (tests/residual_image.py) on hand-made pair words, and the census that makes the GPU tests
(tests/test_gpu_residual_image.py) meaningful: the scenes `tiny` and `crop_small` of tests/two_cameras.py, in their perturbed state,
have pixels with several associated pairs, pixels whose best pair is not their lowest index, winners without a valid colour pixel --
and no exact ties of |raw| inside a pixel, which the permutation test relies on.  Measured with the oracle (pairs / explained pixels /
pixels with 2+ pairs / most pairs in a pixel / best is not the lowest index / ties):
  tiny        keyframe 1   930 /    874 /    56 / 2 /  26 / 0      keyframes 0, 2, 3: 28, 7, 37 pixels with 2+ pairs, no ties
  crop_small  keyframe 1 25 792 / 24 375 / 1 404 / 3 / 718 / 0     10 287 of its pairs have no valid colour pixel
The conditions below are well under these figures."""
import numpy as np
import pytest

from tests import residual_image as ri
from tests import two_cameras as tcam


def _bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def _pairs(rows):
    """rows: (associated, px, py, color_valid, raw, inv_std, (r1, r2)) per surfel."""
    cols = list(zip(*rows)) if rows else [[]] * 7
    return ri.pair_words(cols[0], cols[1], cols[2], cols[3], np.array(cols[4], np.float32), np.array(cols[5], np.float32),
                         np.array(cols[6], np.float32).reshape(-1, 2))


def _empty_planes(img, w, h):
    assert np.all(img["key"] == ri.EMPTY_KEY) and not img["pairs"].any() and np.all(img["index"] == ri.EMPTY_INDEX)
    for name in ri.FLOAT_PLANES:
        assert not _bits(img[name]).any(), name          # +0.0, not -0.0
    assert not img["color_valid"].any()
    assert img["key"].shape == (h, w) and img["desc_residual"].shape == (h, w, 2)


@pytest.mark.parametrize("select", [ri.BEST, ri.WORST])
def test_an_empty_frame(select):
    _empty_planes(ri.image(_pairs([]), 5, 3, select), 5, 3)
    nobody = _pairs([(False, 1, 1, True, 0.5, 2.0, (1.0, 2.0)), (False, 0, 0, False, -0.5, 2.0, (0.0, 0.0))])
    img = ri.image(nobody, 5, 3, select)
    _empty_planes(img, 5, 3)
    assert img["stats"]["pairs"] == 0 and img["stats"]["explained"] == 0


@pytest.mark.parametrize("select", [ri.BEST, ri.WORST])
def test_one_pair(select):
    img = ri.image(_pairs([(False, 0, 0, False, 9.0, 9.0, (9.0, 9.0)), (True, 3, 2, True, -0.25, 4.0, (1.5, -2.5))]), 5, 3, select, index_base=100)
    m = 0x3E800000                                       # bits(0.25)
    assert int(img["key"][2, 3]) == (((0x7FFFFFFF - m) if select else m) << 32) | 101
    assert img["index"][2, 3] == 101 and img["pairs"][2, 3] == 1 and img["color_valid"][2, 3] == 1
    assert img["depth_residual"][2, 3] == np.float32(-0.25) and img["inv_stddev"][2, 3] == np.float32(4.0)
    assert img["desc_residual"][2, 3].tolist() == [1.5, -2.5]
    assert img["stats"] == dict(pairs=1, explained=1, multi=0, most=1, not_lowest=0, ties=0, invalid_winners=0)
    rest = np.ones((3, 5), bool)
    rest[2, 3] = False
    assert np.all(img["key"][rest] == ri.EMPTY_KEY) and np.all(img["index"][rest] == ri.EMPTY_INDEX) and not img["pairs"][rest].any()


def test_two_pairs_in_a_pixel_under_both_selects():
    pairs = _pairs([(True, 1, 1, True, 0.75, 2.0, (1.0, 1.0)), (True, 1, 1, True, -0.5, 3.0, (2.0, 2.0)), (True, 0, 1, True, 3.0, 1.0, (3.0, 3.0))])
    best, worst = ri.image(pairs, 2, 2, ri.BEST), ri.image(pairs, 2, 2, ri.WORST)
    assert best["index"][1, 1] == 1 and best["depth_residual"][1, 1] == np.float32(-0.5) and best["inv_stddev"][1, 1] == np.float32(3.0)
    assert worst["index"][1, 1] == 0 and worst["depth_residual"][1, 1] == np.float32(0.75) and worst["desc_residual"][1, 1].tolist() == [1.0, 1.0]
    for img in (best, worst):
        assert img["pairs"].tolist() == [[0, 0], [1, 2]] and img["index"][1, 0] == 2
        assert img["stats"]["multi"] == 1 and img["stats"]["most"] == 2 and img["stats"]["ties"] == 0
    assert best["stats"]["not_lowest"] == 1 and worst["stats"]["not_lowest"] == 0


@pytest.mark.parametrize("select", [ri.BEST, ri.WORST])
def test_an_exact_tie_goes_to_the_lower_index(select):
    # +0.5 and -0.5 have the same magnitude word: the surfels 2, 3 and 4 tie
    pairs = _pairs([(False, 0, 0, False, 0, 0, (0, 0)), (False, 0, 0, False, 0, 0, (0, 0)), (True, 0, 0, True, -0.5, 1.0, (1.0, 1.0)),
                    (True, 0, 0, True, 0.5, 5.0, (5.0, 5.0)), (True, 0, 0, True, 0.5, 2.0, (2.0, 2.0))])
    img = ri.image(pairs, 1, 1, select, index_base=7)
    assert img["index"][0, 0] == 9 and img["depth_residual"][0, 0] == np.float32(-0.5) and img["pairs"][0, 0] == 3
    assert img["stats"]["ties"] == 1 and ri.magnitude_ties(pairs, 1) == 2


def test_a_nan_residual_is_last_under_best_and_first_under_worst():
    rows = [(True, 0, 0, True, 0.0, 1.0, (1.0, 1.0)), (True, 0, 0, True, 100.0, 2.0, (2.0, 2.0)), (True, 0, 0, True, np.inf, 3.0, (3.0, 3.0))]
    for nan_bits in (0x7FC00000, 0xFFC00000, 0x7F800001):
        pairs = _pairs(rows)
        pairs["depth_residual"].view(np.uint32)[0] = nan_bits
        best, worst = ri.image(pairs, 1, 1, ri.BEST), ri.image(pairs, 1, 1, ri.WORST)
        assert best["index"][0, 0] == 1 and worst["index"][0, 0] == 0
        assert int(_bits(worst["depth_residual"])[0, 0]) == nan_bits                # the winner's word as it is
        alone = _pairs(rows[:1])
        alone["depth_residual"].view(np.uint32)[0] = nan_bits
        assert ri.image(alone, 1, 1, ri.BEST)["index"][0, 0] == 0                    # last, but not dropped
        ri.assert_same_bits({"depth_residual": worst["depth_residual"]}, {"depth_residual": np.full((1, 1), np.nan, np.float32)})


@pytest.mark.parametrize("select", [ri.BEST, ri.WORST])
def test_a_colour_invalid_winner_has_no_descriptor_residuals(select):
    # the loser's valid colour pixel does not leak into the winner's planes
    pairs = _pairs([(True, 0, 0, not select, 0.5, 1.0, (7.0, 8.0)), (True, 0, 0, bool(select), 0.25, 2.0, (-7.0, -8.0))])
    img = ri.image(pairs, 1, 1, select)
    assert img["index"][0, 0] == (0 if select else 1)
    assert img["color_valid"][0, 0] == 0 and not _bits(img["desc_residual"]).any()
    assert img["stats"]["invalid_winners"] == 1
    assert img["depth_residual"][0, 0] == np.float32(0.5 if select else 0.25)


def test_shards_composite_to_the_whole():
    rng = np.random.Generator(np.random.PCG64(3))
    n, w, h = 200, 6, 5
    raw = rng.normal(size=n).astype(np.float32)
    pairs = ri.pair_words(rng.random(n) < 0.8, rng.integers(0, w, n), rng.integers(0, h, n), rng.random(n) < 0.5, raw,
                          rng.random(n).astype(np.float32), rng.normal(size=(n, 2)).astype(np.float32))
    cut = lambda a, b: {k: v[a:b] for k, v in pairs.items()}   # noqa: E731
    for select in (ri.BEST, ri.WORST):
        whole = ri.image(pairs, w, h, select, index_base=11)
        parts = [ri.image(cut(0, 70), w, h, select, index_base=11), ri.image(cut(70, 71), w, h, select, index_base=81),
                 ri.image(cut(71, n), w, h, select, index_base=82)]
        ri.assert_same_bits(ri.composite(parts), whole, select)
        assert whole["stats"]["multi"] > 10


# ---- the census -----------------------------------------------------------------------------------------------------------------------
_ORACLES = {}


def _oracle(name):
    if name not in _ORACLES:
        _ORACLES[name] = tcam.build_oracle(tcam.build_scene(name))
    return _ORACLES[name]


def _census(name):
    ba = _oracle(name)
    w, h = int(ba.depth_cam.width), int(ba.depth_cam.height)
    out = []
    for k in range(len(ba.keyframes)):
        pairs = ri.from_oracle(ba, k)
        stats = ri.image(pairs, w, h, ri.BEST)["stats"]
        stats["magnitude_ties"] = ri.magnitude_ties(pairs, w)
        stats["non_finite"] = int(np.count_nonzero(~np.isfinite(pairs["depth_residual"][pairs["associated"]])))
        stats["invalid_pairs"] = int(np.count_nonzero(pairs["associated"] & ~pairs["color_valid"]))
        print(name, "keyframe", k, stats)
        out.append(stats)
    return out


def test_tiny_has_pixels_with_several_pairs_and_winners_that_are_not_the_lowest_index():
    stats = _census("tiny")
    assert stats[1]["multi"] >= 20 and stats[1]["not_lowest"] >= 10, stats[1]          # measured: 56, 26
    assert stats[1]["pairs"] >= 500 and stats[1]["most"] >= 2
    assert all(s["ties"] == 0 and s["magnitude_ties"] == 0 and s["non_finite"] == 0 for s in stats), stats


def test_crop_small_has_many_such_pixels_a_pixel_with_three_pairs_and_colour_invalid_winners():
    stats = _census("crop_small")
    assert max(s["multi"] for s in stats) >= 500, stats                                # measured: 1 404 on keyframe 1
    assert max(s["most"] for s in stats) >= 3, stats
    assert max(s["invalid_winners"] for s in stats) >= 1000, stats
    assert all(s["ties"] == 0 and s["magnitude_ties"] == 0 and s["non_finite"] == 0 for s in stats), stats
