"""The plain model of frame ingestion at a pyramid level (tests/frame_ingest.py) against cases worked by hand from the rules of the
reference (B/preprocessing.cc:40-85, L/image.h:929-948 and :1003-1053, L/camera.h:1696-1705) -- the reference's own routines cannot be
compiled here, so these cases and the rules' text are the tie --, the block bounds of the integer rule, the exactness claim behind the
9 x 9 limit, a census showing that the images the GPU tests use reach the cases that matter, and PinholeCamera4f::Scaled held to the
model."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import frame_ingest as fi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("values, expected", [
    ([10, 20], 20),                      # average 15: a tie gives the upper value
    ([10, 20, 30, 100], 30),             # average 40: 30 is closer than 20
    ([1, 50, 60, 61], 50),               # average 43: 50 is closer than 60
    ([5, 9, 7], 7),                      # odd count: the middle of the sorted values
    ([0, 0, 0, 7], 7),                   # zeros are not values
    ([0, 0, 0, 0], 0),                   # nothing left: 0
])
def test_block_median_by_hand(values, expected):
    got = fi.downscale_depth_median(np.array(values, np.uint16).reshape(2, 2) if len(values) == 4 else np.array([values], np.uint16), 1, 1)
    assert got.shape == (1, 1) and int(got[0, 0]) == expected


def test_densify_by_hand():
    centre_two = np.zeros((3, 3), np.uint16)
    centre_two[0, 0], centre_two[2, 1] = 4, 8
    assert int(fi.median_filter_and_densify(centre_two)[1, 1]) == 8                  # {4, 8}: average 6, a tie, the upper value fills
    centre_one = np.zeros((3, 3), np.uint16)
    centre_one[0, 2] = 4
    assert int(fi.median_filter_and_densify(centre_one)[1, 1]) == 0                  # one neighbour is not enough
    lone = np.zeros((3, 3), np.uint16)
    lone[1, 1] = 9
    assert np.array_equal(fi.median_filter_and_densify(lone), lone)                  # a lone value stays, nothing is filled around it
    corner = np.array([[0, 30, 500], [10, 20, 600], [700, 800, 900]], np.uint16)
    assert int(fi.median_filter_and_densify(corner)[0, 0]) == 20                     # the 2 x 2 window {30, 10, 20}, not the 3 x 3 one
    assert int(fi.median_filter_and_densify(np.array([[7]], np.uint16))[0, 0]) == 7
    twice = fi.median_filter_and_densify(centre_two, 2)
    assert np.array_equal(twice, fi.median_filter_and_densify(fi.median_filter_and_densify(centre_two)))


@pytest.mark.parametrize("four, expected", [((3, 3, 3, 3), 0), ((255, 255, 255, 255), 252), ((4, 5, 6, 7), 4)])
def test_colour_halving_by_hand(four, expected):
    rgb = np.zeros((2, 2, 3), np.uint8)
    rgb[..., 1] = np.array(four, np.uint8).reshape(2, 2)
    out = fi.downscale_rgb_half(rgb, 1)
    assert out.shape == (1, 1, 3) and out[0, 0].tolist() == [0, expected, 0]


def test_block_bounds_of_the_integer_rule():
    assert fi.block_bounds(13, 7) == [(0, 1), (1, 3), (3, 5), (5, 7), (7, 9), (9, 11), (11, 13)]        # blocks 1 and 2 wide
    assert fi.block_bounds(7, 4) == [(0, 1), (1, 3), (3, 5), (5, 7)]
    assert fi.scaled_size(645, 2) == 161 and fi.scaled_size(5, 2) == 1
    wide = fi.block_bounds(645, 161)
    assert wide[0] == (0, 4) and wide[-1] == (640, 645) and max(b - a for a, b in wide) == 5 and min(b - a for a, b in wide) == 4
    assert wide[0][0] == 0 and all(a[1] == b[0] for a, b in zip(wide, wide[1:]))                        # a partition of the row
    assert fi.downscale_allowed(645, 5, 161, 1)                                                         # ceil(645 / 161) = 5 <= 9
    assert fi.downscale_allowed(72, 9, 8, 1) and not fi.downscale_allowed(80, 9, 8, 1) and not fi.downscale_allowed(73, 9, 8, 1)
    assert not fi.downscale_allowed(8, 8, 9, 8) and not fi.downscale_allowed(8, 8, 0, 8) and not fi.downscale_allowed(65536, 8, 65536, 8)
    # every block's side is at most ceil(size / out_size), the figure the limit is stated on
    for size, out_size in ((13, 7), (645, 161), (72, 8), (64, 8), (1280, 640), (100, 37)):
        assert max(b - a for a, b in fi.block_bounds(size, out_size)) <= -(-size // out_size)


def test_the_sum_of_a_full_block_is_exact_in_binary32():
    assert 81 * 65535 < 2 ** 24 and 9 * 65535 < 2 ** 24
    assert int(np.float32(81 * 65535)) == 81 * 65535
    block = np.full((9, 9), 65535, np.uint16)
    assert int(fi.downscale_depth_median(block, 1, 1)[0, 0]) == 65535


def test_the_images_of_the_gpu_tests_reach_the_cases_that_matter():
    differ = ties = filled = 0
    for index, shape in enumerate(fi.DENSIFY_SHAPES):
        for name, image in fi.densify_inputs(shape, index).items():
            d, t, f = fi.window_census(image)
            differ, ties, filled = differ + d, ties + t, filled + f
    print("densify: even windows with two different middle values", differ, "exact ties", ties, "filled zeros", filled)
    assert differ > 0 and ties > 0 and filled > 0
    differ = ties = 0
    for index, (shape, (oh, ow)) in enumerate(fi.DOWNSCALE_CASES):
        for name, image in fi.downscale_inputs(shape, index).items():
            d, t = fi.block_census(image, ow, oh)
            differ, ties = differ + d, ties + t
    print("downscale: even blocks with two different middle values", differ, "exact ties", ties)
    assert differ > 0 and ties > 0
    # the tie field alone: every interior window is a tie that must give the upper value
    field = fi.tie_field(6, 6)
    assert fi.window_census(field)[1] >= 16 and int(fi.median_filter_and_densify(field)[1, 1]) == 1010


def test_scaled_camera_on_the_host_matches_the_model(tmp_path):
    exe = str(tmp_path / "scaled_camera_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "badslam_amd", "host"), "-I",
                    os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "scaled_camera_check.cc")], check=True, timeout=300)
    rng = np.random.default_rng(5)
    cases = [((525.0, 525.0, 320.0, 240.0), 640, 480, 1), ((535.4, 539.2, 320.6, 247.1), 641, 481, 1), ((535.4, 539.2, 320.6, 247.1), 641, 481, 2), ((535.4, 539.2, 320.6, 247.1), 645, 5, 2),
             ((726.3, 726.3, 641.2, 481.7), 1280, 960, 3), ((100.0, 100.0, 64.0, 48.0), 128, 96, 0)]
    for _ in range(40):
        cases.append((tuple(float(np.float32(v)) for v in rng.uniform(50, 900, 4)), int(rng.integers(1, 2000)), int(rng.integers(1, 2000)),
                      int(rng.integers(0, 4))))
    text = "".join("%r %r %r %r %d %d %d\n" % (*[float(np.float32(v)) for v in p], w, h, level) for p, w, h, level in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True).stdout.strip().splitlines()
    assert len(out) == len(cases)
    for (p, w, h, level), line in zip(cases, out):
        words = line.split()
        got = np.array([struct.unpack("<f", struct.pack("<I", int(v, 16)))[0] for v in words[:4]], np.float32)
        want, want_w, want_h = fi.scaled_camera(p, w, h, level)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (p, level, got, want)
        assert (int(words[4]), int(words[5])) == (want_w, want_h), (w, h, level, words[4:])
    # the rounding cases, from the host program's own output: 641 / 2 + 0.5 = 321.0 and 645 / 4 + 0.5 = 161.75
    by_case = {(w, h, level): tuple(int(v) for v in line.split()[4:]) for (p, w, h, level), line in zip(cases, out)}
    assert by_case[(641, 481, 1)] == (321, 241) and by_case[(645, 5, 2)] == (161, 1)
    assert fi.scaled_size(641, 1) == 321 and fi.scaled_size(645, 2) == 161
