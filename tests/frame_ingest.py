"""The plain model of frame ingestion at a pyramid level ("Frame ingestion at a pyramid level"): the three image
rules of BadSlam::PreprocessFrame that run ahead of the bilateral filter, and the camera scaling that goes with them, in Python integers
and numpy.  Written from the rules as DESIGN.md states them; the only floating-point step is the binary32 average of the even case.

  median rule       of n >= 1 non-zero values, sorted: the middle one for odd n; for even n the one of the two middle values that is
                    strictly closer to float32(sum) / float32(n), the upper one on a tie
  densify           the rule on the non-zero values of the 3 x 3 window clipped to the image; fewer than 2 of them: the pixel is copied
  depth downscale   the rule on the non-zero values of the block [(W x) // ow, (W (x + 1)) // ow) x [(H y) // oh, (H (y + 1)) // oh);
                    none: 0
  colour halving    a // 4 + b // 4 + c // 4 + d // 4 per channel, `levels` times
  camera scaling    parameters times 2^-level in binary32, sizes int(2^-level * size + 0.5)
"""
import numpy as np

MAX_LEVEL = 3
MAX_BLOCK = 9           # the depth downscale refuses blocks wider or higher than this: 81 values * 65535 < 2^24


def median_of_valid(values):
    """The median rule on a collection of integers; zeros are no measurements.  Returns None if nothing is left."""
    valid = sorted(int(v) for v in values if int(v) != 0)
    n = len(valid)
    if n == 0:
        return None
    if n % 2 == 1:
        return valid[n // 2]
    low, high = valid[n // 2 - 1], valid[n // 2]
    average = np.float32(sum(valid)) / np.float32(n)
    to_low, to_high = abs(average - np.float32(low)), abs(average - np.float32(high))
    return low if to_low < to_high else high


def census_of(values):
    """(even count with two different middle values, exact tie) of one set: what makes a median case worth testing."""
    valid = sorted(int(v) for v in values if int(v) != 0)
    n = len(valid)
    if n == 0 or n % 2 == 1 or valid[n // 2 - 1] == valid[n // 2]:
        return False, False
    low, high = valid[n // 2 - 1], valid[n // 2]
    average = np.float32(sum(valid)) / np.float32(n)
    return True, bool(abs(average - np.float32(low)) == abs(average - np.float32(high)))


def median_filter_and_densify(depth, iterations=1):
    depth = np.asarray(depth, np.uint16)
    for _ in range(iterations):
        h, w = depth.shape
        out = depth.copy()
        for y in range(h):
            for x in range(w):
                window = depth[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].ravel()
                if np.count_nonzero(window) >= 2:
                    out[y, x] = median_of_valid(window)
        depth = out
    return depth


def block_bounds(size, out_size):
    """[(start, end)] of the out_size blocks a side of `size` pixels is cut into."""
    return [((size * i) // out_size, (size * (i + 1)) // out_size) for i in range(out_size)]


def downscale_allowed(w, h, ow, oh):
    return (1 <= ow <= w and 1 <= oh <= h and w <= 65535 and h <= 65535 and -(-w // ow) <= MAX_BLOCK and -(-h // oh) <= MAX_BLOCK)


def downscale_depth_median(depth, out_width, out_height):
    depth = np.asarray(depth, np.uint16)
    h, w = depth.shape
    assert downscale_allowed(w, h, out_width, out_height)
    out = np.zeros((out_height, out_width), np.uint16)
    for y, (y0, y1) in enumerate(block_bounds(h, out_height)):
        for x, (x0, x1) in enumerate(block_bounds(w, out_width)):
            m = median_of_valid(depth[y0:y1, x0:x1].ravel())
            out[y, x] = 0 if m is None else m
    return out


def halve_rgb(rgb):
    rgb = np.asarray(rgb, np.uint8)
    assert rgb.shape[0] % 2 == 0 and rgb.shape[1] % 2 == 0
    q = rgb.astype(np.int64) // 4
    return (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]).astype(np.uint8)


def downscale_rgb_half(rgb, levels):
    assert 1 <= levels <= MAX_LEVEL
    for _ in range(levels):
        rgb = halve_rgb(rgb)
    return rgb


def scaled_size(size, level):
    return int(float(np.float32(1.0) / np.float32(1 << level)) * size + 0.5)


def scaled_camera(params, width, height, level):
    """((fx, fy, cx, cy) float32 in the pixel-corner convention, width, height) at a pyramid level."""
    factor = np.float32(1.0) / np.float32(1 << level)
    return (np.asarray(params, np.float32) * factor).astype(np.float32), scaled_size(width, level), scaled_size(height, level)


# ---- the random images of the GPU tests (tests/test_gpu_frame_ingest.py) and their census (tests/test_cpu_frame_ingest.py) -------------
def random_depth(h, w, seed, zero_fraction=0.4, low=1, high=65536, near=None):
    """Raw depth with about `zero_fraction` zeros.  near = (centre, spread): values within a narrow band, so that windows and blocks
    hold equal values and exact ties (two middle values at the same distance from the average) occur."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if near is None:
        d = rng.integers(low, high, (h, w))
    else:
        d = near[0] + rng.integers(-near[1], near[1] + 1, (h, w))
    d = np.where(rng.random((h, w)) < zero_fraction, 0, d)
    return d.astype(np.uint16)


def tie_field(h, w):
    """Every interior 3 x 3 window holds six values in two equal groups (rows of 0 / a / b repeating): an even count with two different
    middle values at the same distance from the average -- the tie must give the upper one."""
    rows = np.array([0, 1000, 1010], np.uint16)
    return np.repeat(rows[np.arange(h) % 3][:, None], w, axis=1)


DENSIFY_SHAPES = [(1, 1), (7, 1), (1, 7), (3, 3), (17, 33), (46, 64), (5, 130)]          # (height, width) of 1x1, 1x7, 7x1, ... as w x h
DOWNSCALE_CASES = [((6, 8), (3, 4)), ((7, 13), (4, 7)), ((5, 645), (1, 161)), ((48, 64), (6, 8)), ((9, 72), (1, 8))]   # (h, w) -> (oh, ow)


def densify_inputs(shape, index):
    h, w = shape
    return {"random": random_depth(h, w, 100 + index), "banded": random_depth(h, w, 200 + index, near=(3000, 3)),
            "zero": np.zeros((h, w), np.uint16), "full": np.full((h, w), 65535, np.uint16), "ties": tie_field(h, w)}


def downscale_inputs(shape, index):
    h, w = shape
    rng = np.random.Generator(np.random.PCG64(400 + index))
    single = np.zeros((h, w), np.uint16)
    single[::3, ::2] = rng.integers(1, 65536, single[::3, ::2].shape)          # sparse: many blocks with one value or none
    return {"random": random_depth(h, w, 300 + index), "banded": random_depth(h, w, 350 + index, zero_fraction=0.2, near=(3000, 2)),
            "zero": np.zeros((h, w), np.uint16), "full": np.full((h, w), 65535, np.uint16), "sparse": single}


def window_census(depth):
    """(windows with an even count and two different middle values, exact ties among them, zeros that get filled)."""
    depth = np.asarray(depth, np.uint16)
    h, w = depth.shape
    differ = ties = filled = 0
    for y in range(h):
        for x in range(w):
            window = depth[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].ravel()
            d, t = census_of(window)
            differ, ties = differ + d, ties + t
            filled += depth[y, x] == 0 and np.count_nonzero(window) >= 2
    return differ, ties, filled


def block_census(depth, out_width, out_height):
    depth = np.asarray(depth, np.uint16)
    differ = ties = 0
    for y0, y1 in block_bounds(depth.shape[0], out_height):
        for x0, x1 in block_bounds(depth.shape[1], out_width):
            d, t = census_of(depth[y0:y1, x0:x1].ravel())
            differ, ties = differ + d, ties + t
    return differ, ties
