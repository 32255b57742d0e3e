"""Frame ingestion at a pyramid level on the GPU (kernels_ingest.hip behind bahip_median_filter_and_densify,
bahip_downscale_depth_median and bahip_downscale_rgb_half) against the plain model of tests/frame_ingest.py, bit for bit: every
comparison here is for equality.  The images sit in device buffers wider than their rows, with foreign values beside them, so a read or
a write outside the image shows; every refusal must leave the output as it was."""
import functools
import gc

import numpy as np
import pytest

from badslam_amd import capi
from badslam_amd import lowlevel as ll
from tests import frame_ingest as fi

pytestmark = pytest.mark.gpu

PAD = 5                      # columns beside the image inside the device buffers
BESIDE_INPUT = 12345         # what lies beside an input image: a plausible depth, so that reading it would change a median
UNTOUCHED = 0xCDCD           # what an output buffer holds before a call


@pytest.fixture(scope="module")
def ctx():
    c = ll.Context()
    yield c
    c.close()


class Plane:
    """An image in the left columns of a wider device buffer."""

    def __init__(self, ctx, h, w, dtype=np.uint16, channels=1, image=None):
        self.h, self.w, self.channels = h, w, channels
        self.buf = ll.DeviceBuffer2D(ctx, h, w + PAD, dtype, channels)
        if image is None:
            self.buf.clear(0xCD)
        else:
            full = np.full((h, w + PAD) + ((channels,) if channels > 1 else ()), BESIDE_INPUT if dtype == np.uint16 else 201, dtype)
            full[:, :w] = image
            self.buf.upload(full)
            self.uploaded = full
        assert self.buf.pitch > w * self.buf.elem_bytes          # a pitch wider than the row

    def image(self):
        return self.buf.download()[:, :self.w]

    def beside(self):
        return self.buf.download()[:, self.w:]

    def untouched(self):
        full = self.buf.download()
        return bool(np.all(full.view(np.uint8) == 0xCD))


@functools.lru_cache(maxsize=None)
def _densify_model(index, name, iterations=1):
    return fi.median_filter_and_densify(fi.densify_inputs(fi.DENSIFY_SHAPES[index], index)[name], iterations)


@functools.lru_cache(maxsize=None)
def _downscale_model(index, name):
    shape, (oh, ow) = fi.DOWNSCALE_CASES[index]
    return fi.downscale_depth_median(fi.downscale_inputs(shape, index)[name], ow, oh)


def _densify(ctx, image):
    h, w = image.shape
    src, dst = Plane(ctx, h, w, image=image), Plane(ctx, h, w)
    capi.check(ctx.lib.bahip_median_filter_and_densify(ctx.handle, src.buf.ptr, src.buf.pitch, dst.buf.ptr, dst.buf.pitch, w, h))
    ctx.synchronize()
    assert np.array_equal(src.buf.download(), src.uploaded)                       # the input plane is unchanged
    assert np.all(dst.beside() == UNTOUCHED)                                      # nothing written beside the image
    return dst.image()


def _downscale(ctx, image, ow, oh):
    h, w = image.shape
    src, dst = Plane(ctx, h, w, image=image), Plane(ctx, oh, ow)
    capi.check(ctx.lib.bahip_downscale_depth_median(ctx.handle, src.buf.ptr, src.buf.pitch, w, h, dst.buf.ptr, dst.buf.pitch, ow, oh))
    ctx.synchronize()
    assert np.array_equal(src.buf.download(), src.uploaded)
    assert np.all(dst.beside() == UNTOUCHED)
    return dst.image()


def _halve(ctx, rgb, levels):
    h, w = rgb.shape[:2]
    src, dst = Plane(ctx, h, w, np.uint8, 3, image=rgb), Plane(ctx, h >> levels, w >> levels, np.uint8, 3)
    capi.check(ctx.lib.bahip_downscale_rgb_half(ctx.handle, src.buf.ptr, src.buf.pitch, w, h, levels, dst.buf.ptr, dst.buf.pitch))
    ctx.synchronize()
    assert np.array_equal(src.buf.download(), src.uploaded)
    assert np.all(dst.beside() == 0xCD)
    return dst.image()


# ---- densify ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(fi.DENSIFY_SHAPES)), ids=["%dx%d" % (w, h) for h, w in fi.DENSIFY_SHAPES])
def test_densify_equals_the_model(ctx, index):
    for name, image in fi.densify_inputs(fi.DENSIFY_SHAPES[index], index).items():
        got, want = _densify(ctx, image), _densify_model(index, name)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])


def test_densify_fills_and_keeps_by_hand(ctx):
    two = np.zeros((3, 3), np.uint16)
    two[0, 0], two[2, 1] = 4, 8
    assert int(_densify(ctx, two)[1, 1]) == 8                                     # a tie gives the upper value
    one = np.zeros((3, 3), np.uint16)
    one[0, 2] = 4
    assert np.array_equal(_densify(ctx, one), one)
    assert int(_densify(ctx, np.array([[9]], np.uint16))[0, 0]) == 9
    field = fi.tie_field(9, 70)
    assert np.array_equal(_densify(ctx, field), fi.median_filter_and_densify(field))
    assert int(_densify(ctx, field)[1, 1]) == 1010


def test_three_densify_iterations_ping_pong(ctx):
    index = fi.DENSIFY_SHAPES.index((17, 33))
    image = fi.densify_inputs(fi.DENSIFY_SHAPES[index], index)["random"]
    want = _densify_model(index, "random", 3)
    assert not np.array_equal(want, _densify_model(index, "random", 1))           # the iterations go on changing the image
    assert np.array_equal(ll.median_filter_and_densify(ctx, image, 3), want)
    assert np.array_equal(ll.median_filter_and_densify(ctx, image, 0), image)
    h, w = image.shape
    a, b = Plane(ctx, h, w, image=image), Plane(ctx, h, w)
    for _ in range(3):
        capi.check(ctx.lib.bahip_median_filter_and_densify(ctx.handle, a.buf.ptr, a.buf.pitch, b.buf.ptr, b.buf.pitch, w, h))
        a, b = b, a
    ctx.synchronize()
    assert np.array_equal(a.image(), want)


def test_densify_refusals_write_nothing(ctx):
    image = fi.random_depth(6, 8, 1)
    src, dst = Plane(ctx, 6, 8, image=image), Plane(ctx, 6, 8)
    call = ctx.lib.bahip_median_filter_and_densify
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, src.buf.ptr, src.buf.pitch, 8, 6) != 0             # in place
    assert b"in place" in ctx.lib.bahip_last_error()
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, dst.buf.ptr, dst.buf.pitch, 0, 6) != 0
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, dst.buf.ptr, dst.buf.pitch, 8, 0) != 0
    assert call(ctx.handle, src.buf.ptr, 14, dst.buf.ptr, dst.buf.pitch, 8, 6) != 0                        # a pitch shorter than the row
    assert call(ctx.handle, None, src.buf.pitch, dst.buf.ptr, dst.buf.pitch, 8, 6) != 0
    ctx.synchronize()
    assert dst.untouched() and np.array_equal(src.buf.download(), src.uploaded)


# ---- depth downscale --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(fi.DOWNSCALE_CASES)),
                         ids=["%dx%d_to_%dx%d" % (s[1], s[0], o[1], o[0]) for s, o in fi.DOWNSCALE_CASES])
def test_depth_downscale_equals_the_model(ctx, index):
    shape, (oh, ow) = fi.DOWNSCALE_CASES[index]
    for name, image in fi.downscale_inputs(shape, index).items():
        got, want = _downscale(ctx, image, ow, oh), _downscale_model(index, name)
        assert got.shape == (oh, ow) and np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        assert np.array_equal(ll.downscale_depth_median(ctx, image, ow, oh), want)


def test_depth_downscale_by_hand(ctx):
    for values, expected in (([10, 20, 0, 0], 20), ([10, 20, 30, 100], 30), ([1, 50, 60, 61], 50), ([5, 9, 7, 0], 7), ([0, 0, 0, 7], 7),
                             ([0, 0, 0, 0], 0), ([65535, 65535, 65535, 65535], 65535), ([65535, 1, 0, 0], 65535), ([7, 7, 7, 9], 7)):
        got = _downscale(ctx, np.array(values, np.uint16).reshape(2, 2), 1, 1)
        assert int(got[0, 0]) == expected, (values, int(got[0, 0]))
    full = np.full((9, 72), 65535, np.uint16)                                     # 81 values: the largest sum the rule admits
    assert np.array_equal(_downscale(ctx, full, 8, 1), np.full((1, 8), 65535, np.uint16))
    full[4, 40] = 0                                                               # 80 values in one block: even, both middles 65535
    assert np.array_equal(_downscale(ctx, full, 8, 1), np.full((1, 8), 65535, np.uint16))
    same = fi.random_depth(7, 9, 3)
    assert np.array_equal(_downscale(ctx, same, 9, 7), same)                      # blocks of one pixel: the image itself


def test_depth_downscale_refusals_write_nothing(ctx):
    image = fi.random_depth(80, 80, 2)
    src, dst = Plane(ctx, 80, 80, image=image), Plane(ctx, 80, 80)
    call = ctx.lib.bahip_downscale_depth_median

    def refused(w, h, ow, oh, out=None, in_pitch=None, out_pitch=None):
        out = dst.buf.ptr if out is None else out
        rc = call(ctx.handle, src.buf.ptr, src.buf.pitch if in_pitch is None else in_pitch, w, h, out,
                  dst.buf.pitch if out_pitch is None else out_pitch, ow, oh)
        return rc != 0 and len(ctx.lib.bahip_last_error()) > 0

    assert refused(80, 80, 0, 8) and refused(80, 80, 8, 0) and refused(80, 80, -1, 8)                      # 1 <= ow, 1 <= oh
    assert refused(40, 40, 41, 40) and refused(40, 40, 40, 41)                                             # ow <= W, oh <= H
    assert refused(80, 72, 8, 8)                                                                           # ceil(W / ow) = 10
    assert refused(72, 80, 8, 8)                                                                           # ceil(H / oh) = 10
    assert refused(73, 72, 8, 8)                                                                           # ceil(73 / 8) = 10 as well
    assert refused(65536, 8, 65536, 8)                                                                     # W <= 65535 (and the pitch)
    assert refused(0, 8, 1, 1) and refused(8, 0, 1, 1)
    assert refused(72, 72, 8, 8, out=src.buf.ptr)                                                          # in place
    assert refused(72, 72, 8, 8, in_pitch=142) and refused(72, 72, 8, 8, out_pitch=14)
    ctx.synchronize()
    assert dst.untouched() and np.array_equal(src.buf.download(), src.uploaded)
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, 72, 72, dst.buf.ptr, dst.buf.pitch, 8, 8) == 0     # ceil = 9 is admitted
    ctx.synchronize()
    assert np.array_equal(dst.image()[:8, :8], fi.downscale_depth_median(image[:72, :72], 8, 8))


# ---- colour -----------------------------------------------------------------------------------------------------------------------------
def test_colour_halving_equals_repeated_halving(ctx):
    rng = np.random.Generator(np.random.PCG64(9))
    small = rng.integers(0, 256, (2, 2, 3)).astype(np.uint8)
    assert np.array_equal(_halve(ctx, small, 1), fi.halve_rgb(small))
    for shape in ((8, 16), (24, 136)):                                            # 16 x 8, and one with more than a workgroup's row
        rgb = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
        step = rgb
        for levels in (1, 2, 3):
            step = fi.halve_rgb(step)
            got = _halve(ctx, rgb, levels)
            assert got.shape == step.shape and np.array_equal(got, step), (shape, levels)
            assert np.array_equal(ll.downscale_rgb_half(ctx, rgb, levels), step)
    # halving twice is not one average of sixteen: the model's and the kernel's level 2 must differ from it somewhere
    sixteen = (rgb.astype(np.int64).reshape(6, 4, 34, 4, 3).sum(axis=(1, 3)) // 16).astype(np.uint8)
    assert not np.array_equal(fi.downscale_rgb_half(rgb, 2), sixteen)


def test_colour_halving_does_not_round(ctx):
    for value, expected in ((3, 0), (255, 252), (4, 4), (7, 4)):
        got = _halve(ctx, np.full((2, 2, 3), value, np.uint8), 1)
        assert got.shape == (1, 1, 3) and got.ravel().tolist() == [expected] * 3
    mixed = np.zeros((2, 2, 3), np.uint8)
    mixed[..., 0] = [[4, 5], [6, 7]]
    mixed[..., 2] = [[255, 3], [3, 3]]
    assert _halve(ctx, mixed, 1).ravel().tolist() == [4, 0, 63]
    # three levels: 255 -> 252 -> 252 -> 252 (252 // 4 = 63 exactly), 7 -> 4 -> 4 -> 4, 3 -> 0
    for value, expected in ((255, 252), (7, 4), (3, 0)):
        assert _halve(ctx, np.full((8, 8, 3), value, np.uint8), 3).ravel().tolist() == [expected] * 3


def test_colour_refusals_write_nothing(ctx):
    rgb = np.random.Generator(np.random.PCG64(10)).integers(0, 256, (16, 16, 3)).astype(np.uint8)
    src, dst = Plane(ctx, 16, 16, np.uint8, 3, image=rgb), Plane(ctx, 16, 16, np.uint8, 3)
    call = ctx.lib.bahip_downscale_rgb_half
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, 16, 16, 4, dst.buf.ptr, dst.buf.pitch) != 0        # level 4
    assert b"1 .. 3" in ctx.lib.bahip_last_error()
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, 16, 16, 0, dst.buf.ptr, dst.buf.pitch) != 0
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, 15, 16, 1, dst.buf.ptr, dst.buf.pitch) != 0        # odd width
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, 16, 15, 1, dst.buf.ptr, dst.buf.pitch) != 0        # odd height
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, 12, 16, 3, dst.buf.ptr, dst.buf.pitch) != 0        # 12 is not divisible by 8
    assert call(ctx.handle, src.buf.ptr, src.buf.pitch, 16, 16, 1, src.buf.ptr, src.buf.pitch) != 0        # in place
    assert call(ctx.handle, src.buf.ptr, 47, 16, 16, 1, dst.buf.ptr, dst.buf.pitch) != 0
    ctx.synchronize()
    assert dst.untouched() and np.array_equal(src.buf.download(), src.uploaded)


# ---- all three --------------------------------------------------------------------------------------------------------------------------
def test_a_fast_flavour_context_gives_the_same_bits(ctx):
    index = fi.DENSIFY_SHAPES.index((17, 33))
    case = 1
    shape, (oh, ow) = fi.DOWNSCALE_CASES[case]
    rgb = np.random.Generator(np.random.PCG64(11)).integers(0, 256, (8, 16, 3)).astype(np.uint8)
    ctx.set_arithmetic("fast")
    try:
        assert ctx.arithmetic == "fast"
        for name in ("random", "banded", "ties"):
            assert np.array_equal(_densify(ctx, fi.densify_inputs(fi.DENSIFY_SHAPES[index], index)[name]), _densify_model(index, name)), name
        for name in ("random", "banded"):
            assert np.array_equal(_downscale(ctx, fi.downscale_inputs(shape, case)[name], ow, oh), _downscale_model(case, name)), name
        assert np.array_equal(_halve(ctx, rgb, 2), fi.downscale_rgb_half(rgb, 2))
    finally:
        ctx.set_arithmetic("exact")


def test_the_calls_allocate_nothing(ctx):
    image = fi.random_depth(12, 16, 4)
    rgb = np.random.Generator(np.random.PCG64(12)).integers(0, 256, (8, 16, 3)).astype(np.uint8)
    src, dst, small = Plane(ctx, 12, 16, image=image), Plane(ctx, 12, 16), Plane(ctx, 6, 8)
    csrc, cdst = Plane(ctx, 8, 16, np.uint8, 3, image=rgb), Plane(ctx, 4, 8, np.uint8, 3)
    gc.collect()
    before = ll.live_allocations()
    capi.check(ctx.lib.bahip_median_filter_and_densify(ctx.handle, src.buf.ptr, src.buf.pitch, dst.buf.ptr, dst.buf.pitch, 16, 12))
    capi.check(ctx.lib.bahip_downscale_depth_median(ctx.handle, src.buf.ptr, src.buf.pitch, 16, 12, small.buf.ptr, small.buf.pitch, 8, 6))
    capi.check(ctx.lib.bahip_downscale_rgb_half(ctx.handle, csrc.buf.ptr, csrc.buf.pitch, 16, 8, 1, cdst.buf.ptr, cdst.buf.pitch))
    ctx.synchronize()
    assert ll.live_allocations() == before
    assert np.array_equal(small.image(), fi.downscale_depth_median(image, 8, 6))


def test_scaled_camera_of_the_python_layer():
    cam = ll.make_camera([535.4, 539.2, 320.5, 247.25], 645, 481)
    for level in range(4):
        got = ll.scaled_camera(cam, level)
        want, w, h = fi.scaled_camera([cam.fx, cam.fy, cam.cx, cam.cy], 645, 481, level)
        assert np.array_equal(np.array([got.fx, got.fy, got.cx, got.cy], np.float32).view(np.uint32), want.view(np.uint32))
        assert (got.width, got.height) == (w, h)
    with pytest.raises(ValueError):
        ll.scaled_camera(cam, 4)
