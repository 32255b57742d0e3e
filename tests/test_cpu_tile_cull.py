"""The numpy model of the tile cull (tests/tile_cull.py) and the edge clouds the GPU tests use, checked without a GPU: the model on
hand-worked cases; the model against the oracle -- it culls no (tile, keyframe) for which the oracle puts a live member into the image
with z > 0, no band --; its binary32 and binary64 forms against each other outside the band; the census that makes the GPU tests
meaningful, per camera shape; and every mutant of the model shown to lose associated pairs on these very inputs."""
import numpy as np
import pytest

from tests import tile_cull as tc

F32 = np.float32
IDENTITY = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F32)
HAND = (32.0, 32.0, 40.0, 30.0)          # at 80 x 60: the planes pass through x = -+2.5, y = -+1.875 at z = 2, all exact in binary32
NAN = np.nan


def _tile(*points):
    p = np.full((3, 64), NAN, F32)
    for j, q in enumerate(points):
        p[:, 5 + 7 * j] = q                  # live entries anywhere in the tile
    return p


def _decide(points, frames=IDENTITY, camera=HAND):
    b = tc.wave_bounds32(_tile(*points))
    may, first = tc.sphere_may_project(F32, camera, frames, b)
    may64, first64 = tc.sphere_may_project(np.float64, camera, frames, b)
    assert np.array_equal(may, may64) and np.array_equal(first, first64)
    return b[0], bool(may[0, 0]), int(first[0, 0])


def test_an_empty_tile():
    b, may, first = _decide([])
    assert list(b) == [0, 0, 0, -1] and not may and first == -2
    b = tc.wave_bounds32(np.full((3, 130), NAN, F32))
    assert b.shape == (3, 4) and (b[:, 3] == -1).all()
    assert np.array_equal(tc.masks_of(np.zeros((3, 70), bool)), np.zeros((3, 2), np.uint64))


def test_one_point():
    b, may, first = _decide([(0.25, -0.5, 2.0)])
    assert list(b[:3]) == [0.25, -0.5, 2.0] and b[3] == F32(0.01) and may and first == -1


def test_the_sphere_of_two_points():
    b, _, _ = _decide([(1.0, 2.0, 3.0), (3.0, 2.0, 7.0)])
    assert list(b[:3]) == [2.0, 2.0, 5.0]
    assert b[3] == np.sqrt(F32(5.0)) * F32(1.001) + F32(0.01)
    b64 = tc.wave_bounds64(_tile((1.0, 2.0, 3.0), (3.0, 2.0, 7.0)))[0]
    assert abs(b64[3] - (5 ** 0.5 * 1.001 + 0.01)) < 1e-15 and abs(float(b[3]) - b64[3]) < 4 * 2.0 ** -24 * b64[3]


@pytest.mark.parametrize("plane,on,normal", [
    (1, (-2.5, 0.3, 2.0), (32.0, 0.0, 40.0)),        # left:   fx x + cx z = 0, inside where positive
    (2, (2.5, -0.4, 2.0), (-32.0, 0.0, 40.0)),       # right:  fx x + (cx - W) z = 0, inside where negative
    (3, (0.2, -1.875, 2.0), (0.0, 32.0, 30.0)),      # top
    (4, (-0.1, 1.875, 2.0), (0.0, -32.0, 30.0)),     # bottom
    (0, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)),           # z = 0
])
def test_a_point_on_each_plane(plane, on, normal):
    """A tile of one point has r = 1 cm: on the plane and up to r outside it the keyframe is kept, beyond r it is culled -- by that
    plane first.  (1 % either side of r: far outside any rounding.)"""
    n = np.array(normal) / np.linalg.norm(normal)
    on = np.array(on)
    assert _decide([on])[1:] == (True, -1)
    assert _decide([on - 0.0099 * n])[1:] == (True, -1)
    assert _decide([on + 0.5 * n])[1] is True                         # half a metre to the inner side
    assert _decide([on - 0.0101 * n])[1:] == (False, plane)
    # the binary64 value on the plane is the margin alone: r * |normal| (r itself on the z plane)
    values, _, _, margins = tc.plane_values(np.float64, HAND, IDENTITY, tc.wave_bounds32(_tile(on)))
    assert abs(abs(values[plane, 0, 0]) - float(F32(0.01)) * (np.linalg.norm(normal) if plane else 1.0)) < 1e-12
    assert abs(margins[plane, 0, 0] - abs(values[plane, 0, 0])) < 1e-12


def test_a_sphere_that_contains_the_camera_centre():
    """Whatever the keyframe looks at: a sphere around its centre reaches into the image."""
    rng = np.random.Generator(np.random.PCG64(2))
    poses = [np.concatenate([q / np.linalg.norm(q), t]) for q, t in zip(rng.normal(size=(20, 4)), rng.uniform(-3, 3, (20, 3)))]
    frames = np.stack([tc.frame_T_global(p) for p in poses])
    for camera in [HAND] + [tc.SHAPES[s]["camera"] for s in tc.SHAPES]:
        for k, pose in enumerate(poses):
            c = pose[4:]
            members = [c + d for d in ((1.5, -2.0, 0.7), (-1.5, 2.0, -0.7), (0.3, 0.2, -0.1))]
            b = tc.wave_bounds32(_tile(*members))
            assert np.abs(b[0, :3] - c).max() < 1e-6 and b[0, 3] > 2.5
            may, first = tc.sphere_may_project(F32, camera, frames[k:k + 1], b)
            assert may[0, 0] and first[0, 0] == -1, (camera, k)


def test_masks_round_trip():
    rng = np.random.Generator(np.random.PCG64(3))
    may = rng.random((5, 70)) < 0.5
    masks = tc.masks_of(may)
    assert masks.shape == (5, 2) and masks.dtype == np.uint64 and not (masks[:, 1] >> np.uint64(6)).any()
    assert np.array_equal(tc.may_of(masks, 70), may)


def test_the_mutants_differ_from_the_model_only_by_their_error():
    """On a sphere deep inside the image no mutant culls; each mutant's own plane is the one that moved."""
    b = tc.wave_bounds32(_tile((0.1, -0.2, 3.0)))
    for mutant in tc.MUTANTS:
        may, _ = tc.sphere_may_project(F32, HAND, IDENTITY, b, mutant)
        assert may[0, 0] == (mutant != "no_size"), mutant
    v = tc.plane_values(np.float64, HAND, IDENTITY, b)[0][:, 0, 0]
    moved = {"inward": [1, 2, 3, 4], "size_minus_1": [2, 4], "z_centre": [], "unscaled_margin": [1, 2, 3, 4], "no_size": [2, 4]}
    for mutant, planes in moved.items():
        m = tc.plane_values(np.float64, HAND, IDENTITY, b, mutant)[0][:, 0, 0]
        assert [q for q in range(5) if m[q] != v[q]] == planes, mutant


# ---- the worlds ------------------------------------------------------------------------------------------------------------------------
SHAPES = list(tc.SHAPES)


@pytest.mark.parametrize("name", SHAPES)
def test_the_keyframe_images_are_valid_in_every_pixel(name):
    w = tc.world(name)
    assert len(w.poses) == len(w.images) == 8 and len(w.kinds) <= tc.MAX_TILES
    for k, image in enumerate(w.images):
        assert image["depth"].shape == (tc.H, tc.W)
        assert not (image["depth"] & 0x8000).any(), k                  # the border ring and the ring inside it included
        assert (image["radius"] != 0).all(), k
        assert 0 < image["min_depth"] <= image["max_depth"]
    kinds = set(w.kinds)
    assert kinds == {"single", "outside", "straddle", "compact", "centre", "dead", "ragged"}
    live = (w.surfels[0] == w.surfels[0]).reshape(-1)
    per = np.add.reduceat(live.astype(int), np.arange(0, len(live), 64))
    assert (per[w.kinds == "single"] == 1).all() and (per[w.kinds == "compact"] == 64).all() and (per[w.kinds == "dead"] == 0).all()
    assert ((per[w.kinds == "outside"] >= 2) & (per[w.kinds == "outside"] <= 5)).all() and set(per[w.kinds == "outside"]) == {2, 3, 4, 5}
    assert w.surfels.shape[1] % 64 == 37 and w.kinds[-1] == "ragged"


@pytest.mark.parametrize("name", SHAPES)
def test_the_model_is_conservative_against_the_oracle(name):
    """No band: wherever the oracle projects a live member of a tile into a keyframe's image with z > 0, the binary32 model keeps that
    keyframe for the tile.  The border surfels sit 0.01 px from the border -- the oracle's own binary32 projection decides on which
    side -- and the outside ones must indeed be outside for it."""
    w, p = tc.world(name), tc.pairs(name)
    bounds = tc.wave_bounds32(w.surfels[:3])
    may, _ = tc.sphere_may_project(F32, w.camera, p.frames, bounds)
    inside = tc.per_tile(p.in_image)
    assert inside.sum() > 500
    assert not (inside & ~may).any(), np.argwhere(inside & ~may)[:5]
    # the singles placed 0.01 px outside a border are outside for the oracle, the ones 0.01 px inside are inside
    singles = np.flatnonzero(w.kinds == "single")
    at_home = p.in_image[w.home[singles], singles * 64]
    assert 0.70 < at_home.mean() < 0.80, at_home.mean()                # three of the four offsets
    # the tiles built around an outside centre have it outside: the sphere's centre alone would not keep the keyframe
    for kind in ("outside", "straddle"):
        t = np.flatnonzero(w.kinds == kind)
        centre_only = bounds[t].copy()
        centre_only[:, 3] = 0
        kept, _ = tc.sphere_may_project(F32, w.camera, p.frames, centre_only)
        home = kept[np.arange(len(t)), w.home[t]]
        assert (~home).mean() > 0.9 and inside[t, w.home[t]].mean() > 0.9, (kind, home.mean())


@pytest.mark.parametrize("name", SHAPES)
def test_binary32_and_binary64_agree_outside_the_band(name):
    w, p = tc.world(name), tc.pairs(name)
    bounds = tc.wave_bounds32(w.surfels[:3])
    b64 = tc.wave_bounds64(w.surfels[:3])
    live = bounds[:, 3] >= 0
    scale = np.abs(b64[live]).max()
    assert np.abs(bounds[live, :3] - b64[live, :3]).max() <= 2.0 ** -23 * scale
    # r: the centre's rounding (2^-24 of a coordinate) comes back in max - centre on each axis, sqrt(3) of it in the half-diagonal, times
    # two for the subtraction's own rounding; then seven more roundings relative to r
    assert (np.abs(bounds[live, 3] - b64[live, 3]) <= 4 * 2.0 ** -24 * scale + 7 * 2.0 ** -24 * b64[live, 3]).all()
    may32, first32 = tc.sphere_may_project(F32, w.camera, p.frames, bounds)
    may64, first64 = tc.sphere_may_project(np.float64, w.camera, p.frames, bounds)
    for fast in (False, True):
        band = tc.in_band(w.camera, p.frames, bounds, fast=fast)
        assert np.array_equal(may32[~band], may64[~band])
        assert band.mean() <= 0.01, band.mean()
    print(f"{name}: {int(tc.in_band(w.camera, p.frames, bounds).sum())} of {may32.size} decisions inside the band (C = {tc.C_BAND}), "
          f"{int((may32 != may64).sum())} differ")


@pytest.mark.parametrize("name", SHAPES)
def test_census(name):
    """What the GPU tests rest on.  Measured (centred / neg_fy / off_image / narrow / wide): 369 tiles, 4141 .. 4159 live surfels,
    11773 .. 14397 associated pairs; associated pairs in the outermost pixel ring 1268 / 1273 / 1285 / 1155 / 1513, at least 270 on
    every side and 17 in every corner; single-entry tiles with an associated pair 207 .. 210; every plane the first to cull at least
    175 decisions; 47 .. 53 % of the decisions culled; (tile, keyframe) decisions with an associated pair that the mutants would lose:
    inward 94 .. 133, size_minus_1 50 .. 76, z_centre 31 .. 40, unscaled_margin 229 .. 259, no_size 905 .. 1172."""
    c = tc.census(name)
    print(name, c)
    assert c["tiles"] <= tc.MAX_TILES
    assert c["outer"] >= 100 and min(c["sides"]) >= 20 and min(c["corners"]) >= 1, c
    assert c["single_associated"] >= 50, c
    assert min(c["first"]) >= 20, c
    assert 0.2 <= c["culled_share"] <= 0.8, c
    assert min(c["mutants"].values()) >= 20, c
    assert c["straddle"] >= 20, c                     # tiles across keyframe 6's z = 0 plane with a member it associates
