"""The tile cull of the surfel sweeps (badslam_amd/csrc/wave_cull.h: wave_bounds, sphere_may_project) restated in numpy, and the
edge clouds that hold it to its promise, for tests/test_cpu_tile_cull.py and tests/test_gpu_tile_cull.py.  A plain module: no
fixtures, no conftest.

MODEL.  wave_bounds32 and sphere_may_project in numpy binary32, operation for operation in the order the C++ source spells them (numpy
rounds every elementwise operation to binary32 and contracts nothing; the exact build has -ffp-contract=off and a correctly rounded
sqrtf, as numpy's), and the same formula in binary64 on the same binary32 inputs (the tile's sphere as the device holds it, the
keyframe's frame_T_global, the camera).

BAND.  A decision of the binary32 form may legitimately differ from the binary64 one only where a plane's value lies within
    C * 2^-24 * (sum of the magnitudes of all terms of that plane's expression)
of zero.  C = 2 * 7 = 14: the longest chain of roundings from the inputs to a plane's value, counted from sphere_may_project, is
    F[0] * cx (1)  + F[1] * cy (2)  + F[2] * cz (3)  + F[3] (4)  |  fx * lx (5)  + (cx - w) * lz (6)  - r * norm (7)
(the other operands arrive with fewer: (cx - w) 1, its square 2, + fx * fx 3, sqrtf 4, r * 5; lz 4; the z plane's lz + r has 5), each
rounding at most 2^-24 relative to a partial result that the sum of the term magnitudes bounds, and twice that for slack.  The fast
flavour contracts at the compiler's discretion (fewer roundings, never more) and takes the approximate square root twice, once in the
sphere's radius and once in the plane's norm: the public CDNA instruction set documentation gives v_sqrt_f32 1 ulp, the compiler flag
that selects it (-fno-hip-fp32-correctly-rounded-divide-sqrt) licenses 2.5 ulp = 5 * 2^-24 relative; the fast band adds
2 * 5 * 2^-24 * |r * norm| (5 * 2^-24 * r on the z plane) for the larger of the two.  The fast flavour the probe reports is the
compilation of the probe's own unit (flushed denormals, contraction as the compiler chose it there), not of any sweep's inlined copy.

MUTANTS of the model (never of the kernels): the formula with one subtle error each -- what a too-tight cull looks like.

WORLDS.  Five depth-camera shapes at 80 x 60 pixels (SHAPES); per shape at most 8 keyframes whose depth, normal and radius images are
valid in EVERY pixel, the two outermost rings included: rendered and preprocessed by the oracle at 84 x 64 with the principal point
shifted by 2, then cropped (the renderer's invalid border and the two rings the preprocessing invalidates fall outside the crop).
Keyframe 6 stands close to the surface, tilted, so that its z = 0 plane cuts through the surfels; keyframe 7 looks away (at a plane of
its own behind the cameras).  The clouds are placed by hand: surfels on the rendered planes on the rays through chosen sub-pixel
positions of a keyframe -- 0.01, 0.5, 0.99 px inside and 0.01 px outside each border, corners included; each then moved along its
ray by up to 0.1 % of its distance, which keeps the pixel position and gives the depth residuals a size -- arranged into tiles of one
live entry (63 NaN), tiles of two to five entries whose centre lies outside the image (or behind keyframe 6's z = 0 plane) while a
member lies inside, full compact tiles over the images' corners and borders, one tile of far-apart members whose sphere holds a camera
centre, an all-dead tile and a ragged last tile.  census() counts what the tests then require of them."""
import ctypes as C
import functools

import numpy as np

from badslam_amd import se3, synthetic
from oracle import binding as ob

F32 = np.float32
W, H = 80, 60
MARGIN = 2                      # rings rendered around the image and cropped away
BASELINE_FX, CELL = 40.0, 2
C_BAND = 14                     # 2 x 7 roundings (see the module docstring)
SQRT_FAST = 5.0                 # the approximate square root: 2.5 ulp = 5 * 2^-24 relative
MAX_TILES = 400
OFFSETS = (0.01, 0.5, 0.99, -0.01)      # px from a border: three inside, one outside
DISPLACEMENT = 1e-3                     # of a surfel's distance, along its ray, off the surface
MUTANTS = ("inward", "size_minus_1", "z_centre", "unscaled_margin", "no_size")
PLANE_NAMES = ("z", "left", "right", "top", "bottom")

# fx, fy, cx, cy (pixel-corner convention); raw_to_float_depth and the planes' distance so that a pixel at that distance is several
# times the 1 cm of a single-entry tile's sphere -- what lets a plane one pixel inward lose that tile (narrow: 10 m / 400 = 2.5 cm);
# slope of the planes, rotation of keyframes 1 .. 5 (rad) and tilt of keyframe 6 (rad, about which axis) so that every ray of every
# keyframe still meets a plane within the raw depth range
SHAPES = {
    "centred":   dict(camera=(30.0, 30.0, 39.5, 29.5), scale=1.0 / 5000, distance=2.5, slope=0.25, rotation=0.12, tilt=(0.45, 1), height=0.5),
    "neg_fy":    dict(camera=(30.0, -30.0, 39.5, 29.5), scale=1.0 / 5000, distance=2.5, slope=0.25, rotation=0.12, tilt=(-0.45, 0), height=0.5),
    "off_image": dict(camera=(30.0, 30.0, -20.0, 75.0), scale=1.0 / 10000, distance=1.5, slope=0.05, rotation=0.04, tilt=(-1.0, 1), height=1.0),
    "narrow":    dict(camera=(400.0, 400.0, 39.5, 29.5), scale=1.0 / 2000, distance=10.0, slope=0.25, rotation=0.02, tilt=(1.0, 1), height=0.15),
    "wide":      dict(camera=(12.0, 12.0, 39.5, 29.5), scale=1.0 / 12000, distance=1.2, slope=0.04, rotation=0.03, tilt=(0.2, 0), height=0.35),
}


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def tiles_of(positions):
    """(3, N) binary32 positions (NaN x = dead) -> (3, T, 64), the ragged last tile padded with dead entries."""
    p = np.asarray(positions, F32)
    n = p.shape[1]
    t = (n + 63) // 64
    out = np.full((3, t * 64), np.nan, F32)
    out[:, :n] = p
    return out.reshape(3, t, 64)


def wave_bounds32(positions):
    """wave_bounds per 64-entry tile: (T, 4) binary32 -- centre and inflated radius; 0, 0, 0, -1 for a tile without a live entry."""
    p = tiles_of(positions)
    valid = p[0] == p[0]
    inf = F32(np.inf)
    lo = [np.where(valid, p[a], inf).min(axis=1) for a in range(3)]
    hi = [np.where(valid, p[a], -inf).max(axis=1) for a in range(3)]
    empty = ~(hi[0] >= lo[0])
    out = np.zeros((p.shape[1], 4), F32)
    with np.errstate(invalid="ignore"):
        c = [F32(0.5) * (lo[a] + hi[a]) for a in range(3)]
        d = [hi[a] - c[a] for a in range(3)]
        r = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) * F32(1.001) + F32(0.01)
    for a in range(3):
        out[:, a] = np.where(empty, F32(0), c[a])
    out[:, 3] = np.where(empty, F32(-1), r)
    assert out.dtype == F32 and all(v.dtype == F32 for v in c + d + [r])
    return out


def wave_bounds64(positions):
    """The same sphere in binary64 from the same binary32 positions (NaN rows for an empty tile)."""
    p = tiles_of(positions).astype(np.float64)
    valid = p[0] == p[0]                                # x alone marks a dead entry
    lo, hi = np.where(valid, p, np.inf).min(axis=2), np.where(valid, p, -np.inf).max(axis=2)
    lo, hi = np.where(hi >= lo, lo, np.nan), np.where(hi >= lo, hi, np.nan)
    c = 0.5 * (lo + hi)
    d = hi - c
    r = np.sqrt((d * d).sum(axis=0)) * 1.001 + 0.01
    return np.concatenate([c, r[None]]).T


def plane_values(dtype, camera, frames, bounds, mutant=None):
    """The five plane expressions of sphere_may_project in `dtype` for every (tile, keyframe): camera = (fx, fy, cx, cy), frames (K, 12)
    frame_T_global, bounds (T, 4).  Returns (values (5, T, K), culled (5, T, K): the plane's own test, magnitudes (5, T, K): the sum
    of the magnitudes of the terms of the plane's expression, margins (5, T, K): |r * norm|)."""
    dt = dtype
    fx, fy, cx, cy = (dt(v) for v in camera)
    w, h = dt(W), dt(H)
    if mutant == "size_minus_1":
        w, h = dt(W - 1), dt(H - 1)
    b = np.asarray(bounds, F32).astype(dt)[:, None, :]
    F = np.asarray(frames, F32).astype(dt)[None, :, :]
    c0, c1, c2, r = b[..., 0], b[..., 1], b[..., 2], b[..., 3]

    def row(o):
        return ((F[..., o] * c0 + F[..., o + 1] * c1) + F[..., o + 2] * c2) + F[..., o + 3]

    def row_magnitude(o):
        return np.abs(F[..., o] * c0) + np.abs(F[..., o + 1] * c1) + np.abs(F[..., o + 2] * c2) + np.abs(F[..., o + 3])

    lx, ly, lz = row(0), row(4), row(8)
    mx, my, mz = row_magnitude(0), row_magnitude(4), row_magnitude(8)
    one = dt(1)
    if mutant == "inward":          # px >= 1, px < W - 1, py >= 1, py < H - 1
        ax = (cx - one, cx - (w - one))
        ay = (cy - one, cy - (h - one))
    elif mutant == "no_size":       # the right and bottom planes without the image size
        ax, ay = (cx, cx), (cy, cy)
    else:
        ax, ay = (cx, cx - w), (cy, cy - h)

    def norm(f, a):
        return one if mutant == "unscaled_margin" else np.sqrt(f * f + a * a)

    values, culled, magnitudes, margins = [lz + r], [(lz if mutant == "z_centre" else lz + r) <= 0], [mz + np.abs(r)], [np.abs(r)]
    for f, l, ml, a, sign in ((fx, lx, mx, ax[0], 1), (fx, lx, mx, ax[1], -1), (fy, ly, my, ay[0], 1), (fy, ly, my, ay[1], -1)):
        margin = r * norm(f, a)
        v = (f * l + a * lz) + margin if sign > 0 else (f * l + a * lz) - margin
        values.append(v)
        culled.append(v < 0 if sign > 0 else v > 0)
        magnitudes.append(np.abs(f) * ml + np.abs(a) * mz + np.abs(margin))
        margins.append(np.abs(margin) + 0 * v)
    shape = np.broadcast(values[1], values[0]).shape
    stack = lambda xs: np.stack([np.broadcast_to(x, shape) for x in xs])    # noqa: E731
    return stack(values), stack(culled), stack(magnitudes), stack(margins)


def sphere_may_project(dtype, camera, frames, bounds, mutant=None):
    """(may (T, K) bool, first (T, K) int: the first plane that culls -- 0 z, 1 left, 2 right, 3 top, 4 bottom --, -1 where none does,
    -2 for an empty tile)."""
    values, culled, _, _ = plane_values(dtype, camera, frames, bounds, mutant)
    empty = (np.asarray(bounds, F32)[:, 3] < 0)[:, None]
    any_culled = culled.any(axis=0)
    first = np.where(any_culled, culled.argmax(axis=0), -1)
    first = np.where(empty, -2, first)
    return ~any_culled & ~empty, first


def in_band(camera, frames, bounds, fast=False):
    """(T, K) bool: some plane's binary64 value lies within the band (the exact flavour's, or the fast flavour's) of zero -- there,
    and only there, a binary32 decision may differ from the binary64 one."""
    values, _, magnitudes, margins = plane_values(np.float64, camera, frames, bounds)
    band = C_BAND * 2.0 ** -24 * magnitudes
    if fast:
        band = band + 2 * SQRT_FAST * 2.0 ** -24 * margins
    empty = (np.asarray(bounds, F32)[:, 3] < 0)[:, None]
    return (np.abs(values) <= band).any(axis=0) & ~empty


def masks_of(may):
    """(T, K) bool -> (T, ceil(K / 64)) uint64 as bahip_debug_tile_cull reports them."""
    t, k = may.shape
    words = (k + 63) // 64
    out = np.zeros((t, max(1, words)), np.uint64)
    for j in range(k):
        out[:, j // 64] |= may[:, j].astype(np.uint64) << np.uint64(j % 64)
    return out[:, :words]


def may_of(masks, k):
    """(T, words) uint64 -> (T, k) bool."""
    m = np.asarray(masks, np.uint64)
    return np.stack([(m[:, j // 64] >> np.uint64(j % 64)) & np.uint64(1) for j in range(k)], axis=1).astype(bool)


def frame_T_global(pose):
    """frame_T_global (12 binary32 words) of a global_T_frame as the oracle -- and the backend's bind -- computes it."""
    kf = ob.Keyframe()
    T = ob.SE3.from_array(pose)
    ob.lib().orc_keyframe_set_global_T_frame(C.byref(kf), C.byref(T))
    return np.array(list(kf.frame_T_global), F32)


# ---- worlds --------------------------------------------------------------------------------------------------------------------------
class World:
    """One camera shape: name, spec, camera (4 binary32), planes, poses (global_T_frame), images (per keyframe: depth, normals, radius,
    color, min_depth, max_depth), surfels (17, N) binary32, kinds (per tile: 'single', 'outside', 'straddle', 'compact', 'centre',
    'dead', 'ragged'), home (per tile: the keyframe it was placed for, -1 none)."""


def _rot(axis, angle):
    xi = np.zeros(6)
    xi[3 + axis] = angle
    return se3.exp(xi)


def _poses(spec):
    fx, fy, cx, cy = spec["camera"]
    d, rot = spec["distance"], spec["rotation"]
    half_w, half_h = 0.5 * W / abs(fx) * d, 0.5 * H / abs(fy) * d
    T0 = se3.exp([0.01, 0.02, 0.03, 0.004, 0.005, 0.006])
    moves = [(0, 0, 0, 0, 0, 0), (0.9, 0.1, 0.02, 0.3, -1, 0.5), (-0.8, -0.15, -0.03, -0.5, 1, -0.3), (0.1, 0.9, 0.04, 1, 0.2, 0.6),
             (-0.1, -0.85, 0.0, -1, -0.3, -0.4), (0.6, -0.6, -0.05, 0.7, 0.7, 1)]
    poses = [se3.mul(T0, se3.exp([mx * half_w, my * half_h, mz * d, rx * rot, ry * rot, rz * rot])) for mx, my, mz, rx, ry, rz in moves]
    # keyframe 6: close to the surface and tilted -- its z = 0 plane meets the surface inside the cloud
    angle, axis = spec["tilt"]
    ray = np.array([(0.5 * W - cx) / fx, (0.5 * H - cy) / fy, 1.0])      # the image centre's ray: where the base keyframe looks
    foot = ray * d
    near = se3.mul(T0, np.concatenate([[0, 0, 0, 1], foot - np.array([0, 0, spec["height"]])]))
    poses.append(se3.mul(near, _rot(axis, angle)))
    # keyframe 7 looks away
    poses.append(se3.mul(T0, _rot(1, np.pi)))
    return poses


def _planes(name, spec):
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name))))
    front = synthetic.random_planes(rng, 3, offset=spec["distance"], slope=spec["slope"])
    back = np.array([[0.0, 0.0, 1.0, 1.5 * spec["distance"]]])         # z = -1.5 d, facing the keyframe that looks away
    return np.concatenate([front, back])


def hits(pose, planes, camera, u, v):
    """The nearest plane hit of the rays through pixel positions (u, v) (pixel-corner convention) of the camera at global_T_frame
    `pose`, in binary64: (points (3, n) global, plane index (n,), depth (n,); inf / -1 where a ray meets no plane)."""
    fx, fy, cx, cy = [float(c) for c in camera]
    R, o = se3.quat_to_rot(pose[:4]), np.asarray(pose[4:], np.float64)
    u, v = np.atleast_1d(np.asarray(u, np.float64)), np.atleast_1d(np.asarray(v, np.float64))
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)])
    g = R @ dirs
    best, which = np.full(u.shape, np.inf), np.full(u.shape, -1)
    for j, pl in enumerate(planes):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -(pl[:3] @ o + pl[3]) / (pl[:3] @ g)
        ok = (t > 0) & np.isfinite(t) & (t < best)
        best, which = np.where(ok, t, best), np.where(ok, j, which)
    return o[:, None] + g * best, which, best


def _images(spec, planes, poses):
    """Per keyframe the oracle's preprocessing of an (W + 4) x (H + 4) rendering, cropped to W x H: every pixel valid."""
    fx, fy, cx, cy = spec["camera"]
    big = np.array([fx, fy, cx + MARGIN, cy + MARGIN], F32)
    bw, bh = W + 2 * MARGIN, H + 2 * MARGIN
    cam = ob.make_camera(big, bw, bh)
    ba = ob.OracleBA(64, spec["scale"], BASELINE_FX, CELL, cam, ob.make_camera(big, bw, bh))
    crop = (slice(MARGIN, MARGIN + H), slice(MARGIN, MARGIN + W))
    out = []
    for k, pose in enumerate(poses):
        raw, rgb = synthetic.render_planes(pose, planes, big, bw, bh, spec["scale"], invalid_border=False)
        ba.add_keyframe(raw, rgb, pose)
        arrs = ba.kf_arrays(k)
        image = {name: np.ascontiguousarray(arrs[name][crop]) for name in ("depth", "normals", "radius", "color")}
        valid = (image["depth"] & 0x8000) == 0
        assert valid.all(), (k, int((~valid).sum()))
        metres = spec["scale"] * image["depth"].astype(np.float64)
        image["min_depth"], image["max_depth"] = float(F32(metres.min())), float(F32(metres.max()))
        out.append(image)
    return out


def _pack_normal10(n):
    L = ob.lib()
    return np.array([L.orc_pack_normal10(float(a), float(b), float(c)) for a, b, c in np.asarray(n).T], np.uint32).view(F32)


class _Cloud:
    def __init__(self, world):
        self.world, self.columns, self.kinds, self.home = world, [], [], []
        self.rng = np.random.Generator(np.random.PCG64(17))

    def surfels(self, pose, u, v):
        """Surfel columns (17, n) on the planes, on the rays through (u, v) of the keyframe at `pose`; rays that meet nothing are left out."""
        w = self.world
        p, which, depth = hits(pose, w.planes, w.camera, u, v)
        ok = which >= 0
        p, which, depth = p[:, ok], which[ok], depth[ok]
        # up to 0.1 % of its distance off the surface ALONG ITS RAY (2.5 mm at 2.5 m, the size of the displacements the other scenes
        # of the suite work with): the pixel position in this keyframe stays what it was placed at, and the depth residuals are not
        # the rounding of the raw depth alone
        o = np.asarray(pose[4:], np.float64)[:, None]
        p = o + (p - o) * (1.0 + self.rng.uniform(-DISPLACEMENT, DISPLACEMENT, p.shape[1]))
        cols = np.zeros((ob.SURFEL_ATTRS, p.shape[1]), F32)
        cols[:3] = p.astype(F32)
        cols[3] = _pack_normal10(w.planes[which, :3].T)
        cols[4] = ((depth / abs(float(w.camera[0]))) ** 2).astype(F32)                 # a pixel's footprint
        cols[5] = np.full(p.shape[1], 0x80808080, np.uint32).view(F32)
        cols[6] = (3.0 * np.sin(7.0 * p[0] + 3.0 * p[1])).astype(F32)
        cols[7] = (3.0 * np.cos(5.0 * p[1] - 2.0 * p[2])).astype(F32)
        return cols

    def tile(self, cols, kind, home):
        assert 0 <= cols.shape[1] <= 64
        full = np.zeros((ob.SURFEL_ATTRS, 64), F32)
        full[0] = np.nan                                # dead entries: NaN x, as a deletion leaves them
        full[:, :cols.shape[1]] = cols
        self.columns.append(full)
        self.kinds.append(kind)
        self.home.append(home)


def _border_positions(border, along, offset):
    """Pixel position `offset` px inside (negative: outside) `border` (0 left, 1 right, 2 top, 3 bottom) at `along` on it."""
    if border == 0:
        return offset, along
    if border == 1:
        return W - offset, along
    if border == 2:
        return along, offset
    return along, H - offset


def _build_cloud(world):
    cloud = _Cloud(world)
    homes = range(7)                                    # every keyframe but the one that looks away
    centre = (0.5 * W, 0.5 * H)
    for k in homes:
        pose = world.poses[k]
        for border in range(4):
            length = H if border < 2 else W
            # tiles of one live entry: eight places along the border, both corner pixels among them, every offset twice
            places = [0.5, 0.17 * length, 0.31 * length, 0.46 * length, 0.58 * length, 0.72 * length, 0.86 * length, length - 0.5]
            for j, along in enumerate(places):
                u, v = _border_positions(border, along, OFFSETS[(j + border + k) % 4])
                cols = cloud.surfels(pose, [u], [v])
                if cols.shape[1]:
                    cloud.tile(cols, "single", k)
            # tiles of two to five entries: one member half a pixel inside, the others further out on the line from the image centre
            for j, along in enumerate((0.27 * length, 0.66 * length)):
                members = 2 + (j + border + k) % 4
                u, v = _border_positions(border, along, 0.5)
                steps = np.concatenate([[0.0], np.linspace(1.2, 2.0, members - 1)])
                us, vs = u + steps * (u - centre[0]), v + steps * (v - centre[1])
                cols = cloud.surfels(pose, us, vs)
                if cols.shape[1] >= 2:
                    cloud.tile(cols, "outside", k)
        # full compact tiles: 8 x 8 pixel patches over the four corners and the middle of the four borders, pixel centres
        for x0, y0 in ((0, 0), (W - 8, 0), (0, H - 8), (W - 8, H - 8), (W // 2 - 4, 0), (W // 2 - 4, H - 8), (0, H // 2 - 4), (W - 8, H // 2 - 4)):
            gx, gy = np.meshgrid(np.arange(8) + x0 + 0.5, np.arange(8) + y0 + 0.5)
            cols = cloud.surfels(pose, gx.ravel(), gy.ravel())
            if cols.shape[1] == 64:
                cloud.tile(cols, "compact", k)
    # tiles that straddle keyframe 6's z = 0 plane: one member inside its image, the others behind it, so that the centre is behind
    k = 6
    inv = se3.inverse(world.poses[k])
    R6, t6 = se3.quat_to_rot(inv[:4]), inv[4:]
    rng = np.random.Generator(np.random.PCG64(6))
    made = 0
    for attempt in range(600):
        if made == 30:
            break
        u, v = rng.uniform(1, W - 1), rng.uniform(1, H - 1)
        front = cloud.surfels(world.poses[k], [u], [v])
        if not front.shape[1]:
            continue
        members = 2 + attempt % 4
        # partners: surfels placed for another keyframe, the ones furthest behind keyframe 6
        pu, pv = rng.uniform(0, W, 64), rng.uniform(0, H, 64)
        cand = cloud.surfels(world.poses[attempt % 6], pu, pv)
        z = (R6 @ cand[:3].astype(np.float64) + t6[:, None])[2]
        cols = np.concatenate([front, cand[:, np.argsort(z)[:members - 1]]], axis=1)
        box = 0.5 * (cols[:3].astype(np.float64).min(axis=1) + cols[:3].astype(np.float64).max(axis=1))
        depth_of_front = float((R6 @ front[:3, 0].astype(np.float64) + t6)[2])
        if float((R6 @ box + t6)[2]) > -0.1 * depth_of_front:          # the sphere's centre must lie clearly behind the z = 0 plane
            continue
        cloud.tile(cols, "straddle", k)
        made += 1
    # far-apart members whose sphere holds keyframe 0's camera centre: two surfels on the surface and their mirror images
    c = np.asarray(world.poses[0][4:], np.float64)
    pair = cloud.surfels(world.poses[0], [0.2 * W, 0.8 * W], [0.3 * H, 0.6 * H])
    mirror = pair.copy()
    mirror[:3] = (2 * c[:, None] - pair[:3].astype(np.float64)).astype(F32)
    cloud.tile(np.concatenate([pair, mirror], axis=1), "centre", 0)
    cloud.tile(np.zeros((ob.SURFEL_ATTRS, 0), F32), "dead", -1)
    # the ragged last tile: 37 entries of a patch in the middle of keyframe 1's image
    gx, gy = np.meshgrid(np.arange(8) + W // 2 + 0.5, np.arange(8) + H // 2 + 0.5)
    ragged = cloud.surfels(world.poses[1], gx.ravel()[:37], gy.ravel()[:37])
    cloud.tile(ragged, "ragged", 1)
    data = np.concatenate(cloud.columns, axis=1)
    data = data[:, :64 * (len(cloud.columns) - 1) + ragged.shape[1]]
    return data, cloud.kinds, cloud.home


@functools.lru_cache(maxsize=None)
def world(name):
    """The world of camera shape `name` (built once per process; nobody changes it)."""
    w = World()
    w.name, w.spec = name, SHAPES[name]
    w.camera = np.array(w.spec["camera"], F32)
    w.planes = _planes(name, w.spec)
    w.poses = _poses(w.spec)
    w.images = _images(w.spec, w.planes, w.poses)
    w.surfels, w.kinds, w.home = _build_cloud(w)
    w.kinds = np.array(w.kinds)
    w.home = np.array(w.home)
    assert len(w.kinds) <= MAX_TILES and len(w.poses) <= 8
    return w


def build_oracle(w, poses=None, max_surfels=None, use_depth=True, use_desc=True, images=None):
    """A fresh oracle holding the world: the keyframes through add_preprocessed_keyframe, the cloud, every surfel and keyframe active.
    poses / images: other keyframes than the world's eight (one image set per pose)."""
    cam = lambda: ob.make_camera(w.camera, W, H)        # noqa: E731
    n = w.surfels.shape[1]
    ba = ob.OracleBA(max_surfels or n + 64, w.spec["scale"], BASELINE_FX, CELL, cam(), cam(), use_depth_residuals=use_depth,
                     use_descriptor_residuals=use_desc)
    for k, image in enumerate(images or w.images):
        ba.add_preprocessed_keyframe(image["depth"], image["normals"], image["radius"], image["color"], (poses or w.poses)[k],
                                     image["min_depth"], image["max_depth"])
    ba.surfel_data[:, :n] = w.surfels
    ba.surfels.surfels_size = n
    ba.surfels.surfel_count = int((w.surfels[0] == w.surfels[0]).sum())
    ba.active[:n] = 1
    return ba


def frames_of(ba):
    return np.array([list(kf.frame_T_global) for kf in ba.keyframes], F32)


def build_gpu(w, ba=None, arithmetic="exact", poses=None, capacity=None, images=None):
    """The world on the backend: the keyframes' buffers filled with the very images the oracle holds (uploaded, as
    tests/test_gpu_golden_reference.py does), and with `ba` the oracle's surfels, flags, poses and intrinsics copied over and bound."""
    from badslam_amd import lowlevel as ll
    from tests import two_cameras
    ctx = ll.Context()
    ctx.set_arithmetic(arithmetic)
    g = ll.Scene(ctx, capacity or w.surfels.shape[1] + 64, w.spec["scale"], BASELINE_FX, CELL, ll.make_camera(w.camera, W, H),
                 ll.make_camera(w.camera, W, H))
    blank_depth, blank_rgb = np.full((H, W), 65535, np.uint16), np.zeros((H, W, 3), np.uint8)
    if images is None:
        images = w.images if poses is None else [w.images[0]] * len(poses)
    for k, image in enumerate(images):
        g.add_keyframe(blank_depth, blank_rgb, (poses or w.poses)[k])
        kf = g.keyframes[k]
        for name in ("depth", "normals", "radius", "color"):
            kf[name].upload(image[name])
        kf["min_depth"], kf["max_depth"] = image["min_depth"], image["max_depth"]
    if ba is not None:
        two_cameras.sync_gpu(g, ba)
    else:
        g.bind_keyframes()
    return g


# ---- what the oracle says about the pairs ----------------------------------------------------------------------------------------------
class Pairs:
    """Per (keyframe, surfel) of a world, from the oracle: associated, px, py (evaluate_pairs) and in_image -- the pair's position has
    z > 0 and lies in the image (pair_pixel_positions: the position orc_project_associate computes, zeros where z <= 0)."""


@functools.lru_cache(maxsize=None)
def pairs(name):
    w = world(name)
    ba = build_oracle(w)
    n, K = w.surfels.shape[1], len(w.poses)
    live = np.flatnonzero(w.surfels[0] == w.surfels[0]).astype(np.uint32)
    p = Pairs()
    p.associated, p.in_image = np.zeros((K, n), bool), np.zeros((K, n), bool)
    p.px, p.py = np.full((K, n), -1), np.full((K, n), -1)
    for k in range(K):
        words = ba.evaluate_pairs(k, live).view(np.int32)
        p.associated[k, live] = words[:, 0] == 1
        p.px[k, live], p.py[k, live] = words[:, 1], words[:, 2]
        xy = ba.pair_pixel_positions(k, live)
        p.in_image[k, live] = ((xy[:, 0] != 0) | (xy[:, 1] != 0)) & (xy[:, 0] >= 0) & (xy[:, 1] >= 0) & (xy[:, 0] < W) & (xy[:, 1] < H)
    assert not (p.associated & ~p.in_image).any()
    p.frames = frames_of(ba)
    return p


def per_tile(flags):
    """(K, N) per-surfel flags -> (T, K): any entry of the tile."""
    K, n = flags.shape
    t = (n + 63) // 64
    padded = np.zeros((K, t * 64), bool)
    padded[:, :n] = flags
    return padded.reshape(K, t, 64).any(axis=2).T


def census(name):
    """What the GPU tests rest on, per camera shape (tests/test_cpu_tile_cull.py::test_census asserts the least of each that the GPU tests need)."""
    w, p = world(name), pairs(name)
    bounds = wave_bounds32(w.surfels[:3])
    may, first = sphere_may_project(F32, w.camera, p.frames, bounds)
    a = p.associated
    outer = a & ((p.px == 0) | (p.px == W - 1) | (p.py == 0) | (p.py == H - 1))
    tile_associated = per_tile(a)
    live_tiles = bounds[:, 3] >= 0
    out = dict(tiles=len(w.kinds), surfels=int(w.surfels.shape[1]), live=int((w.surfels[0] == w.surfels[0]).sum()), associated=int(a.sum()),
               outer=int(outer.sum()),
               sides=[int((a & (p.px == 0)).sum()), int((a & (p.px == W - 1)).sum()), int((a & (p.py == 0)).sum()), int((a & (p.py == H - 1)).sum())],
               corners=[int((a & (p.px == x) & (p.py == y)).sum()) for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))],
               single_associated=int(tile_associated[w.kinds == "single"].any(axis=1).sum()),
               first=[int((first[live_tiles] == q).sum()) for q in range(5)],
               culled_share=float((~may[live_tiles]).mean()),
               straddle=int((tile_associated[:, 6] & (w.kinds == "straddle")).sum()),
               mutants={})
    for mutant in MUTANTS:
        lost, _ = sphere_may_project(F32, w.camera, p.frames, bounds, mutant)
        out["mutants"][mutant] = int((~lost & tile_associated).sum())
    return out
