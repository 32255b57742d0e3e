"""The plain model of a rendered view of the surfel map (bahip_render_surfels; DESIGN.md section 3, "Rendered views of the map"): the
definition in numpy binary32, operation for operation, vectorised per surfel and per candidate offset -- no GPU, no oracle.  The GPU
tests (tests/test_gpu_render_view.py) hold the kernels to it bit for bit; tests/test_cpu_render_view.py holds it to the oracle and to
hand-made cases.  A plain module: no fixtures, no conftest.

numpy has no fused multiply-add: fma() below computes a * b exactly in binary64 (24 x 24 bits), adds c with the rounding error of that
sum known (TwoSum), rounds the binary64 sum to odd and then to binary32 -- the correctly rounded fma for every finite operand whose
product and sum stay inside binary64's normal range (53 >= 2 x 24 + 2 bits: the classical double-rounding argument)."""
from types import SimpleNamespace

import numpy as np

F = np.float32
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
EMPTY_INDEX = np.uint32(0xFFFFFFFF)
PLANES = ("key", "depth", "index", "normal", "color")
POINT, DISC = 0, 1


def options(mode=DISC, max_radius_px=4, cull_backfaces=1, radius_factor=1.0, min_depth=0.0, max_depth=float("inf"), index_base=0):
    """The fields of bahip_render_options (capi.RenderOptions has the same names and defaults)."""
    return SimpleNamespace(mode=int(mode), max_radius_px=int(max_radius_px), cull_backfaces=int(cull_backfaces), radius_factor=radius_factor,
                           min_depth=min_depth, max_depth=max_depth, index_base=int(index_base))


def fma(a, b, c):
    """fmaf(a, b, c) on binary32 arrays."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (np.asarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        odd = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return odd.astype(F)


def _finite(v):
    return (np.asarray(v, F).view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)


def unpack_normal10(bits):
    """ba_device.h: unpack_normal10 (decoded and renormalised), (3, N) binary32."""
    bits = np.asarray(bits, np.uint32)

    def ten(v):
        return ((v << np.uint32(22)).view(np.int32) >> 22).astype(F) * (F(1) / F(511))
    n = [ten(bits), ten(bits >> np.uint32(10)), ten(bits >> np.uint32(20))]
    with np.errstate(divide="ignore", invalid="ignore"):
        factor = F(1) / np.sqrt(fma(n[2], n[2], fma(n[1], n[1], n[0] * n[0])))
        return np.stack([factor * n[0], factor * n[1], factor * n[2]])


def pack_normal10(n):
    """ba_device.h: pack_normal10 of one unit vector (for hand-made surfels)."""
    def ten(v):
        return int(np.trunc(F(v) * F(511) + (F(0.5) if v > 0 else F(-0.5)))) & 0x3ff
    return np.uint32(ten(n[0]) | (ten(n[1]) << 10) | (ten(n[2]) << 20))


def camera(params, width, height):
    """A view camera: fx, fy, cx, cy (pixel-corner convention), width, height -- from a 4-vector or any object with those attributes."""
    if hasattr(params, "fx"):
        return SimpleNamespace(fx=F(params.fx), fy=F(params.fy), cx=F(params.cx), cy=F(params.cy), width=int(params.width), height=int(params.height))
    p = np.asarray(params, F)
    return SimpleNamespace(fx=p[0], fy=p[1], cx=p[2], cy=p[3], width=int(width), height=int(height))


def render(surfels, cam, frame_T_global, opt=None):
    """The definition.  surfels: (>= 6, N) binary32 rows (position, packed normal, r^2, colour word); cam: camera(); frame_T_global: 12
    floats; opt: options().  Returns a dict of the five planes (key uint64, depth float32, index uint32: (h, w); normal float32 (h, w,
    3); color uint8 (h, w, 4)) and `stats`: candidates (h, w) keyed candidates per pixel, tie (h, w) more than one candidate at the
    winning depth, tests (candidate tests in all), keyed (candidates that contributed a key), and surfels by reason: behind_or_outside (finite, and
    local.z <= 0 or no candidate pixel inside the image), backface (in front, nd >= 0 under culling), disc_miss (at least one candidate
    pixel failed the disc test)."""
    opt = opt or options()
    data = np.ascontiguousarray(np.asarray(surfels, F)[:6])
    N = data.shape[1]
    Fm = np.asarray(frame_T_global, F)
    w, h = cam.width, cam.height
    fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    fx_inv, fy_inv = F(1) / fx, F(1) / fy
    cx_inv, cy_inv = -(cx - F(0.5)) * fx_inv, -(cy - F(0.5)) * fy_inv
    cull, disc = bool(opt.cull_backfaces), opt.mode == DISC
    x, y, z = data[0], data[1], data[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        gn = unpack_normal10(data[3].view(np.uint32))
        lz = fma(Fm[10], z, fma(Fm[9], y, fma(Fm[8], x, Fm[11])))
        lx = fma(Fm[2], z, fma(Fm[1], y, fma(Fm[0], x, Fm[3])))
        ly = fma(Fm[6], z, fma(Fm[5], y, fma(Fm[4], x, Fm[7])))
        nl = np.stack([fma(Fm[2], gn[2], fma(Fm[1], gn[1], Fm[0] * gn[0])),
                       fma(Fm[6], gn[2], fma(Fm[5], gn[1], Fm[4] * gn[0])),
                       fma(Fm[10], gn[2], fma(Fm[9], gn[1], Fm[8] * gn[0]))])
        nd = fma(nl[1], ly, fma(nl[0], lx, nl[2] * lz))
        inv_z = F(1) / lz
        pxx, pxy = fma(fx, lx * inv_z, cx), fma(fy, ly * inv_z, cy)
        finite = _finite(x) & _finite(y) & _finite(z)
        in_front = finite & (lz > 0)
        facing = in_front & ((nd < 0) if cull else True)
        ok = facing & (np.abs(pxx) < F(1e6)) & (np.abs(pxy) < F(1e6))
        half = np.zeros(N, np.int64)
        rs2 = np.zeros(N, F)
        if disc:
            r2 = data[4]
            ok &= _finite(r2) & (r2 > 0)
            rs2 = (F(opt.radius_factor) * F(opt.radius_factor)) * r2
            hf = (max(fx, fy) * np.sqrt(np.where(ok, rs2, F(0)))) * inv_z
            small = ok & (hf < F(opt.max_radius_px))
            half = np.where(small, np.minimum(opt.max_radius_px, np.where(small, hf, 0).astype(np.int64) + 1), opt.max_radius_px)
        px = np.floor(np.where(ok, pxx, F(0))).astype(np.int64)
        py = np.floor(np.where(ok, pxy, F(0))).astype(np.int64)
    index = np.arange(N, dtype=np.uint64) + np.uint64(opt.index_base)
    min_depth, max_depth = F(opt.min_depth), F(opt.max_depth)
    all_pix, all_key = [], []
    tests = 0
    tested = np.zeros(N, bool)
    missed = np.zeros(N, bool)
    reach = opt.max_radius_px if disc else 0
    for oy in range(-reach, reach + 1):
        for ox in range(-reach, reach + 1):
            ring = max(abs(ox), abs(oy))
            X, Y = px + ox, py + oy
            sel = np.flatnonzero(ok & (half >= ring) & (X >= 0) & (X < w) & (Y >= 0) & (Y < h))
            if sel.size == 0:
                continue
            tests += sel.size
            tested[sel] = True
            X, Y = X[sel], Y[sel]
            t = lz[sel]
            keep = np.ones(sel.size, bool)
            if disc:
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    dx, dy = fma(fx_inv, X.astype(F), cx_inv), fma(fy_inv, Y.astype(F), cy_inv)
                    den = fma(nl[1][sel], dy, fma(nl[0][sel], dx, nl[2][sel]))
                    t = nd[sel] / den
                    keep = (den < 0) if cull else (t > 0)
                    qx, qy, qz = t * dx - lx[sel], t * dy - ly[sel], t - lz[sel]
                    inside = fma(qz, qz, fma(qy, qy, qx * qx)) <= rs2[sel]
                missed[sel[keep & ~inside]] = True
                keep &= inside
            with np.errstate(invalid="ignore"):
                keep &= (t >= min_depth) & (t <= max_depth)
            all_pix.append((Y * w + X)[keep])
            all_key.append((np.asarray(t, F).view(np.uint32).astype(np.uint64)[keep] << np.uint64(32)) | index[sel][keep])
    pix = np.concatenate(all_pix) if all_pix else np.zeros(0, np.int64)
    keys = np.concatenate(all_key) if all_key else np.zeros(0, np.uint64)
    key = np.full(w * h, EMPTY_KEY, np.uint64)
    np.minimum.at(key, pix, keys)
    candidates = np.bincount(pix, minlength=w * h)
    at_winning_depth = (keys >> np.uint64(32)) == (key[pix] >> np.uint64(32))
    tie = np.bincount(pix[at_winning_depth], minlength=w * h) > 1
    covered = key != EMPTY_KEY
    winner = np.where(covered, (key & np.uint64(0xFFFFFFFF)) - np.uint64(opt.index_base), 0).astype(np.int64)
    depth = np.where(covered, (key >> np.uint64(32)).astype(np.uint32), np.uint32(0)).astype(np.uint32).view(F)
    normal = np.where(covered[:, None], nl[:, winner].T, F(0)).astype(F) if N else np.zeros((w * h, 3), F)
    color = np.where(covered, data[5].view(np.uint32)[winner], np.uint32(0)).astype(np.uint32) if N else np.zeros(w * h, np.uint32)
    stats = dict(candidates=candidates.reshape(h, w), tie=tie.reshape(h, w), tests=int(tests), keyed=int(keys.size),
                 behind_or_outside=int(np.count_nonzero((finite & ~in_front) | (ok & ~tested))),
                 backface=int(np.count_nonzero(in_front & ~facing)), disc_miss=int(np.count_nonzero(missed)))
    return dict(key=key.reshape(h, w), depth=depth.reshape(h, w), index=np.where(covered, key & np.uint64(0xFFFFFFFF), EMPTY_INDEX).astype(np.uint32).reshape(h, w),
                normal=normal.reshape(h, w, 3), color=color.view(np.uint8).reshape(h, w, 4), stats=stats)


def bits(plane):
    """A plane as unsigned words (binary32 planes by their bit patterns: +0.0 is not -0.0, NaN equals NaN)."""
    a = np.ascontiguousarray(plane)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_planes(got, expected, what=""):
    """Every plane of `got` equals the model's bit for bit, no pixel left out; names the first pixels that differ."""
    names = [n for n in PLANES if n in got]
    assert names and set(names) == {n for n in got if n != "stats" and n != "frame_T_global"}, (what, sorted(got))
    for name in names:
        a, b = bits(got[name]), bits(expected[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, len(bad), [(tuple(int(v) for v in p), got[name][tuple(p)], expected[name][tuple(p)]) for p in bad[:5]])


# ---- loaders ----------------------------------------------------------------------------------------------------------------------------
def oracle_surfels(ba):
    """The oracle's surfel rows [0, surfels_size), a copy."""
    return ba.surfel_data[:8, :ba.surfels_size].copy()


def oracle_frame(ba, k):
    """frame_T_global (12 binary32) of the oracle's keyframe k at its current pose."""
    return np.array(list(ba.keyframes[k].frame_T_global), F)


def pose_frame(global_T_frame):
    """frame_T_global (12 binary32) of a pose given as the 7 floats qx, qy, qz, qw, tx, ty, tz: the oracle's own inverse and matrix."""
    from oracle import binding as ob
    T = ob.SE3.from_array(global_T_frame)
    return ob.se3_matrix3x4(ob.se3_inverse(T))


def disc_surfel(position, normal, radius, color=0xff8040c0):
    """One hand-made surfel column (8 rows)."""
    col = np.zeros(8, F)
    col[:3] = position
    col[3:4] = np.array([pack_normal10(np.asarray(normal, np.float64) / np.linalg.norm(normal))], np.uint32).view(F)
    col[4] = F(radius) * F(radius)
    col[5:6] = np.array([color], np.uint32).view(F)
    return col


IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def turned_frame(frame_T_global, yaw_degrees, shift=(0.0, 0.0, 0.0)):
    """Another view of the same cloud: the camera frame of `frame_T_global` turned about its y axis and shifted -- local' = R_y local +
    shift (binary64, rounded once: any 12 floats are a valid frame for both the model and the kernels)."""
    a = np.deg2rad(yaw_degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    M = R @ np.asarray(frame_T_global, np.float64).reshape(3, 4)
    M[:, 3] += np.asarray(shift, np.float64)
    return M.reshape(12).astype(F)


def scaled_camera(cam, width, height):
    """The camera `cam` resampled to width x height pixels (the same field of view)."""
    sx, sy = width / cam.width, height / cam.height
    return camera([cam.fx * sx, cam.fy * sy, cam.cx * sx, cam.cy * sy], width, height)
