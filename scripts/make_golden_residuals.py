#!/usr/bin/env python3
"""Generates tests/golden/composed_residuals.npz: the whole per-pair chain of the bundle adjustment -- projection and association,
depth calibration, depth residual with its inverse standard deviation, depth-to-colour map, three bilinear luma samples, descriptor
residuals, robust weights, pose Jacobians -- evaluated with 60-digit sympy floats on four small scenes of fully specified images.
tests/composed_residuals.py loads the file; tests/test_cpu_composed_residuals.py holds the oracle and the reference's own functions
to it, tests/test_gpu_composed_residuals.py the HIP kernels in both arithmetic flavours (bahip_debug_evaluate_pairs).

Like scripts/make_golden_jacobians.py this script IMPORTS applications/badslam/scripts/jacobians_derivation.py from the reference
tree at generation time (BADSLAM_REFERENCE_SCRIPTS names its directory; the fixture is committed because the tree is not everywhere)
and calls its functions wherever it defines the piece: CorrectDepth, Unproject, Project, SE3exp, SE3Inverse,
MatrixVectorMultiplyHomogeneous, DotProduct3, InterpolateBilinear.  What the script does not define is restated below in sympy from
the reference's formulas, each with its source (B/ = applications/badslam/src/badslam/).  Constants written with an `f` suffix there
(0.1f, 1e-2f, 0.9f, 1e-12f, 0.76604f) enter with their binary32 value.

Scenes (one frame each; the images go into the keyframes as they are, preprocessing is not part of the chain):

  scene  depth image  sparse cell  colour image and camera
  0      64x48        2            64x48, the depth camera's
  1      64x48        4            53x38, its own focal lengths and principal point
  2      64x46        4            53x38, the same colour camera (46 is no multiple of 4: the last cfactor row is a partial cell)
  3      70x45        3            97x71, larger than the depth image

Every configuration is one (surfel, frame) pair, evaluated at `a` = 0 or at the scene's own `a`.  Stored per configuration: the
decisions (associated, the reason if not, colour pixel valid), the expected value `want` of every word of the hook's 40-float record
(layout above evaluate_pairs_kernel in kernels_pose.hip), and for every float word a scale:

  scale_issue[q] = sum over the binary32 inputs of |q(input * (1 + 2^-24)) - q| / 2^-24, one input at a time, decisions frozen.
                   Inputs: 3 surfel coordinates, 12 entries of frame_T_global, 4 + 4 camera parameters, a, the pixel's cfactor,
                   raw_to_float_depth, baseline_fx, the squared radius, the two descriptors.  Integers (raw depth, texels, normal
                   codes) are not perturbed.
  scale[q]       = scale_issue[q]
                   + the same sum over the 24 normalised texel values (texel / 255, a binary32 number in every implementation) of
                     the three value footprints and the three gradient footprints
                   + |q| (q itself is stored as a binary32 number).
                   Both additions are roundings no input of the first list stands for: a descriptor residual 180 (I1 - I0) - d
                   with a small d and a flat image has scale_issue ~ |d|, while I0 and I1 carry 2^-24 * 0.5 each, 180 times; a
                   Tukey weight (1 - (r / 10)^2)^2 at a small r has scale_issue ~ 0 while its own rounding is 2^-25.  The CPU test
                   prints the measured ratios against both scales.

Pose Jacobians are central differences with h = 1e-20 through the script's SE3exp, composed as the reference's kernels compose them
(B/kernel_opt_pose.cu:45-142), NOT as the derivative of the idealised chain:
  depth       inv_stddev * d/dT DotProduct3(nl, SE3exp(T) * u - ls)            nl, ls, inv_stddev held fixed
  descriptor  g . d/dT Project(SE3Inverse(SE3exp(T)) * ls, cfx, cfy, ., .)      ONE projection Jacobian, at the surfel centre ls,
              applied to g = 180 (gradient at the tangent sample - gradient at the centre sample), B/cost_function.cuh:245-253;
              the idealised chain would move each of the three samples by its own projection Jacobian.  Where the two differ the
              golden is the reference's composition.

Margin rules: a configuration is stored only if, at 60 digits, every pixel coordinate (depth pixel, colour pixel) is further than
1e-3 px from an integer, every colour sample further than 1e-3 px from a texel boundary (x - 0.5 from an integer), and every
inequality (z > 0 relative to |p|, the depth-difference threshold, the facing test as a cosine, the normal compatibility, the
|n.x| > 0.9 axis choice, both robust-weight thresholds, |n . (nx, ny, 1)| > 0) holds or fails with relative slack >= 1e-3.  Draws
that miss a margin or land in another category than the one drawn for are rejected and counted (`rejected` in the file).

The depth weight's zero branch (|r| >= 10) IS reachable under the association threshold |z - depth| <= 10 sigma: the residual is
n . (u - ls) / sigma, and besides (depth - z) n . (nx, ny, 1) it holds z (n.x dx / fx + n.y dy / fy) for the surfel's offset
(dx, dy) from the pixel centre, which is of the order of sigma on these small images.  The category `tukey_zero` holds such cases.

Run:  python scripts/make_golden_residuals.py     (needs the reference tree and sympy; 8 worker processes)
Run time: about 1 minute on 8 cores (4 minutes of CPU time; a 60-digit chain evaluation takes 10-20 ms, a configuration 55 of
them).  The output is byte-for-byte reproducible from SEED (fixed zip timestamps).
"""
import io
import multiprocessing
import os
import sys
import time
import zipfile

import numpy as np
import sympy
import sympy.printing.cxx as _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.modules.setdefault("sympy.printing.cxxcode", _cxx)             # sympy >= 1.10 renamed the module the script imports
REF_SCRIPTS = os.environ.get("BADSLAM_REFERENCE_SCRIPTS", "/root/reference/applications/badslam/scripts")   # as make_golden_jacobians.py
sys.path.insert(0, REF_SCRIPTS)
import jacobians_derivation as ref                                 # noqa: E402  (the reference, imported - not copied)

ref.frac = lambda v: v - sympy.floor(v)                            # the script leaves frac() unevaluated; numerically x - floor(x)

SEED = 20241019
PREC = 60
OUT = os.path.join(ROOT, "tests", "golden", "composed_residuals.npz")
MARGIN = 1e-3
REASONS = ("associated", "z", "outside", "invalid_depth", "depth_difference", "facing_away", "normals")
KINDS = ("interior_zero", "interior_cal", "clamp", "colour_invalid", "border", "huber", "tukey_zero") + REASONS[1:]
# words of the hook's record that hold a float quantity, by group (tests/composed_residuals.py: GROUPS)
W_PXX, W_DEPTH, W_R, W_W, W_ISTD, W_JD, W_DR, W_DW, W_J1, W_J2, W_G = 34, 4, 5, 6, 7, 8, 14, 16, 18, 24, 30


def Fl(x):
    return sympy.Float(float(x), PREC)                             # exact: a binary32 / binary64 value fits 203 bits


def c32(x):
    return Fl(np.float32(x))


H_STEP = sympy.Float("1e-20", PREC)
HALF, ONE, ZERO = Fl(0.5), Fl(1), Fl(0)
K01, K001, K09, K1E12, KCOS, K10, K180 = c32(0.1), c32(1e-2), c32(0.9), c32(1e-12), c32(0.76604), Fl(10), Fl(180)


def _exp_steps():
    """SE3exp(+-h e_k) and their inverses, k = 0..5: constants of every central difference."""
    plus, minus = [], []
    for k in range(6):
        for sign, dst in ((1, plus), (-1, minus)):
            T = [ZERO] * 6
            T[k] = sign * H_STEP
            M = ref.SE3exp(sympy.Matrix(T))
            dst.append((M, ref.SE3Inverse(M)))
    return plus, minus


EXP_PLUS, EXP_MINUS = _exp_steps()


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def random_rigid(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    return R, rng.uniform(-1, 1, 3)


def make_scene(rng, W, H, cell, dcam, cw, ch, ccam, a, bfx, angle):
    y, x = np.mgrid[0:H, 0:W]
    s = np.float32(0.0002)
    z = 1.7 + 0.006 * (x - W / 2) + 0.004 * (y - H / 2) + 0.03 * np.sin(x / 7.0) * np.cos(y / 5.0) + rng.normal(scale=0.002, size=(H, W))
    depth = np.round(z / float(s)).astype(np.uint16)
    invalid = rng.uniform(size=(H, W)) < 0.08
    depth[invalid] |= 0x8000
    nx, ny = rng.integers(-28, 29, (H, W)), rng.integers(-28, 29, (H, W))
    normals = ((nx & 0xff) | ((ny & 0xff) << 8)).astype(np.uint16)
    yy, xx = np.mgrid[0:ch, 0:cw]
    luma = np.clip(128 + 60 * np.sin(xx / 2.3) + 45 * np.cos(yy / 1.9) + rng.normal(scale=12, size=(ch, cw)), 0, 255).astype(np.uint8)
    cf_w, cf_h = (W - 1) // cell + 1, (H - 1) // cell + 1
    cfactor = rng.uniform(-4e-3, 4e-3, (cf_h, cf_w)).astype(np.float32)
    cfactor[:, :cf_w // 3] = 0                                   # the cells where a = 0 = cfactor configurations are drawn
    R, t = random_rigid(rng, angle)                              # global_T_frame
    F = np.hstack([R.T, (-R.T @ t)[:, None]]).astype(np.float32)  # frame_T_global as handed to the hook
    return dict(W=W, H=H, cell=cell, dcam=np.asarray(dcam, np.float32), cw=cw, ch=ch, ccam=np.asarray(ccam, np.float32),
                a=np.float32(a), s=s, bfx=np.float32(bfx), depth=depth, normals=normals, luma=luma, cfactor=cfactor, F=F.reshape(12))


def make_scenes(rng):
    d0 = (58.5, 57.25, 31.7, 23.6)
    return [make_scene(rng, 64, 48, 2, d0, 64, 48, d0, 0.05, 160.0, 0.4),
            make_scene(rng, 64, 48, 4, d0, 53, 38, (46.2, 47.9, 21.0, 18.4), -0.03, 240.0, 0.7),
            make_scene(rng, 64, 46, 4, (58.5, 57.25, 31.7, 22.6), 53, 38, (46.2, 47.9, 21.0, 18.4), 0.04, 240.0, 1.1),
            make_scene(rng, 70, 45, 3, (61.0, 59.5, 34.6, 22.9), 97, 71, (80.0, 83.0, 41.0, 35.2), 0.02, 200.0, 0.9)]


# ---- float64 design of a draw (only proposes inputs; every decision is taken at 60 digits below) -----------------------------------
def signed_byte(v):
    v &= 0xff
    return v - 256 if v & 0x80 else v


def decode8(code):
    x = signed_byte(code) / 127.0
    y = signed_byte(code >> 8) / 127.0
    return np.array([x, y, -np.sqrt(max(0.0, 1 - x * x - y * y))])


def pack10(n):
    v = np.clip(np.round(np.asarray(n) * 511.0), -511, 511).astype(np.int64) & 0x3ff
    return int(v[0] | (v[1] << 10) | (v[2] << 20))


def rotate_towards(rng, m, degrees):
    """m turned by `degrees` about a random axis perpendicular to it."""
    p = np.cross(m, rng.normal(size=3))
    p /= np.linalg.norm(p)
    ang = np.radians(degrees)
    return np.cos(ang) * m + np.sin(ang) * np.cross(p, m)


def colour_pixel(sc, pxx, pxy):
    fx, fy, cx, cy = sc["dcam"].astype(np.float64)
    cfx, cfy, ccx, ccy = sc["ccam"].astype(np.float64)
    return cfx / fx * (pxx - cx) + ccx, cfy / fy * (pxy - cy) + ccy


def design_descriptors(sc, gp, bits, r2, centre):
    """180 (I(t) - I(c)) of the two tangent samples in float64 (clamp-addressed bilinear luma)."""
    f = [(bits >> sh) & 0x3ff for sh in (0, 10, 20)]
    n = np.array([v - 1024 if v & 0x200 else v for v in f], np.float64)
    n /= np.linalg.norm(n)
    F = sc["F"].astype(np.float64).reshape(3, 4)
    cfx, cfy, ccx, ccy = sc["ccam"].astype(np.float64)
    luma = sc["luma"].astype(np.float64) / 255.0

    def sample(x, y):
        xb, yb = x - 0.5, y - 0.5
        i, j = int(np.floor(xb)), int(np.floor(yb))
        al, be = xb - i, yb - j
        cx_ = lambda v: min(max(v, 0), sc["cw"] - 1)
        cy_ = lambda v: min(max(v, 0), sc["ch"] - 1)
        top = (1 - al) * luma[cy_(j), cx_(i)] + al * luma[cy_(j), cx_(i + 1)]
        bot = (1 - al) * luma[cy_(j + 1), cx_(i)] + al * luma[cy_(j + 1), cx_(i + 1)]
        return (1 - be) * top + be * bot
    i0 = sample(*centre)
    t = np.cross(n, [0.0, 1.0, 0.0] if abs(n[0]) > 0.9 else [1.0, 0.0, 0.0])
    out = []
    for _ in range(2):
        t = t * 2 * np.sqrt(r2 / max(1e-12, t @ t))
        l = F[:, :3] @ (gp + t) + F[:, 3]
        with np.errstate(all="ignore"):
            x, y = cfx * l[0] / l[2] + ccx, cfy * l[1] / l[2] + ccy
        ok = np.isfinite(x) and np.isfinite(y) and abs(x) < 1e4 and abs(y) < 1e4
        out.append(180 * (sample(x, y) - i0) if ok else 0.0)
        t = np.cross(n, t)
    return np.array(out)


def draw(sc, kind, rng, side=0):
    W, H, cell = sc["W"], sc["H"], sc["cell"]
    fx, fy, cx, cy = sc["dcam"].astype(np.float64)
    cfx = float(sc["ccam"][0])
    valid = (sc["depth"] & 0x8000) == 0
    zero_cf = sc["cfactor"][np.arange(H)[:, None] // cell, np.arange(W)[None, :] // cell] == 0
    a = np.float32(0.0) if kind == "interior_zero" or (kind != "interior_cal" and rng.uniform() < 0.3) else sc["a"]
    for _ in range(1000):
        px, py = int(rng.integers(0, W)), int(rng.integers(0, H))
        if kind == "border":
            px, py = [(0, py), (W - 1, py), (px, 0), (px, H - 1)][side]
        ox, oy = rng.uniform(0.03, 0.97, 2)
        ccx_, ccy_ = colour_pixel(sc, px + ox, py + oy)
        cvalid = 0 <= ccx_ < sc["cw"] and 0 <= ccy_ < sc["ch"]
        edge = min(ccx_, ccy_, sc["cw"] - ccx_, sc["ch"] - ccy_)
        if kind == "invalid_depth":
            ok = not valid[py, px]
        elif kind == "colour_invalid":
            ok = valid[py, px] and not cvalid
        elif kind == "clamp":
            ok = valid[py, px] and cvalid and edge < 1.2
        elif kind == "interior_zero":
            ok = valid[py, px] and cvalid and edge > 5 and zero_cf[py, px]
        elif kind == "interior_cal":
            ok = valid[py, px] and cvalid and edge > 5 and not zero_cf[py, px]
        elif kind in ("z", "outside"):
            ok = True
        elif kind == "border":
            ok = valid[py, px] and cvalid
        else:
            ok = valid[py, px] and cvalid and edge > 5
        if ok:
            break
    else:
        return None
    raw = int(sc["depth"][py, px] & 0x7fff)
    inv_depth = 1.0 / (float(sc["s"]) * raw)
    depth = 1.0 / (inv_depth + float(sc["cfactor"][py // cell, px // cell]) * np.exp(-float(a) * inv_depth))
    m = decode8(int(sc["normals"][py, px]))
    nl = rotate_towards(rng, m, rng.uniform(2, 25))
    if kind == "facing_away":
        nl = -nl
    elif kind == "normals":
        for _ in range(100):
            nl = rotate_towards(rng, m, rng.uniform(45, 70))
            if nl @ np.array([(px + ox - cx) / fx, (py + oy - cy) / fy, 1.0]) < -0.15:
                break
    nxy1 = np.array([(px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1.0])
    sigma = 0.1 * abs(nl @ nxy1) * depth * depth / float(sc["bfx"])
    if kind == "depth_difference":
        z = depth + rng.choice([-1, 1]) * rng.uniform(1.3, 4.0) * 10 * sigma
    elif kind == "tukey_zero":
        # push n . (u - ls) beyond 10 sigma: nearly the whole depth allowance, and the pixel-offset term with the same sign
        sign = rng.choice([-1, 1])
        nl = rotate_towards(rng, m, rng.uniform(25, 38))
        ox = 0.5 - sign * np.sign(nl[0]) * rng.uniform(0.3, 0.47)
        oy = 0.5 - sign * np.sign(nl[1]) * rng.uniform(0.3, 0.47)
        sigma = 0.1 * abs(nl @ nxy1) * depth * depth / float(sc["bfx"])
        z = depth - sign * np.sign(nl @ nxy1) * rng.uniform(0.93, 0.995) * 10 * sigma
    else:
        z = depth + rng.uniform(-0.75, 0.75) * 10 * sigma
    pxx, pxy = px + ox, py + oy
    if kind == "outside":
        side = int(rng.integers(0, 4))
        pxx, pxy = [(-rng.uniform(0.2, 6), pxy), (W + rng.uniform(0.2, 6), pxy), (pxx, -rng.uniform(0.2, 6)), (pxx, H + rng.uniform(0.2, 6))][side]
    local = np.array([z * (pxx - cx) / fx, z * (pxy - cy) / fy, z])
    if kind == "z":
        local = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), -rng.uniform(0.3, 2.0)])
    F = sc["F"].astype(np.float64).reshape(3, 4)
    R = F[:, :3]
    gp = (R.T @ (local - F[:, 3])).astype(np.float32)
    bits = pack10(R.T @ nl)
    tangent_px = rng.uniform(0.7, 1.5) if kind in ("clamp", "border") else rng.uniform(0.4, 2.0)
    radius = 0.5 * tangent_px * abs(z) / cfx
    r2 = np.float32(radius * radius)
    # descriptors a few units off what the image gives, so that the residuals stay below the Huber parameter unless asked for
    res = rng.uniform(-6, 6, 2)
    if kind == "huber":
        res[int(rng.integers(0, 2))] = rng.choice([-1, 1]) * rng.uniform(13, 40)
    d = design_descriptors(sc, gp.astype(np.float64), bits, float(r2), colour_pixel(sc, pxx, pxy)) - res
    return dict(gp=gp, normal_bits=np.uint32(bits), r2=r2, d=d.astype(np.float32), a=a)


# ---- the chain at 60 digits -------------------------------------------------------------------------------------------------------
class Unusable(Exception):
    pass


def unpack_normal10(bits):
    """B/util_nvcc_only.cuh:66-95: three signed 10-bit fields / 511, renormalised."""
    v = []
    for shift in (0, 10, 20):
        f = (bits >> shift) & 0x3ff
        v.append(Fl(f - 1024 if f & 0x200 else f) / 511)
    norm = sympy.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return sympy.Matrix([[c / norm] for c in v])


def unpack_normal8(code):
    """B/util.cuh:138-146: two signed bytes / 127, z = -sqrt(max(0, 1 - x^2 - y^2))."""
    x = Fl(signed_byte(code)) / 127
    y = Fl(signed_byte(code >> 8)) / 127
    zz = 1 - x * x - y * y
    return sympy.Matrix([[x], [y], [-sympy.sqrt(zz if zz > 0 else ZERO)]])


def cross(a, b):
    return sympy.Matrix([[a[1] * b[2] - a[2] * b[1]], [a[2] * b[0] - a[0] * b[2]], [a[0] * b[1] - a[1] * b[0]]])


def inputs_of(sc, cfg):
    return dict(gp=[Fl(v) for v in cfg["gp"]], F=[Fl(v) for v in sc["F"]], dcam=[Fl(v) for v in sc["dcam"]],
                ccam=[Fl(v) for v in sc["ccam"]], a=Fl(cfg["a"]), cf=None, s=Fl(sc["s"]), bfx=Fl(sc["bfx"]), r2=Fl(cfg["r2"]),
                d=[Fl(v) for v in cfg["d"]], tex={})


def chain(sc, cfg, inp, dec=None):
    """One evaluation.  dec = None: decisions are taken and returned with their margins; else they are replayed.  Returns
    (reason, colour_valid, values {word: number}, dec, info)."""
    first = dec is None
    if first:
        dec = dict(px_margin=[], rel_margin=[])

    def decide(key, fn, px=None, rel=None):
        if first:
            dec[key] = fn()
            if px is not None:
                dec["px_margin"].append(float(px()))
            if rel is not None:
                dec["rel_margin"].append(float(rel()))
        return dec[key]

    def to_int(v):
        return abs(v - sympy.floor(v + HALF))                    # distance to the nearest integer

    val, info = {}, {}
    W, H, cell, cw, ch = sc["W"], sc["H"], sc["cell"], sc["cw"], sc["ch"]
    gp = sympy.Matrix(3, 1, inp["gp"])
    Fm = sympy.Matrix(3, 4, inp["F"])
    fx, fy, cx, cy = inp["dcam"]
    local = ref.MatrixVectorMultiplyHomogeneous(Fm, gp)
    # B/surfel_projection_nvcc_only.cuh:332-359 -> B/cuda_matrix.cuh:116-124, B/util.cuh:102-118
    if not decide("z", lambda: bool(local[2] > 0), rel=lambda: abs(local[2]) / local.norm()):
        return 1, False, val, dec, info
    pix = ref.Project(local, fx, fy, cx, cy)
    pxx, pxy = pix[0], pix[1]
    if not decide("inside", lambda: bool(pxx >= 0 and pxy >= 0 and pxx < W and pxy < H), px=lambda: min(to_int(pxx), to_int(pxy))):
        return 2, False, val, dec, info
    px, py = decide("pixel", lambda: (int(sympy.floor(pxx)), int(sympy.floor(pxy))))
    info["pixel"] = (px, py)
    raw = int(sc["depth"][py, px])
    # B/surfel_projection_nvcc_only.cuh:48-127 (IsAssociatedWithPixel), in its order
    if raw & 0x8000:
        return 3, False, val, dec, info
    if inp["cf"] is None:
        inp["cf"] = Fl(sc["cfactor"][py // cell, px // cell])      # :70-71, the cell of the associated pixel
    info["cfactor"] = float(sc["cfactor"][py // cell, px // cell])
    depth = ref.CorrectDepth(inp["cf"], inp["a"], 1 / (inp["s"] * raw))   # B/util.cuh:62-69
    n = unpack_normal10(int(cfg["normal_bits"]))
    nl = Fm[:, :3] * n
    # B/surfel_projection.cuh:92-99: the pixel-centre unprojector of a pixel-corner camera
    fx_inv, fy_inv = 1 / fx, 1 / fy
    cx_inv, cy_inv = -(cx - HALF) * fx_inv, -(cy - HALF) * fy_inv
    nx, ny = fx_inv * px + cx_inv, fy_inv * py + cy_inv
    cosine = nl[0] * nx + nl[1] * ny + nl[2]
    sgn = decide("cosine_sign", lambda: 1 if cosine > 0 else -1, rel=lambda: abs(cosine))
    # B/cost_function.cuh:81-88
    stddev = K01 * (sgn * cosine) * (depth * depth) / inp["bfx"]
    inv_stddev = inp["bfx"] / (K01 * (sgn * cosine) * (depth * depth))
    thr = K10 * stddev                                            # B/cost_function.cuh:48 through :89
    diff = local[2] - depth
    if decide("far", lambda: bool(abs(diff) > thr), rel=lambda: abs(abs(diff) - thr) / thr):
        return 4, False, val, dec, info
    facing = ref.DotProduct3(local, nl)                           # :107-111, (1 / |p|) p . n > 0
    if decide("away", lambda: bool(facing > 0), rel=lambda: abs(facing) / local.norm()):
        return 5, False, val, dec, info
    compat = ref.DotProduct3(nl, unpack_normal8(int(sc["normals"][py, px])))
    if decide("incompatible", lambda: bool(compat < KCOS), rel=lambda: abs(compat - KCOS) / KCOS):
        return 6, False, val, dec, info

    val[W_PXX], val[W_PXX + 1], val[W_DEPTH], val[W_ISTD] = pxx, pxy, depth, inv_stddev
    # B/cost_function.cuh:56-68
    u = ref.Unproject(Fl(px), Fl(py), depth, fx_inv, fy_inv, cx_inv, cy_inv)
    r = inv_stddev * ref.DotProduct3(nl, u - local)
    val[W_R] = r
    # B/robust_weighting.cuh:53-63 with B/cost_function.cuh:44-48,91-93
    if decide("tukey", lambda: bool(abs(r) < K10), rel=lambda: abs(abs(r) - K10) / K10):
        q = r / K10
        val[W_W] = (1 - q * q) ** 2
    else:
        val[W_W] = ZERO
    info["tukey_zero"] = not dec["tukey"]
    for k in range(6):
        fp = ref.DotProduct3(nl, ref.MatrixVectorMultiplyHomogeneous(EXP_PLUS[k][0], u) - local)
        fm = ref.DotProduct3(nl, ref.MatrixVectorMultiplyHomogeneous(EXP_MINUS[k][0], u) - local)
        val[W_JD + k] = inv_stddev * (fp - fm) / (2 * H_STEP)

    # ---- colour: B/surfel_projection.h:105-124 (the map's parameters), B/surfel_projection.cuh:194-207
    cfx, cfy, ccx, ccy = inp["ccam"]
    col = [(cfx / fx) * pxx + (-1 * cfx * cx / fx + ccx), (cfy / fy) * pxy + (-1 * cfy * cy / fy + ccy)]
    if not decide("colour_valid", lambda: bool(col[0] >= 0 and col[1] >= 0 and col[0] < cw and col[1] < ch),
                  px=lambda: min(to_int(col[0]), to_int(col[1]))):
        return 0, False, val, dec, info
    # B/cost_function.cuh:115-136 (ComputeTangentProjections)
    axis_y = decide("axis", lambda: bool(abs(n[0]) > K09), rel=lambda: abs(abs(n[0]) - K09) / K09)
    t1 = cross(n, sympy.Matrix([[0], [1], [0]]) if axis_y else sympy.Matrix([[1], [0], [0]]))
    points = [col]
    t_prev = None
    for which in (1, 2):
        t = t1 if which == 1 else cross(n, t_prev)
        sq = t[0] * t[0] + t[1] * t[1] + t[2] * t[2]
        big = decide(("tangent_length", which), lambda: bool(sq > K1E12), rel=lambda: abs(sq - K1E12) / K1E12)
        t = t * 2 * sympy.sqrt(inp["r2"] / (sq if big else K1E12))
        t_prev = t
        lt = ref.MatrixVectorMultiplyHomogeneous(Fm, gp + t)
        if first and not lt[2] > MARGIN:
            raise Unusable("tangent point behind the camera")
        p = ref.Project(lt, cfx, cfy, ccx, ccy)
        points.append([p[0], p[1]])
    info["samples"] = [[float(p[0]), float(p[1])] for p in points]

    def texel(kind, k, j, x, y):
        x, y = min(max(x, 0), cw - 1), min(max(y, 0), ch - 1)      # clamp addressing
        return Fl(int(sc["luma"][y, x])) / 255 * inp["tex"].get((kind, k, j), ONE)

    values, grads, interior = [], [], True
    for k, (x, y) in enumerate(points):
        xb, yb = x - HALF, y - HALF
        if first and not (xb > -1 + MARGIN and yb > -1 + MARGIN and xb < cw - MARGIN and yb < ch - MARGIN):
            raise Unusable("sample beyond the sampler's coordinate clamp")
        # the linear filter on unnormalised coordinates with clamp addressing (B/keyframe.cc:67-73; CUDA C Programming Guide,
        # "Texture Fetching"): i = floor(x - 0.5), weights frac(x - 0.5)
        ix, iy = decide(("floor", k), lambda: (int(sympy.floor(xb)), int(sympy.floor(yb))), px=lambda: min(to_int(xb), to_int(yb)))
        tl, tr, bl, br = [texel("v", k, j, ix + (j & 1), iy + (j >> 1)) for j in range(4)]
        values.append(ref.InterpolateBilinear(xb - ix, yb - iy, tl, tr, bl, br))
        # B/cost_function.cuh:200-211: the gradient's own footprint and weights
        gx, gy = decide(("gradient_floor", k), lambda: (int(sympy.floor(max(ZERO, xb))), int(sympy.floor(max(ZERO, yb)))))
        tx, ty = xb - gx, yb - gy
        sx, sy = decide(("gradient_clamp", k), lambda: (0 if tx < 0 else (2 if tx > 1 else 1), 0 if ty < 0 else (2 if ty > 1 else 1)))
        tx, ty = (ZERO, tx, ONE)[sx], (ZERO, ty, ONE)[sy]
        tl, tr, bl, br = [texel("g", k, j, gx + (j & 1), gy + (j >> 1)) for j in range(4)]
        grads.append(((br - bl) * ty + (tr - tl) * (1 - ty), (br - tr) * tx + (bl - tl) * (1 - tx)))
        interior = interior and bool(xb >= 0 and xb < cw and yb >= 0 and yb < ch)
    info["interior"] = interior
    # B/cost_function.cuh:140-156 and B/robust_weighting.cuh:81-86 with B/cost_function.cuh:105-109,177-179
    info["huber"] = False
    for q in range(2):
        res = K180 * (values[1 + q] - values[0]) - inp["d"][q]
        val[W_DR + q] = res
        if decide(("huber", q), lambda: bool(abs(res) < K10), rel=lambda: abs(abs(res) - K10) / K10):
            val[W_DW + q] = K001 * ONE
        else:
            val[W_DW + q] = K001 * (K10 / (res if res > 0 else -res))
            info["huber"] = True
        val[W_G + 2 * q] = K180 * (grads[1 + q][0] - grads[0][0])   # B/cost_function.cuh:250-253
        val[W_G + 2 * q + 1] = K180 * (grads[1 + q][1] - grads[0][1])
    for k in range(6):
        pp = ref.Project(ref.MatrixVectorMultiplyHomogeneous(EXP_PLUS[k][1], local), cfx, cfy, ccx, ccy)
        pm = ref.Project(ref.MatrixVectorMultiplyHomogeneous(EXP_MINUS[k][1], local), cfx, cfy, ccx, ccy)
        dP = (pp - pm) / (2 * H_STEP)
        for q in range(2):
            val[(W_J1, W_J2)[q] + k] = val[W_G + 2 * q] * dP[0] + val[W_G + 2 * q + 1] * dP[1]
    return 0, True, val, dec, info


def perturbations(colour):
    keys = [("gp", i) for i in range(3)] + [("F", i) for i in range(12)] + [("dcam", i) for i in range(4)] + \
           [("ccam", i) for i in range(4)] + [("a",), ("cf",), ("s",), ("bfx",), ("r2",), ("d", 0), ("d", 1)]
    tex = [("tex", (kind, k, j)) for kind in "vg" for k in range(3) for j in range(4)] if colour else []
    return keys, tex


def scales(job):
    """want, scale_issue, scale (40 words each) of one accepted, associated configuration."""
    sc, cfg, dec = job
    EPS = sympy.Float(2, PREC) ** -24
    inp = inputs_of(sc, cfg)
    _, colour, centre, _, _ = chain(sc, cfg, inp, dec)
    want, issue, extra = np.zeros(40), np.zeros(40), np.zeros(40)
    for w, v in centre.items():
        want[w] = float(v)
    keys, tex = perturbations(colour)
    for key in keys + tex:
        p = inputs_of(sc, cfg)
        p["cf"] = inp["cf"]
        if key[0] == "tex":
            p["tex"][key[1]] = 1 + EPS
        elif len(key) == 1:
            p[key[0]] = p[key[0]] * (1 + EPS)
        else:
            p[key[0]][key[1]] = p[key[0]][key[1]] * (1 + EPS)
        _, _, moved, _, _ = chain(sc, cfg, p, dec)
        dst = extra if key[0] == "tex" else issue
        for w, v in moved.items():
            dst[w] += float(abs(v - centre[w]) / EPS)
    return want, issue, issue + extra + np.abs(want)


# ---- drawing until the counts are met ---------------------------------------------------------------------------------------------
QUOTA = {"interior_zero": 18, "interior_cal": 18, "clamp": 10, "colour_invalid": 10, "border": 0, "huber": 4, "tukey_zero": 3,
         "z": 2, "outside": 2, "invalid_depth": 2, "depth_difference": 2, "facing_away": 2, "normals": 2}
MAX_DRAWS = 400


def lands_in(kind, reason, colour, info, sc_index):
    if kind in REASONS:
        return reason == REASONS.index(kind)
    if reason != 0:
        return False
    if kind == "colour_invalid":
        return not colour
    if not colour:
        return False
    if kind == "tukey_zero":
        return info["tukey_zero"]
    if info["tukey_zero"]:
        return False
    if kind in ("interior_zero", "interior_cal"):
        return info["interior"] and not info["huber"] and (info["cfactor"] == 0) == (kind == "interior_zero")
    if kind == "clamp":
        return not info["interior"]
    if kind == "huber":
        return info["huber"]
    return True


def accept_draws(scenes, rng):
    accepted, rejected = [], 0
    for si, sc in enumerate(scenes):
        for kind in KINDS:
            quota = QUOTA[kind]
            if kind == "colour_invalid" and si == 0:
                continue                                         # the depth camera's own colour image: no invalid colour pixel
            if kind == "border":
                quota = 12 if si in (0, 3) else 6               # (scenes 1, 2: the left column maps outside the colour image)
            got, draws, sides, misses = 0, 0, [0, 0, 0, 0], [0, 0, 0, 0]
            while got < quota and draws < MAX_DRAWS:
                side = 0
                if kind == "border":                             # the side with the fewest cases so far; one that keeps missing is given up
                    open_sides = [k for k in range(4) if misses[k] < 40]
                    if not open_sides:
                        break
                    side = min(open_sides, key=lambda k: sides[k])
                    misses[side] += 1
                draws += 1
                cfg = draw(sc, kind, rng, side)
                if cfg is None:
                    if kind == "border":
                        misses[side] = 40
                        continue
                    break
                try:
                    reason, colour, _, dec, info = chain(sc, cfg, inputs_of(sc, cfg))
                except Unusable:
                    rejected += 1
                    continue
                margins_ok = min(dec["px_margin"] + [1.0]) > MARGIN and min(dec["rel_margin"] + [1.0]) >= MARGIN
                if not margins_ok or not lands_in(kind, reason, colour, info, si):
                    rejected += 1
                    continue
                if kind == "border":
                    sides[side] += 1
                    misses[side] = 0
                accepted.append(dict(scene=si, kind=KINDS.index(kind), cfg=cfg, dec=dec, reason=reason, colour=colour, info=info))
                got += 1
            print("scene %d %-16s %3d accepted of %3d draws" % (si, kind, got, draws), flush=True)
    return accepted, rejected


def write_npz(path, arrays):
    """np.savez with fixed timestamps: the file depends on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            value = np.asarray(arrays[name])
            np.lib.format.write_array(buf, value if value.ndim == 0 else np.ascontiguousarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    t0 = time.time()
    rng = np.random.default_rng(SEED)
    scenes = make_scenes(rng)
    accepted, rejected = accept_draws(scenes, rng)
    N = len(accepted)
    print("%d configurations accepted, %d draws rejected, %.0f s" % (N, rejected, time.time() - t0), flush=True)
    want, issue, scale = np.zeros((N, 40)), np.zeros((N, 40)), np.zeros((N, 40))
    jobs = [(i, (scenes[c["scene"]], c["cfg"], c["dec"])) for i, c in enumerate(accepted) if c["reason"] == 0]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for (i, _), (w, si, s) in zip(jobs, pool.imap(scales, [j for _, j in jobs], chunksize=2)):
            want[i], issue[i], scale[i] = w, si, s
    for i, c in enumerate(accepted):
        if c["reason"] == 0:
            want[i, 0], want[i, 3] = 1.0, float(c["colour"])
            want[i, 1], want[i, 2] = c["info"]["pixel"]
    arrays = dict(seed=np.int64(SEED), rejected=np.int64(rejected), margin=np.float64(MARGIN),
                  kinds=np.array(KINDS), reasons=np.array(REASONS))
    for si, sc in enumerate(scenes):
        for name in ("depth", "normals", "luma", "cfactor", "F", "dcam", "ccam", "a", "s", "bfx"):
            arrays["scene%d_%s" % (si, name)] = sc[name]
        arrays["scene%d_shape" % si] = np.array([sc["W"], sc["H"], sc["cell"], sc["cw"], sc["ch"]], np.int32)
    arrays.update(
        scene=np.array([c["scene"] for c in accepted], np.int32), kind=np.array([c["kind"] for c in accepted], np.int32),
        reason=np.array([c["reason"] for c in accepted], np.int32), colour_valid=np.array([c["colour"] for c in accepted], np.bool_),
        interior=np.array([bool(c["info"].get("interior", False)) for c in accepted], np.bool_),
        a=np.array([c["cfg"]["a"] for c in accepted], np.float32),
        cfactor=np.array([c["info"].get("cfactor", 0.0) for c in accepted], np.float32),
        position=np.array([c["cfg"]["gp"] for c in accepted], np.float32),
        normal_bits=np.array([c["cfg"]["normal_bits"] for c in accepted], np.uint32),
        radius_squared=np.array([c["cfg"]["r2"] for c in accepted], np.float32),
        descriptors=np.array([c["cfg"]["d"] for c in accepted], np.float32),
        samples=np.array([c["info"].get("samples", [[0, 0]] * 3) for c in accepted], np.float64),
        px_margin=np.array([min(c["dec"]["px_margin"] + [1.0]) for c in accepted], np.float64),
        rel_margin=np.array([min(c["dec"]["rel_margin"] + [1.0]) for c in accepted], np.float64),
        want=want, scale_issue=issue, scale=scale)
    write_npz(OUT, arrays)
    print("wrote %s: %d configurations, %d bytes, %.0f s" % (OUT, N, os.path.getsize(OUT), time.time() - t0))


if __name__ == "__main__":
    main()
