"""The composed per-pair chain against 60-digit goldens: loader of tests/golden/composed_residuals.npz (scripts/make_golden_residuals.py
says what it holds and how it was made), builders that load one of its scenes into the CPU oracle and into the HIP backend, the
mapping of both records to named quantities, and the comparison.  A plain module: no fixtures, no conftest.  Used by
tests/test_cpu_composed_residuals.py and tests/test_gpu_composed_residuals.py.

The comparison, per quantity q of a configuration:   |got - want| <= C[group of q] * 2^-24 * scale[q]
with scale[q] the fixture's componentwise condition of q (sum over the binary32 inputs of |change of q| under a relative perturbation
of 2^-24, plus the texel values' and q's own rounding; `scale_issue` is the sum over the inputs alone).  Where scale[q] is 0 -- the
Tukey weight's zero branch -- the value must be equal.

C is not chosen and not taken from the HIP code: it is 4 x the larger of the two ratios |value - golden| / (2^-24 scale) measured on
the CPU for the reference's own functions compiled for the host (oracle/ref_binding.py: evaluate_pairs, exact bilinear weights) and
for the oracle; tests/test_cpu_composed_residuals.py measures both, prints them and asserts the table below.  4: the fast flavour
replaces correctly rounded divisions, square roots and the exponential by approximations of at most 1 ulp and fuses multiply-adds,
each of which at most doubles one term's rounding contribution; that leaves a further factor of two.

Measured (largest ratio over the fixture's configurations; "-": the implementation's record does not hold the quantity -- the
reference's headers have no pose Jacobians, neither CPU record the float pixel position, which the oracle gives through
orc_pair_pixel_position).  `ops` counts the binary32 operations on the quantity's longest path through the oracle's code
(oracle_core.c: orc_project_associate, orc_evaluate_pair and what they call), the plausibility cap: a ratio above it would mean that
a rounding is missing from the scale.  `issue scale`: the larger ratio against scale_issue, for the record -- unbounded for the
gradients (a gradient between equal descriptors and on a symmetric footprint does not depend on any perturbed input, yet carries the
texels' roundings) and 70 for the descriptor residuals, which is why the texel values and q's own rounding were added to the scale
(the generator's docstring derives both).

  group                  reference  oracle   C = 4 x max   ops   issue scale
  pixel_position         -          0.49     1.96          9     0.662
  calibrated_depth       1.13       1.13     4.52          6     2.25
  inv_stddev             1.14       1.10     4.56          41    1.35
  depth_residual         0.80       0.55     3.20          59    0.795
  depth_weight           0.80       0.56     3.20          63    0.794
  depth_jacobian         -          1.19     4.76          50    1.54
  descriptor_residuals   9.78       3.34     39.12         126   70.1
  descriptor_weights     1.19       1.19     4.76          128   1.65
  gradients              9.43       11.88    47.52         125   inf
  descriptor_jacobians   -          11.18    44.72         145   135

The descriptor quantities' ratios are the texel arithmetic: a gradient 180 ((br - bl) ty + (tr - tl) (1 - ty) - ...) of eight texel values
of about 0.5, each (float)t * (1.0f / 255.0f) with up to 1.5 * 2^-24 of relative error, loses 1e-4 of absolute accuracy whatever the
coordinates do, which is 3 to 12 times 2^-24 times the sum of |180 weight texel|.  (Values rounded up to 0.01.)
"""
import os

import numpy as np

from oracle import binding as ob

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composed_residuals.npz")
ULP = 2.0 ** -24
SCENES = 4
CAPACITY = 128                     # surfels per scene (the fixture holds about 80)
IDENTITY_POSE = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)

# words of the hook's 40-float record (layout above evaluate_pairs_kernel in kernels_pose.hip) per quantity group
GROUPS = {
    "pixel_position": [34, 35],
    "calibrated_depth": [4],
    "inv_stddev": [7],
    "depth_residual": [5],
    "depth_weight": [6],
    "depth_jacobian": list(range(8, 14)),
    "descriptor_residuals": [14, 15],
    "descriptor_weights": [16, 17],
    "gradients": list(range(30, 34)),
    "descriptor_jacobians": list(range(18, 30)),
}
DEPTH_GROUPS = ("pixel_position", "calibrated_depth", "inv_stddev", "depth_residual", "depth_weight", "depth_jacobian")
DESCRIPTOR_WORDS = list(range(14, 34))
# (reference, oracle): the docstring's table; None where the record does not hold the quantity
MEASURED = {
    "pixel_position": (None, 0.49),
    "calibrated_depth": (1.13, 1.13),
    "inv_stddev": (1.14, 1.10),
    "depth_residual": (0.80, 0.55),
    "depth_weight": (0.80, 0.56),
    "depth_jacobian": (None, 1.19),
    "descriptor_residuals": (9.78, 3.34),
    "descriptor_weights": (1.19, 1.19),
    "gradients": (9.43, 11.88),
    "descriptor_jacobians": (None, 11.18),
}
OPS = {"pixel_position": 9, "calibrated_depth": 6, "inv_stddev": 41, "depth_residual": 59, "depth_weight": 63, "depth_jacobian": 50,
       "descriptor_residuals": 126, "descriptor_weights": 128, "gradients": 125, "descriptor_jacobians": 145}
C = {name: 4 * max(v for v in pair if v is not None) for name, pair in MEASURED.items()}
# what the fixture must hold (the issue's table); the CPU test asserts it
MIN_TOTAL, MIN_INTERIOR, MIN_INTERIOR_CALIBRATED, MIN_INTERIOR_UNCALIBRATED = 240, 120, 40, 20
MIN_OTHER_CAMERA, MIN_CLAMP, MIN_COLOUR_INVALID, MIN_BORDER, MIN_BORDER_PER_SIDE, MIN_HUBER, MIN_PER_REASON = 120, 30, 20, 8, 2, 10, 5


def load():
    with np.load(PATH, allow_pickle=False) as f:
        return {name: (f[name][()] if f[name].ndim == 0 else f[name]) for name in f.files}


def scene(fix, si):
    W, H, cell, cw, ch = (int(v) for v in fix["scene%d_shape" % si])
    out = dict(W=W, H=H, cell=cell, cw=cw, ch=ch)
    for name in ("depth", "normals", "luma", "cfactor", "F", "dcam", "ccam", "a", "s", "bfx"):
        out[name] = fix["scene%d_%s" % (si, name)]
    return out


def configurations(fix, si, a=None):
    """Indices of the scene's configurations (with `a`: of those evaluated at that value of the depth parameter a)."""
    keep = fix["scene"] == si
    if a is not None:
        keep &= fix["a"] == np.float32(a)
    return np.flatnonzero(keep)


def values_of_a(fix, si):
    return sorted(set(float(v) for v in fix["a"][fix["scene"] == si]))


def surfel_rows(fix, si):
    """The scene's configurations as the 8 data rows of a surfel buffer, one surfel per configuration, and their indices."""
    idx = configurations(fix, si)
    assert 0 < len(idx) <= CAPACITY
    rows = np.zeros((8, len(idx)), np.float32)
    rows[0:3] = fix["position"][idx].T
    rows[3] = fix["normal_bits"][idx].view(np.float32)
    rows[4] = fix["radius_squared"][idx]
    rows[6:8] = fix["descriptors"][idx].T
    return rows, idx


def rgba(sc):
    return np.repeat(sc["luma"][:, :, None], 4, axis=2)


def build_oracle(fix, si):
    """(OracleBA holding scene si with its images as they are and one surfel per configuration, the configurations' indices)."""
    sc = scene(fix, si)
    rows, idx = surfel_rows(fix, si)
    color = ob.make_camera(sc["ccam"], sc["cw"], sc["ch"])
    depth = ob.make_camera(sc["dcam"], sc["W"], sc["H"])
    ba = ob.OracleBA(CAPACITY, float(sc["s"]), float(sc["bfx"]), sc["cell"], color, depth)
    kf = ba.add_preprocessed_keyframe(sc["depth"], sc["normals"], np.zeros_like(sc["depth"]), rgba(sc), IDENTITY_POSE)
    for j in range(12):
        kf.frame_T_global[j] = float(sc["F"][j])                 # the fixture's matrix, entry for entry (not one derived from a pose)
    ba.cfactor[:] = sc["cfactor"]
    ba.surfel_data[:8, :len(idx)] = rows
    ba.active[:len(idx)] = 1
    ba.surfels.surfels_size = ba.surfels.surfel_count = len(idx)
    return ba, idx


def build_gpu(fix, si, ctx):
    from badslam_amd import lowlevel as ll
    sc = scene(fix, si)
    rows, idx = surfel_rows(fix, si)
    color = ll.make_camera(sc["ccam"], sc["cw"], sc["ch"])
    depth = ll.make_camera(sc["dcam"], sc["W"], sc["H"])
    g = ll.Scene(ctx, CAPACITY, float(sc["s"]), float(sc["bfx"]), sc["cell"], color, depth)
    # (a keyframe of the right shape from a flat wall; its images are then replaced by the fixture's, as they are)
    g.add_keyframe(np.full((sc["H"], sc["W"]), 8000, np.uint16), np.zeros((sc["ch"], sc["cw"], 3), np.uint8), IDENTITY_POSE)
    kf = g.keyframes[0]
    kf["depth"].upload(np.ascontiguousarray(sc["depth"]))
    kf["normals"].upload(np.ascontiguousarray(sc["normals"]))
    kf["color"].upload(np.ascontiguousarray(rgba(sc)))
    g.cfactor.upload(sc["cfactor"])
    g.upload_surfels(rows, np.ones(len(idx), np.uint8))
    g.bind_keyframes()
    return g, idx


def oracle_records(ba, fix, si, evaluate=None, with_pixel_position=True):
    """The 40-word records (float32, the hook's layout) of all configurations of scene si from the oracle -- or from `evaluate(ba, 0,
    surfel indices)` returning the oracle's 37-word layout -- each configuration at its own `a`."""
    idx = configurations(fix, si)
    out = np.zeros((len(idx), 40), np.float32)
    for a in values_of_a(fix, si):
        ba.dp.a = a
        local = np.flatnonzero(fix["a"][idx] == np.float32(a)).astype(np.uint32)
        words = ba.evaluate_pairs(0, local) if evaluate is None else evaluate(ba, 0, local)
        pxy = ba.pair_pixel_positions(0, local) if with_pixel_position else np.zeros((len(local), 2), np.float32)
        out[local] = as_hook_record(words, pxy)
    return out


def gpu_records(g, fix, si):
    idx = configurations(fix, si)
    out = np.zeros((len(idx), 40), np.float32)
    F = scene(fix, si)["F"]
    for a in values_of_a(fix, si):
        g.dp.a = a
        g.set_intrinsics()
        local = np.flatnonzero(fix["a"][idx] == np.float32(a)).astype(np.uint32)
        out[local] = g.evaluate_pairs(0, local, F)
    return out


def as_hook_record(words37, pxy):
    """orc_pair_eval words (oracle.binding.OracleBA.PAIR_FIELDS) -> the hook's 40 floats."""
    f = words37.view(np.float32)
    out = np.zeros((len(words37), 40), np.float32)
    out[:, 0:4] = words37[:, 0:4].view(np.int32)
    out[:, 4:14] = f[:, 4:14]
    out[:, 14:16], out[:, 16:18], out[:, 18:30], out[:, 30:34] = f[:, 15:17], f[:, 17:19], f[:, 19:31], f[:, 33:37]
    out[:, 34:36] = np.where(words37[:, 0:1] != 0, pxy, 0)
    return out


def check_decisions(got, fix, idx):
    """Association, pixel, colour-valid decision and the all-zero rules of `got` (N, 40) against the golden."""
    want = fix["want"][idx]
    associated = fix["reason"][idx] == 0
    assert np.array_equal(got[:, 0] != 0, associated), np.flatnonzero((got[:, 0] != 0) != associated)
    assert np.array_equal(got[:, 0:4].astype(np.float64), want[:, 0:4])            # 0 / 1, the pixel, colour-valid (word 3)
    assert not got[~associated].any(), "a pair that is not associated has a non-zero word"
    invalid = associated & ~fix["colour_valid"][idx]
    assert not got[np.ix_(invalid, DESCRIPTOR_WORDS)].any(), "a colour-invalid pair has a non-zero descriptor word"
    assert not got[:, 36:40].any()


def ratios(got, fix, idx, groups=None, scale="scale"):
    """{group: largest |got - want| / (2^-24 scale)} over the configurations for which the group is defined; entries whose scale is 0
    must be equal and are left out."""
    want, s = fix["want"][idx], fix[scale][idx]
    associated = fix["reason"][idx] == 0
    valid = associated & fix["colour_valid"][idx]
    out = {}
    for name in (GROUPS if groups is None else groups):
        rows = associated if name in DEPTH_GROUPS else valid
        words = GROUPS[name]
        g, w, sq = got[np.ix_(rows, words)].astype(np.float64), want[np.ix_(rows, words)], s[np.ix_(rows, words)]
        assert np.all(np.isfinite(g)), name
        if scale == "scale":
            assert np.array_equal(g[sq == 0], w[sq == 0]), name
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(sq > 0, np.abs(g - w) / (ULP * sq), np.where(g == w, 0.0, np.inf))
        out[name] = float(r.max())
    return out


def check_bounds(got, fix, idx, groups=None, label=""):
    """Every quantity of `got` within C * 2^-24 * scale; returns the ratios."""
    measured = ratios(got, fix, idx, groups)
    print(label, {k: round(v, 3) for k, v in measured.items()})
    for name, value in measured.items():
        assert value <= C[name], (label, name, value, C[name])
    return measured
