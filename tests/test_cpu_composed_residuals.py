"""The oracle's per-pair chain (orc_evaluate_pairs) and the reference's own functions (oracle/ref_binding.py: evaluate_pairs) against
the 60-digit goldens of tests/golden/composed_residuals.npz (scripts/make_golden_residuals.py), composed: which pixel and which cfactor
cell, how the calibrated depth enters the inverse standard deviation and the residual, the depth-to-colour map with a colour camera
of its own, the sample points and clamp addressing at the colour image's border, how three gradients combine into one Jacobian
row, the robust weights.  The bounds are tests/composed_residuals.py's; this module also measures the two ratios its constants
come from and asserts the table there.  tests/test_gpu_composed_residuals.py holds the HIP kernels to the same fixture."""
import numpy as np
import pytest

from oracle import binding as ob
from oracle import ref_binding as rb
from tests import composed_residuals as cr


@pytest.fixture(scope="module")
def fix():
    return cr.load()


@pytest.fixture(scope="module")
def oracle(fix):
    """Per scene: (the configurations' indices, the oracle's records in the hook's layout)."""
    out = []
    for si in range(cr.SCENES):
        ba, idx = cr.build_oracle(fix, si)
        out.append((ba, idx, cr.oracle_records(ba, fix, si)))
    return out


def test_fixture_holds_the_required_categories(fix):
    n = len(fix["scene"])
    kinds, reasons = list(fix["kinds"]), list(fix["reasons"])
    associated = fix["reason"] == 0
    valid = associated & fix["colour_valid"]
    interior = valid & fix["interior"]
    calibrated = interior & (fix["a"] != 0) & (fix["cfactor"] != 0)
    uncalibrated = interior & (fix["a"] == 0) & (fix["cfactor"] == 0)
    other_camera = fix["scene"] != 0
    clamp = valid & ~fix["interior"]
    huber = valid & (np.abs(fix["want"][:, 14:16]) > 10).any(axis=1)
    tukey_zero = associated & (np.abs(fix["want"][:, 5]) >= 10)
    shape = np.array([fix["scene%d_shape" % s][:2] for s in fix["scene"]])
    px, py = fix["want"][:, 1], fix["want"][:, 2]
    sides = [valid & (px == 0), valid & (px == shape[:, 0] - 1), valid & (py == 0), valid & (py == shape[:, 1] - 1)]
    print(f"{n} configurations ({int(fix['rejected'])} draws rejected): interior {interior.sum()} (calibrated {calibrated.sum()}, a = 0 = cfactor "
          f"{uncalibrated.sum()}), other colour camera {other_camera.sum()}, clamp addressing {clamp.sum()}, colour-invalid "
          f"{(associated & ~fix['colour_valid']).sum()}, border pixel {[int(s.sum()) for s in sides]}, Huber {huber.sum()}, Tukey zero branch "
          f"{tukey_zero.sum()}, not associated {[int((fix['reason'] == r).sum()) for r in range(1, len(reasons))]}")
    assert n >= cr.MIN_TOTAL
    assert interior.sum() >= cr.MIN_INTERIOR and calibrated.sum() >= cr.MIN_INTERIOR_CALIBRATED and uncalibrated.sum() >= cr.MIN_INTERIOR_UNCALIBRATED
    assert other_camera.sum() >= cr.MIN_OTHER_CAMERA
    assert clamp.sum() >= cr.MIN_CLAMP
    assert (associated & ~fix["colour_valid"]).sum() >= cr.MIN_COLOUR_INVALID
    assert sum(s.sum() for s in sides) >= cr.MIN_BORDER and all(s.sum() >= cr.MIN_BORDER_PER_SIDE for s in sides)
    assert huber.sum() >= cr.MIN_HUBER
    assert reasons[1:] == ["z", "outside", "invalid_depth", "depth_difference", "facing_away", "normals"]
    for r in range(1, len(reasons)):
        assert (fix["reason"] == r).sum() >= cr.MIN_PER_REASON, reasons[r]
    assert tukey_zero.sum() >= 4                                   # the depth weight's zero branch is reachable: the fixture holds cases
    # the scenes the issue names: sizes, cells, a colour camera of its own, one larger than the depth image, a height no multiple of the cell
    assert [tuple(int(v) for v in fix["scene%d_shape" % s]) for s in range(cr.SCENES)] == [(64, 48, 2, 64, 48), (64, 48, 4, 53, 38),
                                                                                            (64, 46, 4, 53, 38), (70, 45, 3, 97, 71)]
    assert np.array_equal(fix["scene0_dcam"], fix["scene0_ccam"]) and not np.array_equal(fix["scene1_dcam"], fix["scene1_ccam"])
    # the last, partial cfactor row of scene 2 is used
    sc2 = associated & (fix["scene"] == 2) & (py >= 44)
    assert sc2.sum() >= 2
    assert set(kinds) >= {"interior_zero", "interior_cal", "clamp", "colour_invalid", "border", "huber", "tukey_zero"}


def test_stored_decisions_honour_the_margin_rules(fix):
    margin = float(fix["margin"])
    assert margin == 1e-3
    assert fix["px_margin"].min() > margin and fix["rel_margin"].min() >= margin
    # recomputed from the stored values where they allow it: the depth pixel, the colour samples' texel boundaries, the thresholds
    want = fix["want"]
    associated = fix["reason"] == 0
    valid = associated & fix["colour_valid"]

    def to_integer(v):
        return np.abs(v - np.round(v))
    assert to_integer(want[associated][:, 34:36]).min() > margin
    assert np.array_equal(np.floor(want[associated][:, 34:36]), want[associated][:, 1:3])
    assert to_integer(fix["samples"][valid] - 0.5).min() > margin
    assert to_integer(fix["samples"][valid][:, 0]).min() > margin             # the colour pixel's own truncation
    assert (np.abs(np.abs(want[associated][:, 5]) - 10) >= 10 * margin).all()
    assert (np.abs(np.abs(want[valid][:, 14:16]) - 10) >= 10 * margin).all()
    # interior as the fixture says: all three samples inside 0 <= x - 0.5 < w, 0 <= y - 0.5 < h
    size = np.array([fix["scene%d_shape" % s][3:5] for s in fix["scene"]], np.float64)[:, None, :]
    b = fix["samples"] - 0.5
    inside = ((b >= 0) & (b < size)).all(axis=(1, 2))
    assert np.array_equal(inside[valid], fix["interior"][valid])
    assert not want[~associated].any() and not want[associated & ~fix["colour_valid"]][:, 14:34].any()
    for name in ("want", "scale", "scale_issue"):
        assert np.isfinite(fix[name]).all()
    assert (fix["scale"] >= fix["scale_issue"]).all()


def test_stored_inputs_are_exact_binary32_values(fix):
    names = ["position", "radius_squared", "descriptors", "a", "cfactor"]
    for si in range(cr.SCENES):
        names += ["scene%d_%s" % (si, n) for n in ("cfactor", "F", "dcam", "ccam", "a", "s", "bfx")]
        assert fix["scene%d_depth" % si].dtype == np.uint16 and fix["scene%d_normals" % si].dtype == np.uint16
        assert fix["scene%d_luma" % si].dtype == np.uint8
    for name in names:
        v = fix[name]
        assert np.isfinite(v).all() and np.array_equal(v.astype(np.float64), v.astype(np.float32).astype(np.float64)), name
    assert fix["normal_bits"].dtype == np.uint32 and (fix["normal_bits"] >> 30 == 0).all()


def test_oracle_against_the_goldens(fix, oracle):
    for si, (ba, idx, got) in enumerate(oracle):
        cr.check_decisions(got, fix, idx)
        cr.check_bounds(got, fix, idx, label=f"oracle, scene {si}:")


def _reference_records(fix, si):
    ba, idx = cr.build_oracle(fix, si)
    return idx, cr.oracle_records(ba, fix, si, evaluate=rb.evaluate_pairs, with_pixel_position=False)


REFERENCE_GROUPS = [name for name, (reference, _) in cr.MEASURED.items() if reference is not None]


@pytest.mark.skipif(not rb.available(), reason="needs the reference's headers (oracle/_ref/libbadslam_ref.so)")
def test_reference_functions_against_the_goldens(fix):
    for si in range(cr.SCENES):
        idx, got = _reference_records(fix, si)
        got[:, 34:36] = 0                                          # (not in the reference's record)
        want = fix["want"][idx]
        associated = fix["reason"][idx] == 0
        assert np.array_equal(got[:, 0] != 0, associated)
        assert np.array_equal(got[:, 0:4].astype(np.float64), want[:, 0:4])
        assert not got[~associated].any() and not got[np.ix_(associated & ~fix["colour_valid"][idx], cr.DESCRIPTOR_WORDS)].any()
        cr.check_bounds(got, fix, idx, groups=REFERENCE_GROUPS, label=f"reference, scene {si}:")


@pytest.mark.skipif(not rb.available(), reason="needs the reference's headers (oracle/_ref/libbadslam_ref.so)")
def test_constants_are_four_times_the_measured_ratios(fix, oracle):
    """Measures, per quantity group, the largest ratio |value - golden| / (2^-24 scale) of the reference's functions and of the oracle
    over the whole fixture, prints both (and the ratios against the scale of the issue's input list alone), and asserts that
    composed_residuals.MEASURED records them, that C is 4 x the larger, and that none exceeds the operation count of its path."""
    worst = {name: [0.0, 0.0] for name in cr.GROUPS}
    issue = {name: 0.0 for name in cr.GROUPS}
    for si, (ba, idx, got) in enumerate(oracle):
        _, ref = _reference_records(fix, si)
        for col, records, groups in ((0, ref, REFERENCE_GROUPS), (1, got, None)):
            for name, value in cr.ratios(records, fix, idx, groups).items():
                worst[name][col] = max(worst[name][col], value)
            for name, value in cr.ratios(records, fix, idx, groups, scale="scale_issue").items():
                issue[name] = max(issue[name], value)
    print("group, reference, oracle, C, ops, against the issue's scale:")
    for name in cr.GROUPS:
        print(f"  {name:22s} {worst[name][0]:.3f}  {worst[name][1]:.3f}  {cr.C[name]:.2f}  {cr.OPS[name]}  {issue[name]:.3g}")
    for name, (reference, orc) in cr.MEASURED.items():
        for col, recorded in ((0, reference), (1, orc)):
            if recorded is not None:
                assert 0.9 * recorded <= worst[name][col] <= recorded, (name, col, worst[name][col], recorded)   # recorded = measured, rounded up to 0.01
        assert cr.C[name] == 4 * max(v for v in (reference, orc) if v is not None)
        assert max(worst[name]) <= cr.OPS[name], (name, worst[name])
