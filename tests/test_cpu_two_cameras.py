"""The oracle pinned to the REFERENCE's own code on scenes whose colour camera differs from the depth camera (tests/two_cameras.py):
the comparisons of tests/test_cpu_oracle_vs_reference.py -- pairs against the reference's functions, activation + geometry step,
colour assignment, cost evaluation, surfel creation against the reference's kernels -- with that file's tolerances, on scenes where
40 % of the associated pairs have no valid colour pixel and thousands of samples touch the colour image's border; and both the
reference's functions and the oracle held to a plain float64 model of the colour chain (two_cameras.model_pairs).

Measured here (two_cameras.py's docstring has the census of every scene):
  pairs vs the reference's functions, exact weights: 0 association flips and 0 colour-validity flips on crop, crop_small and large;
    largest descriptor-residual difference 2.3e-3 (bound 5e-3);
  float64 model: colour-valid decisions of reference and oracle equal the model's on every pair further than 1e-3 px from a bound
    (5 of 96 191 pairs left out on crop_small, 0 of 3 489 on tiny: cap 0.1 %); largest descriptor-residual deviation of the
    reference's functions from the model 1.52e-3 (crop_small; tiny 7.7e-4), of the oracle 1.52e-3 -> two_cameras.REFERENCE_VS_MODEL =
    1.52e-3 and MODEL_RESIDUAL_BOUND = 4 x 1.52e-3 = 6.08e-3, which the GPU tests reuse;
  creation: the shim exposes the reference's CreateSurfelsForKeyframe path (ReferenceKernels.create_surfels_for_keyframe);
    descriptors within 1.6e-3 (bound 2e-3) on crop_small and large; the truncated colour is one code apart on 1 212 of 31 057
    surfels of crop_small and 6 of large, each where the float64 value is within 5e-3 of an integer (the test's rule; the largest distance
    measured on a differing code is 9e-4).

Skipped where neither the prebuilt reference library nor the reference's sources exist."""
import numpy as np
import pytest

from oracle import binding as ob
from oracle import ref_binding as rb
from tests import two_cameras as tc2
from tests.test_cpu_oracle_vs_reference import _fields, _ulps

pytestmark = pytest.mark.skipif(not rb.available(), reason="needs oracle/_ref/libbadslam_ref.so or /root/reference to build it")

SCENES = ["crop", "crop_small", "large"]


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tc2.build_scene(name)
        return cache[name]
    return get


def _fresh(scenes, name, **kw):
    """A fresh oracle of the scene (the tests below change surfels), checked to hold the work the scene is there for."""
    tc = scenes(name)
    ba = tc2.build_oracle(tc, **kw)
    census = tc2.assert_scene_has_the_work(tc, ba)
    return tc, ba, census


def test_the_census_agrees_with_the_oracle(scenes):
    """two_cameras.census (numpy float64, its own association test) against the oracle's evaluate_pairs on every scene: the same
    number of associated and of colour-invalid pairs up to last-bit decisions (measured: identical), and the scenes of today's
    suite ("same") indeed hold no colour-invalid pair."""
    for name in ("tiny", "same", "large", "crop_small", "crop"):
        tc = scenes(name)
        ba = tc2.build_oracle(tc)
        census = tc2.assert_scene_has_the_work(tc, ba)
        idx = np.arange(ba.surfels_size, dtype=np.uint32)
        associated = invalid = 0
        for k in range(len(ba.keyframes)):
            o = ba.evaluate_pairs(k, idx)
            a = _fields(o, "associated")[:, 0] != 0
            associated += int(a.sum())
            invalid += int((a & (_fields(o, "color_valid")[:, 0] == 0)).sum())
        print(name, census, "oracle:", associated, invalid)
        assert abs(census["associated"] - associated) <= 1e-3 * associated
        assert abs(census["colour_invalid"] - invalid) <= 1e-3 * associated
        if name in ("same", "large"):
            assert invalid == 0 and census["near_border"] == 0


@pytest.mark.parametrize("quantized", [False, True], ids=["exact-weights", "texture-unit-weights"])
@pytest.mark.parametrize("name", SCENES)
def test_pairs_against_the_reference_functions(scenes, name, quantized):
    """test_cpu_oracle_vs_reference.py::test_pairs_against_the_reference_functions with its tolerances, on the two-camera scenes."""
    tc, orc, census = _fresh(scenes, name)
    idx = np.arange(orc.surfels_size, dtype=np.uint32)
    assoc_r = flips = color_flips = pixel_flips = invalid_r = 0
    deltas = {k: [] for k in ("calibrated_depth_ulp", "depth_inv_stddev_rel", "depth_residual_m", "depth_weight", "desc_residual", "desc_weight", "grad")}
    f32 = lambda words, field, mask: _fields(words, field)[mask].view(np.float32).astype(np.float64)
    for k in range(len(orc.keyframes)):
        o = orc.evaluate_pairs(k, idx)
        r = rb.evaluate_pairs(orc, k, idx, quantize_texture_weights=quantized)
        ao, ar = _fields(o, "associated")[:, 0] != 0, _fields(r, "associated")[:, 0] != 0
        assoc_r += int(ar.sum()); flips += int((ao != ar).sum())
        both = ao & ar
        same_pixel = (_fields(o, "px")[:, 0] == _fields(r, "px")[:, 0]) & (_fields(o, "py")[:, 0] == _fields(r, "py")[:, 0])
        pixel_flips += int((both & ~same_pixel).sum())
        both &= same_pixel
        co, cr = _fields(o, "color_valid")[:, 0] != 0, _fields(r, "color_valid")[:, 0] != 0
        color_flips += int((both & (co != cr)).sum())
        invalid_r += int((ar & ~cr).sum())
        cv = both & co & cr
        deltas["calibrated_depth_ulp"].append(_ulps(_fields(o, "calibrated_depth")[both].view(np.float32), _fields(r, "calibrated_depth")[both].view(np.float32))[:, 0])
        inv_std = f32(r, "depth_inv_stddev", both)[:, 0]
        deltas["depth_inv_stddev_rel"].append(np.abs(f32(o, "depth_inv_stddev", both)[:, 0] - inv_std) / inv_std)
        deltas["depth_residual_m"].append(np.abs(f32(o, "depth_residual", both) - f32(r, "depth_residual", both))[:, 0] / inv_std)
        deltas["depth_weight"].append(np.abs(f32(o, "depth_weight", both) - f32(r, "depth_weight", both))[:, 0])
        for field in ("desc_residual", "desc_weight", "grad"):
            deltas[field].append(np.abs(f32(o, field, cv) - f32(r, field, cv)).max(axis=1))
    d = {k: np.concatenate(v) for k, v in deltas.items()}
    print(f"{name}, {'texture-unit' if quantized else 'exact'} weights: {assoc_r} associated pairs by the reference's functions ({invalid_r} without a "
          f"colour pixel), {flips} association flips, {pixel_flips} neighbouring-pixel flips, {color_flips} colour-validity flips")
    for k, v in d.items():
        print("   %-22s median %.3g  99.9 %% %.3g  max %.3g" % ((k,) + tuple(np.quantile(v, [0.5, 0.999, 1.0]))))
    # (the 320x240 scenes hold 96 191 pairs; the VGA scene of the other file, which asks for 100 000, holds 391 078)
    assert assoc_r >= 90000 and invalid_r >= tc2.MIN_INVALID_SHARE[name] * assoc_r
    assert abs(invalid_r - census["colour_invalid"]) <= 1e-3 * assoc_r
    assert flips + pixel_flips <= 1e-3 * assoc_r and color_flips <= 1e-3 * assoc_r
    assert d["calibrated_depth_ulp"].max() <= 1
    assert d["depth_inv_stddev_rel"].max() <= 1e-5
    assert d["depth_residual_m"].max() <= 2e-6
    assert d["depth_weight"].max() <= 1e-5
    assert np.quantile(d["grad"], 0.999) <= 1e-3 and np.count_nonzero(d["grad"] > 1e-2) <= 2e-4 * d["grad"].size
    if not quantized:
        assert np.median(d["desc_residual"]) <= 5e-4 and d["desc_residual"].max() <= 5e-3
        assert d["desc_weight"].max() <= 1e-5
    else:
        assert d["desc_residual"].max() <= 0.25 and d["desc_weight"].max() <= 1e-3


@pytest.mark.parametrize("name", SCENES)
def test_cost_evaluation_matches_the_reference_functions(scenes, name):
    """The full cost by the reference's functions against orc_evaluate_cost: the same residual count -- one depth residual per
    associated pair, two descriptor residuals per colour-valid pair, so FEWER than three per pair here -- and the same cost to 1e-4."""
    tc, orc, census = _fresh(scenes, name)
    orc.use_depth, orc.use_desc = 1, 1
    cost_o, n_o = orc.evaluate_cost()
    cost_r, n_r = rb.evaluate_cost(orc)
    # (206 995 residuals on crop_small: 96 191 + 2 x 55 402; the VGA scene of the other file has over a million)
    assert n_r > 200000 and abs(n_o - n_r) <= 1e-4 * n_r, (n_o, n_r)
    assert abs(cost_o - cost_r) <= 1e-4 * cost_r, (cost_o, cost_r)
    expected = census["associated"] + 2 * (census["associated"] - census["colour_invalid"])
    assert abs(n_r - expected) <= 1e-3 * n_r, (n_r, census)
    if tc2.MIN_INVALID_SHARE[name] > 0:
        assert n_r < 3 * census["associated"] - 2 * 0.2 * census["associated"]


@pytest.mark.parametrize("name", SCENES)
def test_geometry_step_and_activation_against_the_reference_kernels(scenes, name):
    """test_cpu_oracle_vs_reference.py::test_geometry_step_and_activation_against_the_reference_kernels (depth + descriptor residuals)
    with its tolerances: surfels whose sums mix depth-only keyframes with depth-plus-descriptor keyframes."""
    tc, ba, _ = _fresh(scenes, name)
    if name != "crop":
        tc2.displace(ba, 3)
    N = ba.surfels_size
    # crop comes with surfels only its inactive keyframe sees; these scenes' four keyframes overlap almost fully, so fifty surfels are
    # moved out of every keyframe's sight: the flags must discriminate here as well
    if name != "crop":
        ba.surfel_data[0, :50] += 100.0
    before = ba.surfel_data[:8, :N].copy()
    ref = rb.ReferenceKernels(ba)
    assert not ref.pairs_outside_int_range().any()
    ref.update_surfel_activation()
    ba.update_surfel_activation()
    assert np.count_nonzero((ref.active[:N] & 1) != (ba.active[:N] & 1)) == 0
    active = (ba.active[:N] & 1).astype(bool)
    assert 0.8 * N < active.sum() < N                      # the flags do discriminate
    if name != "crop":
        assert not active[:50].any()
    ref.optimize_geometry_iteration(True, True)
    ba.optimize_geometry_iteration()
    got, want = ba.surfel_data[:8, :N], ref.surfel_data[:8, :N]
    assert np.array_equal(got[4:6].view(np.uint32), want[4:6].view(np.uint32))
    assert np.array_equal(got[:, ~active].view(np.uint32), before[:, ~active].view(np.uint32))
    moved = np.abs(got[:3] - before[:3]).max(axis=0)
    assert np.median(moved[active]) > 5e-4
    assert np.count_nonzero(got[3].view(np.uint32) != want[3].view(np.uint32)) <= 1e-3 * N
    dpos = np.abs(got[:3] - want[:3]).max(axis=0)
    ddesc = np.abs(got[6:8] - want[6:8]).max(axis=0)
    print(f"{name}: N {N}; position median {np.median(dpos):.2e} p99.9 {np.percentile(dpos, 99.9):.2e} max {dpos.max():.2e} m, > 1e-6: {(dpos > 1e-6).sum()}; "
          f"descriptor median {np.median(ddesc):.2e} p99.9 {np.percentile(ddesc, 99.9):.2e} max {ddesc.max():.2e}")
    assert np.percentile(dpos, 99.9) <= 5e-7 and np.count_nonzero(dpos > 1e-6) <= 1e-3 * N and dpos.max() < 1e-3
    assert np.median(ddesc) < 5e-4 and np.percentile(ddesc, 99.9) < 5e-3 and np.count_nonzero(ddesc > 1e-2) <= 1e-3 * N
    # surfels seen by depth only keep their descriptors on both sides (no descriptor term in any keyframe): there are such surfels
    untouched = active & (got[6] == before[6]) & (got[7] == before[7])
    if tc2.MIN_INVALID_SHARE[name] > 0:
        assert untouched.sum() > 100
        assert np.array_equal(want[6:8, untouched].view(np.uint32), before[6:8, untouched].view(np.uint32))


@pytest.mark.parametrize("name", SCENES)
def test_colour_assignment_against_the_reference_kernels(scenes, name):
    """test_cpu_oracle_vs_reference.py::test_colour_assignment_against_the_reference_kernels with its tolerances; a surfel whose
    colour pixel is invalid in every keyframe that sees it keeps its colour on both sides."""
    tc, ba, _ = _fresh(scenes, name)
    N = ba.surfels_size
    ba.surfel_data[5, :N] = np.random.Generator(np.random.PCG64(13)).integers(0, 2 ** 32, N, dtype=np.uint32).view(np.float32)
    before = ba.surfel_data[5, :N].copy().view(np.uint32)
    ref = rb.ReferenceKernels(ba)
    assert not ref.pairs_outside_int_range().any()
    ref.assign_colors()
    ba.assign_colors()
    got32, want32 = ba.surfel_data[5, :N].view(np.uint32), ref.surfel_data[5, :N].view(np.uint32)
    got, want = got32.view(np.uint8).reshape(-1, 4).astype(int), want32.view(np.uint8).reshape(-1, 4).astype(int)
    assert np.abs(got - want).max() <= 1
    assert np.count_nonzero((got != want).any(axis=1)) <= 2e-3 * N
    assert len(np.unique(want[:, 0])) > 50
    kept = want32 == before
    assert np.array_equal(kept, got32 == before)
    if tc2.MIN_INVALID_SHARE[name] > 0:
        assert 100 < kept.sum() < N - 1000


@pytest.mark.parametrize("name", ["crop_small", "large"])
def test_surfel_creation_against_the_reference_kernels(scenes, name):
    """Colour row and descriptor rows of surfels created with a distinct colour camera against the reference's CreateSurfelsForKeyframe
    path (B/kernel_create_surfels.cu through oracle/ref_shim), as test_cpu_oracle_vs_reference.py::test_surfel_creation_against_the_
    reference_kernels does, with its tolerances: the colour is a bilinear sample at d2c(pixel centre) whether or not that lies in the
    colour image (clamp addressing), and so are the descriptors' three samples."""
    from scipy.spatial import cKDTree
    tc = scenes(name)
    ba = tc2.build_oracle(tc, create_from=[], perturbed=False)
    ref = rb.ReferenceKernels(ba)
    outside = differing = 0
    shares = []
    for k in range(len(ba.keyframes)):
        first = ba.surfels_size
        created = ba.create_surfels_for_keyframe(k)
        created_ref = ref.create_surfels_for_keyframe(k)
        assert created == created_ref > 0
        got, want = ba.surfel_data[:8, first:first + created], ref.surfel_data[:8, first:first + created]
        distance, partner = cKDTree(want[:3].T.astype(np.float64)).query(got[:3].T.astype(np.float64))
        assert len(np.unique(partner)) == created and distance.max() < 1e-6
        want = want[:, partner]
        for row in (3, 4):
            assert np.array_equal(got[row].view(np.uint32), want[row].view(np.uint32)), row
        ddesc = np.abs(got[6:8] - want[6:8])
        assert np.median(ddesc) < 5e-4 and ddesc.max() < 2e-3
        assert np.abs(got[6:8]).max() > 1.0
        # The colour is 255 x the bilinear sample, TRUNCATED.  With one camera the sample sits on a texel centre and both sides return
        # the texel; here the weights are not 0, the stand-in's filter (weighted sum of four texels) and the oracle's (nested lerps)
        # round differently in binary32, and a value within that rounding of an integer (a plateau of the texture: the true value IS
        # an integer) truncates either way.  So: at most one code apart, only where the float64 value is within 5e-3 of an integer
        # (the colour pixel of the stored binary32 position is known to ~1e-5 px, times 255 x a slope of at most one per pixel), and
        # elsewhere both equal the float64 model's truncation.
        geometry = tc2.colour_geometry(got, ba.pose(k), ba.depth_cam, ba.color_cam)
        codes, codes_ref = (np.ascontiguousarray(v[5]).view(np.uint32).view(np.uint8).reshape(-1, 4).astype(int) for v in (got, want))
        assert np.abs(codes - codes_ref).max() <= 1 and not codes[:, 3].any() and not codes_ref[:, 3].any()
        rgba = ba.kf_arrays(k)["color"]
        for channel in range(3):
            value = 255.0 * tc2.bilinear(rgba[:, :, channel].astype(np.float64) / 255.0, np.clip(geometry["c"][0], -5, 1e4), np.clip(geometry["c"][1], -5, 1e4))
            decided = np.abs(value - np.round(value)) > 5e-3
            assert np.array_equal(codes[decided, channel], np.floor(value[decided])), channel
            assert np.array_equal(codes_ref[decided, channel], np.floor(value[decided])), channel
            shares.append(float(decided.mean()))
            # measured: 0.62 .. 0.84 of the codes decided on crop_small (plateaus of the texture and clamped samples are integers),
            # 0.97 .. 0.99 on large; the guard is against a rule that leaves nothing to compare
            assert decided.mean() > 0.5
        differing += int((codes != codes_ref).any(axis=1).sum())
        outside += int((~geometry["colour_valid"]).sum())
        ref.surfel_data[:, :ba.surfels_size] = ba.surfel_data[:, :ba.surfels_size]
    print(f"{name}: {ba.surfels_size} surfels created, {outside} outside the colour image, {differing} colour words differ by one code; "
          f"share of decided codes per keyframe and channel {min(shares):.2f} .. {max(shares):.2f}")
    if name == "crop_small":
        assert outside > 1000          # surfels created from depth pixels the colour camera does not see


def _against_the_model(ba, evaluate):
    """two_cameras.against_the_model over all keyframes: (pairs, left out, mismatches, largest residual deviation, compared pairs)."""
    idx = np.arange(ba.surfels_size, dtype=np.uint32)
    counts, worst = np.zeros(4, int), 0.0
    for k in range(len(ba.keyframes)):
        words = evaluate(k, idx)
        row = tc2.against_the_model(ba, k, _fields(words, "associated")[:, 0] != 0, _fields(words, "color_valid")[:, 0] != 0,
                                    _fields(words, "desc_residual").view(np.float32).T)
        counts += row[:4]
        worst = max(worst, row[4])
    return int(counts[0]), int(counts[1]), int(counts[2]), worst, int(counts[3])


def test_reference_and_oracle_against_the_float64_model(scenes):
    """The reference's functions and the oracle against two_cameras.model_pairs on crop_small and tiny: colour-valid decisions equal
    wherever the model's colour pixel is more than 1e-3 px from a bound (at most 0.1 % of the pairs are nearer -- a handful); the
    reference's largest residual deviation IS what two_cameras.REFERENCE_VS_MODEL records (so MODEL_RESIDUAL_BOUND is 4 x a measured
    number, not a guess), and the oracle stays inside the bound."""
    worst_reference = 0.0
    for name in ("crop_small", "tiny"):
        tc, ba, census = _fresh(scenes, name)
        ref = _against_the_model(ba, lambda k, idx: rb.evaluate_pairs(ba, k, idx))
        orc = _against_the_model(ba, lambda k, idx: ba.evaluate_pairs(k, idx))
        print(name, "reference (pairs, left out, mismatches, worst, compared):", ref, "oracle:", orc)
        for pairs, left_out, mismatches, worst, compared in (ref, orc):
            assert left_out <= tc2.MODEL_MAX_LEFT_OUT * pairs and mismatches == 0
            assert compared >= 0.5 * pairs and pairs - compared >= tc2.MIN_INVALID_SHARE[name] * pairs
            assert worst <= tc2.MODEL_RESIDUAL_BOUND
        worst_reference = max(worst_reference, ref[3])
    assert 0.9 * tc2.REFERENCE_VS_MODEL <= worst_reference <= tc2.REFERENCE_VS_MODEL, worst_reference
    assert tc2.MODEL_RESIDUAL_BOUND == 4 * tc2.REFERENCE_VS_MODEL
