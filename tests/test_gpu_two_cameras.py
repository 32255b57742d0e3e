"""Every sweep of the HIP backend with a colour camera that differs from the depth camera (tests/two_cameras.py: another image size,
another focal length, another principal point).  Every other scene of the suite gives the colour image the depth image's size and the
depth camera's parameters, so no pair there has an invalid colour pixel, no sample comes near the colour image's border and the index
math of a different colour size never runs.  Here 9 % (tiny) to 42 % (crop_small) of the associated pairs are depth-only -- mixed
with depth-plus-descriptor pairs inside the 64-surfel tiles -- and hundreds to thousands of colour-valid pairs take the border
sampler (the census is in two_cameras.py's docstring; every test asserts it for its scene before anything else).

Exact flavour: bit for bit against the CPU oracle, which tests/test_cpu_two_cameras.py pins to the reference's own code on the same
scenes.  Fast flavour: deterministic, launch-shape invariant, and within the project's existing bounds of the exact one.  Both
flavours' colour-valid decisions and descriptor residuals are also held to the float64 model of the colour chain
(two_cameras.model_pairs) with the bound measured on the reference's functions (two_cameras.MODEL_RESIDUAL_BOUND).

Stage -> scene: preprocessing and planes: tiny, large, crop_small, crop; creation (single call, batch with the chain on and off): large,
crop_small; per-pair hook: tiny, large, crop_small, one keyframe of crop; pose normal equations: tiny (every launch form), large, crop; batched pose
estimation and the fused pose-trial sweep: crop (all keyframes active, poses 5 mm / 1 mrad off); activation + geometry step: tiny
(every launch shape, hybrid included), crop; cost: tiny, large, crop_small, crop; colour assignment: crop_small; intrinsics step and PCG:
crop (all keyframes active); DirectBA: crop's images and cameras.  large -- the one scene whose colour image is the larger one, colour
pixels up to x = 487, y = 363 against a 320x240 depth image -- is what shows a depth size written for a colour size in the sweeps'
footprint addressing (luma_word_clamped): hook, pose sums and cost run on it."""
import ctypes as C
import math

import numpy as np
import pytest

from badslam_amd import capi, synthetic
from oracle import binding as ob
from tests import two_cameras as tc2
from tests.test_gpu_cost import _expected, _huber_cost, _key, _keys, _set_shape, _tukey_cost

pytestmark = pytest.mark.gpu

F32 = np.float32
_WORLD = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _no_signed_zero(words):
    w = np.array(words, np.uint32)
    w[w == 0x80000000] = 0            # -0.0 and +0.0 are the same value (a compiler may turn -fma(a, b, -c) into fma(-a, b, c))
    return w


def _cam(c):
    return np.array([c.fx, c.fy, c.cx, c.cy], np.float64)


def _frame(ba, k):
    return np.array(list(ba.keyframes[k].frame_T_global), np.float32)


def _activate_everything(ba):
    for kf in ba.keyframes:
        kf.activation = ob.KF_ACTIVE
    ba.active[:ba.surfels_size] = 1


def _fresh(name, variant="scene"):
    """A fresh oracle in the scene's state.  variant "active": every keyframe and surfel active and, on crop (whose poses are the
    ground truth), the poses 5 mm / 1 mrad off -- for the phases that move poses or sum over active keyframes only."""
    tc = _WORLD.setdefault(("tc", name), tc2.build_scene(name))
    ba = tc2.build_oracle(tc)
    if variant == "active":
        _activate_everything(ba)
        if name == "crop":
            rng = np.random.Generator(np.random.PCG64(11))
            for k, T in enumerate(tc.scene.poses_gt):
                ba.set_pose(k, synthetic.perturb_pose(rng, T))
    return tc, ba


def _world(name, variant="scene"):
    """(scene, a reference oracle nobody changes, a GPU scene, the census) per scene and variant; asserts -- on every call, so in every
    test -- that the scene holds the colour-invalid and the border work it is there for."""
    key = (name, variant)
    if key not in _WORLD:
        tc, ba = _fresh(name, variant)
        census = tc2.census(ba)
        _WORLD[key] = (tc, ba, tc2.build_gpu(tc, ba), census)
    tc, ba, g, census = _WORLD[key]
    assert census["associated"] > 1000, census
    assert census["colour_invalid"] >= tc2.MIN_INVALID_SHARE[name] * census["associated"], (name, census)
    assert census["non_interior"] >= tc2.MIN_NON_INTERIOR[name], (name, census)
    return tc, ba, g, census


def _launch_shapes(tile_waves, pose_parts):
    capi.check(capi.load().bahip_debug_set_launch_shapes(tile_waves, pose_parts))


def _hybrid_launches():
    n = C.c_longlong()
    capi.check(capi.load().bahip_debug_geometry_hybrid_launches(C.byref(n)))
    return int(n.value)


def _chain_batches():
    n = C.c_longlong()
    capi.check(capi.load().bahip_debug_creation_chain_batches(C.byref(n)))
    return int(n.value)


# ---- preprocessing and planes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "large", "crop_small", "crop"])
def test_keyframe_images(name):
    """bahip_compute_brightness on a cw x ch image (53x38, 487x363, 211x157: no multiple of the 32x8 pixel block) and the depth-side
    images next to it: every word the oracle's."""
    tc, ba, g, _ = _world(name)
    for k in range(len(ba.keyframes)):
        arrs, kf = ba.kf_arrays(k), g.keyframes[k]
        color = kf["color"].download()
        assert color.shape == (tc.color_height, tc.color_width, 4) and np.array_equal(color, arrs["color"]), k
        assert len(np.unique(color[:, :, 3])) > 50
        depth = kf["depth"].download()
        assert np.array_equal(depth, arrs["depth"]) and np.array_equal(kf["normals"].download(), arrs["normals"])
        valid = (depth & 0x8000) == 0
        assert np.array_equal(kf["radius"].download()[valid], arrs["radius"][valid])


# ---- creation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [True, False], ids=["chain", "no-chain"])
@pytest.mark.parametrize("name", ["large", "crop_small"])
def test_creation(name, chain, request):
    """Colour row and both descriptor rows (and every other row) of the surfels bahip_create_surfels_for_keyframe and the batch
    bahip_create_surfels_for_keyframes create -- the batch as one chain launch per keyframe and as the sequence of creations -- against
    the oracle's creations one by one.  On crop_small most creating pixels map outside the colour image: colour and descriptors are
    clamped samples there."""
    tc, _, _, _ = _world(name)
    lib = capi.load()
    capi.check(lib.bahip_debug_set_creation_chain(1 if chain else 0))
    request.addfinalizer(lambda: lib.bahip_debug_set_creation_chain(1))
    orc = tc2.build_oracle(tc, create_from=[], perturbed=False)
    g = tc2.build_gpu(tc)
    g.bind_keyframes()
    K = len(orc.keyframes)
    first = orc.create_surfels_for_keyframe(0)
    assert first == g.create_surfels_for_keyframe(0) > 10000
    plan = [(k, [j for j in range(K) if j != k]) for k in range(1, K)]
    n_ref = [orc.create_surfels_for_keyframe(k, filter_new_surfels=True, covis=covis) for k, covis in plan]
    before = _chain_batches()
    with g.lifecycle_batch(keyframes=[k for k, _ in plan]):
        n_got = g.create_surfels_for_keyframes(plan, filter_new_surfels=True, min_observation_count=2)
    assert _chain_batches() - before == (1 if chain else 0)
    assert n_got == sum(n_ref) and sum(1 for n in n_ref if n > 0) >= 2, (n_got, n_ref)
    n = orc.surfels_size
    assert g.surfels_size == n
    got, ref = g.download_surfels(), orc.surfel_data[:, :n]
    for row, what in ((5, "colour"), (6, "descriptor 1"), (7, "descriptor 2")):
        assert np.array_equal(_bits(got[row]), _bits(ref[row])), what
    assert np.array_equal(_bits(got[:8]), _bits(ref[:8]))
    assert np.abs(ref[6:8]).max() > 1.0 and len(np.unique(_bits(ref[5]))) > 1000
    if name == "crop_small":
        geometry = tc2.colour_geometry(ref[:8, :first], orc.pose(0), orc.depth_cam, orc.color_cam)
        assert (~geometry["colour_valid"]).sum() > 1000          # created from depth pixels the colour camera does not see


# ---- the per-pair hook --------------------------------------------------------------------------------------------------------------
GPU_FIELDS = (([4], "calibrated_depth"), ([5], "depth_residual"), ([6], "depth_weight"), ([7], "depth_inv_stddev"),
              (list(range(8, 14)), "depth_jac_pose"))
GPU_COLOUR_FIELDS = (([14, 15], "desc_residual"), ([16, 17], "desc_weight"), (list(range(18, 30)), "desc_jac_pose"), (list(range(30, 34)), "grad"))


def _hook_against_the_model(ba, k, out):
    """(pairs, left out, colour-valid mismatches, largest residual deviation, compared pairs) of hook words against the float64 model."""
    pairs, left_out, mismatches, compared, worst = tc2.against_the_model(ba, k, out[:, 0] == 1, out[:, 3] == 1, out[:, 14:16].T)
    return pairs, left_out, mismatches, worst, compared


@pytest.mark.parametrize("name,keyframes", [("tiny", None), ("large", None), ("crop_small", None), ("crop", [2])])
def test_pairs(name, keyframes):
    """Every word of bahip_debug_evaluate_pairs over all surfels x keyframes against orc_evaluate_pairs: the association and the
    colour-valid decision of every pair; the depth words of every associated pair; residuals, weights, gradients and pose Jacobians of
    every colour-valid pair -- the general border sampler with its second footprint fetch included -- and zeros where the colour pixel
    is invalid.  Then colour-valid and the residuals against the float64 model."""
    tc, ba, g, census = _world(name)
    idx = np.arange(ba.surfels_size, dtype=np.uint32)
    fields = ba.PAIR_FIELDS
    totals, worst, invalid = np.zeros(4), 0.0, 0
    for k in (range(len(ba.keyframes)) if keyframes is None else keyframes):
        out = g.evaluate_pairs(k, idx, _frame(ba, k))
        got, ref = out.view(np.uint32), ba.evaluate_pairs(k, idx)
        refi = ref.view(np.int32)
        assoc = refi[:, 0] == 1
        assert np.array_equal(out[:, 0] == 1.0, assoc), k
        a = np.flatnonzero(assoc)
        assert np.array_equal(out[a, 1].astype(np.int32), refi[a, 1]) and np.array_equal(out[a, 2].astype(np.int32), refi[a, 2])
        assert np.array_equal(out[a, 3] == 1.0, refi[a, 3] == 1), k
        assert np.array_equal(np.floor(out[a, 34]), out[a, 1]) and np.array_equal(np.floor(out[a, 35]), out[a, 2])
        pixel = tc2.colour_geometry(ba.surfel_data[:8, :ba.surfels_size], ba.pose(k), ba.depth_cam, ba.color_cam)["pixel"]
        assert np.abs(out[a, 34:36].T - pixel[:, a]).max() < 2e-3          # (binary32 projection at x ~ 300: an ulp is 3e-5 px)
        c = a[refi[a, 3] == 1]
        for rows, table in ((a, GPU_FIELDS), (c, GPU_COLOUR_FIELDS)):
            for cols, field in table:
                o, n = fields[field]
                x, y = _no_signed_zero(got[rows][:, cols]), _no_signed_zero(ref[rows][:, o:o + n])
                assert np.array_equal(x, y), (k, field, int((x != y).any(axis=1).sum()), len(rows))
        no_colour = a[refi[a, 3] != 1]
        invalid += len(no_colour)
        assert not got[no_colour][:, 14:34].any()
        assert not got[~assoc].any()
        row = _hook_against_the_model(ba, k, out)
        totals += (row[0], row[1], row[2], row[4])
        worst = max(worst, row[3])
    pairs, left_out, mismatches, compared = totals
    if name == "large":        # the colour image is the larger one: footprints beyond the DEPTH image's width and height are addressed
        c = np.concatenate([tc2.colour_geometry(ba.surfel_data[:8, :ba.surfels_size], ba.pose(k), ba.depth_cam, ba.color_cam)["c"][:, ba.evaluate_pairs(k, idx)[:, 0] != 0]
                            for k in range(len(ba.keyframes))], axis=1)
        assert (c[0] > tc.scene.width + 1).sum() > 1000 and (c[1] > tc.scene.height + 1).sum() > 1000
    print(f"{name}: {int(pairs)} pairs, {invalid} without a colour pixel; float64 model: {int(left_out)} left out, {int(mismatches)} mismatches, "
          f"residual deviation {worst:.3e} (bound {tc2.MODEL_RESIDUAL_BOUND:.2e})")
    assert invalid >= tc2.MIN_INVALID_SHARE[name] * pairs and compared > 0.4 * pairs
    if keyframes is None:
        assert pairs == census["associated"] and invalid == census["colour_invalid"]
    assert left_out <= tc2.MODEL_MAX_LEFT_OUT * pairs and mismatches == 0
    assert worst <= tc2.MODEL_RESIDUAL_BOUND


# ---- pose normal equations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pose_parts", [("tiny", 0), ("tiny", 1), ("tiny", 8), ("tiny", "lds"), ("large", 0), ("crop", 0)])
def test_pose_normal_equations(name, pose_parts, request):
    """H and b of every keyframe, bit for bit the oracle's defined sum, whatever the launch form: tiles in which depth-only lanes sit
    next to lanes with descriptor terms."""
    tc, ba, g, _ = _world(name)
    lib = capi.load()
    if pose_parts == "lds":
        capi.check(lib.bahip_debug_set_pose_form(2))
        request.addfinalizer(lambda: capi.check(lib.bahip_debug_set_pose_form(0)))
    else:
        _launch_shapes(0, pose_parts)
        request.addfinalizer(lambda: _launch_shapes(0, 0))
    ba.use_depth, ba.use_desc = 1, 1
    for k in range(len(ba.keyframes)):
        H_ref, b_ref, n, _ = ba.accumulate_pose_coeffs(k, accumulate_double=True)
        H_def, b_def, _, _ = ba.accumulate_pose_coeffs(k, accumulate_double=False)
        H, b = g.accumulate_pose_coeffs(k, True, True, _frame(ba, k))
        assert n > (300 if name == "tiny" else 10000)
        assert np.array_equal(_bits(H), _bits(H_def)), (k, np.abs(H - H_def).max())
        assert np.array_equal(_bits(b), _bits(b_def)), (k, np.abs(b - b_def).max())
        assert np.allclose(H, H_ref, rtol=0, atol=2e-7 * np.abs(H_ref).max())
    # descriptors only: nothing but the colour branch contributes
    ba.use_depth = 0
    try:
        H_def, b_def, _, _ = ba.accumulate_pose_coeffs(0, accumulate_double=False)
        H, b = g.accumulate_pose_coeffs(0, False, True, _frame(ba, 0))
        assert np.array_equal(_bits(H), _bits(H_def)) and np.array_equal(_bits(b), _bits(b_def)) and np.abs(H_def).max() > 0
    finally:
        ba.use_depth = 1


def test_batched_pose_estimation():
    """bahip_estimate_keyframe_poses on crop, poses 5 mm / 1 mrad off: every keyframe ends on the oracle's pose, bit for bit, after the
    same number of Gauss-Newton steps."""
    tc, ba, g, _ = _world("crop", "active")
    tc2.sync_gpu(g, ba)
    poses, its, conv, rounds = g.estimate_keyframe_poses(True, True)
    for k in range(len(ba.keyframes)):
        est, its_ref, conv_ref = ba.estimate_frame_pose(k, ba.pose(k))
        assert np.array_equal(_bits(poses[k]), _bits(est.to_array())), k
        assert its[k] == its_ref and conv[k] == int(conv_ref) and its_ref >= 2, (k, its[k], its_ref)
    assert rounds == its.max()
    g.bind_keyframes()


# ---- activation + geometry step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tile_waves,fused", [("tiny", 1, False), ("tiny", 4, False), ("tiny", 5, False), ("tiny", 1, True),
                                                   ("tiny", 4, True), ("crop", 0, False), ("crop", 0, True)])
def test_activation_and_geometry_step(name, tile_waves, fused, request):
    """Activation flags and the geometry step's eight surfel rows, bit for bit, for every launch shape: surfels whose sums mix depth-only
    keyframes with depth-plus-descriptor ones.  5: the hybrid shape, which needs the run order a pose phase leaves behind (asserted)."""
    tc, ref_ba, g, _ = _world(name)
    _, ba = _fresh(name)
    if name != "crop":                 # (crop comes with displaced surfels and descriptors)
        n = ba.surfels_size
        rng = np.random.Generator(np.random.PCG64(5))
        ba.surfel_data[2, :n] += rng.uniform(0, 0.004, n).astype(np.float32)
        ba.surfel_data[6, :n] += 3.0
    n = ba.surfels_size
    before = ba.surfel_data[:8, :n].copy()
    tc2.sync_gpu(g, ba, active=np.zeros(n, np.uint8))
    request.addfinalizer(lambda: (_launch_shapes(0, 0), tc2.sync_gpu(g, ref_ba)))
    if tile_waves == 5:
        g.estimate_keyframe_poses(True, True)       # leaves the heavy-first run order; the poses bound below are the scene's again
        g.bind_keyframes()
    _launch_shapes(tile_waves, 0)
    hybrid_before = _hybrid_launches()
    ba.use_depth, ba.use_desc = 1, 1
    ba.update_surfel_activation()
    if fused:
        g.update_activation_and_optimize_geometry(True, True)
    else:
        g.update_surfel_activation()
        assert np.array_equal(g.active_buf.download()[0, :n], ba.active[:n])
        g.optimize_geometry_iteration(True, True)
    ba.optimize_geometry_iteration()
    assert np.array_equal(g.active_buf.download()[0, :n], ba.active[:n])
    assert ba.active[:n].sum() > 0.8 * n
    if tile_waves == 5:
        assert _hybrid_launches() - hybrid_before >= 1
    got, ref = g.download_surfels(), ba.surfel_data[:, :n]
    assert np.array_equal(_bits(got[:8]), _bits(ref[:8])), int((_bits(got[:8]) != _bits(ref[:8])).any(axis=0).sum())
    assert np.abs(ref[2] - before[2]).mean() > 1e-4
    # surfels that only depth-only pairs see keep their descriptors; the others' moved
    kept = (ba.active[:n] & 1).astype(bool) & (ref[6] == before[6]) & (ref[7] == before[7]) & (ref[2] != before[2])
    assert kept.sum() > (10 if name == "tiny" else 100) and (ref[6] != before[6]).sum() > 0.3 * n


# ---- cost ---------------------------------------------------------------------------------------------------------------------------
def _tukey_costs(r):
    """tests/test_gpu_cost.py::_tukey_cost on a binary32 array: the same operations in the same order, each rounded to binary32."""
    k, c = F32(10), F32(1) / F32(6)
    q = r * F32(0.1)
    t = F32(1) - q * q
    return np.where(np.abs(r) < k, F32(1) * (c * k * k * (F32(1) - t * t * t)), F32(1) * (c * k * k)).astype(np.float32)


def _huber_costs(r):
    k = F32(10)
    a = np.abs(r)
    return ((F32(1) * F32(1e-2)) * np.where(a < k, F32(0.5) * r * r, k * (a - F32(0.5) * k))).astype(np.float32)


def _expected_costs(g, ba):
    """tests/test_gpu_cost.py::_expected, vectorised: per keyframe the exact sums (math.fsum) of the per-pair terms of the hook."""
    idx = np.arange(g.surfels_size, dtype=np.uint32)
    per, terms = [], [[], [], []]
    for k in range(len(g.keyframes)):
        out = g.evaluate_pairs(k, idx, _frame(ba, k))
        assoc = out[:, 0] == 1
        col = assoc & (out[:, 3] == 1)
        parts = [_tukey_costs(out[assoc, 5]), _huber_costs(out[col, 14]), _huber_costs(out[col, 15])]
        for t, v in zip(terms, parts):
            t.append(v.astype(np.float64))
        per.append(dict(depth=math.fsum(parts[0].astype(np.float64)), descriptor_1=math.fsum(parts[1].astype(np.float64)),
                        descriptor_2=math.fsum(parts[2].astype(np.float64)), depth_residuals=int(assoc.sum()), descriptor_pairs=int(col.sum())))
    total = dict(depth=math.fsum(np.concatenate(terms[0])), descriptor_1=math.fsum(np.concatenate(terms[1])),
                 descriptor_2=math.fsum(np.concatenate(terms[2])), depth_residuals=sum(c["depth_residuals"] for c in per),
                 descriptor_pairs=sum(c["descriptor_pairs"] for c in per))
    return total, per


def test_the_vectorised_robust_costs_are_the_scalar_ones():
    r = np.concatenate([np.linspace(-30, 30, 2001), [9.999999, 10.0, 10.000001, -10.0, 0.0, 1e-20]]).astype(np.float32)
    assert np.array_equal(_bits(_tukey_costs(r)), _bits([_tukey_cost(v) for v in r]))
    assert np.array_equal(_bits(_huber_costs(r)), _bits([_huber_cost(v) for v in r]))


@pytest.mark.parametrize("name", ["tiny", "large", "crop_small", "crop"])
def test_cost(name):
    """bahip_evaluate_cost and bahip_evaluate_frame_cost: each sum the exact sum of its per-pair terms (on tiny also by test_gpu_cost.py's
    own scalar _expected), with FEWER descriptor pairs than depth residuals in total and in every keyframe; the oracle's residual
    count and cost; and the same bits for every cost shape."""
    tc, ba, g, census = _world(name)
    total, per = g.evaluate_cost(True, True)
    exp_total, exp_per = _expected_costs(g, ba)
    mixed = tc2.MIN_INVALID_SHARE[name] > 0       # (large: every pair has a colour pixel -- it is there for the larger colour image)
    if name == "tiny":
        scalar_total, scalar_per = _expected(g, True, True)
        assert _key(scalar_total) == _key(exp_total) and [_key(c) for c in scalar_per] == [_key(c) for c in exp_per]
    for k, (got, exp) in enumerate(zip(per, exp_per)):
        assert _key(got) == _key(exp), (k, got, exp)
        assert 0 < got["descriptor_pairs"] <= got["depth_residuals"] and (got["descriptor_pairs"] < got["depth_residuals"]) == mixed, (k, got)
        assert _key(g.evaluate_frame_cost(k, _frame(ba, k))) == _key(got), k
    assert _key(total) == _key(exp_total), (total, exp_total)
    assert total["depth_residuals"] == census["associated"]
    assert total["depth_residuals"] - total["descriptor_pairs"] == census["colour_invalid"]
    ba.use_depth, ba.use_desc = 1, 1
    ref, ref_count = ba.evaluate_cost()
    assert (total["descriptor_pairs"] < total["depth_residuals"]) == mixed
    assert total["depth_residuals"] + 2 * total["descriptor_pairs"] == ref_count
    value = total["depth"] + total["descriptor_1"] + total["descriptor_2"]
    assert abs(value - ref) <= 1e-9 * abs(ref), (value, ref)
    for use_depth, use_desc in ((True, False), (False, True)):
        assert _key(g.evaluate_cost(use_depth, use_desc)[0]) == _key(_only(exp_total, use_depth, use_desc))
    reference = _keys(g.evaluate_cost())
    try:
        for shape in [(1, 1, 1, 0), (8, 0, 0, 1), (4, 37, 3, 0), (2, 5, 2, 1), (8, 3, 256, 0), (1, 1000, 4, 1)]:
            _set_shape(*shape)
            assert _keys(g.evaluate_cost()) == reference, shape
    finally:
        _set_shape()


def test_cost_of_two_surfel_shards_is_the_unsharded_cost():
    """One world-2 surfel-sharded cost call on crop (threads on one GPU exchanging through the loopback hook, as
    tests/test_gpu_cost.py::_surfel_shards): both ranks return the unsharded bits, per keyframe and in total."""
    from badslam_amd import multigpu
    from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks
    tc, ba, g, _ = _world("crop")
    reference = _keys(g.evaluate_cost())
    n = ba.surfels_size

    def rank_main(rank, hook):
        gr = tc2.build_gpu(tc, ba)
        mine = multigpu.shard_chunks(n, rank, 2, chunk=1024)
        gr.upload_surfels(np.ascontiguousarray(ba.surfel_data[:, :n][:, mine]), np.ones(mine.size, np.uint8))
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        return dict(cost=_keys(gr.evaluate_cost()), size=int(mine.size), keep=(hook, gr))

    results, loop = _run_ranks(2, rank_main)
    assert all(r["cost"] == reference for r in results) and min(r["size"] for r in results) > 10000
    assert loop.calls == 1


def _only(cost, use_depth, use_desc):
    out = dict(cost)
    if not use_depth:
        out.update(depth=0.0, depth_residuals=0)
    if not use_desc:
        out.update(descriptor_1=0.0, descriptor_2=0.0, descriptor_pairs=0)
    return out


# ---- the fused pose-trial sweep -----------------------------------------------------------------------------------------------------
def test_controlled_pose_phase():
    """bahip_estimate_keyframe_poses_controlled on crop: cost_before / cost_after are bahip_evaluate_cost's per-keyframe entries before
    and after, field by field, every keyframe with fewer descriptor pairs than depth residuals; and with lambda = 0 a keyframe none of
    whose candidates was rejected takes the plain phase's pose (the plain sweeps' normal equations, round after round) and iteration
    count.  Measured on an MI355X: 6 of 6 keyframes without a rejected candidate, 3 to 4 iterations each; at least half are required."""
    tc, ba, g, _ = _world("crop", "active")
    control = (4.0, 0.5, 0.0, 1e6, 4)
    K = len(ba.keyframes)
    try:
        tc2.sync_gpu(g, ba)
        plain_poses, plain_its, plain_conv, _ = g.estimate_keyframe_poses(True, True)
        tc2.sync_gpu(g, ba)
        before = g.evaluate_cost(True, True)[1]
        out = g.estimate_keyframe_poses_controlled([0.0] * K, control)
        after = g.evaluate_cost(True, True)[1]
    finally:
        tc2.sync_gpu(g, ba)
    assert out["iterations"].sum() > 0
    for k in range(K):
        for got, want in ((out["cost_before"][k], before[k]), (out["cost_after"][k], after[k])):
            assert _key(got) == _key(want), (k, got, want)
            assert 0 < got["descriptor_pairs"] < got["depth_residuals"], (k, got)
    clean = [k for k in range(K) if out["rejected"][k] == 0]
    print(f"{len(clean)} of {K} keyframes without a rejected candidate; iterations {list(out['iterations'])}, plain {list(plain_its)}")
    assert len(clean) >= K // 2
    for k in clean:
        assert np.array_equal(_bits(out["poses"][k]), _bits(plain_poses[k])), k
        assert out["iterations"][k] == plain_its[k] and out["converged"][k] == plain_conv[k], k


# ---- colour assignment ------------------------------------------------------------------------------------------------------------
def test_assign_colors():
    """bahip_assign_colors on crop_small -- the colour image smaller than the depth image: sample_rgba's pitch and clamps at cw x ch --
    bit for bit; surfels whose colour pixel is invalid in every keyframe that sees them keep their colour."""
    tc, ref_ba, g, _ = _world("crop_small")
    _, ba = _fresh("crop_small")
    n = ba.surfels_size
    ba.surfel_data[5, :n] = np.random.Generator(np.random.PCG64(13)).integers(0, 2 ** 32, n, dtype=np.uint32).view(np.float32)
    before = ba.surfel_data[:8, :n].copy()
    try:
        tc2.sync_gpu(g, ba)
        g.assign_colors()
        got = g.download_surfels()
    finally:
        tc2.sync_gpu(g, ref_ba)
    ba.assign_colors()
    ref = ba.surfel_data[:, :n]
    assert np.array_equal(_bits(got[5]), _bits(ref[5]))
    kept = _bits(ref[5]) == _bits(before[5])
    assert 100 < kept.sum() < n - 1000, kept.sum()
    for row in (0, 1, 2, 3, 4, 6, 7):
        assert np.array_equal(_bits(got[row]), _bits(before[row]))


# ---- intrinsics step --------------------------------------------------------------------------------------------------------------
def _colour_validity(ba):
    idx = np.arange(ba.surfels_size, dtype=np.uint32)
    words = [ba.evaluate_pairs(k, idx) for k in range(len(ba.keyframes))]
    return np.stack([(w[:, 0] != 0) & (w[:, 3] != 0) for w in words]), np.stack([w[:, 0] != 0 for w in words])


def test_intrinsics_step():
    """bahip_optimize_intrinsics with depth and colour optimisation on crop, cameras 0.5 .. 2 px off, a != 0: the sums
    (bahip_debug_read_intrinsics_sums) are the oracle's accumulators rounded to binary32, and the cameras, `a` and the cfactor image
    the oracle's bits.  The step changes d2c, so pairs change colour validity across it (asserted from the oracle); a second step from
    there ends in the oracle's bits again."""
    tc, ref_ba, g, _ = _world("crop", "active")
    _, ba = _fresh("crop", "active")
    for cam, off in ((ba.depth_cam, (0.5, -0.6, 1.23, -2.17)), (ba.color_cam, (0.4, -0.3, 0.8, -0.6))):
        cam.fx += off[0]; cam.fy += off[1]; cam.cx += off[2]; cam.cy += off[3]
    ba.dp.a = 0.0125
    ba.cfactor[:] = np.random.Generator(np.random.PCG64(5)).uniform(-2e-3, 2e-3, ba.cfactor.shape).astype(np.float32)
    ba.use_depth, ba.use_desc = 1, 1
    try:
        tc2.sync_gpu(g, ba)
        valid_before, assoc_before = _colour_validity(ba)
        assert (assoc_before & ~valid_before).sum() > 0.2 * assoc_before.sum()
        glob, cells = ba.intrinsics_accumulators(True, True)
        start = np.concatenate([_cam(ba.depth_cam), _cam(ba.color_cam)])
        cc_r, dc_r, a_r = ba.optimize_intrinsics(True, True)
        cc_g, dc_g, a_g = g.optimize_intrinsics(True, True)
        got, got_cells = g.read_intrinsics_sums()
        assert np.count_nonzero(got) == 34
        assert np.array_equal(_bits(got), _bits(glob.astype(np.float32))), np.flatnonzero(_bits(got) != _bits(glob.astype(np.float32)))
        assert np.array_equal(_bits(got_cells), _bits(cells.astype(np.float32)))
        for step in range(2):
            assert np.array_equal(_bits(_cam(dc_g)), _bits(_cam(dc_r))), (step, _cam(dc_g), _cam(dc_r))
            assert np.array_equal(_bits(_cam(cc_g)), _bits(_cam(cc_r))), (step, _cam(cc_g), _cam(cc_r))
            assert np.array_equal(_bits([a_g]), _bits([a_r])), (step, a_g, a_r)
            assert np.array_equal(_bits(g.cfactor.download()), _bits(ba.cfactor)), step
            if step == 0:
                moved = np.abs(np.concatenate([_cam(dc_r), _cam(cc_r)]) - start)
                assert moved[:4].max() > 0.1 and moved[4:].max() > 0.05
                valid_after, assoc_after = _colour_validity(ba)
                same = assoc_before & assoc_after
                changed = int((same & (valid_before != valid_after)).sum())
                print(f"{changed} of {int(same.sum())} pairs change colour validity across the step")
                assert changed > 0
                cc_r, dc_r, a_r = ba.optimize_intrinsics(True, True)
                cc_g, dc_g, a_g = g.optimize_intrinsics(True, True)
    finally:
        tc2.sync_gpu(g, ref_ba)


# ---- PCG --------------------------------------------------------------------------------------------------------------------------
def _pcg_state(mode):
    """crop with every keyframe and surfel active, poses 3 mm / 0.5 mrad off (tests/test_gpu_intrinsics_pcg_vs_oracle.py::_pcg_setup's
    magnitudes); mode "all": cameras off as well and a != 0."""
    tc, ba = _fresh("crop", "active")
    rng = np.random.Generator(np.random.PCG64(33))
    for k, T in enumerate(tc.scene.poses_gt):
        ba.set_pose(k, synthetic.perturb_pose(rng, T, 0.003, 0.0005))
    if mode == "all":
        for cam, off in ((ba.depth_cam, (0.3, -0.2, 0.5, -0.4)), (ba.color_cam, (0.2, -0.3, 0.4, -0.2))):
            cam.fx += off[0]; cam.fy += off[1]; cam.cx += off[2]; cam.cy += off[3]
        ba.dp.a = 0.0125
    ba.use_depth, ba.use_desc = 1, 1
    ba.last_ba_iteration_count = ba.ba_iteration_count        # no end-of-scheme tasks ahead of the iteration
    return tc, ba


@pytest.mark.parametrize("mode", ["poses+geometry", "all"])
def test_pcg(mode):
    """The PCG scheme on crop.  Assembled r and M (max_inner_iterations = 0), every entry; one full outer iteration against the oracle --
    inner steps, surfels, poses, cameras, a, cfactors bit for bit; and the windowed iteration with everything active, which must be the
    whole-map one."""
    world = _world("crop", "active")
    tc, ba = _pcg_state(mode)
    g, ref_ba = world[2], world[1]
    di = mode == "all"
    N, K = ba.surfels_size, len(ba.keyframes)
    before = ba.surfel_data[:8, :N].copy()
    try:
        tc2.sync_gpu(g, ba)
        h = tc2.build_gpu(tc, ba)
        r_ref, M_ref = ba.pcg_assemble(True, True, di, di, gauge_keyframe=1)
        g.pcg_iteration(optimize_depth_intrinsics=di, optimize_color_intrinsics=di, max_inner_iterations=0, gauge_keyframe=1)
        U = len(r_ref)
        assert U == 6 * (K - 1) + 3 * N + ((5 + ba.cf_w * ba.cf_h + 4) if di else 0)
        r, M = g.read_pcg_vector(0, U), g.read_pcg_vector(1, U)
        assert np.array_equal(_bits(r), _bits(r_ref)), np.flatnonzero(_bits(r) != _bits(r_ref))[:10]
        assert np.array_equal(_bits(M), _bits(M_ref)), np.flatnonzero(_bits(M) != _bits(M_ref))[:10]
        # descriptor entries of surfels no colour-valid pair sees are zero; the others' are not
        desc_M = M_ref[6 * (K - 1):6 * (K - 1) + 3 * N].reshape(N, 3)[:, 1]
        assert 100 < np.count_nonzero(desc_M == 0) < N - 1000

        tc2.sync_gpu(g, ba)                       # (max_inner_iterations = 0 applies a zero step; start again from the oracle's words)
        stats = ba.bundle_adjustment(optimize_depth_intrinsics=di, optimize_color_intrinsics=di, optimize_poses=True, optimize_geometry=True,
                                     min_iterations=1, max_iterations=1, use_pcg=True, increase_ba_iteration_count=False, pcg_gauge_keyframe=0)
        runs = []
        for scene, windowed in ((g, False), (h, True)):
            scene.update_surfel_normals()
            steps, _ = scene.pcg_iteration(optimize_depth_intrinsics=di, optimize_color_intrinsics=di, gauge_keyframe=0, windowed=windowed)
            runs.append((steps, scene.download_surfels(), [kf["pose"].copy() for kf in scene.keyframes], _cam(scene.depth_cam), _cam(scene.color_cam),
                         scene.dp.a, scene.cfactor.download()))
        ref = ba.surfel_data[:, :N]
        assert 3 <= stats.pcg_inner_steps_total <= 30
        assert np.median(np.abs(ref[:3] - before[:3]).max(axis=0)) > 1e-4
        for what, (steps, surfels, poses, depth_cam, color_cam, a, cfactor) in zip(("whole map", "windowed"), runs):
            assert steps == stats.pcg_inner_steps_total, (what, steps, stats.pcg_inner_steps_total)
            assert np.array_equal(_bits(surfels[:8]), _bits(ref[:8])), (what, np.abs(surfels[:3] - ref[:3]).max())
            for k in range(K):
                assert np.array_equal(_bits(poses[k]), _bits(ba.pose(k))), (what, k)
            assert np.array_equal(_bits(depth_cam), _bits(_cam(ba.depth_cam))) and np.array_equal(_bits(color_cam), _bits(_cam(ba.color_cam))), what
            assert np.array_equal(_bits([a]), _bits([ba.dp.a])) and np.array_equal(_bits(cfactor), _bits(ba.cfactor)), what
    finally:
        tc2.sync_gpu(g, ref_ba)


# ---- DirectBA -----------------------------------------------------------------------------------------------------------------------
def _directba(tc, cap=600000, min_obs=2):
    from badslam_amd.directba import DirectBA
    scene = tc.scene
    ba = DirectBA(cap, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, tc.color_camera, scene.camera,
                  min_observation_count_while_bootstrapping_1=min_obs, min_observation_count_while_bootstrapping_2=min_obs,
                  min_observation_count=min_obs)
    for k in range(len(scene.depth)):
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], scene.poses_gt[k])
    return ba


def _directba_oracle(tc, cap=600000, **kw):
    scene = tc.scene
    orc = ob.OracleBA(cap, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, ob.make_camera(tc.color_camera, tc.color_width, tc.color_height),
                      ob.make_camera(scene.camera, scene.width, scene.height), **kw)
    for k in range(len(scene.depth)):
        orc.add_keyframe(scene.depth[k], scene.rgb[k], scene.poses_gt[k])
    return orc


def test_directba_with_surfel_updates():
    """DirectBA (two cameras at one size; crop's colour camera): BundleAdjustment with do_surfel_updates -- filtered creation, merging,
    deletion and compaction inside BA -- against OracleBA.bundle_adjustment, as tests/test_gpu_directba_vs_oracle.py does: the same
    surfels and poses, bit for bit."""
    tc, _, _, _ = _world("crop")
    orc, ba = _directba_oracle(tc), _directba(tc)
    rng = np.random.Generator(np.random.PCG64(9))
    K = len(tc.scene.poses_gt)
    for k, T in enumerate(tc.scene.poses_gt):
        T = synthetic.perturb_pose(rng, T, 0.002, 0.0005)
        orc.set_pose(k, T)
        ba.set_keyframe_pose(k, T)
    orc.covis = [ba.keyframe_covisibility(k) for k in range(K)]
    orc.spatial_sort_cell, orc.unsorted_surfels = 0.02, ba.unsorted_surfels()
    for call in range(2):
        ba.BundleAdjustment(do_surfel_updates=True, min_iterations=2, max_iterations=2, increase_ba_iteration_count=True)
        orc.bundle_adjustment(do_surfel_updates=True, min_iterations=2, max_iterations=2, increase_ba_iteration_count=True)
        assert ba.surfel_count() == orc.surfels_size, (call, ba.surfel_count(), orc.surfels_size)
    assert orc.surfels_size > 10000
    assert np.array_equal(np.asarray([ba.keyframe_pose(k) for k in range(K)], np.float32), np.asarray([orc.pose(k) for k in range(K)], np.float32))
    got, ref = ba.download_surfels(8), orc.surfel_data[:8, :orc.surfels_size]
    assert np.array_equal(_bits(got), _bits(ref))
    # the colour camera sees less than the depth camera: pairs without a colour pixel were part of every sweep
    idx = np.arange(orc.surfels_size, dtype=np.uint32)
    words = np.concatenate([orc.evaluate_pairs(k, idx) for k in range(K)])
    assert ((words[:, 0] != 0) & (words[:, 3] == 0)).sum() > 0.2 * (words[:, 0] != 0).sum()


def test_directba_with_intrinsics_optimisation():
    """Two iterations of the alternating scheme over geometry, poses, depth intrinsics + deformation and colour intrinsics on a fixed
    surfel set, cameras 0.5 .. 2 px off: surfels, poses, cameras, a and the cfactor image the oracle's bits."""
    tc, _, _, _ = _world("crop")
    _, state = _fresh("crop", "active")
    n, K = state.surfels_size, len(state.keyframes)
    data = state.surfel_data[:, :n].copy()
    orc, ba = _directba_oracle(tc), _directba(tc)
    orc.surfel_data[:, :n] = data
    orc.surfels.surfels_size = orc.surfels.surfel_count = n
    orc.active[:n] = 1
    ba.upload_surfels(data[:8])
    for k in range(K):
        orc.set_pose(k, state.pose(k))
        ba.set_keyframe_pose(k, state.pose(k))
    depth_cam = np.asarray(tc.scene.camera, np.float64) + np.array([0.5, -0.6, 1.23, -2.17])
    color_cam = np.asarray(tc.color_camera, np.float64) + np.array([0.4, -0.3, 0.8, -0.6])
    ba.set_cameras(color_cam, depth_cam, 0.0)
    for name, values in (("depth_cam", depth_cam), ("color_cam", color_cam)):
        c = getattr(orc, name)
        c.fx, c.fy, c.cx, c.cy = [float(np.float32(v)) for v in values]
    ba.set_ba_iteration_counts(1, 1)
    orc.ba_iteration_count, orc.last_ba_iteration_count = 1, 1
    orc.use_depth, orc.use_desc = 1, 1
    call = dict(optimize_depth_intrinsics=True, optimize_color_intrinsics=True, do_surfel_updates=False, optimize_poses=True,
                optimize_geometry=True, min_iterations=2, max_iterations=2, increase_ba_iteration_count=False)
    done, _ = ba.BundleAdjustment(active_keyframe_window_start=0, active_keyframe_window_end=K - 1, **call)
    stats = orc.bundle_adjustment(**call)
    assert done == stats.iterations_done == 2
    assert np.array_equal(_bits(ba.download_surfels(8)), _bits(orc.surfel_data[:8, :n]))
    assert np.array_equal(np.asarray([ba.keyframe_pose(k) for k in range(K)], np.float32), np.asarray([orc.pose(k) for k in range(K)], np.float32))
    cc, dc, a = ba.cameras()
    # (geometry and poses go first and absorb most of the offset: the intrinsics steps move the cameras by hundredths of a pixel --
    # a thousand binary32 ulps of fx = 120 -- not by the tenths bahip_optimize_intrinsics alone moves them in test_intrinsics_step)
    assert np.abs(_cam(orc.depth_cam) - depth_cam).max() > 1e-2 and np.abs(_cam(orc.color_cam) - color_cam).max() > 1e-2
    assert np.array_equal(_bits(dc), _bits(_cam(orc.depth_cam))), (dc, _cam(orc.depth_cam))
    assert np.array_equal(_bits(cc), _bits(_cam(orc.color_cam))), (cc, _cam(orc.color_cam))
    assert np.array_equal(_bits([a]), _bits([orc.dp.a]))
    assert np.array_equal(_bits(ba.cfactor()), _bits(orc.cfactor))


# ---- the fast flavour ---------------------------------------------------------------------------------------------------------------
def _hook(g, ba, arithmetic):
    g.ctx.set_arithmetic(arithmetic)
    try:
        idx = np.arange(g.surfels_size, dtype=np.uint32)
        return [g.evaluate_pairs(k, idx, _frame(ba, k)) for k in range(len(g.keyframes))]
    finally:
        g.ctx.set_arithmetic("exact")


@pytest.mark.parametrize("name", ["tiny", "crop"])
def test_fast_flavour(name):
    """The fast flavour on tiny and crop: the same bits call after call and for every launch shape (cost, pose normal equations, geometry
    step); at most 1e-3 of the pairs flip association or colour validity against the exact flavour; the cost sums within 1e-5 relative
    plus the per-flip slack of tests/test_gpu_cost.py::test_the_fast_flavour_is_deterministic_and_close_to_the_exact_one; the residuals
    within two_cameras.MODEL_RESIDUAL_BOUND of the float64 model."""
    tc, ba, g, census = _world(name)
    K, n = len(ba.keyframes), ba.surfels_size
    exact = g.evaluate_cost()
    exact_words, fast_words = _hook(g, ba, "exact"), _hook(g, ba, "fast")
    g.ctx.set_arithmetic("fast")
    try:
        fast = g.evaluate_cost()
        assert _keys(g.evaluate_cost()) == _keys(fast)
        _set_shape(2, 7, 2, 0)
        assert _keys(g.evaluate_cost()) == _keys(fast)
        _set_shape()
        sums = {}
        for parts, form in ((0, 0), (1, 0), (8, 0), (0, 2)):
            _launch_shapes(0, parts)
            capi.check(capi.load().bahip_debug_set_pose_form(form))
            sums[(parts, form)] = [np.concatenate(g.accumulate_pose_coeffs(k, True, True, _frame(ba, k))) for k in range(K)]
        for key, value in sums.items():
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(value, sums[(0, 0)])), key
        surfels = {}
        for tile_waves in (1, 4):
            _launch_shapes(tile_waves, 0)
            tc2.sync_gpu(g, ba, active=np.zeros(n, np.uint8))
            g.update_activation_and_optimize_geometry(True, True)
            surfels[tile_waves] = (g.download_surfels()[:8].copy(), g.active_buf.download()[0, :n].copy())
        assert np.array_equal(_bits(surfels[1][0]), _bits(surfels[4][0])) and np.array_equal(surfels[1][1], surfels[4][1])
        dpos = np.abs(surfels[1][0][:3] - ba.surfel_data[:3, :n]).max(axis=0)
        assert (dpos > 0).mean() > 0.5                   # the step did move the surfels
    finally:
        _set_shape()
        _launch_shapes(0, 0)
        capi.check(capi.load().bahip_debug_set_pose_form(0))
        g.ctx.set_arithmetic("exact")
        tc2.sync_gpu(g, ba)
    assert _keys(g.evaluate_cost()) == _keys(exact)
    e, f = exact[0], fast[0]
    depth_flips = sum(int(((a[:, 0] == 1) != (b[:, 0] == 1)).sum()) for a, b in zip(exact_words, fast_words))
    colour = lambda w: (w[:, 0] == 1) & (w[:, 3] == 1)
    desc_flips = sum(int((colour(a) != colour(b)).sum()) for a, b in zip(exact_words, fast_words))
    desc_max = max(float(_huber_costs(np.concatenate([w[colour(w), 14], w[colour(w), 15]])).max()) for w in exact_words + fast_words)
    assert depth_flips <= 1e-3 * e["depth_residuals"] and desc_flips <= 1e-3 * e["descriptor_pairs"], (depth_flips, desc_flips)
    assert abs(f["depth_residuals"] - e["depth_residuals"]) <= depth_flips
    assert abs(f["descriptor_pairs"] - e["descriptor_pairs"]) <= desc_flips
    assert 0 < f["descriptor_pairs"] < f["depth_residuals"]
    for field, slack in (("depth", depth_flips * 100.0 / 6.0), ("descriptor_1", desc_flips * desc_max), ("descriptor_2", desc_flips * desc_max)):
        assert abs(f[field] - e[field]) <= 1e-5 * abs(e[field]) + slack, (field, f[field], e[field], slack)
    totals, worst = np.zeros(4), 0.0
    for k in range(K):
        row = _hook_against_the_model(ba, k, fast_words[k])
        totals += (row[0], row[1], row[2], row[4])
        worst = max(worst, row[3])
    pairs, left_out, mismatches, compared = totals
    print(f"{name}, fast flavour: {depth_flips} association flips, {desc_flips} colour flips, residual deviation from the model {worst:.3e}")
    assert left_out <= tc2.MODEL_MAX_LEFT_OUT * pairs and mismatches == 0 and compared > 0.4 * pairs
    assert worst <= tc2.MODEL_RESIDUAL_BOUND
