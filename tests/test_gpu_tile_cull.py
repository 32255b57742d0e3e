"""The tile cull of the surfel sweeps (badslam_amd/csrc/wave_cull.h) held to its promise -- conservative, never changes a result -- where
a cull goes wrong: at the frustum's edges.  Worlds, model, band and census: tests/tile_cull.py (checked without a GPU by
tests/test_cpu_tile_cull.py): five depth-camera shapes, keyframes whose images are valid out to the outermost pixel, surfels placed by
hand 0.01 .. 0.99 px inside and 0.01 px outside every border, most of them alone in their tile (a 1 cm sphere).

Probe (bahip_debug_tile_cull, the cull as the device compiles it).  Exact flavour: spheres and decisions are the binary32 model's, bit
for bit.  Fast flavour: conservative against the oracle with no band, the model's decisions outside its band, the model's spheres within
the rounding of the approximate square root.  70 keyframes (a second mask word), a prefix of the cloud, an empty cloud, refusals that
write nothing, no allocation left behind.

Sweeps on the edge clouds against the UN-CULLED oracle, with the comparators each stage's own test uses.  Exact flavour: bit for bit.
Fast flavour, on off_image and neg_fy, each stage with the comparator of its own fast-flavour test: the geometry step at one wavefront
is the step at four, bit for bit (also from keyframe 1024 on, where the position pass culls on parked bounds); the pose sums and the
batched pose phase do not depend on the launch form; the controlled pose phase reports bahip_evaluate_cost's bits; the per-surfel cost
sums hold within 1e-5 plus the slack of flipped associations (none flips); the windowed PCG iteration is the whole-map one within 1e-5;
the controlled intrinsics step is its by-hand sequence; supporting surfels, merging, colours and residual images -- one kernel for both
flavours -- are the oracle's bits under a fast context.  On all five shapes the pair counts per keyframe (bahip_evaluate_cost) and per
surfel (bahip_evaluate_surfel_costs) and the activation flags are the exact flavour's, and the cost totals hold within the 1e-5
relative of tests/test_gpu_cost.py's fast-flavour test.  By counts only, for want of a fast-flavour comparator anywhere in the suite:
bahip_optimize_intrinsics (the observation count of every sparse cell is the exact flavour's) and the whole-map bahip_pcg_iteration
(the reference of the windowed comparison).  The probe's fast flavour is the compilation of ITS unit (kernels_cull_probe.hip, built
with flushed denormals; contraction is decided per inlining site): it shows that the formula survives the fast flags, not what each
sweep's own inlined copy decides -- that is what the sweeps' pair counts are for.  Camera shapes: all five for
the geometry step, the pose sums and the cost; off_image and neg_fy for the rest."""
import ctypes as C
import math

import numpy as np
import pytest

from badslam_amd import capi, lowlevel as ll, se3, synthetic
from oracle import binding as ob
from tests import residual_image as ri
from tests import surfel_costs as sc
from tests import tile_cull as tc
from tests import two_cameras as tcam
from tests.test_gpu_cost import _key
from tests.test_gpu_pose_step_control import _f, _same_cost

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = list(tc.SHAPES)
TWO = ["off_image", "neg_fy"]
FILL = 0xA5
_WORLD = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle(name, max_surfels=None, poses=None, images=None):
    """A fresh oracle in the world's state: every keyframe and surfel active, the descriptors 3 units off (so that the geometry step
    and the descriptor residuals have something to do)."""
    w = tc.world(name)
    ba = tc.build_oracle(w, max_surfels=max_surfels, poses=poses, images=images)
    n = ba.surfels_size
    ba.surfel_data[6:8, :n] += np.random.Generator(np.random.PCG64(4)).uniform(-3, 3, (2, n)).astype(F32)
    return ba


def _reference(name):
    """The oracle of a shape that no test writes to (its residual switches stay at depth + descriptors, as built)."""
    if ("oracle", name) not in _WORLD:
        _WORLD[("oracle", name)] = _oracle(name)
    return _WORLD[("oracle", name)]


def _world(name, arithmetic="exact"):
    """(world, the reference oracle, a GPU scene in its state that every test leaves as it found it) per shape and flavour."""
    key = (name, arithmetic)
    if key not in _WORLD:
        _WORLD[key] = (tc.world(name), _reference(name), tc.build_gpu(tc.world(name), _reference(name), arithmetic))
    return _WORLD[key]


def _reset(ba, ref):
    n = ref.surfels_size
    ba.surfel_data[:, :n] = ref.surfel_data[:, :n]
    ba.active[:n] = ref.active[:n]
    ba.surfels.surfels_size, ba.surfels.surfel_count = n, ref.surfels.surfel_count


def _launch_shapes(tile_waves, pose_parts):
    capi.check(capi.load().bahip_debug_set_launch_shapes(tile_waves, pose_parts))


def _pose_form(form):
    capi.check(capi.load().bahip_debug_set_pose_form(form))


def _frame(ba, k):
    return np.array(list(ba.keyframes[k].frame_T_global), F32)


# ---- the probe ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_probe_exact_flavour_is_the_model_bit_for_bit(name):
    w, ba, g = _world(name)
    p = tc.pairs(name)
    assert np.array_equal(_bits(p.frames), _bits(tc.frames_of(ba)))
    bounds, masks = g.tile_cull(prefill=FILL)
    expected = tc.wave_bounds32(w.surfels[:3])
    may, _ = tc.sphere_may_project(F32, w.camera, p.frames, expected)
    assert bounds.shape == (len(w.kinds), 4) and masks.shape == (len(w.kinds), 1)
    assert np.array_equal(_bits(bounds), _bits(expected)), np.flatnonzero((_bits(bounds) != _bits(expected)).any(axis=1))[:10]
    assert np.array_equal(masks, tc.masks_of(may)), np.argwhere(tc.may_of(masks, 8) != may)[:10]
    assert not (tc.per_tile(p.in_image) & ~tc.may_of(masks, 8)).any()
    # without the spheres: the same masks
    none, again = g.tile_cull(want_bounds=False, prefill=FILL)
    assert none is None and np.array_equal(again, masks)


@pytest.mark.parametrize("name", ALL)
def test_probe_fast_flavour_is_conservative_and_the_model_outside_its_band(name):
    w, ba, g = _world(name, "fast")
    assert g.ctx.arithmetic == "fast"
    p = tc.pairs(name)
    bounds, masks = g.tile_cull(prefill=FILL)
    got = tc.may_of(masks, 8)
    # conservative against the oracle: no band
    lost = tc.per_tile(p.in_image) & ~got
    assert not lost.any(), np.argwhere(lost)[:10]
    expected = tc.wave_bounds32(w.surfels[:3])
    b64 = tc.wave_bounds64(w.surfels[:3])
    live = expected[:, 3] >= 0
    assert np.array_equal(_bits(bounds[~live]), _bits(expected[~live]))
    assert np.array_equal(_bits(bounds[:, :3]), _bits(expected[:, :3]))                    # min, max, one addition, a product with 0.5
    scale = np.abs(b64[live]).max()
    tolerance = 4 * 2.0 ** -24 * scale + (7 + tc.SQRT_FAST) * 2.0 ** -24 * b64[live, 3]    # tests/test_cpu_tile_cull.py's bound + the square root's
    assert (np.abs(bounds[live, 3] - b64[live, 3]) <= tolerance).all()
    may, _ = tc.sphere_may_project(F32, w.camera, p.frames, expected)
    band = tc.in_band(w.camera, p.frames, expected, fast=True)
    print(f"{name}: {int(band.sum())} decisions inside the fast band, {int((got != may).sum())} differ from the binary32 model, "
          f"{int((_bits(bounds[:, 3]) != _bits(expected[:, 3])).sum())} radii differ in a bit")
    assert np.array_equal(got[~band], may[~band]), np.argwhere((got != may) & ~band)[:10]


def test_probe_with_70_keyframes_fills_a_second_mask_word():
    w, ba, _ = _world("centred")
    rng = np.random.Generator(np.random.PCG64(70))
    poses = [np.asarray(T, F32) for T in w.poses]
    while len(poses) < 70:
        xi = np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-0.4, 0.4, 3)])
        poses.append(np.asarray(se3.mul(w.poses[len(poses) % 7], se3.exp(xi)), F32))
    g = tc.build_gpu(w, poses=poses)
    n = w.surfels.shape[1]
    g.upload_surfels(w.surfels, np.ones(n, np.uint8))
    frames = np.stack([tc.frame_T_global(T) for T in poses])
    bounds, masks = g.tile_cull(prefill=FILL)
    expected = tc.wave_bounds32(w.surfels[:3])
    may, _ = tc.sphere_may_project(F32, w.camera, frames, expected)
    assert masks.shape == (len(w.kinds), 2) and not (masks[:, 1] >> np.uint64(6)).any()
    assert np.array_equal(_bits(bounds), _bits(expected))
    assert np.array_equal(masks, tc.masks_of(may)), np.argwhere(tc.may_of(masks, 70) != may)[:10]
    second = may[:, 64:]
    assert second.any(axis=0).all() and 0.2 < second.mean() < 0.8, second.mean()           # every late keyframe decides both ways
    g.ctx.set_arithmetic("fast")
    g.set_intrinsics()
    _, fast = g.tile_cull(prefill=FILL)
    band = tc.in_band(w.camera, frames, expected, fast=True)
    assert np.array_equal(tc.may_of(fast, 70)[~band], may[~band])


def test_probe_on_a_prefix_an_empty_cloud_refusals_and_allocations():
    w, ba, g = _world("off_image")
    p = tc.pairs("off_image")
    lib = capi.load()
    before = ll.live_allocations(lib)
    # a prefix that ends inside a tile (and inside that tile's live entries: a compact one)
    compact = int(np.flatnonzero(w.kinds == "compact")[3])
    size = compact * 64 + 23
    bounds, masks = g.tile_cull(size=size, prefill=FILL)
    expected = tc.wave_bounds32(w.surfels[:3, :size])
    may, _ = tc.sphere_may_project(F32, w.camera, p.frames, expected)
    assert bounds.shape == (compact + 1, 4)
    assert np.array_equal(_bits(bounds), _bits(expected)) and np.array_equal(masks, tc.masks_of(may))
    assert not np.array_equal(_bits(expected[compact]), _bits(tc.wave_bounds32(w.surfels[:3])[compact]))
    # an empty cloud: no tile, nothing written
    s = g.surfels_struct(0)
    out_b, out_m = np.full(8, FILL, np.uint8), np.full(16, FILL, np.uint8)
    capi.check(lib.bahip_debug_tile_cull(g.ctx.handle, C.byref(s), out_b.ctypes.data_as(C.POINTER(C.c_float)), out_m.ctypes.data_as(C.POINTER(C.c_uint64))))
    assert (out_b == FILL).all() and (out_m == FILL).all()
    # refusals write nothing: NULL arguments ...
    s = g.surfels_struct()
    tiles = len(w.kinds)
    out_b, out_m = np.full(16 * tiles, FILL, np.uint8), np.full(8 * tiles, FILL, np.uint8)
    pb, pm = out_b.ctypes.data_as(C.POINTER(C.c_float)), out_m.ctypes.data_as(C.POINTER(C.c_uint64))
    for args in ((None, C.byref(s), pb, pm), (g.ctx.handle, None, pb, pm), (g.ctx.handle, C.byref(s), pb, None)):
        assert lib.bahip_debug_tile_cull(*args) != 0
        assert b"bahip_debug_tile_cull" in lib.bahip_last_error()
        assert (out_b == FILL).all() and (out_m == FILL).all()
    # ... and a context without a bound keyframe table
    bare = ll.Scene(ll.Context(), 256, w.spec["scale"], tc.BASELINE_FX, tc.CELL, ll.make_camera(w.camera, tc.W, tc.H), ll.make_camera(w.camera, tc.W, tc.H))
    bare.upload_surfels(w.surfels[:, :128], np.ones(128, np.uint8))
    with pytest.raises(capi.BackendError, match="no keyframes bound") as refused:
        bare.tile_cull(prefill=FILL)
    assert all((a.view(np.uint8) == FILL).all() for a in refused.value.arrays)
    bare.ctx.close()
    del bare
    # the context is as usable as before, and nothing stays allocated
    again_b, again_m = g.tile_cull(size=size, prefill=FILL)
    assert np.array_equal(_bits(again_b), _bits(bounds)) and np.array_equal(again_m, masks)
    import gc
    gc.collect()
    assert ll.live_allocations(lib) == before


# ---- the sweeps: exact flavour, bit for bit against the un-culled oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_activation_and_geometry_step(name, request):
    """Activation flags and the eight surfel rows after the geometry step: one and four wavefronts per tile, the fused call and the two
    calls, with descriptors and without.  (With eight keyframes the position pass replays the normals pass's candidate masks: the cull on
    parked bounds is test_geometry_step_beyond_the_replayed_masks's.)"""
    w, ref, g = _world(name)
    ba = _oracle(name)
    n = ref.surfels_size
    request.addfinalizer(lambda: (_launch_shapes(0, 0), tcam.sync_gpu(g, ref)))
    expected = {}
    for use_desc in (True, False):
        _reset(ba, ref)
        ba.active[:n] = 0
        ba.use_depth, ba.use_desc = 1, int(use_desc)
        ba.update_surfel_activation()
        flags = ba.active[:n].copy()
        ba.optimize_geometry_iteration()
        expected[use_desc] = (flags, ba.active[:n].copy(), ba.surfel_data[:8, :n].copy())
    live = ref.surfel_data[0, :n] == ref.surfel_data[0, :n]
    flags, _, rows = expected[True]
    assert flags[live].mean() > 0.9 and not flags[~live].any()
    assert (_bits(rows[:3]) != _bits(ref.surfel_data[:3, :n])).any(axis=0).sum() > 1000
    assert (_bits(rows[6:8]) != _bits(ref.surfel_data[6:8, :n])).any(axis=0).sum() > 1000
    for tile_waves in (1, 4):
        for fused in (False, True):
            for use_desc in (True, False):
                flags, active, rows = expected[use_desc]
                tcam.sync_gpu(g, ref, active=np.zeros(n, np.uint8))
                _launch_shapes(tile_waves, 0)
                if fused:
                    g.update_activation_and_optimize_geometry(True, use_desc)
                else:
                    g.update_surfel_activation()
                    assert np.array_equal(g.active_buf.download()[0, :n], flags), (tile_waves, use_desc)
                    g.optimize_geometry_iteration(True, use_desc)
                what = (tile_waves, fused, use_desc)
                assert np.array_equal(g.active_buf.download()[0, :n], active), what
                got = g.download_surfels()[:8]
                assert np.array_equal(_bits(got), _bits(rows)), (what, np.flatnonzero((_bits(got) != _bits(rows)).any(axis=0))[:10])


LATE_FILLERS = 1032            # keyframes that look away, ahead of the world's eight: those sit at 1032 .. 1039, in the fifth chunk of every sum class


@pytest.mark.parametrize("name", TWO)
def test_geometry_step_beyond_the_replayed_masks(name, request):
    """From keyframe 1024 on (four sum classes, kMaskChunks = 4) the position pass of the one-wavefront geometry kernel no longer replays
    the normals pass's candidate masks: with descriptors it tests those keyframes itself, on the bounding sphere it parked in LDS and
    with intrinsics the compiler cannot see through (kernels_surfel.hip: kParked).  Here the only keyframes that see the edge clouds ARE
    the ones beyond 1024, so every position and descriptor update passes through that cull: the oracle's bits in the exact flavour,
    fused or not; in the fast flavour the four-wavefront shape's bits (which parks nothing) and the exact flavour's flags."""
    w = tc.world(name)
    poses = [w.poses[7]] * LATE_FILLERS + list(w.poses)
    images = [w.images[7]] * LATE_FILLERS + list(w.images)
    ba = _oracle(name, poses=poses, images=images)
    n = ba.surfels_size
    start = ba.surfel_data[:, :n].copy()
    live = start[0] == start[0]
    ba.active[:n] = 0
    ba.use_depth, ba.use_desc = 1, 1
    ba.update_surfel_activation()
    ba.optimize_geometry_iteration()
    flags, rows = ba.active[:n].copy(), ba.surfel_data[:8, :n].copy()
    assert flags[live].mean() > 0.9
    assert (_bits(rows[:3]) != _bits(start[:3])).any(axis=0).sum() > 1000 and (_bits(rows[6:8]) != _bits(start[6:8])).any(axis=0).sum() > 1000
    ba.surfel_data[:, :n] = start
    g = tc.build_gpu(w, ba, poses=poses, images=images)
    assert len(g.keyframes) == LATE_FILLERS + 8
    request.addfinalizer(lambda: _launch_shapes(0, 0))
    zeros = np.zeros(n, np.uint8)

    def step(tile_waves, fused):
        tcam.sync_gpu(g, ba, active=zeros)
        _launch_shapes(tile_waves, 0)
        if fused:
            g.update_activation_and_optimize_geometry(True, True)
        else:
            g.update_surfel_activation()
            g.optimize_geometry_iteration(True, True)
        return g.download_surfels()[:8].copy(), g.active_buf.download()[0, :n].copy()

    for fused in (False, True):
        got, active = step(1, fused)
        assert np.array_equal(active, flags), fused
        assert np.array_equal(_bits(got), _bits(rows)), (fused, np.flatnonzero((_bits(got) != _bits(rows)).any(axis=0))[:10])
    g.ctx.set_arithmetic("fast")
    g.set_intrinsics()
    for fused in (False, True):
        four, one = step(4, fused), step(1, fused)
        assert np.array_equal(_bits(one[0]), _bits(four[0])) and np.array_equal(one[1], four[1]), fused
        assert np.array_equal(one[1], flags), fused
        assert (_bits(one[0][:3]) != _bits(start[:3])).any(axis=0).sum() > 1000


@pytest.mark.parametrize("name", ALL)
def test_pose_normal_equations(name, request):
    """H and b of every keyframe in forms 1 and 2 with pose_parts 1 and 4: the oracle's defined sum, bit for bit."""
    w, ba, g = _world(name)
    request.addfinalizer(lambda: (_launch_shapes(0, 0), _pose_form(0)))
    K = len(ba.keyframes)
    reference = [ba.accumulate_pose_coeffs(k, accumulate_double=False) for k in range(K)]
    assert sum(1 for r in reference if r[2] > 300) >= 7 and reference[7][2] < 10           # the keyframe that looks away sees next to nothing
    for form in (1, 2):
        for parts in (1, 4):
            _pose_form(form)
            _launch_shapes(0, parts)
            for k in range(K):
                H, b = g.accumulate_pose_coeffs(k, True, True, _frame(ba, k))
                assert np.array_equal(_bits(H), _bits(reference[k][0])), (form, parts, k, np.abs(H - reference[k][0]).max())
                assert np.array_equal(_bits(b), _bits(reference[k][1])), (form, parts, k, np.abs(b - reference[k][1]).max())


def _perturbed(name, seed=11):
    """A fresh oracle with the poses 5 mm / 1 mrad off; the keyframe that looks away (it sees no surfel) takes no part."""
    w = tc.world(name)
    ba = _oracle(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in range(7):
        ba.set_pose(k, synthetic.perturb_pose(rng, w.poses[k]))
    ba.keyframes[7].activation = ob.KF_INACTIVE
    return ba


@pytest.mark.parametrize("name", TWO)
def test_batched_pose_estimation(name, request):
    """bahip_estimate_keyframe_poses from perturbed poses: every keyframe ends on the pose of the oracle's estimate_frame_pose after the
    same number of steps; at least two rounds, so the later rounds run on the bounds the first round stored."""
    w, ref, g = _world(name)
    ba = _perturbed(name)
    request.addfinalizer(lambda: tcam.sync_gpu(g, ref))
    tcam.sync_gpu(g, ba)
    poses, its, conv, rounds = g.estimate_keyframe_poses(True, True)
    assert rounds >= 2
    for k in range(7):
        est, its_ref, conv_ref = ba.estimate_frame_pose(k, ba.pose(k))
        assert np.array_equal(_bits(poses[k]), _bits(est.to_array())), (k, poses[k], est.to_array())
        assert its[k] == its_ref and conv[k] == int(conv_ref), (k, its[k], its_ref)
    assert rounds == its.max() and (its[:7] >= 2).sum() >= 4, its


@pytest.mark.parametrize("name", TWO)
def test_controlled_pose_phase(name, request):
    """bahip_estimate_keyframe_poses_controlled (the fused sweep with cull_intrinsics and its own stored bounds): cost_before / cost_after
    are bahip_evaluate_cost's entries, no objective rises, and with lambda = 0 a keyframe without a rejected candidate takes the plain
    phase's pose and iteration count -- which test_batched_pose_estimation holds to the oracle."""
    w, ref, g = _world(name)
    ba = _perturbed(name)
    request.addfinalizer(lambda: tcam.sync_gpu(g, ref))
    control = (4.0, 0.5, 0.0, 1e6, 4)
    tcam.sync_gpu(g, ba)
    plain_poses, plain_its, plain_conv, _ = g.estimate_keyframe_poses(True, True)
    tcam.sync_gpu(g, ba)
    start = [np.asarray(kf["pose"], F32).copy() for kf in g.keyframes]
    before = g.evaluate_cost(True, True)[1]
    out = g.estimate_keyframe_poses_controlled([0.0] * 8, control)
    after = g.evaluate_cost(True, True)[1]
    assert out["iterations"][:7].sum() > 0 and out["rounds"] >= 2
    for k in range(7):
        assert _same_cost(out["cost_before"][k], before[k]), (k, out["cost_before"][k], before[k])
        assert _same_cost(out["cost_after"][k], after[k]), (k, out["cost_after"][k], after[k])
    for k in range(7):                                                 # no objective rises; it stays exactly where no step was accepted
        fb, fa = _f(out["cost_before"][k]), _f(out["cost_after"][k])
        if out["iterations"][k] == 0:
            assert _same_cost(out["cost_before"][k], out["cost_after"][k]) and np.array_equal(_bits(out["poses"][k]), _bits(start[k])), k
        else:
            assert fa < fb, (k, fb, fa)
            assert out["trials"][k] == out["iterations"][k] + out["rejected"][k]
    clean = [k for k in range(7) if out["rejected"][k] == 0]
    print(f"{name}: {len(clean)} of 7 keyframes without a rejected candidate; iterations {list(out['iterations'])}, plain {list(plain_its)}")
    assert len(clean) >= 3
    for k in clean:
        assert np.array_equal(_bits(out["poses"][k]), _bits(plain_poses[k])), k
        assert out["iterations"][k] == plain_its[k] and out["converged"][k] == plain_conv[k], k


def _expected_costs(words):
    """Per keyframe and in total the exact sums (math.fsum) of the robust costs of the ORACLE's pair words."""
    per, terms = [], [[], [], []]
    for kw in words:
        associated, paired, depth, desc1, desc2 = sc.pair_terms(kw)
        parts = [depth[associated].astype(np.float64), desc1[paired].astype(np.float64), desc2[paired].astype(np.float64)]
        for t, v in zip(terms, parts):
            t.append(v)
        per.append(dict(depth=math.fsum(parts[0]), descriptor_1=math.fsum(parts[1]), descriptor_2=math.fsum(parts[2]),
                        depth_residuals=int(associated.sum()), descriptor_pairs=int(paired.sum())))
    total = dict(depth=math.fsum(np.concatenate(terms[0])), descriptor_1=math.fsum(np.concatenate(terms[1])),
                 descriptor_2=math.fsum(np.concatenate(terms[2])), depth_residuals=sum(c["depth_residuals"] for c in per),
                 descriptor_pairs=sum(c["descriptor_pairs"] for c in per))
    return total, per


def _pair_words(name):
    key = ("words", name)
    if key not in _WORLD:
        _WORLD[key] = sc.oracle_pair_words(_world(name)[1])
    return _WORLD[key]


@pytest.mark.parametrize("name", ALL)
def test_cost(name):
    """bahip_evaluate_cost: per keyframe and in total the exact sums of the oracle's per-pair terms, and the oracle's own value."""
    w, ba, g = _world(name)
    total, per = g.evaluate_cost(True, True)
    exp_total, exp_per = _expected_costs(_pair_words(name))
    assert exp_total["depth_residuals"] == int(tc.pairs(name).associated.sum()) > 10000
    for k, (got, exp) in enumerate(zip(per, exp_per)):
        assert _key(got) == _key(exp), (k, got, exp)
        assert _key(g.evaluate_frame_cost(k, _frame(ba, k))) == _key(got), k
    assert _key(total) == _key(exp_total), (total, exp_total)
    value, count = ba.evaluate_cost()
    assert total["depth_residuals"] + 2 * total["descriptor_pairs"] == count
    mine = total["depth"] + total["descriptor_1"] + total["descriptor_2"]
    assert abs(mine - value) <= 1e-9 * abs(value), (mine, value)


@pytest.mark.parametrize("name", TWO)
def test_surfel_costs(name):
    w, ba, g = _world(name)
    for use_depth, use_desc in sc.KINDS:
        got = g.evaluate_surfel_costs(use_depth, use_desc, prefill=0xFF)
        expected = sc.model(_pair_words(name), use_depth, use_desc)
        sc.assert_same_bits(got, expected, (name, use_depth, use_desc))
    assert sc.totals(expected)["descriptor_pairs"] > 5000


def _cam(c):
    return np.array([c.fx, c.fy, c.cx, c.cy], np.float64)


@pytest.mark.parametrize("name", TWO)
def test_intrinsics_step(name):
    """bahip_optimize_intrinsics, depth and colour, cameras a few tenths of a pixel off and a != 0: the sums, the cameras, a and the
    cfactor image are the oracle's bits."""
    w = tc.world(name)
    ba = _oracle(name)
    for cam, off in ((ba.depth_cam, (0.05, -0.06, 0.123, -0.217)), (ba.color_cam, (0.04, -0.03, 0.08, -0.06))):
        cam.fx += off[0]; cam.fy += off[1]; cam.cx += off[2]; cam.cy += off[3]
    ba.dp.a = 0.0125
    ba.cfactor[:] = np.random.Generator(np.random.PCG64(5)).uniform(-2e-3, 2e-3, ba.cfactor.shape).astype(F32)
    ba.use_depth, ba.use_desc = 1, 1
    g = tc.build_gpu(w, ba)
    glob, cells = ba.intrinsics_accumulators(True, True)
    cc_r, dc_r, a_r = ba.optimize_intrinsics(True, True)
    cc_g, dc_g, a_g = g.optimize_intrinsics(True, True)
    got, got_cells = g.read_intrinsics_sums()
    assert np.isfinite(glob).all() and np.count_nonzero(glob) == 34
    assert np.array_equal(_bits(got), _bits(glob.astype(F32))), np.flatnonzero(_bits(got) != _bits(glob.astype(F32)))
    assert np.array_equal(_bits(got_cells), _bits(cells.astype(F32)))
    assert np.array_equal(_bits(_cam(dc_g)), _bits(_cam(dc_r))), (_cam(dc_g), _cam(dc_r))
    assert np.array_equal(_bits(_cam(cc_g)), _bits(_cam(cc_r))), (_cam(cc_g), _cam(cc_r))
    assert np.array_equal(_bits([a_g]), _bits([a_r])) and np.array_equal(_bits(g.cfactor.download()), _bits(ba.cfactor))
    assert np.isfinite(_cam(dc_r)).all() and np.isfinite(_cam(cc_r)).all()


@pytest.mark.parametrize("name", TWO)
def test_pcg(name):
    """bahip_pcg_iteration with 0 inner steps (the assembled r and M, every entry) and with 1 (surfels and poses after the step), and the
    windowed form with everything active, which must be the whole-map one.  The keyframe that looks away is the gauge."""
    w = tc.world(name)
    ba = _oracle(name)
    rng = np.random.Generator(np.random.PCG64(33))
    for k in range(7):
        ba.set_pose(k, synthetic.perturb_pose(rng, w.poses[k], 0.003, 0.0005))
    ba.use_depth, ba.use_desc = 1, 1
    ba.last_ba_iteration_count = ba.ba_iteration_count                 # no end-of-scheme tasks ahead of the iteration
    N, K = ba.surfels_size, len(ba.keyframes)
    g, h = tc.build_gpu(w, ba), tc.build_gpu(w, ba)
    r_ref, M_ref = ba.pcg_assemble(True, True, False, False, gauge_keyframe=7)
    g.pcg_iteration(max_inner_iterations=0, gauge_keyframe=7)
    U = len(r_ref)
    assert U == 6 * (K - 1) + 3 * N
    r, M = g.read_pcg_vector(0, U), g.read_pcg_vector(1, U)
    assert np.array_equal(_bits(r), _bits(r_ref)), np.flatnonzero(_bits(r) != _bits(r_ref))[:10]
    assert np.array_equal(_bits(M), _bits(M_ref)), np.flatnonzero(_bits(M) != _bits(M_ref))[:10]
    assert np.count_nonzero(r_ref[:6 * (K - 1)]) == 6 * (K - 1)
    tcam.sync_gpu(g, ba)                                               # (0 inner steps apply a zero step; start again from the oracle's words)
    before = ba.surfel_data[:8, :N].copy()
    stats = ba.bundle_adjustment(optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=1, use_pcg=True,
                                 increase_ba_iteration_count=False, pcg_max_inner_iterations=1, pcg_gauge_keyframe=7)
    assert stats.pcg_inner_steps_total == 1
    expected = ba.surfel_data[:8, :N]
    assert (_bits(expected[:3]) != _bits(before[:3])).any(axis=0).sum() > 1000
    for what, scene, windowed in (("whole map", g, False), ("windowed", h, True)):
        scene.update_surfel_normals()
        steps, _ = scene.pcg_iteration(max_inner_iterations=1, gauge_keyframe=7, windowed=windowed)
        assert steps == 1, what
        got = scene.download_surfels()[:8]
        assert np.array_equal(_bits(got), _bits(expected)), (what, np.flatnonzero((_bits(got) != _bits(expected)).any(axis=0))[:10])
        for k in range(K):
            assert np.array_equal(_bits(scene.keyframes[k]["pose"]), _bits(ba.pose(k))), (what, k)


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
@pytest.mark.parametrize("name", TWO)
def test_supporting_surfels_and_a_merge_batch(name, arithmetic):
    """The supporting-surfel lists of two keyframes, and a merge batch over five (the tile lists of a batch that knows its frames come
    from the cull) on the cloud plus a near-duplicate, 1 mm off, of every live surfel: the oracle's lists and the oracle's deletions.
    The lifecycle kernels exist once: a context set to the fast flavour must give the oracle's bits as well."""
    w, ref = tc.world(name), _reference(name)
    n = ref.surfels_size
    live = np.flatnonzero(ref.surfel_data[0, :n] == ref.surfel_data[0, :n])
    dup = ref.surfel_data[:, live].copy()
    dup[:3] += np.random.Generator(np.random.PCG64(3)).normal(0, 0.001, (3, len(live))).astype(F32)
    both = np.concatenate([ref.surfel_data[:, :n], dup], axis=1)
    m = both.shape[1]
    ba = _oracle(name, max_surfels=m + 64)
    ba.surfel_data[:, :m] = both
    ba.surfels.surfels_size, ba.surfels.surfel_count = m, 2 * len(live)
    ba.active[:m] = 0
    g = tc.build_gpu(w, ba, arithmetic, capacity=m + 64)
    assert g.ctx.arithmetic == arithmetic
    g.surfel_count = 2 * len(live)
    for k in (0, 6):
        planes, merged = g.determine_supporting_surfels(k, _frame(ba, k), merge=False)
        expected = ba.determine_supporting_surfels(k, merge=False)
        assert merged == 0 and np.array_equal(planes, expected), k
        assert (expected[0] != 0xffffffff).sum() > 200 and (expected[1] != 0xffffffff).sum() > 100
    order = (0, 6, 3, 1, 0)
    Fs = [_frame(ba, k) for k in order]
    before = int(ba.surfels.surfel_count)
    with g.lifecycle_batch(frames=Fs):
        planes, merged = g.merge_surfels_for_keyframes(order, Fs, merge_dist_factor=ba.merge_factor)
    for k in order:
        ba.determine_supporting_surfels(k, merge=True)
    assert merged == before - int(ba.surfels.surfel_count) > 300, merged
    got = g.surfel_buf.download()[:8, :m]
    assert np.array_equal(_bits(got), _bits(ba.surfel_data[:8, :m])), np.flatnonzero((_bits(got) != _bits(ba.surfel_data[:8, :m])).any(axis=0))[:10]


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
@pytest.mark.parametrize("name", TWO)
def test_assign_colors(name, arithmetic, request):
    """bahip_assign_colors (one kernel for both flavours): the oracle's colours under either setting of the context."""
    w, ref, g = _world(name, arithmetic)
    ba = _oracle(name)
    n = ba.surfels_size
    ba.surfel_data[5, :n] = np.random.Generator(np.random.PCG64(13)).integers(0, 2 ** 32, n, dtype=np.uint32).view(F32)
    before = ba.surfel_data[:8, :n].copy()
    request.addfinalizer(lambda: tcam.sync_gpu(g, ref))
    tcam.sync_gpu(g, ba)
    g.assign_colors()
    got = g.download_surfels()[:8]
    ba.assign_colors()
    expected = ba.surfel_data[:8, :n]
    assert np.array_equal(_bits(got), _bits(expected))
    changed = _bits(expected[5]) != _bits(before[5])
    live = before[0] == before[0]
    assert changed[live].mean() > 0.9 and not changed[~live].any()


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
@pytest.mark.parametrize("name", TWO)
def test_residual_image_on_every_keyframe(name, arithmetic):
    """All seven planes on every keyframe under both selects: the model's bits, and under the fast flavour too (the unit exists once, as
    tests/test_gpu_residual_image.py::test_the_fast_flavour_gives_the_exact_flavours_planes holds it)."""
    w, ba, g = _world(name, arithmetic)
    assert g.ctx.arithmetic == arithmetic
    explained = 0
    for k in range(len(ba.keyframes)):
        pairs = ri.from_oracle(ba, k)
        for select in (ri.BEST, ri.WORST):
            expected = ri.image(pairs, tc.W, tc.H, select)
            got = g.residual_image(k, _frame(ba, k), select=select, prefill=FILL)
            ri.assert_same_bits(got, expected, (name, k, select))
        explained += expected["stats"]["explained"]
        # the outermost ring is explained too
        ring = np.ones((tc.H, tc.W), bool)
        ring[1:-1, 1:-1] = False
        if k < 7:
            assert (expected["pairs"][ring] > 0).sum() >= 20, k
    assert explained > 2000


# ---- the sweeps: fast flavour ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_fast_flavour_counts_the_exact_flavours_pairs(name):
    """Per keyframe and per surfel the fast flavour associates the pairs the exact flavour does (a culled pair would be missing from
    both counts), activates the same surfels, and its cost sums over all keyframes hold within 1e-5 relative of the exact flavour's (the
    bound tests/test_gpu_cost.py's fast-flavour test puts on those totals when no association flips).  Measured on an MI355X: depth
    totals within 2.3e-6, descriptor totals within 2.2e-7.  The sums of single keyframes are printed, not bounded: their depth sums
    differ by up to 1.2e-5 (2 277 pairs) and by 3.1e-5 on the keyframe that sees two surfels -- the residual of a surfel a millimetre
    off the surface is a difference of nearly equal numbers."""
    w, ba, g = _world(name)
    _, _, f = _world(name, "fast")
    n = ba.surfels_size
    exact_total, exact_per = g.evaluate_cost(True, True)
    fast_total, fast_per = f.evaluate_cost(True, True)
    fields = ("depth", "descriptor_1", "descriptor_2")
    for k, (e, c) in enumerate(zip(exact_per + [exact_total], fast_per + [fast_total])):
        print(name, "total" if k == len(exact_per) else f"keyframe {k}", e["depth_residuals"], e["descriptor_pairs"],
              ["%.2e" % (abs(c[field] - e[field]) / abs(e[field]) if e[field] else 0.0) for field in fields])
        assert (c["depth_residuals"], c["descriptor_pairs"]) == (e["depth_residuals"], e["descriptor_pairs"]), (k, c, e)
    for field in fields:           # the sums over all keyframes, as that test compares them
        assert abs(fast_total[field] - exact_total[field]) <= 1e-5 * abs(exact_total[field]), (field, fast_total[field], exact_total[field])
    assert exact_total["depth_residuals"] > 10000
    counts = ("depth_residuals", "descriptor_pairs")
    exact_counts, fast_counts = g.evaluate_surfel_costs(planes=counts, prefill=0xFF), f.evaluate_surfel_costs(planes=counts, prefill=0xFF)
    for plane in counts:
        assert np.array_equal(fast_counts[plane], exact_counts[plane]), (plane, np.flatnonzero(fast_counts[plane] != exact_counts[plane])[:10])
    try:
        flags = []
        for scene in (g, f):
            tcam.sync_gpu(scene, ba, active=np.zeros(n, np.uint8))
            scene.update_surfel_activation()
            flags.append(scene.active_buf.download()[0, :n].copy())
    finally:
        tcam.sync_gpu(g, ba)
        tcam.sync_gpu(f, ba)
    assert np.array_equal(flags[0], flags[1]) and flags[0].sum() > 3000


# The stages below run in the fast flavour on the edge clouds with the comparators of their own fast-flavour tests.  The stages with one
# kernel for both flavours -- supporting surfels and merging, colours, residual images -- are held to the oracle's bits under a fast
# context above.  bahip_optimize_intrinsics and the whole-map bahip_pcg_iteration have no fast-flavour comparator against the oracle
# anywhere in the suite: here the intrinsics sweep's observation counts per cell are the exact flavour's and the controlled step is its
# by-hand sequence (tests/test_gpu_intrinsics_step_control.py), and the whole-map PCG iteration is the reference the windowed one is
# held to (tests/test_gpu_pcg_window.py).
def _flags_and_rows_after_the_exact_step(name):
    ref = _reference(name)
    n = ref.surfels_size
    out = {}
    for use_desc in (True, False):
        ba = _oracle(name)
        ba.active[:n] = 0
        ba.use_depth, ba.use_desc = 1, int(use_desc)
        ba.update_surfel_activation()
        ba.optimize_geometry_iteration()
        out[use_desc] = (ba.active[:n].copy(), ba.surfel_data[:8, :n].copy())
    return out


@pytest.mark.parametrize("name", TWO)
def test_fast_geometry_step_at_one_wavefront_is_the_step_at_four(name, request):
    """tests/test_gpu_geometry_parked_state.py's and tests/test_gpu_two_cameras.py's rule for the fast flavour: the one-wavefront shape
    gives the four-wavefront shape's bits, fused or not, with and without descriptors.  And the flags are the exact flavour's.  The
    distance to the exact flavour's positions is printed, not bounded: without descriptors it stays within 4.8e-7 m, with them the 99.9th
    percentile is 1.1e-3 m (off_image) and 8.7e-3 m (neg_fy) -- on these 80 x 60 images of a texture finer than a pixel the ORACLE's own
    step moves 68 / 624 surfels by more than a millimetre (up to 2.2 cm) when every input word goes up by one ulp."""
    w, ref, f = _world(name, "fast")
    n = ref.surfels_size
    request.addfinalizer(lambda: (_launch_shapes(0, 0), tcam.sync_gpu(f, ref)))
    exact = _flags_and_rows_after_the_exact_step(name)
    live = ref.surfel_data[0, :n] == ref.surfel_data[0, :n]
    for use_desc in (True, False):
        for fused in (False, True):
            runs = {}
            for tile_waves in (4, 1):
                tcam.sync_gpu(f, ref, active=np.zeros(n, np.uint8))
                _launch_shapes(tile_waves, 0)
                if fused:
                    f.update_activation_and_optimize_geometry(True, use_desc)
                else:
                    f.update_surfel_activation()
                    f.optimize_geometry_iteration(True, use_desc)
                runs[tile_waves] = (f.download_surfels()[:8].copy(), f.active_buf.download()[0, :n].copy())
            what = (use_desc, fused)
            assert np.array_equal(_bits(runs[1][0]), _bits(runs[4][0])), (what, np.flatnonzero((_bits(runs[1][0]) != _bits(runs[4][0])).any(axis=0))[:10])
            assert np.array_equal(runs[1][1], runs[4][1]), what
            assert np.array_equal(runs[1][1], exact[use_desc][0]), what
            moved = (_bits(runs[1][0][:3]) != _bits(ref.surfel_data[:3, :n])).any(axis=0)
            assert moved[live].mean() > 0.9 and not moved[~live].any(), what
            dpos = np.abs(runs[1][0][:3, live] - exact[use_desc][1][:3, live]).max(axis=0)
            print(name, what, "fast against exact positions: 99.9th percentile %.2e m, max %.2e m" % (np.percentile(dpos, 99.9), dpos.max()))


@pytest.mark.parametrize("name", TWO)
def test_fast_pose_sums_do_not_depend_on_the_launch_form(name, request):
    """tests/test_gpu_two_cameras.py::test_fast_flavour's rule: H and b of every keyframe, the same bits in forms 1 and 2 with pose_parts
    1 and 4."""
    w, ba, f = _world(name, "fast")
    request.addfinalizer(lambda: (_launch_shapes(0, 0), _pose_form(0)))
    sums = {}
    for form in (1, 2):
        for parts in (1, 4):
            _pose_form(form)
            _launch_shapes(0, parts)
            sums[(form, parts)] = [np.concatenate(f.accumulate_pose_coeffs(k, True, True, _frame(ba, k))) for k in range(8)]
    for key, value in sums.items():
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(value, sums[(1, 1)])), key
    exact = [np.concatenate(ba.accumulate_pose_coeffs(k, accumulate_double=False)[:2]) for k in range(7)]
    worst = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(sums[(1, 1)][:7], exact))
    print(name, "fast pose sums against the exact ones: %.2e of the largest entry" % worst)
    assert all(np.abs(v).max() > 0 for v in sums[(1, 1)][:7])


@pytest.mark.parametrize("name", TWO)
def test_fast_batched_pose_estimation_does_not_depend_on_the_pose_form(name, request):
    """tests/test_gpu_fast_flavour.py's rule (deterministic, launch-shape invariant) on the phase whose later rounds use stored bounds."""
    w, ref, f = _world(name, "fast")
    ba = _perturbed(name)
    request.addfinalizer(lambda: (_pose_form(0), tcam.sync_gpu(f, ref)))
    runs = []
    for form in (1, 2, 1):
        _pose_form(form)
        tcam.sync_gpu(f, ba)
        runs.append(f.estimate_keyframe_poses(True, True))
    for poses, its, conv, rounds in runs[1:]:
        assert np.array_equal(_bits(poses), _bits(runs[0][0])) and np.array_equal(its, runs[0][1]) and np.array_equal(conv, runs[0][2])
        assert rounds == runs[0][3] >= 2


@pytest.mark.parametrize("name", TWO)
def test_fast_controlled_pose_phase_reports_the_cost_sweeps_bits(name, request):
    """tests/test_gpu_pose_step_control.py::test_cost_bits[fast]: cost_before / cost_after are bahip_evaluate_cost's entries."""
    w, ref, f = _world(name, "fast")
    ba = _perturbed(name)
    request.addfinalizer(lambda: tcam.sync_gpu(f, ref))
    tcam.sync_gpu(f, ba)
    before = f.evaluate_cost(True, True)[1]
    out = f.estimate_keyframe_poses_controlled([1e-3] * 8, (4.0, 0.5, 0.0, 1e6, 4))
    after = f.evaluate_cost(True, True)[1]
    assert out["iterations"][:7].sum() > 0 and out["rounds"] >= 2
    for k in range(7):
        assert _same_cost(out["cost_before"][k], before[k]), (k, out["cost_before"][k], before[k])
        assert _same_cost(out["cost_after"][k], after[k]), (k, out["cost_after"][k], after[k])


@pytest.mark.parametrize("name", TWO)
def test_fast_surfel_costs(name):
    """tests/test_gpu_surfel_costs.py::test_the_fast_flavour_is_deterministic_and_close_to_the_exact_one: the same bits call after call;
    the sums over the surfels within 1e-5 relative of the exact flavour's plus, per association the flavours decide differently
    (counted from the per-pair hook of both), the largest term."""
    w, ba, g = _world(name)
    _, _, f = _world(name, "fast")
    exact, fast = g.evaluate_surfel_costs(prefill=0xFF), f.evaluate_surfel_costs(prefill=0xFF)
    sc.assert_same_bits(f.evaluate_surfel_costs(prefill=0xFF), fast, "fast again")
    idx = np.arange(ba.surfels_size, dtype=np.uint32)
    depth_flips = desc_flips = 0
    desc_max = 0.0
    for k in range(8):
        a, b = g.evaluate_pairs(k, idx, _frame(ba, k)), f.evaluate_pairs(k, idx, _frame(ba, k))
        depth_flips += int(((a[:, 0] == 1) != (b[:, 0] == 1)).sum())
        colour = [(o[:, 0] == 1) & (o[:, 3] == 1) for o in (a, b)]
        desc_flips += int((colour[0] != colour[1]).sum())
        for o, c in zip((a, b), colour):
            if c.any():
                desc_max = max(desc_max, float(sc.huber_cost(np.concatenate([o[c, 14], o[c, 15]])).max()))
    e, c = sc.totals(exact), sc.totals(fast)
    print(name, "flips", depth_flips, desc_flips, "exact", e, "fast", c)
    assert depth_flips <= 1e-3 * e["depth_residuals"] and desc_flips <= 1e-3 * e["descriptor_pairs"], (depth_flips, desc_flips)
    assert abs(c["depth_residuals"] - e["depth_residuals"]) <= depth_flips and abs(c["descriptor_pairs"] - e["descriptor_pairs"]) <= desc_flips
    for field, slack in (("depth", depth_flips * 100.0 / 6.0), ("descriptor_1", desc_flips * desc_max), ("descriptor_2", desc_flips * desc_max)):
        assert abs(c[field] - e[field]) <= 1e-5 * abs(e[field]) + slack, (field, c[field], e[field], slack)


def _pcg_state(name):
    w = tc.world(name)
    ba = _oracle(name)
    rng = np.random.Generator(np.random.PCG64(33))
    for k in range(7):
        ba.set_pose(k, synthetic.perturb_pose(rng, w.poses[k], 0.003, 0.0005))
    return w, ba


@pytest.mark.parametrize("name", TWO)
def test_fast_windowed_pcg_is_the_fast_whole_map_iteration_within_tolerance(name):
    """tests/test_gpu_pcg_window.py::test_all_active_fast_flavour_is_the_whole_map_iteration_within_tolerance: everything active, the
    windowed fast sweeps against the whole-map fast sweeps -- 99.9 % of the live surfels' positions and every pose within 1e-5, the same
    number of inner steps give or take one."""
    w, ba = _pcg_state(name)
    n = ba.surfels_size
    g, h = tc.build_gpu(w, ba, "fast"), tc.build_gpu(w, ba, "fast")
    runs = []
    for scene, windowed in ((g, False), (h, True)):
        scene.update_surfel_normals()
        steps, _ = scene.pcg_iteration(gauge_keyframe=7, windowed=windowed)
        runs.append((steps, scene.download_surfels()[:3].copy(), [kf["pose"].copy() for kf in scene.keyframes]))
    (ref_steps, ref_rows, ref_poses), (steps, rows, poses) = runs
    assert h.ctx.arithmetic == "fast" and ref_steps > 0 and abs(steps - ref_steps) <= 1, (steps, ref_steps)
    live = ba.surfel_data[0, :n] == ba.surfel_data[0, :n]
    dpos = np.abs(rows[:, live] - ref_rows[:, live]).max(axis=0)
    print(name, "inner steps", ref_steps, steps, "99.9th percentile %.2e m" % np.percentile(dpos, 99.9))
    assert np.percentile(dpos, 99.9) < 1e-5, np.percentile(dpos, 99.9)
    assert (np.abs(ref_rows[:, live] - ba.surfel_data[:3, :n][:, live]).max(axis=0) > 0).mean() > 0.9      # a real update happened
    for k in range(8):
        assert np.abs(poses[k].astype(np.float64) - ref_poses[k]).max() < 1e-5, k


def _miscalibrated(name):
    w = tc.world(name)
    ba = _oracle(name)
    for cam, off in ((ba.depth_cam, (0.05, -0.06, 0.123, -0.217)), (ba.color_cam, (0.04, -0.03, 0.08, -0.06))):
        cam.fx += off[0]; cam.fy += off[1]; cam.cx += off[2]; cam.cy += off[3]
    ba.dp.a = 0.0125
    ba.cfactor[:] = np.random.Generator(np.random.PCG64(5)).uniform(-2e-3, 2e-3, ba.cfactor.shape).astype(F32)
    return w, ba


@pytest.mark.parametrize("name", TWO)
def test_fast_intrinsics_sweep_counts_the_exact_flavours_observations_and_the_controlled_step_is_the_by_hand_sequence(name):
    """The observation count of every sparse cell (word 7 of its sums) is the exact flavour's; and
    tests/test_gpu_intrinsics_step_control.py::test_state_r_the_call_is_the_by_hand_sequence[fast]'s comparator: the controlled step is
    the sums, the damped solves and the cost evaluations played by hand on a twin scene."""
    from tests import intrinsics_step_control as isc
    w, ba = _miscalibrated(name)
    e, g, hand = tc.build_gpu(w, ba), tc.build_gpu(w, ba, "fast"), tc.build_gpu(w, ba, "fast")
    _, exact_cells = isc.gpu_sums(e)
    _, fast_cells = isc.gpu_sums(hand)
    assert np.array_equal(fast_cells[:, 7], exact_cells[:, 7]) and exact_cells[:, 7].sum() > 10000
    assert (exact_cells[0, 7] > 0) and (exact_cells[-1, 7] > 0)                 # the corner cells are observed
    want = isc.gpu_controlled_step_by_hand(hand, 0.0)
    res = g.optimize_intrinsics_controlled(0.0)
    for key in ("accepted", "trials", "lambda_accepted", "lam", "cost_before", "cost_after"):
        assert res[key] == want[key], (key, res[key], want[key])
    got = dict(depth_cam=res["depth_camera"], color_cam=res["color_camera"], a=res["a"], cfactor=g.cfactor.download())
    for key in ("depth_cam", "color_cam", "a", "cfactor"):
        assert np.array_equal(_bits(got[key]).ravel(), _bits(want["state"][key]).ravel()), key
    print(name, "controlled fast intrinsics step: accepted", res["accepted"], "trials", res["trials"])
