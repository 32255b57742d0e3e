"""Step control of the pose phase through the C ABI (kernels_pose_trial.hip, capi_pose_trial.hip): the damped solve against its
definition, the cost bits of the fused sweep against bahip_evaluate_cost, per-keyframe descent with the damping rule, agreement with
the plain phase where no step is rejected, the first rung of a perturbation ladder at which the plain phase raises a keyframe's
cost, launch shapes, activation, surfel sharding, refusals."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

from badslam_amd import capi, multigpu, synthetic
from tests import common

pytestmark = pytest.mark.gpu

CONTROL = (4.0, 0.5, 0.0, 1e6, 4)   # lambda_up, lambda_down, lambda_min, lambda_max, max_trials
LADDER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pose_step_control_ladder.json")
LADDER_SEED, LADDER_RUNGS = 5, 7     # sigma 5 mm x 2^rung, 2 mrad x 2^rung
_SCENE = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f(c):
    return (c["depth"] + c["descriptor_1"]) + c["descriptor_2"]


def _same_cost(a, b):
    return all(np.float64(a[n]).view(np.uint64) == np.float64(b[n]).view(np.uint64) for n in ("depth", "descriptor_1", "descriptor_2")) and \
        a["depth_residuals"] == b["depth_residuals"] and a["descriptor_pairs"] == b["descriptor_pairs"]


def scene_and_surfels():
    """small_scene(5 keyframes, 320 x 240, seed 21) and its created surfels (computed once, never modified)."""
    if not _SCENE:
        scene = common.small_scene(num_keyframes=5, seed=21)
        g = common.build_gpu(scene, 400000)
        _SCENE.update(scene=scene, data=g.download_surfels())
    return _SCENE["scene"], _SCENE["data"]


def perturbed(sigma_t=0.005, sigma_r=0.002, seed=5, arithmetic="exact", columns=None, ctx=None):
    """The scene on the GPU, poses perturbed with synthetic.perturb_pose; `columns`: the surfels of a shard."""
    scene, data = scene_and_surfels()
    g = common.build_gpu(scene, 400000, create_from=[], ctx=ctx)
    mine = data if columns is None else np.ascontiguousarray(data[:, columns])
    g.upload_surfels(mine, np.ones(mine.shape[1], np.uint8))
    rng = np.random.Generator(np.random.PCG64(seed))
    for k, T in enumerate(scene.poses_gt):
        g.keyframes[k]["pose"] = np.asarray(synthetic.perturb_pose(rng, T, sigma_t, sigma_r), np.float32)
    if arithmetic != "exact":
        g.ctx.set_arithmetic(arithmetic)
        g.set_intrinsics()
    g.bind_keyframes()
    return g


def device_poses(g):
    K = len(g.keyframes)
    poses = (C.c_float * (7 * K))()
    capi.check(g.ctx.lib.bahip_get_keyframe_poses(g.ctx.handle, poses, K))
    return np.array(list(poses), np.float32).reshape(K, 7)


def _normal_equations(g, k):
    from oracle import binding as ob
    F = ob.se3_matrix3x4(ob.se3_inverse(ob.SE3.from_array(g.keyframes[k]["pose"])))
    H, b = g.accumulate_pose_coeffs(k, True, True, F)
    return np.concatenate([H, b]).astype(np.float32)


def _step(ctx, hb, T, lam=None):
    out = np.zeros(25, np.float32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    if lam is None:
        capi.check(ctx.lib.bahip_debug_pose_step(ctx.handle, p(hb), p(T), p(out)))
    else:
        capi.check(ctx.lib.bahip_debug_pose_step_damped(ctx.handle, p(hb), p(T), float(lam), p(out)))
    return out


def test_damped_solve():
    """lambda = 0: the 25 words of bahip_debug_pose_step.  lambda in {1e-3, 1, 1e3} on the scene's normal equations: the binary32 x is that
    of numpy's binary64 solve of (H + lambda diag H) x = b and of the oracle's LDLT on that binary64 matrix -- compared as
    test_pose_update_step_bit_exact (tests/test_gpu_kernels_vs_oracle.py) compares x: word for word."""
    from oracle import binding as ob
    g = perturbed()
    L = ob.lib()
    for k in range(len(g.keyframes)):
        hb = _normal_equations(g, k)
        T = np.asarray(g.keyframes[k]["pose"], np.float32)
        assert np.array_equal(_step(g.ctx, hb, T).view(np.uint32), _step(g.ctx, hb, T, 0.0).view(np.uint32)), k
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = hb[:21].astype(np.float64)
        H = H + np.triu(H, 1).T
        b = hb[21:].astype(np.float64)
        for lam in (1e-3, 1.0, 1e3):
            A = H.copy()
            A[np.diag_indices(6)] = np.diag(H) + np.float64(np.float32(lam)) * np.diag(H)
            x_numpy = np.linalg.solve(A, b).astype(np.float32)
            x_ldlt = np.zeros(6)
            L.orc_ldlt_solve(6, np.ascontiguousarray(A).ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)),
                             x_ldlt.ctypes.data_as(C.POINTER(C.c_double)))
            out = _step(g.ctx, hb, T, lam)
            print("keyframe", k, "lambda", lam, "x", out[:6], "numpy", x_numpy, "max |diff|", np.abs(out[:6] - x_numpy).max())
            assert np.array_equal(out[:6].view(np.uint32), x_ldlt.astype(np.float32).view(np.uint32)), (k, lam)
            assert np.array_equal(out[:6].view(np.uint32), x_numpy.view(np.uint32)), (k, lam, out[:6], x_numpy)
            assert not np.array_equal(out[:6].view(np.uint32), _step(g.ctx, hb, T)[:6].view(np.uint32))


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
@pytest.mark.parametrize("residuals", [(True, False), (False, True), (True, True)])
def test_cost_bits(residuals, arithmetic):
    """cost_before / cost_after are bahip_evaluate_cost's per-keyframe entries on the table before / after the call, field by field."""
    use_depth, use_desc = residuals
    g = perturbed(arithmetic=arithmetic)
    K = len(g.keyframes)
    before = g.evaluate_cost(use_depth, use_desc)[1]
    out = g.estimate_keyframe_poses_controlled([1e-3] * K, CONTROL, use_depth, use_desc)
    after = g.evaluate_cost(use_depth, use_desc)[1]
    assert out["iterations"].sum() > 0
    for k in range(K):
        assert _same_cost(out["cost_before"][k], before[k]), (k, out["cost_before"][k], before[k])
        assert _same_cost(out["cost_after"][k], after[k]), (k, out["cost_after"][k], after[k])
    assert np.array_equal(_bits(device_poses(g)), _bits(out["poses"]))


def _check_descent(g, start_poses, lambdas, out, control=CONTROL):
    up, _down, _lo, hi, _trials = control
    table = device_poses(g)
    for k in range(len(g.keyframes)):
        fb, fa = _f(out["cost_before"][k]), _f(out["cost_after"][k])
        if out["iterations"][k] == 0:
            assert fa == fb and _same_cost(out["cost_before"][k], out["cost_after"][k]), k
            assert np.array_equal(_bits(table[k]), _bits(start_poses[k])) and np.array_equal(_bits(out["poses"][k]), _bits(start_poses[k])), k
            lam = np.float32(lambdas[k])
            for _ in range(out["trials"][k]):
                lam = min(np.float32(lam * np.float32(up)), np.float32(hi))
            assert np.float32(out["lambdas"][k]) == lam, (k, out["lambdas"][k], lam)
            assert out["rejected"][k] == out["trials"][k] and not out["converged"][k]
        else:
            assert fa < fb, (k, fb, fa)
            assert out["trials"][k] == out["iterations"][k] + out["rejected"][k]


def test_descent():
    """No keyframe's objective rises; it stays exactly where no step was accepted, and there the pose keeps every word and lambda has
    grown by lambda_up per trial.  Keyframe 4 is moved a hundred metres away: it sees no surfel, its cost is 0 and cannot fall, so the
    branch without an accepted step is met whatever the others do."""
    g = perturbed(0.02, 0.008)
    K = len(g.keyframes)
    g.keyframes[4]["pose"][4:7] += np.float32(100.0)
    g.bind_keyframes()
    seen = set()
    lambdas = [1e-3] * K
    for _ in range(3):
        start = [np.asarray(kf["pose"], np.float32).copy() for kf in g.keyframes]
        out = g.estimate_keyframe_poses_controlled(lambdas, CONTROL)
        _check_descent(g, start, lambdas, out)
        assert out["iterations"][4] == 0 and out["trials"][4] == CONTROL[4] and _f(out["cost_before"][4]) == 0.0
        seen |= {"none" if i == 0 else "some" for i in out["iterations"]}
        lambdas = list(out["lambdas"])
    assert seen == {"none", "some"}, seen


def test_agreement_with_the_plain_phase():
    """lambda = 0, lambda_min = 0, from 5 mm / 2 mrad: a keyframe none of whose candidates was rejected has the plain phase's pose bits
    and iteration count."""
    g, h = perturbed(0.005, 0.002), perturbed(0.005, 0.002)
    K = len(g.keyframes)
    poses, its, conv, _ = h.estimate_keyframe_poses(True, True)
    out = g.estimate_keyframe_poses_controlled([0.0] * K, (4.0, 0.5, 0.0, 1e6, 4))
    clean = [k for k in range(K) if out["rejected"][k] == 0]
    for k in clean:
        assert np.array_equal(_bits(out["poses"][k]), _bits(poses[k].astype(np.float32))), k
        assert out["iterations"][k] == its[k] and out["converged"][k] == conv[k], (k, out["iterations"][k], its[k])
        assert out["lambdas"][k] == 0.0
    assert len(clean) >= 1, "%d of %d keyframes without a rejected candidate" % (len(clean), K)
    print("%d of %d keyframes without a rejected candidate" % (len(clean), K))


def ladder_rung(rung):
    """One rung of the ladder: what the plain and the controlled phase do to every keyframe's cost."""
    s = 2.0 ** rung
    g = perturbed(0.005 * s, 0.002 * s, LADDER_SEED)
    K = len(g.keyframes)
    before = [_f(c) for c in g.evaluate_cost()[1]]
    g.estimate_keyframe_poses(True, True)
    after = [_f(c) for c in g.evaluate_cost()[1]]
    h = perturbed(0.005 * s, 0.002 * s, LADDER_SEED)
    out = h.estimate_keyframe_poses_controlled([1e-3] * K, CONTROL)
    return dict(rung=rung, sigma_t=0.005 * s, sigma_r=0.002 * s, seed=LADDER_SEED, cost_before=before, plain_cost_after=after,
                plain_raised=[k for k in range(K) if not after[k] <= before[k]],
                controlled_cost_after=[_f(c) for c in out["cost_after"]], controlled_rejected=[int(v) for v in out["rejected"]],
                controlled_iterations=[int(v) for v in out["iterations"]])


def test_a_rejection_happens_and_is_undone():
    """At the first rung of the committed ladder at which the plain phase raises some keyframe's cost, the controlled phase rejects at
    least one candidate and leaves no keyframe's cost above its start."""
    table = json.load(open(LADDER))
    raised = [row["rung"] for row in table["rungs"] if row["plain_raised"]]
    assert raised, "the plain phase raised no keyframe's cost on the whole ladder"
    assert table["first_raised_rung"] == min(raised)
    row = ladder_rung(table["first_raised_rung"])
    print(row)
    assert row["plain_raised"], row                      # the rung's premise, measured again
    assert sum(row["controlled_rejected"]) >= 1, row
    assert all(a <= b for a, b in zip(row["controlled_cost_after"], row["cost_before"])), row


def _result_words(out):
    costs = [[c[n] for n in ("depth", "descriptor_1", "descriptor_2")] + [float(c["depth_residuals"]), float(c["descriptor_pairs"])]
             for c in out["cost_before"] + out["cost_after"]]
    return (_bits(out["poses"]).tolist(), _bits(out["lambdas"]).tolist(), np.array(costs, np.float64).view(np.uint64).tolist(),
            out["iterations"].tolist(), out["converged"].tolist(), out["trials"].tolist(), out["rejected"].tolist(), out["rounds"])


def test_launch_shape_does_not_matter():
    K = 5
    reference = _result_words(perturbed(0.02, 0.008).estimate_keyframe_poses_controlled([1e-3] * K, CONTROL))
    lib = capi.load()
    try:
        for waves, shift, tile_waves, parts in ((1, 3, 1, 8), (16, 0, 4, 1), (1, 0, 5, 8), (16, 3, 0, 0)):
            capi.check(lib.bahip_debug_set_pose_lds_shape(waves, shift))
            capi.check(lib.bahip_debug_set_launch_shapes(tile_waves, parts))
            got = _result_words(perturbed(0.02, 0.008).estimate_keyframe_poses_controlled([1e-3] * K, CONTROL))
            assert got == reference, (waves, shift, tile_waves, parts)
    finally:
        capi.check(lib.bahip_debug_set_pose_lds_shape(0, -1))
        capi.check(lib.bahip_debug_set_launch_shapes(0, 0))


def test_activation():
    """kInactive keyframes are untouched; with update_activation the table's activations and moved[] follow the plain rule on the
    poses before and after the call."""
    from badslam_amd import se3
    g = perturbed(0.02, 0.008)
    K = len(g.keyframes)
    g.keyframes[1]["activation"] = capi.KF_INACTIVE
    g.keyframes[3]["activation"] = capi.KF_COVISIBLE_ACTIVE
    g.bind_keyframes()
    start = [np.asarray(kf["pose"], np.float32).copy() for kf in g.keyframes]
    lambdas = [1e-3, 7.0, 1e-3, 1e-3, 1e-3]
    out = g.estimate_keyframe_poses_controlled(lambdas, CONTROL, update_activation=True)
    zero = dict(depth=0.0, descriptor_1=0.0, descriptor_2=0.0, depth_residuals=0, descriptor_pairs=0)
    assert np.array_equal(_bits(out["poses"][1]), _bits(start[1])) and out["lambdas"][1] == np.float32(7.0)
    assert out["converged"][1] == 1 and out["iterations"][1] == 0 and out["trials"][1] == 0 and out["moved"][1] == 0
    assert out["cost_before"][1] == zero and out["cost_after"][1] == zero
    expected_moved = []
    for k in range(K):
        lg = se3.log(se3.mul(se3.inverse(start[k].astype(np.float64)), out["poses"][k].astype(np.float64)))
        expected_moved.append(int(np.sum(lg[:3] ** 2) + np.sum((10.0 * lg[3:]) ** 2) >= 1e-6))
    expected_moved[1] = 0
    assert out["moved"].tolist() == expected_moved, (out["moved"], expected_moved)   # (centimetre moves or none: far from the threshold)
    assert out["num_converged"] == 1 + sum(1 for k in range(K) if k != 1 and not expected_moved[k])
    # the table: a second phase leaves out exactly the keyframes that are kInactive now
    again = g.estimate_keyframe_poses_controlled(list(out["lambdas"]), CONTROL)
    skipped = [k for k in range(K) if again["trials"][k] == 0 and again["iterations"][k] == 0 and again["cost_before"][k] == zero]
    assert skipped == [k for k in range(K) if not expected_moved[k]], (skipped, expected_moved)


@pytest.mark.parametrize("world", [2, 4])
def test_surfel_sharding(world):
    """Loopback shards in chunks of 1024 (world 4: one rank's shard empty): every rank returns the unsharded call's words."""
    import torch
    from tests.test_gpu_sharded_loopback import _Loopback
    torch.cuda.set_device(0)
    _, data = scene_and_surfels()
    K = 5
    N = data.shape[1] if world == 2 else 3 * 1024     # three chunks over four ranks: rank 3 holds nothing
    reference = _result_words(perturbed(0.02, 0.008, columns=np.arange(N)).estimate_keyframe_poses_controlled([1e-3] * K, CONTROL))
    loop = _Loopback(world)
    results, errors = [None] * world, []

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            mine = multigpu.shard_chunks(N, rank, world, chunk=1024)
            g = perturbed(0.02, 0.008, columns=mine)
            hook = loop.hook_for(rank)
            capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, hook, None))
            results[rank] = (_result_words(g.estimate_keyframe_poses_controlled([1e-3] * K, CONTROL)), mine.size, hook, g)
        except Exception as e:
            errors.append((rank, repr(e)))
            loop.barrier.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    if world == 4:
        assert results[3][1] == 0
    for rank in range(world):
        assert results[rank][0] == reference, rank
    assert sum(reference[3]) > 0   # steps were taken


def test_refusals():
    g = perturbed()
    K = len(g.keyframes)
    start = device_poses(g)
    for bad in ((0.5, 0.5, 0.0, 1e6, 4), (4.0, 0.0, 0.0, 1e6, 4), (4.0, 1.5, 0.0, 1e6, 4), (4.0, 0.5, 2.0, 1.0, 4), (4.0, 0.5, -1.0, 1e6, 4),
                (4.0, 0.5, 0.0, float("inf"), 4), (4.0, 0.5, 0.0, 1e6, 0), (float("nan"), 0.5, 0.0, 1e6, 4)):
        with pytest.raises(RuntimeError):
            g.estimate_keyframe_poses_controlled([1e-3] * K, bad)
    for bad_lambda in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            g.estimate_keyframe_poses_controlled([1e-3] * (K - 1) + [bad_lambda], CONTROL)
    capi.check(g.ctx.lib.bahip_context_set_keyframe_sharding(g.ctx.handle, 0, 2))
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.estimate_keyframe_poses_controlled([1e-3] * K, CONTROL)
    capi.check(g.ctx.lib.bahip_context_set_keyframe_sharding(g.ctx.handle, 0, 1))
    assert np.array_equal(_bits(device_poses(g)), _bits(start))
    # a NaN in one surfel row (a descriptor: the pair's terms are not finite): the plain phase's error
    data = g.download_surfels()
    data[6, 100] = np.nan
    errors = []
    for controlled in (False, True):
        h = perturbed()
        h.upload_surfels(data, np.ones(data.shape[1], np.uint8))
        with pytest.raises(RuntimeError) as info:
            if controlled:
                h.estimate_keyframe_poses_controlled([1e-3] * K, CONTROL)
            else:
                h.estimate_keyframe_poses(True, True)
        errors.append(str(info.value).rsplit(" (", 1)[0])   # without the source position
    assert errors[0] == errors[1] and "pose normal equations" in errors[0], errors
    # the context works afterwards
    out = g.estimate_keyframe_poses_controlled([1e-3] * K, CONTROL)
    assert out["iterations"].sum() > 0
