"""Step control for the PCG scheme through the C ABI (kernels_pcg_trial.hip, capi_pcg_trial.hip): the damped system against its
definition, the three entry paths as one system, bit-exact undo of a rejected step, the monotone sequence of accepted costs with the
damping factor's update rule, the plain scheme's first failing rung of a fixed perturbation ladder, and surfel sharding."""
import ctypes as C
import threading

import numpy as np
import pytest

from badslam_amd import capi, multigpu, synthetic
from oracle import binding as ob
from tests import common
from tests.test_gpu_intrinsics_pcg_vs_oracle import _pcg_setup
from tests.test_gpu_pcg_stages import INVALID, _Vec, _pose_index

pytestmark = pytest.mark.gpu

EPS = np.float32(1e-8)      # kDiagEpsilon
PRIOR = np.float32(100.0)   # kAPriorWeight squared, at the unknown `a`
CONTROL = (4.0, 0.5, 0.0, 1e6, 6)   # lambda_up, lambda_down, lambda_min, lambda_max, max_trials


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scalar(c):
    return (c["depth"] + c["descriptor_1"]) + c["descriptor_2"]


def _scene(mode="poses+geometry", seed=21, K=5):
    scene = common.small_scene(num_keyframes=K, seed=seed)
    _, g, data, _ = _pcg_setup(scene, mode)
    return scene, g, data


def _state(g):
    return dict(surfels=g.download_surfels(), active=g.active_buf.download()[0, :g.surfels_size].copy(),
                poses=[np.array(kf["pose"], np.float32) for kf in g.keyframes], cfactor=g.cfactor.download(), a=g.dp.a,
                cams=[getattr(cam, f) for cam in (g.depth_cam, g.color_cam) for f in ("fx", "fy", "cx", "cy")])


def _device_poses(g):
    K = len(g.keyframes)
    poses = (C.c_float * (7 * K))()
    capi.check(g.ctx.lib.bahip_get_keyframe_poses(g.ctx.handle, poses, K))
    return np.array(list(poses), np.float32).reshape(K, 7)


def _same_state(a, b):
    assert np.array_equal(_bits(a["surfels"]), _bits(b["surfels"]))
    assert np.array_equal(a["active"], b["active"])
    for k, (p, q) in enumerate(zip(a["poses"], b["poses"])):
        assert np.array_equal(_bits(p), _bits(q)), k
    assert np.array_equal(_bits(a["cfactor"]), _bits(b["cfactor"]))
    assert a["a"] == b["a"] and a["cams"] == b["cams"]


def _plain(g, di=False, windowed=False, gauge=1, max_inner_iterations=30):
    g.update_surfel_normals()
    return g.pcg_iteration(optimize_poses=True, optimize_geometry=True, optimize_depth_intrinsics=di, optimize_color_intrinsics=di,
                           gauge_keyframe=gauge, windowed=windowed, max_inner_iterations=max_inner_iterations)


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
@pytest.mark.parametrize("mode", ["poses+geometry", "all"])
def test_off_is_off(mode, arithmetic):
    """bahip_context_set_pcg_damping(ctx, 0), then bahip_pcg_iteration: the bits of a context that never heard of damping."""
    di = mode == "all"
    _, g, _ = _scene(mode)
    _, h, _ = _scene(mode)
    for x in (g, h):
        x.ctx.set_arithmetic(arithmetic)
        x.set_intrinsics()
    h.set_pcg_damping(0.0)
    steps_g, conv_g = _plain(g, di)
    steps_h, conv_h = _plain(h, di)
    assert steps_g == steps_h > 0 and conv_g == conv_h
    _same_state(_state(g), _state(h))


@pytest.mark.parametrize("mode", ["poses+geometry", "all"])
def test_the_damped_system_is_the_defined_one(mode):
    """lambda > 0: p after PCGInit2 is r / (((M + 1e-8) + prior) + lambda * M) in binary32, in that order, over all unknowns; and after
    one inner step z (left in g) is the new r over the same denominator."""
    di = mode == "all"
    lam = np.float32(0.37)
    _, g, data = _scene(mode)
    K, N, S = len(g.keyframes), data.shape[1], g.cf_w * g.cf_h
    U = 6 * (K - 1) + 3 * N + ((5 + S + 4) if di else 0)
    g.set_pcg_damping(float(lam))
    _plain(g, di, max_inner_iterations=0)
    r, M, p = g.read_pcg_vector(0, U), g.read_pcg_vector(1, U), g.read_pcg_vector(4, U)
    prior = np.zeros(U, np.float32)
    rhs = r.copy()
    if di:
        a_index = 6 * (K - 1) + 3 * N + 4
        prior[a_index] = PRIOR
        rhs[a_index] = r[a_index] + np.float32(-PRIOR * np.float32(g.dp.a))
    denominator = ((M + EPS) + prior) + lam * M
    assert denominator.dtype == np.float32 and np.count_nonzero(M) > 0.5 * U
    with np.errstate(all="ignore"):
        expected = rhs / denominator
    assert np.array_equal(_bits(p), _bits(expected)), np.flatnonzero(_bits(p) != _bits(expected))[:10]
    # the undamped p differs: the check above is not vacuous
    assert not np.array_equal(_bits(p), _bits(rhs / ((M + EPS) + prior)))
    # one inner step (no update of p follows the last step): g = z = r_new / denominator
    _, h, _ = _scene(mode)
    h.set_pcg_damping(float(lam))
    _plain(h, di, max_inner_iterations=1)
    r1, M1, z, p1 = (h.read_pcg_vector(w, U) for w in (0, 1, 3, 4))
    assert np.array_equal(_bits(M1), _bits(M)) and np.array_equal(_bits(p1), _bits(p))
    assert np.array_equal(_bits(z), _bits(r1 / denominator))


def _stage_driver(h, di, gauge, lam):
    """The reference's driver over the stage entry points (tests/test_gpu_pcg_stages.py), under the context's damping factor."""
    h.set_pcg_damping(lam)
    h.update_surfel_normals()
    lib, ctx = h.ctx.lib, h.ctx.handle
    K, N, S = len(h.keyframes), h.surfels_struct().surfels_size, h.cf_w * h.cf_h
    P = 6 * (K - 1)
    U = P + 3 * N + ((5 + S + 4) if di else 0)
    layout = capi.PCGLayout(1, 1, int(di), int(di), 1, 1, U, P, (P + 3 * N) if di else INVALID, (P + 3 * N + 5 + S) if di else INVALID)
    r, M, delta, gv, p = (_Vec(h.ctx, U) for _ in range(5))
    an, ad, bn = (_Vec(h.ctx, 1) for _ in range(3))
    s = h.surfels_struct()
    frames = [h.frame_struct(k) for k in range(K)]
    Fs = [(C.c_float * 12)(*[float(v) for v in ob.se3_matrix3x4(ob.se3_inverse(ob.SE3.from_array(h.keyframes[k]["pose"])))]) for k in range(K)]
    capi.check(lib.bahip_pcg_begin(ctx, C.byref(layout), N))
    for k in range(K):
        capi.check(lib.bahip_pcg_init(ctx, C.byref(layout), C.byref(frames[k]), Fs[k], _pose_index(k, gauge), int(k != gauge), C.byref(s), r.ptr, M.ptr))
    capi.check(lib.bahip_pcg_init2(ctx, C.byref(layout), N, h.dp.a, r.ptr, M.ptr, delta.ptr, gv.ptr, p.ptr, an.ptr))
    prev, no_improvement, steps = np.inf, 0, 0
    for step in range(30):
        steps += 1
        if step > 0:
            an, bn = bn, an
            gv.buf.clear(0)
        for k in range(K):
            capi.check(lib.bahip_pcg_step1(ctx, C.byref(layout), C.byref(frames[k]), Fs[k], _pose_index(k, gauge), int(k != gauge), C.byref(s), p.ptr, gv.ptr))
        capi.check(lib.bahip_pcg_step2(ctx, C.byref(layout), N, r.ptr, M.ptr, delta.ptr, gv.ptr, p.ptr, an.ptr, ad.ptr, bn.ptr))
        r_norm = float(np.sqrt(np.float32(bn.get()[0])))
        if r_norm < prev - 1e-3:
            no_improvement = 0
        else:
            no_improvement += 1
            if no_improvement >= 3:
                break
        prev = r_norm
        if step < 29:
            capi.check(lib.bahip_pcg_step3(ctx, C.byref(layout), N, gv.ptr, p.ptr, an.ptr, bn.ptr))
    return steps, delta.get(), U


@pytest.mark.parametrize("mode", ["poses+geometry", "all"])
def test_three_paths_one_system(mode):
    """The same damping factor through the fused iteration, the windowed iteration with everything active and the stage-by-stage
    driver: the same inner steps and the same delta, bit for bit."""
    di = mode == "all"
    lam = 0.25
    _, g, data = _scene(mode)
    g.set_pcg_damping(lam)
    steps, _ = _plain(g, di)
    _, w, _ = _scene(mode)
    for kf in w.keyframes:
        kf["activation"] = capi.KF_ACTIVE
    w.bind_keyframes()
    w.set_pcg_damping(lam)
    steps_w, _ = _plain(w, di, windowed=True)
    _, h, _ = _scene(mode)
    steps_h, delta_h, U = _stage_driver(h, di, 1, lam)
    delta = g.read_pcg_vector(2, U)
    assert steps == steps_w == steps_h > 0
    assert np.array_equal(_bits(w.read_pcg_vector(2, U)), _bits(delta))
    assert np.array_equal(_bits(delta_h), _bits(delta))
    _same_state(_state(g), _state(w))
    # and the damping did something: the undamped delta is another one
    _, u, _ = _scene(mode)
    _plain(u, di)
    assert not np.array_equal(_bits(u.read_pcg_vector(2, U)), _bits(delta))


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("mode", ["poses+geometry", "all"])
def test_a_rejected_step_leaves_no_trace(mode, windowed):
    """A step that is rejected (the caller's cost_before is zero, below which no cost lies; lambda_up = 1, max_trials = 1) leaves every
    surfel row, the active flags, the poses (host and device table), intrinsics, a and the cfactor plane bit-equal to before the
    call; under a window that covers part of the scene, nothing outside it was written at all (NaN planted in an inactive surfel
    stays, and so does everything else there).  The same step without control does change the state."""
    di = mode == "all"
    _, g, data = _scene(mode)
    N = data.shape[1]
    if windowed:
        acts = [capi.KF_INACTIVE, capi.KF_COVISIBLE_ACTIVE, capi.KF_ACTIVE, capi.KF_ACTIVE, capi.KF_COVISIBLE_ACTIVE]
        for k, a in enumerate(acts):
            g.keyframes[k]["activation"] = a
        g.bind_keyframes()
        active = (np.arange(N) // 64) % 3 != 1
        marked = data.copy()
        marked[6, ~active] = -0.0        # what a write-back through the update kernel would turn into +0
        g.upload_surfels(marked, active.astype(np.uint8))
    before = _state(g)
    table_before = _device_poses(g)
    zero = capi.Cost()
    out = g.pcg_iteration_controlled(0.0, (1.0, 1.0, 0.0, 1.0, 1), optimize_depth_intrinsics=di, optimize_color_intrinsics=di,
                                     gauge_keyframe=2 if windowed else 1, windowed=windowed, update_normals=True, cost_before=zero)
    assert not out["accepted"] and out["trials"] == 1 and out["steps"] > 0 and out["lam"] == 0.0
    assert out["cost_after"] == out["cost_before"]
    _same_state(_state(g), before)
    assert np.array_equal(_bits(_device_poses(g)), _bits(table_before))
    # the context still works, and the step that was undone is a real one
    _plain(g, di, windowed=windowed, gauge=2 if windowed else 1)
    after = _state(g)
    assert not np.array_equal(_bits(after["surfels"][:3]), _bits(before["surfels"][:3]))
    if windowed:
        assert np.array_equal(_bits(after["surfels"][:, ~active]), _bits(before["surfels"][:, ~active]))


def _perturb(g, scene, sigma_t, sigma_r, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    for k, T in enumerate(scene.poses_gt):
        g.keyframes[k]["pose"] = np.asarray(synthetic.perturb_pose(rng, T, sigma_t, sigma_r), np.float32)
    g.bind_keyframes()


def _next_lambda(lam, accepted, trials, control):
    up, down, lo, hi, _ = (np.float32(v) for v in control)
    lam = np.float32(lam)
    for _ in range(trials - (1 if accepted else 0)):
        lam = min(np.float32(lam * up), hi)
    if accepted:
        lam = max(np.float32(lam * down), lo)
    return float(lam)


def test_monotone_by_construction():
    """Ten controlled outer iterations from perturbed poses: the accepted costs fall strictly, each is bahip_evaluate_cost of the state
    at that moment bit for bit, the previous cost_after serves as the next cost_before, and lambda follows the update rule."""
    scene, g, _ = _scene()
    _perturb(g, scene, 0.02, 0.008, seed=5)
    lam, last, carried, accepted_any = 1e-3, None, None, 0
    for it in range(10):
        out = g.pcg_iteration_controlled(lam, CONTROL, update_normals=True, cost_before=carried)
        now, _ = g.evaluate_cost(per_keyframe=False)
        print(it, out["accepted"], out["trials"], out["lam"], _scalar(out["cost_before"]), _scalar(out["cost_after"]),
              out["cost_after"]["depth_residuals"], out["cost_after"]["descriptor_pairs"])
        assert now == out["cost_after"], it          # every field, the doubles by value (no NaN here) = bit for bit
        if last is not None:
            assert out["cost_before"] == last
        assert out["lam"] == _next_lambda(lam, out["accepted"], out["trials"], CONTROL), it
        if out["accepted"]:
            accepted_any += 1
            assert np.isfinite(_scalar(out["cost_after"])) and _scalar(out["cost_after"]) < _scalar(out["cost_before"]), it
            assert out["trials"] >= 1
        else:
            assert out["trials"] == CONTROL[4] and out["cost_after"] == out["cost_before"], it
        lam, last, carried = out["lam"], out["cost_after"], out["cost_after_struct"]
    assert accepted_any >= 1


# The ladder of check 6: translation sigma 5 mm x 2^rung, rotation sigma 2 mrad x 2^rung, rung 0 .. 6, seed 5, on small_scene(5, seed 21)
# with the surfels of _pcg_setup; ten plain outer iterations each.  Rung 0 is the first at which a plain outer iteration raises the cost
# (the tenth, next to convergence: 420.555 -> 420.600); rungs 1 - 4 never do, rungs 5 and 6 do early (DESIGN.md section 3 has the table).
LADDER_RUNG = dict(sigma_t=0.005, sigma_r=0.002, seed=5, iterations=10)
DEFAULTS = dict(lam=1e-3, control=(10.0, 0.33, 0.0, 1e6, 6))   # DirectBA::PCGStepControl's defaults


def _pose_rmse(scene, g, gauge=1):
    from badslam_amd import se3
    errors = []
    for k in range(len(g.keyframes)):
        rel = se3.mul(se3.inverse(np.asarray(g.keyframes[gauge]["pose"], np.float64)), np.asarray(g.keyframes[k]["pose"], np.float64))
        gt = se3.mul(se3.inverse(np.asarray(scene.poses_gt[gauge], np.float64)), np.asarray(scene.poses_gt[k], np.float64))
        errors.append(np.linalg.norm(common.pose_error(gt, rel)))
    return float(np.sqrt(np.mean(np.square(errors))))


def test_it_helps_where_the_plain_scheme_fails():
    """At the first rung of the ladder where the plain scheme raises its cost: after the same number of outer iterations the controlled
    scheme's cost is no higher than the plain scheme's, and its pose error against ground truth (relative to the gauge keyframe) no
    larger."""
    n = LADDER_RUNG["iterations"]
    scene, g, _ = _scene()
    _perturb(g, scene, LADDER_RUNG["sigma_t"], LADDER_RUNG["sigma_r"], LADDER_RUNG["seed"])
    costs = [_scalar(g.evaluate_cost(per_keyframe=False)[0])]
    for _ in range(n):
        _plain(g)
        costs.append(_scalar(g.evaluate_cost(per_keyframe=False)[0]))
    assert any(b > a for a, b in zip(costs, costs[1:])), costs   # the rung's premise
    scene, h, _ = _scene()
    _perturb(h, scene, LADDER_RUNG["sigma_t"], LADDER_RUNG["sigma_r"], LADDER_RUNG["seed"])
    lam = DEFAULTS["lam"]
    for _ in range(n):
        out = h.pcg_iteration_controlled(lam, DEFAULTS["control"], gauge_keyframe=1, update_normals=True)
        lam = out["lam"]
    final = _scalar(h.evaluate_cost(per_keyframe=False)[0])
    print("plain", costs[-1], _pose_rmse(scene, g), "controlled", final, _pose_rmse(scene, h))
    assert final <= costs[-1]
    assert _pose_rmse(scene, h) <= _pose_rmse(scene, g)


def test_surfel_sharding_takes_the_same_decisions():
    """Two surfel shards through the in-process loopback: the accept / reject sequence, lambda, the costs and the state of one GPU."""
    import torch
    from tests.test_gpu_sharded_loopback import _Loopback
    torch.cuda.set_device(0)
    world, rounds = 2, 4
    control = (4.0, 0.5, 0.0, 1e6, 3)

    def drive(g):
        lam, log = 0.0, []
        for _ in range(rounds):
            out = g.pcg_iteration_controlled(lam, control, update_normals=True)
            log.append((out["accepted"], out["trials"], out["lam"], out["steps"], out["cost_before"], out["cost_after"]))
            lam = out["lam"]
        return log

    scene, g, data = _scene()
    _perturb(g, scene, 0.04, 0.016, seed=5)
    start_poses = [np.array(kf["pose"], np.float32) for kf in g.keyframes]
    N = data.shape[1]
    ref_log = drive(g)
    ref = _state(g)
    loop = _Loopback(world)
    results, errors = [None] * world, []

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            _, gr, _, _ = _pcg_setup(scene, "poses+geometry")
            mine = multigpu.shard_chunks(N, rank, world, chunk=1024)
            gr.upload_surfels(np.ascontiguousarray(data[:, mine]), np.ones(len(mine), np.uint8))
            for k, T in enumerate(start_poses):
                gr.keyframes[k]["pose"] = T.copy()
            gr.bind_keyframes()
            hook = loop.hook_for(rank)
            capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
            results[rank] = dict(mine=mine, log=drive(gr), state=_state(gr), keep=hook, scene=gr)
        except Exception as e:
            errors.append((rank, repr(e)))
            loop.barrier.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    assert all(r is not None for r in results)
    merged = np.zeros_like(ref["surfels"])
    for r in results:
        assert r["log"] == ref_log
        for k in range(len(start_poses)):
            assert np.array_equal(_bits(r["state"]["poses"][k]), _bits(ref["poses"][k])), k
        merged[:, r["mine"]] = r["state"]["surfels"]
    assert np.array_equal(_bits(merged[:8]), _bits(ref["surfels"][:8]))


def test_refusals_leave_the_context_usable():
    _, g, _ = _scene()
    with pytest.raises(RuntimeError, match="max_trials"):
        g.pcg_iteration_controlled(0.0, (2.0, 0.5, 0.0, 1.0, 0))
    with pytest.raises(RuntimeError, match="lambda_up"):
        g.pcg_iteration_controlled(0.0, (0.5, 0.5, 0.0, 1.0, 1))
    with pytest.raises(RuntimeError, match="damping factor"):
        g.set_pcg_damping(-1.0)
    capi.check(g.ctx.lib.bahip_context_set_keyframe_sharding(g.ctx.handle, 0, 2))
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.pcg_iteration_controlled(0.0, CONTROL)
    capi.check(g.ctx.lib.bahip_context_set_keyframe_sharding(g.ctx.handle, 0, 1))
    out = g.pcg_iteration_controlled(0.0, CONTROL, update_normals=True)
    assert out["trials"] >= 1
