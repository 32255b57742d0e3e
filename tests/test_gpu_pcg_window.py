"""bahip_pcg_iteration_windowed: one outer PCG iteration over the active keyframe window (kernels_pcg_window.hip: "DEFINITION of the
windowed system") -- against bahip_pcg_iteration with everything active, against the stage-by-stage driver run over the swept
keyframes on a buffer of the active surfels alone, on inputs it must not read, under its refusals and under surfel sharding."""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

from badslam_amd import capi, multigpu
from oracle import binding as ob
from tests import common
from tests.test_gpu_intrinsics_pcg_vs_oracle import _pcg_setup
from tests.test_gpu_pcg_stages import INVALID, _Vec

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _unknowns(g, N, pose_kfs, di):
    return 6 * pose_kfs + 3 * N + ((5 + g.cf_w * g.cf_h + 4) if di else 0)


def _run(g, windowed, di=False, gauge=1, max_inner_iterations=30):
    g.update_surfel_normals()
    steps, conv = g.pcg_iteration(optimize_poses=True, optimize_geometry=True, optimize_depth_intrinsics=di, optimize_color_intrinsics=di,
                                  gauge_keyframe=gauge, max_inner_iterations=max_inner_iterations, windowed=windowed)
    return dict(steps=steps, conv=conv, surfels=g.download_surfels(), poses=[kf["pose"].copy() for kf in g.keyframes],
                cfactor=g.cfactor.download(), a=g.dp.a)


def _window_scene(mode, activations, active_mask, seed=21, num_keyframes=5):
    scene = common.small_scene(num_keyframes=num_keyframes, seed=seed)
    _, g, data, _ = _pcg_setup(scene, mode)
    for k, a in enumerate(activations):
        g.keyframes[k]["activation"] = a
    g.bind_keyframes()
    if active_mask is not None:
        g.upload_surfels(data, active_mask(data.shape[1]).astype(np.uint8))
    return scene, g, data


@pytest.mark.parametrize("mode", ["poses+geometry", "all"])
def test_all_active_is_the_whole_map_iteration(mode):
    """Every keyframe kActive and every surfel active: the system of bahip_pcg_iteration with the same gauge -- delta, inner steps,
    poses, surfel rows 0-7, cfactors and intrinsics bit for bit."""
    di = mode == "all"
    K = 5
    _, g, data = _window_scene(mode, [capi.KF_ACTIVE] * K, None)
    _, h, _ = _window_scene(mode, [capi.KF_ACTIVE] * K, None)
    N = data.shape[1]
    U = _unknowns(g, N, K - 1, di)
    ref = _run(g, windowed=False, di=di)
    out = _run(h, windowed=True, di=di)
    assert h.ctx.arithmetic == "exact"
    assert out["steps"] == ref["steps"] > 0 and out["conv"] == ref["conv"]
    assert np.array_equal(_bits(h.read_pcg_vector(2, U)), _bits(g.read_pcg_vector(2, U)))
    for k in range(K):
        assert np.array_equal(_bits(out["poses"][k]), _bits(ref["poses"][k])), k
    assert np.array_equal(_bits(out["surfels"][:8]), _bits(ref["surfels"][:8]))
    assert np.array_equal(_bits(out["cfactor"]), _bits(ref["cfactor"]))
    assert out["a"] == ref["a"] and h.depth_cam.fx == g.depth_cam.fx and h.color_cam.cx == g.color_cam.cx
    sk, tiles = C.c_int(), C.c_uint32()
    capi.check(h.ctx.lib.bahip_pcg_window_size(h.ctx.handle, C.byref(sk), C.byref(tiles)))
    assert sk.value == K and tiles.value == -(-N // 64)


@pytest.mark.parametrize("mode", ["poses+geometry", "all"])
def test_all_active_fast_flavour_is_the_whole_map_iteration_within_tolerance(mode):
    """The fast flavour of the windowed sweeps (bahip::fast, FASTFTZ_kernels_pcg_window) against the fast flavour of the whole-map
    iteration, everything active: the bars of tests/test_gpu_fast_flavour.py -- 99.9 % of the surfel positions and every pose within
    1e-5 -- and the same number of inner steps give or take one."""
    di = mode == "all"
    K = 5
    _, g, data = _window_scene(mode, [capi.KF_ACTIVE] * K, None)
    _, h, _ = _window_scene(mode, [capi.KF_ACTIVE] * K, None)
    for scene in (g, h):
        scene.ctx.set_arithmetic("fast")
    ref = _run(g, windowed=False, di=di)
    out = _run(h, windowed=True, di=di)
    assert h.ctx.arithmetic == "fast" and ref["steps"] > 0
    assert abs(out["steps"] - ref["steps"]) <= 1, (out["steps"], ref["steps"])
    dpos = np.abs(out["surfels"][:3] - ref["surfels"][:3]).max(axis=0)
    assert np.percentile(dpos, 99.9) < 1e-5, np.percentile(dpos, 99.9)
    moved = np.abs(out["surfels"][:3] - data[:3]).max(axis=0)
    assert np.median(moved) > 1e-4                      # a real update happened
    for k in range(K):
        assert np.abs(out["poses"][k].astype(np.float64) - ref["poses"][k]).max() < 1e-5, k
    if di:
        assert abs(out["a"] - ref["a"]) < 1e-5 and abs(h.depth_cam.fx - g.depth_cam.fx) < 1e-3


def test_disjoint_groups_windowed_on_one_are_the_oracle_on_that_group_alone():
    """Group A: the scene of tests/test_gpu_intrinsics_pcg_vs_oracle.py.  Group B: the same keyframes and surfels 100 m away (nothing
    co-visible).  Windowed on A (A kActive, B kInactive, B's surfels inactive), with a gauge named in B -- so the fall-back to the first
    kActive keyframe holds it -- the call equals the CPU oracle's whole-map PCG on a scene of A alone with gauge 0: inner steps, A's
    surfel rows 0-7 and poses bit for bit.  B keeps every bit.  (B's surfels start inside A's last 64-surfel tile: inactive lanes add
    exact zeros there, as the lanes past the end of A's buffer do in the oracle.)"""
    scene = common.small_scene(num_keyframes=5, seed=21)
    ba, g, data, perturbed = _pcg_setup(scene, "poses+geometry")
    K, N = len(perturbed), data.shape[1]
    shift = np.float32(100.0)
    b_poses = []
    for k, T in enumerate(perturbed):
        T2 = np.asarray(T, np.float32).copy()
        T2[4] += shift                                   # (qx, qy, qz, qw, tx, ty, tz)
        g.add_keyframe(scene.depth[k], scene.rgb[k], T2)
        b_poses.append(T2)
    data_b = data.copy()
    data_b[0] += shift
    both = np.ascontiguousarray(np.concatenate([data, data_b], axis=1))
    g.upload_surfels(both, np.concatenate([np.ones(N, np.uint8), np.zeros(N, np.uint8)]))
    for k in range(2 * K):
        g.keyframes[k]["activation"] = capi.KF_ACTIVE if k < K else capi.KF_INACTIVE
    g.bind_keyframes()
    b_before = g.download_surfels()[:, N:].copy()

    stats = ba.bundle_adjustment(optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=1, use_pcg=True,
                                 increase_ba_iteration_count=False, pcg_gauge_keyframe=0)
    out = _run(g, windowed=True, gauge=K + 2)
    assert 3 <= stats.pcg_inner_steps_total <= 30
    assert out["steps"] == stats.pcg_inner_steps_total, (out["steps"], stats.pcg_inner_steps_total)
    ref = ba.surfel_data[:, :N]
    assert np.median(np.abs(ref[:3] - data[:3]).max(axis=0)) > 1e-4   # a real update happened
    assert np.array_equal(_bits(out["surfels"][:8, :N]), _bits(ref[:8])), np.abs(out["surfels"][:3, :N] - ref[:3]).max()
    for k in range(K):
        assert np.array_equal(_bits(out["poses"][k]), _bits(np.asarray(ba.pose(k), np.float32))), k
        assert np.array_equal(_bits(out["poses"][K + k]), _bits(b_poses[k])), K + k
    assert np.array_equal(_bits(out["surfels"][:8, N:]), _bits(b_before[:8]))
    sk = C.c_int()
    capi.check(g.ctx.lib.bahip_pcg_window_size(g.ctx.handle, C.byref(sk), None))
    assert sk.value == K


def _chain_activations():
    # window [3, 5] of 8 keyframes; 2 and 6 co-visible; 0, 1 and 7 inactive
    A, CV, IN = capi.KF_ACTIVE, capi.KF_COVISIBLE_ACTIVE, capi.KF_INACTIVE
    return [IN, IN, CV, A, A, A, CV, IN]


def _half(n):
    rng = np.random.Generator(np.random.PCG64(5))
    return rng.uniform(size=n) < 0.6


def _tiles(n):
    # whole 64-surfel tiles active or not: the buffer of the active surfels alone then has the same tiles, and the pose entries -- exact
    # sums of per-(tile, keyframe) binary32 halving trees (kernels_pcg.hip: "DEFINITION of the dense sums") -- the same terms
    return (np.arange(n) // 64) % 3 != 1


def test_the_stage_driver_over_the_swept_keyframes_on_the_active_surfels():
    """The fused windowed call equals the stage-by-stage driver run over the swept keyframes (per-keyframe pose indices, co-visible
    poses fixed) on a buffer of the active surfels in the same order and the same tiles: delta, inner steps, updated poses and
    surfels; inactive surfels and fixed poses keep their bits."""
    acts = _chain_activations()
    K = len(acts)
    mode = "poses+geometry"
    _, g, data = _window_scene(mode, acts, _tiles, num_keyframes=K)
    active = _tiles(data.shape[1])
    N = data.shape[1]
    before_surfels = g.download_surfels()
    before_poses = [kf["pose"].copy() for kf in g.keyframes]
    out = _run(g, windowed=True, gauge=3)
    swept = [k for k in range(K) if acts[k] != capi.KF_INACTIVE]
    pose_kfs = [k for k in swept if acts[k] == capi.KF_ACTIVE]   # co-visible keyframes exist: no kActive pose is the gauge
    P = 6 * len(pose_kfs)
    U = P + 3 * N
    delta = g.read_pcg_vector(2, U)
    assert out["steps"] > 0 and out["conv"] >= K - len(pose_kfs)
    # bits that must not change: inactive surfels' rows, the poses that are not unknowns
    assert np.array_equal(_bits(out["surfels"][:8, ~active]), _bits(before_surfels[:8, ~active]))
    for k in range(K):
        if k not in pose_kfs:
            assert np.array_equal(_bits(out["poses"][k]), _bits(before_poses[k])), k
    assert not np.array_equal(_bits(out["surfels"][:8, active]), _bits(before_surfels[:8, active]))

    # the stage-by-stage driver on a scene that holds only the active surfels
    scene = common.small_scene(num_keyframes=K, seed=21)
    _, h, data2, _ = _pcg_setup(scene, mode)
    assert np.array_equal(data, data2)
    Na = int(active.sum())
    h.upload_surfels(np.ascontiguousarray(data[:, active]), np.ones(Na, np.uint8))
    for k in range(K):
        h.keyframes[k]["activation"] = acts[k]
    h.bind_keyframes()
    h.update_surfel_normals()
    lib, ctx = h.ctx.lib, h.ctx.handle
    Ua = P + 3 * Na
    layout = capi.PCGLayout(1, 1, 0, 0, 1, 1, Ua, P, INVALID, INVALID)
    r, M, dl, gv, p = (_Vec(h.ctx, Ua) for _ in range(5))
    an, ad, bn = (_Vec(h.ctx, 1) for _ in range(3))
    s = h.surfels_struct()
    frames = {k: h.frame_struct(k) for k in swept}
    Fs = {k: (C.c_float * 12)(*[float(v) for v in ob.se3_matrix3x4(ob.se3_inverse(ob.SE3.from_array(h.keyframes[k]["pose"])))]) for k in swept}
    index = {k: (6 * pose_kfs.index(k) if k in pose_kfs else INVALID) for k in swept}
    capi.check(lib.bahip_pcg_begin(ctx, C.byref(layout), Na))
    for k in swept:
        capi.check(lib.bahip_pcg_init(ctx, C.byref(layout), C.byref(frames[k]), Fs[k], index[k], int(k in pose_kfs), C.byref(s), r.ptr, M.ptr))
    capi.check(lib.bahip_pcg_init2(ctx, C.byref(layout), Na, h.dp.a, r.ptr, M.ptr, dl.ptr, gv.ptr, p.ptr, an.ptr))
    prev, no_improvement, steps = np.inf, 0, 0
    for step in range(30):
        steps += 1
        if step > 0:
            an, bn = bn, an
            gv.buf.clear(0)
        for k in swept:
            capi.check(lib.bahip_pcg_step1(ctx, C.byref(layout), C.byref(frames[k]), Fs[k], index[k], int(k in pose_kfs), C.byref(s), p.ptr, gv.ptr))
        capi.check(lib.bahip_pcg_step2(ctx, C.byref(layout), Na, r.ptr, M.ptr, dl.ptr, gv.ptr, p.ptr, an.ptr, ad.ptr, bn.ptr))
        r_norm = float(np.sqrt(np.float32(bn.get()[0])))
        if r_norm < prev - 1e-3:
            no_improvement = 0
        else:
            no_improvement += 1
            if no_improvement >= 3:
                break
        prev = r_norm
        if step < 29:
            capi.check(lib.bahip_pcg_step3(ctx, C.byref(layout), Na, gv.ptr, p.ptr, an.ptr, bn.ptr))
    assert steps == out["steps"], (steps, out["steps"])
    d = dl.get()
    assert np.array_equal(_bits(d[:P]), _bits(delta[:P]))
    rows = delta[P:].reshape(N, 3)
    assert np.array_equal(_bits(d[P:].reshape(Na, 3)), _bits(rows[active]))
    assert not rows[~active].any()
    capi.check(lib.bahip_update_surfels_from_pcg_delta(ctx, C.byref(s), 1, P, dl.ptr))
    assert np.array_equal(_bits(h.download_surfels()[:8]), _bits(out["surfels"][:8, active]))


def test_inputs_outside_the_window_are_not_read_and_a_nan_inside_fails_the_call():
    """A kInactive keyframe's pose and an inactive surfel are not read: changing them (NaN in the surfel) changes no bit.  A NaN in
    an active surfel's descriptor trips the sticky flag: the call fails, and the context serves the next call."""
    acts = _chain_activations()
    K = len(acts)
    _, g, data = _window_scene("poses+geometry", acts, _half, num_keyframes=K)
    active = _half(data.shape[1])
    ref = _run(g, windowed=True, gauge=3)

    _, h, _ = _window_scene("poses+geometry", acts, _half, num_keyframes=K)
    bad = data.copy()
    bad[:3, np.flatnonzero(~active)[:50]] = np.nan
    bad[6, np.flatnonzero(~active)[50:100]] = np.nan   # descriptor 1
    h.upload_surfels(bad, active.astype(np.uint8))
    far = h.keyframes[0]["pose"].copy()
    far[4:] += 0.25                       # an inactive keyframe moved (its pose is not read)
    h.keyframes[0]["pose"] = far
    h.keyframes[7]["pose"] = far
    h.bind_keyframes()
    out = _run(h, windowed=True, gauge=3)
    assert out["steps"] == ref["steps"]
    assert np.array_equal(_bits(out["surfels"][:8, active]), _bits(ref["surfels"][:8, active]))
    for k in range(2, 7):
        assert np.array_equal(_bits(out["poses"][k]), _bits(ref["poses"][k])), k

    worse = data.copy()
    worse[6, active] = np.nan             # descriptor 1 of every active surfel: non-finite descriptor residuals
    h.upload_surfels(worse, active.astype(np.uint8))
    with pytest.raises(capi.BackendError, match="non-finite"):
        _run(h, windowed=True, gauge=3)
    h.upload_surfels(data, active.astype(np.uint8))
    _run(h, windowed=True, gauge=3)       # usable again


def test_a_kinactive_keyframes_images_are_not_read_and_a_swept_ones_are():
    """Garbage in the depth image of a kInactive keyframe (0) changes no bit of the windowed result; the same garbage in a swept,
    co-visible keyframe (2) changes it.  (Depth is uint16: no NaN there; a non-finite term is the descriptor case below.)"""
    acts = _chain_activations()
    K = len(acts)
    scene = common.small_scene(num_keyframes=K, seed=21)
    _, _, data, perturbed = _pcg_setup(scene, "poses+geometry")
    active = _half(data.shape[1])
    garbage = np.random.Generator(np.random.PCG64(8)).integers(1, 65535, np.asarray(scene.depth[0]).shape, dtype=np.uint16)

    def run(poisoned):
        s = copy.copy(scene)
        s.depth = list(scene.depth)
        if poisoned is not None:
            s.depth[poisoned] = garbage
        h = common.build_gpu(s, 400000, create_from=[])
        h.upload_surfels(data, active.astype(np.uint8))
        for k in range(K):
            h.keyframes[k]["pose"] = np.asarray(perturbed[k], np.float32)
            h.keyframes[k]["activation"] = acts[k]
        h.bind_keyframes()
        return _run(h, windowed=True, gauge=3)

    ref, inactive, swept = run(None), run(0), run(2)
    assert ref["steps"] > 0
    assert inactive["steps"] == ref["steps"]
    assert np.array_equal(_bits(inactive["surfels"][:8]), _bits(ref["surfels"][:8]))
    for k in range(K):
        assert np.array_equal(_bits(inactive["poses"][k]), _bits(ref["poses"][k])), k
    assert not np.array_equal(_bits(swept["surfels"][:8, active]), _bits(ref["surfels"][:8, active]))


def test_refusals_leave_the_context_usable():
    _, g, _ = _window_scene("poses+geometry", [capi.KF_ACTIVE] * 5, None)
    g.set_pcg_sum_classes(2)
    with pytest.raises(capi.BackendError, match="keyframe class"):
        _run(g, windowed=True)
    g.set_pcg_sum_classes(1)
    lib, ctx = g.ctx.lib, g.ctx.handle
    capi.check(lib.bahip_context_set_keyframe_sharding(ctx, 0, 2))
    with pytest.raises(capi.BackendError, match="keyframe sharding"):
        _run(g, windowed=True)
    capi.check(lib.bahip_context_set_keyframe_sharding(ctx, 0, 1))
    assert _run(g, windowed=True)["steps"] > 0


def test_no_active_keyframe_is_nothing_to_solve():
    _, g, _ = _window_scene("poses+geometry", [capi.KF_COVISIBLE_ACTIVE, capi.KF_INACTIVE] * 2 + [capi.KF_INACTIVE], None)
    g.update_surfel_normals()             # (the normals update of _run then writes the same bits again)
    before = g.download_surfels()
    out = _run(g, windowed=True)
    assert out["steps"] == 0 and out["conv"] == 5
    assert np.array_equal(_bits(out["surfels"]), _bits(before))


@pytest.mark.parametrize("world", [2, 4])
def test_surfel_sharding_is_the_unsharded_windowed_call(world):
    """Surfel shards (chunks of 1024) exchanged through an in-process loopback: the windowed call on every rank gives the unsharded
    call's bits.  The active surfels lie in the first half of the cloud, so at world 4 some rank has no active tile."""
    import torch
    from tests.test_gpu_sharded_loopback import _Loopback
    torch.cuda.set_device(0)
    acts = [capi.KF_INACTIVE, capi.KF_COVISIBLE_ACTIVE, capi.KF_ACTIVE, capi.KF_ACTIVE, capi.KF_COVISIBLE_ACTIVE]
    first_half = lambda n: np.arange(n) < min(n // 2, 2048)   # noqa: E731
    scene, g, data = _window_scene("poses+geometry", acts, first_half)
    N = data.shape[1]
    active = first_half(N)
    ref = _run(g, windowed=True, gauge=2)

    loop = _Loopback(world)
    results, errors = [None] * world, []

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            _, gr, _, _ = _pcg_setup(scene, "poses+geometry")
            mine = multigpu.shard_chunks(N, rank, world, chunk=1024)
            gr.upload_surfels(np.ascontiguousarray(data[:, mine]), active[mine].astype(np.uint8))
            for k, a in enumerate(acts):
                gr.keyframes[k]["activation"] = a
            gr.bind_keyframes()
            hook = loop.hook_for(rank)
            capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
            out = _run(gr, windowed=True, gauge=2)
            tiles = C.c_uint32()
            capi.check(gr.ctx.lib.bahip_pcg_window_size(gr.ctx.handle, None, C.byref(tiles)))
            results[rank] = dict(mine=mine, out=out, tiles=tiles.value, keep=hook, scene=gr)
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
    if world == 4:
        assert min(r["tiles"] for r in results) == 0
    merged = np.zeros_like(ref["surfels"])
    for r in results:
        assert r["out"]["steps"] == ref["steps"]
        for k in range(len(acts)):
            assert np.array_equal(_bits(r["out"]["poses"][k]), _bits(ref["poses"][k])), k
        merged[:, r["mine"]] = r["out"]["surfels"]
    assert np.array_equal(_bits(merged[:8]), _bits(ref["surfels"][:8]))
