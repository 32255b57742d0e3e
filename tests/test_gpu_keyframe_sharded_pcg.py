"""The PCG scheme under KEYFRAME sharding (bahip_context_set_keyframe_sharding + bahip_context_set_pcg_sum_classes).

The surfel block of r, M (PCGInit) and g (PCGStep1) is defined over C keyframe classes: per surfel entry and class a binary32 chain
over the class's keyframes (k % C == c) in ascending order, and the entry is ((p0 + p1) + p2) + ... (kernels_pcg.hip).  C = 1
(default) is the one chain over all keyframes of before.  A rank that holds whole classes sweeps its own, the class partials are
summed over the ranks as integers (bit patterns), the dense head and the dot products are exact sums as under surfel sharding -- so
every rank ends with the bits of the unsharded run with the same C.  The definition is pinned to the oracle: orc_pcg_assemble over
one class's keyframes gives that class's chains."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import common
from tests.test_gpu_keyframe_sharded_intrinsics import COLOR_OFFSET, DEPTH_OFFSET, _bits, _cam, _perturb, _run_ranks

pytestmark = pytest.mark.gpu


def _perturbed_scene(num_keyframes, seed=21):
    """A small scene, its surfels moved off the surfaces a little and its poses perturbed (what the PCG step has to correct)."""
    scene = common.small_scene(num_keyframes=num_keyframes, seed=seed)
    rng = np.random.Generator(np.random.PCG64(33))
    g = common.build_gpu(scene, 400000)
    data = g.download_surfels()
    data[2] += rng.uniform(0, 0.003, data.shape[1]).astype(np.float32)
    poses = [common.synthetic.perturb_pose(rng, T, 0.003, 0.0005) for T in scene.poses_gt]
    return scene, data, poses


def _prepare(g, data, poses, arithmetic="exact", classes=1, sum_classes=4, intrinsics=False):
    g.ctx.set_arithmetic(arithmetic)
    g.set_sum_classes(sum_classes)
    g.set_pcg_sum_classes(classes)
    g.upload_surfels(data, np.ones(data.shape[1], np.uint8))
    for k, T in enumerate(poses):
        g.keyframes[k]["pose"] = np.asarray(T, np.float32)
    if intrinsics:
        _perturb(g)
        g.dp.a = 0.0125
    g.set_intrinsics()


# ---- (a) the default is the definition of before -----------------------------------------------------------------------------
def test_class_count_set_back_to_one_is_the_default_pcg_iteration():
    """C = 4 and back to 1 on one context: r and M after the init alone (max_inner_iterations = 0) and after a whole outer iteration,
    the inner step count, poses and surfels are bit for bit those of a fresh context."""
    import torch
    torch.cuda.set_device(0)
    scene, data, poses = _perturbed_scene(5)

    def run(toggle):
        g = common.build_gpu(scene, 400000, create_from=[])
        _prepare(g, data, poses)
        if toggle:
            g.set_pcg_sum_classes(4)
            g.set_pcg_sum_classes(1)
        g.bind_keyframes()
        g.pcg_iteration(max_inner_iterations=0, gauge_keyframe=1)
        U = 6 * (len(poses) - 1) + 3 * data.shape[1]
        init = (g.read_pcg_vector(0, U), g.read_pcg_vector(1, U))
        g.update_surfel_normals()
        steps, conv = g.pcg_iteration(max_inner_iterations=30, gauge_keyframe=1)
        return dict(init=init, steps=steps, conv=conv, r=g.read_pcg_vector(0, U), M=g.read_pcg_vector(1, U),
                    poses=np.asarray([kf["pose"] for kf in g.keyframes]), surfels=g.download_surfels()[:8])

    fresh, toggled = run(False), run(True)
    assert fresh["steps"] >= 3
    assert (fresh["steps"], fresh["conv"]) == (toggled["steps"], toggled["conv"])
    for x, y in zip(fresh["init"], toggled["init"]):
        assert np.array_equal(_bits(x), _bits(y))
    for key in ("r", "M", "poses", "surfels"):
        assert np.array_equal(_bits(fresh[key]), _bits(toggled[key])), key


# ---- (b) the class definition, held against the oracle -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def pinned_pair():
    """Oracle + GPU scenes with identical surfels and poses, 9 keyframes (every class of C = 8 has one)."""
    scene = common.small_scene(num_keyframes=9, seed=21)
    rng = np.random.Generator(np.random.PCG64(33))
    ba = common.build_oracle(scene, 600000)
    g = common.build_gpu(scene, 600000, create_from=[])
    data, _ = common.oracle_surfels(ba)
    data[2] += rng.uniform(0, 0.003, data.shape[1]).astype(np.float32)
    ba.surfel_data[:, :data.shape[1]] = data
    g.upload_surfels(data, np.ones(data.shape[1], np.uint8))
    for k, T in enumerate(scene.poses_gt):
        T = common.synthetic.perturb_pose(rng, T, 0.003, 0.0005)
        ba.set_pose(k, T)
        g.keyframes[k]["pose"] = np.asarray(T, np.float32)
    g.bind_keyframes()
    ba.use_depth, ba.use_desc = 1, 1
    return ba, g, data.shape[1]


def _oracle_on(ba, keyframes, optimize_poses=True, gauge=0):
    """orc_pcg_assemble over the given keyframes only (in this order): (pose block, surfel block of r, of M)."""
    saved = ba.keyframes
    ba.keyframes = [saved[k] for k in keyframes]
    try:
        r, M = ba.pcg_assemble(optimize_poses, True, False, False, gauge_keyframe=gauge)
    finally:
        ba.keyframes = saved
    ps = 6 * (len(keyframes) - 1) if optimize_poses else 0
    return (r[:ps], M[:ps]), r[ps:], M[ps:]


def test_oracle_surfel_block_depends_only_on_the_keyframes_it_is_given(pinned_pair):
    ba, _g, N = pinned_pair
    ks = [1, 4, 7]
    _, r0, M0 = _oracle_on(ba, ks, gauge=0)
    _, r1, M1 = _oracle_on(ba, ks, gauge=2)
    _, r2, M2 = _oracle_on(ba, ks, optimize_poses=False)
    assert r0.size == 3 * N and np.count_nonzero(M0) > N
    for r, M in ((r1, M1), (r2, M2)):
        assert np.array_equal(_bits(r), _bits(r0)) and np.array_equal(_bits(M), _bits(M0))


@pytest.mark.parametrize("classes", [2, 8])
def test_class_chains_of_the_init_are_the_oracle_per_class(pinned_pair, classes):
    """The init's surfel block of r and M on one GPU with C classes = the per-class oracle blocks added in binary32 in class order;
    the pose entries (exact sums) = each keyframe's entries in its class's oracle state and in the all-keyframe one."""
    ba, g, N = pinned_pair
    K = len(ba.keyframes)
    g.set_pcg_sum_classes(classes)
    try:
        g.pcg_iteration(max_inner_iterations=0, gauge_keyframe=0)
        U = 6 * (K - 1) + 3 * N
        r, M = g.read_pcg_vector(0, U), g.read_pcg_vector(1, U)
    finally:
        g.set_pcg_sum_classes(1)
    ps = 6 * (K - 1)
    ref_r = ref_M = None
    for c in range(classes):
        ks = [k for k in range(K) if k % classes == c]
        (pr, pM), br, bM = _oracle_on(ba, ks)
        ref_r = br.copy() if ref_r is None else (ref_r + br).astype(np.float32)
        ref_M = bM.copy() if ref_M is None else (ref_M + bM).astype(np.float32)
        for j, k in enumerate(ks[1:], start=1):                                 # (the class state's gauge: its first keyframe)
            assert np.array_equal(_bits(r[6 * (k - 1):6 * k]), _bits(pr[6 * (j - 1):6 * j])), (c, k)
            assert np.array_equal(_bits(M[6 * (k - 1):6 * k]), _bits(pM[6 * (j - 1):6 * j])), (c, k)
    assert np.array_equal(_bits(r[ps:]), _bits(ref_r)), np.flatnonzero(_bits(r[ps:]) != _bits(ref_r))[:10]
    assert np.array_equal(_bits(M[ps:]), _bits(ref_M)), np.flatnonzero(_bits(M[ps:]) != _bits(ref_M))[:10]
    (all_pr, all_pM), one_r, _ = _oracle_on(ba, list(range(K)))
    assert np.array_equal(_bits(r[:ps]), _bits(all_pr)) and np.array_equal(_bits(M[:ps]), _bits(all_pM))
    assert np.count_nonzero(M[ps:]) > N
    assert not np.array_equal(_bits(ref_r), _bits(one_r))   # the class count is part of the definition


# ---- (c) loopback parity: keyframe shards vs the unsharded run with the same class count --------------------------------------
OUTER = 2


@pytest.mark.parametrize("intrinsics", [False, True], ids=["poses+geometry", "poses+geometry+intrinsics"])
@pytest.mark.parametrize("world,arithmetic", [(2, "exact"), (2, "fast"), (4, "exact"), (4, "fast"), (8, "exact"), (8, "fast")])
def test_keyframe_shards_reproduce_the_unsharded_pcg_iterations(world, arithmetic, intrinsics):
    """Two outer iterations (normals update + bahip_pcg_iteration) from perturbed poses (and cameras): every rank ends with the
    unsharded run's inner step counts, poses, surfels, cameras, a and cfactor, bit for bit."""
    import torch
    from badslam_amd import capi
    torch.cuda.set_device(0)
    scene, data, poses = _perturbed_scene(7 if world < 8 else 11)
    classes = 8 if world == 8 else 4
    opts = dict(optimize_depth_intrinsics=intrinsics, optimize_color_intrinsics=intrinsics, max_inner_iterations=30, gauge_keyframe=0)

    def run(gr):
        gr.bind_keyframes()
        out = []
        for _ in range(OUTER):
            gr.update_surfel_normals()
            out.append(gr.pcg_iteration(**opts))
        return dict(out=out, surfels=gr.download_surfels()[:8], poses=np.asarray([kf["pose"] for kf in gr.keyframes]),
                    color=_cam(gr.color_cam), depth=_cam(gr.depth_cam), a=np.float32(gr.dp.a), cfactor=gr.cfactor.download())

    g = common.build_gpu(scene, 400000, create_from=[])
    _prepare(g, data, poses, arithmetic, classes, classes, intrinsics)
    ref = run(g)

    def rank_main(rank, hook):
        gr = common.build_gpu(scene, 400000, create_from=[])
        _prepare(gr, data, poses, arithmetic, classes, classes, intrinsics)
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        gr.set_keyframe_sharding(rank, world)
        out = run(gr)
        out["keep"] = (hook, gr)
        return out

    results, loop = _run_ranks(world, rank_main)
    assert all(steps >= 3 for steps, _ in ref["out"]), ref["out"]
    assert loop.calls >= OUTER * (1 + 3 + 3 * min(steps for steps, _ in ref["out"]))
    for r in results:
        assert r["out"] == ref["out"]
        for key in ("poses", "surfels", "color", "depth", "a", "cfactor"):
            assert np.array_equal(_bits(r[key]), _bits(ref[key])), key
    assert np.count_nonzero(ref["surfels"][:3] != data[:3]) > data.shape[1]      # the iterations did something
    if intrinsics:
        assert np.abs(ref["depth"] - (np.asarray(scene.camera) + np.array(DEPTH_OFFSET)).astype(np.float32)).max() > 1e-3
        assert np.abs(ref["color"] - (np.asarray(scene.camera) + np.array(COLOR_OFFSET)).astype(np.float32)).max() > 1e-3


# ---- (d) DirectBA on a configs[2]-shaped slice, eight keyframe shards ----------------------------------------------------------
def test_eight_keyframe_shards_of_directba_pcg_are_the_unsharded_call():
    """BundleAdjustment(use_pcg = true, do_surfel_updates = false) of eight DirectBA instances in lockstep on one GPU,
    SetKeyframeSharding(rank, 8) with SetSumClasses(8) and SetPCGSumClasses(8), on a slice of the configs[2] scene (640 x 480,
    16 keyframes): every rank ends with the unsharded call's poses and surfels (same class counts), bit for bit.  The ranks leave
    the gauge keyframe to the keyframe-sharded default (keyframe 0); the unsharded call names it.  The 8-class definition against
    the 1-class one (everything else alike) is reported and held to BASELINE's pose bar (1e-5 m)."""
    import torch
    from badslam_amd import capi
    from badslam_amd.directba import DirectBA
    from tests.test_gpu_scale_parity import _bench_scene
    torch.cuda.set_device(0)
    bench_ba, data, poses_gt, args = _bench_scene(width=640, height=480, keyframes=16, surfels=10 ** 9)
    frames = args.frames
    K, N, WORLD = bench_ba.keyframe_count(), data.shape[1], 8
    assert N > 300000 and K == len(frames) == 16
    start_poses = [bench_ba.keyframe_pose(k) for k in range(K)]
    bench_ba.close()
    cam = common.synthetic.test_camera(args.width, args.height)
    call = dict(optimize_depth_intrinsics=False, optimize_color_intrinsics=False, do_surfel_updates=False, optimize_poses=True,
                optimize_geometry=True, min_iterations=1, max_iterations=1, use_pcg=True, active_keyframe_window_start=0,
                active_keyframe_window_end=K - 1, increase_ba_iteration_count=False, pcg_max_inner_iterations=10)

    def build(classes, gauge):
        rb = DirectBA(N + 4096, 1.0 / 5000, 40.0, args.cell, args.width, args.height, cam, cam)
        for (raw, rgb), T in zip(frames, poses_gt):
            rb.AddKeyframe(raw, rgb, T)
        for k, T in enumerate(start_poses):
            rb.set_keyframe_pose(k, T)
        rb.upload_surfels(data)
        rb.set_ba_iteration_counts(1, 1)                  # equal counters: no end-of-scheme tasks (fixed surfel set)
        rb.SetSumClasses(8)
        rb.SetPCGSumClasses(classes)
        if gauge is not None:
            rb.set_pcg_gauge_keyframe(gauge)
        return rb

    def outcome(rb, done):
        return dict(done=done, steps=rb.last_stats()["pcg_inner_steps"], poses=np.asarray([rb.keyframe_pose(k) for k in range(K)], np.float32),
                    surfels=rb.download_surfels(8))

    refs = {}
    for classes in (8, 1):
        rb = build(classes, 0)
        refs[classes] = outcome(rb, rb.BundleAdjustment(**call)[0])
        rb.close()
    ref = refs[8]
    assert ref["done"] == 1 and ref["steps"] >= 3

    ranks = [build(8, None) for _ in range(WORLD)]

    def rank_main(rank, hook):
        rb = ranks[rank]
        capi.check(capi.load().bahip_context_set_allreduce(rb.backend_context().handle, hook, None))
        rb.SetKeyframeSharding(rank, WORLD)
        out = outcome(rb, rb.BundleAdjustment(**call)[0])
        out["keep"] = hook
        return out

    t0 = time.perf_counter()
    results, loop = _run_ranks(WORLD, rank_main, timeout=900)
    wall = time.perf_counter() - t0
    for rb in ranks:
        rb.close()
    print(f"eight keyframe shards in loopback (one GPU, threads, torch copies for the all-reduce -- not a link measurement): one outer "
          f"iteration, {ref['steps']} inner steps, {loop.calls} exchanges: {wall:.2f} s wall")
    for rank, r in enumerate(results):
        assert (r["done"], r["steps"]) == (ref["done"], ref["steps"]), rank
        for key in ("poses", "surfels"):
            assert np.array_equal(_bits(r[key]), _bits(ref[key])), (rank, key)
    moved = np.abs(ref["poses"][:, 4:].astype(np.float64) - np.asarray(start_poses, np.float64)[:, 4:]).max()
    assert moved > 1e-6                                                           # the call did something

    one = refs[1]
    d = ref["poses"][:, 4:].astype(np.float64) - one["poses"][:, 4:]
    rmse = float(np.sqrt(np.mean(np.sum(d * d, axis=1))))
    print(f"configs[2] slice, PCG with 8 classes vs 1 (one outer iteration, {N} surfels, {ref['steps']} / {one['steps']} inner steps): "
          f"position RMSE {rmse:.3e} m, max {np.abs(d).max():.3e} m")
    assert rmse <= 1e-5


# ---- (e) robustness ----------------------------------------------------------------------------------------------------------
def test_a_non_finite_term_on_one_rank_fails_the_keyframe_sharded_pcg_call_on_every_rank():
    """Rank 1's copy of the cloud holds NaN descriptors (only rank 1's keyframes see them through its data), rank 0's is clean: both
    calls end with the same error after the same exchanges, none hangs (the flag travels in exchange 2)."""
    import torch
    from badslam_amd import capi
    torch.cuda.set_device(0)
    scene, data, poses = _perturbed_scene(5, seed=10)
    N = data.shape[1]
    outcomes = [None, None]

    def rank_main(rank, hook):
        gr = common.build_gpu(scene, 400000, create_from=[])
        mine = data.copy()
        if rank == 1:
            mine[6, N // 2:N // 2 + 256] = np.nan                               # descriptor 1 of a patch of surfels
        _prepare(gr, mine, poses, classes=2)
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        gr.set_keyframe_sharding(rank, 2)
        gr.bind_keyframes()
        gr.update_surfel_normals()
        try:
            gr.pcg_iteration(max_inner_iterations=30)
            outcomes[rank] = "no error"
        except RuntimeError as e:
            outcomes[rank] = str(e)
        return (outcomes[rank], hook, gr)

    results, loop = _run_ranks(2, rank_main, timeout=300)
    messages = [r[0] for r in results]
    assert all("non-finite term" in m for m in messages), messages
    assert messages[0] == messages[1]
    assert loop.calls == 1 + 3 + 3 * 6          # normals, the init's three exchanges, the first group of six inner steps (three each)


def test_what_the_keyframe_sharded_pcg_scheme_refuses():
    import torch
    from badslam_amd import capi
    torch.cuda.set_device(0)
    scene = common.small_scene(num_keyframes=3, seed=3)
    g = common.build_gpu(scene, 200000)
    lib, h = g.ctx.lib, g.ctx.handle
    for bad in (0, 3, 5, 16, -1):
        assert lib.bahip_context_set_pcg_sum_classes(h, bad) != 0 and b"1, 2, 4 or 8" in lib.bahip_last_error()
    for good in (1, 2, 4, 8):
        capi.check(lib.bahip_context_set_pcg_sum_classes(h, good))
    g.set_pcg_sum_classes(1)
    g.set_keyframe_sharding(1, 2)
    g.bind_keyframes()
    with pytest.raises(RuntimeError, match="keyframe sharding needs an all-reduce hook or an RCCL communicator"):
        g.pcg_iteration()
    with pytest.raises(RuntimeError, match="keyframe sharding needs an all-reduce hook or an RCCL communicator"):
        g.update_surfel_normals()
    hook = capi.ALLREDUCE_FN(lambda *a: 1)                                      # (a refused call never reaches the exchange)
    capi.check(lib.bahip_context_set_allreduce(h, hook, None))
    with pytest.raises(RuntimeError, match="keyframe sharding of the PCG scheme.*bahip_context_set_pcg_sum_classes"):
        g.pcg_iteration()                                                        # two ranks over one class
    g.set_sum_classes(8)
    g.set_keyframe_sharding(0, 8)
    g.bind_keyframes()
    g.set_pcg_sum_classes(4)
    with pytest.raises(RuntimeError, match="keyframe sharding of the PCG scheme.*bahip_context_set_pcg_sum_classes"):
        g.pcg_iteration()                                                        # eight ranks over four classes
    # the stage entry points, the colour assignment and the lifecycle stay refused
    g.set_pcg_sum_classes(8)
    with pytest.raises(RuntimeError, match="keyframe sharding.*bahip_pcg_iteration"):
        capi.check(lib.bahip_pcg_begin(h, C.byref(capi.PCGLayout()), 0))
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        capi.check(lib.bahip_assign_colors(h, C.byref(g.surfels_struct())))
    with pytest.raises(RuntimeError, match="keyframe sharding"):
        g.delete_surfels_and_update_radii(1)
    # a failing exchange of the normals update says what it was doing
    with pytest.raises(RuntimeError, match="keyframe sharding: the exchange of the normals update"):
        g.update_surfel_normals()
    capi.check(lib.bahip_context_set_allreduce(h, capi.ALLREDUCE_FN(), None))
    g.set_keyframe_sharding(0, 1)
    g.bind_keyframes()
    g.pcg_iteration(max_inner_iterations=2)                                      # unsharded again: runs (8 classes on one GPU)
