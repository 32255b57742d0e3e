"""The value of the BA objective on the GPU (bahip_evaluate_cost / bahip_evaluate_frame_cost; kernels_cost.hip).

Definition: over every associated (surfel, keyframe) pair, the depth term 1 * TukeyCost(raw, 10) and -- where the colour pixel is valid --
the two descriptor terms 1e-2 * HuberCost(raw, 10); each sum the exact sum of its binary32 terms, rounded once to binary64.  So the sums
are checked bit for bit against math.fsum of the per-pair terms (the production residuals from the per-pair hook, the robust costs
written as the oracle writes them), and must not move with the launch shape, the tile order, the surfel order or the sharding."""
import ctypes as C
import math

import numpy as np
import pytest

from badslam_amd import capi, multigpu, synthetic
from tests import common
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks
from tests.test_gpu_keyframe_sharded_lifecycle import _frame_T_global_3x4

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = [(True, True), (True, False), (False, True)]


def _tukey_cost(r):
    """oracle_internal.h: weighted_depth_residual = 1 * tukey_residual(r, 10), in binary32 operation for operation."""
    k = F32(10)
    c = F32(1) / F32(6)
    if abs(r) < k:
        q = r * F32(0.1)
        t = F32(1) - q * q
        return F32(1) * (c * k * k * (F32(1) - t * t * t))
    return F32(1) * (c * k * k)


def _huber_cost(r):
    """oracle_internal.h: weighted_descriptor_residual = 1 * 1e-2 * huber_residual(r, 10)."""
    k = F32(10)
    a = abs(r)
    h = (F32(0.5) * r * r) if a < k else (k * (a - F32(0.5) * k))
    return (F32(1) * F32(1e-2)) * h


def _expected(g, use_depth, use_desc):
    """Per keyframe [depth, desc1, desc2, depth count, pair count] from the per-pair hook and math.fsum; and the term lists."""
    idx = np.arange(g.surfels_size, dtype=np.uint32)
    per, terms = [], [[], [], []]
    for k, kf in enumerate(g.keyframes):
        out = g.evaluate_pairs(k, idx, _frame_T_global_3x4(kf["pose"]))
        assoc = out[:, 0] == 1
        col = assoc & (out[:, 3] == 1)
        d = [_tukey_cost(F32(r)) for r in out[assoc, 5]] if use_depth else []
        d1 = [_huber_cost(F32(r)) for r in out[col, 14]] if use_desc else []
        d2 = [_huber_cost(F32(r)) for r in out[col, 15]] if use_desc else []
        for t, v in zip(terms, (d, d1, d2)):
            t.extend(v)
        per.append(dict(depth=math.fsum(map(float, d)), descriptor_1=math.fsum(map(float, d1)), descriptor_2=math.fsum(map(float, d2)),
                        depth_residuals=len(d), descriptor_pairs=len(d1)))
    total = dict(depth=math.fsum(map(float, terms[0])), descriptor_1=math.fsum(map(float, terms[1])),
                 descriptor_2=math.fsum(map(float, terms[2])), depth_residuals=len(terms[0]), descriptor_pairs=len(terms[1]))
    return total, per


def _key(cost):
    """Bits of a cost dict (NaN compares equal to NaN)."""
    return tuple(np.float64(cost[n]).view(np.uint64).item() for n in ("depth", "descriptor_1", "descriptor_2")) + \
        (cost["depth_residuals"], cost["descriptor_pairs"])


def _keys(result):
    total, per = result
    return _key(total), [_key(c) for c in per]


def _scene_gpu(num_keyframes=5, seed=3, perturb=True):
    scene = common.small_scene(num_keyframes=num_keyframes, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    poses = [T if (k == 0 or not perturb) else synthetic.perturb_pose(rng, T, 0.01, 0.004) for k, T in enumerate(scene.poses_gt)]
    g = common.build_gpu(scene, 400000, create_from=[0, 2])
    for k, T in enumerate(poses):
        g.keyframes[k]["pose"] = np.asarray(T, np.float32)
    g.bind_keyframes()
    return scene, poses, g


def _set_shape(waves=0, workgroups=0, slice_=0, tile_order=-1):
    capi.check(capi.load().bahip_debug_set_cost_shape(waves, workgroups, slice_, tile_order))


@pytest.fixture(scope="module")
def scene_gpu():
    return _scene_gpu()


# ---- (1) exactness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_depth,use_desc", KINDS)
def test_sums_are_the_exact_sums_of_the_per_pair_terms(scene_gpu, use_depth, use_desc):
    _, _, g = scene_gpu
    total, per = g.evaluate_cost(use_depth, use_desc)
    exp_total, exp_per = _expected(g, use_depth, use_desc)
    assert exp_total["depth_residuals"] + exp_total["descriptor_pairs"] > 1000, exp_total
    for k, (got, exp) in enumerate(zip(per, exp_per)):
        assert _key(got) == _key(exp), (k, got, exp)
    assert _key(total) == _key(exp_total), (total, exp_total)


@pytest.mark.parametrize("use_depth,use_desc", KINDS)
def test_total_matches_the_oracle_cost(use_depth, use_desc):
    scene = common.small_scene(num_keyframes=3, seed=11)
    ba = common.build_oracle(scene, 300000, use_depth=use_depth, use_desc=use_desc)
    g = common.build_gpu(scene, 300000, create_from=[])
    data, active = common.oracle_surfels(ba)
    g.upload_surfels(data, active)
    g.bind_keyframes()
    total, _ = g.evaluate_cost(use_depth, use_desc)
    ref, ref_count = ba.evaluate_cost()
    got = total["depth"] + total["descriptor_1"] + total["descriptor_2"]
    assert ref_count > 1000
    assert total["depth_residuals"] + 2 * total["descriptor_pairs"] == ref_count
    assert abs(got - ref) <= 1e-9 * abs(ref), (got, ref)


# ---- (2) determinism ----------------------------------------------------------------------------------------------------------------
def test_same_bits_across_calls_shapes_tile_orders_and_surfel_order():
    scene, poses, g = _scene_gpu(seed=5)
    g.estimate_keyframe_poses(True, True)     # a pose phase over the table leaves the heavy-first run order behind
    for k, T in enumerate(poses):
        g.keyframes[k]["pose"] = np.asarray(T, np.float32)
    g.bind_keyframes()
    ref = _keys(g.evaluate_cost())
    assert _keys(g.evaluate_cost()) == ref
    try:
        for shape in [(1, 1, 1, 0), (8, 0, 0, 1), (4, 37, 3, 0), (2, 5, 2, 1), (8, 3, 256, 0), (1, 1000, 4, 1)]:
            _set_shape(*shape)
            assert _keys(g.evaluate_cost()) == ref, shape
    finally:
        _set_shape()
    data = g.download_surfels()
    perm = np.random.Generator(np.random.PCG64(8)).permutation(data.shape[1])
    g.upload_surfels(np.ascontiguousarray(data[:, perm]), np.ones(data.shape[1], np.uint8))
    assert _keys(g.evaluate_cost()) == ref


def _pair_terms(g, use_fast):
    """Per keyframe, from the per-pair hook in one flavour: associated mask, colour-valid mask, and the largest descriptor term."""
    g.ctx.set_arithmetic("fast" if use_fast else "exact")
    try:
        idx = np.arange(g.surfels_size, dtype=np.uint32)
        out = []
        for k, kf in enumerate(g.keyframes):
            o = g.evaluate_pairs(k, idx, _frame_T_global_3x4(kf["pose"]))
            assoc = o[:, 0] == 1
            col = assoc & (o[:, 3] == 1)
            desc = [_huber_cost(F32(r)) for r in np.concatenate([o[col, 14], o[col, 15]])]
            out.append((assoc, col, float(max(desc, default=0.0))))
        return out
    finally:
        g.ctx.set_arithmetic("exact")


def test_the_fast_flavour_is_deterministic_and_close_to_the_exact_one():
    _, _, g = _scene_gpu(seed=7)
    exact = g.evaluate_cost()
    g.ctx.set_arithmetic("fast")
    try:
        fast = g.evaluate_cost()
        assert _keys(g.evaluate_cost()) == _keys(fast)
        _set_shape(2, 7, 2, 0)
        assert _keys(g.evaluate_cost()) == _keys(fast)
    finally:
        _set_shape()
        g.ctx.set_arithmetic("exact")
    assert _keys(g.evaluate_cost()) == _keys(exact)
    e, f = exact[0], fast[0]
    # The flavours may decide a few associations differently (tests/test_gpu_fast_flavour.py: at most 1e-3 of the pairs).  Those
    # pairs, counted from the per-pair hook of both flavours, are the only slack beyond 1e-5 relative: each moves a sum by at most its
    # largest term (depth: the Tukey cost's ceiling 100 / 6; descriptors: the largest term either flavour has).  None flipped: 1e-5.
    ex, fa = _pair_terms(g, False), _pair_terms(g, True)
    depth_flips = sum(int(np.count_nonzero(a[0] != b[0])) for a, b in zip(ex, fa))
    desc_flips = sum(int(np.count_nonzero(a[1] != b[1])) for a, b in zip(ex, fa))
    desc_max = max(max(a[2], b[2]) for a, b in zip(ex, fa))
    assert depth_flips <= 1e-3 * e["depth_residuals"] and desc_flips <= 1e-3 * e["descriptor_pairs"], (depth_flips, desc_flips)
    assert abs(f["depth_residuals"] - e["depth_residuals"]) <= depth_flips
    assert abs(f["descriptor_pairs"] - e["descriptor_pairs"]) <= desc_flips
    for n, slack in (("depth", depth_flips * 100.0 / 6.0), ("descriptor_1", desc_flips * desc_max), ("descriptor_2", desc_flips * desc_max)):
        assert abs(f[n] - e[n]) <= 1e-5 * abs(e[n]) + slack, (n, f[n], e[n], slack)


# ---- (3) sharding ---------------------------------------------------------------------------------------------------------------------
def _surfel_shards(scene_gpu, world, chunk):
    scene, poses, g = scene_gpu
    ref = _keys(g.evaluate_cost())
    data = g.download_surfels()
    N = data.shape[1]
    chunk = chunk or 64 * -(-N // (64 * (world - 1)))     # 0: the cloud fits world - 1 chunks, the last rank's shard is empty

    def rank_main(rank, hook):
        gr = common.build_gpu(scene, 400000, create_from=[])
        mine = multigpu.shard_chunks(N, rank, world, chunk=chunk)
        gr.upload_surfels(np.ascontiguousarray(data[:, mine]), np.ones(mine.size, np.uint8))
        for k, T in enumerate(poses):
            gr.keyframes[k]["pose"] = np.asarray(T, np.float32)
        gr.bind_keyframes()
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        frame = gr.evaluate_frame_cost(1, _frame_T_global_3x4(poses[1]))
        return dict(cost=_keys(gr.evaluate_cost()), frame=_key(frame), size=int(mine.size), keep=(hook, gr))

    results, loop = _run_ranks(world, rank_main)
    for rank, r in enumerate(results):
        assert r["cost"] == ref, rank
        assert r["frame"] == ref[1][1], rank
    assert loop.calls == 2
    return [r["size"] for r in results]


@pytest.mark.parametrize("world", [2, 4, 8])
def test_surfel_shards_give_the_unsharded_bits(scene_gpu, world):
    _surfel_shards(scene_gpu, world, 1024)


def test_an_empty_surfel_shard_joins_the_exchange_and_returns_the_unsharded_bits(scene_gpu):
    """A rank whose shard holds no surfel (a small cloud over many ranks) sweeps nothing but still takes part in both exchanges; every
    rank, the empty one included, returns the unsharded bits."""
    sizes = _surfel_shards(scene_gpu, 8, 0)
    assert sizes[-1] == 0 and min(sizes[:-1]) > 0, sizes


@pytest.mark.parametrize("world", [2, 4, 8])
def test_keyframe_shards_give_the_unsharded_bits(world):
    scene, poses, g = _scene_gpu(num_keyframes=9, seed=13)
    ref = _keys(g.evaluate_cost())
    data = g.download_surfels()
    N = data.shape[1]

    def rank_main(rank, hook):
        gr = common.build_gpu(scene, 400000, create_from=[])
        gr.upload_surfels(data, np.ones(N, np.uint8))
        for k, T in enumerate(poses):
            gr.keyframes[k]["pose"] = np.asarray(T, np.float32)
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        gr.set_sum_classes(8)                                  # (the cost does not depend on it; sharding over 8 ranks needs it)
        gr.set_keyframe_sharding(rank, world)
        rng = np.random.Generator(np.random.PCG64(3 + rank))
        for k in range(len(poses)):                            # other ranks' keyframes: scrambled images, and handed over
            if k % world != rank:
                for which in ("depth", "normals", "radius"):
                    buf = gr.keyframes[k][which]
                    buf.upload(rng.integers(0, 1 << 16, size=(buf.height, buf.width), dtype=np.uint16))
        gr.kf_shard = (0, 1)                                   # (bind_keyframes then passes every frame's pointers)
        gr.bind_keyframes()
        own = rank % len(poses)
        frame = gr.evaluate_frame_cost(own, _frame_T_global_3x4(poses[own]))
        return dict(cost=_keys(gr.evaluate_cost()), frame=(own, _key(frame)), keep=(hook, gr))

    results, loop = _run_ranks(world, rank_main)
    for rank, r in enumerate(results):
        assert r["cost"] == ref, rank
        own, frame = r["frame"]
        assert frame == ref[1][own], rank
    assert loop.calls == 1                                     # the frame call exchanges nothing under keyframe sharding


def test_a_failing_exchange_fails_the_call_and_leaves_the_context_usable(scene_gpu):
    _, _, g = scene_gpu
    ref = _keys(g.evaluate_cost())
    failing = capi.ALLREDUCE_FN(lambda *_: 1)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, failing, None))
    try:
        with pytest.raises(capi.BackendError, match="cost rows over the ranks"):
            g.evaluate_cost()
    finally:
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
    assert _keys(g.evaluate_cost()) == ref


# ---- (4) semantics ---------------------------------------------------------------------------------------------------------------------
def test_cost_falls_over_a_pose_phase():
    _, _, g = _scene_gpu(seed=17)
    before, _ = g.evaluate_cost()
    g.estimate_keyframe_poses(True, True)        # the device table carries the new poses
    after, _ = g.evaluate_cost()
    value = lambda c: c["depth"] + c["descriptor_1"] + c["descriptor_2"]
    assert value(after) < value(before), (before, after)


def test_a_nan_descriptor_poisons_exactly_the_keyframes_that_see_it():
    _, _, g = _scene_gpu(seed=19)
    data = g.download_surfels()
    idx = np.arange(data.shape[1], dtype=np.uint32)
    seen = np.zeros(data.shape[1], int)
    pairs = []
    for k, kf in enumerate(g.keyframes):
        out = g.evaluate_pairs(k, idx, _frame_T_global_3x4(kf["pose"]))
        pairs.append((out[:, 0] == 1) & (out[:, 3] == 1))
        seen += pairs[-1]
    victim = int(np.flatnonzero((seen >= 1) & (seen < len(g.keyframes)))[0])
    data[capi.SURFEL_DESCRIPTOR1, victim] = np.nan
    g.upload_surfels(data, np.ones(data.shape[1], np.uint8))
    total, per = g.evaluate_cost()
    assert all(math.isnan(total[n]) for n in ("depth", "descriptor_1", "descriptor_2"))
    for k, c in enumerate(per):   # a keyframe's three sums are NaN together; the other keyframes stay finite
        assert [math.isnan(c[n]) for n in ("depth", "descriptor_1", "descriptor_2")] == [bool(pairs[k][victim])] * 3, (k, c)


def test_frame_cost_of_a_bound_keyframe_is_its_entry(scene_gpu):
    _, poses, g = scene_gpu
    _, per = g.evaluate_cost()
    for k in range(len(poses)):
        assert _key(g.evaluate_frame_cost(k, _frame_T_global_3x4(poses[k]))) == _key(per[k]), k


def test_no_surfels_gives_zeros_without_a_launch(scene_gpu):
    scene, poses, _ = scene_gpu
    g = common.build_gpu(scene, 1000, create_from=[])
    g.bind_keyframes()
    total, per = g.evaluate_cost()
    assert _key(total) == _key(dict(depth=0.0, descriptor_1=0.0, descriptor_2=0.0, depth_residuals=0, descriptor_pairs=0))
    assert all(c["depth_residuals"] == 0 for c in per)
