"""The state a lifecycle call leaves in the context, checked by the sweeps that come after it: the packed BA planes of the bound
keyframes (bahip_set_keyframes packs keyframe k into library slot 1 + k, and the keyframe table points there), the planes a merge
batch packs for frames handed over without planes, and slot 0 of the single-frame calls.

Every test builds the oracle and the HIP scene from the same synthetic scene, sets the same perturbed poses on both sides, binds the
keyframes, runs the lifecycle call under test on both sides and then -- WITHOUT rebinding -- runs the sweeps that read the bound
planes on both sides, bit for bit: activation + geometry step, the batched pose phase against the oracle's estimate_frame_pose of
every keyframe, and one colour-intrinsics step.  A test here must not call bind_keyframes() between the lifecycle call and the sweeps,
and must not use the lowlevel.Scene wrappers that do so implicitly (create_surfels_for_keyframe, create_surfels_for_keyframes and
lifecycle_batch(keyframes=...)): a rebind repacks every bound slot and would hide a call that wrote into them."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi, synthetic
from tests import common

pytestmark = pytest.mark.gpu

N = 6              # keyframes: a batch of a few of them leaves bound slots behind it that it must not touch either
CAPACITY = 500000


def _rows(a):
    return np.ascontiguousarray(a[:8]).view(np.uint32)


def _bits(values):
    return np.asarray(values, np.float32).view(np.uint32)


def _cam_tuple(c):
    return np.array([c.fx, c.fy, c.cx, c.cy], dtype=np.float64)


@pytest.fixture(scope="module")
def cloud():
    """The scene and a surfel cloud for it: the oracle's surfels of every keyframe (ground-truth poses) followed by 1 mm near-duplicates
    of a third of them, candidates for merging (as test_gpu_lifecycle_stages.py's test_merge_bit_exact builds it)."""
    scene = common.small_scene(num_keyframes=N, seed=31)
    data, _ = common.oracle_surfels(common.build_oracle(scene, CAPACITY))
    n = data.shape[1]
    rng = np.random.Generator(np.random.PCG64(3))
    pick = np.sort(rng.choice(n, n // 3, replace=False))
    dup = data[:, pick].copy()
    dup[:3] += rng.normal(0, 0.001, (3, len(pick))).astype(np.float32)
    return scene, np.concatenate([data, dup], axis=1)


def _world(cloud):
    """Oracle and HIP scene holding the same cloud, with the same perturbed poses and colour camera, keyframes bound."""
    scene, data = cloud
    orc = common.build_oracle(scene, CAPACITY, create_from=[])
    g = common.build_gpu(scene, CAPACITY, create_from=[])
    rng = np.random.Generator(np.random.PCG64(33))
    for k, T in enumerate(scene.poses_gt):
        P = synthetic.perturb_pose(rng, T, 0.003, 0.0005)
        orc.set_pose(k, P)
        g.keyframes[k]["pose"] = np.asarray(P, np.float32)
    for obj in (orc, g):            # so that the colour-intrinsics step has something to correct
        cam = obj.color_cam
        cam.fx += 0.4; cam.fy -= 0.3; cam.cx += 0.8; cam.cy -= 0.6
    g.set_intrinsics()
    g.bind_keyframes()
    orc.use_depth, orc.use_desc = 1, 1
    n = data.shape[1]
    orc.surfel_data[:, :n] = data
    orc.surfels.surfels_size = orc.surfels.surfel_count = n
    g.upload_surfels(data, np.zeros(n, np.uint8))
    return orc, g


def _frames(orc, order):
    return [np.array(list(orc.keyframes[k].frame_T_global), np.float32) for k in order]


def _cell_batches():
    out = C.c_longlong()
    capi.check(capi.load().bahip_debug_merge_cells_batches(C.byref(out)))
    return out.value


def _merge_with_planes(g, order, Fs, merge_dist_factor, planes):
    """bahip_merge_surfels_for_keyframes with planes[j] (a bahip_frame_planes handle, or None) in frame j's bahip_frame."""
    structs = (capi.Frame * len(order))(*[g.frame_struct(k) for k in order])
    for j, p in enumerate(planes):
        structs[j].planes = p
    F = (C.c_float * (12 * len(order)))(*[float(v) for T in Fs for v in T])
    merged = C.c_uint32()
    s = g.surfels_struct()
    capi.check(g.lib.bahip_merge_surfels_for_keyframes(g.ctx.handle, float(merge_dist_factor), structs, F, len(order), C.byref(s),
                                                       g._supporting_ptrs(), g.supporting[0].pitch, C.byref(merged)))
    g.ctx.synchronize()
    g.surfel_count -= merged.value
    return merged.value


def _merge_batch(orc, g, order, by_cells=True, planes=None, min_merged=100):
    """One merge batch on a lifecycle batch that knows its frames, against the oracle's merges in the same order; then compaction on
    both sides (what the BA loop does next).  by_cells: the route the batch must take (bahip_debug_merge_cells_batches)."""
    Fs = _frames(orc, order)
    batches, before = _cell_batches(), int(orc.surfels.surfel_count)
    n = orc.surfels_size
    with g.lifecycle_batch(frames=Fs):
        if planes is None:
            _, merged = g.merge_surfels_for_keyframes(order, Fs, merge_dist_factor=orc.merge_factor)
        else:
            merged = _merge_with_planes(g, order, Fs, orc.merge_factor, planes)
    for k in order:
        orc.determine_supporting_surfels(k, merge=True)
    assert _cell_batches() - batches == (1 if by_cells else 0), "the merge batch took the other route"
    assert merged == before - int(orc.surfels.surfel_count) and merged >= min_merged, (merged, before - int(orc.surfels.surfel_count))
    assert np.array_equal(_rows(g.surfel_buf.download()[:, :n]), _rows(orc.surfel_data[:, :n])), "merged surfels differ"
    g.compact_surfels(with_active=True)
    orc.compact_surfels()
    assert g.surfels_size == orc.surfels_size


def _sweeps(orc, g, label, intrinsics=True):
    """The sweeps that read the bound keyframes' planes, on both sides, bit for bit: activation + geometry step, the pose phase of every
    bound keyframe, and (last: it adopts the new colour camera) one colour-intrinsics step."""
    n = g.surfels_size
    assert n == orc.surfels_size and n > 10000
    g.update_surfel_activation()
    orc.update_surfel_activation()
    assert np.array_equal(g.active_buf.download()[0, :n], orc.active[:n]), f"{label}: activation"
    g.optimize_geometry_iteration(True, True)
    orc.optimize_geometry_iteration()
    got, ref = _rows(g.download_surfels()), _rows(orc.surfel_data[:, :n])
    assert np.array_equal(got, ref), f"{label}: geometry step: {np.count_nonzero(np.any(got != ref, axis=0))} of {n} surfels differ"
    poses, its, conv, _ = g.estimate_keyframe_poses(True, True)
    bound = len(g.keyframes)
    for k in range(bound):
        est, its_ref, conv_ref = orc.estimate_frame_pose(k, orc.pose(k))
        assert np.array_equal(_bits(poses[k]), _bits(est.to_array())), (f"{label}: pose of keyframe {k}", common.pose_error(est.to_array(), poses[k]))
        assert its[k] == its_ref and conv[k] == int(conv_ref), (f"{label}: keyframe {k}", its[k], its_ref, conv[k], conv_ref)
        # the device table carries the new poses (bahip_estimate_keyframe_poses); the oracle and a later bind follow
        orc.set_pose(k, est)
        g.keyframes[k]["pose"] = poses[k].astype(np.float32)
    if intrinsics:
        cc_r, _, _ = orc.optimize_intrinsics(False, True)
        cc_g, _, _ = g.optimize_intrinsics(False, True)
        assert np.array_equal(_bits(_cam_tuple(cc_g)), _bits(_cam_tuple(cc_r))), (label, _cam_tuple(cc_g), _cam_tuple(cc_r))


@pytest.mark.parametrize("order", [[3, 1], [(k + 1) % N for k in range(N)], [2, 0, 2], list(range(N))],
                         ids=["subset descending", "rotation", "repeated keyframe", "identity"])
def test_reordered_merge_batch_leaves_bound_planes(cloud, order):
    """A merge batch by cell lists whose frames come without BA planes, in an order other than 0, 1, 2, ...: the planes it packs for
    its frames must not be the bound keyframes' planes (the identity order is the control case)."""
    orc, g = _world(cloud)
    _merge_batch(orc, g, order)
    _sweeps(orc, g, f"after the batch {order}")


@pytest.mark.parametrize("length,by_cells", [(64, True), (65, False)], ids=["64 frames by cell lists", "65 frames pipelined"])
def test_merge_batch_at_the_frame_limit(cloud, length, by_cells):
    """64 frames without planes still go by cell lists, 65 take the pipelined route (which re-packs slot 0).  Frame j is keyframe
    (N - 1 - j) mod N: in the order 0, 1, ..., N - 1 frame j would land in keyframe j's own slot and hide an overwrite."""
    orc, g = _world(cloud)
    _merge_batch(orc, g, [(N - 1 - j) % N for j in range(length)], by_cells=by_cells)
    _sweeps(orc, g, f"after a batch of {length} frames")


def test_merge_batch_mixing_frames_with_and_without_planes(cloud):
    """A rotated batch in which every other frame brings BA planes of its own (bahip_frame_planes_create / _update) and the others
    are packed by the library."""
    orc, g = _world(cloud)
    lib, h = g.lib, g.ctx.handle
    order = [(k + 1) % N for k in range(N)]
    dc, cc = g.depth_cam, g.color_cam
    planes = [None] * len(order)
    try:
        for j in range(0, len(order), 2):
            p = C.c_void_p()
            capi.check(lib.bahip_frame_planes_create(h, dc.width, dc.height, cc.width, cc.height, C.byref(p)))
            planes[j] = p.value
            fr = g.frame_struct(order[j])
            capi.check(lib.bahip_frame_planes_update(h, p, C.byref(fr)))
        _merge_batch(orc, g, order, planes=planes)
        _sweeps(orc, g, "after the mixed batch")
    finally:
        g.ctx.synchronize()
        for p in planes:
            if p:
                lib.bahip_frame_planes_destroy(p)


def test_single_frame_calls_between_bound_sweeps(cloud):
    """The single-frame calls pack their frame into slot 0; interleaved with the sweeps over the bound keyframes, every step against
    the oracle: a merge for a keyframe other than 0, the pose normal equations of one frame, and the per-pair terms of one frame."""
    orc, g = _world(cloud)
    _sweeps(orc, g, "first", intrinsics=False)
    k = 3
    F = _frames(orc, [k])[0]
    before = int(orc.surfels.surfel_count)
    planes, merged = g.determine_supporting_surfels(k, F, merge=True, merge_dist_factor=orc.merge_factor)
    ref = orc.determine_supporting_surfels(k, merge=True)
    assert merged == before - int(orc.surfels.surfel_count) and merged > 100, merged
    assert np.array_equal(planes, ref)
    n = orc.surfels_size
    assert np.array_equal(_rows(g.surfel_buf.download()[:, :n]), _rows(orc.surfel_data[:, :n]))
    g.compact_surfels(with_active=True)
    orc.compact_surfels()
    _sweeps(orc, g, f"after the merge of keyframe {k}", intrinsics=False)
    k = 4
    H, b = g.accumulate_pose_coeffs(k, True, True, _frames(orc, [k])[0])
    H_ref, b_ref, count, _ = orc.accumulate_pose_coeffs(k, accumulate_double=False)
    assert count > 1000
    assert np.array_equal(_bits(H), _bits(H_ref)) and np.array_equal(_bits(b), _bits(b_ref))
    _sweeps(orc, g, f"after the pose sums of keyframe {k}", intrinsics=False)
    k = 2
    idx = np.arange(0, g.surfels_size, 7, dtype=np.uint32)
    out = g.evaluate_pairs(k, idx, _frames(orc, [k])[0])
    words, refi = out.view(np.uint32), orc.evaluate_pairs(k, idx)
    assoc = refi.view(np.int32)[:, 0] == 1
    assert np.array_equal(out[:, 0] == 1.0, assoc) and assoc.sum() > 1000, assoc.sum()
    a = np.flatnonzero(assoc)
    assert np.array_equal(out[a, 1].astype(np.int32), refi.view(np.int32)[a, 1]) and np.array_equal(out[a, 2].astype(np.int32), refi.view(np.int32)[a, 2])
    # (-0.0 and +0.0 are the same value: a compiler may turn -fma(a, b, -c) into fma(-a, b, c))
    x, y = words[a][:, 4:14].copy(), refi[a][:, 4:14].copy()      # calibrated depth, depth residual, weight, inverse stddev, Jacobian
    x[x == 0x80000000] = 0
    y[y == 0x80000000] = 0
    assert np.array_equal(x, y)
    _sweeps(orc, g, f"after the pair terms of keyframe {k}")


def test_rebinding_another_keyframe_count_between_merge_batches(cloud):
    """Merge batch, bind N - 2 keyframes, a second reordered merge batch, bind N again -- the sweeps after every step.  Whatever slots
    the batches pack into must stay apart from the bound ones when the bound count shrinks and grows again."""
    orc, g = _world(cloud)
    everyone = g.keyframes
    _merge_batch(orc, g, [(k + 1) % N for k in range(N)])
    _sweeps(orc, g, "after the first batch, N bound")
    g.keyframes = everyone[:N - 2]
    orc.deleted = {N - 2, N - 1}          # NULL entries at the end of the oracle's list: the first N - 2 keyframes
    g.bind_keyframes()
    _sweeps(orc, g, "N - 2 bound")
    _merge_batch(orc, g, [3, 0, 2, 1], min_merged=0)   # (the first batch merged most candidates away)
    _sweeps(orc, g, "after the second batch, N - 2 bound")
    g.keyframes = everyone
    orc.deleted = set()
    g.bind_keyframes()
    _sweeps(orc, g, "N bound again")
