"""The keyframe activation state machine of the alternating scheme on the device -- kActive / kCovisibleActive / kInactive, the rules
of B/direct_ba_alternating.cc:353-371 and :556-577 and B/direct_ba.cc:549-564 -- held to the oracle (oracle/oracle_ba.c) and to the
plain model of tests/keyframe_activation.py, which tests/test_cpu_keyframe_activation.py holds to the oracle.  Every comparison is
exact (integers and bit patterns), in the exact arithmetic flavour.  The device table is read with
bahip_debug_read_keyframe_activations.

  a  the activation kernels alone against the model, 1 .. 1025 keyframes: bahip_propagate_covisible_activation launches
     propagate_covisible_kernel at every K; bahip_apply_activation_window launches window_and_propagate_kernel (with its early
     return) up to 1024 keyframes and window_activation_kernel + propagate_covisible_kernel at 1025
  b  the pose phase's activation update at 1025 keyframes on an empty cloud (pose_init_from_keyframes_kernel<false> and its count)
  c  propagation, geometry step and pose phase, stage by stage, against the oracle iteration by iteration (S1, S2)
  d  bahip_alternating_iterations without a fixed window (iteration_begin_body modes 0 and 2) and with a partial one (mode 1),
     fused and unfused, with a pose phase that outruns the queue, against one oracle call
  e  DirectBA::BundleAdjustment with windows (-1, -1) and (2, 3) and with surfel updates against the oracle, under the host's own
     co-visibility lists
"""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi
from tests import common
from tests import keyframe_activation as ka

pytestmark = pytest.mark.gpu

A, CV, I = ka.ACTIVE, ka.COVISIBLE, ka.INACTIVE


# ---- a: the activation kernels alone --------------------------------------------------------------------------------------------------
def _table_case(K, seed):
    """Random states, a random partial window and random lists for K keyframes, with what makes a wrong kernel visible: an empty
    row; a row of more than 64 entries with duplicates whose only new target sits behind entry 64 (the lanes' stride loop);
    self-references; non-empty rows beyond the first pass of the 16 wavefronts, the last of them -- row K - 1; at K = 1025 in the
    table's last workgroup -- with a target nobody else lists."""
    rng = np.random.Generator(np.random.PCG64(seed))
    state = [int(v) for v in rng.integers(0, 3, K)]
    window = [int(v) for v in (rng.random(K) < 0.3)]
    if K == 1:
        return state, [0], [[0] * 70]
    lists = [[int(v) for v in rng.integers(0, K, int(rng.integers(1, 4)))] for _ in range(K)]
    for k in range(0, K, 5):
        lists[k].append(k)                                       # self-references
    long_row, far, empty, last, last_target = 3, 5, 1, K - 1, 9
    for l in lists:
        l[:] = [j for j in l if j not in (far, last_target)]
    lists[long_row] = [long_row] * 40 + [7] * 30 + [far] + [int(v) for v in rng.integers(0, K, 20) if v not in (far, last_target)]
    lists[empty] = []
    lists[last] = lists[last] + [last_target]
    for k, s, w in ((long_row, A, 1), (last, A, 1), (far, I, 0), (last_target, I, 0), (7, I, 0)):
        state[k], window[k] = s, w
    # More than 16 non-empty rows -- except at K = 17, where the empty row leaves exactly 16.  The kernels stride by row INDEX
    # (row = wave, wave + 16, ...), so what a second pass of the wavefronts needs is a non-empty row of index >= 16: row K - 1.
    assert sum(1 for l in lists if l) > (15 if K == 17 else 16) and last >= 16 and lists[last] and len(lists[long_row]) > 64
    return state, window, lists


@pytest.mark.parametrize("K", [1, 17, 65, 1024, 1025])
def test_activation_kernels_against_the_model(K):
    state, window, lists = _table_case(K, 100 + K)
    scene = common.small_scene(num_keyframes=1, width=64, height=48, seed=3)       # nothing samples the images
    g = common.build_gpu(scene, 1024, create_from=[])
    g.keyframes = [dict(g.keyframes[0], activation=s) for s in state]             # K table entries on one image set
    g.bind_keyframes()
    ka.set_covisibility(g, lists)
    assert g.read_keyframe_activations() == state                                  # the hook reads what was bound
    # the propagation on a mixed state
    want = ka.propagation_rule(state, lists)
    if K > 1:
        assert want[5] == CV and want[9] == CV and want != state                   # (the test's own lists do what they are for)
    ka.propagate(g)
    assert g.read_keyframe_activations() == want
    # a partial window, whatever the table held
    ka.set_window(g, window)
    want = ka.propagation_rule(ka.window_rule(window), lists)
    if K > 1:
        assert want[5] == CV and want[9] == CV and set(want) == {A, CV, I}
    ka.apply_window(g)
    assert g.read_keyframe_activations() == want
    # a window that holds every keyframe
    ka.set_window(g, [1] * K)
    ka.apply_window(g)
    assert g.read_keyframe_activations() == [A] * K
    # ... and back: nothing of the full window sticks
    ka.set_window(g, window)
    ka.apply_window(g)
    assert g.read_keyframe_activations() == want


# ---- b: the pose phase's activation update on a table of more than 1024 keyframes -------------------------------------------------
def test_pose_phase_activation_update_at_1025_keyframes_on_an_empty_cloud():
    """No surfels: H = b = 0, no pose moves.  Every keyframe that is not kInactive takes its one Gauss-Newton step, does not move and
    becomes kInactive; the kInactive ones are skipped; all K count as converged (pose_init_from_keyframes_kernel<false>: thread 0
    counts the inactive keyframes of the whole table).  Every pose keeps its bits."""
    K = 1025
    rng = np.random.Generator(np.random.PCG64(7))
    scene = common.small_scene(num_keyframes=1, width=64, height=48, seed=3)
    g = common.build_gpu(scene, 1024, create_from=[])
    state = [int(v) for v in rng.integers(0, 3, K)]
    state[0], state[1023], state[1024] = I, A, I
    # one pose per keyframe, each a fixed point of the step T <- T * exp(-0): a quaternion whose squared norm is exactly 1 in binary32
    # (se3_mul renormalises any other, on the device as in the oracle) and a translation of its own
    axes = np.eye(4, dtype=np.float32)
    poses = [np.concatenate([axes[k % 4], rng.uniform(0.5, 2.0, 3).astype(np.float32) * (1 if k % 3 else -1)]) for k in range(K)]
    first = g.keyframes[0]
    g.keyframes = [dict(first, activation=state[k], pose=poses[k]) for k in range(K)]
    g.bind_keyframes()
    assert g.surfels_size == 0
    r = ka.pose_phase(g)
    skipped = [s == I for s in state]
    assert [n == 0 for n in r["iterations"]] == skipped
    assert all(n <= 1 for n in r["iterations"])
    assert r["moved"] == [0] * K
    assert r["num_converged"] == K
    assert np.array_equal(ka.bits(r["poses"]), ka.bits(np.asarray(poses)))
    table = (C.c_float * (7 * K))()
    capi.check(g.lib.bahip_get_keyframe_poses(g.ctx.handle, table, K))
    assert np.array_equal(ka.bits(np.array(list(table), np.float32).reshape(K, 7)), ka.bits(np.asarray(poses)))
    assert g.read_keyframe_activations() == [I] * K


# ---- c: the stage-driven loop against the oracle, iteration by iteration ----------------------------------------------------------------
_oracle_cache = {}


def _oracle(name):
    """Per scenario, computed once and left unchanged: the oracle's surfels at the start, its iteration-by-iteration trace (S1, S2)
    and the result of one call."""
    if name not in _oracle_cache:
        sc = ka.scenario(name)
        orc = ka.build_oracle(sc)
        start = orc.surfel_data[:, :orc.surfels_size].copy()
        trace = ka.oracle_trace(sc) if name in ("S1", "S2") else None
        stats = orc.bundle_adjustment(min_iterations=1, max_iterations=sc.max_iterations, window_start=sc.window[0], window_end=sc.window[1],
                                      increase_ba_iteration_count=False)
        _oracle_cache[name] = dict(sc=sc, start=start, trace=trace, iterations_done=int(stats.iterations_done), converged=int(stats.converged),
                                   gn_steps=int(stats.pose_gn_steps_total), activation=ka.oracle_state(orc), poses=ka.oracle_poses(orc),
                                   surfels=orc.surfel_data[:8, :orc.surfels_size].copy())
    return _oracle_cache[name]


def _gpu(ref):
    return ka.build_gpu(ref["sc"], ref["start"])


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_stage_driven_loop_against_the_oracle_iteration_by_iteration(name):
    ref = _oracle(name)
    sc, trace = ref["sc"], ref["trace"]
    K = sc.num_keyframes
    g = _gpu(ref)
    for n, it in enumerate(trace):
        if n > 0:
            ka.propagate(g)                                       # closes iteration n - 1 (B/direct_ba_alternating.cc:703-709)
        assert g.read_keyframe_activations() == it["at_pose"], n  # the states the oracle's pose phase met
        g.optimize_geometry_iteration(True, True)
        r = ka.pose_phase(g)
        after_pose, num_converged = ka.pose_phase_rule(it["at_pose"], it["moved"])
        assert r["moved"] == it["moved"], (n, r["moved"], it["moved"])
        assert r["num_converged"] == num_converged, n
        assert r["iterations"] == it["steps"], (n, r["iterations"], it["steps"])
        assert g.read_keyframe_activations() == after_pose, n
        assert np.array_equal(ka.bits(r["poses"]), ka.bits(it["poses"])), n
        assert np.array_equal(ka.bits(g.download_surfels()[:8]), ka.bits(it["surfels"])), n
        assert (num_converged == K) == bool(it["converged"])
    assert trace[-1]["converged"] and g.read_keyframe_activations() == trace[-1]["after"] == ref["activation"]


# ---- d: the device-driven loop against one oracle call -----------------------------------------------------------------------------------
@pytest.fixture
def loop_switches():
    lib = capi.load()

    def set_switches(fused_begin, rounds_ahead):
        capi.check(lib.bahip_debug_set_device_loop(1))
        capi.check(lib.bahip_debug_set_fused_iteration_begin(int(fused_begin)))
        capi.check(lib.bahip_debug_set_pose_rounds_ahead(int(rounds_ahead)))
    yield set_switches
    capi.check(lib.bahip_debug_set_device_loop(1))
    capi.check(lib.bahip_debug_set_fused_iteration_begin(0))
    capi.check(lib.bahip_debug_set_pose_rounds_ahead(0))


@pytest.mark.parametrize("rounds_ahead", [0, 1], ids=["rounds as hinted", "one round queued: phases outrun the queue"])
@pytest.mark.parametrize("fused_begin", [0, 1], ids=["iteration_begin launch", "phase end opens the next iteration"])
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_device_driven_loop_against_the_oracle(loop_switches, name, fused_begin, rounds_ahead):
    ref = _oracle(name)
    sc = ref["sc"]
    g = _gpu(ref)
    loop_switches(fused_begin, rounds_ahead)
    fixed = ka.is_fixed_window(sc.window)
    r = ka.alternating_iterations(g, fixed_window=fixed, max_iterations=sc.max_iterations)
    assert r["handled"] == 1
    assert (r["iterations_done"], r["converged"]) == (ref["iterations_done"], ref["converged"])
    assert r["pose_steps"] == ref["gn_steps"]
    assert r["not_converged"] == 0
    if rounds_ahead == 1:
        assert r["pose_rounds"] > r["iterations_done"]            # phases of more than one round: the hand-over to the host was exercised
    assert g.read_keyframe_activations() == r["activation"]
    # The oracle runs determine_covisible_active after an iteration that did not end the loop; the device table, by contract, is
    # left without it (include/badslam_hip.h: "the caller applies DetermineCovisibleActiveKeyframes itself when *converged_out == 0").
    # S3 ends that way: the model's propagation is applied to activation_out before the comparison.  S1 and S2 end by convergence.
    assert bool(ref["converged"]) == (not fixed)
    got = r["activation"] if r["converged"] else ka.propagation_rule(r["activation"], sc.covis)
    assert got == ref["activation"], (got, ref["activation"])
    assert np.array_equal(ka.bits(r["poses"]), ka.bits(ref["poses"]))
    assert np.array_equal(ka.bits(g.download_surfels()[:8]), ka.bits(ref["surfels"]))


# ---- e: DirectBA::BundleAdjustment against the oracle, under the host's co-visibility lists ----------------------------------------------
def _directba(sc):
    from badslam_amd.directba import DirectBA
    scene = sc.scene
    ba = DirectBA(ka.MAX_SURFELS, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, scene.width, scene.height, scene.camera, scene.camera)
    for k in range(sc.num_keyframes):
        ba.AddKeyframe(scene.depth[k], scene.rgb[k], scene.poses_gt[k])
    lists = [ba.keyframe_covisibility(k) for k in range(sc.num_keyframes)]
    # the lists of the host's frustum test: not complete -- and the ones the CPU test checked the scenarios' conditions under
    K = sc.num_keyframes
    assert any(k not in lists[j] for j in range(K) for k in range(K) if k != j)
    assert lists == ka.HOST_COVIS[ka.HOST_TRANSLATION_RANGE[sc.name]], lists
    return ba, lists


def _compare(ba, orc, done, conv, stats, call=0):
    K = len(orc.keyframes)
    assert (done, int(conv)) == (stats.iterations_done, stats.converged), (call, done, conv, stats.iterations_done, stats.converged)
    assert [ba.keyframe_activation(k) for k in range(K)] == ka.oracle_state(orc), call
    assert [ba.keyframe_ba_iterations(k) for k in range(K)] == [(kf.last_active_in_ba_iteration, kf.last_covis_in_ba_iteration)
                                                                for kf in orc.keyframes], call
    assert ba.surfel_count() == orc.surfels_size, (call, ba.surfel_count(), orc.surfels_size)
    assert np.array_equal(ka.bits([ba.keyframe_pose(k) for k in range(K)]), ka.bits(ka.oracle_poses(orc))), call
    assert np.array_equal(ka.bits(ba.download_surfels(8)), ka.bits(orc.surfel_data[:8, :orc.surfels_size])), call


@pytest.mark.parametrize("name", ["S1", "S3"], ids=["window (-1, -1)", "window (2, 3)"])
def test_directba_fixed_surfels_against_the_oracle(name):
    sc = ka.host_scenario(name)
    ba, lists = _directba(sc)
    orc = common.build_oracle(sc.scene, ka.MAX_SURFELS)
    data, _ = common.oracle_surfels(orc)
    ba.upload_surfels(data[:8])
    for k, T in enumerate(sc.poses):
        orc.set_pose(k, T)
        ba.set_keyframe_pose(k, T)
    orc.covis = lists
    orc.spatial_sort_cell, orc.unsorted_surfels = 0.02, ba.unsorted_surfels()      # the end tasks reorder on both sides
    before = ka.oracle_poses(orc)
    args = dict(do_surfel_updates=False, optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=sc.max_iterations,
                increase_ba_iteration_count=True)
    done, conv = ba.BundleAdjustment(active_keyframe_window_start=sc.window[0], active_keyframe_window_end=sc.window[1], **args)
    stats = orc.bundle_adjustment(window_start=sc.window[0], window_end=sc.window[1], **args)
    _compare(ba, orc, done, conv, stats)
    assert not np.array_equal(ka.bits(before), ka.bits(ka.oracle_poses(orc)))       # the call did move poses
    if name == "S1":
        assert conv and 2 <= done < sc.max_iterations
    else:
        # keyframes outside the window and unseen by it stayed kInactive: never solved, every pose bit kept (by the comparison above
        # the oracle's); all three states at the end
        final = [ba.keyframe_activation(k) for k in range(sc.num_keyframes)]
        after = ka.oracle_poses(orc)
        assert not conv and set(final) == {A, CV, I}, final
        assert all(np.array_equal(ka.bits(before[k]), ka.bits(after[k])) for k in range(sc.num_keyframes) if final[k] == I)


def test_directba_surfel_updates_under_deactivation_against_the_oracle():
    sc = ka.host_scenario("S4")
    ba, lists = _directba(sc)
    orc = common.build_oracle(sc.scene, ka.MAX_SURFELS, create_from=[])
    for k, T in enumerate(sc.poses):
        orc.set_pose(k, T)
        ba.set_keyframe_pose(k, T)
    orc.covis = lists
    orc.spatial_sort_cell, orc.unsorted_surfels = 0.02, ba.unsorted_surfels()
    args = dict(do_surfel_updates=True, optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=sc.max_iterations,
                increase_ba_iteration_count=True)
    for call in range(2):
        done, conv = ba.BundleAdjustment(active_keyframe_window_start=-1, active_keyframe_window_end=-1, **args)
        stats = orc.bundle_adjustment(window_start=-1, window_end=-1, **args)
        _compare(ba, orc, done, conv, stats, call)
    marks = [ba.keyframe_ba_iterations(k) for k in range(sc.num_keyframes)]
    assert len(set(marks)) > 1 and orc.surfels_size > 5000, marks
