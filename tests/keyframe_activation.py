"""The keyframe activation state machine of the alternating scheme (B/direct_ba_alternating.cc:353-371 and :556-577,
B/direct_ba.cc:549-564) for tests/test_cpu_keyframe_activation.py and tests/test_gpu_keyframe_activation.py: a plain Python model of
its three rules on integer lists, the scenarios S1-S4 in which the states diverge, the helpers that load a scenario into the CPU
oracle and into the HIP backend, and the oracle's trajectory iteration by iteration.  A plain module: no fixtures, no conftest.

States: 0 kActive, 1 kCovisibleActive, 2 kInactive.

  the window rule       inside the window -> kActive, otherwise kInactive
  the propagation rule  every kInactive keyframe listed by a kActive keyframe becomes kCovisibleActive; the sources are the keyframes
                        that are kActive before the step
  the pose-phase rule   a keyframe that was not kInactive becomes kActive if it moved, otherwise kInactive; a kInactive keyframe stays;
                        num_converged = the keyframes that were kInactive + the keyframes that did not move

The scenarios share one scene -- common.small_scene(num_keyframes=8, width=160, height=120, seed=41, translation_range=2.5,
rotation_range=0.8) --, surfels created from all keyframes at the ground-truth poses (none in S4), the chain co-visibility
covis[k] = [k - 1, k + 1] clipped to the range, and poses perturbed with synthetic.perturb_pose from PCG64(4) (one draw per keyframe
that the scenario names, in keyframe order; the others stay at the ground truth):

  S1  deactivation: all keyframes kActive, keyframes 0 and 5 perturbed, window (-1, -1)
  S2  newest keyframe only: keyframe 7 perturbed and kActive, keyframe 6 kCovisibleActive, the rest kInactive, window (-1, -1)
  S3  a partial fixed window (2, 3), all keyframes perturbed, 3 iterations
  S4  surfel updates under deactivation: no surfels at the start, keyframes 0 and 5 perturbed, window (-1, -1), do_surfel_updates,
      max_iterations = 10, increase_ba_iteration_count, called twice

What makes them worth running is asserted on the oracle alone in tests/test_cpu_keyframe_activation.py.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from badslam_amd import synthetic
from oracle import binding as ob
from tests import common

ACTIVE, COVISIBLE, INACTIVE = 0, 1, 2
MAX_SURFELS = 200000


# ---- the model --------------------------------------------------------------------------------------------------------------------
def window_rule(in_window):
    return [ACTIVE if inside else INACTIVE for inside in in_window]


def propagation_rule(state, covis):
    out = list(state)
    for k, s in enumerate(state):
        if s != ACTIVE:
            continue
        for other in covis[k]:
            if state[other] == INACTIVE:
                out[other] = COVISIBLE
    return out


def pose_phase_rule(state, moved):
    """(the states after the pose phase, num_converged)"""
    out, num_converged = [], 0
    for s, m in zip(state, moved):
        if s == INACTIVE or not m:
            out.append(INACTIVE)
            num_converged += 1
        else:
            out.append(ACTIVE)
    return out, num_converged


def window_flags(window, num_keyframes):
    return [1 if window[0] <= k <= window[1] else 0 for k in range(num_keyframes)]


def is_fixed_window(window):
    """B/direct_ba_alternating.cc:338-340: the active set is fixed when either end of the window is positive."""
    return window[0] > 0 or window[1] > 0


# ---- the scenarios ----------------------------------------------------------------------------------------------------------------
@dataclass
class Scenario:
    name: str
    scene: synthetic.Scene
    poses: list                        # global_T_frame of every keyframe at the start
    activation: list                   # state of every keyframe at the start
    covis: list                        # co-visibility lists
    window: tuple = (-1, -1)
    max_iterations: int = 40
    with_surfels: bool = True

    @property
    def num_keyframes(self):
        return len(self.poses)


def chain_covisibility(num_keyframes):
    return [[j for j in (k - 1, k + 1) if 0 <= j < num_keyframes] for k in range(num_keyframes)]


_scenes = {}


def the_scene(translation_range=2.5):
    if translation_range not in _scenes:
        _scenes[translation_range] = common.small_scene(num_keyframes=8, width=160, height=120, seed=41,
                                                        translation_range=translation_range, rotation_range=0.8)
    return _scenes[translation_range]


def scenario(name, translation_range=2.5):
    scene = the_scene(translation_range)
    K = len(scene.poses_gt)
    rng = np.random.Generator(np.random.PCG64(4))
    which = {"S1": (0, 5), "S2": (7,), "S3": tuple(range(K)), "S4": (0, 5)}[name]
    poses = [np.asarray(synthetic.perturb_pose(rng, scene.poses_gt[k]) if k in which else scene.poses_gt[k], np.float64) for k in range(K)]
    activation = [ACTIVE] * K
    if name == "S2":
        activation = [INACTIVE] * (K - 2) + [COVISIBLE, ACTIVE]
    return Scenario(name, scene, poses, activation, chain_covisibility(K), window=(2, 3) if name == "S3" else (-1, -1),
                    max_iterations={"S1": 40, "S2": 40, "S3": 3, "S4": 10}[name], with_surfels=name != "S4")


def build_oracle(sc, covis=None):
    """The scenario in the CPU oracle.  Without surfel updates the BA iteration counters are set so that no call runs the end-of-scheme
    tasks (callers pass increase_ba_iteration_count=False): the surfel set and its order stay."""
    orc = common.build_oracle(sc.scene, MAX_SURFELS, create_from=None if sc.with_surfels else [])
    for k, T in enumerate(sc.poses):
        orc.set_pose(k, T)
        orc.keyframes[k].activation = sc.activation[k]
    orc.covis = [list(l) for l in (sc.covis if covis is None else covis)]
    if sc.with_surfels:
        orc.ba_iteration_count = orc.last_ba_iteration_count = 1
    return orc


def oracle_state(orc):
    return [int(kf.activation) for kf in orc.keyframes]


def oracle_poses(orc):
    return np.asarray([orc.pose(k) for k in range(len(orc.keyframes))], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_moved(before, after):
    """The reference's moved test (B/direct_ba_alternating.cc:556-577) on two poses with the oracle's own functions:
    log(old^-1 * new) fails is_scale1_pose_converged."""
    L = ob.lib()
    a, b = ob.SE3.from_array(before), ob.SE3.from_array(after)
    lg = (C.c_float * 6)()
    diff = ob.se3_mul(ob.se3_inverse(a), b)
    L.orc_se3_log(C.byref(diff), lg)
    return 0 if L.orc_is_scale1_pose_converged(lg) else 1


def oracle_trace(sc):
    """The oracle's trajectory through a scenario without a fixed window (fixed surfels), one bundle_adjustment(max_iterations=1) call
    per iteration -- pose phase, stopping rule, and the propagation unless the call converged -- until a call reports convergence or
    sc.max_iterations calls are made.  Per iteration a dict:
      at_pose      the states the pose phase met (no window rule: the states at the top of the call)
      after        the states the call left
      poses_before / poses (K x 7 binary32), changed (pose bits changed), moved (the reference's test on those two poses)
      steps        Gauss-Newton steps per keyframe: orc_estimate_frame_pose from poses_before against the surfels the call left (the
                   ones its pose phase met); it must return the call's pose, and the steps must add up to the call's pose_gn_steps_total
      gn_steps, converged, surfels (rows 0-7 after the call)."""
    assert not is_fixed_window(sc.window)
    orc = build_oracle(sc)
    K = sc.num_keyframes
    trace = []
    for _ in range(sc.max_iterations):
        at_pose, poses_before = oracle_state(orc), oracle_poses(orc)
        stats = orc.bundle_adjustment(min_iterations=1, max_iterations=1, window_start=sc.window[0], window_end=sc.window[1],
                                      increase_ba_iteration_count=False)
        assert stats.iterations_done == 1
        poses = oracle_poses(orc)
        steps = [0] * K
        for k in range(K):
            if at_pose[k] == INACTIVE:
                continue
            est, steps[k], _ = orc.estimate_frame_pose(k, poses_before[k])
            assert np.array_equal(bits(est.to_array()), bits(poses[k])), k
        assert sum(steps) == stats.pose_gn_steps_total, (steps, stats.pose_gn_steps_total)
        trace.append(dict(at_pose=at_pose, after=oracle_state(orc), poses_before=poses_before, poses=poses,
                          changed=[int(not np.array_equal(bits(poses_before[k]), bits(poses[k]))) for k in range(K)],
                          moved=[oracle_moved(poses_before[k], poses[k]) for k in range(K)], steps=steps,
                          gn_steps=int(stats.pose_gn_steps_total), converged=int(stats.converged),
                          surfels=orc.surfel_data[:8, :orc.surfels_size].copy()))
        if stats.converged:
            break
    return trace


# ---- the HIP backend through the C boundary ------------------------------------------------------------------------------------------
def csr(covis):
    offsets, indices = [0], []
    for l in covis:
        indices += list(l)
        offsets.append(len(indices))
    return offsets, indices


def set_covisibility(g, covis):
    from badslam_amd import capi
    offsets, indices = csr(covis)
    capi.check(g.lib.bahip_set_covisibility(g.ctx.handle, (C.c_int * len(offsets))(*offsets), (C.c_int * max(1, len(indices)))(*indices),
                                            len(covis)))


def set_window(g, flags):
    from badslam_amd import capi
    capi.check(g.lib.bahip_set_activation_window(g.ctx.handle, (C.c_uint8 * max(1, len(flags)))(*flags), len(flags)))


def apply_window(g):
    from badslam_amd import capi
    capi.check(g.lib.bahip_apply_activation_window(g.ctx.handle))


def propagate(g):
    from badslam_amd import capi
    capi.check(g.lib.bahip_propagate_covisible_activation(g.ctx.handle))


def pose_phase(g, use_depth=True, use_desc=True):
    """bahip_estimate_keyframe_poses_and_update_activation: dict(poses (K x 7 binary32), iterations, converged, moved, rounds,
    num_converged)."""
    from badslam_amd import capi
    K = len(g.keyframes)
    poses = (C.c_float * (7 * K))()
    its, conv, moved = (C.c_int * K)(), (C.c_int * K)(), (C.c_int * K)()
    rounds, num_converged = C.c_int(), C.c_int()
    s = g.surfels_struct()
    capi.check(g.lib.bahip_estimate_keyframe_poses_and_update_activation(g.ctx.handle, int(use_depth), int(use_desc), C.byref(s), poses, its,
                                                                         conv, moved, C.byref(rounds), C.byref(num_converged)))
    return dict(poses=np.array(list(poses), np.float32).reshape(K, 7), iterations=[int(v) for v in its], converged=[int(v) for v in conv],
                moved=[int(v) for v in moved], rounds=rounds.value, num_converged=num_converged.value)


def alternating_iterations(g, fixed_window, max_iterations, min_iterations=1, activate_in_geometry=False):
    """bahip_alternating_iterations on the bound scene: dict(handled, iterations_done, converged, pose_rounds, pose_steps, not_converged,
    activation, poses (K x 7 binary32))."""
    from badslam_amd import capi
    K = len(g.keyframes)
    opt = capi.AlternatingOptions(1, 1, int(fixed_window), int(activate_in_geometry), g.surfels_size if activate_in_geometry else 0,
                                  int(min_iterations), int(max_iterations))
    poses, activation = (C.c_float * (7 * K))(), (C.c_int * K)()
    handled, done, conv, rounds, steps, not_conv = (C.c_int() for _ in range(6))
    s = g.surfels_struct()
    capi.check(g.lib.bahip_alternating_iterations(g.ctx.handle, C.byref(opt), C.byref(s), poses, activation, C.byref(handled), C.byref(done),
                                                  C.byref(conv), C.byref(rounds), C.byref(steps), C.byref(not_conv)))
    return dict(handled=handled.value, iterations_done=done.value, converged=conv.value, pose_rounds=rounds.value, pose_steps=steps.value,
                not_converged=not_conv.value, activation=[int(v) for v in activation], poses=np.array(list(poses), np.float32).reshape(K, 7))


def build_gpu(sc, surfels):
    """The scenario in the HIP backend with the given surfel rows (the oracle's at the start; every flag 1, as the oracle's loop sets
    them outside a full window), the keyframes bound with the scenario's poses and states, its co-visibility lists and its window."""
    g = common.build_gpu(sc.scene, MAX_SURFELS, create_from=[])
    g.upload_surfels(surfels, np.ones(surfels.shape[1], np.uint8))
    for k in range(sc.num_keyframes):
        g.keyframes[k]["pose"] = np.asarray(sc.poses[k], np.float32)
        g.keyframes[k]["activation"] = int(sc.activation[k])
    g.bind_keyframes()
    set_covisibility(g, sc.covis)
    set_window(g, window_flags(sc.window, sc.num_keyframes))
    return g


# ---- the scenes of the DirectBA-level comparison: co-visibility lists from the host's frustum test ----------------------------------
# vis::DirectBA::AddKeyframe builds its lists with CameraFrustum::Intersects.  On the scenarios' scene (translation_range 2.5) every
# pair of frustums intersects: complete lists, under which the propagation rule cannot go wrong visibly.  The comparison with
# DirectBA::BundleAdjustment therefore runs on the same scene with a wider translation_range, one per scenario:
#   S1, S4  5.5: 9 of the 28 pairs are missing (3.5: one pair, 4.5: two) and the deactivation run still converges in 8 iterations
#   S3      9.0: up to 7.0 keyframes 2 and 3 together list every other keyframe, so the window (2, 3) would wake them all; at 9.0
#           keyframes 1 and 4 (seen by nobody) stay kInactive throughout and keyframe 5 is kInactive at every pose phase and is only
#           woken by the propagation that closes the last iteration (S1 no longer converges within 40 iterations at that range)
# HOST_COVIS[range] is what tests/cpp/frustum_lists.cc gives for the scene's ground-truth poses (the poses AddKeyframe sees) with the
# oracle's min / max depths; the CPU test rebuilds the lists and checks the scenarios' conditions under them, the GPU test asserts that
# the host library made the same lists.
HOST_TRANSLATION_RANGE = {"S1": 5.5, "S3": 9.0, "S4": 5.5}
HOST_COVIS = {
    5.5: [[1, 2, 3, 5, 6, 7], [0, 2], [0, 1, 3, 5, 6, 7], [0, 2, 4, 5, 6, 7], [3, 6], [0, 2, 3, 6, 7], [0, 2, 3, 4, 5, 7], [0, 2, 3, 5, 6]],
    9.0: [[2, 3, 5, 6, 7], [], [0, 3, 6, 7], [0, 2, 6, 7], [], [0, 7], [0, 2, 3, 7], [0, 2, 3, 5, 6]],
}


def host_scenario(name):
    sc = scenario(name, HOST_TRANSLATION_RANGE[name])
    sc.covis = [list(l) for l in HOST_COVIS[HOST_TRANSLATION_RANGE[name]]]
    return sc


def frustum_lists(scene, orc, build_dir):
    """The lists of tests/cpp/frustum_lists.cc for the scene's ground-truth poses and the oracle's keyframe depth ranges."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(build_dir), "frustum_lists")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "badslam_amd", "host"), "-I",
                    os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "cpp", "frustum_lists.cc")], check=True, timeout=300)
    K = len(scene.poses_gt)
    lines = ["%d %d %d %s" % (K, scene.width, scene.height, " ".join(repr(float(v)) for v in np.asarray(scene.camera, np.float32)))]
    for k in range(K):
        kf = orc.keyframes[k]
        lines.append("%r %r %s" % (float(kf.min_depth), float(kf.max_depth),
                                   " ".join(repr(float(v)) for v in np.asarray(scene.poses_gt[k], np.float32))))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True).stdout
    return [[] if line.strip() == "-" else [int(v) for v in line.split()] for line in out.strip().splitlines()]
