"""Build-time guard for the step control of the pose phase (no GPU needed: hipcc cross-compiles gfx950).  The new unit
(kernels_pose_trial.hip) is compiled with the Makefile's flags, in both arithmetic flavours: the fused sweep takes no scratch -- the
plain persistent sweep (pose_accumulate_lds_kernel) takes none either -- and allows the wavefronts per SIMD that sweep allows for the
same residual types (4 / 7 / 4 for descriptors / depth / both).  What moved into pose_device.h and cost_device.h is inlined as before:
every function of kernels_pose.hip and kernels_cost.hip compiles to the gfx950 code of before (digests as
tests/test_cpu_pcg_window_kernel_resources.py takes them)."""
import re

import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels
from tests.isa_pins import _digest, _functions

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

# wavefronts per SIMD and scratch of pose_accumulate_lds_kernel<kUseDepth, kUseDesc, false> before this unit existed, both flavours alike
PLAIN_SWEEP = {"Lb0ELb1E": (4, 0), "Lb1ELb0E": (7, 0), "Lb1ELb1E": (4, 0)}

# sha256 (first 24 hex digits) of each function's normalised gfx950 code before the step control of the pose phase, by mangled name
PARENT = {'kernels_cost': {'exact': {'_ZN5bahip24cost_resolve_rows_kernelEPKxiPxP10bahip_cost': '17d2aafbca1fcf4d695776ff',
                            '_ZN5bahip25cost_resolve_total_kernelEPKxiP10bahip_cost': 'bdbada1a090920ada74a7344',
                            '_ZN5bahip5exact11cost_kernelILb0ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEiijjNS_11SurfelsViewEjjPKjPx': '7bd8473acffd6f7c8c6d05be',
                            '_ZN5bahip5exact11cost_kernelILb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEiijjNS_11SurfelsViewEjjPKjPx': 'b418e7b7a6872b0e9d3bd5be',
                            '_ZN5bahip5exact11cost_kernelILb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEiijjNS_11SurfelsViewEjjPKjPx': 'b6c82f779248d0d1a8cce265'},
                  'fast': {'_ZN5bahip4fast11cost_kernelILb0ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEiijjNS_11SurfelsViewEjjPKjPx': 'f3f096c365d08724d32853da',
                           '_ZN5bahip4fast11cost_kernelILb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEiijjNS_11SurfelsViewEjjPKjPx': 'ce98767515a1c419da4dec93',
                           '_ZN5bahip4fast11cost_kernelILb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEiijjNS_11SurfelsViewEjjPKjPx': '1007713443460b8714bf9e5f'}},
 'kernels_pose': {'exact': {'_ZN5bahip17pose_solve_kernelEPNS_8PoseWorkEiPxPNS_7KfEntryEiiiS1_iNS_15PoseLoopControlE': '598e515c26606f18e32e3f4d',
                            '_ZN5bahip17tile_order_kernelEPjjS0_': 'adb304b195513b2540846444',
                            '_ZN5bahip21jacobian_debug_kernelEiPKfPf': 'cd6ebc3cf29c6bc0c7c9e2d7',
                            '_ZN5bahip22iteration_begin_kernelEPNS_7KfEntryEiiPKhPKiS5_PNS_8PoseWorkEPxS7_S5_': '67a9bb345d2701a7545938d5',
                            '_ZN5bahip22pose_step_debug_kernelEPKfPf': 'a690e01e5dea65d3adf8e403',
                            '_ZN5bahip23exact_math_debug_kernelEiPKfPfm': '7e9ea40ff2c2c22114ac23e0',
                            '_ZN5bahip23pose_limbs_debug_kernelEPKfPxm': 'fe2a4b6105717ca38fc05284',
                            '_ZN5bahip23pose_solve_begin_kernelEPNS_8PoseWorkEiPxPNS_7KfEntryEiiiS1_iNS_15PoseLoopControlE': '7c61944d2a970ecf9095e8de',
                            '_ZN5bahip24wave_reduce_debug_kernelEPKfPf': '88acac10c0c6c371d3b8c35b',
                            '_ZN5bahip24window_activation_kernelEPNS_7KfEntryEiPKhPKi': 'a63b9c1a33425f5c05bd7819',
                            '_ZN5bahip26propagate_covisible_kernelEPNS_7KfEntryEiPKiS3_S3_': 'b11898f15615ff278046530b',
                            '_ZN5bahip27window_and_propagate_kernelEPNS_7KfEntryEiPKhPKiS5_S5_': 'f4771dc1ff29c1416ac1b34a',
                            '_ZN5bahip31pose_init_from_keyframes_kernelILb0EEEvPKNS_7KfEntryEiPNS_8PoseWorkEPxS5_jjPKi': '329a080b645f84e4a76bad13',
                            '_ZN5bahip31pose_init_from_keyframes_kernelILb1EEEvPKNS_7KfEntryEiPNS_8PoseWorkEPxS5_jjPKi': 'a07b1d0bb8bb0e47d0004ffd',
                            '_ZN5bahip5exact21evaluate_pairs_kernelENS_10IntrinsicsENS_7KfEntryENS_11SurfelsViewEPKjiPf': '394025832d19cff456151060',
                            '_ZN5bahip5exact22pose_accumulate_kernelILb0ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPiPjPKjPKiSI_': '2c59cdd1a4918acaa3783da2',
                            '_ZN5bahip5exact22pose_accumulate_kernelILb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPiPjPKjPKiSI_': '51436b3f9e743f9b05357195',
                            '_ZN5bahip5exact22pose_accumulate_kernelILb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPiPjPKjPKiSI_': 'f3e22af3d1c3b55d220025eb',
                            '_ZN5bahip5exact26pose_accumulate_lds_kernelILb0ELb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': '08e75a11dbf0a76930d9bfbb',
                            '_ZN5bahip5exact26pose_accumulate_lds_kernelILb0ELb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': 'c555d0348720cc68dc1cb175',
                            '_ZN5bahip5exact26pose_accumulate_lds_kernelILb1ELb0ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': 'e192b89e5eb0b899049e3cee',
                            '_ZN5bahip5exact26pose_accumulate_lds_kernelILb1ELb0ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': '90fccca0d6136d01f04761db',
                            '_ZN5bahip5exact26pose_accumulate_lds_kernelILb1ELb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': '02bac055e29490f34b7dd32a',
                            '_ZN5bahip5exact26pose_accumulate_lds_kernelILb1ELb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': '6f3849e339a56e9a3cdbeda3'},
                  'fast': {'_ZN5bahip4fast21evaluate_pairs_kernelENS_10IntrinsicsENS_7KfEntryENS_11SurfelsViewEPKjiPf': '82233875e3233fc40d26af95',
                           '_ZN5bahip4fast22pose_accumulate_kernelILb0ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPiPjPKjPKiSI_': '48bf548c4a0a144eb49505c7',
                           '_ZN5bahip4fast22pose_accumulate_kernelILb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPiPjPKjPKiSI_': '8dd18ff21a61b2bf675397c1',
                           '_ZN5bahip4fast22pose_accumulate_kernelILb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPiPjPKjPKiSI_': '273ece7c5e407373c3826d1b',
                           '_ZN5bahip4fast26pose_accumulate_lds_kernelILb0ELb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': 'a85dc9a86c921ba1fcd1b0a2',
                           '_ZN5bahip4fast26pose_accumulate_lds_kernelILb0ELb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': '63ff705ab634f62185ced312',
                           '_ZN5bahip4fast26pose_accumulate_lds_kernelILb1ELb0ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': 'cf650abf839701c835ac955e',
                           '_ZN5bahip4fast26pose_accumulate_lds_kernelILb1ELb0ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': 'c77d64125164b1274f7b306d',
                           '_ZN5bahip4fast26pose_accumulate_lds_kernelILb1ELb1ELb0EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': '1a49b9cdee16099363557c27',
                           '_ZN5bahip4fast26pose_accumulate_lds_kernelILb1ELb1ELb1EEEvNS_10IntrinsicsEPKNS_7KfEntryEPKNS_8PoseWorkEiNS_11SurfelsViewEPxPNS_10WaveBoundsEiiPijPjiiiSE_PKjPKijSI_': 'f9faa90be95d5bd236eff46a'}}}


def _unit(tmp_path_factory, unit, flavour):
    d = tmp_path_factory.mktemp("isa_%s_%s" % (unit, flavour))
    return _compile(d, unit, _fast_flags(unit) if flavour == "fast" else [], "_fast" if flavour == "fast" else "")


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_the_fused_sweep_keeps_the_plain_sweeps_budget(tmp_path_factory, flavour):
    kernels = _kernels(_unit(tmp_path_factory, "kernels_pose_trial", flavour))
    sweeps = {name: v for name, v in kernels.items() if "pose_trial_sweep_kernel" in name}
    assert len(sweeps) == 3, sorted(kernels)   # <kUseDepth, kUseDesc>
    for name, (body, vgprs, scratch, occupancy) in sweeps.items():
        assert ("5exact" if flavour == "exact" else "4fast") in name, name
        variant = re.search(r"pose_trial_sweep_kernelI(Lb\dELb\dE)", name).group(1)
        plain_occupancy, plain_scratch = PLAIN_SWEEP[variant]
        assert scratch <= plain_scratch, (name, scratch)
        assert vgprs <= 128 and occupancy >= plain_occupancy, (name, vgprs, occupancy)
        assert "flat_load" not in body and "flat_atomic" not in body, name            # gathers and LDS atomics in their address spaces
        assert not re.search(r"\bv_pk_(fma|mul|add)_f32\b", body), name               # SLP packing stays off
        assert "global_atomic_add_f32" not in body and "global_atomic_cmpswap" not in body, name   # integer sums only
    others = [name for name in kernels if name not in sweeps]
    assert len(others) == (2 if flavour == "exact" else 0), others   # the controlled solve and the debug hook exist once
    for name in others:
        assert kernels[name][2] == 0, (name, kernels[name][2])


@pytest.mark.parametrize("flavour", ["exact", "fast"])
@pytest.mark.parametrize("unit", ["kernels_pose", "kernels_cost"])
def test_the_plain_units_are_the_code_of_before(tmp_path_factory, unit, flavour):
    functions = _functions(_unit(tmp_path_factory, unit, flavour))
    parent = PARENT[unit][flavour]
    assert set(functions) == set(parent), sorted(set(functions) ^ set(parent))
    changed = sorted(name for name, digest in parent.items() if _digest(functions[name]) != digest)
    assert not changed, changed


def test_the_unit_has_both_flavours_and_the_cost_units_flags():
    import os
    makefile = open(os.path.join(os.path.dirname(__file__), "..", "badslam_amd", "csrc", "Makefile")).read()
    assert "kernels_pose_trial.o" in makefile and "kernels_pose_trial_fast.o" in makefile
    assert _fast_flags("kernels_pose_trial") == _fast_flags("kernels_cost")   # the cost bits of the fast flavour are the cost unit's
