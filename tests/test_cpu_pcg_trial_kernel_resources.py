"""Build-time guard for the step control of the PCG scheme (no GPU needed: hipcc cross-compiles gfx950).  The new unit
(kernels_pcg_trial.hip) is compiled once, with the Makefile's flags: its snapshot / restore kernels take no scratch, make no scalar
memory writes and stay within 32 VGPRs -- the 8 wavefronts per SIMD the unit's comment claims for a copy --, and its damped
per-unknown kernels keep the shape of the undamped ones (no scratch, at least the 4 wavefronts per SIMD their LDS columns allow).  Step
control adds no pair sweep of its own: the whole-map sweeps (init, step 1, the LDS form) and the windowed ones compile to their recorded
gfx950 code, in both arithmetic flavours (digests as tests/test_cpu_pcg_window_kernel_resources.py takes them; since the pair bodies
are shared through pcg_device.h, 54 of the 64 are the digests of that tree, held to the earlier instruction mix by SWEEP_PARENT there)."""
import re

import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels
from tests.isa_pins import _digest, _functions
from tests.test_cpu_pcg_window_kernel_resources import PARENT

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

# sha256 (first 24 hex digits) of the windowed sweeps' normalised gfx950 code, by mangled name (of the tree that shared the pair bodies
# with the whole-map sweeps: tests/test_cpu_pcg_window_kernel_resources.py, PARENT and SWEEP_PARENT)
WINDOW_PARENT = {
    "exact": {
        "_ZN5bahip5exact22pcg_window_init_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "18cdf73667da3e179c123d13",
        "_ZN5bahip5exact22pcg_window_init_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "3d08002fc1de9ea05348e0ea",
        "_ZN5bahip5exact22pcg_window_init_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "c374fd1c2b76bf96851e7530",
        "_ZN5bahip5exact22pcg_window_init_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "81f4bcb0d6d9f5008819f3f8",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "1a679e98c62ed9bea13af0cf",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "23abbebc9caff3a26c44d798",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "00469b4d1ea61d181ffeb655",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "c6c5a900f10f53d1f7cd1b8e",
    },
    "fast": {
        "_ZN5bahip4fast22pcg_window_init_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "1782f9e0949d410810fb38bd",
        "_ZN5bahip4fast22pcg_window_init_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "f8d07d0461ee5b6f57148ce7",
        "_ZN5bahip4fast22pcg_window_init_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "d8d6d0c82d51f73a60d87f82",
        "_ZN5bahip4fast22pcg_window_init_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "49518194ef3ff11c17d9ab91",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "dffe91e5189110d3ad9ea8e6",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "54ed21dff5b8fd66e498e74e",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "cbd3dc75c6012b6ade55e29b",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "326877cd373a59d208e397ab",
    },
}
SCALAR_WRITES = re.compile(r"\b(" + "|".join(["s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic",
                                               "s_dcache_" + "wb", "s_dcache_" + "discard"]) + r")\w*")


@pytest.fixture(scope="module")
def trial(tmp_path_factory):
    return _kernels(_compile(tmp_path_factory.mktemp("isa_trial"), "kernels_pcg_trial", [], ""))


def test_the_snapshot_and_restore_kernels_keep_their_budget(trial):
    copies = {name: v for name, v in trial.items() if "pcg_trial_copy_kernel" in name}
    assert len(copies) == 2, sorted(trial)   # <kRestore>
    for name, (body, vgprs, scratch, occupancy) in copies.items():
        assert scratch == 0 and vgprs <= 32 and occupancy >= 8, (name, vgprs, scratch, occupancy)
        assert not SCALAR_WRITES.search(body), (name, SCALAR_WRITES.search(body).group(0))
        assert re.search(r"\bglobal_load_dword\b", body) and re.search(r"\bglobal_store_dword\b", body), name   # vector memory both ways


def test_the_damped_per_unknown_kernels_keep_the_shape_of_the_undamped_ones(trial):
    damped = {name: v for name, v in trial.items() if "pcg_damped_" in name}
    assert len(damped) == 4, sorted(trial)   # init2, step2, step3, the epsilon terms
    for name, (body, vgprs, scratch, occupancy) in damped.items():
        assert scratch == 0 and vgprs <= 64 and occupancy >= 4, (name, vgprs, scratch, occupancy)
        assert not SCALAR_WRITES.search(body), name


def test_the_unit_has_no_fast_flavour():
    import os
    makefile = open(os.path.join(os.path.dirname(__file__), "..", "badslam_amd", "csrc", "Makefile")).read()
    assert "kernels_pcg_trial.o" in makefile and "kernels_pcg_trial_fast.o" not in makefile


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_the_pair_sweeps_are_the_code_of_before(tmp_path_factory, flavour):
    d = tmp_path_factory.mktemp("isa_sweeps_" + flavour)
    extra = (lambda unit: _fast_flags(unit)) if flavour == "fast" else (lambda unit: [])
    suffix = "_fast" if flavour == "fast" else ""
    whole = _functions(_compile(d, "kernels_pcg", extra("kernels_pcg"), suffix))
    window = _functions(_compile(d, "kernels_pcg_window", extra("kernels_pcg_window"), suffix))
    sweeps = {name: digest for name, digest in PARENT[flavour].items() if re.search(r"pcg_(init|step1|step1_lds)_kernelI", name)}
    assert len(sweeps) == 24, sorted(sweeps)
    changed = sorted(name for name, digest in sweeps.items() if name not in whole or _digest(whole[name]) != digest)
    assert not changed, changed
    assert len(WINDOW_PARENT[flavour]) == 8
    changed = sorted(name for name, digest in WINDOW_PARENT[flavour].items() if name not in window or _digest(window[name]) != digest)
    assert not changed, changed
