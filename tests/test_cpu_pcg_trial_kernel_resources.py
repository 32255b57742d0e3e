"""Build-time guard for the step control of the PCG scheme (no GPU needed: hipcc cross-compiles gfx950).  The new unit
(kernels_pcg_trial.hip) is compiled once, with the Makefile's flags: its snapshot / restore kernels take no scratch, make no scalar
memory writes and stay within 32 VGPRs -- the 8 wavefronts per SIMD the unit's comment claims for a copy --, and its damped
per-unknown kernels keep the shape of the undamped ones (no scratch, at least the 4 wavefronts per SIMD their LDS columns allow).  The
pair sweeps were not touched: the whole-map sweeps (init, step 1, the LDS form) and the windowed ones compile to the gfx950 code of
before, in both arithmetic flavours (digests as tests/test_cpu_pcg_window_kernel_resources.py takes them)."""
import re

import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels
from tests.test_cpu_pcg_window_kernel_resources import PARENT, _digest, _functions

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

# sha256 (first 24 hex digits) of the windowed sweeps' normalised gfx950 code before step control, by mangled name
WINDOW_PARENT = {
    "exact": {
        "_ZN5bahip5exact22pcg_window_init_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "080048e992e87443ee7677a3",
        "_ZN5bahip5exact22pcg_window_init_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "d8f1d8ac0f026216f3eb9b0e",
        "_ZN5bahip5exact22pcg_window_init_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "bc232bdf07305a1e659d0a29",
        "_ZN5bahip5exact22pcg_window_init_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "4b718362489b47d10d4a2b25",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "1a679e98c62ed9bea13af0cf",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "23abbebc9caff3a26c44d798",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "294df01ec9333ceb6a68c029",
        "_ZN5bahip5exact23pcg_window_step1_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "d6fbe06d9ed4b7bdffbd8cd8",
    },
    "fast": {
        "_ZN5bahip4fast22pcg_window_init_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "06eee103807164514103ee85",
        "_ZN5bahip4fast22pcg_window_init_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "469a963fa8e5f72485452ef1",
        "_ZN5bahip4fast22pcg_window_init_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "ea2e2bd40920df832b0f563f",
        "_ZN5bahip4fast22pcg_window_init_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            "947eb98aba327df2e2b8aa70",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "6206c122b24e3e27850c6ecf",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "5d041051ef2abe6cca4e1e91",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "21d70ea7268ea99a18db4e47",
        "_ZN5bahip4fast23pcg_window_step1_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            "74aa12cf26d881180e97366c",
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
