"""Build-time guard for the windowed PCG scheme (no GPU needed: hipcc cross-compiles gfx950).  The windowed sweeps live in a unit of
their own (kernels_pcg_window.hip) and share device helpers with kernels_pcg.hip through pcg_device.h; moving those helpers must not
change the whole-map unit: every function of kernels_pcg.hip, in both arithmetic flavours, compiles with the Makefile's flags to the
parent's gfx950 code -- the whole function up to its end label, every exit included (label numbers and comments aside).  The
new unit's sweeps keep the PCG sweeps' budget -- 4 wavefronts per SIMD (<= 128 VGPRs), at most 64 bytes of scratch -- each in its
flavour's namespace."""
import hashlib
import re

import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")


def _functions(listing):
    """mangled name -> the function's whole code, from its label to its .Lfunc_end label (every exit included)"""
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", listing, re.S | re.M)}


def _digest(body):
    body = re.sub(r";.*", "", body)                          # comments
    body = re.sub(r"\.L(BB|tmp)\d+_", r".L\1_", body)        # label numbers follow the function's place in the unit
    return hashlib.sha256("\n".join(line.rstrip() for line in body.splitlines() if line.strip()).encode()).hexdigest()[:24]


# sha256 (first 24 hex digits) of each function's normalised gfx950 code before the windowed scheme, by mangled name
PARENT = {
    "exact": {
        "_ZN5bahip11exact_valueERA9_Kx":
            "3c84f7df13329ea533423a8d",
        "_ZN5bahip16pcg_init2_kernelENS_9PcgLayoutENS_8PcgExactEfPKfS3_PfS4_S4_":
            "5181170dcbb2242773f0c44b",
        "_ZN5bahip16pcg_step2_kernelENS_9PcgLayoutENS_8PcgExactEPfPKfS2_S2_S4_S4_S4_PKNS_10PcgControlE":
            "dda1544f2ff2a2b956cb5054",
        "_ZN5bahip16pcg_step3_kernelENS_9PcgLayoutENS_8PcgExactEPKfPfS3_S3_PKNS_10PcgControlE":
            "2c527dae77c2ea8931ee0c1c",
        "_ZN5bahip18pcg_control_kernelENS_8PcgExactEPNS_10PcgControlEPf":
            "67c2784fcdb5884d05cf2dbd",
        "_ZN5bahip18pcg_resolve_kernelILb0EEEvNS_9PcgLayoutENS_8PcgExactEPfS3_S3_dPKNS_10PcgControlE":
            "7cbaeae541e8db00973802f7",
        "_ZN5bahip18pcg_resolve_kernelILb1EEEvNS_9PcgLayoutENS_8PcgExactEPfS3_S3_dPKNS_10PcgControlE":
            "bd5758cff9640b86333427e4",
        "_ZN5bahip20pcg_eps_terms_kernelENS_9PcgLayoutENS_8PcgExactEPKf":
            "ac9faf65bb7c0c5bd637eb87",
        "_ZN5bahip22exact_sum_debug_kernelENS_8PcgExactEPKfmi":
            "23e84b61ba24da1e24d7f2a0",
        "_ZN5bahip23pcg_control_init_kernelENS_8PcgExactEPNS_10PcgControlEPf":
            "22ccb32f30702aef964124a0",
        "_ZN5bahip24pcg_class_combine_kernelENS_9PcgLayoutENS_10PcgClassesEjPfS2_PKNS_10PcgControlE":
            "81f7b8b98bc0a7a79400be0b",
        "_ZN5bahip25pcg_update_surfels_kernelENS_9PcgLayoutENS_11SurfelsViewEPKf":
            "72047279becc38ef8753440b",
        "_ZN5bahip26pcg_update_cfactors_kernelENS_10IntrinsicsEjPKfPfj":
            "596d0c411b6c4459c07f210e",
        "_ZN5bahip30exact_sum_debug_resolve_kernelENS_8PcgExactEPd":
            "505daa3a8e3f73c0f47f81c1",
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "6ec0526de443bd6825d0f830",
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "7d6eee6d876489b83a410d77",
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "4f8aed25e5eb9cb9cfa4f735",
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "f263292b152a48eafbf180ea",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "643d00ee2ef0dbcfed0379d4",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "63c25efd9eb7a380e75dbcb7",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "a5e82ea1bd695f05172ab9ab",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "0d4b66b7259ba672e24361b1",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "0c7942f450024255e8e4cf40",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "0ea5f623b85a7d21bb828c71",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "48943eb0c127e1f07f95e488",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "08704f6b9bd5a0bbd3fb0d53",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "382f84346eb2eabecaafc267",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "e810c07ba89cd2a4ea850f31",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "6ef0eb1fd569539b3101f418",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "971812d7dece1f32b5419d2b",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "232fbda68079df5640768e66",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "0ef9105f9b1afc5072d26d4e",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "6ff51c056a39b9382277fdb8",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "7826763bb0c02350ff561901",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "e054af80b92357b0a094c991",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "fcd020c613e25585cfcdbeb0",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "ce9c10d7c01b71b05cb34eec",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "e537e81ee3b28892a0d36027",
    },
    "fast": {
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "d8ad6adb0667dfe8d30adf11",
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "d7eeb4ffa18121ad85eabedc",
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "c8e29a2783ff87087d5cc88d",
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "caf92028a308cd3c4ee8a502",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "6766e8824a5bfaf6c4945c4b",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "c5c1fab61c51373c90fbd4c8",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "f4286f548dbf91c55fb169e5",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "61e5624fb75cc0e4f2afefba",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "cc28588e885b08018e691748",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "b7dc8791e1a84459f9e36ae3",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "eed9ce9e142e64f348458988",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "b67ee2d66e2a6d0b387cf244",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "0bc48ed9c9d37b4679a0d7c9",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "c186eeb785a17e78426a6710",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "b195244f349f1513c1e201e8",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "888e3900c0f8d4194bab9b3b",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "83546f06097590f2e4c43c2e",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "9df2266928045bd89ed0e0b7",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "b05ecd1356d87df6959a11ec",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "f707723aaabdf2f64dbe97fd",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "eafd5a6e7b8d436847e743ef",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "11fbfc70400568b094d3ed28",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "f2e719998f2f37c517f31300",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "177e3183a16d945bfa5122d0",
    },
}

def _listings(tmp_path_factory, unit):
    d = tmp_path_factory.mktemp("isa_" + unit)
    return {flavour: _compile(d, unit, _fast_flags(unit) if flavour == "fast" else [], "" if flavour == "exact" else "_fast")
            for flavour in ("exact", "fast")}


@pytest.fixture(scope="module")
def pcg(tmp_path_factory):
    return {flavour: _functions(listing) for flavour, listing in _listings(tmp_path_factory, "kernels_pcg").items()}


@pytest.fixture(scope="module")
def window(tmp_path_factory):
    return {flavour: _kernels(listing) for flavour, listing in _listings(tmp_path_factory, "kernels_pcg_window").items()}


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_the_whole_map_pcg_unit_is_the_code_of_before(pcg, flavour):
    functions = pcg[flavour]
    assert set(functions) == set(PARENT[flavour]), sorted(set(functions) ^ set(PARENT[flavour]))
    changed = sorted(name for name, digest in PARENT[flavour].items() if _digest(functions[name]) != digest)
    assert not changed, changed


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_the_windowed_sweeps_keep_the_pcg_sweep_budget(window, flavour):
    kernels = window[flavour]
    namespace = "5exact" if flavour == "exact" else "4fast"
    for sweep in ("pcg_window_init_kernel", "pcg_window_step1_kernel"):
        mine = {name: v for name, v in kernels.items() if f"{len(sweep)}{sweep}I" in name}
        assert len(mine) == 4, (sweep, sorted(mine))   # <kDepthIntr, kColorIntr>
        for name, (_body, vgprs, scratch, occupancy) in mine.items():
            assert namespace in name, name
            assert vgprs <= 128 and occupancy >= 4 and scratch <= 64, (name, vgprs, scratch, occupancy)
    # the tile list and the masked surfel update: plain code, compiled once (exact unit), no scratch
    helpers = [name for name in kernels if "pcg_window_tiles_kernel" in name or "pcg_window_update_surfels_kernel" in name]
    assert len(helpers) == (2 if flavour == "exact" else 0), helpers
    for name in helpers:
        assert kernels[name][2] == 0, name
