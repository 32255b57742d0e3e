"""Build-time guard for the PCG sweeps (no GPU needed: hipcc cross-compiles gfx950).  The whole-map sweeps (kernels_pcg.hip) and the
windowed ones (kernels_pcg_window.hip, a unit of its own) are built from one definition of each pair body, in pcg_device.h.  What is
held, with the Makefile's flags and in both arithmetic flavours:
  - every function of kernels_pcg.hip that is no sweep (the per-unknown, control, resolve and debug kernels, exact_value) compiles to
    the gfx950 code of before the windowed scheme -- the whole function up to its end label, every exit included (label numbers and
    comments aside);
  - every sweep kernel compiles to its recorded code (PARENT here, WINDOW_PARENT in tests/test_cpu_pcg_trial_kernel_resources.py:
    the digests of this tree where sharing the pair bodies changed register numbering or instruction order);
  - every sweep kernel has the instruction mix and the resources of the commit before the pair bodies were shared (SWEEP_PARENT): the
    same number of instructions per mnemonic, the same NumVgprs, ScratchSize and Occupancy;
  - the two plain kernels of the windowed unit (tile list, masked surfel update) compile to the code they had before (WINDOW_PLAIN);
  - the windowed sweeps keep the PCG sweeps' budget -- 4 wavefronts per SIMD (<= 128 VGPRs), at most 64 bytes of scratch -- each in
    its flavour's namespace."""
import re

import pytest

from tests.isa_pins import _digest, _functions, _histogram   # noqa: F401  (re-exported: other resource tests import them from here)
from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")


# sha256 (first 24 hex digits) of each function's normalised gfx950 code by mangled name: before the windowed scheme for the functions
# that are no sweep, of the tree that shared the pair bodies for the sweep kernels whose register numbering or instruction order that
# moved (10 of the 64 sweep kernels of both tables kept the digest they had; the others hold SWEEP_PARENT's instruction mix)
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
            "0cf9b2aaedbd85ddf280e649",
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "7d6eee6d876489b83a410d77",
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "b2db1411ee6f9c0212424578",
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "83e741cbe2b11cab6e7af530",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "21fea1ad91107b7df1b6b1fc",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "76ade6e9b9169995fd33e658",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "87be7ec57df02d5332bae6a8",
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "e13f00f6086041a2b783a678",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "0c7942f450024255e8e4cf40",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "0ea5f623b85a7d21bb828c71",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "48943eb0c127e1f07f95e488",
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "08704f6b9bd5a0bbd3fb0d53",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "7f597db9a6d01d26b240b94c",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "d8ed085df221b426332935d2",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "31ec99bf05c3ac6da4cfa8b4",
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "9f2d59af83e1006201b68cb8",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "2cfa7b2f69d14639d2af9af7",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "0ef9105f9b1afc5072d26d4e",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "c03b7a618ed850c17dcf5dde",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "7826763bb0c02350ff561901",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "4db471f97f4a490996c1c337",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "a9b8d661a14ce64803bbd503",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "f7c112a20d478bf0f955243d",
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "5de6666d209fd04a812d497a",
    },
    "fast": {
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "6577745445f8734f0424e27e",
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "d7eeb4ffa18121ad85eabedc",
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "76cdc95bc08b1ba98fbe8f2d",
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "7ec062245042b5bc35b78ce0",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "2e27effcd7a31cfce38e42b1",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "5d4ea46d18054523047c59aa",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            "170eeb64e56648ff6442b1d5",
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            "9e992d5f1f7db6229cdc5e22",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "63db06c4f1bb32019ae889e3",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "ff8f8cf85826936054403660",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "9c03879c99ba62334bc01e1f",
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "870ee5af7dff86b8ae14310c",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "4fee7051be55f7206af2a8ae",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "221fab9f9bd1a36ed571b526",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "d020f06d15da72753dc7bef7",
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            "fe0242b0eade9847aaf77812",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "041ffe076bce6c126bc4a040",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "c0118f165c7bc9ffe8c1f592",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "6c3aeca3ddd0d5f5417a2196",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "578168d418669bdf0d2cc16b",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "c4c5b9de33f2e1cfa6703c1e",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "b96633fb117dc0896e9499ec",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "18d43293b83db6642faaff19",
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            "7dc29a196b5a08d52ff64fd6",
    },
}

# The sweep kernels (24 whole-map + 8 windowed per flavour) at commit 7a6ae13, the parent of the commit that shared the pair bodies: per
# mangled name (digest of the sorted (mnemonic, count) list of the function's instructions, their number, NumVgprs, ScratchSize,
# Occupancy).  Regenerate: `git worktree add --detach <dir> 7a6ae13 && python scripts/pcg_sweep_mix.py <dir>` prints this table.
SWEEP_PARENT = {
    "exact": {
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("4b1292ac09702c01", 2180, 119, 0, 4),
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("21b4e5d3b7767f45", 2205, 121, 0, 4),
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("1927857da5b8c510", 2868, 124, 0, 4),
        "_ZN5bahip5exact15pcg_init_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("3e70f0e7aadd3c08", 2872, 126, 0, 4),
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("a39c3bd2fe3e6724", 3457, 128, 12, 4),
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("9efe9382967586d7", 3498, 128, 16, 4),
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("e292af0820c45bd1", 3481, 128, 20, 4),
        "_ZN5bahip5exact15pcg_init_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("ac14c731a1fddc02", 3618, 128, 24, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("dbe5838e78068667", 2344, 115, 0, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("90a5957737ac2eb0", 2355, 116, 0, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("fdaa2a4379a6d57d", 2647, 119, 0, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("6e70617bdc546db3", 2653, 120, 0, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("58d08cc9063908fb", 3068, 125, 0, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("3cfcd60537523cca", 3124, 127, 0, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("679d950f3bf07dcc", 3093, 127, 0, 4),
        "_ZN5bahip5exact16pcg_step1_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("84aafb7737cf3394", 3131, 128, 0, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("1d001d6eb8ff7505", 2773, 125, 0, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("338fc53ff0657d15", 2815, 126, 0, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("d66d72be7712a036", 3121, 128, 0, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("d4c05f9820ab204d", 3130, 128, 8, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("113f660f8bf26c6a", 3541, 128, 8, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("1d058edcaa9fd812", 3552, 128, 0, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("960e7f5a2e7ecf22", 3570, 128, 16, 4),
        "_ZN5bahip5exact20pcg_step1_lds_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("6b19de83648b15f6", 3635, 128, 0, 4),
        "_ZN5bahip5exact22pcg_window_init_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("290c339e413a0861", 2063, 121, 0, 4),
        "_ZN5bahip5exact22pcg_window_init_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("a62d8fdbbff03bcb", 2716, 125, 0, 4),
        "_ZN5bahip5exact22pcg_window_init_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("7bbb1909f62b6c1c", 3343, 128, 16, 4),
        "_ZN5bahip5exact22pcg_window_init_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("50171b19936b33e4", 3406, 128, 36, 4),
        "_ZN5bahip5exact23pcg_window_step1_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("0591f169b0b08e51", 2278, 115, 0, 4),
        "_ZN5bahip5exact23pcg_window_step1_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("7b5a2d56c9ec9530", 2565, 119, 0, 4),
        "_ZN5bahip5exact23pcg_window_step1_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("bb7243e0aaef30e5", 2960, 125, 0, 4),
        "_ZN5bahip5exact23pcg_window_step1_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("59636cbc9079349c", 3003, 127, 0, 4),
    },
    "fast": {
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("5e1f25ef590fc4ff", 1957, 119, 0, 4),
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("549ee21ed9fd8220", 1989, 121, 0, 4),
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("9a0b21ade4c37fde", 2635, 124, 0, 4),
        "_ZN5bahip4fast15pcg_init_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("60aff522f6ad10b2", 2652, 126, 0, 4),
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("182d1650710aad5c", 3174, 128, 16, 4),
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("9868863f12c2a337", 3226, 128, 20, 4),
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfS9_PjPKjDpT2_":
            ("43b89ac2ec8b3d2d", 3196, 128, 24, 4),
        "_ZN5bahip4fast15pcg_init_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPfSA_PjPKjDpT2_":
            ("ba57d21a50e69191", 3238, 128, 28, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("d4328393e49030ba", 2116, 115, 0, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("166bebe160667538", 2128, 116, 0, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("b46e99ddf7b2f7dd", 2411, 119, 0, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("aa97fb8285d26b09", 2418, 120, 0, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("d28216c175936553", 2764, 125, 0, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("5c13bc2ee99d2265", 2789, 127, 0, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("73899e0c72f41fe6", 2801, 127, 0, 4),
        "_ZN5bahip4fast16pcg_step1_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjDpT2_":
            ("3fc9d272a7b8ffca", 2836, 128, 0, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("e76a5ecde7a6256b", 2555, 124, 0, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("561e05cb01db5de6", 2584, 125, 0, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("c661fb906adf7018", 2843, 127, 0, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb0ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("f96d8c0d78a4bae6", 2877, 128, 0, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb0ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("25b10243ab7c7be4", 3197, 128, 28, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb0ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("f828260a4b465e5d", 3270, 128, 20, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb1ELb0EJEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("f7bb4acfb4f2df92", 3254, 128, 28, 4),
        "_ZN5bahip4fast20pcg_step1_lds_kernelILb1ELb1ELb1EJNS_10PcgClassesEEEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryEiNS_11SurfelsViewEPKfPfPKNS_10PcgControlEPKjjPjijDpT2_":
            ("eec70bf69c5f0249", 3329, 128, 24, 4),
        "_ZN5bahip4fast22pcg_window_init_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("8d353c988acab57e", 1839, 121, 0, 4),
        "_ZN5bahip4fast22pcg_window_init_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("4e463e07af8d8d0d", 2494, 125, 0, 4),
        "_ZN5bahip4fast22pcg_window_init_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("7bbf2aefefed5efb", 3081, 128, 20, 4),
        "_ZN5bahip4fast22pcg_window_init_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPfSA_":
            ("8e60222634918a66", 3117, 128, 28, 4),
        "_ZN5bahip4fast23pcg_window_step1_kernelILb0ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("faf7f4bee5b64221", 2047, 115, 0, 4),
        "_ZN5bahip4fast23pcg_window_step1_kernelILb0ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("00e8e25dd2c407ed", 2337, 119, 0, 4),
        "_ZN5bahip4fast23pcg_window_step1_kernelILb1ELb0EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("6e5920a299286ac5", 2678, 125, 0, 4),
        "_ZN5bahip4fast23pcg_window_step1_kernelILb1ELb1EEEvNS_9PcgLayoutENS_8PcgExactENS_10IntrinsicsEPKNS_7KfEntryENS_9PcgWindowENS_11SurfelsViewEPKfPfPKNS_10PcgControlE":
            ("0fc762ce99936c55", 2745, 127, 0, 4),
    },
}


# The two plain kernels of the windowed unit (tile list, masked surfel update: compiled once, in the exact unit), digests as PARENT's; they
# are the bytes of commit 7a6ae13 -- pcg_update_surfel (pcg_device.h) became the body of both update kernels without moving either
WINDOW_PLAIN = {
    "_ZN5bahip23pcg_window_tiles_kernelENS_11SurfelsViewEPjS1_":
        "9b6044f692fa129dab906436",
    "_ZN5bahip32pcg_window_update_surfels_kernelENS_9PcgLayoutENS_11SurfelsViewEPKf":
        "44738f8d95ca67a13eb935ce",
}


def _listings(tmp_path_factory, unit):
    d = tmp_path_factory.mktemp("isa_" + unit)
    return {flavour: _compile(d, unit, _fast_flags(unit) if flavour == "fast" else [], "" if flavour == "exact" else "_fast")
            for flavour in ("exact", "fast")}


@pytest.fixture(scope="module")
def pcg_listings(tmp_path_factory):
    return _listings(tmp_path_factory, "kernels_pcg")


@pytest.fixture(scope="module")
def window_listings(tmp_path_factory):
    return _listings(tmp_path_factory, "kernels_pcg_window")


@pytest.fixture(scope="module")
def pcg(pcg_listings):
    return {flavour: _functions(listing) for flavour, listing in pcg_listings.items()}


@pytest.fixture(scope="module")
def window(window_listings):
    return {flavour: _kernels(listing) for flavour, listing in window_listings.items()}


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


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_every_sweep_kernel_has_the_parents_instruction_mix_and_resources(pcg_listings, window_listings, flavour):
    """One definition of a pair body serves kernels that used to have a copy each; register numbering and instruction order may move
    with that, what a sweep costs may not: per kernel the instructions per mnemonic, the registers, the scratch and the occupancy of
    the parent commit.  No kernel is excepted."""
    functions, kernels = {}, {}
    for listing in (pcg_listings[flavour], window_listings[flavour]):
        functions.update(_functions(listing))
        kernels.update(_kernels(listing))
    parent = SWEEP_PARENT[flavour]
    assert len(parent) == 32 and set(parent) == {name for name in functions if re.search(r"\d+pcg_(window_)?(init|step1|step1_lds)_kernelI", name)}
    moved = {name: (_histogram(functions[name]) + kernels[name][1:], expected) for name, expected in parent.items()
             if _histogram(functions[name]) + kernels[name][1:] != expected}
    assert not moved, moved


def test_the_plain_kernels_of_the_windowed_unit_are_the_code_of_before(window_listings):
    functions = _functions(window_listings["exact"])
    changed = sorted(name for name, digest in WINDOW_PLAIN.items() if name not in functions or _digest(functions[name]) != digest)
    assert len(WINDOW_PLAIN) == 2 and not changed, changed
