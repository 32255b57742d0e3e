"""Build-time guard for the kernels of the intrinsics step's control (kernels_intrinsics_trial.hip; no GPU needed: hipcc cross-compiles
gfx950).  The damped Schur complement, the back-substitution between two planes and the plane copy exist once, in the exact unit only
(compiled with the fast flavour's flags the unit is empty: both flavours of the sweep launch the one build, and there is no contracted
lambda * D + D); none of them uses scratch, an atomic or flat access; the Schur complement divides by the IEEE sequence."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

UNIT = "kernels_intrinsics_trial"
KERNELS = ("intrinsics_schur_damped_kernel", "intrinsics_backsub_kernel", "intrinsics_plane_copy_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_intrinsics_trial")
    # (the unit has no FASTFTZ_ line of its own: it is never built fast; the intrinsics unit's flags are what a fast build would pass)
    return {"exact": _kernels(_compile(d, UNIT, [], "")), "fast": _kernels(_compile(d, UNIT, _fast_flags("kernels_intrinsics"), "_fast"))}


def test_each_kernel_exists_once_in_the_exact_unit_only(kernels):
    for wanted in KERNELS:
        found = [name for name in kernels["exact"] if wanted in name]
        assert len(found) == 1, (wanted, sorted(kernels["exact"]))
        assert "5exact" not in found[0] and "4fast" not in found[0], found
    # (intrinsics_finish_kernel is reused from kernels_intrinsics.hip: declared here, not compiled a second time)
    assert len(kernels["exact"]) == len(KERNELS), sorted(kernels["exact"])
    assert not kernels["fast"], sorted(kernels["fast"])


def test_no_scratch_and_full_occupancy(kernels):
    for name, (body, vgprs, scratch, occupancy) in kernels["exact"].items():
        assert scratch == 0, (name, scratch)
        assert vgprs <= 64 and occupancy >= 8, (name, vgprs, occupancy)      # bandwidth kernels: eight wavefronts per SIMD


def test_no_atomics_and_no_flat_access(kernels):
    for name, (body, *_rest) in kernels["exact"].items():
        assert "global_atomic" not in body and "buffer_atomic" not in body and "flat_atomic" not in body, name
        assert not re.search(r"\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg|pk_add)\w*", body), name     # LDS atomics
        assert "flat_load" not in body and "flat_store" not in body, name


def test_the_schur_complement_is_not_contracted_and_divides_exactly(kernels):
    body = [v[0] for name, v in kernels["exact"].items() if "intrinsics_schur_damped_kernel" in name][0]
    assert "v_div_fixup_f32" in body and "v_div_fmas_f32" in body, "1 / D' is not the IEEE sequence"
    assert not re.search(r"\bv_pk_(fma|mul|add)_f32\b", body)
    # lambda * D is a product of its own, then an add (v_fma appears inside the division sequence only); with it the distinct products
    # of the terms and the table: 5 B_r D'^-1 (shared by the table's D'^-1 B), 15 (B_r D'^-1) B_c, D'^-1 b2 and 5 B_c (D'^-1 b2)
    assert len(re.findall(r"\bv_mul_f32", body)) >= 1 + 26, len(re.findall(r"\bv_mul_f32", body))
    outside_division = re.sub(r"v_div_scale_f32.*?v_div_fixup_f32", "", body, flags=re.S)
    assert "v_fma_f32" not in outside_division and "v_fmac_f32" not in outside_division
    src = open(os.path.join(CSRC, UNIT + ".hip")).read()
    assert "#pragma clang fp contract(off)" in src


def test_the_back_substitution_is_not_contracted(kernels):
    body = [v[0] for name, v in kernels["exact"].items() if "intrinsics_backsub_kernel" in name][0]
    assert "v_fma_f32" not in body and "v_fmac_f32" not in body
    assert len(re.findall(r"\bv_mul_f32", body)) >= 5


def test_the_makefile_builds_the_two_new_objects_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_intrinsics_trial.o", "capi_intrinsics_trial.o"):
        assert text.count(f"$(OUT)/{obj}") == 1, obj
    assert "kernels_intrinsics_trial_fast.o" not in text and "capi_intrinsics_trial_fast.o" not in text
