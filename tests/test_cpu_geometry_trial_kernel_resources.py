"""Build-time guard for the kernels of the geometry phase's step control (kernels_geometry_trial.hip; no GPU needed: hipcc
cross-compiles gfx950).  The trial solve and the decision exist once, in the exact unit only (compiled with the fast flavour's flags the
unit is empty: both flavours of the sweeps launch the one build, and there is no contracted lambda * a + (a + 1e-6f)); none of the
unit's kernels uses scratch or an atomic of any kind; the solve has the plain step's division and square-root count."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

UNIT = "kernels_geometry_trial"
KERNELS = ("geometry_trial_snapshot_kernel", "geometry_trial_solve_kernel", "geometry_trial_decide_kernel", "geometry_trial_count_kernel",
           "geometry_trial_finish_kernel", "geometry_trial_restore_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_geometry_trial")
    # (the unit has no FASTFTZ_ line of its own: it is never built fast; the surfel unit's flags are what a fast build would pass)
    return {"exact": _kernels(_compile(d, UNIT, [], "")), "fast": _kernels(_compile(d, UNIT, _fast_flags("kernels_surfel"), "_fast"))}


def test_both_kernels_exist_once_in_the_exact_unit_only(kernels):
    for wanted in KERNELS:
        found = [name for name in kernels["exact"] if wanted in name]
        assert len(found) == 1, (wanted, sorted(kernels["exact"]))
        assert "5exact" not in found[0] and "4fast" not in found[0], found
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


def test_the_solve_is_not_contracted_and_divides_exactly(kernels):
    body = [v[0] for name, v in kernels["exact"].items() if "geometry_trial_solve_kernel" in name][0]
    # correctly rounded division and square root (the compiler's IEEE sequences), never the bare approximations' results
    assert "v_div_fixup_f32" in body and "v_div_fmas_f32" in body, "the solve's divisions are not the IEEE sequence"
    assert not re.search(r"\bv_pk_(fma|mul|add)_f32\b", body)
    # the damped diagonal is a product and then an add: v_fma appears inside the division / square-root sequences only, so there are
    # v_mul_f32 for the three products lambda * a and the six products of the Cholesky steps at least
    assert len(re.findall(r"\bv_mul_f32", body)) >= 9, len(re.findall(r"\bv_mul_f32", body))
    src = open(os.path.join(CSRC, UNIT + ".hip")).read()
    assert "#pragma clang fp contract(off)" in src


def test_the_makefile_builds_the_two_new_objects_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_geometry_trial.o", "capi_geometry_trial.o"):
        assert f"$(OUT)/{obj}" in text, obj
    assert "kernels_geometry_trial_fast.o" not in text
