"""Build-time guard for frame ingestion at a pyramid level (kernels_ingest.hip; no GPU needed: hipcc cross-compiles gfx950).  The unit
exists in the exact flavour only; no kernel of it uses scratch (no private array is indexed dynamically), a flat access, LDS or an
atomic; each keeps at least four wavefronts per SIMD; the division of the even-count rule is the correctly rounded one; the Makefile
links the unit and its boundary once."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels, _makefile_flags

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic\w*|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_ingest")
    fast = _fast_flags("kernels_cost")          # what any fast unit is built with: this one must compile to nothing under them
    return {"exact": _kernels(_compile(d, "kernels_ingest", [], "")), "fast": _kernels(_compile(d, "kernels_ingest", fast, "_fast"))}


def _named(kernels, part):
    return {name: v for name, v in kernels["exact"].items() if part in name}


def test_the_unit_compiles_in_the_exact_flavour_only(kernels):
    assert not kernels["fast"], sorted(kernels["fast"])
    names = sorted(kernels["exact"])
    assert len(_named(kernels, "median_densify_kernel")) == 1 and len(_named(kernels, "downscale_depth_median_kernel")) == 1, names
    assert len(_named(kernels, "downscale_rgb_half_kernel")) == 3, names          # levels 1, 2, 3
    assert len(names) == 5, names
    assert not any("5exact" in name or "4fast" in name for name in names), names
    assert "-ffp-contract=off" in _makefile_flags()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "kernels_ingest.hip")).read()


def test_no_kernel_uses_scratch_a_flat_access_lds_or_an_atomic(kernels):
    for name, (body, vgprs, scratch, occupancy) in kernels["exact"].items():
        assert scratch == 0, (name, scratch)
        assert "flat_" not in body and "scratch_" not in body, name
        assert not ATOMIC.search(body), name
        assert not re.search(r"\bds_(read|write|load|store)\w*", body), name
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        assert "global_load" in body and "global_store" in body, name


def test_the_average_is_divided_with_correct_rounding(kernels):
    """float(sum) / float(count): the IEEE quotient (v_div_scale / v_div_fmas / v_div_fixup), never a bare reciprocal times the sum."""
    for part in ("median_densify_kernel", "downscale_depth_median_kernel"):
        for name, (body, *_rest) in _named(kernels, part).items():
            assert "v_div_scale_f32" in body and "v_div_fixup_f32" in body, name
    for name, (body, *_rest) in _named(kernels, "downscale_rgb_half_kernel").items():
        assert "v_rcp_f32" not in body and "v_div_scale_f32" not in body, name          # integer shifts and adds only


def test_the_makefile_links_the_unit_and_its_boundary_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_ingest.o", "capi_ingest.o"):
        assert text.count(f"$(OUT)/{obj}") == 1, obj
    assert "kernels_ingest_fast.o" not in text and "FASTFTZ_kernels_ingest" not in text
