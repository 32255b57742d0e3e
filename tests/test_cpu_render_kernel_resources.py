"""Build-time guard for the rendered views of the map (kernels_render.hip; no GPU needed: hipcc cross-compiles gfx950).  The unit exists
in the exact flavour only; no kernel of it uses scratch or a flat access; every splat kernel takes its minimum with the native 64-bit
unsigned atomic (global_atomic_umin_x2, no value returned) and never with a compare-and-swap loop; the clear and resolve kernels hold
no atomic at all; the Makefile links the unit and its boundary once."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels, _makefile_flags

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic\w*|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_render")
    fast = _fast_flags("kernels_cost")          # what any fast unit is built with: this one must compile to nothing under them
    return {"exact": _kernels(_compile(d, "kernels_render", [], "")), "fast": _kernels(_compile(d, "kernels_render", fast, "_fast"))}


def _named(kernels, part):
    return {name: v for name, v in kernels["exact"].items() if part in name}


def test_the_unit_compiles_in_the_exact_flavour_only(kernels):
    assert not kernels["fast"], sorted(kernels["fast"])
    names = sorted(kernels["exact"])
    assert len(_named(kernels, "render_clear_kernel")) == 1 and len(_named(kernels, "render_resolve_kernel")) == 1, names
    assert len(_named(kernels, "render_splat_kernel")) == 4, names           # <disc, census>
    assert len(names) == 6, names
    assert not any("5exact" in name or "4fast" in name for name in names), names
    assert "-ffp-contract=off" in _makefile_flags()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "kernels_render.hip")).read()


def test_no_kernel_uses_scratch_or_a_flat_access(kernels):
    for name, (body, vgprs, scratch, occupancy) in kernels["exact"].items():
        assert scratch == 0, (name, scratch)
        assert "flat_" not in body and "scratch_" not in body, name
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)


def test_the_splat_takes_its_minimum_with_the_native_64_bit_atomic(kernels):
    for name, (body, *_rest) in _named(kernels, "render_splat_kernel").items():
        assert "global_atomic_umin_x2" in body, name
        assert "cmpswap" not in body, name
        assert not re.search(r"global_atomic_umin_x2 [^\n]*\b(sc0|glc)\b", body), name          # no value returned
        census = re.search(r"render_splat_kernelILb[01]ELb1E", name) is not None
        others = {m.group(0) for m in ATOMIC.finditer(body)} - {"global_atomic_umin_x2"}
        assert others <= ({"global_atomic_add_x2"} if census else set()), (name, others)
        assert "global_load_dwordx2" not in body, name          # the key is never read back: the atomic is the only access to the plane


def test_the_census_variants_are_the_only_ones_that_count(kernels):
    counting = [name for name, (body, *_rest) in _named(kernels, "render_splat_kernel").items() if "global_atomic_add_x2" in body]
    assert len(counting) == 2 and all(re.search(r"render_splat_kernelILb[01]ELb1E", name) for name in counting), counting


def test_clear_and_resolve_hold_no_atomic(kernels):
    for part in ("render_clear_kernel", "render_resolve_kernel"):
        for name, (body, *_rest) in _named(kernels, part).items():
            assert not ATOMIC.search(body), name
            assert "global_store" in body, name


def test_the_makefile_links_the_unit_and_its_boundary_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_render.o", "capi_render.o"):
        assert f"$(OUT)/{obj}" in text, obj
    assert "kernels_render_fast.o" not in text and "FASTFTZ_kernels_render" not in text
