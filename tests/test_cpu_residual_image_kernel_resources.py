"""Build-time guard for the residual images (kernels_residual_image.hip; no GPU needed: hipcc cross-compiles gfx950).  The unit exists
in the exact flavour only; none of its kernels -- clear, sweep, resolve with and without descriptors -- uses scratch or a flat access;
the sweep takes its minimum with the native 64-bit unsigned atomic and counts with the 32-bit add, both without a returned value and
never through a compare-and-swap loop, and never reads the planes; clear and resolve hold no atomic; the Makefile links the unit and
its boundary once.  VGPRs as measured with the pinned toolchain: clear 8, sweep 44, resolve 33 with descriptors and 23 without, all at
occupancy 8."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels, _makefile_flags

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic\w*|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*")
# kernel -> VGPRs measured (the doc string); a kernel may use fewer, or up to a quarter more before somebody should look
MEASURED_VGPRS = {"residual_image_clear_kernel": 8, "residual_image_sweep_kernel": 44, "residual_image_resolve_kernelILb1E": 33,
                  "residual_image_resolve_kernelILb0E": 23}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_residual_image")
    fast = _fast_flags("kernels_cost")          # what any fast unit is built with: this one must compile to nothing under them
    return {"exact": _kernels(_compile(d, "kernels_residual_image", [], "")),
            "fast": _kernels(_compile(d, "kernels_residual_image", fast, "_fast"))}


def _named(kernels, part):
    return {name: v for name, v in kernels["exact"].items() if part in name}


def test_the_unit_compiles_in_the_exact_flavour_only(kernels):
    assert not kernels["fast"], sorted(kernels["fast"])
    names = sorted(kernels["exact"])
    for part in MEASURED_VGPRS:
        assert len(_named(kernels, part)) == 1, (part, names)
    assert len(names) == 4, names
    assert not any("5exact" in name or "4fast" in name for name in names), names
    assert "-ffp-contract=off" in _makefile_flags()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "kernels_residual_image.hip")).read()


def test_no_kernel_uses_scratch_or_a_flat_access(kernels):
    for name, (body, vgprs, scratch, occupancy) in kernels["exact"].items():
        assert scratch == 0, (name, scratch)
        assert "flat_" not in body and "scratch_" not in body, name


def test_registers_stay_near_what_was_measured(kernels):
    for part, measured in MEASURED_VGPRS.items():
        (name, (body, vgprs, scratch, occupancy)), = _named(kernels, part).items()
        print(name, "VGPRs", vgprs, "occupancy", occupancy)
        assert vgprs <= measured + measured // 4 and occupancy == 8, (name, vgprs, occupancy)


def test_the_sweep_uses_the_native_atomics_without_a_returned_value(kernels):
    (name, (body, *_rest)), = _named(kernels, "residual_image_sweep_kernel").items()
    assert "global_atomic_umin_x2" in body and "global_atomic_add " in body, name
    assert "cmpswap" not in body, name
    assert not re.search(r"global_atomic_(umin_x2|add) [^\n]*\b(sc0|glc)\b", body), name          # no value returned
    assert {m.group(0) for m in ATOMIC.finditer(body)} == {"global_atomic_umin_x2", "global_atomic_add"}, name
    assert "global_load_dwordx2" not in body, name          # the key is never read back: the atomics are the only accesses to the planes
    assert not re.search(r"\bds_(read|write|load|store)", body), name          # no LDS table (the cull's ds_swizzle touches no memory)


def test_clear_and_resolve_hold_no_atomic(kernels):
    for part in ("residual_image_clear_kernel", "residual_image_resolve_kernel"):
        for name, (body, *_rest) in _named(kernels, part).items():
            assert not ATOMIC.search(body), name
            assert "global_store" in body, name


def test_the_makefile_links_the_unit_and_its_boundary_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_residual_image.o", "capi_residual_image.o"):
        assert text.count(f"$(OUT)/{obj}") == 1, obj
    assert "kernels_residual_image_fast.o" not in text and "FASTFTZ_kernels_residual_image" not in text
