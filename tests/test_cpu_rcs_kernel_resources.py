"""Build-time guard for the reduced camera system (kernels_rcs.hip; no GPU needed: hipcc cross-compiles gfx950).  The unit exists in
the exact flavour only; none of its kernels -- the three sweeps (depth and descriptors, depth only, descriptors only), the resolve
kernel, the work-item kernel -- uses scratch or a flat access; the sweeps add their limbs with the native 64-bit atomic without a
returned value, never through a compare-and-swap loop, and keep their lists in LDS, which is sized at launch.  VGPRs as measured with
the pinned toolchain (what DESIGN.md section 3 states): the sweeps with descriptors 149 at occupancy 3, the depth-only sweep 108 at
occupancy 4, resolve 26 and work items 28 at occupancy 8."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels, _makefile_flags

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic\w*|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*")
SWEEPS = {"rcs_sweep_kernelILb1ELb1EE": (149, 3), "rcs_sweep_kernelILb1ELb0EE": (108, 4), "rcs_sweep_kernelILb0ELb1EE": (149, 3)}
# kernel -> (VGPRs measured, occupancy); a kernel may use fewer registers, or up to an eighth more before somebody should look
MEASURED = dict(SWEEPS, rcs_resolve_kernel=(26, 8), rcs_work_kernel=(28, 8))


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_rcs")
    fast = _fast_flags("kernels_cost")          # what any fast unit is built with: this one must compile to nothing under them
    return {"exact": _compile(d, "kernels_rcs", [], ""), "fast": _compile(d, "kernels_rcs", fast, "_fast")}


@pytest.fixture(scope="module")
def kernels(listings):
    return {flavour: _kernels(text) for flavour, text in listings.items()}


def _named(kernels, part):
    return {name: v for name, v in kernels["exact"].items() if part in name}


def test_the_unit_compiles_in_the_exact_flavour_only(kernels):
    assert not kernels["fast"], sorted(kernels["fast"])
    names = sorted(kernels["exact"])
    for part in MEASURED:
        assert len(_named(kernels, part)) == 1, (part, names)
    assert len(names) == 5, names
    assert not any("5exact" in name or "4fast" in name for name in names), names
    assert "-ffp-contract=off" in _makefile_flags()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "kernels_rcs.hip")).read()


def test_no_kernel_uses_scratch_or_a_flat_access(kernels):
    for name, (body, vgprs, scratch, occupancy) in kernels["exact"].items():
        assert scratch == 0, (name, scratch)
        assert "flat_" not in body and "scratch_" not in body, name


def test_registers_and_occupancy_are_what_the_design_states(kernels):
    for part, (measured, wanted) in MEASURED.items():
        (name, (body, vgprs, scratch, occupancy)), = _named(kernels, part).items()
        print(name, "VGPRs", vgprs, "occupancy", occupancy)
        assert vgprs <= measured + measured // 8 and occupancy == wanted, (name, vgprs, occupancy)


def test_the_list_is_dynamic_lds_within_a_compute_units(listings):
    sizes = re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", listings["exact"])
    assert sizes == ["0"] * 5, sizes          # sized at launch
    text = open(os.path.join(CSRC, "rcs_launch.h")).read()
    value = lambda name: int(re.search(r"\b%s = (\d+)" % name, text).group(1))          # noqa: E731
    entry = 12 + 18 * 64 * 4                  # a 64-bit mask, a keyframe index, 6 x 3 words of Y per lane
    assert entry == 4620 and value("kRcsDefaultWaves") * value("kRcsDefaultListCapacity") * entry == 36960 <= 64 * 1024
    assert value("kRcsMaxListCapacity") * entry <= 160 * 1024 and "160 * 1024" in text


def test_the_sweeps_add_with_native_64_bit_atomics_without_a_returned_value(kernels):
    for part in SWEEPS:
        (name, (body, *_rest)), = _named(kernels, part).items()
        assert "global_atomic_add_x2 " in body and "cmpswap" not in body, name
        assert not re.search(r"global_atomic_add(_x2)? [^\n]*\b(sc0|glc)\b", body), name          # no value returned
        assert {m.group(0) for m in ATOMIC.finditer(body)} == {"global_atomic_add_x2"}, name
        assert re.search(r"\bds_write\w*_b32\b", body) and re.search(r"\bds_read\w*_b32\b", body), name   # Y in the list
        assert "v_permlane32_swap" in body and "v_permlane16_swap" in body, name                    # the halving butterflies


def test_the_work_item_kernel_holds_no_atomic_and_resolve_only_its_flag(kernels):
    (name, (body, *_rest)), = _named(kernels, "rcs_work_kernel").items()
    assert not ATOMIC.search(body) and "global_store" in body, name
    (name, (body, *_rest)), = _named(kernels, "rcs_resolve_kernel").items()
    assert {m.group(0) for m in ATOMIC.finditer(body)} == {"global_atomic_add_x2"} and "global_store_dwordx2" in body, name


def test_the_makefile_links_the_unit_and_its_boundary_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_rcs.o", "capi_rcs.o"):
        assert text.count(f"$(OUT)/{obj}") == 1, obj
    assert "kernels_rcs_fast.o" not in text and "FASTFTZ_kernels_rcs" not in text
