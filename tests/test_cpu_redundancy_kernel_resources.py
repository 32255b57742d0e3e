"""Build-time guard for the keyframe redundancy (kernels_redundancy.hip; no GPU needed: hipcc cross-compiles gfx950).  The unit exists in
the exact flavour only; none of its kernels -- clear, sweep, widen, narrow -- uses scratch or a flat access; the sweep adds with the
native 32-bit atomic without a returned value (its census words with the 64-bit one), never through a compare-and-swap loop, and keeps
its list and the bins of a tile in LDS, which is sized at launch: no static LDS, 12 bytes per entry and wavefront, list_capacity + 64
entries, 18 432 bytes per workgroup in the default shape and 49 152 at most.  VGPRs as measured with the pinned toolchain (what
DESIGN.md section 3 states): sweep 70 at occupancy 7 -- beside the co-visibility sweep's 68 at 7 --, clear 4, widen and narrow 6, at
occupancy 8."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels, _makefile_flags

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic\w*|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*")
# kernel -> (VGPRs measured, occupancy); a kernel may use fewer registers, or up to an eighth more before somebody should look
MEASURED = {"redundancy_clear_kernel": (4, 8), "redundancy_sweep_kernel": (70, 7), "redundancy_widen_kernel": (6, 8),
            "redundancy_narrow_kernel": (6, 8)}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_redundancy")
    fast = _fast_flags("kernels_cost")          # what any fast unit is built with: this one must compile to nothing under them
    return {"exact": _compile(d, "kernels_redundancy", [], ""), "fast": _compile(d, "kernels_redundancy", fast, "_fast")}


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
    assert len(names) == 4, names
    assert not any("5exact" in name or "4fast" in name for name in names), names
    assert "-ffp-contract=off" in _makefile_flags()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "kernels_redundancy.hip")).read()


def test_no_kernel_uses_scratch_or_a_flat_access(kernels):
    for name, (body, vgprs, scratch, occupancy) in kernels["exact"].items():
        assert scratch == 0, (name, scratch)
        assert "flat_" not in body and "scratch_" not in body, name


def test_registers_and_occupancy_are_what_the_design_states(kernels):
    for part, (measured, wanted) in MEASURED.items():
        (name, (body, vgprs, scratch, occupancy)), = _named(kernels, part).items()
        print(name, "VGPRs", vgprs, "occupancy", occupancy)
        assert vgprs <= measured + measured // 8 and occupancy == wanted, (name, vgprs, occupancy)
    design = open(os.path.join(os.path.dirname(CSRC), "..", "DESIGN.md")).read()
    assert "70 VGPRs" in design[design.index("### Keyframe redundancy"):]


def test_the_list_is_dynamic_lds_of_the_stated_size(listings):
    sizes = re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", listings["exact"])
    assert sizes == ["0"] * 4, sizes          # sized at launch
    text = open(os.path.join(CSRC, "ba_launch.h")).read()
    value = lambda name: int(re.search(r"\b%s = (\d+)" % name, text).group(1))          # noqa: E731
    assert value("kRedundancyEntryBytes") == 12 == 8 + 4          # a 64-bit mask and a keyframe index or a bin
    assert value("kRedundancyMaxBins") == 64                       # one (bin, mask) entry per lane at most
    assert value("kRedundancyDefaultWaves") * (value("kRedundancyDefaultListCapacity") + 64) * value("kRedundancyEntryBytes") == 18432
    assert value("kRedundancyMaxWaves") * (value("kRedundancyMaxListCapacity") + 64) * value("kRedundancyEntryBytes") == 49152 <= 64 * 1024


def test_the_sweep_adds_with_native_atomics_without_a_returned_value(kernels):
    (name, (body, *_rest)), = _named(kernels, "redundancy_sweep_kernel").items()
    assert "global_atomic_add " in body and "cmpswap" not in body, name
    assert not re.search(r"global_atomic_add(_x2)? [^\n]*\b(sc0|glc)\b", body), name          # no value returned
    assert {m.group(0) for m in ATOMIC.finditer(body)} == {"global_atomic_add", "global_atomic_add_x2"}, name
    assert re.search(r"\bds_write_b64\b", body) and re.search(r"\bds_read_b64\b", body), name  # the list of masks
    assert "s_bcnt1_i32_b64" in body or "v_bcnt_u32_b32" in body, name                         # the population count


def test_the_other_kernels_hold_no_atomic(kernels):
    for part in ("redundancy_clear_kernel", "redundancy_widen_kernel", "redundancy_narrow_kernel"):
        for name, (body, *_rest) in _named(kernels, part).items():
            assert not ATOMIC.search(body), name
            assert "global_store" in body, name


def test_the_makefile_links_the_unit_and_its_boundary_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_redundancy.o", "capi_redundancy.o"):
        assert text.count(f"$(OUT)/{obj}") == 1, obj
    assert "kernels_redundancy_fast.o" not in text and "FASTFTZ_kernels_redundancy" not in text
