"""Build-time guard for the tile mask table (kernels_tile_masks.hip; no GPU needed: hipcc cross-compiles gfx950).  The unit exists in the
exact flavour only; none of its kernels uses scratch or a flat access; the reductions add with the native 32-bit atomic without a
returned value (the counters with the 64-bit one), never through a compare-and-swap loop; no kernel waits for another workgroup (no
acquire / release traffic, no sleep); LDS only in the redundancy reduction, sized at launch: 12 bytes per (bin, mask) entry, 64 entries
per wavefront, 6 144 bytes per workgroup at most.  VGPRs as measured with the pinned toolchain (what DESIGN.md section 3 states): the
count sweep 51 and the fill sweep 50 at occupancy 7, the payload sweep 66 at 7 without and 90 at 5 with descriptors, everything that
reads the table only at most 26 at occupancy 8."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels, _makefile_flags

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic\w*|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*")
# kernel -> (VGPRs measured, occupancy); a kernel may use fewer registers, or up to an eighth more before somebody should look
MEASURED = {"tile_mask_count_kernel": (51, 7), "tile_mask_offsets_kernel": (8, 8), "tile_mask_fill_kernel": (50, 7),
            "tile_mask_pack_kernel": (8, 8), "tile_mask_unpack_kernel": (10, 8), "tile_mask_merge_kernel": (16, 8),
            "tile_mask_covisibility_kernel": (21, 8), "tile_mask_redundancy_kernel": (26, 8), "tile_mask_observation_counts_kernel": (12, 8),
            "tile_mask_observation_keyframes_kernel": (18, 8), "tile_mask_payload_kernelILb0": (66, 7), "tile_mask_payload_kernelILb1": (90, 5),
            "tile_mask_words_pack_kernel": (7, 8), "tile_mask_words_unpack_kernel": (5, 8), "tile_mask_census_kernel": (6, 8)}
ADDING = {"tile_mask_covisibility_kernel": {"global_atomic_add", "global_atomic_add_x2"},
          "tile_mask_redundancy_kernel": {"global_atomic_add", "global_atomic_add_x2"},
          "tile_mask_count_kernel": {"global_atomic_add_x2"}, "tile_mask_observation_counts_kernel": {"global_atomic_add_x2"},
          "tile_mask_payload_kernelILb0": {"global_atomic_add_x2"}, "tile_mask_payload_kernelILb1": {"global_atomic_add_x2"}}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_tile_masks")
    fast = _fast_flags("kernels_cost")          # what any fast unit is built with: this one must compile to nothing under them
    return {"exact": _compile(d, "kernels_tile_masks", [], ""), "fast": _compile(d, "kernels_tile_masks", fast, "_fast")}


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
    assert len(names) == len(MEASURED), names
    assert not any("5exact" in name or "4fast" in name for name in names), names
    assert "-ffp-contract=off" in _makefile_flags()
    source = open(os.path.join(CSRC, "kernels_tile_masks.hip")).read()
    assert "#pragma clang fp contract(off)" in source and "#ifndef BAHIP_FAST_MATH" in source


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
    section = design[design.index("### The tile mask table"):]
    assert "51 VGPRs" in section and "90 VGPRs" in section


def test_lds_is_dynamic_and_of_the_stated_size(listings):
    sizes = re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", listings["exact"])
    assert sizes == ["0"] * len(MEASURED), sizes          # sized at launch, and only the redundancy reduction asks for any
    text = open(os.path.join(CSRC, "ba_launch.h")).read()
    value = lambda name: int(re.search(r"\b%s = (\d+)" % name, text).group(1))          # noqa: E731
    assert value("kTileMaskBinBytes") == 12 == 8 + 4          # a 64-bit mask and a bin
    assert value("kTileMaskMaxWaves") * 64 * value("kTileMaskBinBytes") == 6144


def test_adds_are_native_atomics_without_a_returned_value(kernels):
    for part in MEASURED:
        (name, (body, *_rest)), = _named(kernels, part).items()
        found = {m.group(0) for m in ATOMIC.finditer(body)}
        assert found == ADDING.get(part, set()), (name, found)
        assert "cmpswap" not in body, name
        assert not re.search(r"global_atomic_add(_x2)? [^\n]*\b(sc0|glc)\b", body), name          # no value returned
    for part in ("tile_mask_covisibility_kernel", "tile_mask_redundancy_kernel"):
        (name, (body, *_rest)), = _named(kernels, part).items()
        assert "global_atomic_add " in body, name
        assert "s_bcnt1_i32_b64" in body or "v_bcnt_u32_b32" in body, name          # the population count


def test_no_kernel_waits_for_another_workgroup(kernels):
    for name, (body, *_rest) in kernels["exact"].items():
        assert "s_sleep" not in body and "buffer_wbl2" not in body and "buffer_inv" not in body, name
        assert not re.search(r"global_load[^\n]*\bsc1\b", body), name


def test_the_makefile_links_the_unit_and_its_boundary_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_tile_masks.o", "capi_tile_masks.o"):
        assert text.count(f"$(OUT)/{obj}") == 1, obj
    assert "kernels_tile_masks_fast.o" not in text and "FASTFTZ_kernels_tile_masks" not in text
