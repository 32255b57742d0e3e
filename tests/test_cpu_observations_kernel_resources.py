"""Build-time guard for the observation lists (kernels_observations.hip; no GPU needed: hipcc cross-compiles gfx950).  The unit exists in
the exact flavour only; none of its kernels -- the count sweep and the four fill sweeps (direct and staged, each with and without the
descriptor payload) -- uses scratch or a flat access; the fill sweeps hold no atomic at all and the count sweep only the one 64-bit add
of its total; the staged fill keeps its window in LDS, which is sized at launch: no static LDS, 2 + 4 + 8 bytes per entry and
wavefront for the planes asked for, 57 344 bytes per workgroup in the default shape with every plane and 65 536 at most.  VGPRs as
measured with the pinned toolchain (what DESIGN.md section 3 states): count 52 at occupancy 8; direct fill 57 at occupancy 7 -- the
co-visibility sweep's -- without descriptors and 80 at occupancy 6 with them (cost_pairs<true, true>: the descriptor gathers);
staged fill 78 at 6 and 103 at 4 (it carries the window's addresses and the range's base beside the direct form's state; its
residency is set by its LDS, not by its registers: two workgroups of four wavefronts per compute unit with every plane)."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels, _makefile_flags

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

ATOMIC = re.compile(r"\b(global|flat|buffer)_atomic\w*|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*")
# kernel -> (VGPRs measured, occupancy); a kernel may use fewer registers, or up to an eighth more before somebody should look
MEASURED = {"observations_count_kernel": (52, 8), "observations_fill_direct_kernelILb0E": (57, 7), "observations_fill_direct_kernelILb1E": (80, 6),
            "observations_fill_staged_kernelILb0E": (78, 6), "observations_fill_staged_kernelILb1E": (103, 4)}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_observations")
    fast = _fast_flags("kernels_cost")          # what any fast unit is built with: this one must compile to nothing under them
    return {"exact": _compile(d, "kernels_observations", [], ""), "fast": _compile(d, "kernels_observations", fast, "_fast")}


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
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "kernels_observations.hip")).read()


def test_no_kernel_uses_scratch_or_a_flat_access(kernels):
    for name, (body, vgprs, scratch, occupancy) in kernels["exact"].items():
        assert scratch == 0, (name, scratch)
        assert "flat_" not in body and "scratch_" not in body, name


def test_registers_and_occupancy_are_what_the_design_states(kernels):
    for part, (measured, wanted) in MEASURED.items():
        (name, (body, vgprs, scratch, occupancy)), = _named(kernels, part).items()
        print(name, "VGPRs", vgprs, "occupancy", occupancy)
        assert vgprs <= measured + measured // 8 and occupancy == wanted, (name, vgprs, occupancy)


def test_the_window_is_dynamic_lds_of_the_stated_size(listings):
    sizes = re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", listings["exact"])
    assert sizes == ["0"] * 5, sizes          # sized at launch
    text = open(os.path.join(CSRC, "ba_launch.h")).read()
    value = lambda name: int(re.search(r"\b%s = (\d+)" % name, text).group(1))          # noqa: E731
    entry = value("kObsKeyframeBytes") + value("kObsDepthBytes") + value("kObsDescriptorBytes")
    assert entry == 14 == 2 + 4 + 8          # a keyframe index, a depth word, two descriptor words
    assert value("kObsDefaultWaves") * value("kObsDefaultStageEntries") * entry == 57344
    assert value("kObsMaxLdsBytes") == 65536 == 64 * 1024          # what the launcher clamps waves x window x entry bytes to
    assert "kObsMaxLdsBytes / (g.waves * entry)" in open(os.path.join(CSRC, "kernels_observations.hip")).read()


def test_the_fill_kernels_hold_no_atomic(kernels):
    for part in [p for p in MEASURED if "fill" in p]:
        for name, (body, *_rest) in _named(kernels, part).items():
            assert not ATOMIC.search(body), name


def test_the_count_kernel_holds_only_the_add_of_its_total(kernels):
    (name, (body, *_rest)), = _named(kernels, "observations_count_kernel").items()
    assert [m.group(0) for m in ATOMIC.finditer(body)] == ["global_atomic_add_x2"], name


def test_the_makefile_links_the_unit_and_its_boundary_once():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_observations.o", "capi_observations.o"):
        assert text.count(f"$(OUT)/{obj}") == 1, obj
    assert "kernels_observations_fast.o" not in text and "FASTFTZ_kernels_observations" not in text
