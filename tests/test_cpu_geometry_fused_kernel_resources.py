"""Build-time guard for the fused route of the geometry step (no GPU needed: hipcc cross-compiles gfx950), from the listings of
kernels_surfel.hip compiled with the Makefile's own flags, read the way tests/test_cpu_geometry_occupancy_resources.py reads them.
geometry_fused_kernel runs where the classic one-wavefront kernel ran and must keep its budget in both arithmetic flavours: at most 96
VGPRs (five wavefronts per SIMD), no scratch, at most 8192 bytes of LDS per workgroup -- with ten more parked values than the classic
kernel, which is why the tile's bounding sphere lives in SGPRs there.  geometry_fixup_kernel is the four-wavefront shape: four
wavefronts per SIMD, no scratch.  The classic kernels are all still there."""
import re

import pytest

from tests.test_cpu_geometry_occupancy_resources import HIPCC, MAX_LDS, MAX_VGPRS, WAVES, kernels   # noqa: F401 (kernels: the fixture)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

FUSED = [(1, 1), (0, 1)]   # (use_depth, use_desc): the depth-only solve keeps the classic kernel


def _named(kernels, tag):
    flavour, res = kernels
    prefix = "4fast" if flavour == "fast" else "5exact"
    return {n: v for n, v in res.items() if prefix + tag in n}


def test_fused_kernels_fit_five_waves_per_simd_without_scratch(kernels):
    for depth, desc in FUSED:
        for activate in (0, 1):
            found = _named(kernels, "21geometry_fused_kernelILb%dELb%dELb%dEEE" % (depth, desc, activate))
            assert len(found) == 1, (depth, desc, activate, list(found))
            (name, (body, vgprs, scratch, occupancy, lds)), = found.items()
            assert vgprs <= MAX_VGPRS, (name, vgprs)
            assert scratch == 0 and "scratch_" not in body, (name, scratch)
            assert occupancy >= WAVES, (name, occupancy)
            assert 256 < lds <= MAX_LDS, (name, lds)
            assert "flat_load" not in body and "flat_store" not in body, name
            assert not re.search(r"\bv_pk_\w+_f32\b", body), name
            assert len(re.findall(r"^\s+global_load_dword\s", body, re.M)) >= 8, name
    assert len(_named(kernels, "21geometry_fused_kernelIL")) == 2 * len(FUSED)


def test_fixup_kernels_keep_four_waves_per_simd_without_scratch(kernels):
    found = _named(kernels, "21geometry_fixup_kernelIL")
    assert len(found) == 2, list(found)
    for name, (body, vgprs, scratch, occupancy, lds) in found.items():
        assert scratch == 0 and "scratch_" not in body, (name, scratch)
        assert occupancy >= 4 and vgprs <= 128, (name, occupancy, vgprs)
        assert "flat_load" not in body, name


def test_the_classic_geometry_kernels_are_all_still_there(kernels):
    for depth, desc in [(1, 0), (1, 1), (0, 1)]:
        for activate in (0, 1):
            for waves in (1, 4):
                assert len(_named(kernels, "15geometry_kernelILb%dELb%dELi%dELb%dEEE" % (depth, desc, waves, activate))) == 1, (depth, desc, waves, activate)
            assert len(_named(kernels, "22geometry_hybrid_kernelILb%dELb%dELb%dEEE" % (depth, desc, activate))) == 1
            for phase in (1, 2, 3):
                assert len(_named(kernels, "21geometry_phase_kernelILb%dELb%dELb%dELi%dEEE" % (depth, desc, activate, phase))) == 1
    for waves in (1, 4):
        assert len(_named(kernels, "14normals_kernelILi%dEEE" % waves)) == 1
