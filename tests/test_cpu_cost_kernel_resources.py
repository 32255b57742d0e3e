"""Build-time guard for the cost sweep (kernels_cost.hip; no GPU needed: hipcc cross-compiles gfx950).  Every instantiation of the sweep,
in both arithmetic flavours, keeps the budget of the hot sweeps: at most 128 VGPRs, 4 wavefronts per SIMD, no scratch.  The LDS table of
a workgroup at the largest slice fits the 64 KB a workgroup may take without an opt-in."""
import re

import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")


@pytest.fixture(scope="module")
def cost_kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_cost")
    return {"exact": _kernels(_compile(d, "kernels_cost", [], "")),
            "fast": _kernels(_compile(d, "kernels_cost", _fast_flags("kernels_cost"), "_fast"))}


def test_every_cost_sweep_instantiation_keeps_the_budget(cost_kernels):
    for flavour, kernels in cost_kernels.items():
        sweeps = {name: v for name, v in kernels.items() if "cost_kernel" in name}
        assert len(sweeps) == 3, (flavour, sorted(kernels))          # depth + descriptors, depth only, descriptors only
        assert all(f"5bahip{len(flavour)}{flavour}" in name for name in sweeps), (flavour, sorted(sweeps))
        for name, (body, vgprs, scratch, occupancy) in sweeps.items():
            assert vgprs <= 128 and occupancy >= 4 and scratch == 0, (flavour, name, vgprs, scratch, occupancy)
            assert not re.search(r"\bv_pk_(fma|mul|add)_f32\b", body), name       # SLP packing stays off


def test_the_largest_lds_table_fits_a_workgroup_without_an_opt_in():
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "badslam_amd", "csrc", "ba_launch.h")).read()
    slice_ = int(re.search(r"kCostMaxSlice = (\d+)", src).group(1))
    cell = int(re.search(r"kCostCellWords = (\d+)", src).group(1))
    assert slice_ * (3 * cell + 3) * 8 <= 64 * 1024
