"""Build-time guard for the per-surfel cost sweep (kernels_surfel_cost.hip; no GPU needed: hipcc cross-compiles gfx950).  Every
instantiation of the sweep, in both arithmetic flavours: no scratch, at most 128 VGPRs, at least the register occupancy of the cost
sweep with the same residual selection; its sink is plain LDS read-modify-write in per-lane columns and plain global stores -- no
atomic of any kind, no flat access, no packed-binary32 arithmetic.  The kernel that resolves staged words exists once."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

SELECTIONS = ("ILb1ELb1E", "ILb1ELb0E", "ILb0ELb1E")     # <depth, desc>


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_surfel_cost")
    return {unit: {"exact": _kernels(_compile(d, unit, [], "")), "fast": _kernels(_compile(d, unit, _fast_flags(unit), "_fast"))}
            for unit in ("kernels_surfel_cost", "kernels_cost")}


def _sweeps(kernels, flavour):
    return {name: v for name, v in kernels["kernels_surfel_cost"][flavour].items() if "surfel_cost_kernel" in name}


def test_three_sweep_kernels_per_flavour_within_the_budget(kernels):
    for flavour in ("exact", "fast"):
        sweeps = _sweeps(kernels, flavour)
        assert len(sweeps) == 3, (flavour, sorted(kernels["kernels_surfel_cost"][flavour]))
        assert all(f"5bahip{len(flavour)}{flavour}" in name for name in sweeps), (flavour, sorted(sweeps))
        for name, (body, vgprs, scratch, occupancy) in sweeps.items():
            assert scratch == 0 and vgprs <= 128, (flavour, name, vgprs, scratch)


def test_each_sweep_allows_the_occupancy_of_the_cost_sweep_of_its_selection(kernels):
    for flavour in ("exact", "fast"):
        sweeps = _sweeps(kernels, flavour)
        cost = {name: v for name, v in kernels["kernels_cost"][flavour].items() if "cost_kernel" in name}
        for selection in SELECTIONS:
            mine = [v for name, v in sweeps.items() if "surfel_cost_kernel" + selection in name]
            theirs = [v for name, v in cost.items() if "cost_kernel" + selection in name and "surfel" not in name]
            assert len(mine) == 1 and len(theirs) == 1, (flavour, selection, sorted(sweeps), sorted(cost))
            assert mine[0][3] >= theirs[0][3], (flavour, selection, mine[0][3], theirs[0][3])


def test_the_sink_has_no_atomic_no_flat_access_and_no_packed_arithmetic(kernels):
    for flavour in ("exact", "fast"):
        for name, (body, *_rest) in _sweeps(kernels, flavour).items():
            assert "flat_load" not in body and "flat_store" not in body, name
            assert "global_atomic" not in body and "buffer_atomic" not in body and "flat_atomic" not in body, name
            assert not re.search(r"\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg|pk_add)\w*", body), name     # LDS atomics
            assert not re.search(r"\bv_pk_(fma|mul|add)_f32\b", body), name
            # the accumulators: 64-bit LDS reads and writes in the lane's own columns, the results: global stores
            assert re.search(r"\bds_read2?_b64\b", body) and re.search(r"\bds_write2?_b64\b", body), name
            assert "global_store_dwordx2" in body and "global_store_dword " in body, name


def test_the_resolve_kernel_exists_once_in_the_exact_flavour_only(kernels):
    exact = [name for name in kernels["kernels_surfel_cost"]["exact"] if "surfel_cost_resolve_kernel" in name]
    fast = [name for name in kernels["kernels_surfel_cost"]["fast"] if "resolve" in name]
    assert len(exact) == 1 and not fast, (exact, fast)
    assert "5exact" not in exact[0] and "4fast" not in exact[0], exact
    body, vgprs, scratch, occupancy = kernels["kernels_surfel_cost"]["exact"][exact[0]]
    assert scratch == 0, (exact[0], scratch)
    assert "global_atomic" not in body, exact[0]
    # nothing but the sweeps is compiled a second time
    assert all("4fast" in name for name in kernels["kernels_surfel_cost"]["fast"]), sorted(kernels["kernels_surfel_cost"]["fast"])


def test_the_makefile_builds_both_flavours_with_the_cost_units_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    for obj in ("kernels_surfel_cost.o", "kernels_surfel_cost_fast.o", "capi_surfel_cost.o"):
        assert f"$(OUT)/{obj}" in text, obj
    assert _fast_flags("kernels_surfel_cost") == _fast_flags("kernels_cost")


def test_two_workgroups_of_the_default_shape_fit_a_compute_unit():
    src = open(os.path.join(CSRC, "ba_launch.h")).read()
    per_wave = 3 * int(re.search(r"kCostCellWords = (\d+)", src).group(1)) * 64 * 8
    assert per_wave == 13824
    waves = int(re.search(r"kSurfelCostDefaultWaves = (\d+)", src).group(1))
    per_unit = int(re.search(r"kSurfelCostWorkgroupsPerUnit = (\d+)", src).group(1))
    assert per_unit >= 2 and per_unit * waves * per_wave <= 160 * 1024
    assert waves * per_wave <= 64 * 1024                                 # the default shape needs no opt-in for its LDS
