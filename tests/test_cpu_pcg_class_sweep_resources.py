"""Build-time guard for the PCG sweeps (no GPU needed: hipcc cross-compiles gfx950): every instantiation of pcg_init_kernel,
pcg_step1_kernel and the persistent pcg_step1_lds_kernel -- intrinsics on / off in both kinds, one keyframe class (the sweeps without
the class loop) and several (bahip_context_set_pcg_sum_classes, keyframe sharding) -- in both arithmetic flavours, compiled with the
Makefile's own flags, keeps 4 wavefronts per SIMD (<= 128 VGPRs) and the PCG unit's scratch budget; the normals update's two
keyframe-sharded phases (kernels_surfel.hip: normals_phase_kernel) keep the surfel unit's (none)."""
import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

SWEEPS = ("pcg_init_kernel", "pcg_step1_kernel", "pcg_step1_lds_kernel")


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_pcg_classes")
    out = {}
    for flavour, suffix in (("exact", ""), ("fast", "_fast")):
        for unit in ("kernels_pcg", "kernels_surfel"):
            extra = _fast_flags(unit) if flavour == "fast" else []
            out[(flavour, unit)] = _kernels(_compile(d, unit, extra, suffix))
    return out


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_every_pcg_sweep_keeps_four_waves_per_simd_and_its_scratch_budget(listings, flavour):
    kernels = listings[(flavour, "kernels_pcg")]
    namespace = "5exact" if flavour == "exact" else "4fast"
    for sweep in SWEEPS:
        mine = {name: v for name, v in kernels.items() if f"{len(sweep)}{sweep}I" in name}
        # <kDepthIntr, kColorIntr, kClassed, Classes...>: no further argument without the class loop, one PcgClasses with it
        expected = {f"ILb{d}ELb{c}ELb{k}EJ{'NS_10PcgClassesE' if k else ''}EE" for d in (0, 1) for c in (0, 1) for k in (0, 1)}
        found = {t for t in expected for name in mine if t in name}
        assert found == expected, (sweep, sorted(mine), sorted(expected - found))
        assert len(mine) == len(expected), (sweep, sorted(mine))
        for name, (_body, vgprs, scratch, occupancy) in mine.items():
            assert namespace in name, name
            assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
            assert scratch <= 64, (name, scratch)


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_class_combine_and_normals_phases_exist_once_per_unit(listings, flavour):
    pcg = listings[(flavour, "kernels_pcg")]
    combine = [name for name in pcg if "pcg_class_combine_kernel" in name]
    assert len(combine) == (1 if flavour == "exact" else 0), combine          # plain binary32 adds: compiled once, in the exact unit
    surfel = listings[(flavour, "kernels_surfel")]
    phases = {name: v for name, v in surfel.items() if "normals_phase_kernel" in name}
    assert {("ILi1E" in n, "ILi2E" in n) for n in phases} == {(True, False), (False, True)}, sorted(phases)
    for name, (_body, vgprs, scratch, occupancy) in phases.items():
        assert vgprs <= 128 and occupancy >= 4 and scratch == 0, (name, vgprs, scratch, occupancy)
