"""Build-time guard for the intrinsics sweep (no GPU needed: hipcc cross-compiles gfx950): every instantiation of
intrinsics_accumulate_kernel -- depth + colour, depth, colour; one keyframe class (the sweep without the class loop) and several
(bahip_context_set_intrinsics_sum_classes, keyframe sharding) -- in both arithmetic flavours, compiled with the Makefile's own
flags, keeps 4 wavefronts per SIMD (<= 128 VGPRs) and no scratch (spills)."""
import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _fast_flags, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_intrinsics")
    out = {}
    for flavour, extra, suffix in (("exact", [], ""), ("fast", _fast_flags("kernels_intrinsics"), "_fast")):
        kernels = _kernels(_compile(d, "kernels_intrinsics", extra, suffix))
        out[flavour] = {name: v for name, v in kernels.items() if "intrinsics_accumulate_kernel" in name}
    return out


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_every_intrinsics_sweep_keeps_four_waves_per_simd_without_spills(sweeps, flavour):
    kernels = sweeps[flavour]
    # <kDepth, kColor, kClassed>: (1, 1), (1, 0), (0, 1) x (one class, classes)
    expected = {f"ILb{d}ELb{c}ELb{k}EE" for d, c in ((1, 1), (1, 0), (0, 1)) for k in (0, 1)}
    found = {t for t in expected for name in kernels if t in name}
    assert found == expected, (sorted(kernels), sorted(expected - found))
    assert len(kernels) == len(expected)
    namespace = "5exact" if flavour == "exact" else "4fast"
    for name, (_body, vgprs, scratch, occupancy) in kernels.items():
        assert namespace in name, name
        assert vgprs <= 128 and occupancy >= 4, (name, vgprs, occupancy)
        assert scratch == 0, (name, scratch)
