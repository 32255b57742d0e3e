"""Build-time guard for the one-wavefront geometry kernel (no GPU needed: hipcc cross-compiles gfx950), from the listings of
kernels_surfel.hip compiled with the Makefile's own flags, the way tests/test_cpu_kernel_resources.py reads them: every
geometry_kernel<depth, desc, 1, activate> must keep what DESIGN.md section 3 ("five wavefronts per SIMD") relies on in both
arithmetic flavours -- at most 96 VGPRs (512 registers / 5 wavefronts at the allocation granule of 8), no scratch, the cold
per-lane state parked in at most 8192 bytes of LDS per workgroup (160 KiB / 20 workgroups per compute unit), gathers through
global_load, no packed-binary32 VALU code."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "badslam_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

# (use_depth, use_desc) x activation decided inside the sweep: the instantiations launch_geometry_shape<1, .> can start
SELECTIONS = [(1, 0), (1, 1), (0, 1)]
WAVES = 5
MAX_VGPRS = 512 // WAVES // 8 * 8      # 96
MAX_LDS = 160 * 1024 // (4 * WAVES)    # 8192


def _flags(fast):
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = [f for f in re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split() if f != "-fPIC"]
    if fast:
        flags += re.search(r"^FASTFLAGS \?= (.*)$", text, re.M).group(1).split()
        per_unit = re.search(r"^FASTFTZ_kernels_surfel \?=(.*)$", text, re.M).group(1).strip()
        flags += re.search(r"^FASTFTZ \?= (.*)$", text, re.M).group(1).split() if per_unit == "$(FASTFTZ)" else per_unit.split()
    return flags


@pytest.fixture(scope="module", params=["exact", "fast"])
def kernels(request, tmp_path_factory):
    """name -> (body, NumVgprs, ScratchSize, Occupancy, LDS bytes) of every kernel of the unit, in one flavour"""
    path = str(tmp_path_factory.mktemp("isa_geometry") / ("kernels_surfel_%s.s" % request.param))
    subprocess.run([HIPCC] + _flags(request.param == "fast") + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", path,
                    os.path.join(CSRC, "kernels_surfel.hip")], check=True, timeout=900, capture_output=True)
    res = {}
    for m in re.finditer(r"^(_Z\w+):\s*;.*?\n(.*?)s_endpgm.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; LDSByteSize: (\d+).*?; Occupancy: (\d+)",
                         open(path).read(), re.S | re.M):
        res[m.group(1)] = (m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(6)), int(m.group(5)))
    return request.param, res


def _one_wavefront_kernels(kernels):
    flavour, res = kernels
    picked = {}
    for depth, desc in SELECTIONS:
        for activate in (0, 1):
            tag = "%s15geometry_kernelILb%dELb%dELi1ELb%dEEE" % ("4fast" if flavour == "fast" else "5exact", depth, desc, activate)
            names = [n for n in res if tag in n]
            assert len(names) == 1, (tag, names)
            picked[(depth, desc, activate)] = res[names[0]]
    return picked


def test_one_wavefront_geometry_kernels_fit_five_waves_per_simd_without_scratch(kernels):
    for key, (body, vgprs, scratch, occupancy, lds) in _one_wavefront_kernels(kernels).items():
        assert vgprs <= MAX_VGPRS, (kernels[0], key, vgprs)
        assert scratch == 0 and "scratch_" not in body, (kernels[0], key, scratch)
        assert occupancy >= WAVES, (kernels[0], key, occupancy)
        assert lds <= MAX_LDS, (kernels[0], key, lds)


def test_the_joint_solve_parks_its_cold_state_in_lds_and_the_depth_only_solve_does_not(kernels):
    """The block is [slot][64 lanes] of dwords behind one base address per lane: every access is a ds_read / ds_write of dwords with
    an immediate offset (single, or two slots at a stride of 64 dwords), none wider and none through a flat address."""
    for (depth, desc, activate), (body, vgprs, scratch, occupancy, lds) in _one_wavefront_kernels(kernels).items():
        parked = re.findall(r"^\s+(ds_(?:read|write)\w*)\s", body, re.M)
        if not desc:
            assert lds == 256 and not [op for op in parked if op not in ("ds_read_b64", "ds_write_b64", "ds_swizzle_b32")], (depth, desc, activate, lds)
            continue
        assert 256 < lds <= MAX_LDS and lds % 256 == 0, lds
        allowed = {"ds_read_b32", "ds_write_b32", "ds_read2st64_b32", "ds_write2st64_b32", "ds_read2_b32", "ds_write2_b32",
                   "ds_read_b64", "ds_write_b64"}      # (b64: the candidate masks, one word per chunk)
        assert set(parked) <= allowed, set(parked) - allowed
        assert sum(op.startswith("ds_read") and op != "ds_read_b64" for op in parked) >= 6, parked
        assert "flat_load" not in body and "flat_store" not in body


def test_gathers_stay_global_loads_and_the_slp_vectoriser_stays_off(kernels):
    for key, (body, *_rest) in _one_wavefront_kernels(kernels).items():
        assert "flat_load" not in body, key
        assert len(re.findall(r"^\s+global_load_dword\s", body, re.M)) >= 8, key
        assert not re.search(r"\bv_pk_\w+_f32\b", body), key


def test_the_other_shapes_keep_their_budget(kernels):
    """The four-wavefront shape, the hybrid shape and the phase kernels of keyframe sharding are not parked: no block of theirs
    grew, and they stay at four wavefronts per SIMD."""
    flavour, res = kernels
    seen = 0
    for name, (body, vgprs, scratch, occupancy, lds) in res.items():
        if "geometry_kernelILb" in name and "ELi4E" in name:
            seen += 1
            assert lds == 8 * 8 * 64 * 4 and occupancy >= 4 and scratch == 0, (name, lds, occupancy, scratch)   # (the class partials alone)
        if "geometry_phase_kernel" in name:
            seen += 1
            assert lds == 0 and occupancy >= 4, (name, lds, occupancy)
    assert seen >= 6 + 18
