"""Build-time guard for the lifecycle dealt over a surfel partition (no GPU needed: hipcc cross-compiles gfx950).  Its kernels live in a
unit of their own, kernels_lifecycle_dealt.hip (kernels_lifecycle.hip's exact kernel set is pinned by
tests/test_cpu_lifecycle_shard_kernel_resources.py): the chunk-restricted deletion sweep and the unpack of its exchanged rows.  Both
keep the lifecycle unit's budget -- at most 64 VGPRs, 8 wavefronts per SIMD, no scratch -- with the Makefile's flags and with the fast
flavour's flags on top (the library links the exact build: the lifecycle exists once, and the deletion's bits are delete_update's)."""
import os
import re

import pytest

from tests.test_cpu_kernel_resources import CSRC, HIPCC, _compile, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

UNIT = "kernels_lifecycle_dealt"
KERNELS = {"delete_chunks_kernel", "delete_unpack_kernel"}


def _fast_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    fast = re.search(r"^FASTFLAGS \?= (.*)$", text, re.M).group(1).split()
    ftz = re.search(r"^FASTFTZ \?= (.*)$", text, re.M).group(1).split()
    return fast + ftz


def _name(mangled):
    m = re.match(r"_ZN5bahip(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else None


@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_the_dealt_lifecycle_kernels_keep_the_lifecycle_budget(tmp_path, flavour):
    listing = _compile(tmp_path, UNIT, [] if flavour == "exact" else _fast_flags(), "_" + flavour)
    kernels = {_name(k): v for k, v in _kernels(listing).items()}
    assert set(kernels) == KERNELS, sorted(kernels)
    for name, (_body, vgprs, scratch, occupancy) in kernels.items():
        assert vgprs <= 64 and occupancy >= 8 and scratch == 0, (flavour, name, vgprs, scratch, occupancy)


def test_the_unit_is_in_the_library():
    text = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS := (.*?)\n\n", text, re.M | re.S).group(1)
    assert f"$(OUT)/{UNIT}.o" in objs
