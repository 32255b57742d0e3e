"""Build-time guard for the keyframe-sharded lifecycle (no GPU needed: hipcc cross-compiles gfx950).  The sharded calls add kernels of
their own (the creation batch's candidate export, filter count and decide; deletion's partial sweep and decide) and reuse the batch
kernels over one row at a time; no kernel of the unsharded lifecycle changes.  So: every kernel the unit had before compiles, with the
Makefile's flags, to the same gfx950 code (block labels and comments aside: their numbers follow the kernel's place in the unit), and
the new kernels keep the unit's budget -- 8 wavefronts per SIMD, no scratch."""
import hashlib
import re

import pytest

from tests.test_cpu_kernel_resources import HIPCC, _compile, _kernels

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the build container has it)")

# sha256 (first 24 hex digits) of each kernel's normalised gfx950 code before keyframe sharding reached the lifecycle
UNSHARDED = {
    "sort_keys_kernel": "fad7b0a09145dad93837a027",
    "create_flag_kernel": "67cc89a7b19683e609cea112",
    "gather_rows_kernel": "568239ee3bd06041fd519514",
    "merge_apply_kernel": "c0d15f4b15fdd17eba88f12b",
    "merge_pairs_kernel": "81a116e48f33011f060819a9",
    "compact_flag_kernel": "2c7e8028507d81a37e3b8f7b",
    "compact_move_kernel": "c62141d923b24b6f479a8102",
    "create_chain_kernel": "46c0b9286302bdad984f3a2e",
    "merge_decide_kernel": "c40c482de7bb6369746dde4b",
    "create_append_kernel": "add75efcdbf71e356d29364d",
    "create_filter_kernel": "27510a2026fee2a7a909c6f6",
    "delete_update_kernel": "f9e37f28cd6fc7e11985087f",
    "cloud_to_shard_kernel": "057b7b101191ec9ae3237141",
    "shard_to_cloud_kernel": "e4ccb97f39b74c4b1601b41e",
    "supporting_fill_kernel": "022b23cd9710a7e259c3e8ae",
    "lifecycle_bounds_kernel": "21f511faa29d96d121a96c25",
    "merge_batch_fill_kernel": "fc64221eb171a85e147394eb",
    "compact_free_list_kernel": "60f9d553e271f307fedaadff",
    "create_batch_flag_kernel": "28b44b0a775e63f9cdbd2302",
    "merge_batch_apply_kernel": "89fc79e214da6594121e170a",
    "scatter_rows_back_kernel": "6fb4e231aa66fa3f8cbdd433",
    "supporting_insert_kernel": "1cec1ed2a2b16c6179768411",
    "merge_apply_insert_kernel": "0112a9c540bd66bfe0159d5d",
    "create_append_fused_kernel": "fd63c0483bfa15dd49a8199f",
    "create_batch_filter_kernel": "d17954b66205d82c04ea684e",
    "create_batch_records_kernel": "68dd4d432ef2ac08528383d8",
    "merge_batch_associate_kernel": "3d1971ab63f3d6b2dbee02eb",
    "create_batch_occupancy_kernel": "9a95e9f641735700d8521428",
    "lifecycle_visible_tiles_kernel": "14bef9297c883b966a4346be",
    "merge_batch_frame_first_kernel": "54def10152822ac35742fbf2",
}
SHARDED = ("create_batch_export_kernel", "create_batch_filter_count_kernel", "create_batch_filter_decide_kernel", "delete_partial_kernel",
           "delete_decide_kernel")


def _name(mangled):
    m = re.match(r"_ZN5bahip(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else None


def _digest(body):
    body = re.sub(r";.*", "", body)
    body = re.sub(r"\.LBB\d+_", ".LBB_", body)
    return hashlib.sha256("\n".join(line.rstrip() for line in body.splitlines() if line.strip()).encode()).hexdigest()[:24]


@pytest.fixture(scope="module")
def lifecycle(tmp_path_factory):
    kernels = _kernels(_compile(tmp_path_factory.mktemp("isa_lifecycle"), "kernels_lifecycle", [], ""))
    return {_name(k): v for k, v in kernels.items() if _name(k)}


def test_the_unsharded_lifecycle_kernels_are_the_code_of_before(lifecycle):
    missing = sorted(set(UNSHARDED) - set(lifecycle))
    assert not missing, missing
    changed = sorted(name for name, digest in UNSHARDED.items() if _digest(lifecycle[name][0]) != digest)
    assert not changed, changed


def test_the_sharded_lifecycle_kernels_keep_the_units_budget(lifecycle):
    assert set(lifecycle) == set(UNSHARDED) | set(SHARDED), sorted(set(lifecycle) ^ (set(UNSHARDED) | set(SHARDED)))
    for name in SHARDED:
        _body, vgprs, scratch, occupancy = lifecycle[name]
        assert vgprs <= 64 and occupancy >= 8 and scratch == 0, (name, vgprs, scratch, occupancy)
