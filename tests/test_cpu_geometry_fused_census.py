"""The census that gives tests/test_gpu_geometry_fused.py its meaning, taken on the CPU oracle: how many surfels of each 64-surfel
tile get a NEW packed normal (word 3 of the surfel row) in each of four successive geometry steps on the clouds that the GPU test
uses.  The fused route of the geometry step (kernels_surfel.hip: geometry_step, kFused) decides per tile from exactly that count
whether it holds, runs its position pass again or leaves surfels to the fix-up launch; a cloud on which the count were always zero,
or always large, would exercise one route only.  The counts are the oracle's and do not depend on the GPU."""
import numpy as np
import pytest

from tests import common
from tests.test_gpu_geometry_parked_state import _cloud, _first_keyframes

STEPS = 4


@pytest.fixture(scope="module")
def scene():
    return common.small_scene(num_keyframes=257, width=160, height=120, seed=21, translation_range=0.3, rotation_range=0.15)


@pytest.fixture(scope="module")
def oracles(scene):
    built = {}

    def get(keyframes):
        if keyframes not in built:
            ba = common.build_oracle(_first_keyframes(scene, keyframes), 8192, create_from=[0])
            built[keyframes] = (ba, common.oracle_surfels(ba)[0])
        return built[keyframes]
    return get


def changed_per_tile(ba, cloud, steps=STEPS):
    """Per step, per tile: surfels whose packed normal the step changed (activation and geometry step, joint solve)."""
    n = cloud.shape[1]
    ba.use_depth, ba.use_desc = 1, 1
    ba.surfel_data[:, :n] = cloud
    ba.active[:n] = 0
    ba.surfels.surfels_size = ba.surfels.surfel_count = n
    counts = []
    for _ in range(steps):
        before = ba.surfel_data[3, :n].view(np.uint32).copy()
        ba.update_surfel_activation()
        ba.optimize_geometry_iteration()
        changed = np.zeros((n + 63) // 64 * 64, bool)
        changed[:n] = ba.surfel_data[3, :n].view(np.uint32) != before
        counts.append(changed.reshape(-1, 64).sum(axis=1).tolist())
    return counts


@pytest.mark.parametrize("keyframes, expected", [
    (5, [[25, 0, 63, 1], [1, 0, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0]]),
    (257, [[60, 0, 64, 1], [5, 0, 4, 0], [0, 0, 0, 0], [0, 0, 0, 0]]),
    (1, [[0, 0, 0, 0]] * 4),     # one keyframe: the measured normal is the one the surfel was created with
])
def test_normals_that_change_in_four_steps_on_the_193_surfel_cloud(oracles, keyframes, expected):
    ba, data = oracles(keyframes)
    cloud, _ = _cloud(data, 193)
    assert changed_per_tile(ba, cloud) == expected


@pytest.mark.parametrize("keyframes", [5, 257])
def test_the_first_1024_surfels_as_created_hold_some_tiles_in_the_second_step(oracles, keyframes):
    ba, data = oracles(keyframes)
    first, second = changed_per_tile(ba, data[:, :1024].copy(), steps=2)
    assert len(first) == 16 and 28 <= min(first) and max(first) <= 64, first
    assert max(second) <= 5 and 0 in second and any(second), second


def test_one_keyframe_changes_no_normal_on_the_whole_cloud(oracles):
    ba, data = oracles(1)
    assert not np.any(changed_per_tile(ba, data.copy(), steps=2))
