"""The CPU model of the objective per surfel (tests/surfel_costs.py) against the oracle's own total (orc_evaluate_cost), on the scenes
of tests/two_cameras.py whose colour camera differs from the depth camera; and that those scenes give the model real work.  The GPU
tests (tests/test_gpu_surfel_costs.py) hold the new sweep to this model bit for bit."""
import math

import pytest

from tests import surfel_costs as sc
from tests import two_cameras as tcam


@pytest.fixture(scope="module", params=["tiny", "crop_small"])
def loaded(request):
    tc = tcam.build_scene(request.param)
    ba = tcam.build_oracle(tc)
    return tc, ba, sc.oracle_pair_words(ba)


@pytest.mark.parametrize("use_depth,use_desc", sc.KINDS)
def test_the_models_grand_total_is_the_oracles_cost(loaded, use_depth, use_desc):
    tc, ba, words = loaded
    planes = sc.model(words, use_depth, use_desc)
    kept = ba.use_depth, ba.use_desc
    ba.use_depth, ba.use_desc = int(use_depth), int(use_desc)
    try:
        ref, ref_count = ba.evaluate_cost()
    finally:
        ba.use_depth, ba.use_desc = kept
    t = sc.totals(planes)
    got = math.fsum(t[name] for name in sc.SUMS)
    assert ref_count > 1000
    assert t["depth_residuals"] + 2 * t["descriptor_pairs"] == ref_count
    assert abs(got - ref) <= 1e-9 * abs(ref), (got, ref)       # the bar of test_gpu_cost.py::test_total_matches_the_oracle_cost
    assert (t["depth_residuals"] > 0) == use_depth and (t["descriptor_pairs"] > 0) == use_desc
    assert all(planes[name].shape == (ba.surfels_size,) for name in sc.PLANES)


def test_the_scenes_give_the_model_real_work(loaded):
    tc, ba, words = loaded
    census = tcam.assert_scene_has_the_work(tc, ba)
    planes = sc.model(words, True, True)
    t = sc.totals(planes)
    K = len(ba.keyframes)
    assert t["depth_residuals"] == census["associated"], (t, census)
    assert t["depth_residuals"] - t["descriptor_pairs"] == census["colour_invalid"], (t, census)
    mine = sc.census(planes, K)
    # Surfels every keyframe sees and surfels with a depth term but no descriptor pair exist in both scenes.  Surfels without any
    # term: crop_small has 217 of them with all four keyframes bound; tiny has NONE (measured: every one of its 1 142 surfels is
    # associated with at least one of the four keyframes) -- there they exist with one keyframe bound (201 .. 437, depending on the
    # keyframe), which is the state the GPU tests' "one bound keyframe" case sweeps, and where the GPU tests delete surfels.
    assert mine["by_all"] > 0 and mine["depth_only"] > 0, mine
    single = [sc.census(sc.model(words[k:k + 1], True, True), 1) for k in range(K)]
    assert all(s["none"] > 0 and s["by_all"] > 0 and s["depth_only"] > 0 for s in single), single
    if tc.name == "crop_small":
        assert mine["none"] > 0, mine
    if tc.name == "tiny":
        assert ba.surfels_size == 1142 and K == 4 and t["depth_residuals"] == 3489, (ba.surfels_size, K, t)
        assert ba.surfels_size % 64 != 0 and -(-ba.surfels_size // 64) == 18       # 18 tiles, the last one partial
