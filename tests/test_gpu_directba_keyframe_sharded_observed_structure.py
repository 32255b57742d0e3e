"""DirectBA::ComputeObservedCovisibility, ComputeSurfelObservations, ComputeKeyframeRedundancy, FindRedundantKeyframes and
CullRedundantKeyframes under DirectBA::SetKeyframeSharding: two objects in lockstep on one device (the loopback of
tests/test_gpu_keyframe_sharded_intrinsics.py) against the unsharded object -- after a BundleAdjustment with surfel updates, which
the ranks run bit for bit like the unsharded object, and on the duplicated-views scene of tests/test_gpu_directba_keyframe_redundancy.py,
where find and cull must follow the unsharded sequence (the model's) on both ranks.  Equalities of integers and bit patterns."""
import numpy as np
import pytest

from badslam_amd import capi
from tests import keyframe_redundancy as kr
from tests.test_gpu_directba_cost import _build
from tests.test_gpu_directba_keyframe_redundancy import _duplicated_views
from tests.test_gpu_directba_surfel_costs import _adjust, _scene
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu


def _structure(ba):
    return dict(covisibility=ba.observed_covisibility(), lists=ba.surfel_observations(residuals=True), redundancy=ba.keyframe_redundancy(16))


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _transport(ba, hook):
    ctx = ba.backend_context()
    capi.check(ctx.lib.bahip_context_set_allreduce(ctx.handle, hook, None))


def test_the_three_results_after_a_bundle_adjustment_are_the_unsharded_objects():
    scene, start = _scene()
    ref_ba = _build(scene, start)
    _adjust(ref_ba)
    ref = _structure(ref_ba)
    assert ref["covisibility"][0] == list(range(6)) and len(ref["lists"]["keyframes"]) > 10000

    def rank_main(rank, hook):
        ba = _build(scene, start)
        _transport(ba, hook)
        ba.SetKeyframeSharding(rank, 2)
        _adjust(ba)
        return dict(got=_structure(ba), keep=(hook, ba))

    results, _ = _run_ranks(2, rank_main)
    for rank, r in enumerate(results):
        got = r["got"]
        assert got["covisibility"][0] == ref["covisibility"][0] and np.array_equal(got["covisibility"][1], ref["covisibility"][1]), rank
        assert got["redundancy"][0] == ref["redundancy"][0] and np.array_equal(got["redundancy"][1], ref["redundancy"][1]), rank
        assert got["lists"]["keyframe_ids"] == ref["lists"]["keyframe_ids"], rank
        for name in ("first", "keyframes", "depth_raw", "descriptor_raw"):
            assert np.array_equal(_words(got["lists"][name]), _words(ref["lists"][name])), (rank, name)


def test_find_and_cull_follow_the_unsharded_sequence_on_both_ranks():
    m, f = kr.CULL_RULE
    K = kr.DUPLICATED_VIEWS
    _, _, _, _, A = kr.duplicated_views()
    rules = ((m, f), (3, 0.9), (9, 0.65))
    expected, by_rule = kr.cull(A, m, f, K, 1)
    assert len(expected) >= 2 and by_rule
    left = [k for k in range(K) if k not in expected]

    def rank_main(rank, hook):
        ba, _ = _duplicated_views()
        _transport(ba, hook)
        ba.SetKeyframeSharding(rank, 2)
        out = dict(table=ba.keyframe_redundancy(), found=[ba.find_redundant_keyframes(*rule) for rule in rules])
        out["first_two"] = ba.cull_redundant_keyframes(m, f, 2, protect_newest=1)
        out["after_two"] = ba.keyframe_redundancy()[0]
        out["rest"] = ba.cull_redundant_keyframes(m, f, K, protect_newest=1)
        out["end"] = ba.keyframe_redundancy()
        out["keep"] = (hook, ba)
        return out

    results, _ = _run_ranks(2, rank_main)
    for rank, r in enumerate(results):
        assert r["table"][0] == list(range(K)) and np.array_equal(r["table"][1].astype(np.int64), kr.table(A, 16)), rank
        assert r["found"] == [kr.find(kr.table(A, 16), *rule) for rule in rules], rank
        assert r["first_two"] == expected[:2] and r["after_two"] == [k for k in range(K) if k not in expected[:2]], rank
        assert r["rest"] == expected[2:], rank
        assert r["end"][0] == left and np.array_equal(r["end"][1].astype(np.int64), kr.table(A[left], 16)), rank
