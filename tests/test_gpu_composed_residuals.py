"""The HIP per-pair chain (bahip_debug_evaluate_pairs: the device functions of ba_device.h and pose_device.h that every sweep calls)
against the 60-digit goldens of tests/golden/composed_residuals.npz, in both arithmetic flavours: decisions equal to the golden,
every quantity within tests/composed_residuals.py's bound C * 2^-24 * scale -- the constants measured on the CPU from the reference's
functions and the oracle, the same for both flavours -- and, for the exact flavour, every word equal to the oracle's bits.  Reads the
committed fixture only.  326 pairs on images of at most 97x71."""
import numpy as np
import pytest

from tests import composed_residuals as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return cr.load()


def _records(fix, arithmetic):
    """Per scene: (the configurations' indices, the hook's records) with the given flavour selected."""
    from badslam_amd import lowlevel as ll
    ctx = ll.Context()
    ctx.set_arithmetic(arithmetic)
    assert ctx.arithmetic == arithmetic
    out = []
    for si in range(cr.SCENES):
        g, idx = cr.build_gpu(fix, si, ctx)
        out.append((idx, cr.gpu_records(g, fix, si)))
    return out


@pytest.fixture(scope="module")
def exact(fix):
    return _records(fix, "exact")


@pytest.fixture(scope="module")
def fast(fix):
    return _records(fix, "fast")


def test_exact_flavour_against_the_goldens(fix, exact):
    for si, (idx, got) in enumerate(exact):
        cr.check_decisions(got, fix, idx)
        cr.check_bounds(got, fix, idx, label=f"exact flavour, scene {si}:")


def test_exact_flavour_has_the_oracle_bits(fix, exact):
    for si, (idx, got) in enumerate(exact):
        ba, _ = cr.build_oracle(fix, si)
        ref = cr.oracle_records(ba, fix, si)
        same = got.view(np.uint32) == ref.view(np.uint32)
        assert same.all(), (si, np.argwhere(~same)[:10], got[~same][:10], ref[~same][:10])


def test_fast_flavour_against_the_goldens(fix, fast, exact):
    differing = 0
    for si, (idx, got) in enumerate(fast):
        cr.check_decisions(got, fix, idx)
        cr.check_bounds(got, fix, idx, label=f"fast flavour, scene {si}:")
        differing += int((got.view(np.uint32) != exact[si][1].view(np.uint32)).sum())
    print(f"fast flavour: {differing} words differ from the exact flavour's")
    assert differing > 0, "the fast flavour produced the exact flavour's bits on every word: was it selected?"


@pytest.mark.parametrize("arithmetic", ["exact", "fast"])
def test_word_3_is_the_colour_valid_decision(fix, exact, fast, arithmetic):
    seen = set()
    for idx, got in (exact if arithmetic == "exact" else fast):
        associated = fix["reason"][idx] == 0
        valid = fix["colour_valid"][idx]
        assert np.array_equal(got[associated, 3], valid[associated].astype(np.float32))
        assert not got[~associated, 3].any()
        seen |= set(valid[associated].tolist())
    assert seen == {False, True}
