"""The intrinsics step of the alternating scheme under step control on the GPU (bahip_optimize_intrinsics_controlled;
kernels_intrinsics_trial.hip, DESIGN.md section 3, "Step control of the intrinsics step").

Held to: the plain step and the oracle at lambda 0; the binary32 model of the damped solve (tests/intrinsics_step_control.py) on the
read-back sums; a controlled step played by hand through entry points that existed before, word for word; the property the control
exists for -- no accepted step raises the objective; and the bits a rejected step must put back.  The states: state R (crop_small after
4 plain steps: the plain step raises the cost, lambda = 1 lowers it) and state H (small21 after 9 plain steps: no rung of the default
ladder lowers it) -- tests/test_cpu_intrinsics_step_control.py asserts that they are what they are called."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import capi, multigpu
from tests import intrinsics_step_control as isc
from tests.test_cpu_intrinsics_step_control import STATE_H, STATE_R
from tests.test_gpu_keyframe_sharded_intrinsics import _run_ranks

pytestmark = pytest.mark.gpu

DEPTH_OFFSET = (0.5, -0.6, 1.23, -2.17)   # the perturbed cameras of tests/test_gpu_intrinsics_pcg_vs_oracle.py


def _bits(values):
    return np.ascontiguousarray(np.asarray(values, np.float32)).view(np.uint32)


def _pair(name, steps=0, offset=None):
    """(oracle, GPU scene) in the same state: the scene `name` after `steps` plain steps [and the depth camera moved by `offset`]."""
    ba = isc.build_oracle(name, steps)
    if offset is not None:
        cam = ba.depth_cam
        cam.fx += offset[0]; cam.fy += offset[1]; cam.cx += offset[2]; cam.cy += offset[3]
    return ba, isc.build_gpu(name, ba)


def _same_state(a, b, what=""):
    for key in ("depth_cam", "color_cam", "a", "cfactor"):
        assert np.array_equal(_bits(a[key]).ravel(), _bits(b[key]).ravel()), (what, key)


def _same_result(got, want, what=""):
    for key in ("accepted", "trials", "lambda_accepted", "lam", "cost_before", "cost_after"):
        assert got[key] == want[key], (what, key, got[key], want[key])


def _result_state(g, res):
    """The state a controlled call reports (out_* arguments) and leaves (the plane)."""
    return dict(depth_cam=res["depth_camera"], color_cam=res["color_camera"], a=res["a"], cfactor=g.cfactor.download())


def _plane_with_padding(g):
    """Every byte of the cfactor plane's rows, pitch padding included."""
    buf = g.cfactor
    out = np.empty((buf.height, buf.pitch), np.uint8)
    capi.check(g.ctx.lib.bahip_memcpy_2d(g.ctx.handle, out.ctypes.data, buf.pitch, buf.ptr, buf.pitch, buf.pitch, buf.height, 2))
    return out


def _fill_padding(g, byte=0xEE):
    """Fills the whole pitched allocation with `byte` and puts the plane back: a write into the padding shows."""
    buf = g.cfactor
    plane = buf.download()
    capi.check(g.ctx.lib.bahip_memset_2d(g.ctx.handle, buf.ptr, buf.pitch, byte, buf.pitch, buf.height))
    buf.upload(plane)
    assert buf.pitch > buf.width * 4, "the plane has no padding to watch"


@pytest.fixture(params=[0, 1], ids=["records added by LDS f64 atomics", "records sorted by cell in LDS"])
def reduce_form(request):
    lib = capi.load()
    capi.check(lib.bahip_debug_set_intrinsics_reduce_form(request.param))
    yield request.param
    capi.check(lib.bahip_debug_set_intrinsics_reduce_form(-1))


# ---- (1) lambda = 0 accepted: the plain step ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", [("tiny", None), ("small21", DEPTH_OFFSET)])
def test_lambda_zero_accepted_is_the_plain_step_and_the_oracles(name, offset, reduce_form):
    ba, g = _pair(name, 0, offset)
    _, twin = _pair(name, 0, offset)
    want_before, _ = g.evaluate_cost(per_keyframe=False)
    _fill_padding(g)
    padding_before = _plane_with_padding(g)[:, g.cfactor.width * 4:].copy()
    res = g.optimize_intrinsics_controlled(0.0)
    assert res["accepted"] and res["trials"] == 1 and res["lambda_accepted"] == 0.0 and res["lam"] == 0.0
    assert res["cost_before"] == want_before
    assert res["cost_after"] == g.evaluate_cost(per_keyframe=False)[0]          # (the context kept the new intrinsics)
    assert isc.objective(res["cost_after"]) < isc.objective(res["cost_before"])
    assert np.array_equal(_plane_with_padding(g)[:, g.cfactor.width * 4:], padding_before)
    # the plain call on a twin scene
    cc, dc, a = twin.optimize_intrinsics(True, True)
    got = _result_state(g, res)
    _same_state(got, dict(depth_cam=isc.camera_of(dc), color_cam=isc.camera_of(cc), a=a, cfactor=twin.cfactor.download()), "plain call")
    # the oracle
    occ, odc, oa = ba.optimize_intrinsics(True, True)
    _same_state(got, dict(depth_cam=isc.camera_of(odc), color_cam=isc.camera_of(occ), a=oa, cfactor=ba.cfactor), "oracle")
    _same_state(got, isc.gpu_state(g), "the scene adopted what the call reports")


# ---- (2) the damped solve ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_the_damped_solve_is_the_model_on_the_read_back_sums(name):
    _, g = _pair(name)
    glob, cells = isc.gpu_sums(g)
    assert cells.shape[0] % 64 != 0 or name != "tiny"
    at = isc.gpu_state(g)
    for lam in (0.0, 1.0, 4.0, 16.0, 1e4):
        x1, xc, table = g.intrinsics_solve_damped(lam)
        want = isc.damped_step(glob, cells, lam, at["depth_cam"], at["color_cam"], at["a"], at["cfactor"])
        assert np.array_equal(_bits(x1), _bits(want["x1"])), (lam, x1, want["x1"])
        assert np.array_equal(_bits(xc), _bits(want["xc"])), (lam, xc, want["xc"])
        assert np.array_equal(_bits(table), _bits(want["cells_after"])), lam
        assert np.any(x1 != 0) and np.any(xc != 0)
    _same_state(isc.gpu_state(g), at, "nothing is applied")
    # one system only: the other's update is zeros, and the table exists with the depth intrinsics only
    x1, xc, table = g.intrinsics_solve_damped(4.0, optimize_depth=False)
    assert not np.any(x1) and table is None and np.array_equal(_bits(xc), _bits(isc.solve_color(glob, 4.0)))


# ---- (3) state R: the call is the by-hand sequence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_state_r_the_call_is_the_by_hand_sequence(flavour):
    name, steps = STATE_R
    _, g = _pair(name, steps)
    _, hand = _pair(name, steps)
    for scene in (g, hand):
        scene.ctx.set_arithmetic(flavour)
    want = isc.gpu_controlled_step_by_hand(hand, 0.0)
    res = g.optimize_intrinsics_controlled(0.0)
    _same_result(res, want, flavour)
    _same_state(_result_state(g, res), want["state"], flavour)
    assert isc.objective(res["cost_after"]) <= isc.objective(res["cost_before"])
    if flavour == "exact":   # what the census says of this state: the plain step is rejected, lambda = 1 accepted
        assert res["accepted"] and res["trials"] == 2 and res["lambda_accepted"] == 1.0 and res["lam"] == 0.0
        plain = _pair(name, steps)[1]
        before = isc.objective(plain.evaluate_cost(per_keyframe=False)[0])
        plain.optimize_intrinsics(True, True)
        assert isc.objective(plain.evaluate_cost(per_keyframe=False)[0]) > before


# ---- (4) state H: nothing is accepted, every bit is back ---------------------------------------------------------------------------
def test_state_h_nothing_is_accepted_and_every_bit_is_back():
    name, steps = STATE_H
    _, g = _pair(name, steps)
    _fill_padding(g)
    before_state, before_plane = isc.gpu_state(g), _plane_with_padding(g)
    res = g.optimize_intrinsics_controlled(0.0)
    assert not res["accepted"] and res["trials"] == 4 and res["lambda_accepted"] == 0.0
    assert res["lam"] == float(isc.up(isc.DEFAULTS, isc.rungs(isc.DEFAULTS, 0.0)[-1])) == 64.0
    assert res["cost_after"] == res["cost_before"] == g.evaluate_cost(per_keyframe=False)[0]
    assert np.array_equal(_plane_with_padding(g), before_plane)
    _same_state(_result_state(g, res), before_state, "the out_* arguments are the context's unchanged values")
    _same_state(isc.gpu_state(g), before_state)


# ---- (5) a rejection that does not depend on the census -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "crop_small"])
def test_a_nan_descriptor_rejects_every_trial_and_every_bit_is_back(name):
    _, g = _pair(name)
    data = g.download_surfels()
    data[6, data.shape[1] // 2] = np.nan
    g.upload_surfels(data, g.active_buf.download().ravel()[:data.shape[1]].copy())
    _fill_padding(g)
    before_state, before_plane = isc.gpu_state(g), _plane_with_padding(g)
    res = g.optimize_intrinsics_controlled(0.0)
    assert not np.isfinite(isc.objective(res["cost_before"]))
    assert not res["accepted"] and res["trials"] == 4 and res["lam"] == 64.0
    assert np.array_equal(_plane_with_padding(g), before_plane)
    _same_state(_result_state(g, res), before_state)
    after = g.evaluate_cost(per_keyframe=False)[0]
    assert after["depth_residuals"] == res["cost_before"]["depth_residuals"] and after["descriptor_pairs"] == res["cost_before"]["descriptor_pairs"]
    assert not np.isfinite(isc.objective(after))


# ---- (6) the property ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["exact", "fast"])
@pytest.mark.parametrize("name", ["crop_small", "small21"])
def test_no_accepted_step_raises_the_objective(name, flavour):
    _, g = _pair(name)
    _, plain = _pair(name)
    for scene in (g, plain):
        scene.ctx.set_arithmetic(flavour)
    lam, cost, accepted, struct = 0.0, isc.objective(g.evaluate_cost(per_keyframe=False)[0]), 0, None
    for step in range(8):
        res = g.optimize_intrinsics_controlled(lam, cost_before=struct)
        assert isc.objective(res["cost_before"]) == cost, step
        if res["accepted"]:
            assert isc.objective(res["cost_after"]) < cost, (step, res)
            accepted += 1
        else:
            assert res["cost_after"] == res["cost_before"]
        assert res["cost_after"] == g.evaluate_cost(per_keyframe=False)[0], step
        lam, cost, struct = res["lam"], isc.objective(res["cost_after"]), res["cost_after_struct"]
        plain.optimize_intrinsics(True, True)
    assert accepted >= 4
    print(name, flavour, "controlled", cost, "plain", isc.objective(plain.evaluate_cost(per_keyframe=False)[0]))
    if name == "crop_small":
        assert cost <= isc.objective(plain.evaluate_cost(per_keyframe=False)[0])


# ---- (7) edges ----------------------------------------------------------------------------------------------------------------------------
def test_max_trials_one_and_a_start_at_lambda_max():
    name, steps = STATE_R
    _, g = _pair(name, steps)
    before = isc.gpu_state(g)
    res = g.optimize_intrinsics_controlled(0.0, control=dict(max_trials=1))
    assert not res["accepted"] and res["trials"] == 1 and res["lam"] == 1.0
    _same_state(isc.gpu_state(g), before)
    # at lambda_max: one trial; rejected, the ladder ends there and lambda stays; accepted, lambda goes down one rung
    _, hand = _pair(name, steps)
    for c in (dict(lambda_max=4.0), dict(lambda_max=4.0, max_trials=1)):
        want = isc.gpu_controlled_step_by_hand(hand, 4.0, isc.control(**c))
        res = g.optimize_intrinsics_controlled(4.0, control=c)
        assert res["trials"] == 1
        _same_result(res, want, c)
        _same_state(isc.gpu_state(g), want["state"], c)
    _, h = _pair(*STATE_H)
    res = h.optimize_intrinsics_controlled(16.0, control=dict(lambda_max=16.0))
    assert not res["accepted"] and res["trials"] == 1 and res["lam"] == 16.0


@pytest.mark.parametrize("optimize_depth,optimize_color", [(True, False), (False, True)], ids=["depth", "colour"])
def test_one_block_only_is_the_by_hand_sequence_and_leaves_the_other_alone(optimize_depth, optimize_color):
    name, steps = STATE_R
    _, g = _pair(name, steps)
    _, hand = _pair(name, steps)
    before = isc.gpu_state(g)
    for lam in (0.0, 4.0):
        want = isc.gpu_controlled_step_by_hand(hand, lam, None, optimize_depth, optimize_color)
        res = g.optimize_intrinsics_controlled(lam, optimize_depth, optimize_color)
        _same_result(res, want, lam)
        _same_state(_result_state(g, res), want["state"], lam)
    after = isc.gpu_state(g)
    for key in (("color_cam",) if optimize_depth else ("depth_cam", "a", "cfactor")):
        assert np.array_equal(_bits(after[key]), _bits(before[key])), key


def test_no_surfels_and_no_keyframes_run_no_trial():
    _, g = _pair("tiny")
    before = isc.gpu_state(g)
    data = g.download_surfels()
    flags = g.active_buf.download().ravel()[:data.shape[1]].copy()
    g.upload_surfels(data[:, :0], flags[:0])
    res = g.optimize_intrinsics_controlled(4.0)
    assert not res["accepted"] and res["trials"] == 0 and res["lam"] == 4.0 and res["cost_after"] == res["cost_before"]
    _same_state(_result_state(g, res), before)
    g.upload_surfels(data, flags)
    kept, g.keyframes = g.keyframes, []
    g.bind_keyframes()
    res = g.optimize_intrinsics_controlled(4.0)
    assert not res["accepted"] and res["trials"] == 0 and res["lam"] == 4.0 and res["cost_before"]["depth_residuals"] == 0
    _same_state(_result_state(g, res), before)
    g.keyframes = kept
    g.bind_keyframes()
    assert g.optimize_intrinsics_controlled(0.0)["accepted"]


def test_bad_control_blocks_are_refused_and_the_context_stays_usable():
    _, g = _pair("tiny")
    before = isc.gpu_state(g)
    for bad in (dict(lambda_first=0.0), dict(lambda_first=-1.0), dict(lambda_up=1.0), dict(lambda_first=2.0, lambda_max=1.0),
                dict(lambda_first=float("nan")), dict(lambda_up=float("inf")), dict(lambda_max=float("inf")), dict(max_trials=0)):
        assert not isc.control_ok(isc.control(**bad))
        with pytest.raises(capi.BackendError):
            g.optimize_intrinsics_controlled(0.0, control=bad)
        assert g.ctx.lib.bahip_last_error()
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(capi.BackendError):
            g.optimize_intrinsics_controlled(lam)
    with pytest.raises(capi.BackendError):
        g.optimize_intrinsics_controlled(0.0, optimize_depth=False, optimize_color=False)
    _same_state(isc.gpu_state(g), before)
    assert g.optimize_intrinsics_controlled(0.0)["accepted"]


def test_a_given_cost_before_is_taken_as_it_is():
    name, steps = STATE_R
    _, g = _pair(name, steps)
    _, twin = _pair(name, steps)
    want = twin.optimize_intrinsics_controlled(0.0)
    given = capi.Cost()
    for key, value in want["cost_before"].items():
        setattr(given, key, value)
    res = g.optimize_intrinsics_controlled(0.0, cost_before=given)
    _same_result(res, want)
    # a caller's cost below every trial's: the call believes it and rejects them all
    given.depth, given.descriptor_1, given.descriptor_2 = 1.0, 0.0, 0.0
    _, h = _pair(name, steps)
    res = h.optimize_intrinsics_controlled(0.0, cost_before=given)
    assert not res["accepted"] and res["trials"] == 4 and res["cost_before"]["depth"] == 1.0 and res["cost_after"] == res["cost_before"]


def test_forced_slices_and_no_record_buffers_give_the_same_bits():
    name, steps = STATE_R
    _, ref = _pair(name, steps)
    want = ref.optimize_intrinsics_controlled(0.0)
    want_state = isc.gpu_state(ref)
    for slices, capacity in ((2, -1), (0, 0), (2, 0)):
        _, g = _pair(name, steps)
        capi.check(g.ctx.lib.bahip_debug_set_intrinsics_slices(g.ctx.handle, slices))
        capi.check(g.ctx.lib.bahip_debug_set_intrinsics_bin_capacity(g.ctx.handle, capacity))
        res = g.optimize_intrinsics_controlled(0.0)
        _same_result(res, want, (slices, capacity))
        _same_state(isc.gpu_state(g), want_state, (slices, capacity))


# ---- (8) sharding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,empty", [(2, False), (3, True)])
def test_surfel_shards_take_one_gpus_decisions_and_end_with_its_bits(world, empty):
    name, steps = STATE_R
    ba, ref = _pair(name, steps)
    want = ref.optimize_intrinsics_controlled(0.0)
    want_state = isc.gpu_state(ref)
    n = ba.surfels_size

    def rank_main(rank, hook):
        gr = isc.build_gpu(name, ba)
        data = gr.download_surfels()
        flags = gr.active_buf.download().ravel()[:n].copy()
        if empty:     # the last rank has nothing; the others share the cloud
            mine = np.arange(0) if rank == world - 1 else multigpu.shard_chunks(n, rank, world - 1, chunk=64)
        else:
            mine = multigpu.shard_chunks(n, rank, world, chunk=64)
        gr.upload_surfels(np.ascontiguousarray(data[:, mine]), flags[mine])
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        res = gr.optimize_intrinsics_controlled(0.0)
        res.update(state=isc.gpu_state(gr), keep=(hook, gr), size=int(mine.size))
        return res

    results, loop = _run_ranks(world, rank_main)
    assert sum(r["size"] for r in results) == n and (not empty or results[-1]["size"] == 0)
    for rank, r in enumerate(results):
        _same_result(r, want, rank)
        _same_state(r["state"], want_state, rank)
    assert loop.calls == 1 + 1 + want["trials"]     # the cost before, the sums, one cost per trial


def test_keyframe_shards_end_with_the_unsharded_bits():
    name, steps = STATE_R
    world, classes = 2, 2
    ba, ref = _pair(name, steps)
    ref.set_intrinsics_sum_classes(classes)
    want = ref.optimize_intrinsics_controlled(0.0)
    want_state = isc.gpu_state(ref)

    def rank_main(rank, hook):
        gr = isc.build_gpu(name, ba)
        gr.set_intrinsics_sum_classes(classes)
        capi.check(gr.ctx.lib.bahip_context_set_allreduce(gr.ctx.handle, hook, None))
        gr.set_keyframe_sharding(rank, world)
        gr.bind_keyframes()
        res = gr.optimize_intrinsics_controlled(0.0)
        res.update(state=isc.gpu_state(gr), keep=(hook, gr))
        return res

    results, loop = _run_ranks(world, rank_main)
    for rank, r in enumerate(results):
        _same_result(r, want, rank)
        _same_state(r["state"], want_state, rank)
    assert want["accepted"] and want["trials"] == 2 and loop.calls == 1 + 1 + want["trials"]


@pytest.mark.parametrize("fail_at", [0, 1, 2, 3])
def test_a_failing_exchange_fails_the_call_restores_the_state_and_the_next_call_succeeds(fail_at):
    """Exchanges of a call on state R with a transport (a lone rank whose own words are the sum): 0 carries the cost before, 1 the sums, 2 and 3 the costs of the trials at lambda 0 and
    1 -- inside the loop, where a candidate is in the plane and in the context when the exchange fails."""
    name, steps = STATE_R
    _, g = _pair(name, steps)
    _, ref = _pair(name, steps)
    want = ref.optimize_intrinsics_controlled(0.0)
    calls = []

    def hook(buf, count, dtype, stream, user):                     # a lone rank of two: its own words are the sum
        calls.append(count)
        return 1 if len(calls) - 1 == fail_at else 0

    failing = capi.ALLREDUCE_FN(hook)
    capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, failing, None))
    _fill_padding(g)
    before_plane = _plane_with_padding(g)
    try:
        with pytest.raises(capi.BackendError):
            g.optimize_intrinsics_controlled(0.0)
        assert len(calls) == fail_at + 1
        assert np.array_equal(_plane_with_padding(g), before_plane), "the plane is back"
    finally:
        capi.check(g.ctx.lib.bahip_context_set_allreduce(g.ctx.handle, C.cast(None, capi.ALLREDUCE_FN), None))
    # the context's intrinsics are back too: the next call finds the state of before and gives the call's result
    res = g.optimize_intrinsics_controlled(0.0)
    assert res["cost_before"] == want["cost_before"] and want["trials"] == 2
    _same_result(res, want, "after the failed call")
    _same_state(isc.gpu_state(g), isc.gpu_state(ref), "after the failed call")
