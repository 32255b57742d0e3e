"""A plain model of the step control of the geometry phase (bahip_optimize_geometry_iteration_controlled; DESIGN.md section 3, "Step
control of the geometry phase") for tests/test_cpu_geometry_step_control.py, tests/test_gpu_geometry_step_control.py and
tests/test_gpu_directba_geometry_step_control.py, and the scene states they share.  A plain module: no fixtures, no conftest.

  ladder        the damping factors of the trials, in binary32;
  damped_solve  the trial solve in numpy float32, operation for operation as kernels_geometry_trial.hip spells it (numpy rounds every
                elementwise operation to binary32 and contracts nothing; division and square root are correctly rounded on both sides);
  decide        the accept / reject rule on two sets of cost planes;
  by_hand       one controlled step played through entry points that existed before it: the plain step for flags and normals,
                upload_surfels for every candidate state, evaluate_surfel_costs for c0 and every c1.  The per-surfel sums are an
                input (bahip_debug_read_geometry_sums; the lambda-0 test pins them, with damped_solve, to the plain step's words).

Scene states (tests/two_cameras.py: `tiny`, 1 142 surfels, poses perturbed, colour camera of its own):
  T0  tiny after update_surfel_activation;
  T2  T0 after two plain geometry steps of the oracle.
"""
from fractions import Fraction

import numpy as np

from tests import surfel_costs as sc
from tests import two_cameras as tcam

F32 = np.float32
DEFAULTS = dict(lambda_initial=0.0, lambda_up=4.0, lambda_min=1.0, lambda_max=1e4, max_trials=4, guard_pairs=1)
ROWS = (0, 1, 2, 6, 7)                 # x, y, z, descriptor_1, descriptor_2: the five words a geometry step may write
RESTORED = 255
STATS = ("candidates", "accepted", "restored", "rejected_cost", "rejected_pairs", "trials")


def control(**fields):
    out = dict(DEFAULTS)
    out.update(fields)
    return out


def ladder(ctl):
    """lambda_0 = lambda_initial, lambda_{t+1} = min(max(lambda_t * lambda_up, lambda_min), lambda_max), every operation in binary32."""
    up, lo, hi = F32(ctl["lambda_up"]), F32(ctl["lambda_min"]), F32(ctl["lambda_max"])
    lam, out = F32(ctl["lambda_initial"]), []
    with np.errstate(over="ignore"):
        for _ in range(int(ctl["max_trials"])):
            out.append(lam)
            lam = min(max(F32(lam * up), lo), hi)
    return out


# ---- the packed normal, as ba_device.h unpacks it ----------------------------------------------------------------------------------------
def _round_f32(value):
    """A Fraction rounded once to binary32 (nearest, ties to even)."""
    if value == 0:
        return F32(0)
    guess = F32(float(value))           # (two roundings: the neighbours are compared exactly below)
    best = None
    for c in (np.nextafter(guess, F32(-np.inf)), guess, np.nextafter(guess, F32(np.inf))):
        err = abs(Fraction(float(c)) - value)
        even = (int(np.asarray(c, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, c)
    return F32(best[1])


def _fma32(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


_NORMALS = {}


def unpack_normal10(words):
    """unpack_normal10 of ba_device.h in binary32: components s / 511 as one product with the rounded 1 / 511, the squared length as
    the chain fma(z, z, fma(y, y, x * x)), then (1 / sqrt) * component.  (3, N) float32."""
    words = np.asarray(words, np.uint32)
    out = np.zeros((3, words.size), F32)
    for j, w in enumerate(words.tolist()):
        if w not in _NORMALS:
            comps = []
            for shift in (0, 10, 20):
                v = (w >> shift) & 0x3ff
                comps.append(F32(F32(v - 1024 if v >= 512 else v) * (F32(1) / F32(511))))
            x, y, z = comps
            sq = _fma32(z, z, _fma32(y, y, F32(x * x)))
            with np.errstate(divide="ignore", invalid="ignore"):
                factor = F32(1) / np.sqrt(sq, dtype=F32)
                _NORMALS[w] = (F32(factor * x), F32(factor * y), F32(factor * z))
        out[:, j] = _NORMALS[w]
    return out


# ---- the damped solve ----------------------------------------------------------------------------------------------------------------------
def damped_solve(sums, words, normals, lam, use_desc):
    """The candidate words (5, N) uint32 of every surfel: `sums` (2 or 8, N) float32 totals, `words` (5, N) uint32 the old words in the
    order of ROWS, `normals` (3, N) float32 the unpacked normal row, `lam` the trial's damping factor."""
    sums = np.asarray(sums, F32)
    words = np.ascontiguousarray(words, np.uint32)
    old = words.view(F32)
    gp, gn, lam = old[0:3], np.asarray(normals, F32), F32(lam)
    cand = words.copy()
    eps, one80 = F32(1e-6), F32(180)
    with np.errstate(all="ignore"):
        if not use_desc:
            H, b = sums[0], sums[1]
            gate = H > eps
            damping = lam * H
            t = (F32(-1) * b) / (H + damping)
            np_ = (gp + t[None, :] * gn).astype(F32)
            cand[0:3] = np.where(gate[None, :], np_.view(np.uint32), words[0:3])
            return cand
        a0, a1, a2, a3, a5, a6, a7, a8 = sums
        d1, d2 = old[3], old[4]
        t0, t3, t5 = lam * a0, lam * a3, lam * a5
        H00, H01, H02, H11, H12, H22 = (a0 + eps) + t0, a1, a2, (a3 + eps) + t3, np.zeros_like(a0), (a5 + eps) + t5
        H00 = np.sqrt(H00)
        H01 = H01 / H00
        H11 = np.sqrt(H11 - H01 * H01)
        H02 = H02 / H00
        H12 = (H12 - H02 * H01) / H11
        H22 = np.sqrt(H22 - H02 * H02 - H12 * H12)
        y0 = a6 / H00
        y1 = (a7 - H01 * y0) / H11
        y2 = (a8 - H02 * y0 - H12 * y1) / H22
        x2 = y2 / H22
        x1 = (y1 - H12 * x2) / H11
        x0 = (y0 - H02 * x2 - H01 * x1) / H00
        np_ = (gp - x0[None, :] * gn).astype(F32)
        cand[0:3] = np.where((x0 != 0)[None, :], np_.view(np.uint32), words[0:3])
        n1 = np.fmax(-one80, np.fmin(one80, d1 - x1)).astype(F32)       # fmaxf / fminf: a NaN operand loses
        n2 = np.fmax(-one80, np.fmin(one80, d2 - x2)).astype(F32)
        cand[3] = np.where(x1 != 0, n1.view(np.uint32), words[3])
        cand[4] = np.where(x2 != 0, n2.view(np.uint32), words[4])
    assert all(v.dtype == F32 for v in (H00, H11, H22, x0, x1, x2, np_, n1, n2)), "an operation left binary32"
    return cand


# ---- the decision ----------------------------------------------------------------------------------------------------------------------------
def objective(planes):
    """f(c) = (depth + descriptor_1) + descriptor_2 in binary64."""
    return (np.asarray(planes["depth"], np.float64) + planes["descriptor_1"]) + planes["descriptor_2"]


def decide(cand, c0, c1, guard_pairs):
    """(accepted, lost_pairs) per surfel: accepted iff the five candidate words are finite, f(c1) is finite, f(c1) < f(c0) and -- under
    the guard -- neither count of c1 is below c0's; lost_pairs: the cost test passed and the guard alone rejected."""
    finite = np.isfinite(np.ascontiguousarray(cand, np.uint32).view(F32)).all(axis=0)
    f0, f1 = objective(c0), objective(c1)
    with np.errstate(invalid="ignore"):
        lower = finite & np.isfinite(f1) & (f1 < f0)
    kept = (c1["depth_residuals"] >= c0["depth_residuals"]) & (c1["descriptor_pairs"] >= c0["descriptor_pairs"])
    lost = lower & bool(guard_pairs) & ~kept
    return lower & ~lost, lost


# ---- scene states ---------------------------------------------------------------------------------------------------------------------------
_STATES = {}


def scene():
    if "tc" not in _STATES:
        _STATES["tc"] = tcam.build_scene("tiny")
    return _STATES["tc"]


def oracle_state(name, use_depth=True, use_desc=True):
    """A fresh oracle in state T0 or T2 (the caller may change it)."""
    ba = tcam.build_oracle(scene(), use_depth=use_depth, use_desc=use_desc)
    ba.update_surfel_activation()
    for _ in range({"T0": 0, "T2": 2}[name]):
        ba.optimize_geometry_iteration()
    return ba


def state_arrays(name):
    """(surfel rows (17, N) float32, flags (N,) uint8) of state T0 / T2 with both residual types; cached, do not change."""
    if name not in _STATES:
        ba = oracle_state(name)
        n = ba.surfels_size
        _STATES[name] = (ba.surfel_data[:, :n].copy(), ba.active[:n].copy())
    return _STATES[name]


def plain_step_census(ba):
    """One plain geometry step of the oracle on `ba` (left in the state after it), judged per surfel as the control would: c0 = the cost
    of the rows before the step with the normal row after it, c1 = the cost after the step.  dict(moved, lowered, raised,
    lowered_losing_a_pair)."""
    n = ba.surfels_size
    before = ba.surfel_data[:, :n].copy()
    ba.optimize_geometry_iteration()
    after = ba.surfel_data[:, :n].copy()
    ba.surfel_data[:, :n] = before
    ba.surfel_data[3, :n] = after[3]
    c0 = sc.model(sc.oracle_pair_words(ba), bool(ba.use_depth), bool(ba.use_desc))
    ba.surfel_data[:, :n] = after
    c1 = sc.model(sc.oracle_pair_words(ba), bool(ba.use_depth), bool(ba.use_desc))
    moved = (before[list(ROWS)].view(np.uint32) != after[list(ROWS)].view(np.uint32)).any(axis=0)
    f0, f1 = objective(c0), objective(c1)
    lost = (c1["depth_residuals"] < c0["depth_residuals"]) | (c1["descriptor_pairs"] < c0["descriptor_pairs"])
    return dict(moved=int(moved.sum()), lowered=int((moved & (f1 < f0)).sum()), raised=int((moved & (f1 > f0)).sum()),
                lowered_losing_a_pair=int((moved & (f1 < f0) & lost).sum()))


# ---- one controlled step by hand ------------------------------------------------------------------------------------------------------------
def plain_step(g, rows, flags, use_depth, use_desc, activation):
    """The plain step's result on (rows, flags): (rows after, flags after).  activation: None = the flags are kept."""
    g.upload_surfels(rows, flags)
    if activation is None:
        g.optimize_geometry_iteration(use_depth, use_desc)
    else:
        g.update_activation_and_optimize_geometry(use_depth, use_desc, activation)
    n = rows.shape[1]
    return g.download_surfels().copy(), g.active_buf.download()[0, :n].copy()


def by_hand(g, rows, flags, sums, ctl, use_depth=True, use_desc=True, activation=None):
    """One controlled step on the state (rows (17, N), flags) played through g's existing entry points; `sums` = the per-surfel totals of
    that state.  Returns (rows after (17, N), flags after, outcome (N,) uint8, stats dict).  Leaves g in the final state."""
    rows = np.ascontiguousarray(rows, F32)
    n = rows.shape[1]
    plain_rows, new_flags = plain_step(g, rows, flags, use_depth, use_desc, activation)
    s1 = rows.copy()
    s1[3] = plain_rows[3]                                    # S1: the pre-call rows with the post-call normal row and flags
    g.upload_surfels(s1, new_flags)
    c0 = g.evaluate_surfel_costs(use_depth, use_desc)
    saved = np.ascontiguousarray(s1[list(ROWS)]).view(np.uint32).copy()
    normals = unpack_normal10(np.ascontiguousarray(s1[3]).view(np.uint32))
    open_ = ((new_flags & 1) != 0) & ~np.isnan(s1[0])
    outcome = np.zeros(n, np.uint8)
    stats = dict.fromkeys(STATS, 0)
    current = saved.copy()                                   # the words in the rows between trials: saved, or an accepted candidate
    state = s1.copy()
    for t, lam in enumerate(ladder(ctl)):
        cand = damped_solve(sums, saved, normals, lam, use_desc)
        if t == 0:
            open_ &= (cand != saved).any(axis=0)
            stats["candidates"] = int(open_.sum())
        trial = current.copy()
        trial[:, open_] = cand[:, open_]
        state[list(ROWS)] = trial.view(F32)
        g.upload_surfels(state, new_flags)
        c1 = g.evaluate_surfel_costs(use_depth, use_desc)
        accepted, lost = decide(trial, c0, c1, ctl["guard_pairs"])
        accepted &= open_
        lost &= open_
        stats["accepted"] += int(accepted.sum())
        stats["rejected_pairs"] += int(lost.sum())
        stats["rejected_cost"] += int((open_ & ~accepted & ~lost).sum())
        stats["trials"] = t + 1
        outcome[accepted] = 1 + t
        current[:, accepted] = trial[:, accepted]
        open_ = open_ & ~accepted
        if not open_.any():
            break
    state[list(ROWS)] = current.view(F32)
    outcome[open_] = RESTORED
    stats["restored"] = int(open_.sum())
    g.upload_surfels(state, new_flags)
    return state, new_flags, outcome, stats
