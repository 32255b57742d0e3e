"""Step control of the intrinsics step: the definition of include/badslam_hip.h (bahip_optimize_intrinsics_controlled) restated in numpy
binary32 / Python binary64, operation for operation, plus a controlled step played by hand -- on the oracle, and on the GPU through the
older entry points.  A plain module: tests/test_cpu_intrinsics_step_control.py pins it to the oracle at lambda = 0 and takes the census
of states the GPU tests stand on; tests/test_gpu_intrinsics_step_control.py holds the library to it."""
import math

import numpy as np

f32 = np.float32
DEFAULTS = dict(lambda_first=1.0, lambda_up=4.0, lambda_max=1e4, max_trials=4)


# ---- the ladder and the accept rule --------------------------------------------------------------------------------------------
def control(**fields):
    out = dict(DEFAULTS)
    out.update(fields)
    return out


def control_ok(c):
    """The argument checks of bahip_intrinsics_step_control."""
    first, up, top = float(c["lambda_first"]), float(c["lambda_up"]), float(c["lambda_max"])
    return (all(math.isfinite(v) for v in (first, up, top)) and first > 0 and up > 1 and first <= top and int(c["max_trials"]) >= 1)


def up(c, lam):
    lam = f32(lam)
    if lam == 0:
        return f32(c["lambda_first"])
    return min(f32(lam * f32(c["lambda_up"])), f32(c["lambda_max"]))


def down(c, lam):
    t = f32(f32(lam) / f32(c["lambda_up"]))
    return f32(0) if t < f32(c["lambda_first"]) else t


def rungs(c, lam):
    """The damping factors a call starting at `lam` tries at most: it stops after max_trials, or after a rejection at lambda_max."""
    out = [f32(lam)]
    while len(out) < int(c["max_trials"]) and out[-1] < f32(c["lambda_max"]):
        out.append(up(c, out[-1]))
    return out


def objective(cost):
    """f(c) = (depth + descriptor_1) + descriptor_2 in binary64 of a cost dict (lowlevel.cost_dict)."""
    return (float(cost["depth"]) + float(cost["descriptor_1"])) + float(cost["descriptor_2"])


def accepts(f_before, f_after):
    return math.isfinite(f_after) and f_after < f_before


# ---- the damped solve -----------------------------------------------------------------------------------------------------------
def wave_xor_sum(values):
    """The xor butterfly (32, 16, 8, 4, 2, 1) over the 64 lanes of every row of `values` (G, 64) in binary32: (G,)."""
    v = np.asarray(values, f32)
    lanes = np.arange(64)
    for stride in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ stride]
    return v[:, 0]


def damped_schur(glob, cells, lam):
    """The damped Schur complement from the binary32-rounded sums (glob[34], cells[S, 8] = B0..B4, D, b2, observation count):
    (glob_after[34], cells_after[S, 8]) as the damped Schur kernel and intrinsics_finish_kernel leave them."""
    glob, cells = np.asarray(glob, f32), np.asarray(cells, f32)
    S = cells.shape[0]
    lam = f32(lam)
    B, D, b2 = cells[:, :5], cells[:, 5], cells[:, 6]
    with np.errstate(all="ignore"):
        scaled = lam * D                      # one product ...
        damped = D + scaled                   # ... one add
        D_inverse = f32(1) / damped
        ok = D_inverse < f32(1e12)
        D_inv_b2 = D_inverse * b2
        padded = (S + 63) // 64 * 64
        part = np.zeros((padded, 20), f32)
        q = 0
        for row in range(5):
            for col in range(row, 5):
                part[:S, q] = np.where(ok, f32(-1) * ((B[:, row] * D_inverse) * B[:, col]), f32(0))
                q += 1
        for c in range(5):
            part[:S, 15 + c] = np.where(ok, f32(-1) * (B[:, c] * D_inv_b2), f32(0))
        after = cells.copy()
        after[:, :5] = np.where(ok[:, None], D_inverse[:, None] * B, B)
        after[:, 5] = np.where(ok, D_inv_b2, f32(np.nan))
        total = np.zeros(20, f32)
        waves = np.stack([wave_xor_sum(part[:, q].reshape(-1, 64)) for q in range(20)], axis=1)   # (wavefronts, 20)
        for w in range(waves.shape[0]):       # the ordered chain of wavefront partials, from 0
            total = total + waves[w]
        out = glob.copy()
        out[:20] = glob[:20] + total
    return out, after


def ldlt_solve_sym(n, A, b):
    """csrc/ldlt.h in Python floats: LDL^T with symmetric diagonal pivoting and the pseudo-inverse rule on D."""
    A = [float(v) for v in A]
    perm = list(range(n))
    tiny = 2.2250738585072014e-308
    for k in range(n):
        piv, best = k, abs(A[k * n + k])
        for c in range(k + 1, n):
            if abs(A[c * n + c]) > best:
                best, piv = abs(A[c * n + c]), c
        if piv != k:
            for j in range(n):
                A[k * n + j], A[piv * n + j] = A[piv * n + j], A[k * n + j]
            for j in range(n):
                A[j * n + k], A[j * n + piv] = A[j * n + piv], A[j * n + k]
            perm[k], perm[piv] = perm[piv], perm[k]
        d = A[k * n + k]
        if abs(d) > tiny:
            for c in range(k + 1, n):
                A[c * n + k] /= d
            for c in range(k + 1, n):
                for j in range(k + 1, c + 1):
                    A[c * n + j] -= A[c * n + k] * d * A[j * n + k]
                    A[j * n + c] = A[c * n + j]
        else:
            for c in range(k + 1, n):
                A[c * n + k] = 0.0
    y = [float(b[perm[c]]) for c in range(n)]
    for c in range(n):
        for j in range(c):
            y[c] -= A[c * n + j] * y[j]
    for c in range(n):
        d = A[c * n + c]
        y[c] = y[c] / d if abs(d) > tiny else 0.0
    for c in range(n - 1, -1, -1):
        for j in range(c + 1, n):
            y[c] -= A[j * n + c] * y[j]
    x = [0.0] * n
    for c in range(n):
        x[perm[c]] = y[c]
    return x


def _symmetric(n, upper):
    M = [0.0] * (n * n)
    q = 0
    for row in range(n):
        for col in range(row, n):
            M[row * n + col] = M[col * n + row] = float(upper[q])
            q += 1
    return M


def solve_depth(glob_after, a, lam):
    """x1[5] (binary32) of the reduced system: the prior on a in binary32, then M_ii + (double)lambda * M_ii, then the LDL^T solve."""
    g = np.asarray(glob_after, f32)
    M = _symmetric(5, g[:15])
    rhs = [float(v) for v in g[15:20]]
    M[24] = float(f32(f32(M[24]) + f32(10) * f32(10)))
    rhs[4] = float(f32(f32(rhs[4]) + f32(f32(10) * f32(10)) * f32(a)))
    for i in range(5):
        M[i * 5 + i] = M[i * 5 + i] + float(f32(lam)) * M[i * 5 + i]
    return np.array(ldlt_solve_sym(5, M, rhs), np.float64).astype(f32)


def solve_color(glob, lam):
    g = np.asarray(glob, f32)
    M = _symmetric(4, g[20:30])
    for i in range(4):
        M[i * 4 + i] = M[i * 4 + i] + float(f32(lam)) * M[i * 4 + i]
    return np.array(ldlt_solve_sym(4, M, [float(v) for v in g[30:34]]), np.float64).astype(f32)


def update_depth_camera(depth_cam, a, x1):
    """(fx, fy, cx, cy), a after the update x1, in binary32 (the unprojection form of the plain step)."""
    fx, fy, cx, cy = (f32(v) for v in depth_cam)
    with np.errstate(all="ignore"):
        fx_inv, fy_inv = f32(1) / fx, f32(1) / fy
        cx_inv, cy_inv = -(cx - f32(0.5)) * fx_inv, -(cy - f32(0.5)) * fy_inv
        new_fx = f32(1) / (fx_inv - x1[0])
        new_fy = f32(1) / (fy_inv - x1[1])
        new_cx = -(new_fx * (cx_inv - x1[2])) + f32(0.5)
        new_cy = -(new_fy * (cy_inv - x1[3])) + f32(0.5)
        return np.array([new_fx, new_fy, new_cx, new_cy], f32), f32(f32(a) - x1[4])


def back_substitute(cells_after, x1, cfactor):
    """cfactor (S,) - (D'^-1 b2 - sum_c D'^-1 B_c x_c), zero where the observation count is 0."""
    cells_after, cfactor = np.asarray(cells_after, f32), np.asarray(cfactor, f32).reshape(-1)
    with np.errstate(all="ignore"):
        offset = cells_after[:, 5].copy()
        for c in range(5):
            offset = offset - cells_after[:, c] * f32(x1[c])
        offset = np.where(np.isnan(cells_after[:, 5]), f32(0), offset)
        value = cfactor - offset
    return np.where(cells_after[:, 7] == 0, f32(0), value).astype(f32)


def damped_step(glob, cells, lam, depth_cam, color_cam, a, cfactor, optimize_depth=True, optimize_color=True):
    """One damped step from the rounded sums at the intrinsics given: dict(x1, xc, depth_cam, color_cam, a, cfactor (S,), cells_after)."""
    out = dict(x1=np.zeros(5, f32), xc=np.zeros(4, f32), depth_cam=np.asarray(depth_cam, f32).copy(), color_cam=np.asarray(color_cam, f32).copy(),
               a=f32(a), cfactor=np.asarray(cfactor, f32).reshape(-1).copy(), cells_after=None)
    if optimize_depth:
        glob_after, out["cells_after"] = damped_schur(glob, cells, lam)
        out["x1"] = solve_depth(glob_after, a, lam)
        out["depth_cam"], out["a"] = update_depth_camera(depth_cam, a, out["x1"])
        out["cfactor"] = back_substitute(out["cells_after"], out["x1"], cfactor)
    if optimize_color:
        out["xc"] = solve_color(glob, lam)
        out["color_cam"] = (np.asarray(color_cam, f32) - out["xc"]).astype(f32)
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
_SCENES, _STATES = {}, {}


def scene(name):
    """"small21" = common.small_scene(num_keyframes=5, seed=21) with the cameras at ground truth, else the scene `name` of
    tests/two_cameras.py (in its perturbed state)."""
    from tests import common, two_cameras
    if name not in _SCENES:
        _SCENES[name] = common.small_scene(num_keyframes=5, seed=21) if name == "small21" else two_cameras.build_scene(name)
    return _SCENES[name]


def build_oracle(name, plain_steps=0):
    """The oracle of the scene after `plain_steps` plain intrinsics steps (depth and colour); the state after the steps is kept, so a
    second oracle of the same state costs its construction only."""
    from tests import common, two_cameras
    ba = common.build_oracle(scene(name), 400000) if name == "small21" else two_cameras.build_oracle(scene(name))
    if plain_steps:
        if (name, plain_steps) not in _STATES:
            for _ in range(plain_steps):
                ba.optimize_intrinsics(True, True)
            _STATES[(name, plain_steps)] = oracle_state(ba)
        oracle_put(ba, _STATES[(name, plain_steps)])
    return ba


def build_gpu(name, ba, ctx=None):
    """A GPU scene with the oracle's state: surfels, flags, poses, cameras, a, cfactor image; keyframes bound."""
    from tests import common, two_cameras
    if name == "small21":
        return two_cameras.sync_gpu(common.build_gpu(scene(name), 400000, create_from=[], ctx=ctx), ba)
    return two_cameras.build_gpu(scene(name), ba, ctx=ctx)


# ---- on the oracle ----------------------------------------------------------------------------------------------------------------
def camera_of(cam):
    return np.array([cam.fx, cam.fy, cam.cx, cam.cy], f32)


def put_camera(cam, values):
    cam.fx, cam.fy, cam.cx, cam.cy = (float(v) for v in values)


def oracle_state(ba):
    return dict(depth_cam=camera_of(ba.depth_cam), color_cam=camera_of(ba.color_cam), a=f32(ba.dp.a), cfactor=ba.cfactor.copy())


def oracle_put(ba, state):
    put_camera(ba.depth_cam, state["depth_cam"])
    put_camera(ba.color_cam, state["color_cam"])
    ba.dp.a = float(state["a"])
    ba.cfactor[...] = np.asarray(state["cfactor"], f32).reshape(ba.cfactor.shape)


def oracle_sums(ba, optimize_depth=True, optimize_color=True):
    glob, cells = ba.intrinsics_accumulators(optimize_depth, optimize_color)
    return glob.astype(f32), cells.astype(f32)


def oracle_trial(ba, sums, saved, lam, optimize_depth=True, optimize_color=True):
    """Puts the damped step at `lam` from the saved state into the oracle and returns (its cost, the step)."""
    step = damped_step(sums[0], sums[1], lam, saved["depth_cam"], saved["color_cam"], saved["a"], saved["cfactor"], optimize_depth, optimize_color)
    oracle_put(ba, step)
    return ba.evaluate_cost()[0], step


def oracle_controlled_step(ba, lam, c=None, optimize_depth=True, optimize_color=True):
    """A controlled step on the oracle with the model: dict(accepted, trials, lambda_accepted, lam, cost_before, cost_after, costs)."""
    c = c or DEFAULTS
    before = ba.evaluate_cost()[0]
    sums, saved = oracle_sums(ba, optimize_depth, optimize_color), oracle_state(ba)
    costs = []
    for trial, rung in enumerate(rungs(c, lam), 1):
        cost, _ = oracle_trial(ba, sums, saved, rung, optimize_depth, optimize_color)
        costs.append((float(rung), cost))
        if accepts(before, cost):
            return dict(accepted=True, trials=trial, lambda_accepted=float(rung), lam=float(down(c, rung)), cost_before=before, cost_after=cost, costs=costs)
        oracle_put(ba, saved)
    return dict(accepted=False, trials=len(costs), lambda_accepted=0.0, lam=float(up(c, costs[-1][0])), cost_before=before, cost_after=before,
                costs=costs)


# ---- on the GPU, by hand through the older entry points ------------------------------------------------------------------------------
def gpu_state(g):
    return dict(depth_cam=camera_of(g.depth_cam), color_cam=camera_of(g.color_cam), a=f32(g.dp.a), cfactor=g.cfactor.download().copy())


def gpu_put(g, state):
    put_camera(g.depth_cam, state["depth_cam"])
    put_camera(g.color_cam, state["color_cam"])
    g.dp.a = float(state["a"])
    g.cfactor.upload(np.asarray(state["cfactor"], f32).reshape(g.cf_h, g.cf_w))
    g.set_intrinsics()


def gpu_sums(g, optimize_depth=True, optimize_color=True):
    """The rounded sums of the current state: the plain step (which overwrites the cfactor plane: put back here), then the debug read."""
    saved = gpu_state(g)
    g.optimize_intrinsics(optimize_depth, optimize_color, apply=False)
    gpu_put(g, saved)
    return g.read_intrinsics_sums(True)


def gpu_controlled_step_by_hand(g, lam, c=None, optimize_depth=True, optimize_color=True, use_depth=True, use_desc=True):
    """The definition played through optimize_intrinsics-style sums, read_intrinsics_sums, set_intrinsics, a cfactor upload and
    evaluate_cost; the fields of Scene.optimize_intrinsics_controlled's result, plus `state` (what the scene is left with)."""
    c = c or DEFAULTS
    before, _ = g.evaluate_cost(use_depth, use_desc, per_keyframe=False)
    if not g.keyframes or g.surfels_size == 0:
        return dict(accepted=False, trials=0, lambda_accepted=0.0, lam=float(f32(lam)), cost_before=before, cost_after=before, state=gpu_state(g))
    saved = gpu_state(g)
    sums = gpu_sums(g, optimize_depth, optimize_color)
    trials = 0
    for rung in rungs(c, lam):
        trials += 1
        step = damped_step(sums[0], sums[1], rung, saved["depth_cam"], saved["color_cam"], saved["a"], saved["cfactor"], optimize_depth, optimize_color)
        gpu_put(g, step)
        after, _ = g.evaluate_cost(use_depth, use_desc, per_keyframe=False)
        if accepts(objective(before), objective(after)):
            return dict(accepted=True, trials=trials, lambda_accepted=float(rung), lam=float(down(c, rung)), cost_before=before, cost_after=after,
                        state=gpu_state(g))
        gpu_put(g, saved)
    return dict(accepted=False, trials=trials, lambda_accepted=0.0, lam=float(up(c, rung)), cost_before=before, cost_after=before, state=gpu_state(g))


# ---- the ladder table (scripts/intrinsics_step_control_ladder.py -> profiles/intrinsics_step_control_ladder.json) ---------------------
LADDER_RUNGS = (0.0, 0.25, 1.0, 4.0, 10.0, 16.0, 64.0, 100.0, 256.0)
LADDER_DEFAULT_RUNGS = (0.0, 1.0, 4.0, 16.0)
LADDER_CHOICES = {
    "default (first 1, up 4, max 1e4, 4 trials)": control(),
    "first 0.25, up 4": control(lambda_first=0.25),
    "first 1, up 10": control(lambda_up=10.0),
    "first 4, up 4": control(lambda_first=4.0),
}
LADDER_TABLE_SCENES = ("crop_small", "small21", "tiny")
LADDER_SEARCH_SCENES = ("crop_small", "small21", "tiny", "same", "small1", "small2", "small3", "small7")
LADDER_STEPS = 12


def _ladder_build(name):
    from tests import common, two_cameras
    if name.startswith("small"):
        return common.build_oracle(common.small_scene(num_keyframes=5, seed=int(name[5:])), 400000)
    return two_cameras.build_oracle(two_cameras.build_scene(name))


def ladder_plain_table(name):
    ba = _ladder_build(name)
    rows = []
    for step in range(LADDER_STEPS):
        saved = oracle_state(ba)
        before = ba.evaluate_cost()[0]
        sums = oracle_sums(ba)
        costs = {str(lam): oracle_trial(ba, sums, saved, lam)[0] for lam in LADDER_RUNGS}
        rel = [(costs[str(lam)] - before) / before for lam in LADDER_DEFAULT_RUNGS]
        kind = "falls" if rel[0] < 0 else ("H" if min(rel) > 0 else "R")
        rows.append(dict(step=step, before=before, costs=costs, kind=kind, relative_change_default_rungs=rel))
        oracle_put(ba, saved)
        ba.optimize_intrinsics(True, True)
    return rows


def ladder_sequence(name, choice):
    ba = _ladder_build(name)
    lam, rows = 0.0, []
    for step in range(8):
        r = oracle_controlled_step(ba, lam, choice)
        lam = r["lam"]
        rows.append(dict(step=step, accepted=r["lambda_accepted"] if r["accepted"] else None, trials=r["trials"], cost=r["cost_after"]))
    return dict(steps=rows, final=rows[-1]["cost"])


def ladder_profile():
    """What scripts/intrinsics_step_control_ladder.py writes: the table of the plain sequences, the controlled sequences per choice of
    ladder, and the search for the states R and H."""
    tables = {name: ladder_plain_table(name) for name in LADDER_SEARCH_SCENES}
    search = [dict(scene=name, step=row["step"], kind=row["kind"], relative_change_default_rungs=row["relative_change_default_rungs"])
              for name in LADDER_SEARCH_SCENES for row in tables[name] if row["kind"] != "falls"]
    sequences = {name: {label: ladder_sequence(name, choice) for label, choice in LADDER_CHOICES.items()} for name in LADDER_TABLE_SCENES}
    return dict(rungs=list(LADDER_RUNGS), default_rungs=list(LADDER_DEFAULT_RUNGS), table={name: tables[name] for name in LADDER_TABLE_SCENES},
                plain_final={name: tables[name][8]["before"] for name in LADDER_TABLE_SCENES}, sequences=sequences, search=search)
