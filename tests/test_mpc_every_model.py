"""The receding-horizon path -- cddp_hip_mpc_advance, cddp_hip_mpc_run_plant, cddp_hip_track_plan -- on every model struct of
PLANT_MODEL_LIST, on both stack layouts above nx = 8, on every registered kernel set that carries a constraint, in two tile groups at
nx > 8 and on the other three resident solvers above the smallest plants.  tests/test_mpc_advance.py and tests/test_plant_device.py hold
the same contracts on the pendulum and the unicycle; their helpers are the ones used here, and as there every comparison is BITWISE
(include/cddp_hip.h: each mode IS its host sequence, the plant loop IS the loop written out, tracking IS the host loop).

  1. every model: SHIFT_PROVIDED, SHIFT_EXISTING + SHIFT_DUALS and KEEP_PLAN against their host sequences, three rounds of "advance, then
     solve"; round 1 passes a measured state (x_1 plus a tenth of the row's spread), rounds 0 and 2 the plan's own x_1;
  2. every model: mpc_run_plant against test_plant_device.plant_loop, three steps, the mode alternating over the model table;
  3. every model: track_plan against test_plant_device.host_track;
  4. 1 to 3 again under CDDP_HIP_T4=0 for the models with nx > 8 (the G = 16 sweep's stacks wave-tiled instead of sub-tile-minor);
  5. every constrained kernel set: SHIFT_EXISTING + SHIFT_DUALS, the terminal duals included; the sets in_mpc_check refuses the flag
     for (no path duals) are named in REFUSED_SETS and their refusal is asserted;
  6. two tile groups (B = 130) at nx = 10 and nx = 14: the b0 offsets of the staging buffer, W, the parameter array and the logs;
  7. CLDDP, LogDDP and MSIPDDP on one plant with nx <= 8 and one with nx = 10 each (`compare` rows of tests/plant_matrix.py).

B = 70 (a full tile and a ragged one), the horizon of tests/model_cases.py, IPDDP with the model's control box, cold solves of two
iterations.  The tables below are held to the sources by tests/test_model_cases.py (CPU).  Every output is asserted finite before it is
compared: the equality helper treats NaN as equal to NaN."""
import numpy as np
import pytest

import model_cases as MC
import plant_matrix as PM
import test_mpc_advance as M
import test_plant_device as PD
from test_mpc_advance import same, shift

pytestmark = pytest.mark.gpu

B, ROUNDS, STEPS = MC.B, 3, 3
SEED = 20271100

# ---------------------------------------------------------------------------------------------------------------- the tables
T4_KEYS = ["quadrotor13", "quad12", "manip7", "quadrotor_rate", "spacecraft_nonlinear"]      # the models with nx > 8
MODEL_CASES = [(key, "default") for key in MC.MODEL_KEYS] + [(key, "t4=0") for key in T4_KEYS]
MODEL_IDS = ["%s-%s" % c for c in MODEL_CASES]
# sets for which cddp_hip_mpc_advance refuses CDDP_HIP_MPC_SHIFT_DUALS (m = 0: no path duals to shift)
REFUSED_SETS = ["lti1x1/none+terminal"]
SET_CASES = [name for name in MC.SET_NAMES if name not in REFUSED_SETS]
GROUP_KEYS = ["quadrotor_rate", "manip7"]                                                     # nx = 10 and nx = 14, two tile groups
GROUP_B = 130
# (kernel set, solver) pairs marked `compare` in plant_matrix.MATRIX: per solver one plant with nx <= 8 and one with nx = 10; MSIPDDP
# with a control box is refused at nu != 1, so its two rows are `/none` sets
SOLVER_CASES = ["acrobot_ctrlbox-clddp", "quadrotor_rate_ctrlbox-clddp", "usv_3dof_ctrlbox-logddp", "spacecraft_nonlinear_ctrlbox-logddp",
                "mrp_attitude_none-msipddp", "spacecraft_nonlinear_none-msipddp"]
# Rows whose x0 spread is widened (a factor on the row's, or one per coordinate) so that the plant loop's saturation is mixed: with the row's
# own spread the handle's u_0 of all 70 trajectories and three steps lies on one side of model_cases.plant_box.  Measured on the device,
# applied controls on the box / inside it, before -> after: the two HCW plants and the scalar integrator never reach the box (their u_0 is
# linear in x0 and moves by 0.002 .. 0.06 over the row's spread; 0 / 630 -> 81 / 549, 0 / 630 -> 74 / 556, 0 / 210 -> 79 / 131; the fuel
# plant's mass and its unused last state keep their spread), the rocket and the acrobot never leave it (two iterations from the cold
# start keep every u_0 within 0.4 of one bound; 210 / 0 -> 158 / 52 and 170 / 40).  The wider batch serves all three items of the row.
RAISED = {"hcw": {"spread": 300.0}, "linear_fuel": {"spread": [300.0] * 6 + [1.0, 1.0]}, "lti1x1": {"spread": 10.0},
          "dreyfus_rocket": {"spread": 100.0}, "acrobot": {"spread": 30.0}}
# models whose shift rounds must hold trajectories in two or more live slots within one advance (the per-lane slot addressing of
# k_mpc_shift, on both sides of nx = 8); the rows' own spread and two iterations reach that, no row is raised for it
MIXED_SLOT_KEYS = ["pendulum", "unicycle", "manipulator3", "usv_3dof", "quadrotor13", "quad12", "manip7", "quadrotor_rate"]

MODE_FLAGS = {"provided": ("MPC_SHIFT_PROVIDED", False), "existing+duals": ("MPC_SHIFT_EXISTING", True), "existing": ("MPC_SHIFT_EXISTING", False),
              "keep": ("MPC_KEEP_PLAN", False)}
MODEL_MODES = ("provided", "existing+duals", "keep")


def seed_of(key, item):
    return SEED + 100 * item + MC.MODEL_KEYS.index(key)


def finite(where, *arrays):
    for a in arrays:
        assert np.isfinite(np.asarray(a, dtype=np.float64)).all(), where


def model_problem(api, key):
    """-> row, problem (IPDDP, the model's control box, the horizon of its size, two iterations), x0 spread"""
    row = MC.MODELS[MC.KEYS[key]]
    p = MC.build_row(api, row)
    assert p.N == MC.horizon(p.nx) and p.c.solver == api.SOLVER_IPDDP
    over = RAISED.get(key, {})
    p.options.max_iterations = over.get("max_iterations", 2)
    return row, p, np.asarray(row.spread, dtype=np.float64) * np.asarray(over.get("spread", 1.0), dtype=np.float64)


def model_plant(api, row, p, batch, seed, **kw):
    """the problem's plant with a parameter block per trajectory (where it takes one)"""
    params = MC.plant_params(row, p, seed, b=batch)
    if params is not None:
        kw["params"] = params
        if row.nparams:
            assert len(np.unique(params, axis=0)) == batch
    dp = api.DevicePlant.of_problem(p, batch, **kw)
    assert bool(dp.desc.params_per_trajectory) == row.per_traj
    return dp


def disturbance(spread, rng, batch, steps):
    """a hundredth of the row's spread per coordinate"""
    return np.ascontiguousarray(0.01 * spread[None, None, :] * rng.uniform(-1.0, 1.0, (batch, steps, len(spread))))


# ---------------------------------------------------------------------------------------------------------------- the modes
def check_solved(a, b, where, duals=True, costates=True, terminal=False):
    """both handles' outputs finite, then equal"""
    for h in (a, b):
        X, U = h.trajectory()
        finite(where, X, U, h.results()["final_objective"])
        if duals:
            finite(where, *h.duals())
    M.assert_same_solve(a, b, where, duals=duals)
    if costates:
        La, Lb = a.costates(), b.costates()
        finite(where, La, Lb)
        assert La.shape == Lb.shape and same(La, Lb), (where, "costates")
    if terminal:
        for ta, tb, name in zip(a.terminal(), b.terminal(), ("S_T", "Y_T", "G_T", "Lambda_T")):
            finite(where, ta, tb)
            assert ta.shape == tb.shape and same(ta, tb), (where, name)


def advance(api, a, b, mode, x_next, where):
    """the host sequence of the mode on handle a, the entry point on handle b; b's getters return the shifted plan"""
    flag, sd = MODE_FLAGS[mode]
    X, U = a.trajectory()
    if mode == "keep":
        xn = a.plan_head()[1] if x_next is None else x_next
        assert x_next is not None or same(xn, X[:, 1])
        a.set_initial_state(xn)
        Xe, Ue = X.copy(), U
        Xe[:, 0] = xn
    else:
        if sd:
            S, Y, _ = a.duals()
        Xe, Ue = M.host_shift(a, mode == "provided", x_next=x_next, shift_duals=sd)
        assert same(Xe[:, 1:-1], X[:, 2:]) and same(Xe[:, -1], X[:, -1]) and same(Ue[:, :-1], U[:, 1:]) and same(Ue[:, -1], U[:, -1])
    b.mpc_advance(getattr(api, flag), x_next=x_next, shift_duals=sd)
    Xb, Ub = b.trajectory()
    finite(where, Xb, Ub)
    assert same(Xb, Xe) and same(Ub, Ue), (where, "the getter returns the shifted plan")
    if x_next is not None:
        assert same(Xb[:, 0], x_next), where
    if sd:
        Sb, Yb, _ = b.duals(); Sa, Ya, _ = a.duals()
        assert same(Sb, shift(S)) and same(Yb, shift(Y)), (where, "the getter returns the shifted duals")
        assert same(Sb, Sa) and same(Yb, Ya), where


def rounds(api, a, b, mode, n, spread, rng, where, **checks):
    """n rounds of "advance, then solve"; -> the distinct live slots in the batch before each advance"""
    slots = []
    for k in range(n):
        slots.append(np.unique(b.live_slots()).tolist())
        x1 = a.plan_head()[1]
        x_next = np.ascontiguousarray(x1 + 0.1 * spread[None, :] * rng.uniform(-1.0, 1.0, x1.shape)) if k % 2 == 1 else None
        advance(api, a, b, mode, x_next, where + (k,))
        a.solve(); b.solve()
        check_solved(a, b, where + (k,), **checks)
    return slots


def run_modes(api, key, layout):
    seen = {}
    for i, mode in enumerate(MODEL_MODES):
        row, p, spread = model_problem(api, key)                  # a new problem object: pair() leaves warm start on in the one it is given
        seed = seed_of(key, 1) + 1000 * i
        a, b, _, _ = M.pair(api, p, B, seed, spread=spread)
        check_solved(a, b, (key, layout, mode, "cold"))
        seen[mode] = rounds(api, a, b, mode, ROUNDS, spread, np.random.default_rng(seed), (key, layout, mode))
        a.close(); b.close()
    print("live slots %s nx=%d [%s] before each advance: %s" % (key, p.nx, layout, seen))
    if key in MIXED_SLOT_KEYS:
        assert any(len(s) >= 2 for mode in ("provided", "existing+duals") for s in seen[mode]), (key, seen)


# ---------------------------------------------------------------------------------------------------------------- the plant loop
def run_loop(api, key, mode, batch=B, groups=None):
    """mpc_run_plant against plant_loop: the plant has its own parameters per trajectory, two substeps (where it is not discrete), the
    box of model_cases.plant_box and a disturbance"""
    row, p, spread = model_problem(api, key)
    p.options.warm_start = 1
    seed = seed_of(key, 2)
    x0 = api.batch_x0(p, batch, seed, spread); U0 = api.batch_U0(p, batch)
    a = api.HipBatchSolver(p, batch); a.set_initial(x0, U0)
    b = api.HipBatchSolver(p, batch); b.set_initial(x0, U0)
    if groups is not None:
        assert a.num_groups() == groups and b.num_groups() == groups
    box = MC.plant_box(api, p)
    W = disturbance(spread, np.random.default_rng(seed), batch, STEPS)
    if groups is not None:
        assert len(np.unique(W[:, 0], axis=0)) == batch
    kw = dict(u_lower=box[0], u_upper=box[1], **({} if row.discrete else {"substeps": 2}))
    pa, pb = model_plant(api, row, p, batch, seed, **kw), model_plant(api, row, p, batch, seed, **kw)
    flag, sd = MODE_FLAGS[mode]
    heads = []
    U, X, it, st, _, model_x1, n_it = PD.plant_loop(api, a, pa, STEPS, getattr(api, flag), sd, W, box, heads=heads)
    X[:, 0] = x0
    r = b.mpc_run_plant(pb, STEPS, getattr(api, flag), shift_duals=sd, W=W)
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    where = (key, mode, batch)
    finite(where, U, X, r["U_applied"], r["X_visited"], Xa, Ua, Xb, Ub)
    assert same(r["U_applied"], U), (where, int(np.sum(r["U_applied"] != U)))
    assert same(r["X_visited"], X), (where, int(np.sum(r["X_visited"] != X)))
    assert same(r["iterations"], it) and same(r["status"], st), where
    assert same(Xa, Xb) and same(Ua, Ub), where
    assert r["stats"].traj_iterations == n_it == int(it.sum()), where
    # conditions on the inputs: the saturation is mixed, and the plant is not the model
    Uapp, raw = r["U_applied"], np.stack(heads, axis=1)
    print("applied controls %s [%s]: %d on the plant's box, %d inside; %d differ from the handle's own u_0" %
          (key, mode, int(((Uapp == box[0]) | (Uapp == box[1])).sum()), int(((Uapp > box[0]) & (Uapp < box[1])).sum()), int((Uapp != raw).sum())))
    assert ((Uapp == box[0]) | (Uapp == box[1])).any(), (where, "no applied control on the plant's box")
    assert ((Uapp > box[0]) & (Uapp < box[1])).any(), (where, "no applied control inside the plant's box")
    assert (Uapp != raw).any(), (where, "every applied u_0 is the handle's own")
    assert np.all(np.any(r["X_visited"][:, 1] != model_x1[0], axis=1)), (where, "the plant is the model on some trajectory")
    a.close(); b.close(); pa.close(); pb.close()


# ---------------------------------------------------------------------------------------------------------------- tracking
def run_track(api, key, batch=B, groups=None):
    row, p, spread = model_problem(api, key)
    seed = seed_of(key, 3)
    a, b, _, _ = M.pair(api, p, batch, seed, spread=spread)              # two solved handles; b never tracks
    if groups is not None:
        assert a.num_groups() == groups and b.num_groups() == groups
    Xp, Up = a.trajectory(); Kp, kp = a.gains()
    finite(key, Xp, Up, Kp, kp)
    rng = np.random.default_rng(seed)
    xs = np.ascontiguousarray(Xp[:, 0] + 0.1 * spread[None, :] * rng.uniform(-1.0, 1.0, (batch, p.nx)))
    W = disturbance(spread, rng, batch, p.N)
    if groups is not None:
        assert len(np.unique(W[:, 0], axis=0)) == batch
    # 0.8 of the plan's own control range about its middle (for a plan symmetric about zero: 0.8 max |U|, the box of
    # test_plant_device.test_track_plan_is_the_host_loop): the plan's extremes lie outside it, its middle inside
    lo, up = Up.min(axis=(0, 1)), Up.max(axis=(0, 1))
    box = (0.5 * (lo + up) - 0.4 * (up - lo), 0.5 * (lo + up) + 0.4 * (up - lo))
    assert (box[0] < box[1]).all(), key
    kw = dict(u_lower=box[0], u_upper=box[1], **({} if row.discrete else {"substeps": 2, "integrator": api.RK4}))
    dp = model_plant(api, row, p, batch, seed, **kw)
    Xr, Ur, clipped = PD.host_track(a, dp, xs, W, box)
    Xo, Uo = a.track_plan(dp, x0=xs, W=W)
    finite(key, Xr, Ur, Xo, Uo)
    assert same(Xo, Xr), (key, int(np.sum(Xo != Xr)))
    assert same(Uo, Ur), (key, int(np.sum(Uo != Ur)))
    assert same(Xo[:, 0], xs) and np.all(Uo >= box[0]) and np.all(Uo <= box[1]), key
    dp.close()
    # conditions on the inputs: mixed saturation, another first control than the plan's, feedback on every control row
    assert clipped > 0 and ((Ur == box[0]) | (Ur == box[1])).any(), (key, "no applied control on the plant's box")
    assert ((Ur > box[0]) & (Ur < box[1])).any(), (key, "no applied control inside the plant's box")
    assert (Ur[:, 0] != Up[:, 0]).any(), (key, "every applied u_0 is the handle's own")
    fb = np.einsum("btij,btj->bti", Kp, Xr[:, :-1] - Xp[:, :-1])
    assert (fb != 0.0).any(axis=(0, 1)).all(), (key, "a row of K without feedback", (fb != 0.0).any(axis=(0, 1)))
    # the model as the plant, from the plan's own start: the plan itself
    dm = api.DevicePlant.of_problem(p, batch)
    Xo, Uo = a.track_plan(dm)
    assert same(Xo, Xp) and same(Uo, Up), key
    dm.close()
    # the handle was only read, and solves like its twin
    Xa, Ua = a.trajectory(); Ka, ka = a.gains()
    assert same(Xa, Xp) and same(Ua, Up) and same(Ka, Kp) and same(ka, kp), key
    Xb, Ub = b.trajectory(); Kb, kb = b.gains()
    assert same(Xa, Xb) and same(Ua, Ub) and same(Ka, Kb) and same(ka, kb), key
    a.solve(); b.solve()
    check_solved(a, b, (key, "a solve after tracking"))
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- items 1 - 4
def layout_env(monkeypatch, layout):
    """nx > 8: the IPDDP handle runs the G = 16 cooperative sweep, whose A / Bm stacks are sub-tile-minor (route.t4) and whose gains also live
    as d.Kt.  The library has no getter of the route, so, as tests/test_plan_cov_shapes.py does, those models also run under CDDP_HIP_T4=0."""
    if layout == "t4=0":
        monkeypatch.setenv("CDDP_HIP_T4", "0")


@pytest.mark.parametrize("key,layout", MODEL_CASES, ids=MODEL_IDS)
def test_modes_are_their_host_sequences(api, monkeypatch, key, layout):
    layout_env(monkeypatch, layout)
    run_modes(api, key, layout)


@pytest.mark.parametrize("key,layout", MODEL_CASES, ids=MODEL_IDS)
def test_plant_loop_is_the_loop_written_out(api, monkeypatch, key, layout):
    layout_env(monkeypatch, layout)
    run_loop(api, key, MODEL_MODES[MC.MODEL_KEYS.index(key) % 3])


@pytest.mark.parametrize("key,layout", MODEL_CASES, ids=MODEL_IDS)
def test_track_plan_is_the_host_loop(api, monkeypatch, key, layout):
    layout_env(monkeypatch, layout)
    run_track(api, key)


# ---------------------------------------------------------------------------------------------------------------- item 5
def set_pair(api, name):
    p, x0, _ = MC.set_case(api, name)
    p.options.max_iterations = 2
    assert MC.set_of(api, p) == name and x0.shape == (B, p.nx)
    a, b, _, _ = M.pair(api, p, B, 0, x0=x0)
    assert a.m == b.m == p.dual_dim()
    return p, a, b, np.abs(x0 - p.x0[None, :]).max(axis=0)


@pytest.mark.parametrize("name", SET_CASES)
def test_every_constrained_set_shifts_its_duals(api, name):
    p, a, b, spread = set_pair(api, name)
    assert a.m > 0
    terminal = name.endswith("+terminal")
    assert terminal == bool(p._terms)
    check_solved(a, b, (name, "cold"), terminal=terminal)
    slots = rounds(api, a, b, "existing+duals", ROUNDS, spread, np.random.default_rng(SEED + 500), (name,), terminal=terminal)
    print("live slots %s m=%d before each advance: %s" % (name, a.m, slots))
    a.close(); b.close()


@pytest.mark.parametrize("name", REFUSED_SETS)
def test_sets_without_path_duals_refuse_the_flag(api, name):
    p, a, b, spread = set_pair(api, name)
    assert a.m == 0 and bool(p._terms)
    with pytest.raises(api.HipError):
        b.mpc_advance(api.MPC_SHIFT_EXISTING, shift_duals=True)
    assert b"no path duals" in api.load_hip().cddp_hip_last_error()
    # the refusal changed nothing, and without the flag the set's shift is its host sequence, terminal duals included
    check_solved(a, b, (name, "after the refusal"), terminal=True)
    rounds(api, a, b, "existing", ROUNDS, spread, np.random.default_rng(SEED + 501), (name,), terminal=True)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- item 6
@pytest.mark.parametrize("key", GROUP_KEYS)
def test_two_tile_groups(api, monkeypatch, key):
    """a parameter block and a disturbance of its own for every trajectory (asserted in model_plant and in the two runs): the b0 offsets
    into the staging buffer, W, the parameter array and the tiled logs of the second group"""
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    run_loop(api, key, "provided", batch=GROUP_B, groups=2)
    run_track(api, key, batch=GROUP_B, groups=2)


# ---------------------------------------------------------------------------------------------------------------- item 7
@pytest.mark.parametrize("case", SOLVER_CASES)
def test_other_resident_solvers(api, case):
    plant, _, solver = PM.parse(case)
    nx = PM.PLANTS[plant][0]
    spread = np.asarray(PM.PLANTS[plant][4], dtype=np.float64)
    ms = solver == "msipddp"
    for i, mode in enumerate(("provided", "keep") + (("existing",) if ms else ())):
        p = PM.problem(api, case, N=MC.horizon(nx), max_iterations=2)
        assert p.nx == nx and p.N == MC.horizon(nx)
        seed = SEED + 700 + 10 * SOLVER_CASES.index(case) + i
        a, b, _, _ = M.pair(api, p, B, seed, spread=spread)
        check_solved(a, b, (case, mode, "cold"), duals=ms, costates=ms)
        rounds(api, a, b, mode, 2, spread, np.random.default_rng(seed), (case, mode), duals=ms, costates=ms)
        a.close(); b.close()
