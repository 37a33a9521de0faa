"""Scoring candidate control sequences on the device and seeding from the best (cddp_hip_score_rollouts, cddp_hip_seed_best;
csrc/inst_score.hip, csrc/score_select.hpp).

The header fixes the arithmetic, so every check is BITWISE (np.array_equal with NaN = NaN; values, so -0.0 == 0.0: the library is built
with -fno-signed-zeros).  References: the solver's own initialisation (cost, states), the numpy restatement of the header's formulas
(constraint rows, objective), the constraint probe for the rows that take a square root, DevicePlant.step, track_plan and
set_initial_device.  Shapes: B = 70 (two tiles, the second ragged), S = 3 (B * S = 210: a wavefront straddles trajectories) and S = 65 (a
trajectory's candidates straddle wavefronts), N = 5; the nx = 12 plant at B = 66, S = 2, N = 3."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, S, N = 70, 3, 5


def torch_():
    import torch
    return torch


def same(a, b):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    if hasattr(b, "detach"):
        b = b.detach().cpu().numpy()
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def dev(a):
    return None if a is None else torch_().from_numpy(np.ascontiguousarray(a)).cuda()


def dmax(a, b):
    """dev_linalg.hpp::dmax, elementwise: (a < b) ? b : a"""
    return np.where(a < b, b, a)


# ---- problems: (name, builder(api, solver), x0 spread, control scale of the candidates)
def _pendulum(api, solver):
    return api.pendulum_problem(solver, True, horizon=N)


def _cartpole(api, solver):
    return api.cartpole_problem(solver, True, horizon=N)


def _unicycle(api, solver):
    p = api.unicycle_problem(solver, horizon=N)
    p.x0 = np.array([0.7, 0.8, np.pi / 4])        # next to the obstacle, so that the ball row takes both signs
    return p


def _quad12(api, solver):
    return api.quadrotor12_problem(solver, horizon=3)


def _pendulum_ref(api, solver):
    o = api.default_options(); o.max_iterations = 30; o.reg_initial_value = 1e-6
    ref = np.stack([np.linspace(np.pi, 0.0, N + 1), np.linspace(0.0, 0.5, N + 1)], axis=1)
    p = api.Problem(solver, api.MODEL_PENDULUM, api.EULER, 2, 1, N, 0.02, np.diag([2.0, 0.3]), 0.1 * np.eye(1), 100.0 * np.eye(2), [0.0, 0.0],
                    model_params=[0.5, 1.0, 0.01, 9.81], x_ref_traj=ref, options=o)
    p.add_control_box("ControlConstraint", [-20.0], [20.0])
    p.x0 = np.array([np.pi, 0.0])
    return p


def _lti_terminal(api, solver):
    p = api.scalar_integrator_problem(horizon=N, path_constraint=True, terminal_inequality=True, solver=solver)
    p.x0 = np.array([-0.2])
    return p


def _pendulum_statebox(api, solver):
    p = api.pendulum_problem(solver, True, horizon=N)
    p.add_state_box("StateConstraint", [3.0, -0.6], [3.3, 0.6])
    return p


def _lti_linear(api, solver):
    p = api.scalar_integrator_problem(horizon=N, solver=solver)
    p.add_linear("LinearConstraint", np.array([[1.0]]), np.array([0.25]))
    p.x0 = np.array([0.1])
    return p


def _cone(api, solver):
    return api.unicycle_cone_problem(solver, horizon=N)


def _thrust2(api, solver):
    return api.unicycle_thrust_problem(solver, horizon=N, two_sided=True)


def _thrust1(api, solver):
    return api.unicycle_thrust_problem(solver, horizon=N, two_sided=False)


# spread of x0 around p.x0, scale of the candidate controls: chosen so that some candidates violate their rows and some do not
PROBLEMS = {
    "pendulum": (_pendulum, [0.2, 0.3], 18.0, B, S),
    "cartpole_rk4": (_cartpole, [0.1, 0.3, 0.1, 0.1], 4.0, B, S),
    "unicycle_box_ball": (_unicycle, [0.3, 0.3, 0.4], [1.0, 2.5], B, S),
    "quad12": (_quad12, [0.1] * 12, 2.0, 66, 2),
    "pendulum_xref_traj": (_pendulum_ref, [0.2, 0.3], 18.0, B, S),
    "lti_terminal_ineq": (_lti_terminal, [0.3], 0.4, B, S),
    "pendulum_statebox": (_pendulum_statebox, [0.2, 0.5], 18.0, B, S),
    "lti_linear": (_lti_linear, [0.3], 0.2, B, S),
    "unicycle_cone": (_cone, [0.4, 0.6, 0.4], [1.0, 2.5], B, S),
    "unicycle_thrust2": (_thrust2, [0.3, 0.3, 0.4], [0.8, 0.8], B, S),
    "unicycle_thrust1": (_thrust1, [0.3, 0.3, 0.4], [1.2, 1.2], B, S),
}


def case(api, name, solver=None, ncand=None, seed=7):
    """-> problem, x0 (b, nx), U (b, s, n, nu)"""
    build, spread, scale, b, s = PROBLEMS[name]
    s = ncand or s
    p = build(api, api.SOLVER_IPDDP if solver is None else solver)
    rng = np.random.default_rng(seed)
    x0 = p.x0[None, :] + np.asarray(spread)[None, :] * rng.uniform(-1.0, 1.0, (b, p.nx))
    U = np.asarray(scale) * rng.standard_normal((b, s, p.N, p.nu))
    if name == "quad12":
        U = U + p.U0_const
    U[:, 0] *= 0.25                                   # a tame candidate per trajectory
    return p, np.ascontiguousarray(x0), np.ascontiguousarray(U)


@pytest.fixture(scope="module")
def scored(api):
    """score_rollouts of every problem on an IPDDP handle, host pointers, all four outputs: computed once, shared, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            p, x0, U = case(api, name)
            h = api.HipBatchSolver(p, x0.shape[0])
            out = h.score_rollouts(U, x0=x0, want=("cost", "viol", "X", "U"))
            h.close()
            for v in out.values():
                v.setflags(write=False)
            cache[name] = (p, x0, U, out)
        return cache[name]
    return get


# ---- 1. cost and states against the solver's own initialisation
@pytest.mark.parametrize("name", ["pendulum", "cartpole_rk4", "unicycle_box_ball", "quad12", "pendulum_xref_traj", "lti_terminal_ineq"])
def test_cost_and_states_are_the_solvers_initialisation(api, scored, name):
    p, x0, U, out = scored(name)
    b, s = U.shape[:2]
    assert p.options.warm_start == 0
    h = api.HipBatchSolver(p, b)
    for c in range(s):
        h.set_initial(x0, np.ascontiguousarray(U[:, c])); h.initialize()
        J = h.results()["final_objective"]; X = h.trajectory()[0]
        assert np.isfinite(J).all(), (name, c)
        assert same(out["cost"][:, c], J), (name, c, np.abs(out["cost"][:, c] - J).max())
        assert same(out["X"][:, c], X), (name, c)
        assert same(out["U"][:, c], U[:, c]), (name, c)          # no plant: the controls are applied as given
    h.close()
    # device pointers give the same bits, as device tensors
    h = api.HipBatchSolver(p, b)
    d = h.score_rollouts(dev(U), x0=dev(x0), want=("cost", "viol", "X", "U"))
    assert all(v.is_cuda and v.dtype == torch_().float64 for v in d.values())
    for k in out:
        assert same(d[k], out[k]), (name, k)
    h.close()


@pytest.mark.parametrize("name", ["pendulum", "unicycle_box_ball"])
def test_clddp_handle_gives_the_same_score(api, scored, name):
    p, x0, U, out = scored(name)
    pc, _, _ = case(api, name, solver=api.SOLVER_CLDDP)
    h = api.HipBatchSolver(pc, x0.shape[0])
    got = h.score_rollouts(U, x0=x0, want=("cost", "viol", "X"))
    h.close()
    for k in got:
        assert same(got[k], out[k]), (name, k)


def test_candidates_straddle_wavefronts(api):
    """S = 65: a trajectory's candidates lie in two wavefronts; every candidate equals its own S = 1 call"""
    p, x0, U = case(api, "pendulum", ncand=65)
    h = api.HipBatchSolver(p, B)
    out = h.score_rollouts(U, x0=x0, want=("cost", "viol", "X"))
    for c in (0, 1, 63, 64):
        one = h.score_rollouts(np.ascontiguousarray(U[:, c:c + 1]), x0=x0, want=("cost", "viol", "X"))
        for k in one:
            assert same(one[k][:, 0], out[k][:, c]), (c, k)
    h.set_initial(x0, np.ascontiguousarray(U[:, 64])); h.initialize()
    assert same(out["cost"][:, 64], h.results()["final_objective"])
    h.close()


# ---- 2. viol against a numpy restatement of the header (box, ball, linear rows) and the constraint probe (cone, thrust rows)
def rows_numpy(api, p, c, X, U):
    """The rows of constraint object c at every (b, s, t): list of (b, s, n) arrays in stacked order, or None for the probe's kinds"""
    KINDS = api
    api_kind = c.kind
    scale = c.scale

    def vec(ptr, n):
        return np.array([ptr[i] for i in range(n)])
    Xt = X[:, :, :-1]
    if api_kind in (KINDS.CON_CONTROL_BOX, KINDS.CON_STATE_BOX):
        V = U if api_kind == KINDS.CON_CONTROL_BOX else Xt
        lo, up = vec(c.lower, c.dim), vec(c.upper, c.dim)
        return [(-V[..., i]) * scale - (-lo[i]) * scale for i in range(c.dim)] + [V[..., i] * scale - up[i] * scale for i in range(c.dim)]
    if api_kind == KINDS.CON_BALL:
        ce = vec(c.center, c.dim)
        sq = np.zeros(Xt.shape[:3])
        for i in range(c.dim):
            df = Xt[..., i] - ce[i]
            sq = sq + df * df
        return [-(scale * sq) - (-(c.radius * c.radius) * scale)]
    if api_kind == KINDS.CON_LINEAR:
        nx = X.shape[-1]
        A, bb = vec(c.A, c.dim * nx).reshape(c.dim, nx), vec(c.b, c.dim)
        out = []
        for r in range(c.dim):
            s = np.zeros(Xt.shape[:3])
            for j in range(nx):
                s = s + A[r, j] * Xt[..., j]
            out.append(s - bb[r])
        return out
    return None


def rows_probe(api, c, X, U):
    """Cone and thrust rows from the device routine itself (tests/plant_probe.py): nx = 4, nu = 3 there, the spare entries zero (the cone
    reads x[:3]; a zero third control adds an exact 0 to the squared norm)"""
    import plant_probe as P
    lib = P.D.device()
    Xt = X[:, :, :-1]
    n = Xt.shape[0] * Xt.shape[1] * Xt.shape[2]
    x4 = np.zeros((n, P.CON_NX)); u3 = np.zeros((n, P.CON_NU))
    x4[:, :X.shape[-1]] = Xt.reshape(n, -1); u3[:, :U.shape[-1]] = U.reshape(n, -1)
    pool = P.Pool()
    if c.kind == api.CON_SOC:
        pool._con("soc", 3, 1, None, center=pool._put([c.center[i] for i in range(3)]), lower=pool._put([c.lower[i] for i in range(3)]),
                  scale=c.scale, radius=c.radius)
        tag = "soc"
    elif c.kind == api.CON_THRUST:
        pool._con("thrust2", 3, 2, None, lower=pool._put([c.lower[0]]), scale=c.scale, radius=c.radius)
        tag = "thrust2"
    else:
        pool._con("thrust1", 3, 1, None, scale=c.scale, radius=c.radius)
        tag = "thrust1"
    g = P.run_con(lib, tag, pool, x4, u3)[0]["g"]          # the ConDev / pool form: the one the scoring kernel calls
    return [g[:, i].reshape(Xt.shape[:3]) for i in range(g.shape[1])]


def viol_reference(api, p, X, U):
    """-> viol (b, s), the smallest and the largest row value met"""
    cons = sorted(p._cons, key=lambda c: c.name)            # the stacked order: constraint objects sorted by name
    per_con = []
    for c in cons:
        r = rows_numpy(api, p, c, X, U)
        per_con.append(r if r is not None else rows_probe(api, c, X, U))
    viol = np.zeros(X.shape[:2]); lo, hi = np.inf, -np.inf
    for t in range(U.shape[2]):
        for rows in per_con:
            for g in rows:
                viol = dmax(viol, g[:, :, t]); lo = min(lo, g.min()); hi = max(hi, g.max())
    for tc in sorted(p._terms, key=lambda c: c.name):
        if tc.kind != api.TERM_INEQUALITY:
            continue
        nx = X.shape[-1]
        for r in range(tc.dim):
            s = np.zeros(X.shape[:2])
            for j in range(nx):
                s = s + tc.A[r * nx + j] * X[:, :, -1, j]
            g = s - tc.b[r]
            viol = dmax(viol, g); lo = min(lo, g.min()); hi = max(hi, g.max())
    return viol, lo, hi


@pytest.mark.parametrize("name", ["pendulum", "unicycle_box_ball", "pendulum_statebox", "lti_linear", "lti_terminal_ineq", "unicycle_cone",
                                  "unicycle_thrust2", "unicycle_thrust1"])
def test_viol_is_the_headers_formula(api, scored, name):
    p, x0, U, out = scored(name)
    ref, lo, hi = viol_reference(api, p, out["X"], out["U"])
    print(name, "rows in [%g, %g]; viol > 0 on %d of %d" % (lo, hi, int((ref > 0).sum()), ref.size))
    assert lo < 0 < hi, (name, lo, hi)                                  # both signs occur among the rows
    assert (ref > 0).any() and (ref == 0).any(), name                   # ... and among the candidates: some violate, some do not
    assert same(out["viol"], ref), (name, np.abs(out["viol"] - ref).max())


def test_each_kind_alone_takes_both_signs(api, scored):
    """the state-dependent rows specifically: the ball next to the unicycle's start, the state box, the linear row, the cone"""
    for name, kind in (("unicycle_box_ball", api.CON_BALL), ("pendulum_statebox", api.CON_STATE_BOX), ("lti_linear", api.CON_LINEAR),
                       ("unicycle_cone", api.CON_SOC)):
        p, x0, U, out = scored(name)
        c = [c for c in p._cons if c.kind == kind][0]
        rows = rows_numpy(api, p, c, out["X"], out["U"]) or rows_probe(api, c, out["X"], out["U"])
        g = np.stack(rows)
        assert g.min() < 0 < g.max(), (name, g.min(), g.max())


# ---- 3. plant mode: per-trajectory parameters, two substeps, an actuator box
def objective_numpy(p, X, U):
    """running_cost / terminal_cost of dev_constraints.hpp in the stated association (e^T Q) e: per column j a zero accumulator
    r += e[i] * Q[i][j], then s += r * e[j]"""
    nx, nu = p.nx, p.nu
    Qdt, Rdt, Qf, xr = p.Q * p.dt, p.R * p.dt, p.Qf, p.x_ref
    ref = getattr(p, "x_ref_traj", None)

    def quad(M, e, n):
        s = np.zeros(e.shape[:-1])
        for j in range(n):
            r = np.zeros(e.shape[:-1])
            for i in range(n):
                r = r + e[..., i] * M[i, j]
            s = s + r * e[..., j]
        return s
    cost = np.zeros(X.shape[:2])
    for t in range(U.shape[2]):
        e = X[:, :, t] - (ref[t] if ref is not None else xr)
        cost = cost + (quad(Qdt, e, nx) + quad(Rdt, U[:, :, t], nu))
    return cost + quad(Qf, X[:, :, -1] - xr, nx)


def test_objective_restatement_is_the_kernels(api, scored):
    """the numpy objective is validated where the solver's own initialisation is the reference, before it serves as one below"""
    for name in ("cartpole_rk4", "pendulum_xref_traj", "unicycle_box_ball"):
        p, x0, U, out = scored(name)
        assert same(objective_numpy(p, out["X"], out["U"]), out["cost"]), name


def test_plant_mode(api):
    p, x0, U = case(api, "cartpole_rk4", seed=11)
    rng = np.random.default_rng(3)
    params = np.tile(np.array(list(p.c.model_params)[:5]), (B, 1))
    params[:, 1] *= rng.uniform(0.8, 1.3, B)                           # every trajectory its own pole mass
    dp = api.DevicePlant.of_problem(p, B, params=params, substeps=2, u_lower=[-3.0], u_upper=[2.5])
    h = api.HipBatchSolver(p, B)
    out = h.score_rollouts(U, x0=x0, plant=dp, want=("cost", "viol", "X", "U"))
    Usat = np.minimum(np.maximum(U, -3.0), 2.5)
    assert (Usat != U).any() and (Usat == U).any()
    assert same(out["U"], Usat)
    X = np.zeros((B, S, N + 1, p.nx))
    for c in range(S):
        x = x0.copy(); X[:, c, 0] = x
        for t in range(N):
            x = dp.step(x, np.ascontiguousarray(U[:, c, t])); X[:, c, t + 1] = x
    assert same(out["X"], X)
    assert same(out["cost"], objective_numpy(p, X, Usat))
    ref, lo, hi = viol_reference(api, p, X, Usat)
    assert same(out["viol"], ref) and (ref == 0).all()                 # the plant's box lies inside the problem's: the applied controls are admissible
    # the model's own score differs: the plant is not the model
    own = h.score_rollouts(U, x0=x0, want=("cost",))
    assert not same(own["cost"], out["cost"])
    d = h.score_rollouts(dev(U), x0=dev(x0), plant=dp, want=("cost", "viol", "X", "U"))
    for k in out:
        assert same(d[k], out[k]), k
    h.close(); dp.close()


# ---- 4. feedback mode
def test_feedback_mode_is_track_plan(api):
    p, x0, _ = case(api, "cartpole_rk4", seed=5)
    p.options.max_iterations = 3
    h = api.HipBatchSolver(p, B)
    h.set_initial(x0); h.solve()
    Xp, Up = h.trajectory()
    dp = api.DevicePlant.of_problem(p, B)                              # a plant equal to the model
    rng = np.random.default_rng(9)
    off = 0.05 * rng.standard_normal((B, S, p.nx)); off[:, 0] = 0.0
    x0c = np.ascontiguousarray(Xp[:, None, 0, :] + off)
    out = h.score_rollouts(None, x0=x0c, plant=dp, feedback=True, want=("cost", "X", "U"))
    for c in range(S):
        Xt, Ut = h.track_plan(dp, x0=np.ascontiguousarray(x0c[:, c]))
        assert same(out["X"][:, c], Xt), c
        assert same(out["U"][:, c], Ut), c
    assert same(out["X"][:, 0], Xp) and same(out["U"][:, 0], Up)       # zero offset: the plan itself
    assert not same(out["X"][:, 1], Xp)
    # x0 = None is row 0 of the plan; the handle's own model is the plant equal to the model
    a = h.score_rollouts(None, feedback=True, want=("cost", "X"))
    assert a["X"].shape == (B, 1, N + 1, p.nx) and same(a["X"][:, 0], Xp)
    b = h.score_rollouts(None, x0=x0c, feedback=True, want=("cost", "X", "U"))
    for k in b:
        assert same(b[k], out[k]), k
    # candidate controls under feedback: U_c + K (x - X); with U_c the plan's own U this is the line above
    Uc = np.ascontiguousarray(np.repeat(Up[:, None], S, axis=1))
    e = h.score_rollouts(Uc, x0=x0c, feedback=True, want=("cost", "X", "U"))
    for k in e:
        assert same(e[k], out[k]), k
    d = h.score_rollouts(None, x0=dev(x0c), plant=dp, feedback=True, want=("cost", "X", "U"))
    for k in out:
        assert same(d[k], out[k]), k
    h.close(); dp.close()


# ---- 5. scoring leaves the handle alone
def snapshot(api, h):
    out = {}
    for f in api.FIELD_NAMES:
        try:
            out[f] = h.field_device(f).cpu().numpy()
        except api.HipError:
            out[f] = None
    out["results"] = h.results_device()["cols"].cpu().numpy(), h.results_device()["icols"].cpu().numpy()
    return out


def same_snapshot(a, b):
    for k in a:
        if k == "results":
            if not (same(a[k][0], b[k][0]) and same(a[k][1], b[k][1])):
                return k
        elif (a[k] is None) != (b[k] is None) or (a[k] is not None and not same(a[k], b[k])):
            return k
    return None


def solve_record(h):
    st = h.solve()
    X, U = h.trajectory()
    return h.results().copy(), X, U, (st.sweeps, st.rollouts, st.traj_iterations, st.outer_iterations, st.n_converged)


def same_record(a, b):
    return a[0].tobytes() == b[0].tobytes() and same(a[1], b[1]) and same(a[2], b[2]) and a[3] == b[3]


def test_score_leaves_the_handle_alone(api):
    p, x0, U = case(api, "unicycle_box_ball", seed=13)
    p.options.max_iterations = 4
    U0 = np.ascontiguousarray(U[:, 0])
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0); h.solve()
    before = snapshot(api, h)
    dp = api.DevicePlant.of_problem(p, B, substeps=2)
    h.score_rollouts(U, x0=x0, want=("cost", "viol", "X", "U"))
    h.score_rollouts(dev(U), x0=dev(x0), plant=dp, feedback=True, want=("cost", "viol"))
    assert same_snapshot(before, snapshot(api, h)) is None
    again = solve_record(h)
    twin = api.HipBatchSolver(p, B); twin.set_initial(x0, U0); twin.solve()
    ref = solve_record(twin)
    assert same_record(again, ref)
    h.close(); twin.close(); dp.close()


# ---- 6. seed_best
def select_numpy(cost, viol, tol):
    """The rule of include/cddp_hip.h written out: -> winner (b,)"""
    b, s = cost.shape
    out = np.full(b, -1, dtype=np.int32)
    for i in range(b):
        fin = [c for c in range(s) if np.isfinite(cost[i, c]) and np.isfinite(viol[i, c])]
        adm = [c for c in fin if viol[i, c] <= tol]
        if adm:
            out[i] = min(adm, key=lambda c: (cost[i, c], c))
        elif fin:
            out[i] = min(fin, key=lambda c: (viol[i, c], cost[i, c], c))
    return out


def hand_built_records(b, s, seed):
    rng = np.random.default_rng(seed)
    cost = rng.uniform(1.0, 9.0, (b, s)); viol = np.where(rng.uniform(size=(b, s)) < 0.5, 0.0, rng.uniform(0.0, 2.0, (b, s)))
    cost[0] = 3.0; viol[0] = 0.0                                        # all tied: candidate 0
    cost[1] = [5.0, 2.0, 2.0]; viol[1] = 0.0                            # a tie of the lowest cost: the lower index
    cost[2] = [np.nan, 4.0, 6.0]; viol[2] = 0.0                         # a NaN cost loses
    cost[3] = [1.0, 2.0, 3.0]; viol[3] = [0.5, 0.2, 0.2]                # none admissible: lowest viol, then lowest cost
    cost[4] = [np.nan, np.inf, 1.0]; viol[4] = [0.0, 0.0, np.nan]       # none finite: -1
    cost[5] = [1.0, 2.0, 3.0]; viol[5] = [0.05, 0.0, 0.0]               # viol_tol = 0.1 changes the winner from 1 to 0
    cost[6] = [-np.inf, 2.0, 3.0]; viol[6] = [0.0, 0.3, 0.0]            # -inf is not finite
    cost[7] = [1.0, 2.0, 3.0]; viol[7] = [np.inf, 0.4, 0.4]             # an infinite violation loses; tie of viol: the lower cost
    return np.ascontiguousarray(cost), np.ascontiguousarray(viol)


def test_seed_best_winners_follow_the_rule(api):
    p, x0, U = case(api, "pendulum", seed=17)
    cost, viol = hand_built_records(B, S, 19)
    h = api.HipBatchSolver(p, B)
    for tol in (0.0, 0.1):
        ref = select_numpy(cost, viol, tol)
        w = h.seed_best(U, cost, viol, x0=x0, viol_tol=tol)
        assert w.dtype == np.int32 and same(w, ref), tol
        wd = h.seed_best(dev(U), dev(cost), dev(viol), x0=dev(x0), viol_tol=tol)
        assert wd.is_cuda and wd.dtype == torch_().int32 and same(wd, ref), tol
        assert list(ref[:5]) == [0, 1, 1, 1, -1] and ref[5] == (0 if tol > 0 else 1) and ref[6] == 2 and ref[7] == 1
    w0 = h.seed_best(U, cost, None, x0=x0)                              # viol = None: all 0
    assert same(w0, select_numpy(cost, np.zeros_like(cost), 0.0))
    h.close()


@pytest.mark.parametrize("pointers", ["host", "device"])
def test_seed_best_seeds_as_set_initial_device(api, scored, pointers):
    out = scored("unicycle_box_ball")[3]
    p, x0, U = case(api, "unicycle_box_ball")                           # (the same seed: the arrays that were scored; a problem of this test's own)
    p.options.max_iterations = 4
    conv = dev if pointers == "device" else (lambda a: a)
    cost, viol = out["cost"].copy(), out["viol"].copy()
    cost[3] = np.nan                                                    # one trajectory without a finite candidate: seeded from c = 0
    h = api.HipBatchSolver(p, B)
    w = h.seed_best(conv(U), conv(cost), conv(viol), x0=conv(x0), viol_tol=0.0)
    w = w.cpu().numpy() if pointers == "device" else w
    ref = select_numpy(cost, viol, 0.0)
    assert same(w, ref) and w[3] == -1 and len(set(w.tolist())) > 2     # the winners differ over the batch
    pick = np.ascontiguousarray(U[np.arange(B), np.maximum(w, 0)])
    twin = api.HipBatchSolver(p, B)
    twin.set_initial_device(dev(x0), dev(pick))
    h.initialize(); twin.initialize()
    assert same_snapshot(snapshot(api, twin), snapshot(api, h)) is None
    good = w >= 0
    assert same(h.results()["final_objective"][good], cost[np.arange(B), np.maximum(w, 0)][good])   # the seed's cost is the score
    assert same_record(solve_record(h), solve_record(twin))
    # x0 = None keeps the handle's x0: another seed, the same initial state
    w2 = h.seed_best(conv(U), conv(-cost), None)
    w2 = w2.cpu().numpy() if pointers == "device" else w2
    twin.set_initial_device(dev(x0), dev(np.ascontiguousarray(U[np.arange(B), np.maximum(w2, 0)])))
    assert not same(w2, w)
    h.initialize(); twin.initialize()
    assert same_snapshot(snapshot(api, twin), snapshot(api, h)) is None
    h.close(); twin.close()


def test_two_tile_groups_offset_every_pointer(api, monkeypatch):
    """a handle of two tile groups (B = 150: tiles 2 + 1) against one of a single group: scoring with per-trajectory plant parameters
    and per-candidate x0 under feedback, and seeding, host and device pointers"""
    b = 150
    p, _, _ = case(api, "cartpole_rk4")
    p.options.max_iterations = 3
    rng = np.random.default_rng(31)
    x0 = np.ascontiguousarray(p.x0[None, :] + 0.2 * rng.uniform(-1.0, 1.0, (b, p.nx)))
    U = np.ascontiguousarray(4.0 * rng.standard_normal((b, S, N, p.nu)))
    params = np.tile(np.array(list(p.c.model_params)[:5]), (b, 1)); params[:, 1] *= rng.uniform(0.8, 1.3, b)
    x0c = np.ascontiguousarray(x0[:, None, :] + 0.05 * rng.standard_normal((b, S, p.nx)))
    got = {}
    for groups in (1, 2):
        monkeypatch.setenv("CDDP_HIP_GROUPS", str(groups))
        h = api.HipBatchSolver(p, b)
        assert h.num_groups() == groups
        dp = api.DevicePlant.of_problem(p, b, params=params, substeps=2, u_lower=[-3.0], u_upper=[2.5])
        h.set_initial(x0); h.solve()
        r = {}
        for kind, conv in (("host", lambda a: a), ("device", dev)):
            r[kind, "own"] = h.score_rollouts(conv(U), x0=conv(x0), want=("cost", "viol", "X", "U"))
            r[kind, "plant_fb"] = h.score_rollouts(conv(U), x0=conv(x0c), plant=dp, feedback=True, want=("cost", "viol", "X", "U"))
        sc = r["host", "own"]
        w = h.seed_best(U, sc["cost"], sc["viol"], x0=x0)
        wd = h.seed_best(dev(U), dev(sc["cost"]), dev(sc["viol"]), x0=dev(x0))
        assert same(w, wd)
        h.initialize()
        got[groups] = (r, w, snapshot(api, h))
        h.close(); dp.close()
    r1, w1, s1 = got[1]; r2, w2, s2 = got[2]
    for key in r1:
        for k in r1[key]:
            assert same(r1[key][k], r2[key][k]), (key, k)
            assert same(r1[key][k], r1["host", key[1]][k]), (key, k)
    assert same(w1, w2) and same(w1, select_numpy(r1["host", "own"]["cost"], r1["host", "own"]["viol"], 0.0))
    assert same_snapshot(s1, s2) is None


# ---- 7. refusals: each returns its error, launches nothing, and the handle still solves to the same result
def test_refusals(api):
    p, x0, U = case(api, "pendulum", seed=23)
    p.options.max_iterations = 3
    h = api.HipBatchSolver(p, B); h.set_initial(x0)
    ref = solve_record(h)
    fresh = api.HipBatchSolver(p, B)                                    # never initialised: no plan, no gains
    lib = h.lib
    cost = np.full((B, S), -7.0); viol = np.full((B, S), -7.0)
    other_nx = api.DevicePlant.of_problem(api.cartpole_problem(), B)
    other_batch = api.DevicePlant.of_problem(p, B + 1)
    t = torch_()
    dU, dx0 = dev(U), dev(x0)
    dcost = t.full((B, S), -7.0, dtype=t.float64, device="cuda")
    # (an allocation that ends before the extent: torch's allocator hands out pieces of larger allocations, so that refusal is exercised
    # with a hipMalloc one element short in tests/cpp/test_score_wrapper.cpp, for both entries)
    ptr = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())

    def score(hh, plant, flags, s, x0_, U_, cost_, viol_=None):
        return lib.cddp_hip_score_rollouts(hh.h, plant.h if plant is not None else None, flags, s, ptr(x0_), ptr(U_), ptr(cost_), ptr(viol_), None, None)

    def seed(hh, flags, s, x0_, U_, cost_, viol_=None, winner=None):
        return lib.cddp_hip_seed_best(hh.h, flags, s, ptr(x0_), ptr(U_), ptr(cost_), ptr(viol_), 0.0, ptr(winner))

    def refused(rc, *needles):
        msg = lib.cddp_hip_last_error().decode()
        assert rc < 0, msg
        for n in needles:
            assert n in msg, (n, msg)
        assert (cost == -7.0).all() and bool((dcost == -7.0).all())      # nothing written
        assert same_record(solve_record(h), ref), msg                                                   # the handle still solves alike

    refused(score(h, None, 0, 0, x0, U, cost), "cddp_hip_score_rollouts", "ncand = 0")
    refused(score(h, None, 0, S, x0, U, None), "null cost")
    refused(score(h, None, 0, S, x0, None, cost), "U is NULL without CDDP_HIP_SCORE_FEEDBACK")
    refused(score(fresh, None, api.SCORE_FEEDBACK, S, x0, U, cost), "cddp_hip_score_rollouts needs a solved handle", "no gain stack to track")
    with pytest.raises(api.HipError, match="needs a solved handle: there is no plan and no gain stack to track"):
        fresh.track_plan(api.DevicePlant.of_problem(p, B))              # the same test, the same message
    refused(score(h, other_nx, 0, S, x0, U, cost), "nx = 4")
    refused(score(h, other_batch, 0, S, x0, U, cost), "batch of %d" % (B + 1))
    refused(score(h, None, api.SCORE_DEVICE, S, x0, dU, dcost), "x0 is not device memory")
    refused(score(h, None, api.SCORE_DEVICE, S, dx0, dU, cost), "cost is not device memory")
    refused(score(h, None, 8, S, x0, U, cost), "unknown flag bits")
    refused(score(h, None, api.SCORE_X0_PER_CANDIDATE, S, None, U, cost), "NULL x0")
    refused(score(fresh, None, 0, S, None, U, cost), "x0 is NULL and the handle has no plan")
    refused(seed(h, 0, 0, x0, U, cost), "cddp_hip_seed_best", "ncand = 0")
    refused(seed(h, 0, S, x0, None, cost), "null U")
    refused(seed(h, 0, S, x0, U, None), "null cost")
    refused(seed(h, 2, S, x0, U, cost), "unknown flag bits")
    refused(seed(fresh, 0, S, None, U, cost), "no initial state to keep")
    refused(seed(h, api.SCORE_DEVICE, S, dx0, dU, cost), "cost is not device memory")
    refused(seed(h, api.SCORE_DEVICE, S, dx0, dU, dcost, None, np.zeros(B, dtype=np.int32)), "winner is not device memory")
    h.close(); fresh.close(); other_nx.close(); other_batch.close()


# ---- 8. the facade: score, seed, solve
def test_solve_batch_sampled_is_the_three_calls(api):
    import importlib.util
    import os
    import sys
    name = "pycddp_amd"
    if name not in sys.modules:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py")
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    F = sys.modules[name]
    p, x0, U = case(api, "pendulum", seed=29)
    o = F.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 4
    solver = F.CDDP(x0[0], p.x_ref, p.N, p.dt, o)
    solver.set_dynamical_system(F.Pendulum(p.dt, *list(p.c.model_params)[:3], "euler"))
    solver.set_objective(F.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    solver.add_constraint("ControlConstraint", F.ControlConstraint(np.array([-20.0]), np.array([20.0])))
    out = solver.solve_batch_sampled(dev(x0), dev(U), solver_type=F.SolverType.IPDDP, viol_tol=0.0, want=("X", "U"))
    kind = solver._resident_kind("IPDDP")
    pp = solver._problem(kind)
    h = api.HipBatchSolver(pp, B)
    sc = h.score_rollouts(dev(U), x0=dev(x0))
    w = h.seed_best(dev(U), sc["cost"], sc["viol"], x0=dev(x0), viol_tol=0.0)
    h.solve()
    assert same(out["winner"], w) and same(out["winner"], select_numpy(sc["cost"].cpu().numpy(), sc["viol"].cpu().numpy(), 0.0))
    assert same(out["seed_cost"], sc["cost"].cpu().numpy()[np.arange(B), np.maximum(w.cpu().numpy(), 0)])
    assert same(out["X"], h.field_device("X")) and same(out["U"], h.field_device("U"))
    res = h.results_device()
    for k in ("final_objective", "iterations", "status"):
        assert same(out["results"][k], res[k]), k
    assert len(set(out["winner"].cpu().numpy().tolist())) > 1
    h.close()
