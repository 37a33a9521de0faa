"""cddp_hip_score_rollouts on every model it is compiled for (k_score<M, PER> over PLANT_MODEL_LIST, csrc/inst_score.hip), with shared and with
per-trajectory parameters, and on every registered kernel set that carries a constraint (fold_path_rows at the model's own dimensions).

Shapes: B = 70 (a full tile and a ragged one), S = 3: B * S = 210 lanes, so the last wavefront goes through the LDS staging barrier of the
large plants with 18 live lanes; N = 5, N = 3 for nx >= 12.  Candidate scales are a vector with a distinct ratio to the box per control
(tests/model_cases.py).  Every comparison is BITWISE (same() of tests/test_score_rollouts.py) except the 60-digit objective, whose bound is
derived where it is used.  The conditions on the inputs (every reference finite on every lane, candidates on both sides of every case's rows,
a plant box that clips some entries and not others) are asserted on the references before anything is compared; tests/test_model_cases.py
asserts them on the CPU as well."""
import numpy as np
import pytest

import model_cases as MC
from test_score_rollouts import dev, objective_numpy, same, torch_, viol_reference

pytestmark = pytest.mark.gpu

B, S = MC.B, MC.S


@pytest.fixture(scope="module")
def scored(api):
    """score_rollouts of a model's row (key) or of a constrained set's case (set name) on an IPDDP handle, host pointers, all four outputs:
    computed once, shared, never modified"""
    cache = {}

    def get(name):
        how = MC.SET_CASES.get(name)
        if isinstance(how, str) and how.startswith("own:"):
            name = how[4:]
        if name not in cache:
            p, x0, U = MC.set_case(api, name) if "/" in name else MC.model_case(api, name)[:3]
            h = api.HipBatchSolver(p, B)
            out = h.score_rollouts(U, x0=x0, want=("cost", "viol", "X", "U"))
            h.close()
            for v in (x0, U) + tuple(out.values()):
                v.setflags(write=False)
            cache[name] = (p, x0, U, out)
        return cache[name]
    return get


# ---- 1. the model's own rollout and objective against the solver's initialisation
@pytest.mark.parametrize("model", MC.MODEL_KEYS)
def test_own_model_is_the_solvers_initialisation(api, scored, model):
    p, x0, U, out = scored(model)
    assert p.options.warm_start == 0 and U.shape == (B, S, MC.horizon(p.nx), p.nu)
    h = api.HipBatchSolver(p, B)
    for c in range(S):
        h.set_initial(x0, np.ascontiguousarray(U[:, c])); h.initialize()
        J = h.results()["final_objective"]; X = h.trajectory()[0]
        assert np.isfinite(J).all() and np.isfinite(X).all(), (model, c)           # every lane: no reference entry is left out
        assert same(out["cost"][:, c], J), (model, c, np.abs(out["cost"][:, c] - J).max())
        assert same(out["X"][:, c], X), (model, c)
        assert same(out["U"][:, c], U[:, c]), (model, c)                           # no plant: the controls are applied as given
    h.close()
    h = api.HipBatchSolver(p, B)
    d = h.score_rollouts(dev(U), x0=dev(x0), want=("cost", "viol", "X", "U"))
    assert all(v.is_cuda and v.dtype == torch_().float64 for v in d.values())
    for k in out:
        assert same(d[k], out[k]), (model, k)
    h.close()


# ---- 2. plant mode: per-trajectory parameters over the whole caller-visible block, two substeps, an actuator box
@pytest.mark.parametrize("model", MC.MODEL_KEYS)
def test_rollout_is_the_device_plants_step(api, model):
    """PER = true wherever the plant takes a block per trajectory (the LTI plants' matrices are shared by the batch: PER = false there);
    substeps = 2 except on the two discrete plants, which cddp_hip_plant_create refuses to sub-step."""
    row = MC.MODELS[MC.KEYS[model]]
    p, x0, U, centre, scale = MC.model_case(api, model, seed=11)
    N = p.N
    lo, up = MC.control_box(api, p)
    plo, pup = MC.plant_box(api, p)
    assert (plo > lo).all() and (pup < up).all()                                   # strictly inside the problem's box
    Usat = np.minimum(np.maximum(U, plo), pup)
    assert (Usat != U).any() and (Usat == U).any(), model                          # ... and it clips some entries and leaves others
    params = MC.plant_params(row, p, 3)
    kw = {} if params is None else {"params": params}
    dp = api.DevicePlant.of_problem(p, B, substeps=1 if row.discrete else 2, u_lower=plo, u_upper=pup, **kw)
    assert bool(dp.desc.params_per_trajectory) == row.per_traj
    h = api.HipBatchSolver(p, B)
    out = h.score_rollouts(U, x0=x0, plant=dp, want=("cost", "viol", "X", "U"))
    X = np.zeros((B, S, N + 1, p.nx))
    for c in range(S):
        x = x0.copy(); X[:, c, 0] = x
        for t in range(N):
            x = dp.step(x, np.ascontiguousarray(U[:, c, t])); X[:, c, t + 1] = x
    cost = objective_numpy(p, X, Usat)
    viol, lo_g, hi_g = viol_reference(api, p, X, Usat)
    assert np.isfinite(X).all() and np.isfinite(cost).all() and np.isfinite(viol).all(), model
    assert same(out["U"], Usat), model
    assert same(out["X"], X), (model, np.abs(out["X"] - X).max())
    assert same(out["cost"], cost), (model, np.abs(out["cost"] - cost).max())
    assert same(out["viol"], viol) and (viol == 0).all(), model                    # the applied controls are admissible: the plant's box lies inside
    own = h.score_rollouts(U, x0=x0, want=("cost",))
    assert not same(own["cost"], out["cost"])                                      # the plant is not the model
    d = h.score_rollouts(dev(U), x0=dev(x0), plant=dp, want=("cost", "viol", "X", "U"))
    for k in out:
        assert same(d[k], out[k]), (model, k)
    if row.per_traj and row.nparams == 0:
        # equal blocks at a per-trajectory stride against the one shared block: the same bits (the library fills the vessel's 21 entries)
        shared = api.DevicePlant.of_problem(p, B, substeps=2, u_lower=plo, u_upper=pup)
        assert not shared.desc.params_per_trajectory
        o2 = h.score_rollouts(U, x0=x0, plant=shared, want=("cost", "X"))
        assert same(o2["X"], out["X"]) and same(o2["cost"], out["cost"]), model
        shared.close()
    h.close(); dp.close()


# ---- 3. the objective against 60 digits
LANES = (0, 191, 192, 209, 200, 205)    # g = b * S + c: first and last trajectory of the full tile and of the ragged one, and two inside the last wavefront


def objective_60_digits(p, X, U, lanes):
    """sum_t (e^T (Q dt) e + u^T (R dt) u) + e_N^T Qf e_N of lanes g at 60 digits from the doubles the device returned, and
    sum |e_i| |M_ij| |e_j| over all terms"""
    import mpmath
    mpmath.mp.dps = 60
    mpf = mpmath.mpf
    Qdt, Rdt, Qf, xr = p.Q * p.dt, p.R * p.dt, p.Qf, p.x_ref
    ref = getattr(p, "x_ref_traj", None)
    N = U.shape[2]

    def quad(M, e):
        v = mpf(0); a = mpf(0)
        for i in range(len(e)):
            for j in range(len(e)):
                if M[i, j] != 0.0:
                    t = e[i] * mpf(float(M[i, j])) * e[j]
                    v += t; a += abs(t)
        return v, a
    vals, mags = [], []
    for g in lanes:
        b, c = divmod(g, S)
        v = mpf(0); a = mpf(0)
        for t in range(N + 1):
            goal = ref[t] if (ref is not None and t < N) else xr
            e = [mpf(float(X[b, c, t, i])) - mpf(float(goal[i])) for i in range(p.nx)]
            dv, da = quad(Qdt if t < N else Qf, e)
            v += dv; a += da
            if t < N:
                dv, da = quad(Rdt, [mpf(float(U[b, c, t, i])) for i in range(p.nu)])
                v += dv; a += da
        vals.append(v); mags.append(a)
    return vals, mags


def check_60_digits(p, out, where):
    """Bound: the header orders the sums as  cost += (sx + su),  sx = sum_j (sum_i e_i Q_ij) e_j,  e_i = x_i - ref_i.  A term e_i Q_ij e_j of
    the computed value carries one rounding per factor e (2), one for each of its two products (2), at most nx - 1 for the additions of the
    inner sum and nx - 1 for those of the outer one (2 nx - 2), one for sx + su, and at most N + 1 for the additions of the N + 1 stage
    values: 2 nx + 4 + N at most, below 2 (nx + 2) + N + 2 = k.  (R's terms have nu <= nx in place of nx and no rounded factor.)  With
    u = 2^-53 the computed cost differs from the exact one by at most gamma_k sum |e_i| |M_ij| |e_j|, gamma_k = k u / (1 - k u); the
    two spare roundings of k cover the denominator.  The reference is exact in the doubles X, U the device returned and Q dt, R dt as the
    library forms them (one product each, the one objective_numpy forms)."""
    import mpmath
    vals, mags = objective_60_digits(p, out["X"], out["U"], LANES)
    gamma = (2 * (p.nx + 2) + p.N + 2) * 2.0 ** -53
    worst = 0.0
    for g, v, a in zip(LANES, vals, mags):
        b, c = divmod(g, S)
        err = abs(mpmath.mpf(float(out["cost"][b, c])) - v)
        assert a > 0
        worst = max(worst, float(err / (gamma * a)))
        assert err <= gamma * a, (where, g, float(err), float(gamma * a))
    print("%s: worst error / bound over the six lanes %.3f" % (where, worst))


def _staged_keys():
    return ["manipulator3", "hcw", "euler_attitude", "quaternion_attitude", "mrp_attitude", "twobody", "landing2d", "usv_3dof", "linear_fuel",
            "quadrotor_rate", "spacecraft_nonlinear", "quadrotor13", "quad12", "manip7"]


@pytest.mark.parametrize("model", _staged_keys() + ["cartpole", "forklift"])
def test_objective_in_60_digits(api, scored, model):
    """every model whose objective is staged in LDS (nx^2 + nu^2 + nx > 40), and two hoisted ones as a control: a reference whose
    association is not the kernel's"""
    p, x0, U, out = scored(model)
    assert MC.staged(p) == (model not in ("cartpole", "forklift"))
    check_60_digits(p, out, model)


def test_the_staged_list_is_every_large_model(api):
    assert sorted(_staged_keys()) == sorted(r.key for r in MC.MODELS.values() if MC.staged(MC.build_row(api, r)))


def _quadrotor_tracking(api):
    """the quadrotor (nx = 13) with a reference row per step, every row different (the pattern of test_score_rollouts._pendulum_ref), weights
    of the shipped figure-8 problem, N = 3"""
    N = 3
    q = api.quadrotor_figure8_problem(api.SOLVER_IPDDP, horizon=N)
    ref = np.zeros((N + 1, 13))
    ref[:, 0] = np.linspace(3.0, 2.7, N + 1); ref[:, 1] = np.linspace(0.0, 0.4, N + 1); ref[:, 2] = np.linspace(2.0, 2.2, N + 1)
    ref[:, 3] = np.linspace(1.0, 0.97, N + 1); ref[:, 4] = np.linspace(0.0, 0.05, N + 1); ref[:, 12] = np.linspace(0.1, -0.2, N + 1)
    assert all(not np.array_equal(ref[i], ref[j]) for i in range(N + 1) for j in range(i))
    Q = q.Q.copy(); Q[12, 12] = 0.5; Q[0, 12] = Q[12, 0] = 0.05                  # the last column of the staged block carries weight
    p = api.Problem(api.SOLVER_IPDDP, api.MODEL_QUADROTOR, api.RK4, 13, 4, N, q.dt, Q, q.R, q.Qf, q.x_ref, model_params=list(q.c.model_params)[:6],
                    x_ref_traj=ref, options=q.options)
    p.add_control_box("ControlConstraint", np.zeros(4), 4.0 * np.ones(4))
    p.x0 = q.x0.copy(); p.U0_const = q.U0_const.copy()
    return p


def test_per_step_reference_on_a_staged_objective(api):
    p = _quadrotor_tracking(api)
    assert MC.staged(p) and p.x_ref_traj.shape == (p.N + 1, 13)
    centre, scale = MC.candidate_scale(api, p)
    x0, U = MC.draw(p, [0.02] * 13, centre, scale, 7)
    h = api.HipBatchSolver(p, B)
    out = h.score_rollouts(U, x0=x0, want=("cost", "viol", "X", "U"))
    for c in range(S):
        h.set_initial(x0, np.ascontiguousarray(U[:, c])); h.initialize()
        J = h.results()["final_objective"]
        assert np.isfinite(J).all()
        assert same(out["cost"][:, c], J) and same(out["X"][:, c], h.trajectory()[0]), c
    ref = objective_numpy(p, out["X"], out["U"])
    assert np.isfinite(ref).all() and same(out["cost"], ref), np.abs(out["cost"] - ref).max()
    check_60_digits(p, out, "quadrotor, per-step reference")
    # the reference does enter: the same problem without it scores differently
    q = api.Problem(api.SOLVER_IPDDP, api.MODEL_QUADROTOR, api.RK4, 13, 4, p.N, p.dt, p.Q, p.R, p.Qf, p.x_ref, model_params=list(p.c.model_params)[:6],
                    options=p.options)
    q.add_control_box("ControlConstraint", np.zeros(4), 4.0 * np.ones(4))
    g = api.HipBatchSolver(q, B)
    assert not same(g.score_rollouts(U, x0=x0, want=("cost",))["cost"], out["cost"])
    h.close(); g.close()


def test_staged_block_is_read_to_its_last_element(api):
    """The last element of the staged block Q dt | R dt | x_ref is x_ref[nx - 1].  The shipped builders of the large plants have a zero there
    (or no running weight on that coordinate), so a block staged one element short would go unseen: the 3-link manipulator with a goal
    whose last joint velocity is not zero and running weight on it."""
    row = MC.MODELS["ManipulatorModel"]
    p = MC.build_row(api, row)
    assert MC.staged(p) and p.Q[5, 5] != 0.0
    p.x_ref[3:] = [0.4, -0.3, 0.7]                                                # in place: the descriptor points at this buffer
    centre, scale = MC.candidate_scale(api, p)
    x0, U = MC.draw(p, row.spread, centre, scale, 13)
    h = api.HipBatchSolver(p, B)
    out = h.score_rollouts(U, x0=x0, want=("cost", "X", "U"))
    ref = objective_numpy(p, out["X"], out["U"])
    assert np.isfinite(ref).all() and same(out["cost"], ref), np.abs(out["cost"] - ref).max()
    for c in range(S):
        h.set_initial(x0, np.ascontiguousarray(U[:, c])); h.initialize()
        assert same(out["cost"][:, c], h.results()["final_objective"]), c
    check_60_digits(p, out, "manipulator3, moving goal")
    h.close()


# ---- 4. the constraint rows of every registered set with a constraint part
@pytest.mark.parametrize("name", MC.SET_NAMES)
def test_viol_on_every_constrained_set(api, scored, name):
    p, x0, U, out = scored(name)
    assert MC.set_of(api, p) == name
    ref, lo, hi = viol_reference(api, p, out["X"], out["U"])
    print(name, "rows in [%g, %g]; viol > 0 on %d of %d" % (lo, hi, int((ref > 0).sum()), ref.size))
    assert np.isfinite(ref).all() and np.isfinite(out["X"]).all() and np.isfinite(out["cost"]).all(), name
    assert lo < 0 < hi, (name, lo, hi)                                             # both signs occur among the rows
    assert (ref > 0).any() and (ref == 0).any(), name                              # ... and among the candidates: some violate, some do not
    assert same(out["viol"], ref), (name, np.abs(out["viol"] - ref).max())
    if p._terms:
        # the terminal rows alone take both signs too, and decide the violation of some candidate
        q_ref, _, _ = viol_reference(api, _without_terminal(api, name), out["X"], out["U"])
        assert (q_ref != ref).any() and (q_ref == ref).any(), name


def _without_terminal(api, name):
    p = MC.set_case(api, name)[0]
    p._terms = []
    return p
