"""The device-resident plant (cddp_hip_plant_*, cddp_hip_mpc_run_plant, cddp_hip_track_plan; include/cddp_hip.h "closed loop against a
separate plant").  The header fixes the arithmetic, so every comparison here is np.array_equal:
  1. DevicePlant.step against the plant probe (the gfx950 build of the same Stepper<Model>::step), all 24 plants x 4 integrators, shared
     and per-trajectory parameters;
  2. ... against the C++ oracle's dynamics, with substeps, a control box, a disturbance and three parameter sets;
  3. mpc_run_plant against the loop written out over solve / plan_head / DevicePlant.step / mpc_advance (and, B = 4, the oracle);
  4. the plant being the model: mpc_run_plant against mpc_run;
  5. two tile groups: the batch offsets of W, the parameters and the logs;
  6. track_plan against a host loop over gains() / trajectory() / DevicePlant.step;
  7. refusals that change nothing.
B = 70 is two tiles, the second partial; B = 229 (the probe's point sets) three wavefronts and a partial one."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALES = (1.0, 1.1, 0.9)          # the three parameter sets: every caller entry of the plant times one of these


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def clip(u, lo, up):
    """fmin(fmax(u, lower), upper)"""
    return np.minimum(np.maximum(u, lo), up)


def shift(A):
    return np.ascontiguousarray(np.concatenate([A[:, 1:], A[:, -1:]], axis=1))


# ---- 1. the probe ------------------------------------------------------------------------------------------------------------------
def probe_plant(api, PP, pl, B, integ, params=None):
    kw = dict(lti_A=PP.LTI_A, lti_B=PP.LTI_B) if pl.tag == "lti21" else {}
    return api.DevicePlant(pl.id, integ, pl.dt, pl.nx, pl.nu, B, params=pl.params if params is None else params, **kw)


def probe_tags():
    import plant_probe as PP
    return PP.TAGS


@pytest.mark.parametrize("tag", probe_tags())
def test_step_is_the_probes_step(api, tag):
    import plant_probe as PP
    pl = PP.BY_TAG[tag]
    lib = PP.device()
    x, u = PP.regular_set(pl)
    B = x.shape[0]
    assert B == 229
    for integ in range(4):
        ref = PP.run(lib, "step_" + tag, PP.pack(pl, x, u, integ=integ))[:pl.nx].T
        assert np.all(np.isfinite(ref)), (tag, integ)
        dp = probe_plant(api, PP, pl, B, integ)
        got = dp.step(x, u)
        dp.close()
        assert same(got, ref), (tag, PP.INTEGRATORS[integ], int(np.sum(got != ref)))
    assert not same(got, x)


def parametrised_tags():
    import plant_probe as PP
    return [p.tag for p in PP.PLANTS if len(p.params) > 0]


@pytest.mark.parametrize("tag", parametrised_tags())
def test_per_trajectory_parameters_are_the_probe_run_per_set(api, tag):
    """Three parameter sets cycled over the batch; the reference is the probe run once per set on a copied Plant whose params are that set
    (its p32() derives the block: for the attitude plants three different inverse inertia matrices)."""
    import plant_probe as PP
    pl = PP.BY_TAG[tag]
    lib = PP.device()
    x, u = PP.regular_set(pl)
    B = x.shape[0]
    sets = [np.asarray(pl.params, dtype=np.float64) * s for s in SCALES]
    which = np.arange(B) % 3
    for integ in (0, 3):
        ref = np.zeros((B, pl.nx))
        per_set = []
        for k, ps in enumerate(sets):
            plk = copy.copy(pl); plk.params = list(ps)
            r = PP.run(lib, "step_" + tag, PP.pack(plk, x, u, integ=integ))[:pl.nx].T
            per_set.append(r)
            ref[which == k] = r[which == k]
        assert not same(per_set[0], per_set[1]) and not same(per_set[0], per_set[2]), tag     # the parameters matter at these points
        dp = probe_plant(api, PP, pl, B, integ, params=np.stack([sets[k] for k in which]))
        got = dp.step(x, u)
        dp.close()
        assert same(got, ref), (tag, PP.INTEGRATORS[integ], int(np.sum(got != ref)))


def test_step_on_device_tensors(api):
    import torch
    p = api.cartpole_problem()
    B = 70
    rng = np.random.default_rng(20270101)
    x = rng.normal(0.0, 0.5, (B, p.nx)); u = rng.normal(0.0, 2.0, (B, p.nu)); w = 1e-3 * rng.standard_normal((B, p.nx))
    dp = api.DevicePlant.of_problem(p, B, substeps=3, u_lower=[-1.0], u_upper=[1.5])
    ref = dp.step(x, u, w)
    dev = "cuda:0"
    got = dp.step(torch.from_numpy(x).to(dev), torch.from_numpy(u).to(dev), torch.from_numpy(w).to(dev))
    assert got.is_cuda and same(got.cpu().numpy(), ref)
    assert same(dp.step(torch.from_numpy(x).to(dev), torch.from_numpy(u).to(dev)).cpu().numpy(), dp.step(x, u))
    dp.close()


# ---- 2. the oracle -----------------------------------------------------------------------------------------------------------------
ORACLE_PLANTS = {"pendulum": "pendulum_problem", "cartpole": "cartpole_problem", "unicycle": "unicycle_problem", "bicycle": "bicycle_problem"}
N_PARAMS = {"pendulum": 4, "cartpole": 5, "unicycle": 0, "bicycle": 1}


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("name", list(ORACLE_PLANTS))
def test_step_is_the_oracles_dynamics(api, oracle_built, name, substeps):
    """substeps applications of the oracle's discrete dynamics (the problem with the trajectory's parameters and dt / substeps) to the
    clipped control, plus w.  The unicycle has no parameters: its three "sets" are one, and only the other plants are asked to differ."""
    p = getattr(api, ORACLE_PLANTS[name])()
    B = 70
    npar = N_PARAMS[name]
    integ = api.RK4 if substeps == 3 else int(p.c.integrator)
    base = np.array(list(p.c.model_params)[:npar])
    sets = [base * s for s in SCALES]
    which = np.arange(B) % 3
    rng = np.random.default_rng(20270102 + substeps)
    x = rng.normal(0.0, 0.5, (B, p.nx)); u = rng.normal(0.0, 1.0, (B, p.nu)); w = 1e-2 * rng.standard_normal((B, p.nx))
    lo, up = -0.6 * np.ones(p.nu), 0.4 * np.ones(p.nu)
    us = clip(u, lo, up)
    assert np.any(us != u) and np.any(us == u)                      # some lanes clipped, some not
    dt = float(p.c.dt)
    oracles = []
    for ps in sets:
        q = getattr(api, ORACLE_PLANTS[name])()
        for i, v in enumerate(ps):
            q.c.model_params[i] = float(v)
        q.c.dt = dt / substeps; q.c.integrator = integ
        oracles.append((q, api.Oracle(q)))
    ref = np.zeros((B, p.nx)); ref0 = np.zeros((B, p.nx))
    for b in range(B):
        for k, dst in ((which[b], ref), (0, ref0)):
            xb = x[b].copy()
            for _ in range(substeps):
                xb = oracles[k][1].dynamics(xb, us[b])[1]
            dst[b] = xb + w[b]
    if npar:
        assert np.all(np.any(ref[which != 0] != ref0[which != 0], axis=1)), name      # the other two sets give other states
    params = np.stack([sets[k] for k in which]) if npar else []
    dp = api.DevicePlant(int(p.c.model), integ, dt, p.nx, p.nu, B, params=params, substeps=substeps, u_lower=lo, u_upper=up)
    got = dp.step(x, u, w)
    dp.close()
    assert same(got, ref), (name, substeps, int(np.sum(got != ref)))


# ---- 3. the loop is the hand-written loop --------------------------------------------------------------------------------------------
def plant_loop(api, h, plant, steps, mode, shift_duals=False, W=None, box=None, heads=None):
    """cddp_hip_mpc_run_plant written out; also the seed of every solve after the first and the model's own x_1 of every step (and, into the
    list `heads`, the handle's own u_0 of every step: the control before the plant's box)"""
    B = h.B
    U = np.zeros((B, steps, h.p.nu)); X = np.zeros((B, steps + 1, h.p.nx))
    it = np.zeros((B, steps), dtype=np.int32); st = np.zeros((B, steps), dtype=np.int32)
    seeds, model_x1 = [], []
    n_it = 0
    for k in range(steps):
        s = h.solve(); n_it += int(s.traj_iterations)
        u0, x1 = h.plan_head(); r = h.results()
        Xp, Up = h.trajectory()
        xn = plant.step(np.ascontiguousarray(Xp[:, 0]), u0, None if W is None else np.ascontiguousarray(W[:, k]))
        U[:, k] = u0 if box is None else clip(u0, box[0], box[1])
        X[:, k + 1] = xn; it[:, k] = r["iterations"]; st[:, k] = r["status"]
        model_x1.append(x1)
        if heads is not None:
            heads.append(u0)
        Xs, Us = shift(Xp), shift(Up); Xs[:, 0] = xn
        seeds.append((Xs, Us))
        h.mpc_advance(mode, x_next=xn, shift_duals=shift_duals)
    return U, X, it, st, seeds, model_x1, n_it


def check_loop(api, p, B, mode, make_plant, steps=3, shift_duals=False, W=None, box=None, seed=20270103, spread=None, x0=None):
    import test_gpu_parity as T
    p.options.warm_start = 1
    if x0 is None:
        x0 = api.batch_x0(p, B, seed, T.spread_for(p) if spread is None else spread)
    U0 = api.batch_U0(p, B)
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0)
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0)
    pa, pb = make_plant(), make_plant()
    U, X, it, st, seeds, model_x1, n_it = plant_loop(api, a, pa, steps, mode, shift_duals, W, box)
    X[:, 0] = x0
    r = b.mpc_run_plant(pb, steps, mode, shift_duals=shift_duals, W=W)
    assert same(r["U_applied"], U), int(np.sum(r["U_applied"] != U))
    assert same(r["X_visited"], X), int(np.sum(r["X_visited"] != X))
    assert same(r["iterations"], it) and same(r["status"], st)
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    assert same(Xa, Xb) and same(Ua, Ub)
    assert r["stats"].traj_iterations == n_it == int(it.sum()) and r["stats"].solve_ms > 0.0
    # the plant is not the model: on every trajectory the state the second solve starts from is not the plan's own x_1
    assert np.all(np.any(r["X_visited"][:, 1] != model_x1[0], axis=1))
    ng = (a.num_groups(), b.num_groups())
    a.close(); b.close(); pa.close(); pb.close()
    return r, seeds, x0, U0, ng


def scaled_params(p, index, factor):
    ps = list(p.c.model_params)
    ps[index] = ps[index] * factor
    return ps


def test_loop_pendulum_provided_and_the_oracle(api, oracle_built):
    import test_gpu_parity as T
    p = T.make(api, "pendulum_ipddp_box")
    B, steps = 4, 3
    r, seeds, x0, U0, _ = check_loop(api, p, B, api.MPC_SHIFT_PROVIDED, steps=steps,
                                     make_plant=lambda: api.DevicePlant.of_problem(p, B, params=scaled_params(p, 1, 1.2), substeps=2))
    # every step of the "provided" loop is a NEW solver object given the shifted plan whose row 0 is the plant's state
    for k in range(steps):
        for i in range(B):
            o = api.Oracle(p); o.set_warm_start(True)
            if k == 0:
                o.set_initial(x0[i], np.zeros((p.N, p.nu)) if U0 is None else U0[i], np.tile(x0[i], (p.N + 1, 1)))
            else:
                Xs, Us = seeds[k - 1]
                o.set_initial(Xs[i, 0], Us[i], Xs[i])
            q = o.solve()
            assert q["iterations"] == r["iterations"][i, k] and q["status"] == r["status"][i, k], (k, i, q["iterations"], r["iterations"][i, k])


def test_loop_unicycle_existing_shift_duals_rk4_disturbed(api):
    import test_gpu_parity as T
    p = T.make(api, "unicycle_ipddp_box_ball")
    B, steps = 70, 3
    assert int(p.c.integrator) != api.RK4
    W = 1e-3 * np.random.default_rng(20270104).standard_normal((B, steps, p.nx))
    check_loop(api, p, B, api.MPC_SHIFT_EXISTING, steps=steps, shift_duals=True, W=W,
               make_plant=lambda: api.DevicePlant.of_problem(p, B, integrator=api.RK4))


def test_loop_pendulum_clddp_keep_plan_saturated(api):
    """A saturation tighter than the problem's box: half the smallest |u_0| of the first plan (read from a scratch handle), so the plant
    receives another control than the model on EVERY trajectory."""
    import test_gpu_parity as T
    p = T.make(api, "pendulum_clddp_box")
    B = 70
    p.options.warm_start = 1
    x0 = api.batch_x0(p, B, 20270105, T.spread_for(p))
    c = api.HipBatchSolver(p, B); c.set_initial(x0, api.batch_U0(p, B)); c.solve()
    u0 = c.plan_head()[0]; c.close()
    bound = 0.5 * float(np.min(np.abs(u0)))
    assert bound > 0.0
    box = (np.array([-bound]), np.array([bound]))
    r, *_ = check_loop(api, p, B, api.MPC_KEEP_PLAN, x0=x0, box=box,
                       make_plant=lambda: api.DevicePlant.of_problem(p, B, u_lower=box[0], u_upper=box[1]))
    assert np.all(np.abs(r["U_applied"][:, 0]) == bound)


def test_loop_logddp(api):
    import test_logddp_device as LG
    p = LG.make(api, "pendulum_box")
    B = 70
    check_loop(api, p, B, api.MPC_SHIFT_PROVIDED, spread=0.1 * np.ones(p.nx),
               make_plant=lambda: api.DevicePlant.of_problem(p, B, params=scaled_params(p, 1, 1.2), substeps=2))


# ---- 4. identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pendulum_ipddp_box", "unicycle_ipddp_box_ball"])
def test_the_model_as_the_plant_is_mpc_run(api, case):
    import test_gpu_parity as T
    p = T.make(api, case)
    p.options.warm_start = 1
    B, steps = 70, 3
    x0 = api.batch_x0(p, B, 20270106, T.spread_for(p)); U0 = api.batch_U0(p, B)
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0)
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0)
    dp = api.DevicePlant.of_problem(p, B)
    ra = a.mpc_run(steps, api.MPC_SHIFT_PROVIDED)
    rb = b.mpc_run_plant(dp, steps, api.MPC_SHIFT_PROVIDED)
    for key in ("U_applied", "X_visited", "iterations", "status"):
        assert same(ra[key], rb[key]), (case, key, int(np.sum(ra[key] != rb[key])))
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    assert same(Xa, Xb) and same(Ua, Ub)
    assert ra["stats"].traj_iterations == rb["stats"].traj_iterations
    a.close(); b.close(); dp.close()


# ---- 5. two tile groups --------------------------------------------------------------------------------------------------------------
def test_two_tile_groups_offset_parameters_disturbances_and_logs(api, monkeypatch):
    import test_gpu_parity as T
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    p = T.make(api, "pendulum_ipddp_box")
    B, steps = 130, 3
    rng = np.random.default_rng(20270107)
    base = np.array(list(p.c.model_params)[:4])
    params = np.tile(base, (B, 1))
    params[:, 1] *= 1.05 + 0.3 * rng.random(B)                  # a mass of its own for every trajectory
    params[:, 0] *= 1.0 + 0.002 * np.arange(B)                  # ... and a length
    W = 1e-3 * rng.standard_normal((B, steps, p.nx))
    assert len(np.unique(params[:, 1])) == B and len(np.unique(W[:, 0, 0])) == B
    *_, ng = check_loop(api, p, B, api.MPC_SHIFT_PROVIDED, steps=steps, W=W,
                        make_plant=lambda: api.DevicePlant.of_problem(p, B, params=params, substeps=2))
    assert ng == (2, 2)


# ---- 6. tracking ---------------------------------------------------------------------------------------------------------------------
def host_track(h, plant, x0, W, box):
    """u_t = U_t + K_t (x_t - X_t), the sum over j ascending from a zero accumulator, scalar by scalar (the batch is the only vector axis)"""
    K, _ = h.gains(); X, U = h.trajectory()
    B, N, nu, nx = K.shape
    x = np.ascontiguousarray(X[:, 0] if x0 is None else x0).copy()
    Xo = np.zeros((B, N + 1, nx)); Uo = np.zeros((B, N, nu)); Xo[:, 0] = x
    clipped = 0
    for t in range(N):
        dx = np.zeros((B, nx))
        for j in range(nx):
            dx[:, j] = x[:, j] - X[:, t, j]
        u = np.zeros((B, nu))
        for i in range(nu):
            s = np.zeros(B)
            for j in range(nx):
                s = s + K[:, t, i, j] * dx[:, j]
            u[:, i] = U[:, t, i] + s
        x = plant.step(x, u, None if W is None else np.ascontiguousarray(W[:, t]))
        us = u if box is None else clip(u, box[0], box[1])
        clipped += int(np.sum(us != u))
        Uo[:, t] = us; Xo[:, t + 1] = x
    return Xo, Uo, clipped


@pytest.mark.parametrize("case", ["pendulum_ipddp_box", "unicycle_ipddp_box_ball"])
def test_track_plan_is_the_host_loop(api, case):
    import test_gpu_parity as T
    import test_mpc_advance as M
    p = T.make(api, case)
    B = 70
    a, b, x0, U0 = M.pair(api, p, B, 20270108)                      # two solved handles; b never tracks
    Xp, Up = a.trajectory(); Kp, kp = a.gains()
    rng = np.random.default_rng(20270108)
    xs = np.ascontiguousarray(Xp[:, 0] + 1e-2 * rng.standard_normal((B, p.nx)))
    W = 1e-3 * rng.standard_normal((B, p.N, p.nx))
    bound = 0.8 * np.max(np.abs(Up), axis=(0, 1))                   # inside the plan's own range: the tracking controls reach it
    box = (-bound, bound)
    dp = api.DevicePlant.of_problem(p, B, substeps=2, integrator=api.RK4, u_lower=box[0], u_upper=box[1])
    Xr, Ur, clipped = host_track(a, dp, xs, W, box)
    assert clipped > 0
    Xo, Uo = a.track_plan(dp, x0=xs, W=W)
    assert same(Xo, Xr), int(np.sum(Xo != Xr))
    assert same(Uo, Ur), int(np.sum(Uo != Ur))
    assert same(Xo[:, 0], xs) and np.all(np.abs(Uo) <= bound)
    dp.close()
    # the model as the plant, from the plan's own start: the plan itself
    dm = api.DevicePlant.of_problem(p, B)
    Xo, Uo = a.track_plan(dm)
    assert same(Xo, Xp) and same(Uo, Up)
    dm.close()
    # the handle was only read
    Xa, Ua = a.trajectory(); Ka, ka = a.gains()
    assert same(Xa, Xp) and same(Ua, Up) and same(Ka, Kp) and same(ka, kp)
    Xb, Ub = b.trajectory(); Kb, kb = b.gains()
    assert same(Xa, Xb) and same(Ua, Ub) and same(Ka, Kb) and same(ka, kb)
    a.solve(); b.solve()
    M.assert_same_solve(a, b, (case, "a solve after tracking"), duals=True)
    a.close(); b.close()


# ---- 7. refusals that change nothing -------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(api):
    import test_gpu_parity as T
    import test_mpc_advance as M
    lib = api.load_hip()
    p = T.make(api, "pendulum_ipddp_box")
    B = 70
    x0 = api.batch_x0(p, B, 20270109, T.spread_for(p)); U0 = api.batch_U0(p, B)
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0); a.solve()
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0)
    good = api.DevicePlant.of_problem(p, B)
    other_nx = api.DevicePlant.of_problem(api.cartpole_problem(), B)
    other_batch = api.DevicePlant.of_problem(p, B + 1)

    def refused(call, *words):
        with pytest.raises(api.HipError) as e:
            call()
        msg = lib.cddp_hip_last_error().decode()
        assert len(msg) > 0 and all(w in msg for w in words), (msg, words)
        assert msg in str(e.value)

    refused(lambda: b.track_plan(good), "cddp_hip_track_plan", "solved")                     # never solved: no plan, no gains
    b.solve()
    M.assert_same_solve(a, b, "after the early refusal", duals=True)
    refused(lambda: b.mpc_run_plant(other_nx, 2, api.MPC_SHIFT_PROVIDED), "nx = 4")
    refused(lambda: b.track_plan(other_nx), "nx = 4")
    refused(lambda: b.mpc_run_plant(other_batch, 2, api.MPC_SHIFT_PROVIDED), "batch of %d" % (B + 1))
    refused(lambda: b.track_plan(other_batch), "batch of %d" % (B + 1))
    refused(lambda: b.mpc_run_plant(good, 2, 7), "unknown mode 7")
    refused(lambda: b.mpc_run_plant(good, 0, api.MPC_SHIFT_PROVIDED), "steps must be positive")
    refused(lambda: b.mpc_run_plant(good, 2, api.MPC_KEEP_PLAN, shift_duals=True), "SHIFT_DUALS")
    refused(lambda: b.mpc_run_plant(None, 2, api.MPC_SHIFT_PROVIDED), "null plant")
    good.close()
    refused(lambda: b.track_plan(good), "null plant")                                        # a closed plant is no plant
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    assert same(Xa, Xb) and same(Ua, Ub)
    a.solve(); b.solve()
    M.assert_same_solve(a, b, "after the refusals", duals=True)
    a.close(); b.close(); other_nx.close(); other_batch.close()


def test_facade_solve_mpc_batch_with_a_plant(api):
    import test_gpu_parity as T
    import test_mpc_advance as M
    pycddp = M._facade()
    p = T.make(api, "pendulum_ipddp_box")
    B, steps = 8, 3
    x0 = api.batch_x0(p, B, 20270110, T.spread_for(p))
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False
    o.max_iterations = p.options.max_iterations; o.tolerance = p.options.tolerance; o.acceptable_tolerance = p.options.acceptable_tolerance
    o.regularization.initial_value = p.options.reg_initial_value
    sv = pycddp.CDDP(x0[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.Pendulum(p.dt, *list(p.c.model_params)[:3], "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    sv.add_constraint("ControlConstraint", pycddp.ControlConstraint(np.array([-20.0]), np.array([20.0])))
    pp = sv._problem(api.SOLVER_IPDDP); pp.options.warm_start = 1
    W = 1e-3 * np.random.default_rng(20270110).standard_normal((B, steps, p.nx))
    params = scaled_params(pp, 1, 1.2)[:4]
    out = sv.solve_mpc_batch(list(x0), steps, pycddp.SolverType.IPDDP, plant={"params": params, "substeps": 2, "integrator": "rk4",
                                                                              "u_lower": [-5.0], "u_upper": [5.0]}, disturbances=W)
    h = api.HipBatchSolver(pp, B); h.set_initial(x0)
    dp = api.DevicePlant.of_problem(pp, B, params=params, substeps=2, integrator=api.RK4, u_lower=[-5.0], u_upper=[5.0])
    r = h.mpc_run_plant(dp, steps, api.MPC_SHIFT_PROVIDED, W=W); h.close(); dp.close()
    assert same(out["state_trajectory"], r["X_visited"]) and same(out["control_trajectory"], r["U_applied"]) and same(out["iterations"], r["iterations"])
    # plant=None is today's call
    out0 = sv.solve_mpc_batch(list(x0), steps, pycddp.SolverType.IPDDP)
    h = api.HipBatchSolver(pp, B); h.set_initial(x0)
    r0 = h.mpc_run(steps, api.MPC_SHIFT_PROVIDED); h.close()
    assert same(out0["state_trajectory"], r0["X_visited"]) and same(out0["control_trajectory"], r0["U_applied"])
    assert not same(out["state_trajectory"], out0["state_trajectory"])
