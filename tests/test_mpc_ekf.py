"""The MPC loop closed through the device-resident extended Kalman filter (cddp_hip_mpc_run_ekf; include/cddp_hip.h "extended Kalman
filter on the device; the MPC loop closed through it").  Every comparison is np.array_equal:
  1. unicycle and cart-pole (N = 20), B = 65, steps = 3, SHIFT_PROVIDED and SHIFT_EXISTING, a plant that differs from the estimator's model
     (cart-pole: one parameter; unicycle, which has none: the integrator), W and Yn given: every output against the loop written out over
     the public entries -- ekf update / get, mpc_advance, solve, plan_head, DevicePlant.step, ekf predict, y formed in numpy as the header
     states it -- and a following solve against the twin handle that loop drove;
  2. C = I, no measurement noise, a tiny v: the run stays finite and the estimate tracks the true state (a sanity check: the gap is printed);
  3. the refusals, which change nothing;
  4. the facade: CDDP.solve_mpc_batch(..., estimator=..., meas_noise=...) is the direct call."""
import numpy as np
import pytest

import plan_ekf_ref as PE

pytestmark = pytest.mark.gpu

B, STEPS, N = 65, 3, 20


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def clip(u, lo, up):
    return u if lo is None else np.minimum(np.maximum(u, lo), up)


def problem(api, name):
    p = api.unicycle_problem(api.SOLVER_IPDDP, horizon=N, obstacle=False) if name == "unicycle" else api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N)
    p.options.warm_start = 1
    return p


def plants(api, p, name):
    """-> (the true plant, the estimator's model, the true plant's box)"""
    if name == "unicycle":
        box = (np.array([-0.8, -0.6]), np.array([0.9, 0.7]))
        return (lambda: api.DevicePlant.of_problem(p, B, integrator=api.RK4, u_lower=box[0], u_upper=box[1])), (lambda: api.DevicePlant.of_problem(p, B)), box
    ps = list(p.c.model_params); ps[1] = ps[1] * 1.2                          # the pole is a fifth heavier than the filter believes
    return (lambda: api.DevicePlant.of_problem(p, B, params=ps)), (lambda: api.DevicePlant.of_problem(p, B)), None


def sensors(p, seed):
    rng = np.random.default_rng(seed)
    ny = p.nx - 1
    C = np.eye(p.nx)[:ny] + 0.1 * rng.standard_normal((ny, p.nx))
    v = 1e-4 * (1.0 + rng.random(ny))
    W = 1e-6 * np.eye(p.nx); Wu = 1e-4 * np.eye(p.nu)
    noise = 1e-3 * rng.standard_normal((B, STEPS, p.nx))
    Yn = 1e-2 * rng.standard_normal((B, STEPS + 1, ny))
    return C, v, W, Wu, noise, Yn


def written_out(api, h, plant, ekf, mode, x0_true, C, W, Yn, box, shift_duals=False):
    """cddp_hip_mpc_run_ekf over the public entries"""
    x = x0_true.copy()
    Cb = PE.batched(C, B, C.shape)
    U = np.zeros((B, STEPS, h.p.nu)); X = np.zeros((B, STEPS + 1, h.p.nx)); Xh = np.zeros((B, STEPS, h.p.nx)); nis = np.zeros((B, STEPS))
    it = np.zeros((B, STEPS), dtype=np.int32); st = np.zeros((B, STEPS), dtype=np.int32)
    X[:, 0] = x
    for k in range(STEPS):
        y = PE.measure(Cb, x, None if Yn is None else Yn[:, k])
        nis[:, k] = ekf.update(y)
        xh = ekf.get()[0]
        Xh[:, k] = xh
        if k == 0:
            h.mpc_advance(api.MPC_KEEP_PLAN, x_next=xh)
        else:
            h.mpc_advance(mode, x_next=xh, shift_duals=shift_duals)
        h.solve()
        r = h.results()
        u0, _ = h.plan_head()
        x = plant.step(x, u0, None if W is None else np.ascontiguousarray(W[:, k]))
        ekf.predict(u0)
        U[:, k] = clip(u0, *(box if box else (None, None))); X[:, k + 1] = x; it[:, k] = r["iterations"]; st[:, k] = r["status"]
    return {"U_applied": U, "X_visited": X, "Xh_visited": Xh, "nis": nis, "iterations": it, "status": st}


@pytest.mark.parametrize("name,mode", [("unicycle", "MPC_SHIFT_PROVIDED"), ("unicycle", "MPC_SHIFT_EXISTING"), ("cartpole", "MPC_SHIFT_PROVIDED"),
                                       ("cartpole", "MPC_SHIFT_EXISTING")])
def test_run_is_the_loop_over_the_public_entries(api, name, mode):
    import test_gpu_parity as T
    import test_mpc_advance as M
    mode = getattr(api, mode)
    p = problem(api, name)
    x0 = api.batch_x0(p, B, 20261090, T.spread_for(p)); U0 = api.batch_U0(p, B)
    C, v, W, Wu, noise, Yn = sensors(p, 20261091)
    make_plant, make_model, box = plants(api, p, name)
    xh0 = x0 + 0.01 * np.random.default_rng(20261092).standard_normal(x0.shape)
    P0 = 1e-4 * np.eye(p.nx)
    out = []
    handles = []
    for which in ("loop", "run"):
        h = api.HipBatchSolver(p, B); h.set_initial(xh0, U0); h.initialize()
        plant, model = make_plant(), make_model()
        ekf = api.DeviceEkf(model, C, v, W, Wu)
        ekf.reset(xh0, P0)
        if which == "loop":
            r = written_out(api, h, plant, ekf, mode, x0, C, noise, Yn, box)
        else:
            r = h.mpc_run_ekf(plant, ekf, STEPS, mode, x0, W=noise, Yn=Yn)
            assert r["stats"].traj_iterations == int(r["iterations"].sum()) and r["stats"].solve_ms > 0.0
        r["state"] = ekf.get()
        out.append(r); handles.append((h, plant, model, ekf))
    a, b = out
    for k in ("U_applied", "X_visited", "Xh_visited", "nis", "iterations", "status"):
        assert same(a[k], b[k]), (k, int(np.sum(np.asarray(a[k]) != np.asarray(b[k]))))
    assert all(same(s, t) for s, t in zip(a["state"], b["state"]))              # the estimator is left after the last prediction
    assert np.all(np.isfinite(b["X_visited"])) and np.all(np.isfinite(b["Xh_visited"])) and np.all(b["nis"] >= 0.0) and not b["state"][2].any()
    assert same(b["X_visited"][:, 0], x0) and not same(b["Xh_visited"], b["X_visited"][:, :-1])
    if box:
        assert np.all(b["U_applied"] >= box[0]) and np.all(b["U_applied"] <= box[1])
    (ha, *_), (hb, *_) = handles
    M.assert_same_solve(ha, hb, "after the run", duals=True)
    ha.solve(); hb.solve()
    M.assert_same_solve(ha, hb, "the following solve", duals=True)
    for h, plant, model, ekf in handles:
        ekf.close(); model.close(); plant.close(); h.close()


def test_perfect_sensors_track_the_true_state(api):
    import test_gpu_parity as T
    p = problem(api, "unicycle")
    x0 = api.batch_x0(p, B, 20261093, T.spread_for(p))
    h = api.HipBatchSolver(p, B); h.set_initial(x0, api.batch_U0(p, B)); h.initialize()
    plant = api.DevicePlant.of_problem(p, B); model = api.DevicePlant.of_problem(p, B)
    ekf = api.DeviceEkf(model, np.eye(p.nx), np.full(p.nx, 1e-12), 1e-8 * np.eye(p.nx))
    ekf.reset(x0, 1e-2 * np.eye(p.nx))
    r = h.mpc_run_ekf(plant, ekf, 5, api.MPC_SHIFT_EXISTING, x0)
    assert np.all(np.isfinite(r["X_visited"])) and np.all(np.isfinite(r["Xh_visited"])) and np.all(np.isfinite(r["nis"]))
    gap = float(np.max(np.abs(r["Xh_visited"] - r["X_visited"][:, :-1])))
    print("perfect sensors: largest |xh - x| over 5 steps of %d trajectories: %.3e" % (B, gap))
    assert gap < 1e-6                                                          # (sanity: an estimate that ignored y would be off by the step length, ~1e-2)
    ekf.close(); model.close(); plant.close(); h.close()


def test_refusals_change_nothing(api):
    import test_gpu_parity as T
    import test_mpc_advance as M
    lib = api.load_hip()
    p = problem(api, "unicycle")
    x0 = api.batch_x0(p, B, 20261094, T.spread_for(p)); U0 = api.batch_U0(p, B)
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0); a.solve()
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0)
    plant = api.DevicePlant.of_problem(p, B); model = api.DevicePlant.of_problem(p, B)
    C, v = np.eye(p.nx), np.full(p.nx, 1e-3)
    ekf = api.DeviceEkf(model, C, v); ekf.reset(x0, np.eye(p.nx))
    pc = problem(api, "cartpole")
    model_nx = api.DevicePlant.of_problem(pc, B); ekf_nx = api.DeviceEkf(model_nx, np.eye(4), np.full(4, 1e-3))
    model_b = api.DevicePlant.of_problem(p, B + 1); ekf_b = api.DeviceEkf(model_b, C, v)
    before = ekf.get()

    def refused(call, *words):
        with pytest.raises(api.HipError) as e:
            call()
        msg = lib.cddp_hip_last_error().decode()
        assert len(msg) > 0 and all(w in msg for w in words), (msg, words)
        assert msg in str(e.value)

    refused(lambda: b.mpc_run_ekf(plant, ekf, 2, api.MPC_SHIFT_PROVIDED, x0), "needs a current plan")       # never initialised: no plan to advance
    b.solve()
    M.assert_same_solve(a, b, "after the early refusal", duals=True)
    refused(lambda: b.mpc_run_ekf(plant, ekf_nx, 2, api.MPC_SHIFT_PROVIDED, x0), "cddp_hip_mpc_run_ekf", "the estimator has nx = 4")
    refused(lambda: b.mpc_run_ekf(plant, ekf_b, 2, api.MPC_SHIFT_PROVIDED, x0), "the estimator was created for a batch of %d" % (B + 1))
    refused(lambda: b.mpc_run_ekf(plant, None, 2, api.MPC_SHIFT_PROVIDED, x0), "null estimator")
    refused(lambda: b.mpc_run_ekf(None, ekf, 2, api.MPC_SHIFT_PROVIDED, x0), "null plant")
    refused(lambda: b.mpc_run_ekf(model_b, ekf, 2, api.MPC_SHIFT_PROVIDED, x0), "batch of %d" % (B + 1))
    refused(lambda: b.mpc_run_ekf(plant, ekf, 0, api.MPC_SHIFT_PROVIDED, x0), "steps must be positive")
    refused(lambda: b.mpc_run_ekf(plant, ekf, 2, 7, x0), "unknown mode 7")
    refused(lambda: b.mpc_run_ekf(plant, ekf, 2, api.MPC_KEEP_PLAN, x0, shift_duals=True), "SHIFT_DUALS")
    refused(lambda: b.mpc_run_ekf(plant, ekf, 2, api.MPC_SHIFT_PROVIDED, None), "null x0_true")
    bad = x0.copy(); bad[3, 1] = np.inf
    refused(lambda: b.mpc_run_ekf(plant, ekf, 2, api.MPC_SHIFT_PROVIDED, bad), "x0_true holds a non-finite value")
    refused(lambda: b.mpc_run_ekf(plant, ekf, 2, api.MPC_SHIFT_PROVIDED, x0, W=np.full((B, 2, p.nx), np.nan)), "W holds a non-finite value")
    refused(lambda: b.mpc_run_ekf(plant, ekf, 2, api.MPC_SHIFT_PROVIDED, x0, Yn=np.full((B, 3, p.nx), np.nan)), "only with CDDP_HIP_MPC_EKF_SKIP_NAN")
    assert all(PE.same(s, t) for s, t in zip(before, ekf.get()))
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    assert same(Xa, Xb) and same(Ua, Ub)
    a.solve(); b.solve()
    M.assert_same_solve(a, b, "after the refusals", duals=True)
    for o in (ekf, ekf_nx, ekf_b, model, model_nx, model_b, plant, a, b):
        o.close()


def test_facade_solve_mpc_batch_with_an_estimator(api):
    import test_gpu_parity as T
    import test_mpc_advance as M
    pycddp = M._facade()
    p = T.make(api, "pendulum_ipddp_box")
    Bf, steps = 8, 3
    x0 = api.batch_x0(p, Bf, 20261095, T.spread_for(p))
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False
    o.max_iterations = p.options.max_iterations; o.tolerance = p.options.tolerance; o.acceptable_tolerance = p.options.acceptable_tolerance
    o.regularization.initial_value = p.options.reg_initial_value
    sv = pycddp.CDDP(x0[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.Pendulum(p.dt, *list(p.c.model_params)[:3], "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    sv.add_constraint("ControlConstraint", pycddp.ControlConstraint(np.array([-20.0]), np.array([20.0])))
    pp = sv._problem(api.SOLVER_IPDDP); pp.options.warm_start = 1
    rng = np.random.default_rng(20261096)
    W = 1e-3 * rng.standard_normal((Bf, steps, p.nx)); Yn = 1e-2 * rng.standard_normal((Bf, steps + 1, 1))
    ps = list(pp.c.model_params)[:4]; ps[1] = ps[1] * 1.2
    C, v, Wf, P0 = np.array([[1.0, 0.2]]), np.array([1e-4]), 1e-6 * np.eye(2), 1e-3 * np.eye(2)
    out = sv.solve_mpc_batch(list(x0), steps, pycddp.SolverType.IPDDP, plant={"params": ps, "integrator": "rk4"}, disturbances=W,
                             estimator={"C": C, "v": v, "W": Wf, "P0": P0}, meas_noise=Yn)
    h = api.HipBatchSolver(pp, Bf); h.set_initial(x0); h.initialize()
    dp = api.DevicePlant.of_problem(pp, Bf, params=ps, integrator=api.RK4); mp = api.DevicePlant.of_problem(pp, Bf)
    ekf = api.DeviceEkf(mp, C, v, Wf); ekf.reset(x0, P0)
    r = h.mpc_run_ekf(dp, ekf, steps, api.MPC_SHIFT_PROVIDED, x0, W=W, Yn=Yn)
    ekf.close(); mp.close(); dp.close(); h.close()
    assert same(out["state_trajectory"], r["X_visited"]) and same(out["control_trajectory"], r["U_applied"]) and same(out["iterations"], r["iterations"])
    assert same(out["estimate_trajectory"], r["Xh_visited"]) and same(out["nis"], r["nis"]) and np.all(np.isfinite(out["estimate_trajectory"]))
    with pytest.raises(ValueError, match="pass estimator"):
        sv.solve_mpc_batch(list(x0), steps, pycddp.SolverType.IPDDP, plant={}, meas_noise=Yn)
    with pytest.raises(ValueError, match="observes a plant"):
        sv.solve_mpc_batch(list(x0), steps, pycddp.SolverType.IPDDP, estimator={"C": C, "v": v})
    with pytest.raises(ValueError, match="C and v must be given"):
        sv.solve_mpc_batch(list(x0), steps, pycddp.SolverType.IPDDP, plant={}, estimator={"C": C})
