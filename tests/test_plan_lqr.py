"""Time-varying LQR gains along a solved plan on the device (cddp_hip_plan_tvlqr; csrc/inst_lqr.hip).

The header fixes the arithmetic, so the contract is BITWISE: the reference of every bitwise check is tests/plan_lqr_ref.py (the numpy
restatement that tests/test_plan_lqr_host.py holds to the C++ step bodies and to exact evaluation), fed by get_linearization of the same
handle and by the problem's own Q dt, R dt and Qf where a weight is not given.  Comparisons are by value with NaN = NaN (the header
leaves the sign of an exact zero open).  Shapes: B = 70 (two tiles, the last partial) unless a test says otherwise, N <= 5.

The one tolerance that is not bitwise (the LTI identity with cddp_hip_plan_covariance) is 8 x plan_lqr_ref.MEASURED_REL_DEV_IDENTITY,
the value measured against exact evaluation on the CPU."""
import numpy as np
import pytest

import plan_cov_ref as PC
import plan_lqr_ref as PL
from plan_lqr_ref import same
from test_plan_sens import dev, ref_jvp, solved, stacks, torch_

pytestmark = pytest.mark.gpu

B = 70


def weights(p, seed, per, b=B):
    """(Q, R, Qf): symmetric positive definite, unscaled, with junk above the diagonal -- only the lower triangles may be read"""
    rng = np.random.default_rng(seed)
    lead = (b,) if per else ()
    out = []
    for n, scale in ((p.nx, 1.0), (p.nu, 0.5), (p.nx, 3.0)):
        M = PC.spd(rng, n, scale, lead)
        out.append(np.ascontiguousarray(np.tril(M) + np.triu(rng.standard_normal(lead + (n, n)), 1)))
    return out


def reference(h, Q, R, Qf):
    A, Bm, _ = stacks(h)
    assert np.abs(A).max() > 0 and np.abs(Bm).max() > 0                                   # the sweep has left stacks to read
    Qdt, Rdt, Qf0 = PC.cost_matrices(h.p)
    return PL.tvlqr(A, Bm, Qdt if Q is None else Q * h.p.dt, Rdt if R is None else R * h.p.dt, Qf0 if Qf is None else Qf)


def check(h, Q, R, Qf, where, kinds=("host", "device"), ref=None):
    rK, rP, ri = ref if ref is not None else reference(h, Q, R, Qf)
    for kind in kinds:
        conv = dev if kind == "device" else (lambda a: a)
        out = h.plan_tvlqr(conv(Q), conv(R), conv(Qf), device=kind == "device")
        if kind == "device":
            t = torch_()
            assert all(v.is_cuda and v.is_contiguous() for v in out.values()) and out["K"].dtype == t.float64 and out["info"].dtype == t.int32, where
        else:
            assert all(isinstance(v, np.ndarray) for v in out.values()) and out["info"].dtype == np.int32, where
        assert sorted(out) == ["K", "P", "info"]
        assert tuple(out["K"].shape) == rK.shape and tuple(out["P"].shape) == rP.shape and tuple(out["info"].shape) == ri.shape, (where, kind)
        assert same(out["info"], ri), (where, kind, "info")
        assert same(out["K"], rK), (where, kind, "K")
        assert same(out["P"], rP), (where, kind, "P")
    return rK, rP, ri


def cartpole_handle(api, solver, N=5, b=B, seed=20262001):
    p = api.cartpole_problem(solver, True, horizon=N)
    p.options.max_iterations = 3
    return solved(api, p, b, seed, [0.1, 0.3, 0.1, 0.1])


@pytest.fixture(scope="module")
def cartpole(api):
    """cart-pole IPDDP with its control box, N = 5, three iterations, B = 70.  Shared, never re-solved, nothing installed."""
    h = cartpole_handle(api, api.SOLVER_IPDDP)
    yield h
    h.close()


@pytest.fixture(scope="module")
def cartpole_clddp(api):
    h = cartpole_handle(api, api.SOLVER_CLDDP, seed=20262002)
    yield h
    h.close()


@pytest.fixture(scope="module")
def unicycle(api):
    """unicycle IPDDP with its control box and the ball obstacle, N = 5"""
    p = api.unicycle_problem(api.SOLVER_IPDDP, horizon=5, obstacle=True)
    p.options.max_iterations = 3
    h = solved(api, p, B, 20262003, [0.05, 0.05, 0.02])
    yield h
    h.close()


GIVEN = {"none": (False, False, False), "all": (True, True, True), "Q": (True, False, False), "R+Qf": (False, True, True)}


@pytest.mark.parametrize("which", sorted(GIVEN))
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_traj"])
def test_cartpole_ipddp_bitwise(api, cartpole, per, which):
    Q, R, Qf = weights(cartpole.p, 20262010, per)
    q, r, f = GIVEN[which]
    rK, rP, ri = check(cartpole, Q if q else None, R if r else None, Qf if f else None, ("cartpole", per, which))
    assert np.all(ri == 0) and np.all(np.isfinite(rP)) and np.abs(rK).max() > 0
    assert same(rP, np.swapaxes(rP, 2, 3))


@pytest.mark.parametrize("name", ["cartpole_clddp", "unicycle"])
def test_other_solves_bitwise(api, request, name):
    h = request.getfixturevalue(name)
    for per in (False, True):
        Q, R, Qf = weights(h.p, 20262020, per)
        check(h, Q, R, Qf, (name, per))
    check(h, None, None, None, (name, "own weights"))


@pytest.mark.parametrize("kind", ["host", "device"])
def test_each_output_alone(api, cartpole, kind):
    h = cartpole
    conv = dev if kind == "device" else (lambda a: a)
    Q, R, Qf = weights(h.p, 20262030, True)
    ref = dict(zip(("K", "P", "info"), reference(h, Q, R, Qf)))
    for want in (("K",), ("P",)):
        out = h.plan_tvlqr(conv(Q), conv(R), conv(Qf), want=want)
        assert sorted(out) == sorted(want + ("info",))
        for k in out:
            assert same(out[k], ref[k]), (kind, want, k)
    with pytest.raises(ValueError):
        h.plan_tvlqr(conv(Q), want=())
    with pytest.raises(ValueError):
        h.plan_tvlqr(conv(Q), (dev if kind == "host" else (lambda a: a))(R))                       # one on the host, one on the device
    with pytest.raises(ValueError):
        h.plan_tvlqr(conv(Q), conv(R[0]))                                                          # R shared, Q per trajectory
    with pytest.raises(ValueError):
        h.plan_tvlqr(Q.astype(np.float32))


def test_symmetry_and_last_row(api, cartpole):
    """P[..., i, j] == P[..., j, i] bitwise, and row N is Qf's lower triangle mirrored: the junk above the diagonal of the inputs is never read"""
    h = cartpole
    for per in (False, True):
        Q, R, Qf = weights(h.p, 20262040, per)
        out = h.plan_tvlqr(dev(Q), dev(R), dev(Qf))
        P = out["P"].cpu().numpy()
        assert same(P, np.swapaxes(P, 2, 3))
        assert same(P[:, h.p.N], np.broadcast_to(PC.mirror(Qf), P[:, h.p.N].shape))
        assert not same(PC.mirror(Qf), Qf)
        clean = h.plan_tvlqr(PC.mirror(Q), PC.mirror(R), PC.mirror(Qf))
        assert same(clean["P"], P) and same(clean["K"], out["K"]) and same(clean["info"], out["info"])


def test_two_tile_groups(api, monkeypatch):
    """B = 65, the smallest batch of two tiles and so of two groups (trajectories 0..63 and 64): the caller's pointers are offset per
    group, the per-trajectory weights too"""
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=5)
    p.options.max_iterations = 3
    b = 65
    x0 = api.batch_x0(p, b, 20262050, np.array([1.0, 1.0])); U0 = api.batch_U0(p, b)
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    h = api.HipBatchSolver(p, b); h.set_initial(x0, U0); h.solve()
    assert h.num_groups() == 2
    for per in (False, True):
        Q, R, Qf = weights(p, 20262051, per, b)
        check(h, Q, R, Qf, ("two groups", per))
    out = h.plan_tvlqr(Q, R, Qf, install=True)
    assert same(h.gains()[0], out["K"])
    h.close()


def test_failure_of_one_trajectory(api, cartpole):
    """Per-trajectory R with one trajectory's R negative definite and a small Qf: its first pivot fails at the last step.  info = N, K = 0
    everywhere, P = NaN below row N; every other trajectory is bitwise what the all-good call gives."""
    h = cartpole
    N = h.p.N
    Q, R, Qf = weights(h.p, 20262060, True)
    Qf = 1e-3 * Qf
    good = h.plan_tvlqr(Q, R, Qf)
    assert np.all(good["info"] == 0)
    bad = 66                                                       # in the ragged tile
    Rb = R.copy(); Rb[bad] = -R[bad]
    rK, rP, ri = check(h, Q, Rb, Qf, "failure")
    assert ri[bad] == N and np.all(np.delete(ri, bad) == 0)
    for kind, conv in (("host", lambda a: a), ("device", dev)):
        out = h.plan_tvlqr(conv(Q), conv(Rb), conv(Qf))
        K, P, info = (out[k].cpu().numpy() if kind == "device" else out[k] for k in ("K", "P", "info"))
        assert info[bad] == N and np.all(K[bad] == 0.0) and np.all(np.isnan(P[bad, :N])) and same(P[bad, N], PC.mirror(Qf[bad]))
        keep = np.arange(B) != bad
        assert same(K[keep], good["K"][keep]) and same(P[keep], good["P"][keep]) and np.all(info[keep] == 0)


def test_refusals(api, cartpole):
    t = torch_()
    lib = api.load_hip()
    h = cartpole
    N, nx, nu = h.p.N, h.p.nx, h.p.nu
    Q, R, Qf = weights(h.p, 20262070, False)
    before = h.gains()
    outK = t.zeros((B, N, nu, nx), dtype=t.float64, device="cuda"); hostK = np.zeros((B, N, nu, nx))

    def message():
        return lib.cddp_hip_last_error().decode()

    f = lib.cddp_hip_plan_tvlqr
    assert f(h.h, 8, None, None, None, hostK.ctypes.data, None, None) == -2
    assert "cddp_hip_plan_tvlqr: unknown flag bits 0x8" in message()
    assert f(h.h, 0, Q.ctypes.data, None, None, None, None, None) == -1
    assert "cddp_hip_plan_tvlqr: K_out and P_out are both null" in message()
    assert f(h.h, api.LQR_DEVICE, Q.ctypes.data, None, None, outK.data_ptr(), None, None) != 0
    assert "cddp_hip_plan_tvlqr: Q is not device memory" in message()
    assert f(h.h, api.LQR_DEVICE | api.LQR_INSTALL, None, None, None, hostK.ctypes.data, None, None) != 0
    assert "cddp_hip_plan_tvlqr: K_out is not device memory" in message()
    Qn = Q.copy(); Qn[1, 0] = np.inf
    assert f(h.h, api.LQR_INSTALL, Qn.ctypes.data, None, None, hostK.ctypes.data, None, None) == -2
    assert "cddp_hip_plan_tvlqr: Q holds a non-finite value" in message()
    assert float(outK.abs().max()) == 0.0 and np.all(hostK == 0.0)
    after = h.gains()
    assert same(before[0], after[0]) and same(before[1], after[1])
    # a handle that was never solved
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=5)
    fresh = api.HipBatchSolver(p, 8)
    with pytest.raises(api.HipError, match="cddp_hip_plan_tvlqr needs a solved handle"):
        fresh.plan_tvlqr(Q)
    fresh.close()
    # an MSIPDDP handle
    import test_msipddp_device as MS
    pm = MS.make(api, "pendulum_box")[0]
    pm.options.max_iterations = 2
    ms = solved(api, pm, 8, 20262071, [0.1, 0.1])
    with pytest.raises(api.HipError, match="cddp_hip_plan_tvlqr: not for an MSIPDDP handle"):
        ms.plan_tvlqr(install=True)
    ms.close()


@pytest.mark.parametrize("solver", ["IPDDP", "CLDDP"])
def test_install_wiring(api, solver):
    """After plan_tvlqr(install=True) the gain stack holds K_lqr and k is what it was; plan_jvp, plan_covariance and track_plan evaluate
    the designed controller: bitwise their numpy restatements / host loop fed K_lqr."""
    from test_plant_device import host_track
    h = cartpole_handle(api, getattr(api, "SOLVER_" + solver), seed=20262080)
    p = h.p
    A, Bm, K0 = stacks(h)
    k0 = h.gains()[1]
    Q, R, Qf = weights(p, 20262081, True)
    out = h.plan_tvlqr(dev(Q), dev(R), dev(Qf), install=True)
    K = out["K"].cpu().numpy()
    assert same(K, reference(h, Q, R, Qf)[0]) and not same(K, K0)
    Kg, kg = h.gains()
    assert same(Kg, K) and same(kg, k0)
    assert same(h.field_device("K").view(B, p.N, p.nu, p.nx), K)
    A2, Bm2 = h.linearization()
    assert same(A2, A) and same(Bm2, Bm)
    rng = np.random.default_rng(20262082)
    dx0 = np.ascontiguousarray(rng.standard_normal((B, 2, p.nx)))
    dX, dU = h.plan_jvp(dx0)
    rX, rU = ref_jvp(A, Bm, K, dx0)
    assert same(dX, rX) and same(dU, rU)
    S0 = PC.spd(rng, p.nx, 1.0, (B,)); W = PC.spd(rng, p.nx, 0.05, (B,)); Wu = PC.spd(rng, p.nu, 0.1, (B,))
    cov = h.plan_covariance(S0, W, Wu)
    rSX, rSU, rc = PC.covariance(A, Bm, K, S0, W, Wu, *PC.cost_matrices(p))
    assert same(cov["SX"], rSX) and same(cov["SU"], rSU) and same(cov["dcost"], rc)
    Xp, Up = h.trajectory()
    xs = np.ascontiguousarray(Xp[:, 0] + 1e-2 * rng.standard_normal((B, p.nx)))
    Wn = 1e-3 * rng.standard_normal((B, p.N, p.nx))
    dp = api.DevicePlant.of_problem(p, B, substeps=2, integrator=api.RK4)
    Xr, Ur, _ = host_track(h, dp, xs, Wn, None)                   # (reads gains(): K_lqr, as asserted above)
    Xo, Uo = h.track_plan(dp, x0=xs, W=Wn)
    assert same(Xo, Xr) and same(Uo, Ur)
    dp.close()
    # install without outputs
    h2 = cartpole_handle(api, getattr(api, "SOLVER_" + solver), seed=20262080)
    o2 = h2.plan_tvlqr(Q, R, Qf, install=True, want=())
    assert sorted(o2) == ["info"] and np.all(o2["info"] == 0) and same(h2.gains()[0], K)
    h.close(); h2.close()


@pytest.mark.parametrize("solver", ["IPDDP", "CLDDP"])
def test_install_is_dead_state(api, solver):
    """Two identical solved handles, one installs: mpc_advance(SHIFT_EXISTING) + solve, then set_initial + solve, give the same bits on
    both -- results, X, U, K and k.  The gain stack is rewritten by the first sweep of a solve before anything reads it."""
    import test_mpc_advance as M
    p = api.cartpole_problem(getattr(api, "SOLVER_" + solver), True, horizon=5)
    p.options.max_iterations = 3
    a, b, x0, U0 = M.pair(api, p, B, 20262090, [0.1, 0.3, 0.1, 0.1])
    Q, R, Qf = weights(p, 20262091, True)
    K = a.plan_tvlqr(Q, R, Qf, install=True)["K"]
    assert same(a.gains()[0], K) and not same(b.gains()[0], K)

    def both(where):
        M.assert_same_solve(a, b, where, duals=solver == "IPDDP")
        for x, y, name in zip(a.gains(), b.gains(), ("K", "k")):
            assert same(x, y), (where, name)

    for h in (a, b):
        h.mpc_advance(api.MPC_SHIFT_EXISTING); h.solve()
    both("after the MPC step")
    a.plan_tvlqr(Q, R, Qf, install=True)
    for h in (a, b):
        h.set_initial(x0, U0); h.solve()
    both("after set_initial")
    a.close(); b.close()


def test_lti_identity_with_plan_covariance(api):
    """On an LTI handle, with the handle's own weights installed, the expected cost increase of cddp_hip_plan_covariance under Sigma0 and
    no noise is tr(P_0 Sigma0): two evaluations of one quantity in different orders, 8 x the deviation measured against exact evaluation."""
    from test_plan_sens import lti_problem, lti_seed
    p = lti_problem(api, 5, 5)
    x0 = api.batch_x0(p, B, 20262100, [1.0, 1.0]); U0, X0 = lti_seed(p, x0)
    h = solved(api, p, B, 0, U0=U0, X0=X0, x0=x0)
    out = h.plan_tvlqr(install=True)
    rK, rP, ri = reference(h, None, None, None)
    assert same(out["K"], rK) and same(out["P"], rP) and np.all(out["info"] == 0)
    rng = np.random.default_rng(20262101)
    S0 = PC.spd(rng, p.nx, 1.0, (B,))
    dcost = h.plan_covariance(S0, want=("dcost",))["dcost"]
    tr = np.sum(out["P"][:, 0] * PC.mirror(S0), axis=(1, 2))
    err = (np.abs(dcost - tr) / np.abs(tr)).max()
    print("LTI identity: largest |dcost - tr(P_0 Sigma0)| / tr = %.3e, allowed %.3e" % (err, 8.0 * PL.MEASURED_REL_DEV_IDENTITY))
    assert err <= 8.0 * PL.MEASURED_REL_DEV_IDENTITY
    h.close()


def plain_K(sv, x0, kw):
    return sv.solve_batch_device(x0, kw["U0"], kw["X0"], solver_type=kw["solver_type"], want=("K",))["K"]


def test_facade(api):
    """CDDP.solve_batch_tvlqr = solve_batch_device + the design; with install=True (the default) the field "K" is the designed controller"""
    import os, sys, importlib.util
    name = "pycddp_amd"
    if name in sys.modules:
        pycddp = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py"))
        pycddp = importlib.util.module_from_spec(spec); sys.modules[name] = pycddp; spec.loader.exec_module(pycddp)
    from test_plan_sens import lti_problem, lti_seed
    p = lti_problem(api, 5, 5)
    b = 64
    x0n = api.batch_x0(p, b, 20262110, [1.0, 1.0]); U0n, X0n = lti_seed(p, x0n)
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 5
    sv = pycddp.CDDP(x0n[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.LTISystem(p.lti_A, p.lti_B, p.dt, "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    Q, R, Qf = weights(p, 20262111, True, b)
    kw = dict(U0=dev(U0n), X0=dev(X0n), solver_type=pycddp.SolverType.CLDDP)
    out = sv.solve_batch_tvlqr(dev(x0n), dev(Q), dev(R), dev(Qf), want=("X", "U", "K", "A", "B"), **kw)
    plain = sv.solve_batch_device(dev(x0n), dev(U0n), dev(X0n), solver_type=pycddp.SolverType.CLDDP)
    assert same(out["X"], plain["X"]) and same(out["U"], plain["U"])
    A = out["A"].cpu().numpy().reshape(b, p.N, 2, 2); Bm = out["B"].cpu().numpy().reshape(b, p.N, 2, 1)
    rK, rP, ri = PL.tvlqr(A, Bm, Q * p.dt, R * p.dt, Qf)
    assert same(out["K_lqr"], rK) and same(out["P_lqr"], rP) and same(out["lqr_info"], ri)
    assert same(out["K"].cpu().numpy().reshape(b, p.N, 1, 2), rK)                          # installed before the fields were fetched
    own = sv.solve_batch_tvlqr(dev(x0n), install=False, want=("K",), **kw)                 # the objective's own weights; nothing installed
    rK0, rP0, _ = PL.tvlqr(A, Bm, *PC.cost_matrices(p))
    assert same(own["K_lqr"], rK0) and same(own["P_lqr"], rP0)
    assert same(own["K"], plain_K(sv, dev(x0n), kw))                                        # the sweep's own gains


def test_install_is_dead_state_logddp(api):
    """The same on a LogDDP handle (the third solver the entry accepts), pendulum with its control box: a warm re-solve and a solve from a
    new seed give the same bits whether or not gains were installed before."""
    import test_mpc_advance as M
    p = api.pendulum_problem(api.SOLVER_LOGDDP, True, horizon=5)
    p.options.max_iterations = 3
    a, b, x0, U0 = M.pair(api, p, B, 20262120, [0.3, 0.3])
    Q, R, Qf = weights(p, 20262121, True)
    K = a.plan_tvlqr(Q, R, Qf, install=True)["K"]
    assert same(a.gains()[0], K) and not same(b.gains()[0], K)
    for where in ("warm re-solve", "after set_initial"):
        for h in (a, b):
            if where != "warm re-solve":
                h.set_initial(x0, U0)
            h.solve()
        M.assert_same_solve(a, b, where)
        for x, y, name in zip(a.gains(), b.gains(), ("K", "k")):
            assert same(x, y), (where, name)
        a.plan_tvlqr(Q, R, Qf, install=True)
    a.close(); b.close()
