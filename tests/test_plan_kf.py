"""Kalman filter gains and output-feedback covariance along a solved plan on the device (cddp_hip_plan_kalman; csrc/inst_kf.hip).

The header fixes the arithmetic, so the contract is BITWISE: the reference of every check is tests/plan_kf_ref.py (the numpy restatement
that tests/test_plan_kf_host.py holds to the C++ step bodies and to exact evaluation), fed the handle's own field_device("A" / "B" / "K")
and the problem's Q dt, R dt and Qf.  Comparisons are by value with NaN = NaN (the header leaves the sign of an exact zero open).
Shapes: B = 70 (a full tile and a ragged one), N = 6; cart-pole (4, 1), unicycle (3, 2), pendulum (2, 1)."""
import numpy as np
import pytest

import plan_cov_ref as PC
import plan_kf_ref as PK
from plan_kf_ref import same
from test_plan_sens import dev, solved, torch_

pytestmark = pytest.mark.gpu

B = 70
N = 6
ALL = ("L", "SP", "SF", "SX", "SU", "dcost", "info")


def stacks_dev(h):
    p = h.p
    f = lambda name, shape: h.field_device(name).view((h.B, p.N) + shape).cpu().numpy()
    return f("A", (p.nx, p.nx)), f("B", (p.nx, p.nu)), f("K", (p.nu, p.nx))


def inputs(p, ny, seed, per, b=B, w=True, wu=True):
    """(C, v, Sigma0, W, Wu): spd covariances with junk above the diagonal -- only the lower triangles may be read"""
    rng = np.random.default_rng(seed)
    lead = (b,) if per else ()
    C = np.ascontiguousarray(rng.standard_normal(lead + (ny, p.nx))); v = np.ascontiguousarray(0.05 + rng.random(lead + (ny,)))
    out = [C, v]
    for n, scale, given in ((p.nx, 1.0, True), (p.nx, 0.05, w), (p.nu, 0.1, wu)):
        M = PC.spd(rng, n, scale, lead)
        out.append(np.ascontiguousarray(np.tril(M) + np.triu(rng.standard_normal(lead + (n, n)), 1)) if given else None)
    return out


def reference(h, ins, diag=False):
    A, Bm, K = stacks_dev(h)
    assert np.abs(A).max() > 0 and np.abs(Bm).max() > 0                                   # the sweep has left stacks to read
    return PK.kalman(A, Bm, K, *ins, *PC.cost_matrices(h.p), diag=diag)


def check(h, ins, where, kinds=("host", "device"), diag=False, ref=None):
    ref = ref if ref is not None else reference(h, ins, diag)
    for kind in kinds:
        conv = dev if kind == "device" else (lambda a: a)
        out = h.plan_kalman(*[conv(a) for a in ins], diag=diag, want=ALL)
        if kind == "device":
            t = torch_()
            assert all(v.is_cuda and v.is_contiguous() for v in out.values()) and out["L"].dtype == t.float64 and out["info"].dtype == t.int32, where
        else:
            assert all(isinstance(v, np.ndarray) for v in out.values()) and out["info"].dtype == np.int32, where
        assert sorted(out) == sorted(ALL)
        for k in ALL:
            assert tuple(out[k].shape) == ref[k].shape, (where, kind, k, "shape")
            assert same(out[k], ref[k]), (where, kind, k)
    return ref


def make(api, name, solver=None, seed=20262101, iterations=3):
    if name == "cartpole":
        p = api.cartpole_problem(solver or api.SOLVER_IPDDP, True, horizon=N); spread = [0.1, 0.3, 0.1, 0.1]
    elif name == "unicycle":
        p = api.unicycle_problem(solver or api.SOLVER_IPDDP, horizon=N, obstacle=True); spread = [0.05, 0.05, 0.02]
    else:
        p = api.pendulum_problem(solver or api.SOLVER_LOGDDP, True, horizon=N); spread = [0.3, 0.3]
    p.options.max_iterations = iterations
    return solved(api, p, B, seed, spread)


@pytest.fixture(scope="module")
def cartpole(api):
    """cart-pole IPDDP with its control box, N = 6, three iterations, B = 70.  Shared, never re-solved, nothing installed."""
    h = make(api, "cartpole")
    yield h
    h.close()


@pytest.fixture(scope="module")
def unicycle(api):
    h = make(api, "unicycle", seed=20262102)
    yield h
    h.close()


@pytest.fixture(scope="module")
def pendulum(api):
    """pendulum LogDDP with its control box"""
    h = make(api, "pendulum", seed=20262103)
    yield h
    h.close()


@pytest.fixture(scope="module")
def cartpole_clddp(api):
    h = make(api, "cartpole", api.SOLVER_CLDDP, seed=20262104)
    yield h
    h.close()


@pytest.mark.parametrize("ny", ["1", "nx", "nx+2", "16"])
@pytest.mark.parametrize("name", ["cartpole", "unicycle", "pendulum", "cartpole_clddp"])
def test_bitwise(api, request, name, ny):
    """IPDDP (cart-pole, unicycle), LogDDP (pendulum) and CLDDP handles; shared and per-trajectory inputs; host and device pointers"""
    h = request.getfixturevalue(name)
    m = {"1": 1, "nx": h.p.nx, "nx+2": h.p.nx + 2, "16": 16}[ny]
    for per in (False, True):
        r = check(h, inputs(h.p, m, 20262110 + m, per), (name, ny, per))
        assert np.all(r["info"] == 0) and all(np.all(np.isfinite(r[k])) for k in ALL) and np.abs(r["L"]).max() > 0
        assert same(r["SX"], np.swapaxes(r["SX"], 2, 3)) and r["L"].shape == (B, N + 1, h.p.nx, m)


@pytest.mark.parametrize("w,wu", [(False, False), (True, False), (False, True)], ids=["none", "W", "Wu"])
def test_noise_absent(api, unicycle, w, wu):
    for per in (False, True):
        ins = inputs(unicycle.p, 2, 20262120, per, w=w, wu=wu)
        r = check(unicycle, ins, ("noise", w, wu, per))
        assert np.all(r["info"] == 0)
    full = reference(unicycle, inputs(unicycle.p, 2, 20262120, True))
    assert not same(full["SX"], r["SX"])


def test_diag(api, cartpole, unicycle):
    for h in (cartpole, unicycle):
        for per in (False, True):
            ins = inputs(h.p, h.p.nx, 20262130, per)
            r = check(h, ins, ("diag", per), diag=True)
            assert r["SX"].shape == (B, N + 1, h.p.nx) and r["SU"].shape == (B, N, h.p.nu) and r["L"].shape == (B, N + 1, h.p.nx, h.p.nx)
            full = reference(h, ins)
            assert same(r["SP"], np.diagonal(full["SP"], axis1=2, axis2=3)) and same(r["dcost"], full["dcost"])


@pytest.mark.parametrize("kind", ["host", "device"])
def test_each_output_alone(api, unicycle, kind):
    h = unicycle
    conv = dev if kind == "device" else (lambda a: a)
    ins = inputs(h.p, 5, 20262140, True)
    ref = reference(h, ins)
    args = [conv(a) for a in ins]
    for k in ALL:
        out = h.plan_kalman(*args, want=(k,))
        assert sorted(out) == [k] and same(out[k], ref[k]), (kind, k)
    out = h.plan_kalman(*args)                                                               # the default selection
    assert sorted(out) == ["L", "SU", "SX", "dcost"] and all(same(out[k], ref[k]) for k in out)
    with pytest.raises(ValueError):
        h.plan_kalman(*args, want=())
    with pytest.raises(ValueError):
        h.plan_kalman(*args, want=("K",))
    other = dev if kind == "host" else (lambda a: a)
    with pytest.raises(ValueError):
        h.plan_kalman(args[0], other(ins[1]), args[2])                                       # one on the host, one on the device
    with pytest.raises(ValueError):
        h.plan_kalman(args[0], conv(ins[1][0]), args[2])                                     # v shared, C per trajectory
    with pytest.raises(ValueError):
        h.plan_kalman(conv(np.zeros((B, 17, h.p.nx))), conv(np.ones((B, 17))), args[2])      # ny = 17
    with pytest.raises(ValueError):
        h.plan_kalman(ins[0].astype(np.float32), ins[1], ins[2])


def test_two_tile_groups(api, monkeypatch):
    """B = 65, the smallest batch of two tiles and so of two groups: the caller's pointers are offset per group, the per-trajectory
    inputs too"""
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=N)
    p.options.max_iterations = 3
    b = 65
    x0 = api.batch_x0(p, b, 20262150, np.array([1.0, 1.0])); U0 = api.batch_U0(p, b)
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    h = api.HipBatchSolver(p, b); h.set_initial(x0, U0); h.solve()
    assert h.num_groups() == 2
    for per in (False, True):
        check(h, inputs(p, 3, 20262151, per, b), ("two groups", per))
    h.close()


@pytest.mark.parametrize("solver", ["IPDDP", "CLDDP", "LOGDDP"])
def test_handle_is_not_modified(api, solver):
    """X, U, K, A, B and the result record are what they were, and a following solve is bit for bit that of a twin that never called"""
    import test_mpc_advance as M
    if solver == "LOGDDP":
        p = api.pendulum_problem(api.SOLVER_LOGDDP, True, horizon=N); spread = [0.3, 0.3]
    else:
        p = api.cartpole_problem(getattr(api, "SOLVER_" + solver), True, horizon=N); spread = [0.1, 0.3, 0.1, 0.1]
    p.options.max_iterations = 3
    a, b, x0, U0 = M.pair(api, p, B, 20262160, spread)
    names = ("X", "U", "K", "A", "B")
    before = {n: a.field_device(n).cpu().numpy() for n in names}
    res = a.results()
    ins = inputs(p, 5, 20262161, True)
    a.plan_kalman(*ins, want=ALL)
    a.plan_kalman(*[dev(x) for x in ins], want=ALL)
    for n in names:
        assert same(a.field_device(n), before[n]), n
    assert a.results().tobytes() == res.tobytes()
    for h in (a, b):
        h.solve()
    M.assert_same_solve(a, b, "warm re-solve", duals=solver == "IPDDP")
    for x, y, name in zip(a.gains(), b.gains(), ("K", "k")):
        assert same(x, y), name
    a.close(); b.close()


def test_installed_gains_are_seen(api):
    h = make(api, "cartpole", seed=20262170)
    ins = inputs(h.p, 2, 20262171, True)
    before = check(h, ins, "before the install", kinds=("device",))
    K0 = stacks_dev(h)[2]
    rng = np.random.default_rng(20262172)
    h.plan_tvlqr(PC.spd(rng, h.p.nx), PC.spd(rng, h.p.nu, 0.5), PC.spd(rng, h.p.nx, 3.0), install=True)
    assert not same(stacks_dev(h)[2], K0)
    after = check(h, ins, "after the install")                       # (the restatement is fed the installed K: stacks_dev reads field K)
    assert not same(after["SX"], before["SX"]) and not same(after["SU"], before["SU"])
    assert same(after["L"], before["L"]) and same(after["SP"], before["SP"])          # the filter does not depend on the controller
    h.close()


def test_zero_row_is_no_measurement(api, unicycle):
    h = unicycle
    _, _, S0, W, Wu = inputs(h.p, 1, 20262180, False)
    ins = [np.zeros((1, h.p.nx)), np.array([0.3]), S0, W, Wu]
    r = check(h, ins, "zero row")
    out = h.plan_kalman(*[dev(a) for a in ins], want=("SP", "SF", "SX", "L"))
    assert same(out["SF"], out["SP"]) and same(out["SX"], out["SP"]) and float(out["L"].abs().max()) == 0.0
    A, Bm, K = stacks_dev(h)
    assert same(out["SP"], PC.covariance(A, Bm, np.zeros_like(K), S0, W, Wu)[0])
    assert same(r["SU"], np.broadcast_to(PC.mirror(Wu), r["SU"].shape))


def test_failure_of_one_trajectory(api, cartpole):
    """Per-trajectory inputs with one trajectory's Sigma0 = -I and a small variance on its first row: s = v - |c|^2 < 0 at step 0.
    info = 1, every row NaN; the other 69 trajectories are bitwise those of the run without it."""
    h = cartpole
    ins = inputs(h.p, 3, 20262190, True)
    good = h.plan_kalman(*ins, want=ALL)
    assert np.all(good["info"] == 0)
    bad = 66                                                         # in the ragged tile
    C, v, S0, W, Wu = [a.copy() for a in ins]
    S0[bad] = -np.eye(h.p.nx); v[bad, 0] = 1e-3
    assert np.sum(C[bad, 0] ** 2) > 1e-2
    r = check(h, [C, v, S0, W, Wu], "failure")
    assert r["info"][bad] == 1 and np.all(np.delete(r["info"], bad) == 0)
    keep = np.arange(B) != bad
    for kind, conv in (("host", lambda a: a), ("device", dev)):
        out = h.plan_kalman(*[conv(a) for a in (C, v, S0, W, Wu)], want=ALL)
        out = {k: (x.cpu().numpy() if kind == "device" else x) for k, x in out.items()}
        assert out["info"][bad] == 1 and np.all(out["info"][keep] == 0)
        for k in ALL[:6]:
            assert np.all(np.isnan(out[k][bad])), (kind, k)
            assert same(out[k][keep], good[k][keep]), (kind, k)


def test_refusals(api, cartpole):
    t = torch_()
    lib = api.load_hip()
    h = cartpole
    nx, nu = h.p.nx, h.p.nu
    C, v, S0, W, Wu = inputs(h.p, 2, 20262200, False)
    outX = t.zeros((B, N + 1, nx, nx), dtype=t.float64, device="cuda"); hostX = np.zeros((B, N + 1, nx, nx))
    before = {n: h.field_device(n).cpu().numpy() for n in ("X", "U", "K")}

    def message():
        return lib.cddp_hip_last_error().decode()

    f = lib.cddp_hip_plan_kalman
    hx = hostX.ctypes.data
    nul = [None] * 7
    assert f(h.h, 8, 2, C.ctypes.data, v.ctypes.data, S0.ctypes.data, None, None, None, None, None, hx, None, None, None) == -2
    assert "cddp_hip_plan_kalman: unknown flag bits 0x8" in message()
    for ny in (0, 17):
        assert f(h.h, 0, ny, C.ctypes.data, v.ctypes.data, S0.ctypes.data, None, None, None, None, None, hx, None, None, None) == -2
        assert "cddp_hip_plan_kalman: ny = %d" % ny in message()
    assert f(h.h, 0, 2, C.ctypes.data, v.ctypes.data, S0.ctypes.data, None, None, *nul) == -1
    assert "cddp_hip_plan_kalman: all six outputs and info are null" in message()
    vb = v.copy(); vb[1] = 0.0
    assert f(h.h, 0, 2, C.ctypes.data, vb.ctypes.data, S0.ctypes.data, None, None, None, None, None, hx, None, None, None) == -2
    assert "cddp_hip_plan_kalman: v holds an entry that is not finite and > 0" in message()
    Wn = W.copy(); Wn[1, 0] = np.nan
    assert f(h.h, 0, 2, C.ctypes.data, v.ctypes.data, S0.ctypes.data, Wn.ctypes.data, None, None, None, None, hx, None, None, None) == -2
    assert "cddp_hip_plan_kalman: W holds a non-finite value" in message()
    dC, dv, dS = dev(C), dev(v), dev(S0)
    assert f(h.h, api.KF_DEVICE, 2, C.ctypes.data, dv.data_ptr(), dS.data_ptr(), None, None, None, None, None, outX.data_ptr(), None, None, None) != 0
    assert "cddp_hip_plan_kalman: C is not device memory" in message()
    assert f(h.h, api.KF_DEVICE, 2, dC.data_ptr(), dv.data_ptr(), dS.data_ptr(), None, None, None, None, None, hx, None, None, None) != 0
    assert "cddp_hip_plan_kalman: SX is not device memory" in message()
    assert float(outX.abs().max()) == 0.0 and np.all(hostX == 0.0)
    for n in before:
        assert same(h.field_device(n), before[n]), n
    # a handle that was never solved
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N)
    fresh = api.HipBatchSolver(p, 8)
    with pytest.raises(api.HipError, match="cddp_hip_plan_kalman needs a solved handle"):
        fresh.plan_kalman(C, v, S0)
    fresh.close()
    # an MSIPDDP handle
    import test_msipddp_device as MS
    pm = MS.make(api, "pendulum_box")[0]
    pm.options.max_iterations = 2
    ms = solved(api, pm, 8, 20262201, [0.1, 0.1])
    with pytest.raises(api.HipError, match="cddp_hip_plan_kalman: not for an MSIPDDP handle"):
        ms.plan_kalman(np.ones((1, pm.nx)), np.ones(1), np.eye(pm.nx))
    ms.close()


def test_facade(api):
    """CDDP.solve_batch_lqg = solve_batch_device, the LQR install when a tracking weight is given, then the filter: bitwise the
    restatement fed the fields it returns"""
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
    x0n = api.batch_x0(p, b, 20262210, [1.0, 1.0]); U0n, X0n = lti_seed(p, x0n)
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 5
    sv = pycddp.CDDP(x0n[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.LTISystem(p.lti_A, p.lti_B, p.dt, "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    C, v, S0, W, Wu = inputs(p, 1, 20262211, True, b)
    rng = np.random.default_rng(20262212)
    Q = PC.spd(rng, p.nx, 1.0, (b,))
    kw = dict(U0=dev(U0n), X0=dev(X0n), solver_type=pycddp.SolverType.CLDDP, want=("K", "A", "B"))
    for track in (False, True):
        out = sv.solve_batch_lqg(dev(x0n), dev(C), dev(v), dev(S0), dev(W), dev(Wu), Q_track=dev(Q) if track else None, **kw)
        A = out["A"].cpu().numpy().reshape(b, p.N, 2, 2); Bm = out["B"].cpu().numpy().reshape(b, p.N, 2, 1); K = out["K"].cpu().numpy().reshape(b, p.N, 1, 2)
        ref = PK.kalman(A, Bm, K, C, v, S0, W, Wu, *PC.cost_matrices(p))
        assert sorted(out["kalman"]) == ["L", "SU", "SX", "dcost", "info"]
        for k in out["kalman"]:
            assert same(out["kalman"][k], ref[k]), (track, k)
        assert ("K_lqr" in out) == track
        if track:
            assert same(out["K_lqr"], K)                                                   # installed before the filter ran
