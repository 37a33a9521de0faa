"""State and control covariance along a solved plan on the device (cddp_hip_plan_covariance; csrc/inst_cov.hip).

The header fixes the arithmetic, so the contract is BITWISE: the reference of every bitwise check is tests/plan_cov_ref.py (the numpy
restatement that tests/test_plan_cov_host.py holds to the C++ step bodies and to exact evaluation), fed by get_gains and
get_linearization of the same handle and by the problem's own Q dt, R dt and Qf.  Comparisons are by value with NaN = NaN (the header
leaves the sign of an exact zero open).  Shapes: B = 70 (two tiles, the last partial) unless a test says otherwise, N <= 5.

The one tolerance that is not bitwise (the identity with cddp_hip_plan_jvp) is 8 x plan_cov_ref.MEASURED_REL_DEV, the value measured
against exact evaluation on the CPU, relative to max |Sigma_t|."""
import numpy as np
import pytest

import plan_cov_ref as PC
from plan_cov_ref import same
from test_plan_sens import dev, solved, stacks, torch_

pytestmark = pytest.mark.gpu

B = 70


def noise(p, seed, per, b=B):
    """(Sigma0, W, Wu): symmetric positive definite, with junk above the diagonal -- only the lower triangles may be read"""
    rng = np.random.default_rng(seed)
    lead = (b,) if per else ()
    out = []
    for n, scale in ((p.nx, 1.0), (p.nx, 0.05), (p.nu, 0.1)):
        M = PC.spd(rng, n, scale, lead)
        out.append(np.ascontiguousarray(np.tril(M) + np.triu(rng.standard_normal(lead + (n, n)), 1)))
    return out


def reference(h, S0, W, Wu, diag):
    A, Bm, K = stacks(h)
    assert np.abs(A).max() > 0 and np.abs(Bm).max() > 0 and np.abs(K).max() > 0          # the sweep has left stacks to read
    Qdt, Rdt, Qf = PC.cost_matrices(h.p)
    return PC.covariance(A, Bm, K, S0, W, Wu, Qdt, Rdt, Qf, diag=diag)


def check(h, S0, W, Wu, diag, where, kinds=("host", "device"), ref=None):
    rX, rU, rc = ref if ref is not None else reference(h, S0, W, Wu, diag)
    for kind in kinds:
        conv = dev if kind == "device" else (lambda a: a)
        out = h.plan_covariance(conv(S0), conv(W), conv(Wu), diag=diag)
        if kind == "device":
            t = torch_()
            assert all(v.is_cuda and v.dtype == t.float64 and v.is_contiguous() for v in out.values()), where
        else:
            assert all(isinstance(v, np.ndarray) for v in out.values()), where
        assert sorted(out) == ["SU", "SX", "dcost"]
        assert tuple(out["SX"].shape) == rX.shape and tuple(out["SU"].shape) == rU.shape and tuple(out["dcost"].shape) == rc.shape, (where, kind)
        assert same(out["SX"], rX), (where, kind, "SX")
        assert same(out["SU"], rU), (where, kind, "SU")
        assert same(out["dcost"], rc), (where, kind, "dcost")
    return rX, rU, rc


def cartpole_handle(api, solver, N=5, b=B, seed=20261701):
    p = api.cartpole_problem(solver, True, horizon=N)
    p.options.max_iterations = 3
    return solved(api, p, b, seed, [0.1, 0.3, 0.1, 0.1])


@pytest.fixture(scope="module")
def cartpole(api):
    """cart-pole IPDDP with its control box, N = 5, three iterations, B = 70.  Shared, never re-solved."""
    h = cartpole_handle(api, api.SOLVER_IPDDP)
    yield h
    h.close()


@pytest.fixture(scope="module")
def cartpole_clddp(api):
    h = cartpole_handle(api, api.SOLVER_CLDDP, seed=20261702)
    yield h
    h.close()


@pytest.fixture(scope="module")
def unicycle(api):
    """unicycle IPDDP with its control box and the ball obstacle, N = 5"""
    p = api.unicycle_problem(api.SOLVER_IPDDP, horizon=5, obstacle=True)
    p.options.max_iterations = 3
    h = solved(api, p, B, 20261703, [0.05, 0.05, 0.02])
    yield h
    h.close()


NOISES = {"none": (False, False), "W": (True, False), "Wu": (False, True), "both": (True, True)}


@pytest.mark.parametrize("which", sorted(NOISES))
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_traj"])
@pytest.mark.parametrize("diag", [False, True], ids=["full", "diag"])
def test_cartpole_ipddp_bitwise(api, cartpole, diag, per, which):
    S0, W, Wu = noise(cartpole.p, 20261710, per)
    w, wu = NOISES[which]
    rX, rU, rc = check(cartpole, S0, W if w else None, Wu if wu else None, diag, ("cartpole", diag, per, which))
    assert np.all(np.isfinite(rX)) and np.abs(rX).max() > 0 and np.abs(rU).max() > 0 and np.all(rc > 0)
    if not diag:
        assert same(rX, np.swapaxes(rX, 2, 3))


@pytest.mark.parametrize("name", ["cartpole_clddp", "unicycle"])
@pytest.mark.parametrize("diag", [False, True], ids=["full", "diag"])
def test_other_solves_bitwise(api, request, name, diag):
    h = request.getfixturevalue(name)
    for per in (False, True):
        S0, W, Wu = noise(h.p, 20261720, per)
        check(h, S0, W, Wu, diag, (name, diag, per))
        check(h, S0, None, None, diag, (name, diag, per, "no noise"), kinds=("device",))


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("diag", [False, True], ids=["full", "diag"])
def test_each_output_alone(api, cartpole, diag, kind):
    h = cartpole
    conv = dev if kind == "device" else (lambda a: a)
    S0, W, Wu = noise(h.p, 20261730, True)
    ref = dict(zip(("SX", "SU", "dcost"), reference(h, S0, W, Wu, diag)))
    for want in (("SX",), ("SU",), ("dcost",), ("SX", "dcost"), ("SU", "SX")):
        out = h.plan_covariance(conv(S0), conv(W), conv(Wu), diag=diag, want=want)
        assert sorted(out) == sorted(want)
        for k in want:
            assert same(out[k], ref[k]), (kind, diag, want, k)
    with pytest.raises(ValueError):
        h.plan_covariance(conv(S0), want=())
    with pytest.raises(ValueError):
        h.plan_covariance(conv(S0), conv(W), (dev if kind == "host" else (lambda a: a))(Wu))      # one on the host, one on the device
    with pytest.raises(ValueError, match="shape"):
        h.plan_covariance(conv(S0), conv(W[0]), conv(Wu))                                          # W shared, Sigma0 per trajectory
    with pytest.raises(ValueError):
        h.plan_covariance(S0.astype(np.float32))


def test_symmetry_and_first_row(api, cartpole):
    """SX[..., i, j] == SX[..., j, i] bitwise (SU likewise), and row 0 is Sigma0's lower triangle mirrored: the junk above the diagonal of
    the inputs is never read"""
    h = cartpole
    for per in (False, True):
        S0, W, Wu = noise(h.p, 20261740, per)
        out = h.plan_covariance(dev(S0), dev(W), dev(Wu))
        SX = out["SX"].cpu().numpy(); SU = out["SU"].cpu().numpy()
        assert same(SX, np.swapaxes(SX, 2, 3)) and same(SU, np.swapaxes(SU, 2, 3))
        assert same(SX[:, 0], np.broadcast_to(PC.mirror(S0), SX[:, 0].shape))
        assert not same(PC.mirror(S0), S0)
        clean = h.plan_covariance(PC.mirror(S0), PC.mirror(W), PC.mirror(Wu))
        assert same(clean["SX"], SX) and same(clean["SU"], SU) and same(clean["dcost"], out["dcost"])


def test_user_stream(api, cartpole):
    """The device path on a user stream (set_stream): inputs written by torch ops queued on the stream right before the call are the ones
    used, and the outputs are complete for a torch op queued right after."""
    t = torch_()
    p = cartpole.p
    h = cartpole_handle(api, api.SOLVER_IPDDP)
    S0, W, Wu = noise(p, 20261750, True)
    ref = reference(h, S0, W, Wu, False)
    s = t.cuda.Stream()
    h.set_stream(s.cuda_stream)
    half = [t.from_numpy(0.5 * a).cuda() for a in (S0, W, Wu)]     # (exact halves: doubling restores the bits)
    big = t.zeros((1024, 1024), dtype=t.float64, device="cuda")
    t.cuda.synchronize()
    with t.cuda.stream(s):
        for _ in range(4):
            big = big @ big                      # work in front of the inputs on the stream: an unordered read would see zeros
        ins = [t.zeros_like(a) for a in half]
        for x, a in zip(ins, half):
            x.add_(a, alpha=2.0)
        out = h.plan_covariance(*ins)
        got = [out[k] * 1.0 for k in ("SX", "SU", "dcost")]      # consumed on the stream, no synchronisation in between
    s.synchronize()
    for g, r, k in zip(got, ref, ("SX", "SU", "dcost")):
        assert same(g, r), k
    h.close()


@pytest.mark.parametrize("b", [1, 64])
def test_batch_sizes(api, b):
    """B = 1 (one live lane) and B = 64 (exactly one tile); B = 70 is everywhere else"""
    h = cartpole_handle(api, api.SOLVER_IPDDP, b=b, seed=20261760 + b)
    for per in (False, True):
        S0, W, Wu = noise(h.p, 20261761, per, b)
        check(h, S0, W, Wu, False, ("B", b, per))
        check(h, S0, W, None, True, ("B", b, per, "diag"), kinds=("device",))
    h.close()


def test_shortest_horizon(api):
    """N = 1: one step, then the terminal term"""
    h = cartpole_handle(api, api.SOLVER_IPDDP, N=1, seed=20261770)
    S0, W, Wu = noise(h.p, 20261771, False)
    rX, rU, rc = check(h, S0, W, Wu, False, "N=1")
    assert rX.shape == (B, 2, 4, 4) and rU.shape == (B, 1, 1, 1)
    check(h, S0, None, Wu, True, "N=1 diag")
    h.close()


def test_two_tile_groups(api, monkeypatch):
    """B = 130 in two groups (trajectories 0..127 and 128..129): the caller's pointers are offset per group, the per-trajectory inputs too"""
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=5)
    p.options.max_iterations = 3
    b = 130
    x0 = api.batch_x0(p, b, 20261780, np.array([1.0, 1.0])); U0 = api.batch_U0(p, b)
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    h = api.HipBatchSolver(p, b); h.set_initial(x0, U0); h.solve()
    assert h.num_groups() == 2
    for per in (False, True):
        S0, W, Wu = noise(p, 20261781, per, b)
        for diag in (False, True):
            check(h, S0, W, Wu, diag, ("two groups", per, diag))
    h.close()


def test_state_untouched(api):
    """get_trajectory, get_gains and get_results are the same bits before and after the call, and a following solve gives what it gives
    without the calls."""
    import test_mpc_advance as M
    a = cartpole_handle(api, api.SOLVER_IPDDP, seed=20261790); b = cartpole_handle(api, api.SOLVER_IPDDP, seed=20261790)
    before = (a.trajectory(), a.gains(), a.results())
    S0, W, Wu = noise(a.p, 20261791, True)
    a.plan_covariance(S0, W, Wu); a.plan_covariance(dev(S0), dev(W), dev(Wu), diag=True)
    after = (a.trajectory(), a.gains(), a.results())
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert same(x, y)
    assert before[2].tobytes() == after[2].tobytes()
    a.solve(); b.solve()
    M.assert_same_solve(a, b, "after the covariance", duals=True)
    a.close(); b.close()


def test_refusals_on_the_device(api, cartpole):
    t = torch_()
    lib = api.load_hip()
    h = cartpole
    N, nx, nu = h.p.N, h.p.nx, h.p.nu
    S0, W, Wu = noise(h.p, 20261800, False)
    good = dev(S0)
    outX = t.zeros((B, N + 1, nx, nx), dtype=t.float64, device="cuda"); hostX = np.zeros((B, N + 1, nx, nx))

    def message():
        return lib.cddp_hip_last_error().decode()

    f = lib.cddp_hip_plan_covariance
    assert f(h.h, api.COV_DEVICE, S0.ctypes.data, None, None, outX.data_ptr(), None, None) != 0
    assert "cddp_hip_plan_covariance: Sigma0 is not device memory" in message()
    assert f(h.h, api.COV_DEVICE, good.data_ptr(), W.ctypes.data, None, outX.data_ptr(), None, None) != 0
    assert "cddp_hip_plan_covariance: W is not device memory" in message()
    assert f(h.h, api.COV_DEVICE, good.data_ptr(), None, None, hostX.ctypes.data, None, None) != 0
    assert "cddp_hip_plan_covariance: SX is not device memory" in message()
    assert float(outX.abs().max()) == 0.0 and np.all(hostX == 0.0)
    # a handle that was never solved
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=5)
    fresh = api.HipBatchSolver(p, 8)
    with pytest.raises(api.HipError, match="cddp_hip_plan_covariance needs a solved handle"):
        fresh.plan_covariance(S0)
    fresh.close()
    # an MSIPDDP handle
    import test_msipddp_device as MS
    pm = MS.make(api, "pendulum_box")[0]
    pm.options.max_iterations = 2
    ms = solved(api, pm, 8, 20261801, [0.1, 0.1])
    with pytest.raises(api.HipError, match="cddp_hip_plan_covariance: not for an MSIPDDP handle"):
        ms.plan_covariance(np.eye(pm.nx))
    ms.close()


def test_identity_with_plan_jvp(api, cartpole):
    """W = Wu = NULL: SX_t = Phi_t Sigma0 Phi_t^T with Phi_t = dX_t / dx0 from cddp_hip_plan_jvp on the identity vectors, the products formed
    in numpy.  Two evaluations of one quantity in different orders: 8 x the deviation measured against exact evaluation (relative to
    max |Sigma_t|) is allowed, the factor the feature request sets."""
    h = cartpole
    S0, _, _ = noise(h.p, 20261810, True)
    SX = h.plan_covariance(S0, want=("SX",))["SX"]
    dXdx0, _ = h.plan_jacobian_device()
    Phi = dXdx0.cpu().numpy()                                    # (B, N + 1, nx, nx): [b, t, i, j] = d X_t[i] / d x0[j]
    want = Phi @ PC.mirror(S0)[:, None] @ np.swapaxes(Phi, 2, 3)
    err = np.abs(SX - want).max() / np.abs(SX).max()
    print("identity with plan_jvp: largest deviation / max |Sigma_t| = %.3e, allowed %.3e" % (err, 8.0 * PC.MEASURED_REL_DEV))
    assert err <= 8.0 * PC.MEASURED_REL_DEV


def test_facade(api):
    """CDDP.solve_batch_cov = solve_batch_device + the covariance"""
    import os, sys, importlib.util
    t = torch_()
    name = "pycddp_amd"
    if name in sys.modules:
        pycddp = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py"))
        pycddp = importlib.util.module_from_spec(spec); sys.modules[name] = pycddp; spec.loader.exec_module(pycddp)
    from test_plan_sens import lti_problem, lti_seed
    p = lti_problem(api, 5, 5)
    b = 64
    x0n = api.batch_x0(p, b, 20261820, [1.0, 1.0]); U0n, X0n = lti_seed(p, x0n)
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 5
    sv = pycddp.CDDP(x0n[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.LTISystem(p.lti_A, p.lti_B, p.dt, "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    S0, W, Wu = noise(p, 20261821, False, b)
    out = sv.solve_batch_cov(dev(x0n), dev(S0), dev(W), dev(Wu), U0=dev(U0n), X0=dev(X0n), solver_type=pycddp.SolverType.CLDDP, want=("X", "U", "K", "A", "B"))
    plain = sv.solve_batch_device(dev(x0n), dev(U0n), dev(X0n), solver_type=pycddp.SolverType.CLDDP)
    assert same(out["X"], plain["X"]) and same(out["U"], plain["U"])
    A = out["A"].cpu().numpy().reshape(b, p.N, 2, 2); Bm = out["B"].cpu().numpy().reshape(b, p.N, 2, 1); K = out["K"].cpu().numpy().reshape(b, p.N, 1, 2)
    rX, rU, rc = PC.covariance(A, Bm, K, S0, W, Wu, *PC.cost_matrices(p))
    assert same(out["SX"], rX) and same(out["SU"], rU) and same(out["expected_cost_increase"], rc)


def test_facade_takes_the_seed_of_set_initial_trajectory(api):
    """U0 = X0 = None after set_initial_trajectory: solve_batch_cov starts every member from that trajectory, as solve_batch_device does --
    X and U are its bits, and not those of the solve from the zero seed.  LTI 2 x 1 CLDDP stopped after one iteration."""
    import os, sys, importlib.util
    name = "pycddp_amd"
    if name in sys.modules:
        pycddp = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py"))
        pycddp = importlib.util.module_from_spec(spec); sys.modules[name] = pycddp; spec.loader.exec_module(pycddp)
    from test_plan_sens import lti_problem
    p = lti_problem(api, 5, 1)                                   # one iteration: the result still carries the seed
    b = 64
    x0n = api.batch_x0(p, b, 20261830, [1.0, 1.0])
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 1
    rng = np.random.default_rng(20261831)
    Useed = 0.5 * rng.standard_normal((p.N, p.nu)); Xseed = np.zeros((p.N + 1, p.nx)); Xseed[0] = x0n[0]
    for t in range(p.N):
        Xseed[t + 1] = p.lti_A @ Xseed[t] + p.lti_B @ Useed[t]

    def solver(seed):
        sv = pycddp.CDDP(x0n[0], p.x_ref, p.N, p.dt, o)
        sv.set_dynamical_system(pycddp.LTISystem(p.lti_A, p.lti_B, p.dt, "euler"))
        sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
        if seed:
            sv.set_initial_trajectory(list(Xseed), list(Useed))
        return sv

    S0, W, Wu = noise(p, 20261832, False, b)
    kw = dict(solver_type=pycddp.SolverType.CLDDP)
    out = solver(True).solve_batch_cov(dev(x0n), dev(S0), dev(W), dev(Wu), **kw)
    plain = solver(True).solve_batch_device(dev(x0n), **kw)
    zero = solver(False).solve_batch_device(dev(x0n), **kw)
    assert same(out["X"], plain["X"]) and same(out["U"], plain["U"])
    assert same(out["results"]["iterations"], plain["results"]["iterations"])
    assert not same(plain["U"], zero["U"])                       # the seed does matter here: the check above is not vacuous
