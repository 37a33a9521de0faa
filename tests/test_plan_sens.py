"""Linear response of a solved plan to its initial state on the device (cddp_hip_plan_jvp, cddp_hip_plan_vjp; csrc/inst_sens.hip).

The header fixes the arithmetic, so the contract of the two entries is BITWISE: the reference of every bitwise check is the numpy
restatement of the recursions below (vectorised over the batch only, every accumulation loop written out in the stated order; numpy
rounds each product and each sum, as the library built with -ffp-contract=off does), fed by get_gains and get_linearization of the same
handle.  Comparisons are np.array_equal with NaN = NaN (tests/test_device_io.py::same): values, so that -0.0 == 0.0 -- the library is
built with -fno-signed-zeros and the header leaves the sign of an exact zero open.

Tolerances that are not bitwise are derived where they are used (adjoint consistency: a running error bound on the absolute-value
chain; meaning end to end: 8 x the same quantity measured on the CPU oracle, the factor the feature request sets)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


# ---- the recursions of include/cddp_hip.h in numpy: A (B, N, nx, nx), Bm (B, N, nx, nu), K (B, N, nu, nx)
def ref_jvp(A, Bm, K, dx0):
    """dx0 (B, R, nx) -> dX (B, R, N + 1, nx), dU (B, R, N, nu)"""
    B, N, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    R = dx0.shape[1]
    dX = np.zeros((B, R, N + 1, nx)); dU = np.zeros((B, R, N, nu))
    for r in range(R):
        dX[:, r, 0] = dx0[:, r]
        for t in range(N):
            dx = dX[:, r, t]
            for i in range(nu):
                s = np.zeros(B)
                for j in range(nx):
                    s = s + K[:, t, i, j] * dx[:, j]
                dU[:, r, t, i] = s
            du = dU[:, r, t]
            for i in range(nx):
                s = np.zeros(B)
                for j in range(nx):
                    s = s + A[:, t, i, j] * dx[:, j]
                for k in range(nu):
                    s = s + Bm[:, t, i, k] * du[:, k]
                dX[:, r, t + 1, i] = s
    return dX, dU


def ref_vjp(A, Bm, K, gX, gU, R):
    """gX (B, R, N + 1, nx) or None, gU (B, R, N, nu) or None -> gx0 (B, R, nx)"""
    B, N, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    out = np.zeros((B, R, nx))
    for r in range(R):
        lam = gX[:, r, N].copy() if gX is not None else np.zeros((B, nx))
        for t in range(N - 1, -1, -1):
            mu = np.zeros((B, nu)); new = np.zeros((B, nx))
            for k in range(nu):
                s = np.zeros(B)
                for i in range(nx):
                    s = s + Bm[:, t, i, k] * lam[:, i]
                mu[:, k] = gU[:, r, t, k] + s if gU is not None else s
            for j in range(nx):
                s = np.zeros(B)
                for i in range(nx):
                    s = s + A[:, t, i, j] * lam[:, i]
                for k in range(nu):
                    s = s + K[:, t, k, j] * mu[:, k]
                new[:, j] = gX[:, r, t, j] + s if gX is not None else s
            lam = new
        out[:, r] = lam
    return out


def stacks(h):
    K, _ = h.gains(); A, Bm = h.linearization()
    return A, Bm, K


def vectors(h, R, seed):
    rng = np.random.default_rng(seed)
    p = h.p
    return (np.ascontiguousarray(rng.standard_normal((h.B, R, p.nx))), np.ascontiguousarray(rng.standard_normal((h.B, R, p.N + 1, p.nx))),
            np.ascontiguousarray(rng.standard_normal((h.B, R, p.N, p.nu))))


def dev(a):
    return None if a is None else torch_().from_numpy(np.ascontiguousarray(a)).cuda()


def check_both_entries(h, R, seed, where):
    """JVP and VJP of R vectors against the numpy recursions, through host pointers and through device pointers."""
    A, Bm, K = stacks(h)
    assert np.abs(A).max() > 0 and np.abs(Bm).max() > 0 and np.abs(K).max() > 0, where      # the sweep has left stacks to read
    dx0, gX, gU = vectors(h, R, seed)
    rX, rU = ref_jvp(A, Bm, K, dx0)
    r0 = ref_vjp(A, Bm, K, gX, gU, R)
    for kind, conv in (("host", lambda a: a), ("device", dev)):
        dX, dU = h.plan_jvp(conv(dx0))
        g0 = h.plan_vjp(conv(gX), conv(gU))
        if kind == "device":
            t = torch_()
            assert all(v.is_cuda and v.dtype == t.float64 and v.is_contiguous() for v in (dX, dU, g0)), where
        else:
            assert all(isinstance(v, np.ndarray) for v in (dX, dU, g0)), where
        assert tuple(dX.shape) == rX.shape and tuple(dU.shape) == rU.shape and tuple(g0.shape) == r0.shape, (where, kind)
        assert same(dX, rX), (where, kind, "dX")
        assert same(dU, rU), (where, kind, "dU")
        assert same(g0, r0), (where, kind, "gx0")
    return A, Bm, K


def lti_problem(api, N, max_iterations):
    """LTI 2 x 1, CLDDP, no path constraints, quadratic cost: the optimum is affine in x0"""
    o = api.default_options(); o.max_iterations = max_iterations
    A = np.array([[1.0, 0.1], [-0.2, 0.95]]); Bm = np.array([[0.005], [0.1]])
    p = api.Problem(api.SOLVER_CLDDP, api.MODEL_LTI, api.EULER, 2, 1, N, 0.1, np.diag([1.0, 0.5]), np.array([[0.3]]), np.diag([5.0, 2.0]), np.zeros(2),
                    lti_A=A, lti_B=Bm, options=o)
    p.x0 = np.array([1.0, -0.5])
    return p


def lti_seed(p, x0):
    """U0 = 0 and the rollout of it: CLDDP costs the guess as given, so the guess is made consistent"""
    B = x0.shape[0]
    X0 = np.zeros((B, p.N + 1, p.nx)); X0[:, 0] = x0
    for t in range(p.N):
        X0[:, t + 1] = X0[:, t] @ p.lti_A.T
    return np.zeros((B, p.N, p.nu)), np.ascontiguousarray(X0)


def solved(api, p, B, seed, spread=None, U0=None, X0=None, x0=None):
    if x0 is None:
        x0 = api.batch_x0(p, B, seed, spread)
    if U0 is None:
        U0 = api.batch_U0(p, B)
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0, X0); h.solve()
    return h


@pytest.fixture(scope="module")
def cartpole(api):
    """cart-pole IPDDP with its control box, N = 6, three iterations, B = 70: two tiles, the second one partial.  Shared, never re-solved."""
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=6)
    p.options.max_iterations = 3
    h = solved(api, p, 70, 20261401, [0.1, 0.3, 0.1, 0.1])
    yield h
    h.close()


@pytest.mark.parametrize("chunks", ["default", "4"])
@pytest.mark.parametrize("R", [1, 4, 5])
def test_cartpole_ipddp_bitwise(api, cartpole, monkeypatch, R, chunks):
    """R = 1: one vector per lane; 4: one full chunk; 5: a chunk and a remainder of one -- with chunks of four forced (CDDP_HIP_SENS_RV=4),
    and as the library chooses by itself (one vector per lane and pass at this batch)"""
    if chunks == "4":
        monkeypatch.setenv("CDDP_HIP_SENS_RV", "4")
    check_both_entries(cartpole, R, 20261410 + R, ("cartpole", R, chunks))


@pytest.mark.parametrize("switch", [{"CDDP_HIP_SENS_IO": "staged"}, {"CDDP_HIP_SENS_RV": "4"}, {"CDDP_HIP_SENS_IO": "staged", "CDDP_HIP_SENS_RV": "4"}])
def test_experiment_switches_keep_the_bits(api, cartpole, monkeypatch, switch):
    """The two switches of profiles/scripts/plan_sensitivity.py (read at every call): rows staged through LDS in runs of four steps (N = 6:
    one full run and a tail of two; the second tile's dead lanes help to move the rows) and chunks of four vectors per lane, which a batch
    of two tiles does not get by itself (R = 1: below a chunk; 5: a chunk and a remainder of one; 4: a full chunk)."""
    for k, v in switch.items():
        monkeypatch.setenv(k, v)
    for R in (1, 5):
        check_both_entries(cartpole, R, 20261415 + R, ("cartpole", R, switch))
    A, Bm, K = stacks(cartpole)
    dx0, gX, gU = vectors(cartpole, 4, 20261418)
    assert same(cartpole.plan_jvp(dev(dx0), want=("dU",))[1], ref_jvp(A, Bm, K, dx0)[1])
    assert same(cartpole.plan_vjp(dev(gX), None), ref_vjp(A, Bm, K, gX, None, 4))
    assert same(cartpole.plan_vjp(None, dev(gU)), ref_vjp(A, Bm, K, None, gU, 4))


def test_vector_axis_is_optional(api, cartpole):
    """(B, nx) in, (B, N + 1, nx) out: the same bits as one vector with the axis"""
    h = cartpole
    dx0, gX, gU = vectors(h, 1, 20261420)
    dX, dU = h.plan_jvp(dx0)
    dX1, dU1 = h.plan_jvp(dx0[:, 0])
    assert dX1.shape == (h.B, h.p.N + 1, h.p.nx) and dU1.shape == (h.B, h.p.N, h.p.nu)
    assert same(dX1, dX[:, 0]) and same(dU1, dU[:, 0])
    g = h.plan_vjp(dev(gX[:, 0]), dev(gU[:, 0]))
    assert tuple(g.shape) == (h.B, h.p.nx) and same(g, h.plan_vjp(gX, gU)[:, 0])
    with pytest.raises(ValueError):
        h.plan_vjp(gX, gU[:, 0])                    # one with the axis, one without
    with pytest.raises(ValueError):
        h.plan_vjp(gX, dev(gU))                     # one on the host, one on the device
    with pytest.raises(ValueError):
        h.plan_jvp(dx0, want=())


@pytest.mark.parametrize("kind", ["host", "device"])
def test_null_options(api, cartpole, kind):
    """dX only, dU only, gX = NULL, gU = NULL"""
    h = cartpole
    conv = dev if kind == "device" else (lambda a: a)
    A, Bm, K = stacks(h)
    R = 4
    dx0, gX, gU = vectors(h, R, 20261430)
    rX, rU = ref_jvp(A, Bm, K, dx0)
    dX, none = h.plan_jvp(conv(dx0), want=("dX",))
    assert none is None and same(dX, rX)
    none, dU = h.plan_jvp(conv(dx0), want=("dU",))
    assert none is None and same(dU, rU)
    assert same(h.plan_vjp(None, conv(gU)), ref_vjp(A, Bm, K, None, gU, R))
    assert same(h.plan_vjp(conv(gX), None), ref_vjp(A, Bm, K, gX, None, R))
    lib = api.load_hip()
    buf = np.zeros((h.B, h.p.nx))
    assert lib.cddp_hip_plan_vjp(h.h, 0, 1, None, None, buf.ctypes.data) == 0      # both NULL: the zero gradient
    assert np.all(buf == 0.0)


@pytest.mark.parametrize("t4", ["default", "0"])
def test_quadrotor_sub_tile_minor_bitwise(api, monkeypatch, t4):
    """The quadrotor (nx 13) IPDDP handle with its thrust box runs the G = 16 cooperative sweep, whose A / Bm stacks are sub-tile-minor
    (launch.hpp: route.t4; tests/test_device_io.py::test_sub_tile_minor_linearization reads the same handle).  The library exposes no
    getter of the route, so the layout cannot be asserted from here; instead the same problem also runs under CDDP_HIP_T4=0, which keeps
    the stacks wave-tiled: both maps are walked whichever is the default, and the shapes of cddp_hip_field_shape are asserted."""
    if t4 == "0":
        monkeypatch.setenv("CDDP_HIP_T4", "0")
    p = api.quadrotor_problem(api.SOLVER_IPDDP, 4, True)
    p.options.max_iterations = 2
    assert p.nx > 8
    h = solved(api, p, 70, 20261440, 0.02 * np.ones(p.nx))
    assert h.field_shape("A") == (p.N, p.nx * p.nx) and h.field_shape("B") == (p.N, p.nx * p.nu) and h.field_shape("K") == (p.N, p.nu * p.nx)
    A, Bm = h.linearization(); Ad, Bd = h.linearization_device()
    assert same(Ad, A) and same(Bd, Bm)
    check_both_entries(h, 2, 20261441, ("quadrotor", t4))
    h.close()


def test_pendulum_logddp_bitwise(api):
    p = api.pendulum_problem(api.SOLVER_LOGDDP, True, horizon=5)
    p.options.max_iterations = 3
    h = solved(api, p, 64, 20261450, [0.3, 0.3])
    check_both_entries(h, 3, 20261451, "pendulum logddp")
    h.close()


def test_shortest_horizon_bitwise(api):
    """LTI 2 x 1 CLDDP, N = 1: lam starts at gX_1 and is stepped once"""
    p = lti_problem(api, 1, 3)
    x0 = api.batch_x0(p, 5, 20261460, [1.0, 1.0]); U0, X0 = lti_seed(p, x0)
    h = solved(api, p, 5, 0, x0=x0, U0=U0, X0=X0)
    A, Bm, K = check_both_entries(h, 2, 20261461, "lti N=1")
    assert same(A[:, 0], np.broadcast_to(p.lti_A, (5, 2, 2))) and same(Bm[:, 0], np.broadcast_to(p.lti_B, (5, 2, 1)))
    h.close()


def test_two_tile_groups(api, monkeypatch):
    """B = 130 in two groups (cddp_hip_create: whole tiles per group, the first gets the odd one -- trajectories 0..127 and 128..129): the
    caller's pointers are offset per group, and the results are the bits of two single-group handles over the two parts."""
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=7)
    p.options.max_iterations = 3
    B, R = 130, 5
    split = ((((B + 63) // 64) + 1) // 2) * 64
    x0 = api.batch_x0(p, B, 20261470, np.array([1.0, 1.0])); U0 = api.batch_U0(p, B)
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0); h.solve()
    assert h.num_groups() == 2
    monkeypatch.setenv("CDDP_HIP_GROUPS", "1")
    parts = []
    for sl in (slice(0, split), slice(split, B)):
        q = api.HipBatchSolver(p, sl.stop - sl.start); q.set_initial(x0[sl], U0[sl] if U0 is not None else None); q.solve()
        assert q.num_groups() == 1
        parts.append((sl, q))
    check_both_entries(h, R, 20261471, "two groups")
    dx0, gX, gU = vectors(h, R, 20261472)
    for kind, conv in (("host", lambda a: a), ("device", dev)):
        dX, dU = h.plan_jvp(conv(dx0)); g0 = h.plan_vjp(conv(gX), conv(gU))
        for sl, q in parts:
            qX, qU = q.plan_jvp(conv(dx0[sl])); q0 = q.plan_vjp(conv(gX[sl]), conv(gU[sl]))
            assert same(dX[sl], qX) and same(dU[sl], qU) and same(g0[sl], q0), (kind, sl)
    h.close()
    for _, q in parts:
        q.close()


def test_state_untouched(api):
    """get_trajectory, get_gains and get_results are the same bits before and after a JVP and a VJP, and a following solve gives what it
    gives without the calls."""
    import test_mpc_advance as M
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=6)
    p.options.max_iterations = 3
    a = solved(api, p, 70, 20261480, [0.1, 0.3, 0.1, 0.1]); b = solved(api, p, 70, 20261480, [0.1, 0.3, 0.1, 0.1])
    before = (a.trajectory(), a.gains(), a.results())
    dx0, gX, gU = vectors(a, 4, 20261481)
    a.plan_jvp(dx0); a.plan_vjp(gX, gU); a.plan_jvp(dev(dx0)); a.plan_vjp(dev(gX), dev(gU))
    after = (a.trajectory(), a.gains(), a.results())
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert same(x, y)
    assert before[2].tobytes() == after[2].tobytes()
    a.solve(); b.solve()
    M.assert_same_solve(a, b, "after the sensitivities", duals=True)
    a.close(); b.close()


def test_refusals_on_the_device(api, cartpole):
    t = torch_()
    lib = api.load_hip()
    h = cartpole
    B, N, nx, nu = h.B, h.p.N, h.p.nx, h.p.nu
    dx0, gX, gU = vectors(h, 1, 20261490)
    good0 = dev(dx0); outX = t.zeros((B, 1, N + 1, nx), dtype=t.float64, device="cuda"); outU = t.zeros((B, 1, N, nu), dtype=t.float64, device="cuda")
    host = np.zeros((B, 1, N + 1, nx))

    def message():
        return lib.cddp_hip_last_error().decode()

    # a host pointer passed as a device pointer: never reaches a kernel
    assert lib.cddp_hip_plan_jvp(h.h, api.SENS_DEVICE, 1, dx0.ctypes.data, outX.data_ptr(), outU.data_ptr()) != 0
    assert "cddp_hip_plan_jvp: dx0 is not device memory" in message()
    assert lib.cddp_hip_plan_jvp(h.h, api.SENS_DEVICE, 1, good0.data_ptr(), host.ctypes.data, None) != 0
    assert "cddp_hip_plan_jvp: dX is not device memory" in message()
    assert lib.cddp_hip_plan_vjp(h.h, api.SENS_DEVICE, 1, gX.ctypes.data, None, good0.data_ptr()) != 0
    assert "cddp_hip_plan_vjp: gX is not device memory" in message()
    # a tensor one element short: the binding refuses the shape before the call (the C entry's own check of the allocation's end is
    # exercised below with an nvec the arrays do not hold, and with a hipMalloc one element short in tests/cpp/test_plan_sens_wrapper.cpp:
    # torch's allocator hands out blocks, so the end of a tensor is not the end of its allocation)
    short = t.zeros(B * (N + 1) * nx - 1, dtype=t.float64, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        h.plan_jvp(short)
    with pytest.raises(ValueError, match="shape"):
        h.plan_vjp(dev(gX).reshape(-1)[:-1], None)
    hugeR = 1 << 20                                               # an nvec the arrays do not hold: the end of every allocation is checked
    assert lib.cddp_hip_plan_jvp(h.h, api.SENS_DEVICE, hugeR, good0.data_ptr(), outX.data_ptr(), None) != 0
    assert "its allocation ends after" in message()
    assert float(outX.abs().max()) == 0.0 and float(outU.abs().max()) == 0.0 and np.all(host == 0.0)
    # a handle that was never solved
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=6)
    fresh = api.HipBatchSolver(p, 8)
    with pytest.raises(api.HipError, match="cddp_hip_plan_jvp needs a solved handle"):
        fresh.plan_jvp(np.zeros((8, 4)))
    with pytest.raises(api.HipError, match="cddp_hip_plan_vjp needs a solved handle"):
        fresh.plan_vjp(np.zeros((8, 7, 4)), None)
    fresh.close()
    # an MSIPDDP handle
    import test_msipddp_device as MS
    pm = MS.make(api, "pendulum_box")[0]
    pm.options.max_iterations = 2
    ms = solved(api, pm, 8, 20261491, [0.1, 0.1])
    with pytest.raises(api.HipError, match="cddp_hip_plan_jvp: not for an MSIPDDP handle"):
        ms.plan_jvp(np.zeros((8, pm.nx)))
    with pytest.raises(api.HipError, match="cddp_hip_plan_vjp: not for an MSIPDDP handle"):
        ms.plan_vjp(None, np.zeros((8, pm.N, pm.nu)))
    ms.close()


def test_adjoint_consistency(api, cartpole):
    """The dense dX_N / dx0 of the cart-pole batch, once from the JVP of the nx unit vectors (through plan_jacobian_device) and once from
    the VJP of the nx unit cotangents on row N.  Both evaluate the same product M = Phi_{N-1} ... Phi_0, Phi_t = A_t + B_t K_t, in different
    orders.  Bound: one step of either recursion computes sums of at most nx + nu products each entering through at most one more sum of
    nx products (du or mu first), so every computed entry carries a relative error of at most gamma = (nx + nu + 2) u per step on the
    absolute-value recursion (u = 2^-53: nx + nu - 1 additions, one product, one nested product); over N steps N gamma, and two such
    evaluations differ by at most 2 N (nx + nu + 2) 2^-53 times the chain evaluated on |A_t|, |B_t|, |K_t|.  The same bound holds against
    the chain evaluated by mpmath at 60 digits from the same doubles (one evaluation's error, so half of it would do)."""
    import mpmath
    h = cartpole
    t = torch_()
    B, N, nx, nu = h.B, h.p.N, h.p.nx, h.p.nu
    A, Bm, K = stacks(h)
    dXdx0, dUdx0 = h.plan_jacobian_device()
    assert tuple(dXdx0.shape) == (B, N + 1, nx, nx) and tuple(dUdx0.shape) == (B, N, nu, nx)
    J_fwd = dXdx0[:, N].cpu().numpy()                                     # [b, i, j] = d X_N[i] / d x0[j]
    gX = np.zeros((B, nx, N + 1, nx)); gX[:, np.arange(nx), N, np.arange(nx)] = 1.0
    J_adj = h.plan_vjp(dev(gX), None).cpu().numpy()                        # [b, i, j]: cotangent e_i on row N -> gradient with respect to x0[j]
    absM = np.broadcast_to(np.eye(nx), (B, nx, nx)).copy()
    for s in range(N):
        absM = np.matmul(np.abs(A[:, s]) + np.matmul(np.abs(Bm[:, s]), np.abs(K[:, s])), absM)
    bound = 2.0 * N * (nx + nu + 2) * 2.0 ** -53 * absM
    err = np.abs(J_fwd - J_adj)
    print("adjoint consistency: max |J_fwd - J_adj| = %.3e, smallest bound %.3e, worst ratio %.3f" % (err.max(), bound.min(), (err / bound).max()))
    assert np.all(err <= bound)
    assert same(dXdx0[:, 0], np.broadcast_to(np.eye(nx), (B, nx, nx)))
    mpmath.mp.dps = 60
    worst = 0.0
    for b in (0, 1, 63, 64, B - 1):                                        # both tiles, their edges
        M = mpmath.eye(nx)
        for s in range(N):
            Phi = mpmath.matrix(A[b, s].tolist()) + mpmath.matrix(Bm[b, s].tolist()) * mpmath.matrix(K[b, s].tolist())
            M = Phi * M
        for i in range(nx):
            for j in range(nx):
                for J in (J_fwd, J_adj):
                    e = abs(mpmath.mpf(float(J[b, i, j])) - M[i, j])
                    worst = max(worst, float(e / mpmath.mpf(float(bound[b, i, j]))))
                    assert e <= mpmath.mpf(float(bound[b, i, j])), (b, i, j)
    print("against mpmath: worst error / bound = %.3f" % worst)


def test_meaning_end_to_end(api):
    """LTI 2 x 1, CLDDP, no path constraints, quadratic cost, N = 8, five iterations: the optimum is exactly affine in x0, so the plan solved
    at x0 + d is the plan at x0 plus the linear response to d, up to what the solver leaves.  D = max |X(x0 + d) - X(x0) - dX d| (and the
    same for U) on the GPU must stay within 8 x the same quantity from the CPU oracle's two solves and the numpy recursion on the oracle's
    gains (the factor covers two implementations that agree to rounding only); were the oracle's exactly zero, 8 ulp of max |X| are allowed."""
    p = lti_problem(api, 8, 5)
    B = 64
    rng = np.random.default_rng(20261500)
    x0 = api.batch_x0(p, B, 20261500, [1.0, 1.0])
    assert len(np.unique(x0, axis=0)) == B
    d = rng.standard_normal((B, 2)); d = np.ascontiguousarray(0.1 * d / np.linalg.norm(d, axis=1, keepdims=True))
    U0a, X0a = lti_seed(p, x0); U0b, X0b = lti_seed(p, x0 + d)
    ha = solved(api, p, B, 0, x0=x0, U0=U0a, X0=X0a); hb = solved(api, p, B, 0, x0=x0 + d, U0=U0b, X0=X0b)
    Xa, Ua = ha.trajectory(); Xb, Ub = hb.trajectory()
    dX, dU = ha.plan_jvp(d)
    ha.close(); hb.close()
    Dx_gpu = float(np.abs(Xb - Xa - dX).max()); Du_gpu = float(np.abs(Ub - Ua - dU).max())
    _, oXa, oUa, oKa, _ = api.oracle_solve_batch(p, x0, U0a, X0a, n_threads=4)
    _, oXb, oUb, _, _ = api.oracle_solve_batch(p, x0 + d, U0b, X0b, n_threads=4)
    oA = np.ascontiguousarray(np.broadcast_to(p.lti_A, (B, p.N, 2, 2))); oB = np.ascontiguousarray(np.broadcast_to(p.lti_B, (B, p.N, 2, 1)))
    odX, odU = ref_jvp(oA, oB, oKa, d[:, None, :])
    Dx_ref = float(np.abs(oXb - oXa - odX[:, 0]).max()); Du_ref = float(np.abs(oUb - oUa - odU[:, 0]).max())
    print("meaning: D_gpu X %.3e U %.3e | D_ref X %.3e U %.3e | max |X| %.3e max |U| %.3e" % (Dx_gpu, Du_gpu, Dx_ref, Du_ref, np.abs(Xa).max(), np.abs(Ua).max()))
    assert np.abs(Xb - Xa).max() > 1e-3                              # the plans do differ: the response is not compared with nothing
    ulp = 2.0 ** -52
    assert Dx_gpu <= (8.0 * Dx_ref if Dx_ref > 0.0 else 8.0 * ulp * np.abs(Xa).max())
    assert Du_gpu <= (8.0 * Du_ref if Du_ref > 0.0 else 8.0 * ulp * np.abs(Xa).max())


def _facade():
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py"))
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


def test_autograd(api):
    """solve_batch_diff on the LTI problem, loss = (w X).sum() + (v U).sum(): x0.grad is bitwise plan_vjp(w, v); the seed gets no gradient;
    a second solve on the same solver before loss.backward() raises the stale-plan error; refresh=True re-sweeps at the returned plan."""
    t = torch_()
    pycddp = _facade()
    p = lti_problem(api, 8, 5)
    B = 64
    x0n = api.batch_x0(p, B, 20261510, [1.0, 1.0])
    U0n, X0n = lti_seed(p, x0n)
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 5
    sv = pycddp.CDDP(x0n[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.LTISystem(p.lti_A, p.lti_B, p.dt, "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    rng = np.random.default_rng(20261511)
    w = dev(rng.standard_normal((B, p.N + 1, p.nx))); v = dev(rng.standard_normal((B, p.N, p.nu)))

    def run(refresh=False):
        x0 = dev(x0n).requires_grad_(True); U0 = dev(U0n).requires_grad_(True)
        out = sv.solve_batch_diff(x0, U0, dev(X0n), solver_type=pycddp.SolverType.CLDDP, refresh=refresh)
        return x0, U0, out

    x0, U0, out = run()
    hs = out["solver"]
    plain = sv.solve_batch_device(dev(x0n), dev(U0n), dev(X0n), solver_type=pycddp.SolverType.CLDDP)
    assert same(out["X"], plain["X"]) and same(out["U"], plain["U"]) and same(out["results"]["iterations"], plain["results"]["iterations"])
    assert out["X"].requires_grad and out["U"].requires_grad
    loss = (w * out["X"]).sum() + (v * out["U"]).sum()
    want = hs.plan_vjp(w, v)
    loss.backward()
    assert x0.grad is not None and same(x0.grad, want) and float(want.abs().max()) > 0.0
    assert U0.grad is None
    hs.close()
    # only U enters the loss: gX arrives as zeros (or None), the gradient is plan_vjp(None, v) in value
    x0, U0, out = run()
    (v * out["U"]).sum().backward()
    assert np.allclose(x0.grad.cpu().numpy(), out["solver"].plan_vjp(None, v).cpu().numpy(), rtol=0, atol=0)
    out["solver"].close()
    # the stale plan
    x0, U0, out = run()
    loss = (w * out["X"]).sum()
    out["solver"].solve()
    with pytest.raises(RuntimeError, match="stale plan"):
        loss.backward()
    assert x0.grad is None
    out["solver"].close()
    # refresh: one more sweep at the returned plan; for this problem K does not depend on the iterate, A and B are the plant's
    x0, U0, out = run(refresh=True)
    (w * out["X"]).sum().backward()
    assert same(x0.grad, out["solver"].plan_vjp(w, None))
    out["solver"].close()
