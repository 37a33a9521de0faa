"""Device-resident inputs and outputs of a batch solve (cddp_hip_get_field_device, cddp_hip_get_results_device, cddp_hip_set_initial_device;
csrc/inst_io.hip): the kernels move data and do no arithmetic, so the contract is BITWISE equality with the host entries -- every
comparison is np.array_equal (NaN = NaN, as tests/test_mpc_advance.py::same).
Shapes: B = 1 (one lane of one tile), 64 (one full tile), 70 (a partial second tile: padding lanes), 130 in two tile groups (the pointer
offsets of the second group); horizons whose column counts (N + 1) * nx and N * nu are below, equal to and above the 64 columns a workgroup
of the kernels moves, and no multiple of it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = 64          # columns (t, e) per workgroup of the staged kernels (inst_io.hip::kIoCols)


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


def has_duals(api, p):
    return p.c.solver in (api.SOLVER_IPDDP, api.SOLVER_MSIPDDP) and p.dual_dim() > 0


def has_costates(api, p):
    return p.c.solver in (api.SOLVER_IPDDP, api.SOLVER_MSIPDDP)


def host_fields(api, h):
    """every field the problem has, from its HOST getter, as (B, T, E)"""
    B = h.B
    X, U = h.trajectory(); K, k = h.gains(); Vx, Vxx = h.value(); A, Bm = h.linearization()
    out = {"X": X, "U": U, "K": K.reshape(B, K.shape[1], -1), "KFF": k, "VX": Vx, "VXX": Vxx.reshape(B, Vxx.shape[1], -1),
           "A": A.reshape(B, A.shape[1], -1), "B": Bm.reshape(B, Bm.shape[1], -1)}
    if has_duals(api, h.p):
        out["S"], out["Y"], out["G"] = h.duals()
    if has_costates(api, h.p):
        out["LAMBDA"] = h.costates()
    return out


def assert_getters_equal(api, h, where):
    want = host_fields(api, h)
    for name, ref in want.items():
        got = h.field_device(name)
        assert tuple(got.shape) == ref.shape == (h.B,) + h.field_shape(name), (where, name, tuple(got.shape), ref.shape)
        assert got.dtype == torch_().float64 and got.is_cuda and got.is_contiguous()
        assert same(got, ref), (where, name)
    # the named wrappers return the same arrays in the shapes of their numpy twins
    Xd, Ud = h.trajectory_device(); Kd, kd = h.gains_device(); Vxd, Vxxd = h.value_device(); Ad, Bd = h.linearization_device()
    K, k = h.gains(); Vx, Vxx = h.value(); A, Bm = h.linearization()
    assert same(Xd, want["X"]) and same(Ud, want["U"]) and same(Kd, K) and same(kd, k) and same(Vxd, Vx) and same(Vxxd, Vxx) and same(Ad, A) and same(Bd, Bm), where
    if "S" in want:
        for d, r in zip(h.duals_device(), h.duals()):
            assert same(d, r), where
    if "LAMBDA" in want:
        assert same(h.costates_device(), want["LAMBDA"]), where
    return want


def make_case(api, case):
    import test_gpu_parity as T
    if case == "logddp_pendulum_box":
        import test_logddp_device as LG
        return LG.make(api, "pendulum_box"), 0.1 * np.ones(2)
    if case == "msipddp_pendulum_box":
        import test_msipddp_device as MS
        return MS.make(api, "pendulum_box")[0], 0.1 * np.ones(2)
    import test_mpc_advance as M
    return T.make(api, case), np.array(M.WIDE_SPREAD[case])


GETTER_CASES = ["pendulum_ipddp_box", "unicycle_ipddp_box_ball", "pendulum_clddp_box", "logddp_pendulum_box", "msipddp_pendulum_box"]
WIDE_CASES = ("pendulum_ipddp_box", "unicycle_ipddp_box_ball", "pendulum_clddp_box")   # tests/test_mpc_advance.py::WIDE_SPREAD


@pytest.mark.parametrize("B", [1, 64, 70])
@pytest.mark.parametrize("case", GETTER_CASES)
def test_getters_equal_host_getters(api, case, B):
    """After a cold solve every field the problem has equals its host getter.  At the wide x0 spreads of tests/test_mpc_advance.py the batch
    ends with trajectories in three or more live slots: asserted (cddp_hip_get_live_slots), since with fewer the per-trajectory slot
    addressing of the slotted fields would not be exercised."""
    p, spread = make_case(api, case)
    x0 = api.batch_x0(p, B, 20261201, spread); U0 = api.batch_U0(p, B)
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0); h.solve()
    slots = h.live_slots()
    print("%s B=%d: live slots %s" % (case, B, np.unique(slots).tolist()))
    assert_getters_equal(api, h, (case, B))
    if case in WIDE_CASES and B >= 64:
        assert len(np.unique(slots)) >= 3, (case, B, np.unique(slots).tolist())
    h.close()


@pytest.mark.parametrize("N", [5, 31, 37, 64])
def test_column_chunks(api, N):
    """Pendulum (nx 2, nu 1): N = 5 -> 12 and 5 columns (a fraction of a chunk); N = 31 -> X is exactly one chunk of 64; N = 37 -> 76 columns
    (a full chunk and a short one); N = 64 -> U is exactly one chunk, X two full chunks and a short one."""
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=N)
    p.options.max_iterations = 6
    assert (((N + 1) * p.nx) % COLS == 0) == (N == 31) and ((N * p.nu) % COLS == 0) == (N == 64)
    B = 70
    x0 = api.batch_x0(p, B, 20261202, np.array([3.0, 3.0])); U0 = api.batch_U0(p, B)
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0); h.solve()
    assert_getters_equal(api, h, N)
    # and the seed direction at this horizon
    X, U = h.trajectory()
    a = api.HipBatchSolver(p, B); b = api.HipBatchSolver(p, B)
    a.set_initial(np.ascontiguousarray(X[:, 0]), U, X)
    t = torch_()
    b.set_initial_device(t.from_numpy(np.ascontiguousarray(X[:, 0])).cuda(), t.from_numpy(U).cuda(), t.from_numpy(X).cuda())
    a.solve(); b.solve()
    import test_mpc_advance as M
    M.assert_same_solve(a, b, ("seed", N), duals=True)
    for q in (h, a, b):
        q.close()


@pytest.mark.parametrize("t4", ["default", "0"])
def test_sub_tile_minor_linearization(api, monkeypatch, t4):
    """The quadrotor (nx 13) IPDDP handle runs the G = 16 cooperative sweep, whose A / Bm stacks are sub-tile-minor (launch.hpp: route.t4;
    tests/test_linearization.py reads them through from_t4 on the host).  A, B from the device getter equal linearization() -- on the
    default handle and on one created under CDDP_HIP_T4=0, which keeps the same stacks wave-tiled: both maps are walked whichever is the default."""
    if t4 == "0":
        monkeypatch.setenv("CDDP_HIP_T4", "0")
    p = api.quadrotor_problem(api.SOLVER_IPDDP, 12, True)
    p.options.max_iterations = 3
    B = 70
    x0 = api.batch_x0(p, B, 20261203, 0.02 * np.ones(p.nx))
    h = api.HipBatchSolver(p, B); h.set_initial(x0); h.solve()
    A, Bm = h.linearization()
    assert np.abs(A).max() > 0 and np.abs(Bm).max() > 0
    Ad, Bd = h.linearization_device()
    assert same(Ad, A) and same(Bd, Bm)
    assert_getters_equal(api, h, "quadrotor")
    h.close()


def seed_pair(api, p, B, x0, U0, X0):
    t = torch_()
    a = api.HipBatchSolver(p, B); b = api.HipBatchSolver(p, B)
    a.set_initial(x0, U0, X0)
    dev = lambda v: None if v is None else t.from_numpy(np.ascontiguousarray(v)).cuda()
    b.set_initial_device(dev(x0), dev(U0), dev(X0))
    return a, b


@pytest.mark.parametrize("B", [64, 70])
@pytest.mark.parametrize("case", ["pendulum_ipddp_box", "pendulum_clddp_box"])
def test_seed_from_device_equals_seed_from_host(api, case, B):
    """Handle A: set_initial from numpy; handle B: set_initial_device with the same numbers.  CLDDP linearises X0 as given, so a wrong X0
    row shows; row 0 of X0 is deliberately NOT x0 (the seed's row 0 must be x0 either way).  B = 70: the padding lanes of the last tile."""
    import test_gpu_parity as T
    import test_mpc_advance as M
    p = T.make(api, case)
    rng = np.random.default_rng(20261204 + B)
    x0 = api.batch_x0(p, B, 20261204, np.array([3.0, 3.0]))
    U0 = np.ascontiguousarray(0.5 * rng.standard_normal((B, p.N, p.nu)))
    X0 = np.ascontiguousarray(x0[:, None, :] + 0.05 * rng.standard_normal((B, p.N + 1, p.nx)))
    ip = M.is_ipddp(api, p)
    for name, (u, x) in {"U0 and X0": (U0, X0), "X0 = None": (U0, None), "U0 = None": (None, X0), "neither": (None, None)}.items():
        a, b = seed_pair(api, p, B, x0, u, x)
        a.solve(); b.solve()
        M.assert_same_solve(a, b, (case, B, name), duals=ip)
        a.close(); b.close()


@pytest.mark.parametrize("case", ["pendulum_ipddp_box", "unicycle_ipddp_box_ball", "pendulum_clddp_box"])
def test_warm_resolve_from_a_torch_shift(api, case):
    """solve, trajectory_device(), shift with torch, set_initial_device -- against the host shift sequence of tests/test_mpc_advance.py."""
    import test_gpu_parity as T
    import test_mpc_advance as M
    t = torch_()
    p = T.make(api, case)
    a, b, _, _ = M.pair(api, p, 70, 20261205, spread=np.array(M.WIDE_SPREAD[case]))
    for k, provided in enumerate((True, False, True)):
        Xs, Us = M.host_shift(a, provided)
        X, U = b.trajectory_device()
        Xd = t.cat([X[:, 1:], X[:, -1:]], dim=1).contiguous(); Ud = t.cat([U[:, 1:], U[:, -1:]], dim=1).contiguous()
        assert same(Xd, Xs) and same(Ud, Us), (case, k)
        if provided:
            b.forget_solver_state()
        b.set_initial_device(Xd[:, 0].contiguous(), Ud, Xd)
        a.solve(); b.solve()
        M.assert_same_solve(a, b, (case, k), duals=(not provided) and M.is_ipddp(api, p))
    a.close(); b.close()


def test_two_tile_groups(api, monkeypatch):
    """B = 130 in two groups (two tiles + one partial): the caller's pointers are offset by the group's first trajectory on both sides."""
    import test_gpu_parity as T
    import test_mpc_advance as M
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    p = T.make(api, "pendulum_ipddp_box")
    B = 130
    rng = np.random.default_rng(20261206)
    x0 = api.batch_x0(p, B, 20261206, np.array([3.0, 3.0]))
    U0 = np.ascontiguousarray(0.5 * rng.standard_normal((B, p.N, p.nu)))
    X0 = np.ascontiguousarray(x0[:, None, :] + 0.05 * rng.standard_normal((B, p.N + 1, p.nx)))
    a, b = seed_pair(api, p, B, x0, U0, X0)
    assert a.num_groups() == 2 and b.num_groups() == 2
    a.solve(); b.solve()
    M.assert_same_solve(a, b, "two groups", duals=True)
    assert_getters_equal(api, b, "two groups")
    assert len(np.unique(b.live_slots())) >= 3
    ra, rb = a.results(), b.results_device()
    for name in api.RESULT_DTYPE.names:
        assert same(rb[name], ra[name]), name
    a.close(); b.close()


@pytest.mark.parametrize("case,B", [("pendulum_ipddp_box", 70), ("pendulum_clddp_box", 1), ("msipddp_pendulum_box", 64)])
def test_results_device_equals_results(api, case, B):
    p, spread = make_case(api, case)
    x0 = api.batch_x0(p, B, 20261207, spread)
    h = api.HipBatchSolver(p, B); h.set_initial(x0, api.batch_U0(p, B)); h.solve()
    r = h.results(); d = h.results_device()
    t = torch_()
    assert d["cols"].shape == (B, 10) and d["icols"].shape == (B, 4) and d["icols"].dtype == t.int32
    for name in api.RESULT_DTYPE.names:
        assert d[name].shape == (B,) and same(d[name], r[name]), (case, name)
    assert int(d["iterations"].max()) > 0
    h.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_user_stream_orders_seed_and_outputs(api, monkeypatch, groups):
    """With set_stream(torch stream): a seed written by torch ops queued on that stream right before set_initial_device is the seed the
    solve uses, and a field_device output consumed by a torch op queued on that stream right after is complete.  (One group runs on the
    stream itself; two groups fork from and join to it.)"""
    import test_gpu_parity as T
    import test_mpc_advance as M
    t = torch_()
    monkeypatch.setenv("CDDP_HIP_GROUPS", str(groups))
    p = T.make(api, "pendulum_ipddp_box")
    B = 130
    rng = np.random.default_rng(20261208)
    x0 = api.batch_x0(p, B, 20261208, np.array([3.0, 3.0]))
    U0 = np.ascontiguousarray(0.5 * rng.standard_normal((B, p.N, p.nu)))
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0); a.solve()
    b = api.HipBatchSolver(p, B)
    assert b.num_groups() == groups
    s = t.cuda.Stream()
    b.set_stream(s.cuda_stream)
    half_x = t.from_numpy(0.5 * x0).cuda(); half_u = t.from_numpy(0.5 * U0).cuda()     # (exact halves: doubling restores the bits)
    big = t.zeros((2048, 2048), dtype=t.float64, device="cuda")
    t.cuda.synchronize()
    with t.cuda.stream(s):
        for _ in range(4):
            big = big @ big                      # work in front of the seed on the stream: an unordered read would see zeros
        xd = t.zeros_like(half_x); ud = t.zeros_like(half_u)
        xd.add_(half_x, alpha=2.0); ud.add_(half_u, alpha=2.0)
        b.set_initial_device(xd, ud)
        b.solve()
        Xd = b.field_device("X")
        Xc = Xd * 1.0                            # consumed on the stream, no synchronisation in between
        Ud = b.field_device("U"); Uc = Ud.clone()
    s.synchronize()
    X, U = a.trajectory()
    assert same(Xc, X) and same(Uc, U)
    M.assert_same_solve(a, b, ("stream", groups), duals=True)
    a.close(); b.close()


def test_refusals_change_nothing(api):
    import test_gpu_parity as T
    import test_mpc_advance as M
    t = torch_()
    lib = api.load_hip()
    p = T.make(api, "pendulum_ipddp_box")
    B = 70
    x0 = api.batch_x0(p, B, 20261209, T.spread_for(p)); U0 = api.batch_U0(p, B)
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0); a.solve()
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0); b.solve()

    def unchanged(where):
        a.solve(); b.solve()
        M.assert_same_solve(a, b, where, duals=True)

    good = t.from_numpy(x0).cuda()
    Ud = t.zeros((B, p.N, p.nu), dtype=t.float64, device="cuda")
    bad = {"wrong shape": t.zeros((B, p.nx + 1), dtype=t.float64, device="cuda"),
           "wrong batch": t.zeros((B - 1, p.nx), dtype=t.float64, device="cuda"),
           "wrong dtype": t.zeros((B, p.nx), dtype=t.float32, device="cuda"),
           "non-contiguous": t.zeros((B, 2 * p.nx), dtype=t.float64, device="cuda")[:, ::2],
           "cpu tensor": t.zeros((B, p.nx), dtype=t.float64),
           "numpy array": np.zeros((B, p.nx))}
    if t.cuda.device_count() > 1:
        bad["other device"] = t.zeros((B, p.nx), dtype=t.float64, device="cuda:1")
    for name, v in bad.items():
        assert name != "non-contiguous" or not v.is_contiguous()
        with pytest.raises(ValueError):
            b.set_initial_device(v)
        unchanged(name)
    with pytest.raises(ValueError):
        b.set_initial_device(good, U0=Ud[:, :-1])
    with pytest.raises(ValueError):
        b.set_initial_device(good, X0=Ud)
    with pytest.raises(ValueError):
        b.field_device("X", out=t.zeros((B, p.N + 1, p.nx), dtype=t.float32, device="cuda"))
    with pytest.raises(ValueError):
        b.field_device("Q")
    unchanged("python refusals")

    # in C
    def refused(rc, text):
        assert rc != 0
        msg = lib.cddp_hip_last_error().decode()
        assert text in msg, msg
        with pytest.raises(api.HipError):
            b._check(rc)

    out = t.zeros((B, p.N + 1, p.nx), dtype=t.float64, device="cuda")
    refused(lib.cddp_hip_get_field_device(b.h, 99, out.data_ptr()), "unknown field id 99")
    refused(lib.cddp_hip_get_field_device(b.h, -1, out.data_ptr()), "unknown field id -1")
    refused(lib.cddp_hip_field_shape(b.h, 12, None, None), "unknown field id 12")
    refused(lib.cddp_hip_get_field_device(b.h, api.FIELD_IDS["X"], None), "null output pointer")
    refused(lib.cddp_hip_set_initial_device(b.h, None, None, None), "null x0 pointer")
    refused(lib.cddp_hip_get_results_device(b.h, None, None), "null output pointer")
    unchanged("unknown field / null pointers")
    # a PINNED HOST tensor: the device can address it, so it stays harmless -- and it is refused as not device memory
    pinned = t.zeros((B, p.N + 1, p.nx), dtype=t.float64).pin_memory()
    assert pinned.is_pinned()
    refused(lib.cddp_hip_get_field_device(b.h, api.FIELD_IDS["X"], pinned.data_ptr()), "not device memory")
    assert float(pinned.abs().max()) == 0.0                       # nothing was written
    pin_x0 = t.from_numpy(x0 + 1.0).pin_memory()
    refused(lib.cddp_hip_set_initial_device(b.h, pin_x0.data_ptr(), None, None), "x0 is not device memory")
    refused(lib.cddp_hip_set_initial_device(b.h, good.data_ptr(), pinned.data_ptr(), None), "U0 is not device memory")
    refused(lib.cddp_hip_set_initial_device(b.h, good.data_ptr(), None, pinned.data_ptr()), "X0 is not device memory")
    ipin = t.zeros((B, 4), dtype=t.int32).pin_memory()
    cols = t.zeros((B, 10), dtype=t.float64, device="cuda")
    refused(lib.cddp_hip_get_results_device(b.h, cols.data_ptr(), ipin.data_ptr()), "not device memory")
    assert float(cols.abs().max()) == 0.0                         # checked before anything was launched
    unchanged("pinned host pointers")
    a.close(); b.close()

    pc = T.make(api, "pendulum_clddp_box")
    a = api.HipBatchSolver(pc, B); a.set_initial(x0, U0); a.solve()
    b = api.HipBatchSolver(pc, B); b.set_initial(x0, U0); b.solve()
    for f in ("S", "Y", "G"):
        refused(lib.cddp_hip_get_field_device(b.h, api.FIELD_IDS[f], out.data_ptr()), "no slack/dual trajectories for this problem")
        with pytest.raises(api.HipError):
            b.field_device(f)
    refused(lib.cddp_hip_get_field_device(b.h, api.FIELD_IDS["LAMBDA"], out.data_ptr()), "no costate trajectory for this solver")
    with pytest.raises(api.HipError):
        b.duals_device()
    with pytest.raises(api.HipError):
        b.costates_device()
    a.solve(); b.solve()
    M.assert_same_solve(a, b, "clddp after the refusals")
    a.close(); b.close()


def _facade():
    import importlib.util, os, sys
    name = "pycddp_amd"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py"))
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


def test_facade_solve_batch_device(api):
    import test_gpu_parity as T
    t = torch_()
    pycddp = _facade()
    p = T.make(api, "pendulum_ipddp_box")
    B = 8
    x0 = api.batch_x0(p, B, 20261210, T.spread_for(p))
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False
    o.max_iterations = p.options.max_iterations; o.tolerance = p.options.tolerance; o.acceptable_tolerance = p.options.acceptable_tolerance
    o.regularization.initial_value = p.options.reg_initial_value
    sv = pycddp.CDDP(x0[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.Pendulum(p.dt, *list(p.c.model_params)[:3], "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    sv.add_constraint("ControlConstraint", pycddp.ControlConstraint(np.array([-20.0]), np.array([20.0])))
    sols = sv.solve_batch(list(x0), pycddp.SolverType.IPDDP)
    out = sv.solve_batch_device(t.from_numpy(x0).cuda(), solver_type=pycddp.SolverType.IPDDP, want=("X", "U", "K"))
    assert out["X"].is_cuda and tuple(out["X"].shape) == (B, p.N + 1, p.nx) and tuple(out["K"].shape) == (B, p.N, p.nu * p.nx)
    assert same(out["X"], np.stack([np.stack(s.state_trajectory) for s in sols]))
    assert same(out["U"], np.stack([np.stack(s.control_trajectory) for s in sols]))
    assert same(out["K"].view(B, p.N, p.nu, p.nx), np.stack([np.stack(s.feedback_gains) for s in sols]))
    assert same(out["results"]["iterations"], np.array([s.iterations_completed for s in sols], dtype=np.int32))
    assert same(out["results"]["final_objective"], np.array([s.final_objective for s in sols]))
    with pytest.raises(ValueError):
        sv.solve_batch_device(t.from_numpy(x0), solver_type=pycddp.SolverType.IPDDP)          # a CPU tensor

    class HostPendulum(pycddp.Pendulum):     # a Python plant: solve_batch sends it to the plug-in route, which has no resident handle
        def __init__(self, *a):
            super().__init__(*a); self.model = None
    sv.set_dynamical_system(HostPendulum(p.dt, *list(p.c.model_params)[:3], "euler"))
    with pytest.raises(NotImplementedError):
        sv.solve_batch_device(t.from_numpy(x0).cuda(), solver_type=pycddp.SolverType.IPDDP)
