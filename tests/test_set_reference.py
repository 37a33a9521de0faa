"""Moving the goal and the per-step reference of a live handle (cddp_hip_set_reference, cddp_hip_get_reference).  The contract is BITWISE:
"handle A created with reference r1, set_reference(r2), solve" equals "handle B created with r2, solve" -- results, trajectory, duals --
and get_reference() on A returns r2 bit for bit.  Every comparison is np.array_equal.

Per case and reference change, both handles go through the same calls but for the reference: create, set_initial, a cold solve (A under
r1, B under r2), then A.set_reference(r2), a cold solve on both, and a warm-started one on both ("existing solver state").  The cold solve
after the change shows that nothing of the solve under r1 is left in A; that the change is not a no-op is asserted too (A's objective
values differ from those under r1).

Problems: pendulum IPDDP / CLDDP / LogDDP / MSIPDDP with the control box, unicycle IPDDP box + ball, the smallest plant of
tests/model_cases.py whose objective is staged through LDS (NX*NX + NU*NU + NX > 40), and a plant with nx = 10 on both stack layouts.
B = 70 is two tiles, the second partial; horizons 8 .. 20; solves capped at 8 iterations (equality, not convergence, is the subject).
Reference changes: the goal alone; goal + per-step reference on a handle created without one; new contents on a handle created with one;
clear_traj back to goal-only."""
import ctypes as C

import numpy as np
import pytest

import model_cases as MC
from test_mpc_advance import RESULT_FIELDS, same

pytestmark = pytest.mark.gpu

B = 70
SEED = 20281900


# ---------------------------------------------------------------------------------------------------------------- problems
def smallest_staged_key(api):
    """the row of model_cases.MODELS with the smallest NX*NX + NU*NU + NX above 40 (Objective::stage instead of the hoisted registers)"""
    best = None
    for key in MC.MODEL_KEYS:
        p = MC.build_row(api, MC.MODELS[MC.KEYS[key]])
        size = p.nx * p.nx + p.nu * p.nu + p.nx
        if size > 40 and (best is None or size < best[0]):
            best = (size, key)
    return best[1]


def _row(key, N):
    def mk(api):
        k = smallest_staged_key(api) if key == "staged" else key
        row = MC.MODELS[MC.KEYS[k]]
        p = row.build(api, N)
        if key == "staged":
            assert MC.staged(p), k
        return p, np.asarray(row.spread, dtype=np.float64)
    return mk


# name -> (builder(api) -> (problem, x0 spread), batch, amplitude of the goal changes per coordinate, environment)
CASES = {
    "pendulum_ipddp_box": (lambda api: (api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=12), np.array([0.2, 0.3])), B, 0.3, {}),
    "pendulum_clddp_box": (lambda api: (api.pendulum_problem(api.SOLVER_CLDDP, True, horizon=12), np.array([0.2, 0.3])), B, 0.3, {}),
    "unicycle_ipddp_box_ball": (lambda api: (api.unicycle_problem(api.SOLVER_IPDDP, horizon=20, obstacle=True), np.array([0.3, 0.3, 0.1])), B, 0.2, {}),
    "pendulum_logddp": (lambda api: (api.pendulum_problem(api.SOLVER_LOGDDP, True, horizon=10), np.array([0.1, 0.1])), B, 0.3, {}),
    "pendulum_msipddp": (lambda api: (api.pendulum_problem(api.SOLVER_MSIPDDP, True, horizon=10), np.array([0.1, 0.1])), B, 0.3, {}),
    "staged_objective": (_row("staged", 8), B, 0.05, {}),
    "quadrotor_rate_nx10": (_row("quadrotor_rate", 10), 64, 0.02, {}),
    "quadrotor_rate_nx10_t4=0": (_row("quadrotor_rate", 10), 64, 0.02, {"CDDP_HIP_T4": "0"}),
}
CHANGES = ["goal", "goal+traj", "traj_contents", "clear_traj"]


def make(api, case, monkeypatch):
    mk, batch, amp, env = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, spread = mk(api)
    assert 8 <= p.N <= 20
    p.options.max_iterations = min(p.options.max_iterations, 8)
    p.options.warm_start = 0
    return p, spread, batch, amp


def goal_of(p, amp, rng):
    return np.ascontiguousarray(np.asarray(p.x_ref_builder) + amp * rng.uniform(-1.0, 1.0, p.nx))


def traj_to(p, g, amp, rng):
    """(N + 1, nx): from the builder's x0 to g with a wiggle; the last row is g itself (the reference's constructor rule, exactly)"""
    s = np.linspace(0.0, 1.0, p.N + 1)[:, None]
    T = (1.0 - s) * p.x0[None, :] + s * g[None, :] + 0.3 * amp * np.sin(7.0 * s + rng.uniform(0.0, 3.0, p.nx)[None, :])
    T[p.N] = g
    return np.ascontiguousarray(T)


def references(p, change, amp, seed):
    """-> r1 = (goal, traj or None) the handle is created with, r2 the reference it is moved to, the set_reference arguments"""
    rng = np.random.default_rng(seed)
    g0 = np.ascontiguousarray(p.x_ref_builder)
    g1, g2 = goal_of(p, amp, rng), goal_of(p, amp, rng)
    T1, T2 = traj_to(p, g1, amp, rng), traj_to(p, g2, amp, rng)
    if change == "goal":
        return (g0, None), (g1, None), dict(x_ref=g1)
    if change == "goal+traj":
        return (g0, None), (g1, T1), dict(x_ref=g1, x_ref_traj=T1)
    if change == "traj_contents":
        return (g1, T1), (g2, T2), dict(x_ref=g2, x_ref_traj=T2)
    return (g1, T1), (g2, None), dict(x_ref=g2, clear_traj=True)


def handle(api, p, ref, batch):
    """a handle of problem p created with the reference `ref` (cddp_hip_create copies what the descriptor points to)"""
    if not hasattr(p, "x_ref_builder"):
        p.x_ref_builder = p.x_ref.copy()
    g, T = ref
    p.x_ref = np.ascontiguousarray(g, dtype=np.float64); p.c.x_ref = api._ptr(p.x_ref)
    if T is None:
        p.c.x_ref_traj = None
    else:
        p.x_ref_traj = np.ascontiguousarray(T, dtype=np.float64); p.c.x_ref_traj = api._ptr(p.x_ref_traj)
    return api.HipBatchSolver(p, batch)


def has_duals(api, p, h):
    return p.c.solver in (api.SOLVER_IPDDP, api.SOLVER_MSIPDDP) and h.m > 0


def assert_same(api, p, a, b, where):
    ra, rb = a.results(), b.results()
    for name in RESULT_FIELDS:
        assert same(ra[name], rb[name]), (where, name)
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    assert np.isfinite(Xa).all() and np.isfinite(Ua).all(), where
    assert same(Xa, Xb) and same(Ua, Ub), where
    if has_duals(api, p, a):
        for da, db, name in zip(a.duals(), b.duals(), "SYG"):
            assert same(da, db), (where, name)


def assert_reference(h, ref, where):
    g, T = h.get_reference()
    assert np.array_equal(g, ref[0]), (where, "goal")
    assert (T is None) == (ref[1] is None), (where, "has_traj")
    if T is not None:
        assert np.array_equal(T, ref[1]), (where, "per-step reference")


def run_change(api, p, spread, batch, amp, change, seed, device=False):
    p.x_ref_builder = p.x_ref.copy()
    r1, r2, kw = references(p, change, amp, seed)
    x0 = api.batch_x0(p, batch, seed, spread); U0 = api.batch_U0(p, batch)
    a = handle(api, p, r1, batch); b = handle(api, p, r2, batch)
    for h in (a, b):
        h.set_initial(x0, U0); h.solve()
    assert_reference(a, r1, "as created"); assert_reference(b, r2, "as created")
    old = a.results()["final_objective"].copy()
    if device:
        import torch
        kw = {k: (torch.from_numpy(v).to("cuda:0") if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    a.set_reference(**kw)
    assert_reference(a, r2, "after set_reference")
    assert same(a.results()["final_objective"], old), "the current iterate's scalars stay those under the old reference until the next solve"
    a.solve(); b.solve()
    assert_same(api, p, a, b, (change, "cold solve after the change"))
    assert not same(a.results()["final_objective"], old), (change, "the solve after the change equals the one before it: the cases show nothing")
    for h in (a, b):
        h.set_warm_start(True)
    a.solve(); b.solve()
    assert_same(api, p, a, b, (change, "warm solve, existing solver state"))
    assert_reference(a, r2, "after the solves")
    a.close(); b.close()


@pytest.mark.parametrize("change", CHANGES)
@pytest.mark.parametrize("case", list(CASES))
def test_set_reference_then_solve_is_create_with_it_then_solve(api, monkeypatch, case, change):
    p, spread, batch, amp = make(api, case, monkeypatch)
    run_change(api, p, spread, batch, amp, change, SEED + 10 * list(CASES).index(case) + CHANGES.index(change))


def test_staged_case_is_the_smallest_staged_plant(api):
    """the table's `staged_objective` row: the objective does not fit the hoisted registers, and no model row with a smaller one is staged"""
    key = smallest_staged_key(api)
    p = MC.build_row(api, MC.MODELS[MC.KEYS[key]])
    assert MC.staged(p)
    for k in MC.MODEL_KEYS:
        q = MC.build_row(api, MC.MODELS[MC.KEYS[k]])
        assert not MC.staged(q) or q.nx * q.nx + q.nu * q.nu + q.nx >= p.nx * p.nx + p.nu * p.nu + p.nx


@pytest.mark.parametrize("change", ["goal+traj", "clear_traj"])
def test_device_tensors(api, monkeypatch, change):
    p, spread, batch, amp = make(api, "unicycle_ipddp_box_ball", monkeypatch)
    run_change(api, p, spread, batch, amp, change, SEED + 500 + CHANGES.index(change), device=True)


def test_two_tile_groups_all_receive_the_reference(api, monkeypatch):
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    p, spread, batch, amp = make(api, "pendulum_ipddp_box", monkeypatch)
    probe = handle(api, p, (p.x_ref.copy(), None), 130)
    assert probe.num_groups() == 2
    probe.close()
    for change in ("goal+traj", "clear_traj"):
        p.options.warm_start = 0
        run_change(api, p, spread, 130, amp, change, SEED + 600 + CHANGES.index(change))


@pytest.mark.parametrize("change", ["goal", "goal+traj", "clear_traj"])
def test_score_rollouts_uses_the_new_reference_at_once(api, monkeypatch, change):
    """no solve between set_reference and the scoring: the objective is evaluated under the new reference on the spot"""
    p, spread, batch, amp = make(api, "unicycle_ipddp_box_ball", monkeypatch)
    p.x_ref_builder = p.x_ref.copy()
    seed = SEED + 700 + CHANGES.index(change)
    r1, r2, kw = references(p, change, amp, seed)
    centre, scale = MC.candidate_scale(api, p)
    x0, U = MC.draw(p, spread, centre, scale, seed, b=batch, s=3)
    a = handle(api, p, r1, batch); b = handle(api, p, r2, batch)
    before = a.score_rollouts(U, x0=x0)
    a.set_reference(**kw)
    sa, sb = a.score_rollouts(U, x0=x0), b.score_rollouts(U, x0=x0)
    assert np.isfinite(sa["cost"]).all()
    assert np.array_equal(sa["cost"], sb["cost"]) and np.array_equal(sa["viol"], sb["viol"])
    assert not np.array_equal(sa["cost"], before["cost"])
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- forward
ALPHAS = 0.5 ** np.arange(8)                                      # (a failed trial reports the current iterate's scalars: some must succeed)


def same_trials(ta, tb):
    return all(same(ta[name], tb[name]) for name in ta.dtype.names)


@pytest.mark.parametrize("carrier", ["numpy", "torch"])
def test_forward_after_set_reference_is_forward_on_a_handle_created_with_it(api, monkeypatch, carrier):
    """cddp_hip_forward installs the caller's step sizes by uploading the problem block whole, before and after its launches: the goal in
    that block must be the one the device holds (a device-pointer setter writes it on the device only), during the call and after it."""
    p, spread, batch, amp = make(api, "unicycle_ipddp_box_ball", monkeypatch)
    p.x_ref_builder = p.x_ref.copy()
    seed = SEED + 900
    r1, r2, kw = references(p, "goal+traj", amp, seed)
    x0 = api.batch_x0(p, batch, seed, spread); U0 = api.batch_U0(p, batch)
    if carrier == "torch":
        import torch
        kw = {k: torch.from_numpy(v).to("cuda:0") for k, v in kw.items()}
    a = handle(api, p, r1, batch); b = handle(api, p, r2, batch)
    a.set_initial(x0, U0); b.set_initial(x0, U0)
    a.set_reference(**kw)
    for h in (a, b):
        h.solve(); h.backward()
    ta, tb = a.forward(ALPHAS), b.forward(ALPHAS)
    assert np.isfinite(ta["cost"]).all() and same_trials(ta, tb)
    assert tb["success"].any(), "no trial succeeded: every record repeats the current iterate"
    assert_reference(a, r2, "after forward")
    assert same_trials(a.forward(ALPHAS), tb), "a second forward: the first one left the goal in the problem block"
    a.solve(); b.solve()
    assert_same(api, p, a, b, "solve after forward")
    assert_reference(a, r2, "after forward and solve")
    # at once: after a sweep under r1 the trials are evaluated under the reference set since, whichever way it was carried
    c = handle(api, p, r1, batch); d = handle(api, p, r1, batch)
    for h in (c, d):
        h.set_initial(x0, U0); h.solve(); h.backward()
    before = c.forward(ALPHAS)
    c.set_reference(**kw); d.set_reference(x_ref=r2[0], x_ref_traj=r2[1])
    tc, td = c.forward(ALPHAS), d.forward(ALPHAS)
    assert same_trials(tc, td)
    ok = (tc["success"] == 1) & (before["success"] == 1)
    assert ok.any() and (tc["cost"][ok] != before["cost"][ok]).all(), "successful trials are costed under the new reference"
    assert_reference(c, r2, "after forward"); assert_reference(d, r2, "after forward")
    for h in (a, b, c, d):
        h.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def hip_runtime():
    """the HIP runtime this process already runs on (the one torch loaded and the library is bound to), for a plain hipMalloc / hipFree"""
    with open("/proc/self/maps") as fh:
        paths = sorted({line.split()[-1] for line in fh if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    lib = C.CDLL(paths[0])
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; lib.hipMalloc.restype = C.c_int
    lib.hipFree.argtypes = [C.c_void_p]; lib.hipFree.restype = C.c_int
    return lib


def test_refusals_change_nothing(api, monkeypatch):
    import torch
    lib = api.load_hip()
    p, spread, batch, amp = make(api, "pendulum_ipddp_box", monkeypatch)
    p.x_ref_builder = p.x_ref.copy()
    rng = np.random.default_rng(SEED + 800)
    g1 = goal_of(p, amp, rng); T1 = traj_to(p, g1, amp, rng)
    g2 = goal_of(p, amp, rng); T2 = traj_to(p, g2, amp, rng)
    h = handle(api, p, (g1, T1), batch)          # with a per-step reference
    plain = handle(api, p, (g1, None), batch)    # without one
    nx, N = p.nx, p.N

    def refused(rc, code, *parts):
        msg = lib.cddp_hip_last_error().decode()
        assert rc == code, (rc, msg)
        for s in parts:
            assert s in msg, (s, msg)
        assert_reference(h, (g1, T1), msg); assert_reference(plain, (g1, None), msg)
        assert h.mpc_reference_cursor() == -1 and plain.mpc_reference_cursor() == -1

    sr = lambda hh, flags, x, T: lib.cddp_hip_set_reference(hh.h if hh is not None else None, flags, x.ctypes.data if isinstance(x, np.ndarray) else x,
                                                            T.ctypes.data if isinstance(T, np.ndarray) else T)
    refused(sr(None, 0, g2, None), -1, "cddp_hip_set_reference: null handle")
    refused(sr(h, 4, g2, None), -2, "unknown flag bits 0x4")
    refused(sr(h, api.REF_CLEAR_TRAJ, g2, T2), -2, "CDDP_HIP_REF_CLEAR_TRAJ", "x_ref_traj must be NULL")
    refused(sr(h, 0, None, None), -2, "nothing to change")
    refused(sr(h, api.REF_DEVICE, None, None), -2, "nothing to change")
    # device pointers: a host address; an allocation one element short of the array (hipMalloc itself: torch's allocator hands out parts
    # of larger blocks, so the end of a tensor is not the end of its allocation)
    refused(sr(h, api.REF_DEVICE, g2, None), -2, "x_ref is not device memory")
    gd = torch.from_numpy(g2).to("cuda:0")
    refused(sr(h, api.REF_DEVICE, gd.data_ptr(), T2), -2, "x_ref_traj is not device memory")
    hip = hip_runtime()
    short = [C.c_void_p(), C.c_void_p()]
    assert hip.hipMalloc(C.byref(short[0]), C.c_size_t(8 * nx - 8)) == 0 and hip.hipMalloc(C.byref(short[1]), C.c_size_t(8 * nx * (N + 1) - 8)) == 0
    try:
        refused(sr(h, api.REF_DEVICE, short[0].value, None), -2, "x_ref needs %d bytes, its allocation ends after %d" % (8 * nx, 8 * nx - 8))
        refused(sr(h, api.REF_DEVICE, None, short[1].value), -2,
                "x_ref_traj needs %d bytes, its allocation ends after %d" % (8 * nx * (N + 1), 8 * nx * (N + 1) - 8))
        refused(sr(h, api.REF_DEVICE, gd.data_ptr(), short[1].value), -2, "x_ref_traj needs")
    finally:
        for q in short:
            hip.hipFree(q)
    # host values: non-finite; the last row of the per-step reference against the goal, on the state the call would leave behind
    bad = g2.copy(); bad[nx - 1] = np.inf
    refused(sr(plain, 0, bad, None), -2, "x_ref holds a non-finite value")
    badT = T2.copy(); badT[3, 0] = np.nan
    refused(sr(h, 0, g2, badT), -2, "x_ref_traj holds a non-finite value")
    refused(sr(h, 0, g2, None), -2, "Last reference state must be same as the reference state")          # new goal, the handle's rows
    refused(sr(h, 0, None, T2), -2, "Last reference state must be same as the reference state")          # new rows, the handle's goal
    refused(sr(plain, 0, None, T2), -2, "Last reference state must be same as the reference state")      # first rows, the handle's goal
    off = T2.copy(); off[N, 0] += 2e-6
    refused(sr(h, 0, g2, off), -2, "Last reference state must be same as the reference state")
    near = T2.copy(); near[N, 0] += 5e-7                                                                  # within 1e-6: accepted, as the reference accepts it
    assert sr(h, 0, g2, near) == 0
    assert_reference(h, (g2, near), "within the rule")
    assert sr(h, 0, g1, T1) == 0
    # the path descriptor
    path = np.ascontiguousarray(T2[:5])

    def desc(**kw):
        d = api.RefPathDesc()
        d.abi_version = api.ABI_VERSION; d.flags = 0; d.rows = path.shape[0]; d.start = 0; d.rows_per_step = 1.0; d.path = path.ctypes.data
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bind = lambda hh, d: lib.cddp_hip_mpc_set_reference_path(hh.h if hh is not None else None, C.byref(d) if d is not None else None)
    refused(bind(None, desc()), -1, "cddp_hip_mpc_set_reference_path: null handle")
    refused(bind(h, desc(abi_version=api.ABI_VERSION + 1)), -2, "ABI version mismatch")
    refused(bind(h, desc(flags=2)), -2, "unknown flag bits 0x2")
    refused(bind(h, desc(rows=0)), -2, "at least one row")
    refused(bind(h, desc(start=-1)), -2, "start = -1")
    for r in (0.0, -1.0, float("inf"), float("nan")):
        refused(bind(h, desc(rows_per_step=r)), -2, "rows_per_step must be finite and positive")
    refused(bind(h, desc(path=None)), -1, "null path")
    bad_path = path.copy(); bad_path[2, 1] = np.nan
    refused(bind(h, desc(path=bad_path.ctypes.data)), -2, "the path holds a non-finite value")
    refused(bind(h, desc(flags=api.REF_DEVICE)), -2, "the path is not device memory")
    refused(bind(h, desc(flags=api.REF_DEVICE, path=gd.data_ptr(), rows=1 << 30)), -2, "the path needs", "its allocation ends after")
    c = C.c_int64(5)
    assert lib.cddp_hip_mpc_reference_cursor(h.h, None) == -1
    # while a path is bound the setter is refused; the reference is the path's window, and stays it
    assert bind(h, desc()) == 0
    import ref_window_ref as RW
    w = RW.window(path, 0, N)
    for args in ((0, g2, None), (0, g2, T2), (api.REF_CLEAR_TRAJ, None, None)):
        assert sr(h, *args) == -1 and "a reference path is bound" in lib.cddp_hip_last_error().decode()
        assert_reference(h, (w[N], w), "bound")
    assert lib.cddp_hip_mpc_reference_cursor(h.h, C.byref(c)) == 0 and c.value == 0
    assert bind(h, None) == 0
    assert_reference(h, (w[N], w), "unbound: the reference is left as it stands")
    assert sr(h, 0, g1, T1) == 0
    assert_reference(h, (g1, T1), "after unbinding the setter is accepted again")
    h.close(); plain.close()
