"""A reference path bound to a live handle (cddp_hip_mpc_set_reference_path): every cddp_hip_mpc_advance -- cddp_hip_mpc_run and
cddp_hip_mpc_run_plant included -- moves the cursor by one and installs the next window on the device (inst_ref.hip).

1. Windows: for cursors 0 .. steps, get_reference() equals the numpy restatement of the window (tests/ref_window_ref.py, held to
   csrc/ref_window.hpp by tests/test_ref_window_host.py), bit for bit, for rows_per_step 1.0, 2.0, 0.5 and 0.3, on paths that run out before
   the last window (L = steps + 3 < steps + N: the hold-last-row branch) and on a path of one row; the three advance modes take turns.
2. mpc_run with a bound path equals the hand-written loop {solve; get_plan_head; mpc_advance; set_reference(window k + 1 of the numpy
   restatement)} on a second handle, in each of the three modes and with SHIFT_DUALS: U_applied, X_visited, iterations, status, final plan.
3. The same for mpc_run_plant, against a mismatched plant (RK4, two substeps) with disturbances.
4. The cursor reads back start + steps; after unbinding an advance leaves the reference as it stands.
5. A target that moves by a known offset per step, LTI plant, CLDDP without constraints: the visited states are closer to the current
   window's row 0 than those of the same loop on a handle that keeps what it was created with: the window of cursor 0 replayed at every
   step, and the fixed goal alone.
6. cddp_hip_forward with a path bound: its trials, the reference afterwards and the next solve equal the hand-written loop's.

B = 70 (two tiles, the second partial), N = 12, steps = 5.  Every comparison of 1 - 4 is np.array_equal."""
import numpy as np
import pytest

import ref_window_ref as RW
import test_plant_device as PD
from test_mpc_advance import same

pytestmark = pytest.mark.gpu

B, N, STEPS = 70, 12, 5
SEED = 20281950
RATES = [1.0, 2.0, 0.5, 0.3]

CASES = {
    "pendulum_ipddp_box": (lambda api: api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=N), np.array([0.2, 0.3]), 0.5),
    "unicycle_ipddp_box_ball": (lambda api: api.unicycle_problem(api.SOLVER_IPDDP, horizon=N, obstacle=True), np.array([0.3, 0.3, 0.1]), 1.0),
}
MODES = {"keep": ("MPC_KEEP_PLAN", False), "existing": ("MPC_SHIFT_EXISTING", False), "existing+duals": ("MPC_SHIFT_EXISTING", True),
         "provided": ("MPC_SHIFT_PROVIDED", False)}


def make(api, case):
    mk, spread, rps = CASES[case]
    p = mk(api)
    p.options.max_iterations = min(p.options.max_iterations, 6)
    p.options.warm_start = 1
    return p, spread, rps


def path_for(p, L, seed):
    """L rows from the builder's x0 towards its goal, with a wiggle: no two rows alike, none on a grid"""
    rng = np.random.default_rng(seed)
    if L == 1:
        return np.ascontiguousarray((p.x_ref + 0.1 * rng.uniform(-1.0, 1.0, p.nx))[None, :])
    s = np.linspace(0.0, 1.0, L)[:, None]
    return np.ascontiguousarray((1.0 - s) * p.x0[None, :] + s * p.x_ref[None, :] + 0.05 * np.sin(5.0 * s + rng.uniform(0.0, 3.0, p.nx)[None, :]))


def assert_window(h, path, k, rps, where):
    g, T = h.get_reference()
    w = RW.window(path, k, h.p.N, rps)
    assert T is not None and np.array_equal(T, w), (where, k, "window")
    assert np.array_equal(g, w[h.p.N]), (where, k, "goal = row N of the window")
    assert h.mpc_reference_cursor() == k, (where, k)


class Following:
    """a handle whose mpc_advance is followed by set_reference(window k + 1 of the numpy restatement): the loop a caller writes by hand"""

    def __init__(self, h, path, rps, start=0):
        self.h, self.path, self.rps, self.k = h, path, rps, start
        self.install()

    def install(self):
        w = RW.window(self.path, self.k, self.h.p.N, self.rps)
        self.h.set_reference(x_ref=w[self.h.p.N], x_ref_traj=w)

    def __getattr__(self, name):
        return getattr(self.h, name)

    def mpc_advance(self, *args, **kw):
        self.h.mpc_advance(*args, **kw)
        self.k += 1
        self.install()


# ---------------------------------------------------------------------------------------------------------------- 1, 4
@pytest.mark.parametrize("L", [STEPS + 3, 1])
@pytest.mark.parametrize("rps", RATES)
def test_windows_are_the_numpy_restatement(api, rps, L):
    p, spread, _ = make(api, "pendulum_ipddp_box")
    assert L < STEPS + N
    path = path_for(p, L, SEED + L)
    h = api.HipBatchSolver(p, B)
    h.set_initial(api.batch_x0(p, B, SEED, spread), api.batch_U0(p, B))
    h.initialize()
    assert h.mpc_reference_cursor() == -1 and h.get_reference()[1] is None
    h.mpc_set_reference_path(path, rows_per_step=rps)
    assert_window(h, path, 0, rps, "bound")
    modes = (api.MPC_KEEP_PLAN, api.MPC_SHIFT_EXISTING, api.MPC_SHIFT_PROVIDED)
    for k in range(1, STEPS + 1):
        h.mpc_advance(modes[k % 3])
        assert_window(h, path, k, rps, "advanced")
    held = RW.window(path, STEPS, N, rps)
    if rps >= 1.0 or L == 1:
        assert np.array_equal(held[N], path[L - 1])               # the path has run out within the last window
    # a cursor that starts inside the path; binding again replaces path and cursor
    h.mpc_set_reference_path(path, start=2, rows_per_step=rps)
    assert_window(h, path, 2, rps, "bound again")
    # unbinding: the cursor is gone, the reference stays, and an advance leaves it alone
    before = h.get_reference()
    h.mpc_set_reference_path(None)
    assert h.mpc_reference_cursor() == -1
    h.mpc_advance(api.MPC_SHIFT_EXISTING)
    after = h.get_reference()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    h.close()


def test_path_from_a_device_tensor(api):
    import torch
    p, spread, _ = make(api, "pendulum_ipddp_box")
    path = path_for(p, STEPS + 3, SEED + 20)
    h = api.HipBatchSolver(p, B)
    h.set_initial(api.batch_x0(p, B, SEED, spread), api.batch_U0(p, B))
    h.initialize()
    t = torch.from_numpy(path).to("cuda:0")
    h.mpc_set_reference_path(t, start=1, rows_per_step=0.3)
    del t                                                          # the rows were copied
    assert_window(h, path, 1, 0.3, "device path")
    h.mpc_advance(api.MPC_KEEP_PLAN)
    assert_window(h, path, 2, 0.3, "device path")
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def hand_loop(api, f, steps, mode, shift_duals):
    h = f.h
    U = np.zeros((h.B, steps, h.p.nu)); X = np.zeros((h.B, steps + 1, h.p.nx))
    it = np.zeros((h.B, steps), dtype=np.int32); st = np.zeros((h.B, steps), dtype=np.int32)
    for k in range(steps):
        h.solve()
        u0, x1 = h.plan_head(); r = h.results()
        U[:, k] = u0; X[:, k + 1] = x1; it[:, k] = r["iterations"]; st[:, k] = r["status"]
        f.mpc_advance(mode, shift_duals=shift_duals)
    return U, X, it, st


def assert_same_run(r, U, X, it, st, a, b, where):
    assert np.isfinite(U).all() and np.isfinite(X).all(), where
    assert same(r["U_applied"], U), (where, int(np.sum(r["U_applied"] != U)))
    assert same(r["X_visited"], X), (where, int(np.sum(r["X_visited"] != X)))
    assert same(r["iterations"], it) and same(r["status"], st), where
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    assert same(Xa, Xb) and same(Ua, Ub), (where, "final plan")
    ga, Ta = a.get_reference(); gb, Tb = b.get_reference()
    assert np.array_equal(ga, gb) and np.array_equal(Ta, Tb), (where, "final reference")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_mpc_run_follows_the_path_like_the_hand_written_loop(api, case, mode):
    p, spread, rps = make(api, case)
    flag, sd = MODES[mode]
    path = path_for(p, STEPS + 3, SEED + 30)
    x0 = api.batch_x0(p, B, SEED + 31, spread); U0 = api.batch_U0(p, B)
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0)
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0)
    U, X, it, st = hand_loop(api, Following(a, path, rps), STEPS, getattr(api, flag), sd)
    X[:, 0] = x0
    b.mpc_set_reference_path(path, rows_per_step=rps)
    r = b.mpc_run(STEPS, getattr(api, flag), shift_duals=sd)
    assert_same_run(r, U, X, it, st, a, b, (case, mode))
    assert b.mpc_reference_cursor() == STEPS
    assert_window(b, path, STEPS, rps, (case, mode))
    # the path matters: a run on the problem's fixed goal visits other states
    c = api.HipBatchSolver(p, B); c.set_initial(x0, U0)
    rc = c.mpc_run(STEPS, getattr(api, flag), shift_duals=sd)
    assert not same(rc["X_visited"], r["X_visited"])
    a.close(); b.close(); c.close()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("case,mode", [("pendulum_ipddp_box", "provided"), ("unicycle_ipddp_box_ball", "existing+duals"), ("unicycle_ipddp_box_ball", "keep")])
def test_mpc_run_plant_follows_the_path_like_the_hand_written_loop(api, case, mode):
    p, spread, rps = make(api, case)
    flag, sd = MODES[mode]
    path = path_for(p, STEPS + 3, SEED + 40)
    x0 = api.batch_x0(p, B, SEED + 41, spread); U0 = api.batch_U0(p, B)
    W = np.ascontiguousarray(1e-3 * np.random.default_rng(SEED + 42).standard_normal((B, STEPS, p.nx)))
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0)
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0)
    assert int(p.c.integrator) != api.RK4
    pa, pb = (api.DevicePlant.of_problem(p, B, integrator=api.RK4, substeps=2) for _ in range(2))
    U, X, it, st, _, model_x1, _ = PD.plant_loop(api, Following(a, path, rps, start=1), pa, STEPS, getattr(api, flag), sd, W)
    X[:, 0] = x0
    b.mpc_set_reference_path(path, start=1, rows_per_step=rps)
    r = b.mpc_run_plant(pb, STEPS, getattr(api, flag), shift_duals=sd, W=W)
    assert_same_run(r, U, X, it, st, a, b, (case, mode))
    assert np.all(np.any(r["X_visited"][:, 1] != model_x1[0], axis=1)), "the plant is the model on some trajectory"
    assert b.mpc_reference_cursor() == 1 + STEPS
    assert_window(b, path, 1 + STEPS, rps, (case, mode))
    a.close(); b.close(); pa.close(); pb.close()


# ---------------------------------------------------------------------------------------------------------------- forward
def test_forward_with_a_bound_path_reads_the_window_and_leaves_it(api):
    """after a bound-path advance the goal is newer on the device than in the host's problem block, which cddp_hip_forward uploads whole:
    its trials, the reference afterwards and the next solve equal those of the hand-written loop"""
    p, spread, rps = make(api, "unicycle_ipddp_box_ball")
    path = path_for(p, STEPS + 3, SEED + 60)
    x0 = api.batch_x0(p, B, SEED + 61, spread); U0 = api.batch_U0(p, B)
    alphas = 0.5 ** np.arange(8)
    a = api.HipBatchSolver(p, B); a.set_initial(x0, U0)
    b = api.HipBatchSolver(p, B); b.set_initial(x0, U0)
    f = Following(a, path, rps)
    b.mpc_set_reference_path(path, rows_per_step=rps)
    for k in range(2):
        a.solve(); b.solve()
        f.mpc_advance(api.MPC_KEEP_PLAN); b.mpc_advance(api.MPC_KEEP_PLAN)
        a.backward(); b.backward()
        ta, tb = a.forward(alphas), b.forward(alphas)
        assert np.isfinite(tb["cost"]).all() and tb["success"].any()
        for name in ta.dtype.names:
            assert same(ta[name], tb[name]), (k, name)
        assert_window(b, path, k + 1, rps, "after forward")
    a.solve(); b.solve()
    Xa, Ua = a.trajectory(); Xb, Ub = b.trajectory()
    assert same(Xa, Xb) and same(Ua, Ub) and same(a.results()["final_objective"], b.results()["final_objective"])
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_visited_states_follow_a_moving_target(api):
    """The plant is the scalar integrator x' = x + u (LTI 1 x 1): its state is a position alone, so a target that moves by a fixed offset per
    step is a path the plant can follow (a state with a velocity coordinate would need the path to carry the matching velocity).  State
    cost on every step, CLDDP, no constraint of any kind."""
    from test_plan_sens import lti_seed
    steps = 8
    offset = 0.125                                                 # (a power of two: row k is 1 + k * offset without rounding)
    path = np.ascontiguousarray((1.0 + offset * np.arange(steps + N + 1))[:, None])
    assert np.array_equal(path[1:] - path[:-1], np.full((len(path) - 1, 1), offset))                    # a known offset per step, exactly
    w0 = RW.window(path, 0, N)

    def problem(x_ref, x_ref_traj=None):
        o = api.default_options(); o.max_iterations = 5; o.warm_start = 1
        p = api.Problem(api.SOLVER_CLDDP, api.MODEL_LTI, api.EULER, 1, 1, N, 1.0, np.eye(1), 1e-2 * np.eye(1), np.eye(1), x_ref,
                        lti_A=np.eye(1), lti_B=np.eye(1), x_ref_traj=x_ref_traj, options=o)
        p.x0 = path[0].copy()
        return p

    p = problem(w0[N])
    assert not p._cons and not p._terms                            # no bounds at all: none can be active
    x0 = api.batch_x0(p, B, SEED + 50, np.array([0.05]))
    U0, X0 = lti_seed(p, x0)
    runs = {}
    # what a handle could do before: "fixed" replays the reference it was created with (the window of cursor 0) at every step, "fixed_goal"
    # has the goal alone (that window's last row), fixed
    for name, q in (("moving", p), ("fixed", problem(w0[N], w0)), ("fixed_goal", problem(w0[N]))):
        h = api.HipBatchSolver(q, B); h.set_initial(x0, U0, X0)
        if name == "moving":
            h.mpc_set_reference_path(path)
        runs[name] = h.mpc_run(steps, api.MPC_SHIFT_EXISTING)["X_visited"]
        h.close()
    # X_visited[:, k] is the state solve k starts from; the window of cursor k has path row k as its row 0
    dist = {name: np.linalg.norm(X[:, 1:] - path[None, 1:steps + 1], axis=2) for name, X in runs.items()}
    print("mean distance to the current target: " + ", ".join("%s %.4f" % (n, d.mean()) for n, d in dist.items()))
    for d in dist.values():
        assert np.isfinite(d).all()
    assert np.array_equal(runs["moving"][:, :2], runs["fixed"][:, :2])                                   # the first solve reads the same window
    for base in ("fixed", "fixed_goal"):
        assert (dist["moving"].sum(axis=1) < dist[base].sum(axis=1)).all(), base
        assert (dist["moving"][:, -1] < dist[base][:, -1]).all(), base
