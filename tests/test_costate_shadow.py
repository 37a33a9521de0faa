"""Shadow costate: on the layouts of the role-split IPDDP sweep the costate trial (K4b) leaves the iteration's chain -- k_update accepts
the first trial flagged 1 at once and records it, extra workgroups of the NEXT sweep launch evaluate the rows from the previous sweep's
value stack (the sweeps alternate between two stacks), a flush launch evaluates what is pending at the end, and a non-finite row makes
the host discard the solve and run it again with K4b on the chain (capi.hip::SolveRun, kernels_lean.hpp "K4b, deferred").  The rows are
the same expressions in the same order (kernels.hpp::costate_row_eval), so everything a caller can read must be the SAME BITS as with
CDDP_HIP_COSTATE=sync: result records, trajectories, slack / dual / constraint rows, gains, value function, costates, work counters."""
import numpy as np
import pytest

from test_gpu_parity import make, spread_for

pytestmark = pytest.mark.gpu

COUNTERS = ("sweeps", "rollouts", "rollout_steps", "traj_iterations", "outer_iterations", "n_converged")


def _snapshot(hs, st):
    r = hs.results(); X, U = hs.trajectory(); S, Y, G = hs.duals(); K, k = hs.gains(); Vx, Vxx = hs.value(); L = hs.costates()
    out = [r[name] for name in r.dtype.names] + [X, U, S, Y, G, K, k, Vx, Vxx, L]
    out += [np.int64(getattr(st, c)) for c in COUNTERS]
    return out


def _same(ref, got, tag):
    assert len(ref) == len(got)
    for i, (a, g) in enumerate(zip(ref, got)):
        assert np.array_equal(a, g, equal_nan=True), (tag, i)


def _solve(api, p, B, x0, U0, n_solves=1):
    hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0)
    mode0 = hs.costate_mode()
    snaps = []
    for _ in range(n_solves):
        st = hs.solve()
        snaps.append(_snapshot(hs, st))
    mode = hs.costate_mode(); redos = hs.costate_redos(); groups = hs.num_groups()
    hs.close()
    return snaps, (mode0, mode, redos, groups)


def _ab(api, monkeypatch, p, B, x0, U0, tag, n_solves=1, want_redos=0):
    monkeypatch.setenv("CDDP_HIP_COSTATE", "sync")
    ref, info_s = _solve(api, p, B, x0, U0, n_solves)
    assert info_s[0] == 0 and info_s[1] == 0 and info_s[2] == 0, (tag, info_s)
    monkeypatch.setenv("CDDP_HIP_COSTATE", "shadow")
    got, info = _solve(api, p, B, x0, U0, n_solves)
    assert info[0] == 1, (tag, "not eligible", info)
    if want_redos == 0:
        assert info[1] == 1 and info[2] == 0, (tag, info)
    else:
        assert info[1] == 0 and info[2] == want_redos * info[3], (tag, info)   # every group met the hook once and was run again
    for k, (a, g) in enumerate(zip(ref, got)):
        _same(a, g, (tag, k))
    return ref, info


def _dubins(api):
    return api.dubins_problem()


def _problem(api, case):
    return _dubins(api) if case == "dubins_ipddp_box" else make(api, case)


def _spread(p):
    return spread_for(p)   # (nx = 3, the Dubins car included: 0.05 per state)


CASES = ["cartpole_ipddp_box", "unicycle_ipddp_box_ball", "pendulum_ipddp_box", "dubins_ipddp_box"]


@pytest.mark.parametrize("stages", ["1", "2"])
@pytest.mark.parametrize("case", CASES)
def test_shadow_equals_sync_bitwise(api, case, stages, monkeypatch):
    """Both ladder shapes, a batch that is not a multiple of 64 (idle lanes in the extra blocks, a partial sweep workgroup), two solves
    in a row on one handle (the stamps and the value-stack parity carry over)."""
    monkeypatch.setenv("CDDP_HIP_LS_STAGES", stages)
    p = _problem(api, case)
    B = 64 + 16 + 3
    x0 = api.batch_x0(p, B, 20261201, _spread(p))
    U0 = api.batch_U0(p, B)
    _ab(api, monkeypatch, p, B, x0, U0, (case, stages), n_solves=2)


@pytest.mark.parametrize("case", ["cartpole_ipddp_box", "pendulum_ipddp_box"])
def test_shadow_with_trajectories_that_finish_at_different_iterations(api, case, monkeypatch):
    """Trajectories that converge mid-solve (their last sweep wrote one value stack) next to ones that run into max_iterations (the other
    stack, or the same): the value getter and the costates must not depend on which."""
    p = _problem(api, case)
    B = 150
    x0 = api.batch_x0(p, B, 20261202, [3.0 * v for v in _spread(p)])
    U0 = api.batch_U0(p, B)
    monkeypatch.setenv("CDDP_HIP_COSTATE", "sync")
    hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0); hs.solve(); it = np.sort(hs.results()["iterations"]); hs.close()
    assert it[0] < it[-1], "the batch does not spread over iteration counts"
    for cap in sorted({int(it[len(it) // 2]), int(it[0]) + 1}):
        p.options.max_iterations = cap
        ref, _ = _ab(api, monkeypatch, p, B, x0, U0, (case, cap))
        status = ref[0][[n for n in api.RESULT_DTYPE.names].index("status")]
        assert np.any(status == api.STATUS_MAX_ITERATIONS) and np.any(status != api.STATUS_MAX_ITERATIONS), (case, cap)


@pytest.mark.parametrize("case", CASES)
def test_shadow_single_iteration(api, case, monkeypatch):
    """max_iterations = 1: no sweep launch follows the only accept -- every costate row comes from the flush."""
    p = _problem(api, case)
    p.options.max_iterations = 1
    B = 70
    x0 = api.batch_x0(p, B, 20261203, _spread(p))
    _ab(api, monkeypatch, p, B, x0, api.batch_U0(p, B), case)


def test_shadow_full_batch_two_masked_groups(api, monkeypatch):
    """The benchmark shape: 4096 cart-pole trajectories as two tile groups on CU-masked streams, one sweep workgroup per CU."""
    p = api.cartpole_problem(api.SOLVER_IPDDP, True)
    B = 4096
    x0 = api.batch_x0(p, B, 20260928, [0.1, 0.3, 0.1, 0.1])
    _, info = _ab(api, monkeypatch, p, B, x0, None, "c2")
    assert info[3] == 2


def test_shadow_chunked_batch(api, monkeypatch):
    """A batch above 8192 is solved chunk after chunk (each chunk as two groups)."""
    p = api.pendulum_problem(api.SOLVER_IPDDP, True)
    p.options.max_iterations = 12
    B = 8192 + 200
    x0 = api.batch_x0(p, B, 20261204, _spread(p))
    _, info = _ab(api, monkeypatch, p, B, x0, api.batch_U0(p, B), "chunked")
    assert info[3] > 2


@pytest.mark.parametrize("case", ["cartpole_ipddp_box", "unicycle_ipddp_box_ball"])
def test_shadow_mpc_sequence_and_provided_trajectory(api, case, monkeypatch):
    """A cold solve, MPC re-solves from the existing solver state (these keep K4b on the chain: the solve would not be restartable), then a
    "provided trajectory" warm start after forget_solver_state (deferred again) -- the same bits as the all-sync handle at every round."""
    p = _problem(api, case)
    B = 40
    x0 = api.batch_x0(p, B, 20261205, _spread(p))
    U0 = api.batch_U0(p, B)
    rounds = {}
    for mode in ("sync", "shadow"):
        monkeypatch.setenv("CDDP_HIP_COSTATE", mode)
        p.options.warm_start = 0
        hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0)
        out = [_snapshot(hs, hs.solve())]
        modes = [hs.costate_mode()]
        hs.set_warm_start(True)
        for _ in range(3):
            u0h, x1h = hs.plan_head()
            hs.set_initial_state(x1h)
            out.append(_snapshot(hs, hs.solve())); modes.append(hs.costate_mode())
        X, U = hs.trajectory()
        Xs = np.ascontiguousarray(np.concatenate([X[:, 1:], X[:, -1:]], axis=1)); Us = np.ascontiguousarray(np.concatenate([U[:, 1:], U[:, -1:]], axis=1))
        hs.forget_solver_state(); hs.set_initial(np.ascontiguousarray(Xs[:, 0]), Us, Xs)
        out.append(_snapshot(hs, hs.solve())); modes.append(hs.costate_mode())
        assert hs.costate_redos() == 0
        hs.close()
        rounds[mode] = (out, modes)
    p.options.warm_start = 0
    assert rounds["sync"][1] == [0, 0, 0, 0, 0]
    assert rounds["shadow"][1] == [1, 0, 0, 0, 1]
    for k, (a, g) in enumerate(zip(rounds["sync"][0], rounds["shadow"][0])):
        _same(a, g, (case, k))


@pytest.mark.parametrize("fail_at", [1, 3])
@pytest.mark.parametrize("case", ["cartpole_ipddp_box", "unicycle_ipddp_box_ball"])
def test_non_finite_deferred_costate_redoes_the_solve(api, case, fail_at, monkeypatch):
    """Software hook CDDP_HIP_TEST_FAIL_SHADOW=<outer iteration>: the deferred evaluation of that iteration's accepts reports "not finite".
    The solve is discarded and run again with K4b on the chain: one redo, the bits of the sync handle."""
    p = _problem(api, case)
    B = 83
    x0 = api.batch_x0(p, B, 20261206, _spread(p))
    monkeypatch.setenv("CDDP_HIP_TEST_FAIL_SHADOW", str(fail_at))
    _ab(api, monkeypatch, p, B, x0, api.batch_U0(p, B), (case, fail_at), want_redos=1)


def test_two_masked_groups_redo_independently(api, monkeypatch):
    p = api.cartpole_problem(api.SOLVER_IPDDP, True)
    p.options.max_iterations = 6
    B = 2048
    x0 = api.batch_x0(p, B, 20261207, [0.1, 0.3, 0.1, 0.1])
    monkeypatch.setenv("CDDP_HIP_TEST_FAIL_SHADOW", "2")
    _, info = _ab(api, monkeypatch, p, B, x0, None, "c2-redo", want_redos=1)
    assert info[3] == 2


@pytest.mark.parametrize("env", [{"CDDP_HIP_TEST_FAIL_COSTATE": "1"}, {"CDDP_HIP_GRAPH": "1"}, {"CDDP_HIP_SWEEP": "lane"}, {"CDDP_HIP_SWEEP_ROLES": "0"}])
def test_switches_that_resolve_to_sync(api, env, monkeypatch):
    monkeypatch.setenv("CDDP_HIP_COSTATE", "shadow")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = make(api, "cartpole_ipddp_box")
    B = 16
    hs = api.HipBatchSolver(p, B); hs.set_initial(api.batch_x0(p, B, 20261208, spread_for(p)), api.batch_U0(p, B))
    assert hs.costate_mode() == 0
    hs.solve()
    assert hs.costate_mode() == 0 and hs.costate_redos() == 0
    hs.close()


def test_layouts_that_keep_the_chain(api, monkeypatch):
    """Best-merit rule, full DDP, a terminal set (with and without path rows), an unconstrained problem, a state of more than eight entries
    and the other solvers (CLDDP, LogDDP, MSIPDDP) are not eligible, whatever the switch says."""
    monkeypatch.setenv("CDDP_HIP_COSTATE", "shadow")
    probs = []
    q = make(api, "cartpole_ipddp_box"); q.options.enable_parallel = 1; probs.append(q)
    q = make(api, "cartpole_ipddp_box"); q.options.use_ilqr = 0; probs.append(q)
    probs.append(make(api, "cartpole_ipddp_unc"))
    probs.append(make(api, "cartpole_clddp_box"))
    probs.append(make(api, "path_term_eq"))
    probs.append(make(api, "term_eq_only"))
    probs.append(make(api, "quadrotor_ipddp_box"))
    probs.append(api.cartpole_problem(api.SOLVER_LOGDDP, True))
    probs.append(api.pendulum_problem(api.SOLVER_MSIPDDP, True))
    for q in probs:
        hs = api.HipBatchSolver(q, 8); hs.set_initial(api.batch_x0(q, 8, 20261209, spread_for(q)), api.batch_U0(q, 8))
        assert hs.costate_mode() == 0
        hs.solve()
        assert hs.costate_mode() == 0 and hs.costate_redos() == 0
        hs.close()


def test_default_defers_only_where_the_sweep_leaves_room(api, monkeypatch):
    """CDDP_HIP_COSTATE unset: deferred when the sweep launch has at most one workgroup per CU of the group's share of the chip (16
    trajectories per workgroup: 4096 cart-poles as two groups of 128 workgroups on 128 CUs each), on the chain when it has more (8192)."""
    monkeypatch.delenv("CDDP_HIP_COSTATE", raising=False)
    p = api.cartpole_problem(api.SOLVER_IPDDP, True)
    for B, want in ((83, 1), (4096, 1), (8192, 0)):
        hs = api.HipBatchSolver(p, B); hs.set_initial(api.batch_x0(p, B, 20261210, [0.1, 0.3, 0.1, 0.1]))
        assert hs.costate_mode() == want, (B, hs.costate_mode(), hs.num_groups())
        hs.close()
