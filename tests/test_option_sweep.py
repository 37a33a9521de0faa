"""Every solver option away from its default, on the device, against the oracle.

cddp_hip_options carries about fifty numbers and every solver family reads them in code of its own (kernels.hpp, kernels_lean.hpp,
kernels_pcm.hpp, kernels_coop.hpp, kernels_te.hpp, kernels_logddp.hpp, kernels_msipddp.hpp, dev_boxqp.hpp, plugin_solve.hip).  A family
that kept a literal where an option belongs, or read the neighbouring field, passes every test that leaves the options at their
defaults.  tests/option_cases.py moves each option, on a problem where the move changes the reference solve (tests/test_option_cases.py
holds that, and holds the oracle to the numpy twins on the same rows), on the families that restate the read; here the library runs
the rows:

  * whole solves against api.oracle_solve_batch with the bounds of tests/test_gpu_parity.py::test_full_solve_parity: iterations, status,
    sweeps and rollouts equal for every trajectory, objective 1e-7, X and U 1e-6, K 1e-5, and for IPDDP the iteration history of
    trajectory 0 (cost, merit, residuals, step sizes, mu, regularisation) at 1e-6 -- a wrong barrier update shows there even when the
    counts agree.  Every family's rows run again on the routes a handle takes only when asked (option_cases.ROUTES), the nx > 8 rows
    with the stacks wave-tiled (CDDP_HIP_T4=0) among them;
  * initialize -> backward -> forward(alphas) at 1e-8 for the rows that act before the first accept (initial scales, the
    fraction-to-boundary rule, the filter thresholds, the ladder's shape);
  * create(defaults) -> cddp_hip_set_options(row) -> solve gives the bits of create(row) -> solve: no stale copy of the options, of the
    ladder, of the route or of a captured graph;
  * the pendulum rows through cddp_hip_plugin_solve, whose host loop restates every read (host arithmetic on both sides), and a
    ladder of 40 step sizes, which that route walks whole;
  * the two fixed capacities of a handle: a ladder of CDDP_HIP_MAX_ALPHAS = 32 step sizes and an IPDDP filter of 7 + 1 points solve and
    match the oracle, the next size is refused by cddp_hip_create and by cddp_hip_set_options with a message that names the option."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import option_cases as OC
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = OC.ROWS + OC.IGNORED
TOL_STEP = 1e-8
MAX_ALPHAS, FILTER_SLOTS = 32, 8


def _batch(p):
    return 8 if p.nx <= 4 else 3


def _hip_solve(api, row, p, st, created_with=None):
    """The library's solve of a row's problem p on the starts st.  created_with: the problem the handle is created with; p's options
    then arrive through cddp_hip_set_options."""
    x0, U0, X0 = st
    B = x0.shape[0]
    hs = api.HipBatchSolver(created_with if created_with is not None else p, B)
    if created_with is not None:
        hs.set_options(p.options); hs.p = p
    hs.set_initial(x0, U0, X0)
    if row.start == "warm_duals":
        hs.initialize()
        S, Y = OC.starts_duals(p, B)
        hs.set_duals(S, Y); hs.set_warm_start(True)
    hs.solve()
    out = {"res": hs.results()}
    out["X"], out["U"] = hs.trajectory()
    out["K"], out["k"] = hs.gains()
    if p.options.return_iteration_info:
        out["hist"] = hs.history(1)[0]
    hs.close()
    return out


def _oracle_history(api, row, p, st):
    x0, U0, X0 = st
    o = api.Oracle(p)
    o.set_initial(x0[0], None if U0 is None else U0[0], None if X0 is None else X0[0])
    if row.start == "warm_duals":
        S, Y = OC.starts_duals(p, x0.shape[0])
        o.initialize(); o.set_duals(S[0], Y[0]); o.set_warm_start(True)
    o.solve()
    return o.history()


def _solve_against_oracle(api, name, row=None):
    row = row or OC.BY_NAME[name]
    p = OC.problem(api, row)
    ipddp = row.solver == "ipddp"
    if ipddp:
        p.options.return_iteration_info = 1
    B = _batch(p)
    st = OC.starts(api, p, row, B)
    got = _hip_solve(api, row, p, st)
    ores, oX, oU, oK = OC.oracle_solve(api, OC.problem(api, row), row, st)
    res = got["res"]
    assert OC.counts(res) == OC.counts(ores), (name, [(b, x, y) for b, (x, y) in enumerate(zip(OC.counts(res), OC.counts(ores))) if x != y])
    e = {"J": max(rel_err(res["final_objective"][b], ores["final_objective"][b]) for b in range(B)),
         "X": rel_err(got["X"], oX), "U": rel_err(got["U"], oU), "K": rel_err(got["K"], oK),
         "mu": rel_err(res["barrier_mu"], ores["barrier_mu"]), "reg": rel_err(res["regularization"], ores["regularization"]),
         "alpha": max(rel_err(res["alpha_pr"], ores["alpha_pr"]), rel_err(res["alpha_du"], ores["alpha_du"]))}
    if ipddp:
        q = OC.problem(api, row); q.options.return_iteration_info = 1
        oh = _oracle_history(api, row, q, st)
        assert got["hist"].shape == oh.shape, (name, got["hist"].shape, oh.shape)
        e["hist"] = rel_err(got["hist"], oh)
    print("SOLVE %s %s" % (name, " ".join("%s %.1e" % kv for kv in e.items())))
    assert e["J"] < 1e-7 and e["X"] < 1e-6 and e["U"] < 1e-6 and e["K"] < 1e-5, (name, e)
    assert e["mu"] < 1e-6 and e["reg"] < 1e-6 and e["alpha"] < 1e-6 and e.get("hist", 0.0) < 1e-6, (name, e)


@pytest.mark.parametrize("name", [r.name for r in ALL])
def test_solve_matches_oracle(api, oracle_built, name):
    _solve_against_oracle(api, name)


ROUTE_CASES = [(r.name, "%s=%s" % kv) for r in ALL for env in OC.ROUTES[r.family] for kv in env.items()]


@pytest.mark.parametrize("name,route", ROUTE_CASES)
def test_solve_matches_oracle_on_the_other_routes(api, oracle_built, name, route, monkeypatch):
    """The routes a handle takes only when asked restate the same reads (option_cases.ROUTES): the grouped pair rollout of kernels_pcm.hpp,
    the fused one-lane kernels, the one-wave rollouts, the two-stage ladder, and for nx > 8 the wave-tiled stacks of k_condense, k_post
    and k_update.  The same rows, the same bounds."""
    for k in ("CDDP_HIP_K4_NA", "CDDP_HIP_SWEEP", "CDDP_HIP_LS_STAGES", "CDDP_HIP_T4", "CDDP_HIP_LG_ROLLOUT", "CDDP_HIP_MS_ROLLOUT"):
        monkeypatch.delenv(k, raising=False)
    k, v = route.split("=")
    monkeypatch.setenv(k, v)
    _solve_against_oracle(api, name)


# ---------------------------------------------------------------------------------------------------------------- step level
STEP_PREFIXES = ("init_scales", "tau09", "armijo03", "accept1e2", "maxviol", "minviol", "mu_init0", "ls_factor0", "ls_init06", "ls_one",
                 "ls_flat", "ls_min0", "ls_cap32", "log_mu_init", "log_delta", "ms_costate", "ms_controlled", "ms_seg3", "ms_linear", "ms_hybrid",
                 "theta_l2", "boxqp_", "reg-")
STEP_ROWS = [r.name for r in ALL if r.name.startswith(STEP_PREFIXES) and r.start != "warm_duals"]


@pytest.mark.parametrize("name", STEP_ROWS)
def test_step_level_matches_oracle(api, oracle_built, name):
    """initialize -> backward -> forward(alphas), as tests/test_gpu_parity.py::test_step_level_parity, at its 1e-8: the initial iterate's
    cost, merit, residuals, mu and step sizes, the sweep's verdict and regularisation, K, k, V_x, V_xx, dV, and every trial's verdict,
    cost, merit and theta on the row's own ladder."""
    row = OC.BY_NAME[name]
    p = OC.problem(api, row)
    B = _batch(p)
    x0, U0, X0 = OC.starts(api, p, row, B)
    hs = api.HipBatchSolver(p, B)
    hs.set_initial(x0, U0, X0)
    hs.initialize()
    r0 = hs.results()
    ok = hs.backward()
    K, k = hs.gains(); Vx, Vxx = hs.value(); dV, reg = hs.backward_scalars()
    alphas = api.Oracle(p).alphas()
    trials = hs.forward(alphas)
    hs.close()
    worst = 0.0
    for b in range(B):
        o = api.Oracle(p)
        o.set_initial(x0[b], None if U0 is None else U0[b], None if X0 is None else X0[b])
        o.initialize()
        ro = o.result()
        e = [rel_err(r0[f][b], ro[f]) for f in ("final_objective", "merit_function", "inf_pr", "inf_comp", "barrier_mu", "alpha_pr", "alpha_du", "regularization")]
        assert ok[b] == o.backward(retry=True), (name, b)
        Ko, ko = o.gains(); Vxo, Vxxo = o.value(); dVo, rego = o.backward_scalars()
        assert reg[b] == rego, (name, b, reg[b], rego)
        e += [rel_err(K[b], Ko), rel_err(k[b], ko), rel_err(Vx[b], Vxo), rel_err(Vxx[b], Vxxo), rel_err(dV[b], dVo)]
        for a, alpha in enumerate(alphas):
            t = o.forward(alpha); g = trials[b, a]
            assert g["success"] == t["success"], (name, b, alpha, g, t)
            e += [abs(g["alpha_pr"] - t["alpha_pr"]), abs(g["alpha_du"] - t["alpha_du"])]
            if t["success"]:
                e += [rel_err(g["cost"], t["cost"]), rel_err(g["merit_function"], t["merit_function"]), rel_err(g["theta"], t["theta"])]
        assert all(np.isfinite(v) and v < TOL_STEP for v in e), (name, b, e)
        worst = max(worst, max(e))
    print("STEP %s %.1e" % (name, worst))


# ---------------------------------------------------------------------------------------------------------------- set_options
def _same_ladder(api, row):
    return len(api.Oracle(OC.problem(api, row)).alphas()) == len(api.Oracle(OC.problem(api, row, False)).alphas())


@pytest.mark.parametrize("name", [r.name for r in ALL])
def test_set_options_equals_create(api, oracle_built, name):
    """create(defaults) -> cddp_hip_set_options(row) -> solve against create(row) -> solve: result words, X, U, K and k bit for bit.  (A
    handle's ladder length is fixed at create: rows that change it are refused by set_options, which the test asserts instead.)"""
    row = OC.BY_NAME[name]
    p = OC.problem(api, row)
    st = OC.starts(api, p, row, _batch(p))
    if not _same_ladder(api, row):
        hs = api.HipBatchSolver(OC.problem(api, row, False), st[0].shape[0])
        with pytest.raises(api.HipError, match="ladder size is fixed at create time"):
            hs.set_options(p.options)
        hs.close()
        return
    a = _hip_solve(api, row, p, st)
    b = _hip_solve(api, row, OC.problem(api, row), st, created_with=OC.problem(api, row, False))
    for f in a["res"].dtype.names:
        assert np.array_equal(a["res"][f], b["res"][f], equal_nan=(a["res"][f].dtype.kind == "f")), (name, f)
    for key in ("X", "U", "K", "k"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (name, key)


# ---------------------------------------------------------------------------------------------------------------- host plug-in route
# (the C plug-in has no Hessian callback: the full-DDP row is left to the resident route)
PLUGIN_ROWS = [r.name for r in ALL if r.base == "pendulum40" and r.start == "cold" and r.solver in ("ipddp", "logddp", "msipddp")
               and r.setup.get("use_ilqr", 1)]


@pytest.fixture(scope="module")
def pendulum_plugin(api, tmp_path_factory):
    """tests/cpp/pendulum_plugin.c: the plant, objective and control box of pyapi.pendulum_problem as C callbacks (tests/test_host_plugins.py)."""
    so = str(tmp_path_factory.mktemp("plugin") / "pendulum_plugin.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(REPO, "tests", "cpp", "pendulum_plugin.c"), "-lm"])
    pl = C.CDLL(so)

    class Params(C.Structure):
        _fields_ = [(n, C.c_double) for n in ("dt", "length", "mass", "damping", "gravity", "Qf", "R", "umax")]
    prm = Params(0.02, 0.5, 1.0, 0.01, 9.81, 100.0, 0.1, 20.0)
    ps = api.PluginStruct()
    ps.abi_version = api.ABI_VERSION; ps.options_bytes = C.sizeof(api.Options); ps.user = C.cast(C.pointer(prm), C.c_void_p)
    ps.nx, ps.nu, ps.n_constraints = 2, 1, 1
    ps.constraint_dims[0] = 2
    for field, sym, ftype in (("discrete_dynamics", "pend_dynamics", api._F_DYN), ("jacobians", "pend_jacobians", api._F_JAC), ("running_cost", "pend_running_cost", api._F_RC),
                              ("terminal_cost", "pend_terminal_cost", api._F_TC), ("running_cost_derivatives", "pend_running_cost_derivatives", api._F_RCD),
                              ("terminal_cost_derivatives", "pend_terminal_cost_derivatives", api._F_TCD), ("constraints", "pend_constraints", api._F_CON)):
        setattr(ps, field, C.cast(getattr(pl, sym), ftype))
    return ps, (pl, prm)


def _plugin_against_oracle(api, pendulum_plugin, row):
    p = OC.problem(api, row)
    ps, _keep = pendulum_plugin
    B, N = 6, p.N
    x0, U0, X0 = OC.starts(api, p, row, B)
    lib = api.load_hip()
    res = np.zeros(B, dtype=api.RESULT_DTYPE); X = np.zeros((B, N + 1, 2)); U = np.zeros((B, N, 1))
    rc = lib.cddp_hip_plugin_solve(C.byref(ps), int(p.c.solver), N, C.c_double(p.dt), C.byref(p.options), 0, B, api._ptr(x0), None, None,
                                   res.ctypes.data_as(C.c_void_p), api._ptr(X), api._ptr(U), None)
    assert rc == 0, lib.cddp_hip_last_error().decode()
    ores, oX, oU, _ = OC.oracle_solve(api, p, row, (x0, U0, X0))
    assert OC.counts(res) == OC.counts(ores), (row.name, OC.counts(res), OC.counts(ores))
    eJ = float(np.max(np.abs(res["final_objective"] - ores["final_objective"]) / np.maximum(1.0, np.abs(ores["final_objective"]))))
    eX, eU = float(np.max(np.abs(X - oX))), float(np.max(np.abs(U - oU)))
    print("PLUGIN %s J %.1e X %.1e U %.1e" % (row.name, eJ, eX, eU))
    assert eJ < 1e-9 and eX < 1e-8 and eU < 1e-7, (row.name, eJ, eX, eU)
    return res


@pytest.mark.host_arithmetic
@pytest.mark.parametrize("name", PLUGIN_ROWS)
def test_plugin_route_matches_oracle(api, oracle_built, pendulum_plugin, name):
    """cddp_hip_plugin_solve with the pendulum as a C plug-in, at the bounds of
    tests/test_host_plugins.py::test_c_plugin_matches_the_oracle_on_many_threads: the four counts equal, objective 1e-9, X 1e-8, U 1e-7."""
    _plugin_against_oracle(api, pendulum_plugin, OC.BY_NAME[name])


@pytest.mark.host_arithmetic
@pytest.mark.parametrize("solver", ["ipddp", "logddp", "msipddp"])
def test_plugin_route_walks_a_ladder_longer_than_a_handle_holds(api, oracle_built, pendulum_plugin, solver):
    """The plug-in route's host loop keeps the ladder in a vector: 40 step sizes at a factor of 0.8, which cddp_hip_create refuses, are
    all walked there, as the reference walks them (it used to stop at the first 32).  Against the oracle, at the bounds above."""
    row = _ladder_row("pendulum40", solver, 40)
    p = OC.problem(api, row)
    assert len(api.Oracle(p).alphas()) == 40
    with pytest.raises(api.HipError, match="more than CDDP_HIP_MAX_ALPHAS = 32"):
        api.HipBatchSolver(p, 4)
    _plugin_against_oracle(api, pendulum_plugin, row)
    # the last eight step sizes are reached: with max_iterations = 1 and an Armijo bound no trial can meet, every trial of the ladder runs
    hard = row._replace(opts=dict(row.opts, max_iterations=1, filter_armijo_constant=1e6, filter_merit_acceptance_threshold=1e6))
    res = _plugin_against_oracle(api, pendulum_plugin, hard)
    assert np.all(res["n_forward"] == 40), res["n_forward"]


# ---------------------------------------------------------------------------------------------------------------- the capacities
LADDER_CASES = [("pendulum40", "ipddp"), ("cartpole40", "ipddp"), ("pendulum40", "logddp"), ("pendulum40", "msipddp")]


def _ladder_row(base, solver, n):
    return OC.Row("ladder%d-%s-%s" % (n, base, solver), base, solver, dict(ls_step_reduction_factor=0.8, ls_max_iterations=n), "", "cold", {})


@pytest.mark.parametrize("base,solver", LADDER_CASES)
def test_ladder_at_the_capacity_solves_and_the_next_is_refused(api, oracle_built, base, solver):
    """ls_max_iterations = 32 at a reduction factor of 0.8 is a ladder of CDDP_HIP_MAX_ALPHAS step sizes: it solves and matches the oracle
    (test_solve_matches_oracle's ls_cap32 rows are the same problems).  33 is a ladder the handle cannot hold; the reference walks all
    of it, so cddp_hip_create refuses it, and cddp_hip_set_options refuses it on a live handle, naming the option and the limit."""
    row = _ladder_row(base, solver, MAX_ALPHAS)
    p = OC.problem(api, row)
    assert len(api.Oracle(p).alphas()) == MAX_ALPHAS
    _solve_against_oracle(api, row.name, row)
    over = OC.problem(api, _ladder_row(base, solver, MAX_ALPHAS + 1))
    assert len(api.Oracle(over).alphas()) == MAX_ALPHAS + 1
    msg = "ls_max_iterations = 33 gives a ladder of 33 step sizes, more than CDDP_HIP_MAX_ALPHAS = 32"
    with pytest.raises(api.HipError, match=msg):
        api.HipBatchSolver(over, 4)
    hs = api.HipBatchSolver(p, 4)
    with pytest.raises(api.HipError, match=msg):
        hs.set_options(over.options)
    hs.close()


def test_filter_at_the_capacity_solves_and_the_next_is_refused(api, oracle_built):
    """The IPDDP filter column has eight slots and holds ipddp_max_filter_size + 1 points between an accept and the prune that follows
    it: 7 solves and matches the oracle (rows filter_size7-*), 8 is refused at create and by set_options.  MSIPDDP sizes its filter by
    max_iterations and never reads the option: 8 is accepted there."""
    for name in ("filter_size7-split_unicycle", "filter_size7-split_unicycle_monotonic"):
        _solve_against_oracle(api, name)
    row = OC.BY_NAME["filter_size7-split_unicycle"]
    over = OC.problem(api, row); over.options.ipddp_max_filter_size = FILTER_SLOTS
    msg = "ipddp_max_filter_size = 8: the filter holds max_filter_size \\+ 1 points before it is pruned and has 8 slots, so at most 7"
    with pytest.raises(api.HipError, match=msg):
        api.HipBatchSolver(over, 4)
    hs = api.HipBatchSolver(OC.problem(api, row), 4)
    with pytest.raises(api.HipError, match=msg):
        hs.set_options(over.options)
    hs.close()
    ms = OC.problem(api, OC.BY_NAME["mu_power18-ms_pendulum"]); ms.options.ipddp_max_filter_size = FILTER_SLOTS
    hs = api.HipBatchSolver(ms, 4); hs.set_options(ms.options); hs.close()
