"""Plants 11-23 on every solver and layout they are compiled for.

inst_spacecraft.hip, inst_plants_small.hip and inst_plants_nx10.hip register the thirteen newer plants as 26 kernel sets (each plant
without path rows and with a control box); with the four solvers that is 104 pairs, of which cddp_hip_create accepts 94 and refuses 10
(MSIPDDP with a box at nu != 1).  tests/plant_matrix.py::MATRIX names every pair once.  test_remaining_plants.py and
test_spacecraft_plants.py run 30 of the 94 at B = 1; this file runs the other 64 -- every unconstrained set on CLDDP and IPDDP, LogDDP
on 24 sets, MSIPDDP on 14 -- on a batch of B = 70 built from three distinct initial states laid round-robin, so that every lane group
of the cooperative sweeps and the ragged last tile are live:

  * CPU: the table is complete against the Launcher<...>::set lines; the pyapi descriptor and the golden builder's spec of every set
    agree field by field; the twins stay finite on every case and their decision counts do not move under a relative 1e-12 change of
    x0 (so a count mismatch on the device is the device's); the twin refuses the 10 refused pairs.
  * GPU, against the numpy twins (oracle/twin): one sweep and every line-search trial at 1e-8, the whole solve in counts (equal), objective,
    X and U (1e-6) -- for each of the three members; all copies of a member bit for bit equal wherever they sit in the batch.
  * GPU, form against form, bitwise: cooperative against one-lane sweep (LogDDP; CLDDP and IPDDP without path rows), pair against
    one-wave rollouts, split against fused MSIPDDP sweep.

The tolerances are those test_remaining_plants.py / test_spacecraft_plants.py already hold these plants to against the twin."""
import os
import shutil

import numpy as np
import pytest

import plant_matrix as PM

C, F, R = PM.C, PM.F, PM.R
NEW = PM.cases()                                   # the 64 pairs no other file runs
TOL_STEP, TOL_SOLVE = 1e-8, 1e-6


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ================================================================================ CPU: the table
def _table_against(sets):
    want = {(s, v) for s in sets for v in PM.SOLVERS}
    have = {(s, v) for s, row in PM.MATRIX.items() for v in row}
    return sorted(want - have), sorted(have - want)


def test_matrix_covers_every_registered_set_times_every_solver():
    sets = PM.registered_sets()
    assert len(sets) == len(set(sets)) == 26, sets
    missing, extra = _table_against(sets)
    assert not missing and not extra, (missing, extra)
    modes = [m for row in PM.MATRIX.values() for m in row.values()]
    assert set(modes) <= {C, F, R} and all(set(row) == set(PM.SOLVERS) for row in PM.MATRIX.values())
    assert (len(modes), modes.count(R), modes.count(F)) == (104, 10, 5)
    # refused: exactly MSIPDDP with path rows at nu != 1 and nx != nu (launch.hpp: kMs)
    for s, row in PM.MATRIX.items():
        nx, nu = PM.PLANTS[s.split("/")[0]][:2]
        assert (row["msipddp"] == R) == (s.endswith("/ctrlbox") and nu != 1 and nx != nu), s
        assert R not in (row["clddp"], row["ipddp"], row["logddp"])
    assert len(PM.ELSEWHERE) == 30 and all(PM.MATRIX[s][v] == C for s, v in PM.ELSEWHERE)
    assert len(NEW) == 64 and len(set(NEW)) == 64


def test_a_set_registered_later_is_missed_by_the_table(tmp_path):
    """The completeness test is live: one more Launcher line in a copy of an instantiation file is reported as missing."""
    files = []
    for n in PM.INST_FILES:
        shutil.copy(os.path.join(PM.CSRC, n), tmp_path / n); files.append(str(tmp_path / n))
    with open(files[1]) as f:
        text = f.read()
    line = '  v.push_back(Launcher<DubinsCarModel, ConList<>>::set("dubins_car/none"));'
    assert line in text
    with open(files[1], "w") as f:
        f.write(text.replace(line, line + '\n  v.push_back(Launcher<DubinsCarModel, ConList<StateBox<3>>>::set("dubins_car/statebox"));'))
    missing, extra = _table_against(PM.registered_sets(files))
    assert missing == [("dubins_car/statebox", v) for v in sorted(PM.SOLVERS)] and not extra


OPTION_NAMES = {   # pyapi.Options field -> the twins' option key, for every option a twin reads
    "tolerance": "tolerance", "acceptable_tolerance": "acceptable_tolerance", "max_iterations": "max_iterations", "use_ilqr": "use_ilqr",
    "enable_parallel": "enable_parallel", "termination_scaling_max_factor": "termination_scaling_max_factor",
    "ls_max_iterations": "ls_max_iterations", "ls_initial_step_size": "ls_initial_step_size", "ls_min_step_size": "ls_min_step_size",
    "ls_step_reduction_factor": "ls_step_reduction_factor", "reg_initial_value": "reg_initial_value", "reg_update_factor": "reg_update_factor",
    "reg_max_value": "reg_max_value", "reg_min_value": "reg_min_value", "boxqp_max_iterations": "boxqp_max_iterations",
    "boxqp_min_gradient_norm": "boxqp_min_gradient_norm", "boxqp_min_relative_improvement": "boxqp_min_relative_improvement",
    "boxqp_step_decrease_factor": "boxqp_step_decrease_factor", "boxqp_min_step_size": "boxqp_min_step_size",
    "boxqp_armijo_constant": "boxqp_armijo_constant", "filter_merit_acceptance_threshold": "filter_merit_acceptance_threshold",
    "filter_violation_acceptance_threshold": "filter_violation_acceptance_threshold",
    "filter_max_violation_threshold": "filter_max_violation_threshold",
    "filter_min_violation_for_armijo_check": "filter_min_violation_for_armijo_check", "filter_armijo_constant": "filter_armijo_constant",
    "ipddp_dual_var_init_scale": "dual_var_init_scale", "ipddp_slack_var_init_scale": "slack_var_init_scale",
    "ipddp_barrier_tol_mult": "barrier_tol_mult", "ipddp_barrier_update_dual_weight": "barrier_update_dual_weight",
    "ipddp_mu_kappa_epsilon": "mu_kappa_epsilon", "ipddp_check_state_stationarity": "check_state_stationarity",
    "ipddp_max_filter_size": "max_filter_size", "ipddp_theta_0_floor": "theta_0_floor",
    "ipddp_jacobian_regularization_value": "jacobian_regularization_value",
    "ipddp_jacobian_regularization_exponent": "jacobian_regularization_exponent", "barrier_mu_initial": "mu_initial",
    "barrier_mu_min_value": "mu_min_value", "barrier_mu_update_factor": "mu_update_factor", "barrier_mu_update_power": "mu_update_power",
    "barrier_min_fraction_to_boundary": "min_fraction_to_boundary", "logddp_mu_initial": "log_mu_initial",
    "logddp_mu_min_value": "log_mu_min_value", "logddp_mu_update_factor": "log_mu_update_factor", "logddp_relaxed_delta": "log_relaxed_delta",
    "msipddp_costate_var_init_scale": "ms_costate_var_init_scale", "msipddp_segment_length": "ms_segment_length",
    "msipddp_use_controlled_rollout": "ms_use_controlled_rollout", "warm_start": "warm_start",
}
INTEGRATORS = ["euler", "heun", "rk3", "rk4"]


@pytest.mark.parametrize("set_name", list(PM.MATRIX))
def test_descriptor_and_twin_spec_agree(api, set_name):
    """What the library is handed (pyapi.*_problem) and what the twins are handed (the golden builders) are the same problem: weights,
    goal, start, guess, step, horizon, integrator, box and every option a twin reads -- for each solver's descriptor, at this file's
    horizon and at the builders' own.  And one step of the library's plant with the descriptor's parameters equals the twin plant's."""
    for solver in PM.SOLVERS:
        case = PM.case_id(set_name, solver)
        plant, box, _ = PM.parse(case)
        for N in (PM.horizon(case), PM.DEFAULT_HORIZON[plant]):
            s = {"clddp": api.SOLVER_CLDDP, "ipddp": api.SOLVER_IPDDP, "logddp": api.SOLVER_LOGDDP, "msipddp": api.SOLVER_MSIPDDP}[solver]
            p = PM.PLANTS[plant][2](api, s, box, N)
            sp = PM.PLANTS[plant][3]({"clddp": "CLDDP"}.get(solver, "IPDDP"), box, N)
            assert (p.c.solver, p.nx, p.nu) == (s, sp["model"].nx, sp["model"].nu) == (s,) + PM.PLANTS[plant][:2]
            assert (p.N, p.dt, INTEGRATORS[p.c.integrator]) == (sp["N"], sp["dt"], sp["integrator"]), case
            for got, want in ((p.Q, sp["Q"]), (p.R, sp["R"]), (p.Qf, sp["Qf"]), (p.x_ref, sp["xref"]), (p.x0, sp["x0"])):
                assert np.array_equal(got, np.asarray(want, float)), case
            U0 = api.batch_U0(p, 1)
            assert (U0 is None) == (sp.get("U0") is None), case
            if U0 is not None:
                assert np.array_equal(U0[0], np.asarray(sp["U0"], float)), case
            cons = sp["constraints"]
            assert len(p._cons) == len(cons) == int(box), case
            if box:
                c = p._cons[0]; tb = cons["ControlConstraint"]
                assert c.name == b"ControlConstraint" and c.kind == api.CON_CONTROL_BOX and c.dim == p.nu and c.scale == 1.0
                assert np.array_equal(np.array(c.lower[:c.dim]), tb.lo) and np.array_equal(np.array(c.upper[:c.dim]), tb.up), case
            topt = PM.T.default_options()
            topt.update(dict(log_mu_initial=1.0, log_mu_min_value=1e-10, log_mu_update_factor=0.5, log_relaxed_delta=1e-10,
                             ms_costate_var_init_scale=1e-6, ms_segment_length=5, ms_use_controlled_rollout=False, warm_start=False))
            topt.update(sp["options"])
            assert set(sp["options"]) <= set(OPTION_NAMES.values()), case
            for field, key in OPTION_NAMES.items():
                assert getattr(p.options, field) == topt[key], (case, field)
            assert p.options.barrier_strategy == 0 and topt["barrier_strategy"] == "ADAPTIVE" and p.options.ipddp_theta_norm_l2 == 0 and topt["theta_norm"] == "l1"
            assert p.options.msipddp_rollout_type == 0 and topt.get("ms_rollout_type", "nonlinear") == "nonlinear"
        x = np.asarray(sp["x0"], float); u = np.zeros(p.nu) if sp.get("U0") is None else np.asarray(sp["U0"], float)[0]
        prm = list(p.c.model_params)[:9]
        got = api.model_eval(p.c.model, p.c.integrator, p.dt, prm, p.nx, p.nu, x, u)["step"]
        assert rel_err(got, PM.T.discrete_step(sp["model"], sp["integrator"], sp["dt"], x, u, 0.0)) < 1e-13, case


def test_batch_layout():
    """Three distinct members, round-robin: each one sits in the first lane group, on both sides of lane 63 / 64 and in the ragged tail."""
    x0, where = PM.batch("usv_3dof_none-logddp")
    assert x0.shape == (70, 6) and [len(w) for w in where] == [24, 23, 23]
    assert len({tuple(r) for r in x0}) == 3 and np.array_equal(x0[0], np.zeros(6))
    for w in where:
        assert w[0] < 4 and np.any(w < 64) and np.any(w >= 64) and np.any(w >= 67)
        assert np.all(x0[w] == x0[w[0]])
    assert 63 in where[0] and 64 in where[1] and 65 in where[2]


@pytest.mark.parametrize("case", NEW)
def test_twin_counts_are_not_on_a_knife_edge(case):
    """The twin alone: every member's solve is finite, and a relative 1e-12 change of x0 changes none of its four counts.  A count that
    differs on the device is then not rounding.  PM.SEED was chosen so that this holds: change the seed, not this assertion."""
    for x, r in zip(PM.members(case), PM.twin_solves(case)):
        assert np.isfinite(r["final_objective"]) and np.all(np.isfinite(r["X"])) and np.all(np.isfinite(r["U"])), (case, r["counts"])
        r2 = PM.twin_solve(case, x + 1e-12 * np.maximum(1.0, np.abs(x)), **PM.solve_options(case))
        assert r2["counts"] == r["counts"], (case, r["counts"], r2["counts"])
        if PM.mode_of(case) == F:
            assert r["counts"][0] == 1


@pytest.mark.parametrize("case", PM.cases(modes=(F,)))
def test_first_iteration_cases_overflow_in_the_twin_after_it(case):
    """Why five unconstrained MSIPDDP cases are compared over one iteration only.  The reference's unconstrained sweep factors Q_uu at a
    step only while that step's cached factor is invalid (msipddp_solver.cpp:1169-1175: need_recompute; the flag is cleared by a failed
    factorisation alone, :1183), so the second sweep solves with the first sweep's factors, the value recursion overflows, and the
    trial's NaN cost is accepted through std::copysign(1.0, dJ) (:1523): the solve ends "converged" on a NaN objective.  That is the
    reference's own behaviour, restated by the twin and by the device; past the overflow neither side's bits mean anything."""
    r = PM.twin_solve(case, PM.members(case)[0])
    assert not np.isfinite(r["final_objective"]) and r["counts"][0] >= 2, (case, r["counts"], r["final_objective"])


@pytest.mark.parametrize("case", PM.cases(modes=(R,), new_only=False))
def test_twin_refuses_the_refused_pairs(case):
    with pytest.raises(ValueError, match="1398"):
        PM.M.MSIPDDP(PM.spec(case))


# ================================================================================ GPU: refusals
@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.cases(modes=(R,), new_only=False))
def test_refused_pairs_are_refused_at_create(api, case):
    """The message of test_msipddp_device.py::test_undefined_constrained_shape_is_refused."""
    with pytest.raises(RuntimeError, match="1398"):
        api.HipBatchSolver(PM.problem(api, case), 4)


# ================================================================================ GPU: against the twins
def _same_bits(name, arr, where, case):
    """All copies of one member are the same bits wherever they sit."""
    for w in where:
        ref = arr[w[0]]
        for b in w[1:]:
            assert np.array_equal(arr[b], ref, equal_nan=(arr.dtype.kind == "f")), (case, name, int(w[0]), int(b))


def _same_bits_records(name, rec, where, case):
    for f in rec.dtype.names:
        if not f.startswith("_"):
            _same_bits("%s.%s" % (name, f), rec[f], where, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NEW)
def test_step_level_matches_the_twin(api, case):
    """initialize -> backward -> forward(alphas) on the batch of 70.  Per member against its twin: the sweep's success flag and final
    regularisation exactly; K, k, V_x, V_xx and dV at 1e-8; every trial's success flag exactly, cost and merit at 1e-8 where it
    succeeded; for LogDDP and MSIPDDP the initial cost, merit and violation.  And every field bit for bit equal among a member's copies."""
    _step_against(api, case, PM.problem(api, case), PM.twin_steps(case), "STEP")


def _step_against(api, case, p, tw, label, need_accepted_trial=True):
    solver = PM.parse(case)[2]
    x0, where = PM.batch(case)
    U0 = api.batch_U0(p, PM.B)
    hs = api.HipBatchSolver(p, PM.B)
    hs.set_initial(x0, U0)
    hs.initialize()
    r0 = hs.results()
    ok = hs.backward()
    K, k = hs.gains(); Vx, Vxx = hs.value(); dV, reg = hs.backward_scalars()
    trials = hs.forward(np.array(tw[0]["alphas"]))
    hs.close()
    for name, arr in (("ok", ok), ("K", K), ("k", k), ("Vx", Vx), ("Vxx", Vxx), ("dV", dV), ("reg", reg)):
        _same_bits(name, arr, where, case)
    _same_bits_records("init", r0, where, case)
    _same_bits_records("trial", trials, where, case)
    worst = {}
    for m, t in enumerate(tw):
        b = int(where[m][1])            # any copy: they are the same bits
        assert bool(ok[b]) == t["ok"] and reg[b] == t["reg"], (case, m, ok[b], reg[b], t["ok"], t["reg"])
        assert t["ok"], (case, m)       # (every case's first sweep succeeds in the twin: the comparisons below are never vacuous)
        e = {"K": rel_err(K[b], t["K"]), "k": rel_err(k[b], t["k"]), "Vx": rel_err(Vx[b], t["Vx"]), "Vxx": rel_err(Vxx[b], t["Vxx"]),
             "dV": rel_err(dV[b], t["dV"])}
        if solver in ("logddp", "msipddp"):
            e["init"] = max(rel_err(r0["final_objective"][b], t["cost"]), rel_err(r0["merit_function"][b], t["merit"]),
                            rel_err(r0["inf_pr"][b], t["violation"]))
        n_ok = 0
        e["trial"] = 0.0
        for a, (succ, cost, merit) in enumerate(t["trials"]):
            g = trials[b, a]
            assert bool(g["success"]) == succ, (case, m, a, g, succ)
            if succ:
                n_ok += 1
                e["trial"] = max(e["trial"], rel_err(g["cost"], cost), rel_err(g["merit_function"], merit))
        assert n_ok > 0 or not need_accepted_trial, (case, m)
        for key, v in e.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print("%s %s %s" % (label, case, " ".join("%s %.1e" % kv for kv in worst.items())))
    assert all(np.isfinite(v) and v < TOL_STEP for v in worst.values()), (case, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NEW)
def test_whole_solve_matches_the_twin(api, case):
    """cddp_hip_solve on the batch of 70: iterations, status, sweeps and rollouts equal to the twin's for all three members, objective, X
    and U at 1e-6, and a member's copies bit for bit equal.  MSIPDDP: the costates too, at the objective's bound -- they come out of the
    accepted rollout like X and U, from gains the step-level test holds at 1e-8, and under iLQR they enter nothing else, so no other
    field would show an error in them.  The five compare-first-iteration cases run max_iterations = 1
    (test_first_iteration_cases_overflow_in_the_twin_after_it says why)."""
    solver = PM.parse(case)[2]
    p = PM.problem(api, case, **PM.solve_options(case))
    x0, where = PM.batch(case)
    U0 = api.batch_U0(p, PM.B)
    tw = PM.twin_solves(case)
    hs = api.HipBatchSolver(p, PM.B)
    hs.set_initial(x0, U0)
    hs.solve()
    res = hs.results(); X, U = hs.trajectory()
    Lam = hs.costates() if solver == "msipddp" else None       # (N rows: what the rollout's costate trial k_lambda, K_lambda left)
    hs.close()
    _same_bits_records("result", res, where, case)
    _same_bits("X", X, where, case); _same_bits("U", U, where, case)
    worst = {"J": 0.0, "X": 0.0, "U": 0.0}
    if Lam is not None:
        _same_bits("Lam", Lam, where, case)
        worst["Lam"] = max(rel_err(Lam[int(where[m][1])], t["Lam"]) for m, t in enumerate(tw))
    for m, t in enumerate(tw):
        b = int(where[m][1])
        got = (int(res["iterations"][b]), api.STATUS_STRINGS[int(res["status"][b])], int(res["n_backward"][b]), int(res["n_forward"][b]))
        print("SOLVE %s member %d device %s twin %s J %.12g %.12g" % (case, m, got, t["counts"], res["final_objective"][b], t["final_objective"]))
        assert got == t["counts"], (case, m, got, t["counts"])
        worst["J"] = max(worst["J"], rel_err(res["final_objective"][b], t["final_objective"]))
        worst["X"] = max(worst["X"], float(np.max(np.abs(X[b] - t["X"])))); worst["U"] = max(worst["U"], float(np.max(np.abs(U[b] - t["U"]))))
    print("SOLVE %s %s" % (case, " ".join("%s %.1e" % kv for kv in worst.items())))
    assert all(np.isfinite(v) and v < TOL_SOLVE for v in worst.values()), (case, worst)


# ================================================================================ GPU: full DDP on LogDDP and MSIPDDP
@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.ddp_cases(PM.DDP_TENSORS))
def test_full_ddp_step_level_matches_the_twin(api, case):
    """use_ilqr = 0 under LogDDP and MSIPDDP: the one-lane sweeps with the plants' Hessian tensors (weighed with V_x under LogDDP,
    logddp_solver.cpp:505-515, with the costates under MSIPDDP, msipddp_solver.cpp:1151-1163) against the twins' tensor-term branches
    with their hyper-dual Hessians: the fields and bounds of test_step_level_matches_the_twin, on a horizon of 20 steps (the reason is
    test_remaining_plants.py::test_hip_full_ddp_step_level's).  (No trial of the unconstrained forklift's first member is accepted, in
    the twin and on the device alike.)"""
    p = PM.problem(api, case, PM.DDP_HORIZON, use_ilqr=0)
    _step_against(api, case, p, PM.twin_ddp_steps(case), "DDP", need_accepted_trial=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.ddp_cases(PM.DDP_NONE))
def test_full_ddp_without_an_autodiff_expression_is_refused(api, case):
    """The two-body and nonlinear relative-motion plants: the reference's message, under LogDDP and MSIPDDP as under IPDDP."""
    with pytest.raises(api.HipError, match="getContinuousDynamicsAutodiff must be overridden"):
        api.HipBatchSolver(PM.problem(api, case, use_ilqr=0), 4)
    with pytest.raises(RuntimeError, match="getContinuousDynamicsAutodiff"):
        sp = PM.spec(case)
        sp["model"].hess(np.asarray(sp["x0"], float), np.zeros(sp["model"].nu), 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.ddp_cases(PM.DDP_BLOCKED))
def test_full_ddp_on_blocked_dual_plants_is_refused_with_a_pointer(api, case):
    """The plants whose second-order terms exist on the device in the blocked dual form of the IPDDP sweeps only: refused at create with
    the route that serves them named, as test_logddp_device.py::test_quadrotor_full_ddp_is_refused_with_a_pointer -- no silent fallback."""
    with pytest.raises(api.HipError, match="cddp_hip_plugin_solve"):
        api.HipBatchSolver(PM.problem(api, case, use_ilqr=0), 4)


# ================================================================================ GPU: form against form, bitwise
def _run_forms(api, case, with_gains):
    p = PM.problem(api, case, **PM.solve_options(case))
    x0, _ = PM.batch(case)
    U0 = api.batch_U0(p, PM.B)
    hs = api.HipBatchSolver(p, PM.B); hs.set_initial(x0, U0); hs.initialize(); ok = hs.backward()
    K, k = hs.gains(); Vx, Vxx = hs.value(); dV, reg = hs.backward_scalars(); r1 = hs.results()
    tr = hs.forward(np.array(PM.twin_alphas(case))); hs.close()
    hs = api.HipBatchSolver(p, PM.B); hs.set_initial(x0, U0); hs.solve()
    ms = PM.parse(case)[2] == "msipddp"
    r = hs.results(); X, U = hs.trajectory(); K2, k2 = hs.gains()
    d = (hs.duals() if hs.m > 0 else ()) + (hs.costates(),) if ms else ()
    hs.close()
    succ = tr["success"] == 1
    arrays = [ok, reg, tr["success"], tr["cost"][succ], tr["merit_function"][succ], X, U] + list(d)
    if with_gains:
        arrays += [K, k, Vx, Vxx, dV, K2, k2]
    return arrays, (r1, r)


def _assert_forms_equal(a, b, key):
    for i, (u, v) in enumerate(zip(a[0], b[0])):
        assert np.array_equal(u, v, equal_nan=True), (key, i)
    for u, v in zip(a[1], b[1]):
        for f in u.dtype.names:
            assert np.array_equal(u[f], v[f], equal_nan=(u[f].dtype.kind == "f")), (key, f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.cases(new_only=False, solvers=("logddp",), nx_max=8))
def test_logddp_cooperative_and_lane_sweeps_agree_bitwise(api, case, monkeypatch):
    """k_backward_coop_plain<Model, true, Cons> against the one-lane k_backward_logddp (CDDP_HIP_SWEEP=lane) at NX = 2 ... 8, as
    test_logddp_device.py::test_cooperative_and_lane_sweeps_agree_bitwise does for the older plants: one sweep and the whole solve."""
    monkeypatch.delenv("CDDP_HIP_SWEEP", raising=False)
    a = _run_forms(api, case, True)
    monkeypatch.setenv("CDDP_HIP_SWEEP", "lane")
    _assert_forms_equal(a, _run_forms(api, case, True), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.cases(solvers=("clddp", "ipddp"), box=False))
def test_unconstrained_cooperative_and_lane_sweeps_agree_bitwise(api, case, monkeypatch):
    """Without path rows CLDDP and IPDDP have two sweeps as well: k_backward_coop_plain<Model, CLDDP> is what a handle runs, and
    CDDP_HIP_SWEEP=lane (and, for IPDDP, full DDP) selects the fused one-lane k_backward_clddp / k_backward_ipddp.  The comparisons
    against the twin above see the cooperative form only; this holds the one-lane form of these 13 models to it, bit for bit, as
    test_gpu_parity.py::test_cooperative_and_lane_sweeps_agree_bitwise does for the layouts of the older plants."""
    monkeypatch.delenv("CDDP_HIP_SWEEP", raising=False)
    a = _run_forms(api, case, True)
    monkeypatch.setenv("CDDP_HIP_SWEEP", "lane")
    _assert_forms_equal(a, _run_forms(api, case, True), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.cases(new_only=False, solvers=("logddp",), nx_max=8))
def test_logddp_pair_and_one_wave_rollouts_agree_bitwise(api, case, monkeypatch):
    """k_forward_logddp_pc against the one-wave rollout (CDDP_HIP_LG_ROLLOUT=lane), under both ladder shapes, as
    test_logddp_device.py::test_two_role_rollout_agrees_bitwise."""
    _rollout_forms(api, case, monkeypatch, "CDDP_HIP_LG_ROLLOUT")


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.cases(new_only=False, solvers=("msipddp",)))
def test_msipddp_pair_and_one_wave_rollouts_agree_bitwise(api, case, monkeypatch):
    """k_forward_msipddp_pc with k_rows_msipddp against the one-wave rollout (CDDP_HIP_MS_ROLLOUT=lane), under both ladder shapes, as
    test_msipddp_device.py::test_two_role_rollout_agrees_bitwise: all 16 MSIPDDP sets."""
    _rollout_forms(api, case, monkeypatch, "CDDP_HIP_MS_ROLLOUT")


def _rollout_forms(api, case, monkeypatch, switch):
    out = {}
    for mode in ("lane", "pc"):
        for stages in ("1", "2"):
            if mode == "lane": monkeypatch.setenv(switch, "lane")
            else: monkeypatch.delenv(switch, raising=False)
            monkeypatch.setenv("CDDP_HIP_LS_STAGES", stages)
            out[mode, stages] = _run_forms(api, case, False)
    for key, o in out.items():
        _assert_forms_equal(out["lane", "1"], o, (case,) + key)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM.cases(new_only=False, solvers=("msipddp",), box=True))
def test_msipddp_split_and_fused_sweeps_agree_bitwise(api, case, monkeypatch):
    """k_ms_condense -> k_backward_msipddp_lean -> k_ms_post against the fused one-lane sweep (CDDP_HIP_SWEEP=lane) for the Dubins car, the
    Dreyfus rocket and the acrobot with their box, as test_msipddp_device.py::test_split_and_fused_sweeps_agree_bitwise."""
    monkeypatch.delenv("CDDP_HIP_SWEEP", raising=False)
    a = _run_forms(api, case, True)
    monkeypatch.setenv("CDDP_HIP_SWEEP", "lane")
    _assert_forms_equal(a, _run_forms(api, case, True), case)
