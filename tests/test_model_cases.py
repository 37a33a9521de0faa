"""The tables of tests/model_cases.py held to the sources: every model of PLANT_MODEL_LIST has a row, every pair of SENS_PAIR_LIST a model,
every registered kernel set with a constraint a scoring case -- so the next model, pair or set added without a case fails HERE, on the CPU --
and the inputs those cases draw satisfy, on host references alone, what the GPU modules rely on (tests/test_score_every_model.py,
test_mppi_every_model.py, test_plan_sens_shapes.py): every reference finite on every lane, every constrained case with candidates on both
sides of its rows, the plant's box clipping some entries and not others."""
import numpy as np

import model_cases as MC
from test_score_rollouts import objective_numpy, viol_reference


def test_tables_are_the_compiled_lists(api):
    # 1. the model table is PLANT_MODEL_LIST
    compiled = MC.plant_model_list()
    assert len(compiled) == 25 and len(set(compiled)) == 25, compiled
    assert sorted(MC.MODELS) == sorted(compiled), (set(compiled) ^ set(MC.MODELS))
    assert len(set(MC.MODEL_KEYS)) == len(MC.MODELS)
    # 2. the sensitivity cases are SENS_PAIR_LIST, and each names a model of that shape
    pairs = MC.sens_pair_list()
    assert len(pairs) == 16 and len(set(pairs)) == 16, pairs
    assert sorted(MC.SENS_MODELS) == sorted(pairs), (set(pairs) ^ set(MC.SENS_MODELS))
    for pair in pairs:
        p, spread = MC.sens_problem(api, pair)
        assert (p.nx, p.nu) == pair and len(spread) == p.nx and p.N == MC.SENS_N and p.c.solver == api.SOLVER_IPDDP
        assert any(c.kind == api.CON_CONTROL_BOX for c in p._cons), pair
    # every pair is a model's shape, and every model's shape is a pair
    shapes = set()
    for name, row in MC.MODELS.items():
        p = MC.build_row(api, row)
        shapes.add((p.nx, p.nu))
        assert p.c.solver == api.SOLVER_IPDDP and p.N == MC.horizon(p.nx) and len(row.spread) == p.nx, name
        assert MC.set_of(api, p) == "%s/ctrlbox" % row.key, name
    assert shapes == set(pairs)
    # 3. every registered set with a constraint part is scored by a case that resolves to it
    registered = MC.registered_sets()
    assert len(registered) == len(set(registered)) and len(registered) > 60
    constrained = [s for s in registered if s.split("/")[1] != "none"]
    assert sorted(constrained) == sorted(MC.SET_CASES), (set(constrained) ^ set(MC.SET_CASES))
    for name in MC.SET_NAMES:
        assert MC.set_of(api, MC.set_case(api, name)[0]) == name, name
    # (the sets without a constraint part are the models' own, scored through their control-box rows' model kernel)
    assert {s.split("/")[0] for s in registered} == {s.split("/")[0] for s in constrained}


def test_mpc_tables_are_the_compiled_lists(api):
    """tests/test_mpc_every_model.py: its model cases are PLANT_MODEL_LIST, its T4 cases the models with nx > 8, its constrained cases every
    scoring case but the named sets without path duals, its other-solver cases `compare` rows of plant_matrix.MATRIX"""
    import plant_matrix as PM
    import test_mpc_every_model as E
    nx = {row.key: MC.build_row(api, row).nx for row in MC.MODELS.values()}
    default = [key for key, layout in E.MODEL_CASES if layout == "default"]
    assert sorted(MC.KEYS[key] for key in default) == sorted(MC.plant_model_list()) and len(default) == 25
    assert sorted(key for key, layout in E.MODEL_CASES if layout == "t4=0") == sorted(E.T4_KEYS) == sorted(k for k in nx if nx[k] > 8)
    assert {layout for _, layout in E.MODEL_CASES} == {"default", "t4=0"} and len(set(E.MODEL_CASES)) == len(E.MODEL_CASES) == 25 + len(E.T4_KEYS)
    # the constrained cases: SET_NAMES minus the refused names, and the refused names are exactly the sets without path duals
    assert sorted(E.SET_CASES + E.REFUSED_SETS) == sorted(MC.SET_NAMES) and not set(E.SET_CASES) & set(E.REFUSED_SETS)
    for name in MC.SET_NAMES:
        p = MC.set_case(api, name)[0]
        assert p.c.solver == api.SOLVER_IPDDP and (p.dual_dim() == 0) == (name in E.REFUSED_SETS), name
    # two tile groups: a model of 10 states and manip7
    assert len(E.GROUP_KEYS) == 2 and "manip7" in E.GROUP_KEYS and sorted(nx[k] for k in E.GROUP_KEYS) == [10, 14] and E.GROUP_B > 128
    # the other resident solvers: `compare` rows, per solver one plant with nx <= 8 and one with nx = 10
    sizes = {}
    for case in E.SOLVER_CASES:
        plant, box, solver = PM.parse(case)
        assert PM.mode_of(case) == PM.C, case
        sizes.setdefault(solver, []).append(PM.PLANTS[plant][0])
        assert solver != "msipddp" or not box, case
    assert sorted(sizes) == ["clddp", "logddp", "msipddp"]
    for solver, ns in sizes.items():
        assert len(ns) == 2 and min(ns) <= 8 and max(ns) == 10, (solver, ns)
    # the rows that must show two live slots in one advance: one on each side of nx = 8; the raised rows are models
    assert any(nx[k] <= 8 for k in E.MIXED_SLOT_KEYS) and any(nx[k] > 8 for k in E.MIXED_SLOT_KEYS)
    assert set(E.RAISED) <= set(MC.MODEL_KEYS) and all(set(v) <= {"spread", "max_iterations"} for v in E.RAISED.values())


def test_inputs_meet_the_conditions_on_host_references(api):
    """4. on the CPU, no device: the builder's problem, x0 and U of every row and every constrained case"""
    lo_all, hi_all = np.inf, -np.inf
    for name in MC.SET_NAMES:
        p, x0, U = MC.set_case(api, name)
        assert x0.shape == (MC.B, p.nx) and U.shape == (MC.B, MC.S, p.N, p.nu), name
        X = MC.rollout_host(api, p, x0, U)
        cost = objective_numpy(p, X, U)
        assert np.isfinite(X).all() and np.isfinite(cost).all(), name            # every lane: nothing is masked anywhere
        if name in MC.PROBE_SETS:
            continue                                                              # rows with a square root: the device probe is their reference
        viol, lo, hi = viol_reference(api, p, X, U)
        print("%-32s rows in [%.3g, %.3g]; viol > 0 on %d of %d" % (name, lo, hi, int((viol > 0).sum()), viol.size))
        assert np.isfinite(viol).all(), name
        assert (viol > 0).any() and (viol == 0).any(), name                       # both outcomes among the candidates
        assert lo < 0 < hi, name                                                  # both signs among the rows
        lo_all, hi_all = min(lo_all, lo), max(hi_all, hi)
    assert lo_all < 0 < hi_all
    for name, row in MC.MODELS.items():
        p, x0, U, centre, scale = MC.model_case(api, row.key)
        lo, up = MC.control_box(api, p)
        assert len(set(np.round(scale / (0.5 * (up - lo)), 12))) == p.nu, name   # no two controls in the same ratio to their box
        plo, pup = MC.plant_box(api, p)
        assert (plo > lo).all() and (pup < up).all() and (plo < pup).all(), name  # strictly inside the problem's box
        Usat = np.minimum(np.maximum(U, plo), pup)
        assert (Usat != U).any() and (Usat == U).any(), name                      # the plant's box clips some entries and leaves others
        for i in range(p.nu):
            assert (Usat[..., i] != U[..., i]).any() and (Usat[..., i] == U[..., i]).any(), (name, i)   # ... on every control
        X = MC.rollout_host(api, p, x0, Usat)
        assert np.isfinite(X).all() and np.isfinite(objective_numpy(p, X, Usat)).all(), name
        params = MC.plant_params(row, p, 3)
        if row.per_traj and row.nparams:
            base = np.array(list(p.c.model_params)[:row.nparams])
            f = params[:, base != 0] / base[base != 0]
            assert (f >= 0.9).all() and (f <= 1.1).all() and len(np.unique(params, axis=0)) == MC.B, name
            if row.inertia:
                for b in (0, 1, MC.B - 1):
                    M = params[b].reshape(3, 3)
                    assert np.array_equal(M, M.T) and (np.linalg.eigvalsh(M) > 0).all(), name

