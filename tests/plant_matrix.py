"""Helper of tests/test_plant_solver_matrix.py: the thirteen newer plants (cddp_hip_model ids 11-23) as kernel sets x solvers, the problem
of every pair twice (the pyapi descriptor the library gets, the plain dictionary the numpy twins get: tests/golden/make_plants_golden.py
and make_spacecraft_golden.py), the batch of three distinct initial states, and the twins' step-level and whole-solve records,
memoised per case so that the tests of one case share them.  Nothing here is imported by the product."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(REPO, "oracle", "twin"))
import cddp_twin as T  # noqa: E402
import logddp_twin as L  # noqa: E402
import msipddp_twin as M  # noqa: E402
import make_plants_golden as MG  # noqa: E402
import make_spacecraft_golden as SG  # noqa: E402

CSRC = os.path.join(REPO, "cddp-cpp_amd", "csrc")
INST_FILES = ("inst_spacecraft.hip", "inst_plants_small.hip", "inst_plants_nx10.hip")
SOLVERS = ("clddp", "ipddp", "logddp", "msipddp")
C, F, R = "compare", "compare-first-iteration", "refused"

# Every (kernel set, solver) pair the three files register, once.  `refused`: MSIPDDP with a control box at nu != 1 (nx = nu occurs in
# none of these plants), which cddp_hip_create and the twin both refuse.  `compare-first-iteration`: see
# test_plant_solver_matrix.py::test_whole_solve_matches_the_twin.
MATRIX = {
    "euler_attitude/none":         dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "euler_attitude/ctrlbox":      dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "quaternion_attitude/none":    dict(clddp=C, ipddp=C, logddp=C, msipddp=F),
    "quaternion_attitude/ctrlbox": dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "mrp_attitude/none":           dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "mrp_attitude/ctrlbox":        dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "twobody/none":                dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "twobody/ctrlbox":             dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "landing2d/none":              dict(clddp=C, ipddp=C, logddp=C, msipddp=F),
    "landing2d/ctrlbox":           dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "dubins_car/none":             dict(clddp=C, ipddp=C, logddp=C, msipddp=F),
    "dubins_car/ctrlbox":          dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "dreyfus_rocket/none":         dict(clddp=C, ipddp=C, logddp=C, msipddp=F),
    "dreyfus_rocket/ctrlbox":      dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "acrobot/none":                dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "acrobot/ctrlbox":             dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "usv_3dof/none":               dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "usv_3dof/ctrlbox":            dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "forklift/none":               dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "forklift/ctrlbox":            dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "linear_fuel/none":            dict(clddp=C, ipddp=C, logddp=C, msipddp=F),
    "linear_fuel/ctrlbox":         dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "quadrotor_rate/none":         dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "quadrotor_rate/ctrlbox":      dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
    "spacecraft_nonlinear/none":   dict(clddp=C, ipddp=C, logddp=C, msipddp=C),
    "spacecraft_nonlinear/ctrlbox": dict(clddp=C, ipddp=C, logddp=C, msipddp=R),
}

# The 30 `compare` pairs other files already hold against the twin (at B = 1): not run again here.
ELSEWHERE = {(s, v): "test_hip_matches_twin" for s in MATRIX if s.endswith("/ctrlbox") for v in ("clddp", "ipddp")}
ELSEWHERE.update({("usv_3dof/ctrlbox", "logddp"): "test_remaining_plants.py::test_hip_logddp_solve_matches_its_twin",
                  ("mrp_attitude/ctrlbox", "logddp"): "test_spacecraft_plants.py::test_hip_logddp_solve_matches_its_twin",
                  ("dubins_car/ctrlbox", "msipddp"): "test_remaining_plants.py::test_hip_msipddp_solve_matches_its_twin",
                  ("mrp_attitude/none", "msipddp"): "test_spacecraft_plants.py::test_hip_msipddp_solve_matches_its_twin"})

# kernel-set prefix -> (nx, nu, pyapi builder, twin spec builder, perturbation of x0, horizon or None for the builders' own).
# The perturbations are the SPREAD tables of test_remaining_plants.py / test_spacecraft_plants.py.  A horizon is given where the twin's
# solve on the builder's own horizon takes more than about 2 s; the two builders of a plant get the same one.
_ATT = lambda kind: (lambda api, s, box, N: api.attitude_problem(kind, s, horizon=N, constrained=box, integrator=api.RK4),
                     lambda s, box, N: SG.attitude(kind, s, box=box, N=N))
PLANTS = {
    "euler_attitude": (6, 3) + _ATT("euler") + ([0.05] * 6, None),
    "quaternion_attitude": (7, 3) + _ATT("quaternion") + ([0.05] * 7, 20),
    "mrp_attitude": (6, 3) + _ATT("mrp") + ([0.05] * 6, None),
    "twobody": (6, 3, lambda api, s, box, N: api.twobody_problem(s, horizon=N, constrained=box),
                lambda s, box, N: SG.twobody(s, box=box, N=N), [0.005] * 6, None),
    "landing2d": (6, 2, lambda api, s, box, N: api.landing2d_problem(s, horizon=N, constrained=box),
                  lambda s, box, N: SG.landing2d(s, box=box, N=N), [2.0, 0.2, 5.0, 0.5, 0.02, 0.01], 12),
    "dubins_car": (3, 1, lambda api, s, box, N: api.dubins_problem(s, horizon=N, constrained=box),
                   lambda s, box, N: MG.dubins(s, box=box, N=N), [0.05, 0.05, 0.02], None),
    "dreyfus_rocket": (2, 1, lambda api, s, box, N: api.dreyfus_problem(s, horizon=N, constrained=box),
                       lambda s, box, N: MG.dreyfus(s, box=box, N=N), [0.02, 0.05], None),
    "acrobot": (4, 1, lambda api, s, box, N: api.acrobot_problem(s, horizon=N, constrained=box),
                lambda s, box, N: MG.acrobot(s, box=box, N=N), [0.02] * 4, None),
    "usv_3dof": (6, 3, lambda api, s, box, N: api.usv_problem(s, horizon=N, constrained=box),
                 lambda s, box, N: MG.usv(s, box=box, N=N), [0.05] * 6, None),
    "forklift": (5, 2, lambda api, s, box, N: api.forklift_problem(s, horizon=N, constrained=box),
                 lambda s, box, N: MG.forklift(s, box=box, N=N), [0.05, 0.05, 0.02, 0.02, 0.01], 60),
    "linear_fuel": (8, 3, lambda api, s, box, N: api.linear_fuel_problem(s, horizon=N, constrained=box),
                    lambda s, box, N: MG.linear_fuel(s, box=box, N=N), [0.5, 0.5, 0.5, 0.002, 0.002, 0.002, 0.01, 0.0], 16),
    "quadrotor_rate": (10, 4, lambda api, s, box, N: api.quadrotor_rate_problem(s, horizon=N, constrained=box),
                       lambda s, box, N: MG.quadrotor_rate(s, box=box, N=N), [0.05] * 6 + [0.0, 0.02, 0.02, 0.02], None),
    "spacecraft_nonlinear": (10, 3, lambda api, s, box, N: api.spacecraft_nonlinear_problem(s, horizon=N, constrained=box),
                             lambda s, box, N: MG.spacecraft_nonlinear(s, box=box, N=N), [0.002] * 6 + [0.0] * 4, None),
}
DEFAULT_HORIZON = {"euler_attitude": 60, "quaternion_attitude": 60, "mrp_attitude": 60, "twobody": 60, "landing2d": 80, "dubins_car": 60,
                   "dreyfus_rocket": 50, "acrobot": 80, "usv_3dof": 80, "forklift": 100, "linear_fuel": 80, "quadrotor_rate": 60,
                   "spacecraft_nonlinear": 40}

# The unconstrained forklift under MSIPDDP overflows in its stale-factor sweeps on the short horizon and stays finite on the builder's own.
HORIZON_OF_CASE = {"forklift_none-msipddp": 100}

B = 70              # one full 64-trajectory tile and a ragged one; every lane group of a 4-, 8- or 16-lane cooperative sweep is live
MEMBERS = 3         # distinct initial states, laid round-robin over the batch: position i holds member i % 3
SEED = 2            # of the two perturbed members; test_twin_counts_are_not_on_a_knife_edge holds it (change the seed, not the test)


def registered_sets(files=None):
    """The names in the Launcher<...>::set("...") lines of the three instantiation files."""
    import re
    out = []
    for f in files or [os.path.join(CSRC, n) for n in INST_FILES]:
        with open(f) as fh:
            out += re.findall(r'Launcher<[^;]*>::set\("([^"]+)"\)', fh.read())
    return out


def case_id(set_name, solver):
    return "%s-%s" % (set_name.replace("/", "_"), solver)


def cases(modes=(C, F), new_only=True, solvers=SOLVERS, nx_max=None, box=None):
    out = []
    for s, row in MATRIX.items():
        for v in solvers:
            if row[v] not in modes or (new_only and (s, v) in ELSEWHERE):
                continue
            if nx_max is not None and PLANTS[s.split("/")[0]][0] > nx_max:
                continue
            if box is not None and s.endswith("/ctrlbox") != box:
                continue
            out.append(case_id(s, v))
    return out


def parse(case):
    name, solver = case.rsplit("-", 1)
    plant, layout = name.rsplit("_", 1)
    return plant, layout == "ctrlbox", solver


def mode_of(case):
    plant, box, solver = parse(case)
    return MATRIX["%s/%s" % (plant, "ctrlbox" if box else "none")][solver]


def horizon(case):
    plant = parse(case)[0]
    return HORIZON_OF_CASE.get(case) or PLANTS[plant][5] or DEFAULT_HORIZON[plant]


def spec(case, N=None, **options):
    """The twin's problem: the golden builder's dictionary (a new one on every call)."""
    plant, box, solver = parse(case)
    sp = PLANTS[plant][3]({"clddp": "CLDDP"}.get(solver, "IPDDP"), box, N or horizon(case))
    if solver == "msipddp":
        sp["options"].update(ms_rollout_type="nonlinear", ms_segment_length=5, warm_start=False)
    sp["options"].update(options)
    return sp


def problem(api, case, N=None, **options):
    """The library's problem: the pyapi descriptor."""
    plant, box, solver = parse(case)
    s = {"clddp": api.SOLVER_CLDDP, "ipddp": api.SOLVER_IPDDP, "logddp": api.SOLVER_LOGDDP, "msipddp": api.SOLVER_MSIPDDP}[solver]
    p = PLANTS[plant][2](api, s, box, N or horizon(case))
    if solver == "msipddp":
        p.options.msipddp_segment_length = 5; p.options.msipddp_rollout_type = 0; p.options.warm_start = 0
    for k, v in options.items():
        setattr(p.options, k, v)
    return p


def members(case):
    """(3, nx): the builder's x0 and two seeded perturbations of it."""
    plant = parse(case)[0]
    x0 = np.array(spec(case)["x0"], float)
    rng = np.random.default_rng(SEED)
    pert = rng.uniform(-1.0, 1.0, size=(MEMBERS - 1, x0.size)) * np.asarray(PLANTS[plant][4])[None, :]
    return np.vstack([x0[None, :], x0[None, :] + pert])


def batch(case):
    """(B, nx) initial states and the positions of every member."""
    x0 = members(case)[np.arange(B) % MEMBERS]
    return np.ascontiguousarray(x0), [np.arange(m, B, MEMBERS) for m in range(MEMBERS)]


# ---------------------------------------------------------------------------------------------------------------- the twins
def _new_twin(case, x0, N=None, **options):
    sp = spec(case, N, **options)
    solver = parse(case)[2]
    U0 = sp.get("U0")
    if solver == "logddp":
        tw = L.LogDDP(sp); tw.set_initial(x0, U0)
    elif solver == "msipddp":
        tw = M.MSIPDDP(sp); tw.set_initial(np.array(x0, float), U0, None)
    else:
        tw = T.Twin(sp); tw.set_initial(np.array(x0, float), U0)
    return tw


def _sweep_with_retries(tw, solver):
    """What cddp_hip_backward does: the sweep, regularisation up after a failure, until it succeeds or the limit is reached."""
    o = tw.o
    while True:
        ok = tw.backward() if solver in ("clddp", "ipddp") else tw.backward_pass()
        if ok:
            return True
        tw.reg = min(tw.reg * o["reg_update_factor"], o["reg_max_value"])
        if tw.reg >= o["reg_max_value"]:
            return False


def twin_step(case, x0, N=None, **options):
    """initialize -> backward -> every line-search trial of one member."""
    solver = parse(case)[2]
    tw = _new_twin(case, x0, N, **options)
    tw.initialize()
    out = {"alphas": list(tw.alphas), "cost": tw.cost, "merit": tw.merit, "violation": getattr(tw, "inf_pr", None)}
    if solver in ("clddp", "ipddp"):
        tw.X_lin, tw.U_lin = tw.X, tw.U
    out["ok"] = _sweep_with_retries(tw, solver)
    out["reg"] = tw.reg
    if out["ok"]:
        if solver in ("clddp", "ipddp"):
            out.update(K=tw.K_u.copy(), k=tw.k_u.copy())
        else:
            out.update(K=tw.K.copy(), k=tw.k.copy())
        out.update(Vx=tw.Vx.copy(), Vxx=tw.Vxx.copy(), dV=np.array(tw.dV, float))
    trials = []
    for a in (tw.alphas if out["ok"] else []):
        if solver in ("clddp", "ipddp"):
            r = tw.forward(a)
            trials.append((bool(r["success"]), r["cost"], r["merit"]))
        else:
            r = tw.forward_pass(a)
            trials.append((r is not None, r["cost"] if r else math.nan, r["merit"] if r else math.nan))
    out["trials"] = trials
    return out


def twin_solve(case, x0, **options):
    solver = parse(case)[2]
    tw = _new_twin(case, x0, **options)
    r = tw.solve()
    status = r["status"] if isinstance(r["status"], str) else T.STATUS[r["status"]]
    return {"counts": (int(r["iterations"]), status, int(r["n_backward"]), int(r["n_forward"])), "final_objective": float(r["final_objective"]),
            "X": np.array(tw.X, float), "U": np.array(tw.U, float), "Lam": np.array(tw.Lam, float) if solver == "msipddp" else None}


def solve_options(case):
    """compare-first-iteration: one iteration, in which the twin's arithmetic is finite."""
    return {"max_iterations": 1} if mode_of(case) == F else {}


def twin_alphas(case):
    """The line-search ladder of the case's options (detail::buildLineSearchAlphas)."""
    return list(T.Twin(spec(case)).alphas)


# Full DDP (use_ilqr = 0) on LogDDP and MSIPDDP.  On the device the one-lane kernels carry the tensor terms for the plants with explicit
# Hessian tensors (Model::kHasHess); the plants whose device Hessians exist in the blocked dual form only are refused with a pointer to
# the plug-in route, the two plants without an autodiff expression with the reference's message.
DDP_HORIZON = 20    # test_remaining_plants.py::DDP_HORIZON: over the whole horizon the indefinite first sweep compares rounding
DDP_TENSORS = ("landing2d", "dubins_car", "dreyfus_rocket", "acrobot", "forklift", "linear_fuel")
DDP_BLOCKED = ("euler_attitude", "quaternion_attitude", "mrp_attitude", "usv_3dof", "quadrotor_rate")
DDP_NONE = ("twobody", "spacecraft_nonlinear")


def ddp_cases(plants):
    return [c for c in cases(new_only=False, solvers=("logddp", "msipddp")) if parse(c)[0] in plants]


_memo = {}


def twin_steps(case):
    key = ("step", case)
    if key not in _memo:
        _memo[key] = [twin_step(case, x) for x in members(case)]
    return _memo[key]


def twin_ddp_steps(case):
    key = ("ddp", case)
    if key not in _memo:
        _memo[key] = [twin_step(case, x, DDP_HORIZON, use_ilqr=False) for x in members(case)]
    return _memo[key]


def twin_solves(case):
    key = ("solve", case)
    if key not in _memo:
        _memo[key] = [twin_solve(case, x, **solve_options(case)) for x in members(case)]
    return _memo[key]
