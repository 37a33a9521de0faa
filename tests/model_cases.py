"""Helper of tests/test_model_cases.py, test_score_every_model.py, test_mppi_every_model.py, test_plan_sens_shapes.py and test_mpc_every_model.py: one row per model
struct of PLANT_MODEL_LIST (csrc/plant_models.hpp: what k_score and k_mppi_score are instantiated over), one model per pair of
SENS_PAIR_LIST (csrc/inst_sens.hip: what k_plan_jvp / k_plan_vjp are instantiated over), and one scoring case per registered kernel set
that carries a constraint.  Both lists are parsed from the sources, and tests/test_model_cases.py holds the tables to them: a model or a
pair added without a case fails there.  Nothing here is imported by the product, and nothing here touches a device."""
import os
import re

import numpy as np

import plant_matrix as PM
from test_score_rollouts import PROBLEMS as SCORE_PROBLEMS, case as score_case

CSRC = PM.CSRC
B, S = 70, 3                # a full tile and a ragged one; B * S = 210: the last wavefront holds 18 live lanes


def horizon(nx):
    """N = 5 (N * nu odd where nu is: the last Box-Muller pair is half used), N = 3 for the plants at the register limit"""
    return 3 if nx >= 12 else 5


# ---------------------------------------------------------------------------------------------------------------- the parsed lists
def plant_model_list():
    """The names in PLANT_MODEL_LIST of csrc/plant_models.hpp, in order."""
    with open(os.path.join(CSRC, "plant_models.hpp")) as fh:
        text = fh.read()
    m = re.search(r"#define\s+PLANT_MODEL_LIST\(Y\)((?:[^\n]*\\\n)*[^\n]*)", text)
    return re.findall(r"Y\((\w+)\)", m.group(1))


def sens_pair_list():
    """The (nx, nu) pairs in SENS_PAIR_LIST of csrc/inst_sens.hip, in order."""
    with open(os.path.join(CSRC, "inst_sens.hip")) as fh:
        text = fh.read()
    m = re.search(r"#define\s+SENS_PAIR_LIST\(Y\)((?:[^\n]*\\\n)*[^\n]*)", text)
    return [(int(a), int(b)) for a, b in re.findall(r"Y\((\d+),\s*(\d+)\)", m.group(1))]


def registered_sets():
    """Every Launcher<...>::set("...") name of every csrc/inst_*.hip."""
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.startswith("inst_") and f.endswith(".hip"))
    return PM.registered_sets(files)


_PREFIX = {0: "pendulum", 1: "cartpole", 2: "unicycle", 4: "quadrotor13", 5: "manipulator3", 6: "quad12", 7: "manip7", 8: "bicycle", 9: "car",
           10: "hcw", 11: "euler_attitude", 12: "quaternion_attitude", 13: "mrp_attitude", 14: "twobody", 15: "landing2d", 16: "dubins_car",
           17: "dreyfus_rocket", 18: "acrobot", 19: "usv_3dof", 20: "forklift", 21: "quadrotor_rate", 22: "linear_fuel", 23: "spacecraft_nonlinear"}


def set_of(api, p):
    """The kernel-set name a problem descriptor resolves to: the model's prefix, the constraint objects in name order (as std::map
    iterates them), "+terminal" with any terminal constraint."""
    kinds = {api.CON_CONTROL_BOX: "ctrlbox", api.CON_STATE_BOX: "statebox", api.CON_BALL: "ball", api.CON_LINEAR: "linear", api.CON_SOC: "soc",
             api.CON_THRUST: "thrust", api.CON_MAX_THRUST: "maxthrust"}
    prefix = "lti%dx%d" % (p.nx, p.nu) if p.c.model == api.MODEL_LTI else _PREFIX[p.c.model]
    part = "+".join(kinds[c.kind] for c in sorted(p._cons, key=lambda c: c.name)) or "none"
    return "%s/%s%s" % (prefix, part, "+terminal" if p._terms else "")


# ---------------------------------------------------------------------------------------------------------------- the model table
def _lti21(api, N):
    """the 2 x 1 problem of test_plan_sens.lti_problem on IPDDP with a control box of this table's own"""
    from test_plan_sens import lti_problem
    p = lti_problem(api, N, 3)
    p.c.solver = api.SOLVER_IPDDP
    p.add_control_box("ControlConstraint", [-0.6], [0.4])
    return p


def _matrix(name):
    return lambda api, N: PM.PLANTS[name][2](api, api.SOLVER_IPDDP, True, N)


class Row:
    """key: the short name the test ids carry; build(api, N) -> Problem (IPDDP, control box); spread: of x0 around p.x0; nparams: the
    caller-visible entries of the parameter block; inertia: the block is a 3 x 3 inertia matrix (scaled as a whole: it stays symmetric
    positive definite); discrete: a discrete plant (substeps = 1 is the only choice); per_traj: whether the plant takes a block per
    trajectory (an LTI plant's matrices are shared by the batch)"""

    def __init__(self, key, build, spread, nparams=0, inertia=False, discrete=False, per_traj=True):
        self.key, self.build, self.spread, self.nparams, self.inertia, self.discrete, self.per_traj = key, build, spread, nparams, inertia, discrete, per_traj


def _pm(name, nparams, **kw):
    return Row(name, _matrix(name), PM.PLANTS[name][4], nparams, **kw)


# Spreads: ids 11-23 from plant_matrix.PLANTS (two-body radius within 1 +- 0.03, fuel mass 1 +- 0.01, Euler pitch -0.2 +- 0.05, quaternion
# norm within 1 +- 0.1: the working ranges tests/plant_probe.py documents); the others from tests/test_score_rollouts.py and
# test_plan_sens.py, or a tenth of plant_probe's regular range around the builder's x0.
MODELS = {
    "PendulumModel": Row("pendulum", lambda api, N: api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=N), [0.2, 0.3], 4),
    "CartPoleModel": Row("cartpole", lambda api, N: api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N), [0.1, 0.3, 0.1, 0.1], 5),
    "UnicycleModel": Row("unicycle", lambda api, N: api.unicycle_problem(api.SOLVER_IPDDP, horizon=N, obstacle=False), [0.3, 0.3, 0.4], 0),
    "QuadrotorModel": Row("quadrotor13", lambda api, N: api.quadrotor_problem(api.SOLVER_IPDDP, N, True), [0.02] * 13, 6),
    "ManipulatorModel": Row("manipulator3", lambda api, N: api.manipulator_problem(api.SOLVER_IPDDP, horizon=N), [0.1] * 6, 0),
    "Quad12Model": Row("quad12", lambda api, N: api.quadrotor12_problem(api.SOLVER_IPDDP, horizon=N), [0.1] * 12, 6),
    "Manip7Model": Row("manip7", lambda api, N: api.manipulator7_problem(api.SOLVER_IPDDP, horizon=N, terminal_equality=False), [0.1] * 14, 0),
    "BicycleModel": Row("bicycle", lambda api, N: api.bicycle_problem(api.SOLVER_IPDDP, horizon=N), [0.1, 0.1, 0.1, 0.1], 1),
    "CarModel": Row("car", lambda api, N: api.car_problem(api.SOLVER_IPDDP, horizon=N), [0.1, 0.1, 0.1, 0.1], 1, discrete=True),
    "HCWModel": Row("hcw", lambda api, N: api.hcw_problem(api.SOLVER_IPDDP, horizon=N), [0.5, 0.5, 0.5, 0.002, 0.002, 0.002], 2),
    "EulerAttitudeModel": _pm("euler_attitude", 9, inertia=True),
    "QuaternionAttitudeModel": _pm("quaternion_attitude", 9, inertia=True),
    "MrpAttitudeModel": _pm("mrp_attitude", 9, inertia=True),
    "SpacecraftTwobodyModel": _pm("twobody", 2),
    "SpacecraftLanding2DModel": _pm("landing2d", 6),
    "DubinsCarModel": _pm("dubins_car", 1),
    "DreyfusRocketModel": _pm("dreyfus_rocket", 2),
    "AcrobotModel": _pm("acrobot", 6),
    "Usv3DofModel": _pm("usv_3dof", 0),
    "ForkliftModel": _pm("forklift", 3, discrete=True),
    "QuadrotorRateModel": _pm("quadrotor_rate", 3),
    "SpacecraftLinearFuelModel": _pm("linear_fuel", 3),
    "SpacecraftNonlinearModel": _pm("spacecraft_nonlinear", 4),
    "Lti11": Row("lti1x1", lambda api, N: api.scalar_integrator_problem(horizon=N, path_constraint=True, solver=api.SOLVER_IPDDP), [0.3], 0, discrete=True, per_traj=False),
    "Lti21": Row("lti2x1", _lti21, [0.3, 0.3], 0, discrete=True, per_traj=False),
}
KEYS = {r.key: name for name, r in MODELS.items()}
MODEL_KEYS = [r.key for r in MODELS.values()]


def control_box(api, p):
    """(lower, upper) of the problem's control box"""
    c = [c for c in p._cons if c.kind == api.CON_CONTROL_BOX][0]
    return np.array([c.lower[i] for i in range(c.dim)]), np.array([c.upper[i] for i in range(c.dim)])


def candidate_scale(api, p):
    """-> (centre (nu,), scale (nu,)): 0.75 of the half-width of control i times 1 + 0.25 i -- a vector with no two entries in the same
    ratio to their box, so that an index into sigma or the box that is off by one control shows; centred on U0_const where the builder
    has one, on the box centre otherwise."""
    lo, up = control_box(api, p)
    half = 0.5 * (up - lo)
    centre = np.asarray(p.U0_const, dtype=np.float64) if hasattr(p, "U0_const") else 0.5 * (lo + up)
    return centre, 0.75 * half * (1.0 + 0.25 * np.arange(p.nu))


def draw(p, spread, centre, scale, seed, b=B, s=S):
    """x0 (b, nx) around p.x0 and U (b, s, N, nu) = centre + scale * z, candidate 0 a quarter of that (as test_score_rollouts.case)"""
    rng = np.random.default_rng(seed)
    x0 = p.x0[None, :] + np.asarray(spread)[None, :] * rng.uniform(-1.0, 1.0, (b, p.nx))
    z = rng.standard_normal((b, s, p.N, p.nu))
    z[:, 0] *= 0.25
    return np.ascontiguousarray(x0), np.ascontiguousarray(centre + scale * z)


def model_case(api, key, seed=7, N=None):
    """-> problem, x0 (B, nx), U (B, S, N, nu), centre, scale of the model's row"""
    row = MODELS[KEYS[key]]
    p = build_row(api, row, N)
    centre, scale = candidate_scale(api, p)
    x0, U = draw(p, row.spread, centre, scale, seed)
    return p, x0, U, centre, scale


def build_row(api, row, N=None):
    """the row's problem on the horizon of its size (or on N)"""
    p = row.build(api, N or 5)
    return p if N or horizon(p.nx) == 5 else row.build(api, horizon(p.nx))


def staged(p):
    """Objective<NX, NU>::kHoist is false: Q dt | R dt | x_ref are staged in LDS"""
    return p.nx * p.nx + p.nu * p.nu + p.nx > 40


def plant_box(api, p):
    """A box strictly inside the problem's: 0.3 of the half-width in from below, 0.2 from above"""
    lo, up = control_box(api, p)
    half = 0.5 * (up - lo)
    return lo + 0.3 * half, up - 0.2 * half


def plant_params(row, p, seed, b=B):
    """(b, nparams): every caller-visible entry of the block scaled by a factor of its own in [0.9, 1.1]; an inertia matrix by one factor
    per trajectory.  None for a plant whose block is shared; a plant without caller-visible entries gets one all-zero column: b equal
    blocks, which the library fills (the surface vessel's 21 derived entries) and the kernels read at a per-trajectory stride."""
    if not row.per_traj:
        return None
    if row.nparams == 0:
        return np.zeros((b, 1))
    rng = np.random.default_rng(seed)
    base = np.array(list(p.c.model_params)[:row.nparams])
    f = rng.uniform(0.9, 1.1, (b, 1)) if row.inertia else rng.uniform(0.9, 1.1, (b, row.nparams))
    return np.ascontiguousarray(base[None, :] * f)


# ---------------------------------------------------------------------------------------------------------------- constrained sets
# One scoring case per registered set with a constraint part.  "own": the model's row above (its control box).  "score": a case of
# tests/test_score_rollouts.py::PROBLEMS as it stands.  Otherwise build(api) -> (problem, spread, scale override or None).
# The three builders with a `...+terminal` set offer a terminal EQUALITY only; scoring folds terminal inequality rows alone
# (term_ineq_eval), so these cases add an inequality of their own through add_terminal_inequality: the kernel set is the same one, and a
# set reached through the equality would be covered by its control box rows only.
def _with_statebox(key, lower, upper):
    def build(api):
        row = MODELS[KEYS[key]]
        p = row.build(api, 5)
        for c in p._cons:                              # the unicycle's box is "control_limits": under its reference name it sorts before
            c.name = b"ControlConstraint"              # "StateConstraint", as the set's constraint list has it ('S' < 'c')
        p._rebuild()
        p.add_state_box("StateConstraint", lower, upper)
        return p, row.spread
    return build


def _with_terminal(key, a_row, b):
    def build(api):
        row = MODELS[KEYS[key]]
        p = build_row(api, row)
        A = np.zeros((2, p.nx))
        A[0, :len(a_row)] = a_row                      # a row over the leading coordinates and one on the last coordinate alone
        A[1, p.nx - 1] = 1.0
        p.add_terminal_inequality("TerminalUpperBound", A, b)
        return p, row.spread
    return build


def _lti21_statebox(api):
    from test_plan_sens import lti_problem
    p = lti_problem(api, 5, 3)
    p.c.solver = api.SOLVER_IPDDP
    p.add_state_box("StateConstraint", [0.5, -1.4], [1.32, 0.0])
    return p, [0.3, 0.3]


def _lti11_terminal(linear):
    def build(api):
        p = api.scalar_integrator_problem(horizon=5, terminal_inequality=True, solver=api.SOLVER_IPDDP)
        if linear:
            p.add_linear("LinearConstraint", np.array([[1.0]]), np.array([0.25]))
        p.x0 = np.array([-0.2])
        return p, [0.3]
    return build


SET_CASES = {
    "pendulum/ctrlbox": "score:pendulum",
    "unicycle/ctrlbox+ball": "score:unicycle_box_ball",
    "pendulum/ctrlbox+statebox": "score:pendulum_statebox",
    "lti1x1/linear": "score:lti_linear",
    "lti1x1/ctrlbox+terminal": "score:lti_terminal_ineq",
    "unicycle/ctrlbox+soc": "score:unicycle_cone",
    "unicycle/thrust": "score:unicycle_thrust2",
    "unicycle/maxthrust": "score:unicycle_thrust1",
    "cartpole/ctrlbox+statebox": _with_statebox("cartpole", [-0.15, -0.5, -0.6, -1.5], [0.15, 0.5, 0.6, 1.5]),
    "unicycle/ctrlbox+statebox": _with_statebox("unicycle", [-0.2, -0.2, 0.5], [0.25, 0.25, 1.1]),
    "lti2x1/statebox": _lti21_statebox,
    "lti1x1/none+terminal": _lti11_terminal(False),
    "lti1x1/linear+terminal": _lti11_terminal(True),
    "pendulum/ctrlbox+terminal": _with_terminal("pendulum", [1.0, 0.2], [3.2, 0.0]),
    "manipulator3/ctrlbox+terminal": _with_terminal("manipulator3", [1.0, -1.0, 0.5], [3.1, 0.0]),
    "manip7/ctrlbox+terminal": _with_terminal("manip7", [1.0, -1.0, 0.5, 0.0, 0.0, 0.0, 2.0], [0.0, 0.0]),
}
for _row in MODELS.values():
    SET_CASES.setdefault("%s/ctrlbox" % _row.key, "own:%s" % _row.key)
SET_NAMES = list(SET_CASES)
# kinds whose rows the numpy restatement does not hold (they take a square root: the device probe is their reference)
PROBE_SETS = ("unicycle/ctrlbox+soc", "unicycle/thrust", "unicycle/maxthrust")


def set_case(api, name, seed=7):
    """-> problem, x0 (B, nx), U (B, S, N, nu) of the scoring case of a registered set"""
    how = SET_CASES[name]
    if isinstance(how, str) and how.startswith("score:"):
        assert SCORE_PROBLEMS[how[6:]][3:] == (B, S)
        return score_case(api, how[6:], seed=seed)
    if isinstance(how, str):
        return model_case(api, how[4:], seed=seed)[:3]
    p, spread = how(api)
    if any(c.kind == api.CON_CONTROL_BOX for c in p._cons):
        centre, scale = candidate_scale(api, p)
    else:                                               # no control box: the scale of the scalar-integrator cases of test_score_rollouts.py
        centre, scale = np.zeros(p.nu), 0.4 * (1.0 + 0.25 * np.arange(p.nu))
    x0, U = draw(p, spread, centre, scale, seed)
    return p, x0, U


# ---------------------------------------------------------------------------------------------------------------- sensitivity pairs
SENS_MODELS = {(1, 1): "lti1x1", (2, 1): "dreyfus_rocket", (3, 1): "dubins_car", (3, 2): "unicycle", (4, 1): "acrobot", (4, 2): "bicycle",
               (5, 2): "forklift", (6, 2): "landing2d", (6, 3): "hcw", (7, 3): "quaternion_attitude", (8, 3): "linear_fuel",
               (10, 3): "spacecraft_nonlinear", (10, 4): "quadrotor_rate", (12, 4): "quad12", (13, 4): "quadrotor13", (14, 7): "manip7"}
SENS_N = 4


def sens_problem(api, pair):
    """IPDDP with the control box, N = 4, two iterations (so that the gains are not those of a zero plan)"""
    row = MODELS[KEYS[SENS_MODELS[pair]]]
    p = row.build(api, SENS_N)
    p.options.max_iterations = 2
    assert (p.nx, p.nu) == pair
    return p, row.spread


# ---------------------------------------------------------------------------------------------------------------- CPU references
def rollout_host(api, p, x0, U):
    """X (b, s, N + 1, nx) of the problem's own model on the host (cddp_hip_model_eval; numpy for the LTI plants): no device.  Serves the
    conditions on the inputs (finiteness, which rows are violated), not a bitwise comparison."""
    b, s, N, nu = U.shape
    X = np.zeros((b, s, N + 1, p.nx))
    X[:, :, 0] = x0[:, None, :]
    params = list(p.c.model_params)
    for t in range(N):
        if p.c.model == api.MODEL_LTI:
            X[:, :, t + 1] = X[:, :, t] @ p.lti_A.T + U[:, :, t] @ p.lti_B.T
            continue
        for i in range(b):
            for c in range(s):
                X[i, c, t + 1] = api.model_eval(p.c.model, p.c.integrator, p.dt, params, p.nx, p.nu, X[i, c, t], U[i, c, t])["step"]
    return X
