"""Golden vectors of the spacecraft plants from the numpy twin -- run in the build container only:

    python tests/golden/make_spacecraft_golden.py [case ...]     # writes tests/golden/spacecraft/<case>.json

The plants are tests/golden/spacecraft_twin.py (numpy restatements of the reference sources); the solver is the numpy twin of the
reference path (oracle/twin/cddp_twin.py).  The problems restate cddp-cpp_amd/pyapi.py's attitude_problem / twobody_problem /
landing2d_problem as plain dictionaries.  The fixtures live in a subdirectory so that the globs of tests/test_golden.py
(golden/*.json) and tests/test_twin_golden.py (golden/twin_*.json) do not pick them up.
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_twin_golden as G  # noqa: E402  (run_case, and the twin as G.T)
import spacecraft_twin as P  # noqa: E402

OUT = os.path.join(HERE, "spacecraft")
INERTIA = [[1.0, 0.1, 0.0], [0.1, 1.5, 0.05], [0.0, 0.05, 2.0]]
LANDING = (100000.0, 50.0, 10.0, 880000.0, 2210000.0, 0.349066)


def _attitude_x0(kind):
    y, p_, r = 0.3, -0.2, 0.4
    cy, sy, cp, sp, cr, sr = math.cos(y / 2), math.sin(y / 2), math.cos(p_ / 2), math.sin(p_ / 2), math.cos(r / 2), math.sin(r / 2)
    q = [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]
    att = {"euler": [y, p_, r], "quaternion": q, "mrp": [v / (1.0 + q[0]) for v in q[1:]]}[kind]
    return att + [0.0, 0.0, 0.0]


def attitude(kind, solver, box=True, N=60, integrator="rk4", **opt):
    model = {"euler": P.EulerAttitude, "quaternion": P.QuaternionAttitude, "mrp": P.MrpAttitude}[kind](INERTIA)
    nx = model.nx
    o = dict(max_iterations=60, tolerance=1e-5, acceptable_tolerance=1e-6); o.update(opt)
    goal = [0.0] * nx
    if kind == "quaternion":
        goal[0] = 1.0
    return dict(solver=solver, model=model, integrator=integrator, dt=0.1, N=N, Q=np.zeros((nx, nx)), R=0.1 * np.eye(3),
                Qf=np.diag([100.0] * (nx - 3) + [10.0] * 3), xref=goal,
                constraints={"ControlConstraint": G.T.ControlBox([-1.0] * 3, [1.0] * 3)} if box else {}, options=o, x0=_attitude_x0(kind))


def twobody(solver, box=True, N=60, integrator="euler", **opt):
    o = dict(max_iterations=40, tolerance=1e-5, acceptable_tolerance=1e-6); o.update(opt)
    T = N * 0.05
    return dict(solver=solver, model=P.SpacecraftTwobody(1.0, 1.0), integrator=integrator, dt=0.05, N=N, Q=np.zeros((6, 6)), R=np.eye(3),
                Qf=100.0 * np.eye(6), xref=[math.cos(T), math.sin(T), 0.0, -math.sin(T), math.cos(T), 0.0],
                constraints={"ControlConstraint": G.T.ControlBox([-0.2] * 3, [0.2] * 3)} if box else {}, options=o,
                x0=[1.02, -0.01, 0.01, 0.0, 0.98, 0.02])


def landing2d(solver, box=True, N=80, integrator="rk4", **opt):
    o = dict(max_iterations=60, tolerance=1e-4, acceptable_tolerance=1e-6); o.update(opt)
    mass, _, _, tmin, tmax, gmax = LANDING
    return dict(solver=solver, model=P.SpacecraftLanding2D(*LANDING), integrator=integrator, dt=0.1, N=N, Q=np.zeros((6, 6)),
                R=np.diag([1.0, 1.0]), Qf=np.diag([1e-2, 1e-1, 1e-2, 1e-1, 10.0, 10.0]), xref=[0.0] * 6,
                constraints={"ControlConstraint": G.T.ControlBox([tmin / tmax, -gmax], [1.0, gmax])} if box else {}, options=o,
                x0=[20.0, -2.0, 150.0, -15.0, 0.05, 0.0], U0=np.tile([9.81 * mass / tmax, 0.0], (N, 1)))


CASES = {}
for _k in ("euler", "quaternion", "mrp"):
    for _s in ("CLDDP", "IPDDP"):
        CASES["%s_%s_box" % (_k, _s.lower())] = (lambda k=_k, s=_s: attitude(k, s))
for _s in ("CLDDP", "IPDDP"):
    CASES["twobody_%s_box" % _s.lower()] = (lambda s=_s: twobody(s))
    CASES["landing2d_%s_box" % _s.lower()] = (lambda s=_s: landing2d(s))


def run_case(name, with_solve=True):
    G.CASES[name] = CASES[name]     # make_twin_golden.run_case reads its own table
    return G.run_case(name, with_solve)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for name in sys.argv[1:] or list(CASES):
        o = run_case(name)
        with open(os.path.join(OUT, "%s.json" % name), "w") as f:
            json.dump(o, f)
        print(name, "sweep ok", o["sweep"]["ok"], "trials", [t["success"] for t in o["trials"]][:4], "solve", o["solve"]["iterations"],
              G.T.STATUS[o["solve"]["status"]], o["solve"]["final_objective"], flush=True)
