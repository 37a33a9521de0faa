"""Golden vectors of the Dubins car, Dreyfus rocket, acrobot, surface vessel, forklift and fuel-state HCW plants from the numpy twin --
run in the build container only:

    python tests/golden/make_plants_golden.py [case ...]     # writes tests/golden/plants/<case>.json

The plants are tests/golden/plants_twin.py (numpy restatements of the reference sources); the solver is the numpy twin of the
reference path (oracle/twin/cddp_twin.py).  The problems restate cddp-cpp_amd/pyapi.py's dubins_problem / dreyfus_problem /
acrobot_problem / usv_problem / forklift_problem / linear_fuel_problem / quadrotor_rate_problem / spacecraft_nonlinear_problem as plain dictionaries.  The fixtures live in a subdirectory so
that the globs of tests/test_golden.py (golden/*.json) and tests/test_twin_golden.py (golden/twin_*.json) do not pick them up.
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_twin_golden as G  # noqa: E402  (run_case, and the twin as G.T)
import plants_twin as P  # noqa: E402

OUT = os.path.join(HERE, "plants")


def _box(lo, hi, box):
    return {"ControlConstraint": G.T.ControlBox(list(lo), list(hi))} if box else {}


def dubins(solver, box=True, N=60, integrator="euler", **opt):
    o = dict(max_iterations=60, tolerance=1e-5, acceptable_tolerance=1e-6); o.update(opt)
    return dict(solver=solver, model=P.DubinsCar(1.0), integrator=integrator, dt=0.1, N=N, Q=np.zeros((3, 3)), R=0.1 * np.eye(1),
                Qf=np.diag([100.0, 100.0, 50.0]), xref=[3.8, 3.8, math.pi / 2], constraints=_box([-1.0], [1.0], box), options=o,
                x0=[0.0, 0.0, 0.0], U0=np.tile([0.2], (N, 1)))


def dreyfus(solver, box=True, N=50, integrator="rk4", **opt):
    o = dict(max_iterations=60, tolerance=1e-5, acceptable_tolerance=1e-6); o.update(opt)
    return dict(solver=solver, model=P.DreyfusRocket(64.0, 32.0), integrator=integrator, dt=0.01, N=N, Q=np.zeros((2, 2)), R=0.1 * np.eye(1),
                Qf=np.diag([100.0, 10.0]), xref=[1.0, 0.0], constraints=_box([0.05], [3.0], box), options=o,
                x0=[0.0, 0.0], U0=np.tile([math.pi / 3], (N, 1)))


def acrobot(solver, box=True, N=80, integrator="rk4", **opt):
    o = dict(max_iterations=60, tolerance=1e-4, acceptable_tolerance=1e-6); o.update(opt)
    return dict(solver=solver, model=P.Acrobot(), integrator=integrator, dt=0.02, N=N, Q=np.zeros((4, 4)), R=0.01 * np.eye(1),
                Qf=np.diag([100.0, 100.0, 10.0, 10.0]), xref=[-math.pi / 2, 0.5, 0.0, 0.0], constraints=_box([-10.0], [10.0], box), options=o,
                x0=[-math.pi / 2, 0.0, 0.0, 0.0])


def usv(solver, box=True, N=80, integrator="rk4", **opt):
    o = dict(max_iterations=60, tolerance=1e-4, acceptable_tolerance=1e-6); o.update(opt)
    return dict(solver=solver, model=P.Usv3Dof(), integrator=integrator, dt=0.1, N=N, Q=np.zeros((6, 6)), R=1e-4 * np.eye(3),
                Qf=np.diag([100.0, 100.0, 100.0, 10.0, 10.0, 10.0]), xref=[3.0, 2.0, 0.3, 0.0, 0.0, 0.0],
                constraints=_box([-200.0] * 3, [200.0] * 3, box), options=o, x0=[0.0] * 6)


def forklift(solver, box=True, N=100, **opt):
    o = dict(max_iterations=80, tolerance=1e-4, acceptable_tolerance=1e-6); o.update(opt)
    return dict(solver=solver, model=P.Forklift(2.0, 0.03, True, 0.785398), integrator="euler", dt=0.03, N=N, Q=np.zeros((5, 5)),
                R=np.diag([0.1, 1.0]), Qf=np.diag([100.0, 100.0, 50.0, 10.0, 10.0]), xref=[2.0, 1.0, 0.5, 0.0, 0.0],
                constraints=_box([-1.0, -1.0], [1.0, 1.0], box), options=o, x0=[0.0, 0.0, 0.0, 0.5, 0.0], U0=np.tile([0.1, -0.05], (N, 1)))


def linear_fuel(solver, box=True, N=80, integrator="rk4", **opt):
    o = dict(max_iterations=40, tolerance=1e-5, acceptable_tolerance=1e-6, reg_initial_value=1e-6); o.update(opt)
    n = math.sqrt(3.986004418e14 / (6371e3 + 500e3) ** 3)
    return dict(solver=solver, model=P.SpacecraftLinearFuel(n, 300.0, 9.80665), integrator=integrator, dt=10.0, N=N,
                Q=np.diag([1e-4] * 3 + [1e-2] * 3 + [0.0, 0.0]), R=np.eye(3), Qf=np.diag([10.0] * 3 + [100.0] * 3 + [0.0, 0.0]), xref=[0.0] * 8,
                constraints=_box([-0.5] * 3, [0.5] * 3, box), options=o,
                x0=[-37.59664132226163, 27.312455860666148, 13.656227930333074, 0.015161970413423813, 0.08348413138390476, 0.04174206569195238,
                    1.0, 0.0])


def quadrotor_rate(solver, box=True, N=60, integrator="rk4", **opt):
    o = dict(max_iterations=60, tolerance=1e-4, acceptable_tolerance=1e-6); o.update(opt)
    mass, tmax, wmax = 1.0, 20.0, 0.5
    return dict(solver=solver, model=P.QuadrotorRate(mass, tmax, wmax), integrator=integrator, dt=0.05, N=N, Q=np.zeros((10, 10)),
                R=np.diag([0.01, 0.1, 0.1, 0.1]), Qf=np.diag([100.0] * 3 + [10.0] * 3 + [10.0] * 4), xref=[0.5, 0.3, 0.5, 0, 0, 0, 1.0, 0, 0, 0],
                constraints=_box([0.0, -wmax, -wmax, -wmax], [tmax, wmax, wmax, wmax], box), options=o,
                x0=[0.0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0], U0=np.tile([mass * 9.81, 0.0, 0.0, 0.0], (N, 1)))


def spacecraft_nonlinear(solver, box=True, N=40, integrator="rk4", **opt):
    o = dict(max_iterations=40, tolerance=1e-4, acceptable_tolerance=1e-6); o.update(opt)
    return dict(solver=solver, model=P.SpacecraftNonlinear(1.0, 1.0, 1.0, 1.0), integrator=integrator, dt=0.05, N=N, Q=np.zeros((10, 10)), R=0.1 * np.eye(3),
                Qf=np.diag([100.0] * 6 + [0.0] * 4), xref=[0.0] * 6 + [1.0, 0.0, 0.0, 1.0], constraints=_box([-0.3] * 3, [0.3] * 3, box), options=o,
                x0=[0.02, -0.01, 0.01, 0.0, 0.01, 0.0, 1.0, 0.0, 0.0, 1.0])


BUILDERS = {"dubins": dubins, "dreyfus": dreyfus, "acrobot": acrobot, "usv": usv, "forklift": forklift, "linearfuel": linear_fuel,
            "quadrotorrate": quadrotor_rate, "nonlinear": spacecraft_nonlinear}
CASES = {}
for _k, _b in BUILDERS.items():
    for _s in ("CLDDP", "IPDDP"):
        CASES["%s_%s_box" % (_k, _s.lower())] = (lambda b=_b, s=_s: b(s))


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
