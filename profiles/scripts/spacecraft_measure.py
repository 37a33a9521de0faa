"""Throughput of the spacecraft plants (profiles/r07_spacecraft_plants.md): per plant one IPDDP solve with a control box at B = 4096 on
the resident route (hipEvent time of cddp_hip_solve, one warm-up solve first), and the same problem the only way it could be solved
before the plants had device forms -- a Python DynamicalSystem subclass on the plug-in route (host rollouts) -- at a small batch.
Writes one JSON document to the path given as argv[1]."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import spacecraft_twin as P  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


try:
    import torch  # noqa: F401  (bind the ROCm runtime torch ships before the library, as bench.py does)
except Exception:
    pass
api = _load("cddp_cpp_amd_pyapi", os.path.join(REPO, "cddp-cpp_amd", "pyapi.py"))
pc = _load("pycddp_amd", os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))

INERTIA = np.asarray(api.ATTITUDE_INERTIA)
SPREAD = {"landing2d": [2.0, 0.2, 5.0, 0.5, 0.02, 0.01], "twobody": [0.005] * 6}
PLANTS = {
    "EulerAttitude": ("euler", lambda: api.attitude_problem("euler", api.SOLVER_IPDDP), lambda: P.EulerAttitude(INERTIA)),
    "QuaternionAttitude": ("quaternion", lambda: api.attitude_problem("quaternion", api.SOLVER_IPDDP), lambda: P.QuaternionAttitude(INERTIA)),
    "MrpAttitude": ("mrp", lambda: api.attitude_problem("mrp", api.SOLVER_IPDDP), lambda: P.MrpAttitude(INERTIA)),
    "SpacecraftTwobody": ("twobody", lambda: api.twobody_problem(api.SOLVER_IPDDP), lambda: P.SpacecraftTwobody(1.0, 1.0)),
    "SpacecraftLanding2D": ("landing2d", lambda: api.landing2d_problem(api.SOLVER_IPDDP), lambda: P.SpacecraftLanding2D(*api.LANDING2D_PARAMS)),
}
INTEG = {0: "euler", 1: "heun", 2: "rk3", 3: "rk4"}


class PyPlant(pc.DynamicalSystem):
    """The plant as a user would have had to write it: a Python subclass (the twin's restatement) -> the plug-in route."""
    def __init__(self, tw, dt, integ):
        super().__init__(tw.nx, tw.nu, dt, integ); self.tw = tw
    def get_continuous_dynamics(self, x, u, t=0.0): return self.tw.f(np.asarray(x), np.asarray(u), t)
    def get_state_jacobian(self, x, u, t=0.0): return self.tw.jac(np.asarray(x), np.asarray(u), t)[0]
    def get_control_jacobian(self, x, u, t=0.0): return self.tw.jac(np.asarray(x), np.asarray(u), t)[1]


def resident(p, kind, B, reps):
    x0 = api.batch_x0(p, B, 20261016, SPREAD.get(kind, [0.05] * p.nx)); U0 = api.batch_U0(p, B)
    hs = api.HipBatchSolver(p, B)
    hs.set_initial(x0, U0); hs.solve()                    # warm-up (module load, first-touch)
    ms = []
    for _ in range(reps):
        hs.set_initial(x0, U0); st = hs.solve(); ms.append(st.solve_ms)
    r = hs.results(); hs.close()
    conv = int(np.sum((r["status"] == api.STATUS_OPTIMAL) | (r["status"] == api.STATUS_ACCEPTABLE)))
    med = float(np.median(ms))
    return dict(batch=B, solve_ms=ms, solve_ms_median=med, traj_per_s=B / (med / 1e3), mean_iterations=float(np.mean(r["iterations"])),
                converged=conv)


def plugin(p, kind, tw, B):
    o = pc.CDDPOptions(); o.verbose = False; o.print_solver_header = False
    o.max_iterations = p.options.max_iterations; o.tolerance = p.options.tolerance; o.acceptable_tolerance = p.options.acceptable_tolerance
    s = pc.CDDP(p.x0, p.x_ref, p.N, p.dt, o)
    s.set_dynamical_system(PyPlant(tw, p.dt, INTEG[p.c.integrator]))
    s.set_objective(pc.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    c = p._cons[0]
    s.add_constraint("ControlConstraint", pc.ControlConstraint(np.array(c.lower[:c.dim]), np.array(c.upper[:c.dim])))
    U0 = api.batch_U0(p, 1)
    if U0 is not None:
        s.set_initial_trajectory([p.x0] * (p.N + 1), list(U0[0]))
    x0 = api.batch_x0(p, B, 20261016, SPREAD.get(kind, [0.05] * p.nx))
    t0 = time.perf_counter(); sols = s.solve_batch(list(x0), pc.SolverType.IPDDP); dt = time.perf_counter() - t0
    return dict(batch=B, wall_s=dt, traj_per_s=B / dt, route=sols[0].route, mean_iterations=float(np.mean([x.iterations_completed for x in sols])),
                converged=int(sum(x.status_message in ("OptimalSolutionFound", "AcceptableSolutionFound") for x in sols)))


def main(out):
    res = {}
    only = os.environ.get("SC_ONLY")
    for name, (kind, mk, mk_tw) in PLANTS.items():
        if only and name != only:
            continue
        p = mk()
        res[name] = {"resident": resident(p, kind, 4096, 5)}
        if not only:
            try:
                res[name]["plugin_python_subclass"] = plugin(mk(), kind, mk_tw(), 4)
            except Exception as e:   # recorded, not fatal: the resident numbers are the point of the run
                res[name]["plugin_python_subclass"] = {"error": repr(e)}
        print(name, json.dumps(res[name]), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
