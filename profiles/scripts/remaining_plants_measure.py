"""Throughput of the plants of ids 16-23 (profiles/r08_remaining_plants.md): per plant one IPDDP solve with a control box at B = 4096 on
the resident route (hipEvent time of cddp_hip_solve, one warm-up solve first).  For DubinsCar and SpacecraftLinearFuel also the route
they took before they had kernels -- the facade's numpy restatement on the plug-in route (a subclass with model = None: GPU backward
passes, host rollouts through Python callbacks) -- and the resident route on the SAME problem at the SAME batch (B = 64), so that the
two trajectories-per-second figures compare like with like.  Writes one JSON document to argv[1]."""
import importlib.util
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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

SPREAD = {"dubins": [0.05, 0.05, 0.02], "dreyfus": [0.02, 0.05], "acrobot": [0.02] * 4, "usv": [0.05] * 6, "forklift": [0.05, 0.05, 0.02, 0.02, 0.01],
          "linearfuel": [0.5, 0.5, 0.5, 0.002, 0.002, 0.002, 0.01, 0.0], "quadrotorrate": [0.05] * 6 + [0.0, 0.02, 0.02, 0.02],
          "nonlinear": [0.002] * 6 + [0.0] * 4}
PLANTS = {"DubinsCar": ("dubins", api.dubins_problem), "DreyfusRocket": ("dreyfus", api.dreyfus_problem), "Acrobot": ("acrobot", api.acrobot_problem),
          "Usv3Dof": ("usv", api.usv_problem), "Forklift": ("forklift", api.forklift_problem), "QuadrotorRate": ("quadrotorrate", api.quadrotor_rate_problem),
          "SpacecraftLinearFuel": ("linearfuel", api.linear_fuel_problem), "SpacecraftNonlinear": ("nonlinear", api.spacecraft_nonlinear_problem)}


class HostDubinsCar(pc.DubinsCar):
    model = None


class HostSpacecraftLinearFuel(pc.SpacecraftLinearFuel):
    model = None


def resident(p, kind, B, reps):
    x0 = api.batch_x0(p, B, 20261016, SPREAD[kind]); U0 = api.batch_U0(p, B)
    hs = api.HipBatchSolver(p, B)
    hs.set_initial(x0, U0); hs.solve()                    # warm-up (module load, first-touch)
    ms = []
    for _ in range(reps):
        hs.set_initial(x0, U0); st = hs.solve(); ms.append(st.solve_ms)
    r = hs.results(); hs.close()
    conv = int(np.sum((r["status"] == api.STATUS_OPTIMAL) | (r["status"] == api.STATUS_ACCEPTABLE)))
    med = float(np.median(ms))
    return dict(batch=B, solve_ms=ms, solve_ms_median=med, traj_per_s=B / (med / 1e3), mean_iterations=float(np.mean(r["iterations"])), converged=conv)


def plugin(p, kind, plant, B):
    o = pc.CDDPOptions(); o.verbose = False; o.print_solver_header = False
    o.max_iterations = p.options.max_iterations; o.tolerance = p.options.tolerance; o.acceptable_tolerance = p.options.acceptable_tolerance
    o.regularization.initial_value = p.options.reg_initial_value
    s = pc.CDDP(p.x0, p.x_ref, p.N, p.dt, o)
    s.set_dynamical_system(plant)
    s.set_objective(pc.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    c = p._cons[0]
    s.add_constraint("ControlConstraint", pc.ControlConstraint(np.array(c.lower[:c.dim]), np.array(c.upper[:c.dim])))
    U0 = api.batch_U0(p, 1)
    if U0 is not None:
        s.set_initial_trajectory([p.x0] * (p.N + 1), list(U0[0]))
    x0 = api.batch_x0(p, B, 20261016, SPREAD[kind])
    t0 = time.perf_counter(); sols = s.solve_batch(list(x0), pc.SolverType.IPDDP); dt = time.perf_counter() - t0
    return dict(batch=B, wall_s=dt, traj_per_s=B / dt, route=sols[0].route, mean_iterations=float(np.mean([x.iterations_completed for x in sols])),
                converged=int(sum(x.status_message in ("OptimalSolutionFound", "AcceptableSolutionFound") for x in sols)))


def main(out):
    res = {}
    for name, (kind, mk) in PLANTS.items():
        p = mk(api.SOLVER_IPDDP)
        res[name] = {"resident": resident(p, kind, 4096, 5)}
        host = {"DubinsCar": lambda: HostDubinsCar(1.0, p.dt), "SpacecraftLinearFuel": lambda: HostSpacecraftLinearFuel(p.dt, p.c.model_params[0], 300.0, integration_type="rk4")}.get(name)
        if host is not None:
            res[name]["resident_b64"] = resident(mk(api.SOLVER_IPDDP), kind, 64, 5)
            res[name]["plugin_numpy_restatement_b64"] = plugin(mk(api.SOLVER_IPDDP), kind, host(), 64)
        print(name, json.dumps(res[name]), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
