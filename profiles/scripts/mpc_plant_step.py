"""Wall clock of a closed-loop MPC step against a SEPARATE plant (profiles/r11_mpc_plant.md): solve, step the true plant from the current
state with u_0, seed the next solve from the plant's state -- for the two MPC workloads of bench.py in SHIFT_PROVIDED mode.  The plant is
the model's RK4, substeps = 4, per-trajectory-parameter version.  Three flavours, each from the same cold solve:
  (a) what the library offered before the device plant: cddp_hip_get_plan_head, a host loop over cddp_hip_model_eval (one call per
      trajectory and substep, single-threaded, through ctypes), cddp_hip_mpc_advance with a host x_next;
  (b) cddp_hip_get_plan_head, cddp_hip_plant_step on device pointers (the state stays on the device), cddp_hip_mpc_advance(X_DEVICE);
  (c) cddp_hip_mpc_run_plant, whole call / rounds.
Every interval ends in a device synchronisation; 8 timed rounds after one warm-up round; the step is reported as solve + rest.  (b) and (c)
run the same arithmetic and must walk the same plans (equal iteration sums per round); (a)'s host plant calls the host libm where the
device plant calls the library's own sin / cos, so its states can differ in the last bits: the script reports whether its sums agree.
Also: cddp_hip_track_plan against the host loop over gains() / trajectory() / DevicePlant.step, at the same shape.

  python profiles/scripts/mpc_plant_step.py --workload cartpole|unicycle [--batch B] [--rounds 8] [--out FILE.json]
"""
import argparse
import ctypes as C
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


import torch  # (binds the ROCm runtime torch ships before the library, as bench.py does; device_sync below)
api = _load("cddp_cpp_amd_pyapi", os.path.join(REPO, "cddp-cpp_amd", "pyapi.py"))

WORKLOADS = {   # bench.py::make_problem / DEFAULT_BATCH
    "cartpole": (lambda: api.cartpole_problem(api.SOLVER_IPDDP, True), [0.1, 0.3, 0.1, 0.1], 4096, 5),
    "unicycle": (lambda: api.unicycle_problem(api.SOLVER_IPDDP, 200, True), [0.05, 0.05, 0.05], 8192, 0),
}
SUBSTEPS = 4
MODE = api.MPC_SHIFT_PROVIDED


def device_sync():
    torch.cuda.synchronize()


def summary(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max()), "rounds_ms": [float(x) for x in v]}


def restart(hs, x0, U0):
    hs.set_warm_start(False); hs.set_initial(x0, U0); hs.solve(); hs.set_warm_start(True)
    hs.mpc_advance(MODE, x_next=x0)            # the cold plan's seed, from the state the loop starts in
    device_sync()


class HostPlant:
    """The plant of flavour (a): cddp_hip_model_eval once per trajectory and substep (the host build of the same plants)."""
    def __init__(self, p, params):
        self.lib = api.load_hip()
        self.model, self.nx, self.nu, self.h = int(p.c.model), p.nx, p.nu, float(p.c.dt) / SUBSTEPS
        self.params = np.ascontiguousarray(params)
        self.fn = self.lib.cddp_hip_model_eval
        dp = C.POINTER(C.c_double)
        self.fn.argtypes = [C.c_int, C.c_int, C.c_double, dp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp]
        self.fn.restype = C.c_int

    def step(self, x, u):
        dp = C.POINTER(C.c_double)
        a = np.ascontiguousarray(x).copy(); b = np.empty_like(a)
        for _ in range(SUBSTEPS):
            for i in range(a.shape[0]):
                rc = self.fn(self.model, api.RK4, self.h, self.params[i].ctypes.data_as(dp), self.nx, self.nu, a[i].ctypes.data_as(dp),
                             u[i].ctypes.data_as(dp), b[i].ctypes.data_as(dp), None, None, None, None, None)
                assert rc == 0
            a, b = b, a
        return a


def measure(hs, x0, U0, rounds, plant_step):
    """flavours (a) and (b): plant_step(x_cur, u0) -> (x_next as mpc_advance takes it, x_next as the next round's x_cur)"""
    restart(hs, x0, U0)
    x_cur = x0
    solve, rest, iters = [], [], []
    for k in range(rounds + 1):                # round 0 warms up
        t0 = time.perf_counter(); st = hs.solve(); device_sync(); t1 = time.perf_counter()
        u0, _ = hs.plan_head()
        x_cur = plant_step(x_cur, u0)
        hs.mpc_advance(MODE, x_next=x_cur); device_sync()
        t2 = time.perf_counter()
        if k:
            solve.append(t1 - t0); rest.append(t2 - t1); iters.append(int(st.traj_iterations))
    return {"solve": summary(solve), "rest": summary(rest), "step": summary(np.add(solve, rest)), "traj_iterations_by_round": iters}


def measure_run(hs, x0, U0, rounds, plant):
    restart(hs, x0, U0)
    hs.mpc_run_plant(plant, 1, MODE); hs.mpc_run_plant(plant, rounds, MODE)   # the log's allocation at this length
    restart(hs, x0, U0)
    hs.mpc_run_plant(plant, 1, MODE)           # warm-up round
    device_sync()
    t0 = time.perf_counter(); r = hs.mpc_run_plant(plant, rounds, MODE); device_sync(); t1 = time.perf_counter()
    step = (t1 - t0) * 1e3 / rounds; dev = float(r["stats"].solve_ms) / rounds
    return {"step_mean_ms": step, "device_solve_ms_mean": dev, "rest_upper_ms": step - dev,
            "traj_iterations_by_round": [int(x) for x in r["iterations"].sum(axis=0)]}


def host_track(hs, plant, xs):
    K, _ = hs.gains(); X, U = hs.trajectory()
    x = xs.copy()
    for t in range(K.shape[1]):
        u = U[:, t] + np.einsum("bij,bj->bi", K[:, t], x - X[:, t])
        x = plant.step(x, u)
    return x


def measure_track(hs, x0, U0, plant, reps=3):
    hs.set_warm_start(False); hs.set_initial(x0, U0); hs.solve()
    xs = np.ascontiguousarray(hs.trajectory()[0][:, 0] + 1e-2 * np.random.default_rng(1).standard_normal(x0.shape))
    hs.track_plan(plant, x0=xs); device_sync()
    dev, host = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); hs.track_plan(plant, x0=xs); device_sync(); dev.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); host_track(hs, plant, xs); device_sync(); host.append(time.perf_counter() - t0)
    return {"track_plan_ms": summary(dev), "host_loop_ms": summary(host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cartpole", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    make, spread, B, npar = WORKLOADS[args.workload]
    B = args.batch or B
    p = make()
    x0 = api.batch_x0(p, B, 20260928 + 1, spread); U0 = api.batch_U0(p, B)
    params = np.tile(np.array(list(p.c.model_params)), (B, 1))
    if npar:                                   # domain randomisation: every trajectory its own masses (cart-pole: cart and pole)
        params[:, :2] *= 1.0 + 0.1 * np.random.default_rng(2).random((B, 2))
    hs = api.HipBatchSolver(p, B)
    plant = api.DevicePlant.of_problem(p, B, params=params, integrator=api.RK4, substeps=SUBSTEPS)
    host_plant = HostPlant(p, params)
    out = {"workload": args.workload, "batch": B, "horizon": p.N, "rounds": args.rounds, "substeps": SUBSTEPS, "groups": None}
    try:
        out["groups"] = hs.num_groups()
        hs.set_initial(x0, U0); hs.solve()     # code load / first touch

        def step_a(x_cur, u0):
            return host_plant.step(x_cur, u0)

        def step_b(x_cur, u0):
            xd = x_cur if hasattr(x_cur, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x_cur)).to("cuda:0")
            return plant.step(xd, torch.from_numpy(u0).to("cuda:0"))
        a = measure(hs, x0, U0, args.rounds, step_a)
        b = measure(hs, x0, U0, args.rounds, step_b)
        c = measure_run(hs, x0, U0, args.rounds, plant)
        out.update({"a_host_plant": a, "b_plant_step_device": b, "c_mpc_run_plant": c,
                    "same_iteration_counts_b_c": b["traj_iterations_by_round"] == c["traj_iterations_by_round"],
                    "same_iteration_counts_a_b": a["traj_iterations_by_round"] == b["traj_iterations_by_round"],
                    "tracking": measure_track(hs, x0, U0, plant)})
    finally:
        hs.close(); plant.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
