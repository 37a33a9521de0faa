"""Wall clock of a WHOLE MPC step -- solve, then seed the next solve -- on one handle (profiles/r10_mpc_advance.md): the host sequence
(cddp_hip_get_trajectory + numpy shift + cddp_hip_forget_solver_state + cddp_hip_set_initial, or cddp_hip_get_plan_head +
cddp_hip_set_initial_state) against cddp_hip_mpc_advance and cddp_hip_mpc_run, for the two MPC workloads of bench.py.  Every flavour
starts from the same cold solve and therefore walks the same (bitwise) sequence of plans; 8 timed rounds after one warm-up round; the
step is reported as solve + rest, with the spread of the rounds.  Both intervals of every flavour end in a device synchronisation
(device_sync): cddp_hip_mpc_advance without a host x_next only enqueues its kernels, so without it their run time would be booked to the
next round's solve.

  python profiles/scripts/mpc_step.py --workload cartpole|unicycle [--batch B] [--rounds 8] [--out FILE.json]
"""
import argparse
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
    "cartpole": (lambda: api.cartpole_problem(api.SOLVER_IPDDP, True), [0.1, 0.3, 0.1, 0.1], 4096),
    "unicycle": (lambda: api.unicycle_problem(api.SOLVER_IPDDP, 200, True), [0.05, 0.05, 0.05], 8192),
}


def shift(A):
    return np.ascontiguousarray(np.concatenate([A[:, 1:], A[:, -1:]], axis=1))


def seed_host(hs, mode):
    if mode == api.MPC_KEEP_PLAN:
        _, x1 = hs.plan_head()
        hs.set_initial_state(x1)
    else:
        X, U = hs.trajectory()
        Xs, Us = shift(X), shift(U)
        hs.forget_solver_state()
        hs.set_initial(np.ascontiguousarray(Xs[:, 0]), Us, Xs)


def seed_device(hs, mode):
    hs.mpc_advance(mode)


def device_sync():
    """every stream of the device idle, the handle's own ones included (one process, one runtime)"""
    torch.cuda.synchronize()


def summary(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max()), "rounds_ms": [float(x) for x in v]}


def restart(hs, x0, U0):
    hs.set_warm_start(False); hs.set_initial(x0, U0); hs.solve(); hs.set_warm_start(True)


def measure_steps(hs, x0, U0, mode, seeder, rounds):
    restart(hs, x0, U0)
    seeder(hs, mode)                           # the cold plan's seed
    device_sync()
    solve, rest, iters, digest = [], [], [], []
    for k in range(rounds + 1):                # round 0 warms up
        t0 = time.perf_counter(); st = hs.solve(); device_sync(); t1 = time.perf_counter()
        seeder(hs, mode); device_sync()
        t2 = time.perf_counter()
        if k:
            solve.append(t1 - t0); rest.append(t2 - t1); iters.append(int(st.traj_iterations)); digest.append(float(st.solve_ms))
    return {"solve": summary(solve), "rest": summary(rest), "step": summary(np.add(solve, rest)), "device_solve_ms_mean": float(np.mean(digest)),
            "traj_iterations_by_round": iters}


def measure_run(hs, x0, U0, mode, rounds):
    restart(hs, x0, U0)
    hs.mpc_advance(mode)
    hs.mpc_run(1, mode)                        # warm-up round
    hs.mpc_run(rounds, mode)                   # (the log's allocation at this length; the plans walked on are not the ones (a) and (b) time)
    restart(hs, x0, U0)
    hs.mpc_advance(mode)
    hs.mpc_run(1, mode)
    device_sync()
    t0 = time.perf_counter(); r = hs.mpc_run(rounds, mode); device_sync(); t1 = time.perf_counter()
    return {"step_mean_ms": (t1 - t0) * 1e3 / rounds, "device_solve_ms_mean": float(r["stats"].solve_ms) / rounds,
            "traj_iterations_by_round": [int(x) for x in r["iterations"].sum(axis=0)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cartpole", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    make, spread, B = WORKLOADS[args.workload]
    B = args.batch or B
    p = make()
    x0 = api.batch_x0(p, B, 20260928 + 1, spread); U0 = api.batch_U0(p, B)
    hs = api.HipBatchSolver(p, B)
    out = {"workload": args.workload, "batch": B, "horizon": p.N, "rounds": args.rounds, "groups": None, "modes": {}}
    try:
        out["groups"] = hs.num_groups()
        hs.set_initial(x0, U0); hs.solve()     # code load / first touch
        for name, mode in (("shift_provided", api.MPC_SHIFT_PROVIDED), ("keep_plan", api.MPC_KEEP_PLAN)):
            a = measure_steps(hs, x0, U0, mode, seed_host, args.rounds)
            b = measure_steps(hs, x0, U0, mode, seed_device, args.rounds)
            c = measure_run(hs, x0, U0, mode, args.rounds)
            same_walk = a["traj_iterations_by_round"] == b["traj_iterations_by_round"] == c["traj_iterations_by_round"]
            out["modes"][name] = {
                "a_host_sequence": a, "b_mpc_advance": b, "c_mpc_run": c, "same_iteration_counts_in_a_b_c": same_walk,
                "trajectories_per_s_whole_step": {"a": B / (a["step"]["mean_ms"] * 1e-3), "b": B / (b["step"]["mean_ms"] * 1e-3), "c": B / (c["step_mean_ms"] * 1e-3)},
                "trajectories_per_s_solve_only_a": B / (a["solve"]["mean_ms"] * 1e-3),
            }
    finally:
        hs.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
