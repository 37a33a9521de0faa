"""What following a reference path costs per MPC step (profiles/r19_reference_path.md), at the two MPC workloads of bench.py and
profiles/r10_mpc_advance.md.  Flavours, every one `steps` closed-loop steps from the same cold solve, timed as a whole by a host clock
between two device synchronisations and divided by `steps`:

  (a)  cddp_hip_mpc_run, fixed goal, on the library of ANOTHER tree (--parent DIR: the parent commit's pyapi.py + lib/libcddp_hip.so),
       loaded into the same process under another module name; without --parent the flavour is left out;
  (a') cddp_hip_mpc_run, fixed goal, this tree's library (no path bound: the advance takes no extra launch);
  (b)  cddp_hip_mpc_run with a bound path of ONE row, the problem's own goal: every window is the fixed goal along the horizon, so the
       solves walk the plans of (a) (the iteration sums are compared) and the difference to (a) is what the feature adds -- the window
       launch per step and group, and the solver kernels reading a per-step reference instead of the goal alone;
  (t)  cddp_hip_mpc_run, no path bound, after ONE cddp_hip_set_reference of the same constant rows as a per-step reference: the solver
       kernels read a per-step reference as in (b), the advance takes no window launch -- the control that splits (b) - (a) in two;
  (b') cddp_hip_mpc_run with a bound path that moves (the goal approached along a line): other solves, reported with their iteration sum;
  (c)  the loop a caller writes without the bound path: solve; cddp_hip_mpc_advance; cddp_hip_set_reference(window from the host), with
       the windows of (b).  The plan head is not read back, as mpc_run does not read it either.

The flavours alternate within a round; 8 timed rounds after one warm-up round; median, min and max over the rounds.  Also the time of
one cddp_hip_create (+ destroy) at the shape: what a caller who re-creates the handle to move the goal pays per step today.

  python profiles/scripts/reference_path.py --workload cartpole|unicycle [--parent DIR] [--steps 8] [--rounds 8] [--only b] [--out FILE.json]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import ref_window_ref as RW  # noqa: E402  (the numpy restatement of the window: the host loop's uploads)


def workloads(A):   # bench.py::make_problem / DEFAULT_BATCH
    return {"cartpole": (lambda: A.cartpole_problem(A.SOLVER_IPDDP, True), [0.1, 0.3, 0.1, 0.1], 4096),
            "unicycle": (lambda: A.unicycle_problem(A.SOLVER_IPDDP, 200, True), [0.05, 0.05, 0.05], 8192)}


def device_sync():
    torch.cuda.synchronize()


def restart(hs, x0, U0):
    hs.set_warm_start(False); hs.set_initial(x0, U0); hs.solve(); hs.set_warm_start(True)


def stat(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "rounds_ms": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cartpole", choices=["cartpole", "unicycle"])
    ap.add_argument("--parent", default="")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mode = api.MPC_SHIFT_PROVIDED
    apis = {"new": api}
    if args.parent:
        apis["parent"] = _load("cddp_parent_pyapi", os.path.join(args.parent, "cddp-cpp_amd", "pyapi.py"))
        assert apis["parent"].HIP_LIB_PATH != api.HIP_LIB_PATH and not hasattr(apis["parent"].HipBatchSolver, "set_reference")
    make, spread, B = workloads(api)[args.workload]
    B = args.batch or B
    p = make()
    N, steps = p.N, args.steps
    x0 = api.batch_x0(p, B, 20260928 + 1, spread); U0 = api.batch_U0(p, B)
    const_path = np.ascontiguousarray(p.x_ref[None, :])
    s = np.linspace(0.0, 1.0, N + steps + 1)[:, None]
    moving_path = np.ascontiguousarray((1.0 - s) * (p.x0 + 0.5 * (p.x_ref - p.x0))[None, :] + s * p.x_ref[None, :])
    flavours = {}

    def handle(A):
        q = workloads(A)[args.workload][0]()
        h = A.HipBatchSolver(q, B)
        h.set_initial(x0, U0); h.solve()                       # code load / first touch
        return h

    def run_plain(h):
        return lambda: h.mpc_run(steps, mode)

    def run_path(h, path):
        def go():
            h.mpc_set_reference_path(path)
            return h.mpc_run(steps, mode)
        return go

    def run_fixed_traj(h, path):
        def go():
            w = RW.window(path, 0, N); h.set_reference(x_ref=w[N], x_ref_traj=w)
            return h.mpc_run(steps, mode)
        return go

    def run_host_loop(h, path):
        def go():
            it = 0
            w = RW.window(path, 0, N); h.set_reference(x_ref=w[N], x_ref_traj=w)
            for k in range(steps):
                it += int(h.solve().traj_iterations)
                h.mpc_advance(mode)
                w = RW.window(path, k + 1, N); h.set_reference(x_ref=w[N], x_ref_traj=w)
            return it
        return go

    want = [f for f in args.only.split(",") if f]
    plan = []
    if "parent" in apis:
        plan.append(("a_parent_mpc_run", "parent", lambda h: run_plain(h)))
    plan += [("a_new_mpc_run_no_path", "new", lambda h: run_plain(h)), ("b_mpc_run_bound_path_const", "new", lambda h: run_path(h, const_path)),
             ("t_mpc_run_fixed_traj_no_path", "new", lambda h: run_fixed_traj(h, const_path)),
             ("b_mpc_run_bound_path_moving", "new", lambda h: run_path(h, moving_path)), ("c_host_loop_set_reference", "new", lambda h: run_host_loop(h, const_path))]
    plan = [f for f in plan if not want or f[0].split("_")[0] in want]
    handles = {}
    create_ms = []
    for _ in range(3):
        device_sync(); t0 = time.perf_counter(); h = api.HipBatchSolver(p, B); device_sync(); t1 = time.perf_counter(); h.close(); device_sync()
        create_ms.append((t1 - t0) * 1e3)
    for name, which, mk in plan:
        handles[name] = handle(apis[which])
        flavours[name] = {"go": mk(handles[name]), "ms": [], "iters": []}
    try:
        for r in range(args.rounds + 1):                         # round 0 warms up
            for name, f in flavours.items():
                h = handles[name]
                if name[:2] in ("b_", "c_", "t_"):
                    h.mpc_set_reference_path(None)
                    if h.get_reference()[1] is not None:
                        h.set_reference(x_ref=p.x_ref, clear_traj=True)   # the cold solve of every round on the problem's own goal
                restart(h, x0, U0)
                device_sync(); t0 = time.perf_counter(); out = f["go"](); device_sync(); t1 = time.perf_counter()
                if r:
                    f["ms"].append((t1 - t0) * 1e3 / steps)
                    f["iters"].append(int(out) if not isinstance(out, dict) else int(out["iterations"].sum()))
    finally:
        for h in handles.values():
            h.close()
    res = {"workload": args.workload, "batch": B, "horizon": N, "steps_per_run": steps, "rounds": args.rounds, "mode": "SHIFT_PROVIDED",
           "create_ms": stat(create_ms), "step": {n: dict(stat(f["ms"]), traj_iterations_by_round=f["iters"]) for n, f in flavours.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
