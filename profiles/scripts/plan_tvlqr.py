"""What the gain design costs (profiles/r20_plan_tvlqr.md): cddp_hip_plan_tvlqr with device pointers, both K_out and P_out wanted, with and
without CDDP_HIP_LQR_INSTALL, against the only way to compute the same thing without it -- field_device("A" / "B") (two un-tiled copies of
the stacks) plus the N-step backward loop in torch with bmm, torch.linalg.cholesky and cholesky_solve.  The handle is given torch's stream
(set_stream), so nothing synchronises per call; an interval is a pair of device events around `--reps` queued calls, divided by reps; one
warm-up round, then `--rounds` rounds in which the three variants take turns; the figure reported is the median of the rounds.

  python profiles/scripts/plan_tvlqr.py --workload unicycle|cartpole|quad12|manip7 [--batch B] [--horizon N] [--rounds 8] [--reps 5] [--out FILE.json]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


import torch  # (binds the ROCm runtime torch ships before the library, as bench.py does)
api = _load("cddp_cpp_amd_pyapi", os.path.join(REPO, "cddp-cpp_amd", "pyapi.py"))

WORKLOADS = {   # problem(horizon), spread of x0, batch, horizon: the shapes of profiles/r17_plan_covariance.md
    "unicycle": (lambda N: api.unicycle_problem(api.SOLVER_IPDDP, N, True), [0.05, 0.05, 0.05], 8192, 200),
    "cartpole": (lambda N: api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N), [0.1, 0.3, 0.1, 0.1], 4096, 100),
    "quad12": (lambda N: api.quadrotor12_problem(api.SOLVER_IPDDP, N, True), None, 1024, 100),
    "manip7": (lambda N: api.manipulator7_problem(api.SOLVER_IPDDP, N, False), None, 1024, 100),    # (14, 7): 32 trajectories per workgroup
}


def interval(fn, reps):
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def torch_tvlqr(hs, Qd, Rd, Qf):
    """the composition available without the entry: the two stacks un-tiled into new tensors, then N dependent steps of small bmm and a
    batched Cholesky solve (the Joseph form, as the entry computes it)"""
    B, N, nx, nu = hs.B, hs.p.N, hs.p.nx, hs.p.nu
    A = hs.field_device("A").view(B, N, nx, nx); Bm = hs.field_device("B").view(B, N, nx, nu)
    K = torch.empty((B, N, nu, nx), dtype=torch.float64, device=Qd.device)
    P = torch.empty((B, N + 1, nx, nx), dtype=torch.float64, device=Qd.device)
    Pt = Qf.expand(B, nx, nx)
    P[:, N] = Pt
    for t in range(N - 1, -1, -1):
        At = A[:, t]; Bt = Bm[:, t]
        M = torch.bmm(Pt, Bt)
        L = torch.linalg.cholesky(torch.bmm(Bt.transpose(1, 2), M) + Rd)
        Kt = -torch.cholesky_solve(torch.bmm(M.transpose(1, 2), At), L)
        Acl = At + torch.bmm(Bt, Kt)
        Pt = Qd + torch.bmm(Kt.transpose(1, 2), torch.bmm(Rd.expand(B, nu, nu), Kt)) + torch.bmm(Acl.transpose(1, 2), torch.bmm(Pt, Acl))
        K[:, t] = Kt; P[:, t] = Pt
    return K, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    make, spread, B, N = WORKLOADS[a.workload]
    B = a.batch or B; N = a.horizon or N
    p = make(N)
    p.options.max_iterations = 3                # the stacks of a swept plan; the cost of the walk does not depend on how far the solve got
    hs = api.HipBatchSolver(p, B)
    hs.set_initial(api.batch_x0(p, B, 20262000, spread), api.batch_U0(p, B))
    hs.solve()
    hs.set_stream(torch.cuda.current_stream().cuda_stream)
    nx, nu = p.nx, p.nu
    rng = np.random.default_rng(1)

    def spd(n, scale):
        M = rng.standard_normal((n, n))
        return torch.from_numpy(scale * (M @ M.T / n + 0.1 * np.eye(n))).cuda()

    Q, R, Qf = spd(nx, 1.0), spd(nu, 0.5), spd(nx, 3.0)
    Qd, Rd = Q * p.dt, R * p.dt
    res = {"workload": a.workload, "B": B, "N": N, "nx": nx, "nu": nu, "rounds": a.rounds, "reps": a.reps}
    ours = hs.plan_tvlqr(Q, R, Qf)
    ref = torch_tvlqr(hs, Qd, Rd, Qf)
    res["info_nonzero"] = int((ours["info"] != 0).sum())
    res["max_abs_dev_K_over_max"] = float((ours["K"] - ref[0]).abs().max() / ref[0].abs().max())
    res["max_abs_dev_P_over_max"] = float((ours["P"] - ref[1]).abs().max() / ref[1].abs().max())
    variants = {
        "plan_tvlqr": (lambda: hs.plan_tvlqr(Q, R, Qf), a.reps),
        "plan_tvlqr_install": (lambda: hs.plan_tvlqr(Q, R, Qf, install=True), a.reps),
        "torch_loop": (lambda: torch_tvlqr(hs, Qd, Rd, Qf), max(1, a.reps // 5)),
    }
    times = {k: [] for k in variants}
    for k in range(a.rounds + 1):               # round 0 warms up; the variants take turns within a round
        for name, (fn, reps) in variants.items():
            ms = interval(fn, reps)
            if k:
                times[name].append(ms)
    for name in variants:
        res[name] = summary(times[name])
    res["speedup"] = res["torch_loop"]["median_ms"] / res["plan_tvlqr"]["median_ms"]
    hs.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
