"""What the filter entry costs (profiles/r21_plan_kalman.md): cddp_hip_plan_kalman with device pointers, L, SX, SU and dcost wanted, W and Wu
given, ny = nx (and ny = 1 beside it), against the only way to compute the same thing without it -- field_device("A" / "B" / "K") (three
un-tiled copies of the stacks) plus the N-step forward loop in torch with bmm, torch.linalg.cholesky and cholesky_solve on the batch-form
filter.  The handle is given torch's stream (set_stream), so nothing synchronises per call; an interval is a pair of device events
around `--reps` queued calls, divided by reps; one warm-up round, then `--rounds` rounds in which the variants take turns; the figure
reported is the median of the rounds.

  python profiles/scripts/plan_kalman.py --workload unicycle|cartpole|quad12|manip7 [--batch B] [--horizon N] [--rounds 8] [--reps 5] [--out FILE.json]
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

WORKLOADS = {   # problem(horizon), spread of x0, batch, horizon: the shapes of profiles/r17_plan_covariance.md and r20_plan_tvlqr.md
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


def torch_kalman(hs, C, v, S0, W, Wu, Qdt, Rdt, Qf):
    """the composition available without the entry: the three stacks un-tiled into new tensors, then N + 1 dependent steps of small bmm
    and a batched Cholesky solve (the batch-form filter: L = Sm C^T (C Sm C^T + V)^-1, Sf = (I - L C) Sm)"""
    B, N, nx, nu = hs.B, hs.p.N, hs.p.nx, hs.p.nu
    ny = C.shape[0]
    A = hs.field_device("A").view(B, N, nx, nx); Bm = hs.field_device("B").view(B, N, nx, nu); K = hs.field_device("K").view(B, N, nu, nx)
    dev = C.device
    L = torch.empty((B, N + 1, nx, ny), dtype=torch.float64, device=dev); SX = torch.empty((B, N + 1, nx, nx), dtype=torch.float64, device=dev)
    SU = torch.empty((B, N, nu, nu), dtype=torch.float64, device=dev); dcost = torch.zeros((B,), dtype=torch.float64, device=dev)
    Cb = C.expand(B, ny, nx); V = torch.diag(v)
    Sm = S0.expand(B, nx, nx); Xm = torch.zeros((B, nx, nx), dtype=torch.float64, device=dev)
    for t in range(N + 1):
        CS = torch.bmm(Cb, Sm)
        Lt = torch.cholesky_solve(CS, torch.linalg.cholesky(torch.bmm(CS, Cb.transpose(1, 2)) + V)).transpose(1, 2)
        G = torch.bmm(Lt, CS)
        Sf = Sm - G
        Xh = Xm + G
        Sx = Xh + Sf
        L[:, t] = Lt; SX[:, t] = Sx
        if t == N:
            dcost += (Qf * Sx).sum(dim=(1, 2))
            break
        At = A[:, t]; Bt = Bm[:, t]; Kt = K[:, t]
        Su = torch.bmm(Kt, torch.bmm(Xh, Kt.transpose(1, 2))) + Wu
        SU[:, t] = Su
        dcost += (Qdt * Sx).sum(dim=(1, 2)) + (Rdt * Su).sum(dim=(1, 2))
        Acl = At + torch.bmm(Bt, Kt)
        Sm = torch.bmm(At, torch.bmm(Sf, At.transpose(1, 2))) + W + torch.bmm(Bt, torch.bmm(Wu.expand(B, nu, nu), Bt.transpose(1, 2)))
        Xm = torch.bmm(Acl, torch.bmm(Xh, Acl.transpose(1, 2)))
    return L, SX, SU, dcost


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

    S0, W, Wu = spd(nx, 1.0), spd(nx, 0.05), spd(nu, 0.1)
    C = torch.from_numpy(rng.standard_normal((nx, nx))).cuda(); v = torch.from_numpy(0.05 + rng.random(nx)).cuda()
    C1 = C[:1].contiguous(); v1 = v[:1].contiguous()
    Qdt = torch.from_numpy(np.asarray(p.Q, dtype=np.float64).reshape(nx, nx) * p.dt).cuda()
    Rdt = torch.from_numpy(np.asarray(p.R, dtype=np.float64).reshape(nu, nu) * p.dt).cuda()
    Qf = torch.from_numpy(np.asarray(p.Qf, dtype=np.float64).reshape(nx, nx)).cuda()
    res = {"workload": a.workload, "B": B, "N": N, "nx": nx, "nu": nu, "ny": nx, "rounds": a.rounds, "reps": a.reps}
    want = ("L", "SX", "SU", "dcost", "info")
    ours = hs.plan_kalman(C, v, S0, W, Wu, want=want)
    ref = torch_kalman(hs, C, v, S0, W, Wu, Qdt, Rdt, Qf)
    res["info_nonzero"] = int((ours["info"] != 0).sum())
    for k, r in zip(("L", "SX", "SU"), ref):
        res["max_abs_dev_%s_over_max" % k] = float((ours[k] - r).abs().max() / r.abs().max())
    res["max_rel_dev_dcost"] = float(((ours["dcost"] - ref[3]).abs() / ref[3].abs()).max())
    want = want[:4]
    variants = {
        "plan_kalman": (lambda: hs.plan_kalman(C, v, S0, W, Wu, want=want), a.reps),
        "plan_kalman_ny1": (lambda: hs.plan_kalman(C1, v1, S0, W, Wu, want=want), a.reps),
        "torch_loop": (lambda: torch_kalman(hs, C, v, S0, W, Wu, Qdt, Rdt, Qf), max(1, a.reps // 5)),
    }
    times = {k: [] for k in variants}
    for k in range(a.rounds + 1):               # round 0 warms up; the variants take turns within a round
        for name, (fn, reps) in variants.items():
            ms = interval(fn, reps)
            if k:
                times[name].append(ms)
    for name in variants:
        res[name] = summary(times[name])
    res["speedup"] = res["torch_loop"]["median_ms"] / res["plan_kalman"]["median_ms"]
    res["ny1_over_nynx"] = res["plan_kalman_ny1"]["median_ms"] / res["plan_kalman"]["median_ms"]
    hs.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
