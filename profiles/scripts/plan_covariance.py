"""What the plan covariance costs (profiles/r17_plan_covariance.md): cddp_hip_plan_covariance with device pointers, W and Wu given, full and
diagonal output, against the only way to compute the same thing without it -- field_device("A" / "B" / "K") (three un-tiled copies of
the stacks) plus N dependent steps of torch.bmm triple products.  The handle is given torch's stream (set_stream), so nothing synchronises
per call; an interval is a pair of device events around `--reps` queued calls, divided by reps; one warm-up round, then `--rounds` rounds;
the figure reported is the median of the rounds.

  python profiles/scripts/plan_covariance.py --workload unicycle|cartpole|quad12|manip7 [--batch B] [--horizon N] [--rounds 8] [--reps 5] [--out FILE.json]
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

WORKLOADS = {   # problem(horizon), spread of x0, batch, horizon
    "unicycle": (lambda N: api.unicycle_problem(api.SOLVER_IPDDP, N, True), [0.05, 0.05, 0.05], 8192, 200),
    "cartpole": (lambda N: api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N), [0.1, 0.3, 0.1, 0.1], 4096, 100),
    "quad12": (lambda N: api.quadrotor12_problem(api.SOLVER_IPDDP, N, True), None, 1024, 100),      # the nx >= 12 shape
    "manip7": (lambda N: api.manipulator7_problem(api.SOLVER_IPDDP, N, False), None, 1024, 100),    # (14, 7): the pair at the LDS and register limit
}


def timed(fn, rounds, reps):
    out = []
    for k in range(rounds + 1):               # round 0 warms up
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); a.record()
        for _ in range(reps):
            fn()
        b.record(); torch.cuda.synchronize()
        if k:
            out.append(a.elapsed_time(b) / reps)
    return out


def summary(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def torch_cov(hs, S0, W, Wu, Qdt, Rdt, Qf, diag):
    """the composition available without the entry: the three stacks un-tiled into new tensors, then N dependent steps of small bmm"""
    B, N, nx, nu = hs.B, hs.p.N, hs.p.nx, hs.p.nu
    A = hs.field_device("A").view(B, N, nx, nx); Bm = hs.field_device("B").view(B, N, nx, nu); K = hs.field_device("K").view(B, N, nu, nx)
    SX = torch.empty((B, N + 1, nx) if diag else (B, N + 1, nx, nx), dtype=torch.float64, device=S0.device)
    SU = torch.empty((B, N, nu) if diag else (B, N, nu, nu), dtype=torch.float64, device=S0.device)
    Sig = S0.expand(B, nx, nx)
    dcost = torch.zeros(B, dtype=torch.float64, device=S0.device)
    for t in range(N):
        Kt = K[:, t]; Bt = Bm[:, t]
        Acl = A[:, t] + torch.bmm(Bt, Kt)
        Su = torch.bmm(torch.bmm(Kt, Sig), Kt.transpose(1, 2)) + Wu
        dcost = dcost + (Qdt * Sig).sum((1, 2)) + (Rdt * Su).sum((1, 2))
        if diag:
            SX[:, t] = torch.diagonal(Sig, dim1=1, dim2=2); SU[:, t] = torch.diagonal(Su, dim1=1, dim2=2)
        else:
            SX[:, t] = Sig; SU[:, t] = Su
        Sig = torch.bmm(torch.bmm(Acl, Sig), Acl.transpose(1, 2)) + W + torch.bmm(torch.bmm(Bt, Wu.expand(B, nu, nu)), Bt.transpose(1, 2))
    SX[:, N] = torch.diagonal(Sig, dim1=1, dim2=2) if diag else Sig
    dcost = dcost + (Qf * Sig).sum((1, 2))
    return SX, SU, dcost


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
    hs.set_initial(api.batch_x0(p, B, 20261700, spread), api.batch_U0(p, B))
    hs.solve()
    hs.set_stream(torch.cuda.current_stream().cuda_stream)
    nx, nu = p.nx, p.nu
    rng = np.random.default_rng(1)

    def spd(n, scale):
        M = rng.standard_normal((n, n))
        return torch.from_numpy(scale * (M @ M.T / n + 0.1 * np.eye(n))).cuda()

    S0, W, Wu = spd(nx, 1.0), spd(nx, 0.05), spd(nu, 0.1)
    Qdt = torch.from_numpy(np.asarray(p.Q) * p.dt).cuda(); Rdt = torch.from_numpy(np.asarray(p.R) * p.dt).cuda(); Qf = torch.from_numpy(np.asarray(p.Qf)).cuda()
    res = {"workload": a.workload, "B": B, "N": N, "nx": nx, "nu": nu, "rounds": a.rounds, "reps": a.reps}
    for diag in (False, True):
        mode = "diag" if diag else "full"
        ours = hs.plan_covariance(S0, W, Wu, diag=diag)
        ref = torch_cov(hs, S0, W, Wu, Qdt, Rdt, Qf, diag)
        scale = float(ref[0].abs().max())
        res[mode] = {
            "max_abs_dev_SX_over_max": float((ours["SX"] - ref[0]).abs().max()) / scale if np.isfinite(scale) and scale > 0 else None,
            "plan_covariance": summary(timed(lambda: hs.plan_covariance(S0, W, Wu, diag=diag), a.rounds, a.reps)),
            "plan_covariance_SX_only": summary(timed(lambda: hs.plan_covariance(S0, W, Wu, diag=diag, want=("SX",)), a.rounds, a.reps)),
            "torch_bmm": summary(timed(lambda: torch_cov(hs, S0, W, Wu, Qdt, Rdt, Qf, diag), a.rounds, max(1, a.reps // 5))),
        }
        res[mode]["speedup"] = res[mode]["torch_bmm"]["median_ms"] / res[mode]["plan_covariance"]["median_ms"]
    hs.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
