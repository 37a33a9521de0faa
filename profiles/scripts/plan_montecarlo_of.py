"""What the output-feedback Monte-Carlo entry costs (profiles/r22_plan_montecarlo_of.md): cddp_hip_plan_montecarlo_of with device pointers, all
moments wanted (stats, nviol_step excluded from the comparison's arithmetic but computed; dXmean, SX, dUmean, SU, dEmean, SE), ny = nx,
against
  - cddp_hip_plan_montecarlo at the same shapes and wants (without the error's moments): the ratio is the price of the estimator;
  - the route available without the entry: field_device("A" / "B" / "K"), torch.randn for the four noises, an N-step loop of
    DevicePlant.step on a plant of batch B * S with the estimator's lines as torch.bmm / einsum, and the moments taken in torch per step
    (the friendly form: no [B][S][N][..] array is kept, only the running sums).
The handle is given torch's stream (set_stream).  cddp_hip_plan_montecarlo then synchronises nothing per call: its calls are queued.
cddp_hip_plan_montecarlo_of keeps C and sqrt(v) in the handle's staging scratch, so every call after the first waits on the host for the
call before it (the scratch rule of capi.hip) and uploads the two arrays with blocking copies: its calls run back to back, not queued, and
the host latency of that wait is inside its figure and inside the ratio to plan_montecarlo.  DevicePlant.step synchronises the stream
itself, which is part of that route.  An interval is a pair of device events around `--reps` calls (1 for the torch loop), divided by
reps, a window of a few tenths of a second for the entries; one warm-up round, then `--rounds` rounds in which the variants take turns; the
figure reported is the median of the rounds.  Peak memory is
torch.cuda.max_memory_allocated over one call of each variant (the entries' scratch belongs to the handle and is reported beside it from
the sizes of what it holds: ny * (nx + 1) doubles).

  python profiles/scripts/plan_montecarlo_of.py --workload unicycle|cartpole --nsamp 64|256 [--batch B] [--horizon N] [--rounds 8] [--reps 20] [--out FILE.json]
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

WORKLOADS = {   # problem(horizon), spread of x0, batch, horizon: the shapes of profiles/r18_plan_montecarlo.md
    "unicycle": (lambda N: api.unicycle_problem(api.SOLVER_IPDDP, N, True), [0.05, 0.05, 0.05], 8192, 200),
    "cartpole": (lambda N: api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N), [0.1, 0.3, 0.1, 0.1], 4096, 100),
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


def peak_mib(fn):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2.0 ** 20


def torch_loop(hs, big, S, C, sd, L, L0, Lw, Lu):
    """the composition available without the entry; moments as running sums per step"""
    B, N, nx, nu = hs.B, hs.p.N, hs.p.nx, hs.p.nu
    dev = C.device
    A = hs.field_device("A").view(B, N, nx, nx); Bm = hs.field_device("B").view(B, N, nx, nu); K = hs.field_device("K").view(B, N, nu, nx)
    Xp = hs.field_device("X"); Up = hs.field_device("U")
    ny = C.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    x = Xp[:, None, 0, :] + torch.randn((B, S, nx), **f64) @ L0.T
    xh = torch.zeros((B, S, nx), **f64)
    out = {k: [] for k in ("dXmean", "SX", "dUmean", "SU", "dEmean", "SE")}

    def moments(d, mean, cov):
        m = d.mean(dim=1)
        c = d - m[:, None]
        out[mean].append(m); out[cov].append(torch.einsum("bsi,bsj->bij", c, c) / (S - 1))

    for t in range(N + 1):
        dx = x - Xp[:, None, t]
        y = dx @ C.T + sd * torch.randn((B, S, ny), **f64)
        xh = xh + torch.bmm(y - xh @ C.T, L[:, t].transpose(1, 2))
        moments(dx, "dXmean", "SX"); moments(dx - xh, "dEmean", "SE")
        if t == N:
            break
        fb = torch.bmm(xh, K[:, t].transpose(1, 2))
        u = Up[:, None, t] + torch.randn((B, S, nu), **f64) @ Lu.T + fb
        moments(u - Up[:, None, t], "dUmean", "SU")
        xh = torch.bmm(xh, A[:, t].transpose(1, 2)) + torch.bmm(fb, Bm[:, t].transpose(1, 2))
        w = (torch.randn((B, S, nx), **f64) @ Lw.T).reshape(B * S, nx)
        x = big.step(x.reshape(B * S, nx).contiguous(), u.reshape(B * S, nu).contiguous(), w).view(B, S, nx)
    return {k: torch.stack(v, dim=1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--nsamp", type=int, default=64)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    make, spread, B, N = WORKLOADS[a.workload]
    B = a.batch or B; N = a.horizon or N; S = a.nsamp
    p = make(N)
    p.options.max_iterations = 3                # the stacks of a swept plan; the cost of the walk does not depend on how far the solve got
    hs = api.HipBatchSolver(p, B)
    hs.set_initial(api.batch_x0(p, B, 20262200, spread), api.batch_U0(p, B))
    hs.solve()
    hs.set_stream(torch.cuda.current_stream().cuda_stream)
    nx, nu = p.nx, p.nu
    sx = np.asarray(spread, dtype=np.float64)
    L0 = np.diag(0.1 * sx); Lw = np.diag(0.02 * sx); Lu = 0.05 * np.eye(nu)
    Cn = np.eye(nx) + 0.1 * np.cos(1.0 + np.arange(nx * nx)).reshape(nx, nx); vn = (0.2 * sx) ** 2
    L = hs.plan_kalman(torch.from_numpy(Cn).cuda(), torch.from_numpy(vn).cuda(), torch.from_numpy(L0 @ L0.T).cuda(), torch.from_numpy(Lw @ Lw.T).cuda(),
                       torch.from_numpy(Lu @ Lu.T).cuda(), want=("L", "SF", "info"))
    res = {"workload": a.workload, "B": B, "N": N, "S": S, "nx": nx, "nu": nu, "ny": nx, "rounds": a.rounds, "reps": a.reps,
           "kalman_info_nonzero": int((L["info"] != 0).sum())}
    SF = L["SF"]; L = L["L"]
    big = api.DevicePlant.of_problem(p, B * S)
    want_mc = ("stats", "nviol_step", "dXmean", "SX", "dUmean", "SU")
    want_of = want_mc + ("dEmean", "SE")
    tC, tsd = torch.from_numpy(Cn).cuda(), torch.from_numpy(np.sqrt(vn)).cuda()
    tL0, tLw, tLu = (torch.from_numpy(M).cuda() for M in (L0, Lw, Lu))
    of = lambda: hs.plan_montecarlo_of(Cn, vn, L, L0, Lw, Lu, nsamp=S, seed=1, factors=True, want=want_of, device=True)
    mc = lambda: hs.plan_montecarlo(L0, Lw, Lu, nsamp=S, seed=1, factors=True, want=want_mc, device=True)
    tl = lambda: torch_loop(hs, big, S, tC, tsd, L, tL0, tLw, tLu)
    ours, ref = of(), tl()
    torch.cuda.synchronize()
    for k in ("SX", "SU", "SE"):                # two independent samplings of the same loop: agreement to sampling error, pooled over the batch
        res["pooled_rel_dev_%s" % k] = float((ours[k].mean(dim=0) - ref[k].mean(dim=0)).abs().max() / ref[k].mean(dim=0).abs().max())
    res["pooled_rel_dev_SE_vs_SF"] = float((ours["SE"].mean(dim=0) - SF.mean(dim=0)).abs().max() / SF.mean(dim=0).abs().max())
    res["peak_mib"] = {"plan_montecarlo_of": peak_mib(of), "plan_montecarlo": peak_mib(mc), "torch_loop": peak_mib(tl)}
    res["handle_scratch_bytes"] = 8 * nx * (nx + 1)
    variants = {"plan_montecarlo_of": (of, a.reps), "plan_montecarlo": (mc, a.reps), "torch_loop": (tl, 1)}
    times = {k: [] for k in variants}
    for k in range(a.rounds + 1):               # round 0 warms up; the variants take turns within a round
        for name, (fn, reps) in variants.items():
            ms = interval(fn, reps)
            if k:
                times[name].append(ms)
    for name in variants:
        res[name] = summary(times[name])
    res["speedup_over_torch_loop"] = res["torch_loop"]["median_ms"] / res["plan_montecarlo_of"]["median_ms"]
    res["of_over_mc"] = res["plan_montecarlo_of"]["median_ms"] / res["plan_montecarlo"]["median_ms"]
    hs.close(); big.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
