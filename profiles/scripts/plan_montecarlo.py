"""What a Monte-Carlo evaluation of a solved plan costs (profiles/r18_plan_montecarlo.md): cddp_hip_plan_montecarlo on device tensors with
every moment requested (stats, nviol_step, dXmean, SX, dUmean, SU) at S = 64 and 256 samples per trajectory, against the path the library
offered before -- torch.randn + triangular product -> score_rollouts(FEEDBACK, X_out, U_out) -> torch mean and covariance.  No process
noise in the comparison: the old path cannot inject it (the new path with it is timed on its own).  The handle is given torch's stream
(set_stream), so nothing synchronises per call; an interval is a pair of device events around `--reps` queued calls, divided by reps; one
warm-up round, then `--rounds` rounds, the median is reported.  Peak memory: torch.cuda.max_memory_allocated over one call (on the device
path every array of either route is a torch tensor; the handle's own buffers are the same for both and are not counted).
Shares, by difference on the same handle: reductions = (all moments - cost alone) / all moments; generator = (cost alone - cost alone
without any factor) / all moments.

  python profiles/scripts/plan_montecarlo.py --workload unicycle|cartpole [--batch B] [--samples 64,256] [--rounds 8] [--reps 3] [--out FILE.json]
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

WORKLOADS = {   # bench.py::make_problem / DEFAULT_BATCH
    "cartpole": (lambda: api.cartpole_problem(api.SOLVER_IPDDP, True), [0.1, 0.3, 0.1, 0.1], 4096),
    "unicycle": (lambda: api.unicycle_problem(api.SOLVER_IPDDP, 200, True), [0.05, 0.05, 0.05], 8192),
}
MOMENTS = ("stats", "nviol_step", "dXmean", "SX", "dUmean", "SU")


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
    v = np.asarray(out)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def peak_of(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--samples", default="64,256")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    make, spread, B0 = WORKLOADS[a.workload]
    p = make(); B = a.batch or B0
    p.options.max_iterations = a.iterations
    N, nx, nu = p.N, p.nx, p.nu
    x0 = api.batch_x0(p, B, 20261019, spread)
    hs = api.HipBatchSolver(p, B)
    hs.set_initial(x0, api.batch_U0(p, B)); hs.solve()
    res = {"workload": a.workload, "B": B, "N": N, "nx": nx, "nu": nu, "rounds": a.rounds, "reps": a.reps, "groups": hs.num_groups(), "runs": {}}
    hs.set_stream(torch.cuda.current_stream().cuda_stream)
    Xp, Up = hs.trajectory_device()
    L0 = np.tril(0.02 * np.ones((nx, nx))) + 0.03 * np.eye(nx); Lu = np.tril(0.02 * np.ones((nu, nu))) + 0.05 * np.eye(nu); Lw = 0.2 * L0
    L0d = torch.from_numpy(L0).cuda(); Lud = torch.from_numpy(Lu).cuda()
    gen = torch.Generator(device="cuda"); gen.manual_seed(18)
    for S in [int(s) for s in a.samples.split(",")]:
        kw = dict(nsamp=S, seed=18, factors=True, device=True)

        def new(want=MOMENTS, L0_=L0, Lw_=None, Lu_=Lu):
            return hs.plan_montecarlo(L0_, Lw_, Lu_, want=want, **kw)

        def old():
            Z0 = torch.randn((B, S, nx), dtype=torch.float64, device="cuda", generator=gen) @ L0d.T
            E = torch.randn((B, S, N, nu), dtype=torch.float64, device="cuda", generator=gen) @ Lud.T
            sc = hs.score_rollouts(Up[:, None] + E, x0=Xp[:, None, 0] + Z0, feedback=True, want=("cost", "viol", "X", "U"))
            out = {"cost_mean": sc["cost"].mean(dim=1), "cost_var": sc["cost"].var(dim=1), "n_viol": (sc["viol"] > 0).sum(dim=1)}
            for key, T, ref in (("X", sc["X"], Xp), ("U", sc["U"], Up)):
                d = T - ref[:, None]
                m = d.mean(dim=1)
                d = d - m[:, None]
                out["d%smean" % key] = m
                out["S" + key] = torch.einsum("bsti,bstj->btij", d, d) / (S - 1)
            return out

        run = {}
        r_new = new(); r_old = old()
        # the two routes estimate the same moments from different draws: recorded as a plausibility figure, not a test
        run["SX_ratio_new_over_old_median"] = float((r_new["SX"].diagonal(dim1=2, dim2=3)[:, 1:] / r_old["SX"].diagonal(dim1=2, dim2=3)[:, 1:]).median())
        run["n_finite_min"] = float(r_new["stats"][:, 0].min()); run["n_viol_mean"] = float(r_new["stats"][:, 1].mean())
        del r_new, r_old
        run["new_all_moments"] = timed(new, a.rounds, a.reps)
        run["old_torch_route"] = timed(old, a.rounds, a.reps)
        run["new_cost_only"] = timed(lambda: new(("cost",)), a.rounds, a.reps)
        run["new_cost_only_no_noise"] = timed(lambda: new(("cost",), None, None, None), a.rounds, a.reps)
        run["new_all_moments_with_process_noise"] = timed(lambda: new(MOMENTS, L0, Lw, Lu), a.rounds, a.reps)
        run["new_with_X_U_out"] = timed(lambda: new(MOMENTS + ("X", "U")), a.rounds, a.reps)
        full = run["new_all_moments"]["median_ms"]
        run["share_reductions"] = (full - run["new_cost_only"]["median_ms"]) / full
        run["share_generator"] = (run["new_cost_only"]["median_ms"] - run["new_cost_only_no_noise"]["median_ms"]) / full
        run["ratio_old_over_new"] = run["old_torch_route"]["median_ms"] / full
        run["peak_bytes_new"] = peak_of(new)
        run["peak_bytes_old"] = peak_of(old)
        res["runs"]["S=%d" % S] = run
        print("S=%d" % S, json.dumps(run), flush=True)
    hs.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
