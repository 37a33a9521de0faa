"""What one refinement round costs (profiles/r16_mppi_refine.md): cddp_hip_mppi_refine (iters = 1, candidates drawn inside the kernels) against
the same round built from the pieces the library had before -- torch.randn -> clamp -> score_rollouts on device tensors -> torch softmin and
einsum -- at S = 4, 16, 64 candidates per trajectory.  The two paths alternate inside every round of one process; the handle is given
torch's stream (set_stream), so nothing synchronises inside a path; an interval is a pair of device events around ONE round of a path; one
warm-up round, then `--rounds` rounds, the median reported.  Peak memory: the drop of the device's free memory across a path's first run
from an emptied torch cache (torch's segments and the handle's scratch together) and torch's own peak.  Bytes per round are computed from
the shapes: the fused path moves the mean three times and the [B][S] records; the baseline writes the candidate array once and reads it twice.
--trace PATH runs three rounds of one path alone and no timing, for a rocprofv3 --kernel-trace --stats run of its own.

  python profiles/scripts/mppi_refine.py --workload unicycle|cartpole [--batch B] [--rounds 8] [--cands 4,16,64] [--trace fused|baseline] [--out FILE.json]
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

WORKLOADS = {   # bench.py::make_problem / DEFAULT_BATCH; sigma and the descriptor's box (the problem's own control box)
    "cartpole": (lambda: api.cartpole_problem(api.SOLVER_IPDDP, True), [0.1, 0.3, 0.1, 0.1], 4096, [2.0], [-5.0], [5.0], 50.0),
    "unicycle": (lambda: api.unicycle_problem(api.SOLVER_IPDDP, 200, True), [0.05, 0.05, 0.05], 8192, [0.4, 1.0], [-1.1, -np.pi], [1.1, np.pi], 5.0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--cands", default="4,16,64")
    ap.add_argument("--trace", choices=("fused", "baseline"), default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    make, spread, B0, sigma, lo, up, lam = WORKLOADS[a.workload]
    p = make(); B = a.batch or B0
    N, nx, nu = p.N, p.nx, p.nu
    x0 = api.batch_x0(p, B, 20261019, spread)
    hs = api.HipBatchSolver(p, B)
    hs.set_stream(torch.cuda.current_stream().cuda_stream)
    xd = torch.from_numpy(x0).cuda()
    mean = torch.zeros((B, N, nu), dtype=torch.float64, device="cuda")
    sg = torch.tensor(sigma, dtype=torch.float64, device="cuda"); lod = torch.tensor(lo, dtype=torch.float64, device="cuda")
    upd = torch.tensor(up, dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda"); gen.manual_seed(16)
    res = {"workload": a.workload, "B": B, "N": N, "nx": nx, "nu": nu, "rounds": a.rounds, "groups": hs.num_groups(), "runs": {}}

    def fused(S, k=0):
        return hs.mppi_refine(sigma, S, x0=xd, U_mean=mean, iters=1, lam=lam, seed=16, stream=k, keep_mean=True, u_lower=lo, u_upper=up)

    def baseline(S):
        z = torch.randn((B, S, N, nu), dtype=torch.float64, device="cuda", generator=gen)
        z[:, 0] = 0.0
        U = torch.clamp(mean[:, None] + sg * z, lod, upd)
        sc = hs.score_rollouts(U, x0=xd)
        cost, viol = sc["cost"], sc["viol"]
        adm = torch.isfinite(cost) & torch.isfinite(viol) & (viol <= 0.0)
        rho = torch.where(adm, cost, torch.full_like(cost, float("inf"))).amin(dim=1, keepdim=True)
        w = torch.where(adm, torch.exp(-(cost - rho) / lam), torch.zeros_like(cost))
        eta = w.sum(dim=1, keepdim=True)
        w = w / torch.where(eta > 0, eta, torch.ones_like(eta))
        out = torch.clamp(mean + torch.einsum("bs,bsne->bne", w, U - mean[:, None]), lod, upd)
        return {"U": torch.where((eta > 0)[:, :, None], out, mean), "cost": cost, "viol": viol}

    def event_ms(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def first_run_memory(fn):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated(); free0 = torch.cuda.mem_get_info()[0]
        fn(); torch.cuda.synchronize()
        return {"free_memory_drop_bytes": int(free0 - torch.cuda.mem_get_info()[0]), "torch_peak_bytes": int(torch.cuda.max_memory_allocated() - base)}

    for S in [int(s) for s in a.cands.split(",")]:
        if a.trace:
            for k in range(3):
                (fused if a.trace == "fused" else baseline)(S)
            torch.cuda.synchronize()
            continue
        run = {"fused_memory": first_run_memory(lambda: fused(S)), "baseline_memory": first_run_memory(lambda: baseline(S))}
        tf, tb = [], []
        for k in range(a.rounds + 1):               # round 0 warms up; the paths alternate
            f = event_ms(lambda: fused(S, k)); b = event_ms(lambda: baseline(S))
            if k:
                tf.append(f); tb.append(b)
        for name, v in (("fused", tf), ("baseline", tb)):
            v = np.asarray(v)
            run[name] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}
        run["fused_bytes"] = int(8 * (3 * B * N * nu + B * S * nx + 7 * B * S + 6 * B))
        run["baseline_bytes"] = int(8 * (3 * B * S * N * nu + 2 * B * N * nu + B * S * nx + 6 * B * S))
        run["scratch_bytes"] = int(8 * (2 * B * N * nu + 3 * B * S + 3 * B))
        run["candidate_array_bytes"] = int(8 * B * S * N * nu)
        st = fused(S)["stats"]
        run["n_adm_mean"] = float(st[:, 0].mean()); run["ess_mean"] = float(st[:, 2].mean())
        res["runs"]["S=%d" % S] = run
    hs.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
