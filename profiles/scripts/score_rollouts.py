"""What scoring candidates costs (profiles/r15_score_rollouts.md): cddp_hip_score_rollouts on device tensors at S = 4, 16, 64 candidates per
trajectory against the only way the library offered before -- S times set_initial_device + initialize + results_device --, and
cddp_hip_seed_best against torch indexing + set_initial_device.  The handle is given torch's stream (set_stream), so nothing synchronises
per call; an interval is a pair of device events around `--reps` queued calls, divided by reps; one warm-up round, then `--rounds` rounds.
Bytes counted for the scoring launch: U read once, x0 read once per candidate, cost and viol written, against the 8 TB/s the project uses.
--lib PATH loads a library built from a variant of csrc/inst_score.hip instead of the product (the lane-order comparison of the note).
--headline (cart-pole only): S = 16 bang-bang candidates of different switching times against the zero seed -- how many trajectories end
at a lower objective, and the iteration counts.  A recorded observation, not a test.

  python profiles/scripts/score_rollouts.py --workload unicycle|cartpole [--batch B] [--rounds 8] [--reps 5] [--lib PATH] [--headline] [--out FILE.json]
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
    "cartpole": (lambda: api.cartpole_problem(api.SOLVER_IPDDP, True), [0.1, 0.3, 0.1, 0.1], 4096, 4.0),
    "unicycle": (lambda: api.unicycle_problem(api.SOLVER_IPDDP, 200, True), [0.05, 0.05, 0.05], 8192, 0.8),
}
PEAK = 8.0e12


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


def summary(v, nbytes=None):
    v = np.asarray(v, dtype=np.float64)
    s = {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max())}
    if nbytes is not None:
        s["bytes"] = int(nbytes); s["TBps_at_mean"] = float(nbytes / (v.mean() * 1e-3) / 1e12); s["of_peak"] = float(nbytes / (v.mean() * 1e-3) / PEAK)
    return s


def headline(p, B, x0):
    """cart-pole swing-up: the zero seed against the best of 16 bang-bang candidates (+5 then -5, and the mirror image, eight switching times)"""
    N = p.N
    cand = np.zeros((16, N, 1))
    for k, ts in enumerate(np.linspace(0.1, 0.8, 8)):
        sw = int(ts * N)
        cand[k, :sw] = 5.0; cand[k, sw:] = -5.0
        cand[8 + k] = -cand[k]
    cand *= 0.98                                                     # strictly inside the box
    U = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(cand[None], (B, 16, N, 1)))).cuda()
    xd = torch.from_numpy(x0).cuda()
    out = {}
    hs = api.HipBatchSolver(p, B)
    hs.set_initial_device(xd); st = hs.solve(); r0 = hs.results()
    out["zero_seed"] = {"solve_ms": float(st.solve_ms), "mean_iterations": float(r0["iterations"].mean()), "converged": int(st.n_converged),
                        "median_objective": float(np.median(r0["final_objective"]))}
    sc = hs.score_rollouts(U, x0=xd)
    w = hs.seed_best(U, sc["cost"], sc["viol"], x0=xd, viol_tol=0.0)
    st = hs.solve(); r1 = hs.results()
    out["best_of_16"] = {"solve_ms": float(st.solve_ms), "mean_iterations": float(r1["iterations"].mean()), "converged": int(st.n_converged),
                         "median_objective": float(np.median(r1["final_objective"])),
                         "winner_histogram": np.bincount(w.cpu().numpy().clip(min=0), minlength=16).tolist()}
    out["lower_objective"] = int((r1["final_objective"] < r0["final_objective"]).sum())
    out["higher_objective"] = int((r1["final_objective"] > r0["final_objective"]).sum())
    out["B"] = B
    hs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cands", default="4,16,64")
    ap.add_argument("--lib", default="")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.lib:
        api.HIP_LIB_PATH = os.path.abspath(a.lib)
    make, spread, B0, uscale = WORKLOADS[a.workload]
    p = make(); B = a.batch or B0
    N, nx, nu = p.N, p.nx, p.nu
    x0 = api.batch_x0(p, B, 20261019, spread)
    res = {"workload": a.workload, "B": B, "N": N, "nx": nx, "nu": nu, "rounds": a.rounds, "reps": a.reps, "lib": a.lib or "product", "runs": {}}
    hs = api.HipBatchSolver(p, B)
    res["groups"] = hs.num_groups()
    hs.set_stream(torch.cuda.current_stream().cuda_stream)
    xd = torch.from_numpy(x0).cuda()
    gen = torch.Generator(device="cuda"); gen.manual_seed(15)
    for S in [int(s) for s in a.cands.split(",")]:
        U = uscale * torch.randn((B, S, N, nu), dtype=torch.float64, device="cuda", generator=gen)
        nbytes = 8 * B * S * (N * nu + nx + 2)
        sc = hs.score_rollouts(U, x0=xd)
        run = {"score": summary(timed(lambda: hs.score_rollouts(U, x0=xd), a.rounds, a.reps), nbytes)}
        run["viol_positive"] = int((sc["viol"] > 0).sum())
        run["cost_xor"] = int(np.bitwise_xor.reduce(sc["cost"].cpu().numpy().view(np.uint64).ravel()))   # equal between builds that compute the same bits
        if not a.no_baseline:
            Uc = [U[:, c].contiguous() for c in range(S)]

            def old():
                out = []
                for c in range(S):
                    hs.set_initial_device(xd, Uc[c]); hs.initialize(); out.append(hs.results_device()["final_objective"])
                return out
            ref = torch.stack(old(), dim=1)
            run["same_bits_as_initialize"] = bool(torch.equal(ref, sc["cost"]))
            run["initialize_loop"] = summary(timed(old, a.rounds, 1))
            run["seed_best"] = summary(timed(lambda: hs.seed_best(U, sc["cost"], sc["viol"], x0=xd), a.rounds, a.reps))
            ar = torch.arange(B, device="cuda")

            def old_seed():
                w = torch.where(sc["viol"] <= 0.0, sc["cost"], torch.full_like(sc["cost"], float("inf"))).argmin(dim=1)
                hs.set_initial_device(xd, U[ar, w].contiguous())
            run["torch_seed"] = summary(timed(old_seed, a.rounds, a.reps))
        res["runs"]["S=%d" % S] = run
        del U
    hs.close()
    if a.headline:
        res["headline"] = headline(p, B, x0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
