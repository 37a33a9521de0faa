"""What the plan sensitivities cost (profiles/r14_plan_sensitivity.md): cddp_hip_plan_jvp and cddp_hip_plan_vjp with device pointers at
nvec = 1 and nvec = nx, against the only way to compute the same thing without them -- field_device("A" / "B" / "K") (three un-tiled
copies of the stacks) plus the N dependent steps of torch.bmm.  Both variants of the batch-major rows (CDDP_HIP_SENS_IO=direct: one 8-byte
access per lane and element; =staged: runs of a few steps through LDS) and, at nvec = nx, one vector per lane and pass
(CDDP_HIP_SENS_RV=1) against chunks of four (=4).  The handle is given torch's stream (set_stream), so nothing synchronises per call; an
interval is a pair of device events around `--reps` queued calls, divided by reps; one warm-up round, then `--rounds` rounds.
Achieved bytes per second count the matrix bytes (nx^2 + 2 nx nu) * 8 * N * B once per chunk pass plus the vectors read and written, against
the 8 TB/s the project uses.

  python profiles/scripts/plan_sensitivity.py --workload unicycle|cartpole [--batch B] [--rounds 8] [--reps 10] [--out FILE.json]
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


def torch_jvp(hs, dx0):
    """the composition available without the entry: the three stacks un-tiled into new tensors, then N dependent steps of small bmm"""
    B, N, nx, nu = hs.B, hs.p.N, hs.p.nx, hs.p.nu
    A = hs.field_device("A").view(B, N, nx, nx); Bm = hs.field_device("B").view(B, N, nx, nu); K = hs.field_device("K").view(B, N, nu, nx)
    dx = dx0.transpose(1, 2)                   # (B, nx, R)
    R = dx.shape[2]
    dX = torch.empty((B, N + 1, nx, R), dtype=torch.float64, device=dx0.device); dU = torch.empty((B, N, nu, R), dtype=torch.float64, device=dx0.device)
    dX[:, 0] = dx
    for t in range(N):
        du = torch.bmm(K[:, t], dx)
        dx = torch.bmm(A[:, t], dx) + torch.bmm(Bm[:, t], du)
        dU[:, t] = du; dX[:, t + 1] = dx
    return dX, dU


def torch_vjp(hs, gX, gU):
    B, N, nx, nu = hs.B, hs.p.N, hs.p.nx, hs.p.nu
    A = hs.field_device("A").view(B, N, nx, nx); Bm = hs.field_device("B").view(B, N, nx, nu); K = hs.field_device("K").view(B, N, nu, nx)
    gx = gX.permute(0, 2, 3, 1); gu = gU.permute(0, 2, 3, 1)      # (B, T, e, R)
    lam = gx[:, N]
    for t in range(N - 1, -1, -1):
        mu = gu[:, t] + torch.bmm(Bm[:, t].transpose(1, 2), lam)
        lam = gx[:, t] + torch.bmm(A[:, t].transpose(1, 2), lam) + torch.bmm(K[:, t].transpose(1, 2), mu)
    return lam.transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    make, spread, B0 = WORKLOADS[a.workload]
    p = make(); B = a.batch or B0
    N, nx, nu = p.N, p.nx, p.nu
    hs = api.HipBatchSolver(p, B)
    hs.set_initial(api.batch_x0(p, B, 20261014, spread), api.batch_U0(p, B))
    st = hs.solve()
    hs.set_stream(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda"); gen.manual_seed(14)
    mat = (nx * nx + 2 * nx * nu) * 8 * N * B
    res = {"workload": a.workload, "B": B, "N": N, "nx": nx, "nu": nu, "groups": hs.num_groups(), "solve_ms": float(st.solve_ms),
           "rounds": a.rounds, "reps": a.reps, "matrix_bytes": mat, "runs": {}}
    for R in (1, nx):
        dx0 = torch.randn((B, R, nx), dtype=torch.float64, device="cuda", generator=gen)
        gX = torch.randn((B, R, N + 1, nx), dtype=torch.float64, device="cuda", generator=gen)
        gU = torch.randn((B, R, N, nu), dtype=torch.float64, device="cuda", generator=gen)
        vec = 8 * B * R * (nx + (N + 1) * nx + N * nu)               # vectors read + written, either direction
        ref = None
        for io in ("direct", "staged"):
            for rv in (("wide", "1") if R >= 4 else ("1",)):
                os.environ["CDDP_HIP_SENS_IO"] = io
                os.environ["CDDP_HIP_SENS_RV"] = "1" if rv == "1" else "4"
                chunk = 1 if rv == "1" else 4
                passes = (R + chunk - 1) // chunk
                nbytes = mat * passes + vec
                dX, dU = hs.plan_jvp(dx0); g0 = hs.plan_vjp(gX, gU)
                if ref is None:
                    ref = (dX.clone(), dU.clone(), g0.clone())
                same = bool(torch.equal(dX, ref[0]) and torch.equal(dU, ref[1]) and torch.equal(g0, ref[2]))
                key = "nvec=%d io=%s rv=%s" % (R, io, rv)
                res["runs"][key] = {"jvp": summary(timed(lambda: hs.plan_jvp(dx0), a.rounds, a.reps), nbytes),
                                    "vjp": summary(timed(lambda: hs.plan_vjp(gX, gU), a.rounds, a.reps), nbytes), "same_bits_as_first": same}
        os.environ.pop("CDDP_HIP_SENS_IO", None); os.environ.pop("CDDP_HIP_SENS_RV", None)
        tX, tU = torch_jvp(hs, dx0); t0 = torch_vjp(hs, gX, gU)
        err = {"jvp_max_abs_diff": float((tX.permute(0, 3, 1, 2) - ref[0]).abs().max()), "vjp_max_abs_diff": float((t0 - ref[2]).abs().max()),
               "jvp_max_abs": float(ref[0].abs().max()), "vjp_max_abs": float(ref[2].abs().max())}
        res["runs"]["nvec=%d torch" % R] = {"jvp": summary(timed(lambda: torch_jvp(hs, dx0), a.rounds, a.torch_reps)),
                                            "vjp": summary(timed(lambda: torch_vjp(hs, gX, gU), a.rounds, a.torch_reps)), "agreement": err}
    hs.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
