"""What the device-resident inputs and outputs cost (profiles/r12_device_io.md): reading a solved plan back and seeding the next solve with it,
  (a) on the host path:   trajectory() + set_initial()                  -- copies to the host, single-threaded un-tiling / tiling, upload
  (b) on the device path: trajectory_device() + set_initial_device()    -- with BOTH kernel mappings of csrc/inst_io.hip
                          (CDDP_HIP_IO_MAP=staged, the LDS transpose; =naive, lane per trajectory), alternating round by round
  (c) a device-to-device copy of the same byte count (tensor.clone() of X and U, twice: once for the read, once for the seed) -- the
      yardstick of a kernel that only moves data
and, per field (X, U, K, VXX) and mapping, the getter alone against a clone of the same tensor.  Every interval is a host clock around work
that ends in a device synchronisation; one warm-up round, then `--rounds` rounds reported with their spread.  The per-field windows queue
`--reps` calls on a stream given to set_stream (no per-call synchronisation), so a window is long enough to time.  The solve time of the
shape (device events, cddp_hip_stats::solve_ms) is recorded next to it.

  python profiles/scripts/device_io.py --workload unicycle|cartpole [--batch B] [--rounds 8] [--reps 20] [--out FILE.json]
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


import torch  # (binds the ROCm runtime torch ships before the library, as bench.py does)
api = _load("cddp_cpp_amd_pyapi", os.path.join(REPO, "cddp-cpp_amd", "pyapi.py"))

WORKLOADS = {   # bench.py::make_problem / DEFAULT_BATCH
    "cartpole": (lambda: api.cartpole_problem(api.SOLVER_IPDDP, True), [0.1, 0.3, 0.1, 0.1], 4096),
    "unicycle": (lambda: api.unicycle_problem(api.SOLVER_IPDDP, 200, True), [0.05, 0.05, 0.05], 8192),
}
MAPPINGS = ("staged", "naive")


def device_sync():
    torch.cuda.synchronize()


def set_mapping(name):
    os.environ["CDDP_HIP_IO_MAP"] = name      # read by the library at every call (inst_io.hip::io_map_naive)


def summary(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max()), "rounds_ms": [float(x) for x in v]}


def host_round(hs):
    X, U = hs.trajectory()
    hs.set_initial(np.ascontiguousarray(X[:, 0]), U, X)


def device_round(hs):
    X, U = hs.trajectory_device()
    hs.set_initial_device(X[:, 0].contiguous(), U, X)
    return X, U


def clone_round(X, U):
    a = X.clone(); b = U.clone()              # the read: X and U once
    c = a.clone(); d = b.clone()              # the seed: X and U once more
    return c, d


def timed(fn, rounds):
    out = []
    for k in range(rounds + 1):               # round 0 warms up
        device_sync(); t0 = time.perf_counter(); fn(); device_sync(); t1 = time.perf_counter()
        if k:
            out.append(t1 - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="unicycle", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_io.py measures on the GPU: no device found")
    make, spread, B = WORKLOADS[args.workload]
    B = args.batch or B
    p = make()
    x0 = api.batch_x0(p, B, 20260928 + 1, spread); U0 = api.batch_U0(p, B)
    hs = api.HipBatchSolver(p, B)
    out = {"workload": args.workload, "batch": B, "horizon": p.N, "nx": p.nx, "nu": p.nu, "rounds": args.rounds, "reps": args.reps}
    try:
        out["groups"] = hs.num_groups()
        solve_ms = []
        for k in range(4):                    # solve 0: code load / first touch
            hs.set_initial(x0, U0); st = hs.solve(); device_sync()
            if k:
                solve_ms.append(float(st.solve_ms))
        out["solve_ms"] = {"mean": float(np.mean(solve_ms)), "min": float(np.min(solve_ms)), "max": float(np.max(solve_ms))}
        Xh, Uh = hs.trajectory()
        bytes_xu = int(Xh.nbytes + Uh.nbytes)
        out["bytes_X_plus_U"] = bytes_xu
        # the three ways agree before they are timed
        for m in MAPPINGS:
            set_mapping(m)
            Xd, Ud = hs.trajectory_device()
            assert np.array_equal(Xd.cpu().numpy(), Xh, equal_nan=True) and np.array_equal(Ud.cpu().numpy(), Uh, equal_nan=True), m
        # (a), (b) per mapping, (c): alternating within every round
        a, c = [], []
        b = {m: [] for m in MAPPINGS}
        Xd, Ud = hs.trajectory_device()
        for k in range(args.rounds + 1):
            device_sync(); t0 = time.perf_counter(); host_round(hs); device_sync(); t1 = time.perf_counter()
            tb = {}
            for m in (MAPPINGS if k % 2 else MAPPINGS[::-1]):   # (the second of the two finds the plan in the cache: take turns)
                set_mapping(m)
                device_sync(); s0 = time.perf_counter(); device_round(hs); device_sync(); tb[m] = time.perf_counter() - s0
            device_sync(); u0 = time.perf_counter(); clone_round(Xd, Ud); device_sync(); u1 = time.perf_counter()
            if k:
                a.append(t1 - t0); c.append(u1 - u0)
                for m in MAPPINGS:
                    b[m].append(tb[m])
        out["a_host_path"] = summary(a)
        out["b_device_path"] = {m: summary(b[m]) for m in MAPPINGS}
        out["c_clone_same_bytes"] = summary(c)
        out["b_over_c"] = {m: out["b_device_path"][m]["mean_ms"] / out["c_clone_same_bytes"]["mean_ms"] for m in MAPPINGS}
        out["a_over_b"] = {m: out["a_host_path"]["mean_ms"] / out["b_device_path"][m]["mean_ms"] for m in MAPPINGS}
        # per field: `reps` getter calls queued on torch's stream per window, against `reps` clones of the same tensor
        hs.set_stream(torch.cuda.current_stream().cuda_stream)
        fields = {}
        for name in ("X", "U", "K", "VXX"):
            ref = hs.field_device(name); device_sync()
            buf = torch.empty_like(ref)
            row = {"bytes": int(ref.numel() * 8)}

            def clones():
                for _ in range(args.reps):
                    buf.copy_(ref)
            row["clone"] = summary(np.asarray(timed(clones, args.rounds)) / args.reps)
            for m in MAPPINGS:
                set_mapping(m)

                def gets():
                    for _ in range(args.reps):
                        hs.field_device(name, out=buf)
                row[m] = summary(np.asarray(timed(gets, args.rounds)) / args.reps)
                row[m + "_over_clone"] = row[m]["mean_ms"] / row["clone"]["mean_ms"]
                row[m + "_GBps_read_plus_written"] = 2 * row["bytes"] / (row[m]["mean_ms"] * 1e-3) / 1e9
            row["clone_GBps_read_plus_written"] = 2 * row["bytes"] / (row["clone"]["mean_ms"] * 1e-3) / 1e9
            fields[name] = row
        # the seed kernels alone, the same way
        Xs, Us = hs.trajectory_device(); x0s = Xs[:, 0].contiguous(); device_sync()
        row = {"bytes": int((Xs.numel() + Us.numel()) * 8)}
        bx, bu = torch.empty_like(Xs), torch.empty_like(Us)

        def clones2():
            for _ in range(args.reps):
                bx.copy_(Xs); bu.copy_(Us)
        row["clone"] = summary(np.asarray(timed(clones2, args.rounds)) / args.reps)
        for m in MAPPINGS:
            set_mapping(m)

            def sets():
                for _ in range(args.reps):
                    hs.set_initial_device(x0s, Us, Xs)
            row[m] = summary(np.asarray(timed(sets, args.rounds)) / args.reps)
            row[m + "_over_clone"] = row[m]["mean_ms"] / row["clone"]["mean_ms"]
        fields["seed_X_and_U"] = row
        out["per_call_queued"] = fields
        set_mapping("staged")
    finally:
        os.environ.pop("CDDP_HIP_IO_MAP", None)
        hs.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
