"""Measurements of profiles/r23_ekf.md, on one MI355X:  python profiles/r23_ekf_measure.py [filter] [mpc] [host] > log

filter: cddp_hip_ekf_run (one launch) against the same filter as a Python loop of cddp_hip_ekf_update / cddp_hip_ekf_predict, both on
        device tensors, alternating, 8 rounds, median (min - max); for the LTI plant also a torch.bmm / cholesky_solve Kalman loop.
mpc:    the whole step of cddp_hip_mpc_run_ekf against cddp_hip_mpc_run_plant from the same cold handle state, alternating, 8 rounds.
host:   the route the loop replaces: get_plan_head -> numpy EKF on the host (model_eval per trajectory) -> mpc_advance with a host x_next.
Every timed window ends in a synchronising call (the entries return after their outputs are written)."""
import importlib.util
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def load_api():
    spec = importlib.util.spec_from_file_location("cddp_cpp_amd_pyapi", os.path.join(REPO, "cddp-cpp_amd", "pyapi.py"))
    mod = importlib.util.module_from_spec(spec); sys.modules["cddp_cpp_amd_pyapi"] = mod; spec.loader.exec_module(mod)
    return mod


def stat(ts):
    ts = np.asarray(ts) * 1e3
    return "%.3f (%.3f - %.3f)" % (np.median(ts), ts.min(), ts.max())


def spd(rng, n, scale):
    M = rng.standard_normal((n, n))
    return scale * (M @ M.T / n + 0.1 * np.eye(n))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def filter_shapes(api):
    return [("unicycle", api.unicycle_problem(api.SOLVER_IPDDP, horizon=5, obstacle=False), 8192, 200, 2),
            ("cartpole", api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=5), 4096, 100, 2),
            ("quad12", api.quadrotor12_problem(api.SOLVER_IPDDP, horizon=5), 1024, 100, 6),
            ("manip7", api.manipulator7_problem(api.SOLVER_IPDDP, horizon=5, terminal_equality=False), 1024, 100, 7)]


def measure_filter(api, rounds=8):
    print("| shape | ekf_run, one launch [ms] | Python loop of update / predict [ms] | ratio | per step and trajectory, one launch [ns] |")
    print("|---|---|---|---|---|")
    for name, p, B, T, ny in filter_shapes(api):
        rng = np.random.default_rng(23)
        nx, nu = p.nx, p.nu
        plant = api.DevicePlant.of_problem(p, B)
        C = np.eye(nx)[:ny] + 0.05 * rng.standard_normal((ny, nx)); v = 1e-3 * (1.0 + rng.random(ny))
        ekf = api.DeviceEkf(plant, C, v, 1e-6 * np.eye(nx), 1e-4 * np.eye(nu))
        x0 = dev(p.x0[None, :] + 0.01 * rng.standard_normal((B, nx))); P0 = dev(1e-3 * np.eye(nx))
        Y = dev((p.x0 @ C.T)[None, None, :] + 0.01 * rng.standard_normal((B, T + 1, ny)))
        U = dev(0.01 * rng.standard_normal((B, T, nu)))
        Yt = [Y[:, t].contiguous() for t in range(T + 1)]; Ut = [U[:, t].contiguous() for t in range(T)]
        torch.cuda.synchronize()

        def one():
            ekf.reset(x0, P0)
            t0 = time.perf_counter(); r = ekf.run(Y, U, want=("Xh", "nis")); return time.perf_counter() - t0, r

        def loop():
            ekf.reset(x0, P0)
            t0 = time.perf_counter()
            for t in range(T + 1):
                if t > 0:
                    ekf.predict(Ut[t - 1])
                nis = ekf.update(Yt[t])
            return time.perf_counter() - t0, (ekf.get(device=True)[0], nis)
        (_, r), (_, l) = one(), loop()                                      # warm-up, and the two routes agree bit for bit
        assert torch.equal(r["Xh"][:, -1], l[0]) and torch.equal(r["nis"][:, -1], l[1]) and bool(torch.isfinite(r["Xh"]).all())
        a, b = [], []
        for _ in range(rounds):
            a.append(one()[0]); b.append(loop()[0])
        print("| %s B = %d, T = %d, ny = %d | %s | %s | %.1f x | %.1f |" % (name, B, T, ny, stat(a), stat(b), np.median(b) / np.median(a),
                                                                       np.median(a) * 1e9 / (B * (T + 1))))
        ekf.close(); plant.close()
    # LTI: the Kalman filter in torch (batched matrices, the gain by a Cholesky solve), the usual way to write it on this device
    B, T, ny, dt = 8192, 200, 2, 0.1
    A = np.array([[1.0, 0.1], [-0.2, 0.95]]); Bm = np.array([[0.005], [0.1]])
    rng = np.random.default_rng(24)
    C = np.array([[1.0, 0.0], [0.3, 1.0]]); v = np.array([0.04, 0.09]); W = spd(rng, 2, 0.02); P0 = spd(rng, 2, 0.5)
    plant = api.DevicePlant(api.MODEL_LTI, api.EULER, dt, 2, 1, B, lti_A=A, lti_B=Bm)
    ekf = api.DeviceEkf(plant, C, v, W)
    x0 = dev(rng.standard_normal((B, 2))); Y = dev(rng.standard_normal((B, T + 1, ny))); U = dev(0.2 * rng.standard_normal((B, T, 1)))
    P0d = dev(P0)
    At, Bt, Ct, Vt, Wt = dev(A), dev(Bm), dev(C), dev(np.diag(v)), dev(W)

    def one():
        ekf.reset(x0, P0d)
        t0 = time.perf_counter(); r = ekf.run(Y, U, want=("Xh",)); return time.perf_counter() - t0, r["Xh"]

    def torch_loop():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        x = x0.clone(); P = P0d.expand(B, 2, 2).contiguous(); out = []
        for t in range(T + 1):
            if t > 0:
                x = x @ At.T + U[:, t - 1] @ Bt.T
                P = At @ P @ At.T + Wt
            S = Ct @ P @ Ct.T + Vt
            K = torch.cholesky_solve(Ct @ P, torch.linalg.cholesky(S)).transpose(1, 2)      # P C^T S^-1
            x = x + torch.bmm(K, (Y[:, t] - x @ Ct.T).unsqueeze(2)).squeeze(2)
            P = P - K @ Ct @ P
            out.append(x)
        Xh = torch.stack(out, dim=1); torch.cuda.synchronize()
        return time.perf_counter() - t0, Xh
    (_, r), (_, l) = one(), torch_loop()
    gap = float((r - l).abs().max())
    a, b = [], []
    for _ in range(rounds):
        a.append(one()[0]); b.append(torch_loop()[0])
    print("| lti 2 x 1 B = %d, T = %d, ny = %d: torch.bmm / cholesky_solve loop instead of the Python loop (largest |difference| of the estimates %.1e) | %s | %s | %.1f x | %.1f |"
          % (B, T, ny, gap, stat(a), stat(b), np.median(b) / np.median(a), np.median(a) * 1e9 / (B * (T + 1))))
    ekf.close(); plant.close()


def mpc_shapes(api):
    return [("unicycle", api.unicycle_problem(api.SOLVER_IPDDP, horizon=200), 8192), ("cartpole", api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=100), 4096)]


def mpc_setup(api, p, B, name):
    rng = np.random.default_rng(25)
    spread = np.full(p.nx, 0.05); x0 = p.x0[None, :] + spread * rng.uniform(-1, 1, (B, p.nx))
    ny = p.nx - 1
    C = np.eye(p.nx)[:ny]; v = np.full(ny, 1e-4)
    return np.ascontiguousarray(x0), api.batch_U0(p, B), C, v, 1e-3 * rng.standard_normal((B, 64, p.nx)), 1e-2 * rng.standard_normal((B, 65, ny))


def measure_mpc(api, rounds=8, steps=8):
    print("| shape | mpc_run_plant, whole step [ms] | mpc_run_ekf, whole step [ms] | added [ms / step] | device time of the solves, plant / ekf [ms / step] |")
    print("|---|---|---|---|---|")
    for name, p, B in mpc_shapes(api):
        p.options.warm_start = 1
        x0, U0, C, v, Wn, Yn = mpc_setup(api, p, B, name)
        plant = api.DevicePlant.of_problem(p, B, integrator=api.RK4)
        model = api.DevicePlant.of_problem(p, B)
        ekf = api.DeviceEkf(model, C, v, 1e-6 * np.eye(p.nx), 1e-4 * np.eye(p.nu))
        h = api.HipBatchSolver(p, B)

        def run(with_ekf):
            h.set_initial(x0, U0); h.initialize()
            ekf.reset(x0, 1e-4 * np.eye(p.nx))
            t0 = time.perf_counter()
            if with_ekf:
                r = h.mpc_run_ekf(plant, ekf, steps, api.MPC_SHIFT_EXISTING, x0, W=Wn[:, :steps], Yn=Yn[:, :steps + 1])
            else:
                r = h.mpc_run_plant(plant, steps, api.MPC_SHIFT_EXISTING, W=Wn[:, :steps])
            return (time.perf_counter() - t0) / steps, r["stats"].solve_ms / steps, r
        run(False); run(True)
        a, b, sa, sb = [], [], [], []
        for _ in range(rounds):
            t, s, _ = run(False); a.append(t); sa.append(s)
            t, s, r = run(True); b.append(t); sb.append(s)
        assert np.all(np.isfinite(r["X_visited"])) and np.all(np.isfinite(r["Xh_visited"]))
        print("| %s B = %d, N = %d, %d steps | %s | %s | %.3f | %.2f / %.2f |" % (name, B, p.N, steps, stat(a), stat(b), (np.median(b) - np.median(a)) * 1e3,
                                                                              np.median(sa), np.median(sb)))
        h.close(); ekf.close(); model.close(); plant.close()


def measure_host(api, rounds=3, steps=3):
    import plan_ekf_ref as PE
    print("| shape | host route, whole step [ms] | of which the numpy EKF [ms] |")
    print("|---|---|---|")
    for name, p, B in mpc_shapes(api):
        p.options.warm_start = 1
        x0, U0, C, v, Wn, Yn = mpc_setup(api, p, B, name)
        plant = api.DevicePlant.of_problem(p, B, integrator=api.RK4)
        model = PE.HostModel(api, p.c.model, p.c.integrator, p.dt, p.nx, p.nu, list(p.c.model_params))
        h = api.HipBatchSolver(p, B)
        Cb = PE.batched(C, B, C.shape)
        ts, fs = [], []
        for _ in range(rounds):
            h.set_initial(x0, U0); h.initialize()
            f = PE.Filter(model, B, C, v, 1e-6 * np.eye(p.nx), 1e-4 * np.eye(p.nu)); f.reset(x0, 1e-4 * np.eye(p.nx))
            x = x0.copy(); tf = 0.0
            t0 = time.perf_counter()
            for k in range(steps):
                t1 = time.perf_counter()
                f.update(PE.measure(Cb, x, Yn[:, k])); tf += time.perf_counter() - t1
                h.mpc_advance(api.MPC_KEEP_PLAN if k == 0 else api.MPC_SHIFT_EXISTING, x_next=f.xh)
                h.solve()
                u0, _ = h.plan_head()
                x = plant.step(x, u0, np.ascontiguousarray(Wn[:, k]))
                t1 = time.perf_counter(); f.predict(u0); tf += time.perf_counter() - t1
            ts.append((time.perf_counter() - t0) / steps); fs.append(tf / steps)
        print("| %s B = %d, N = %d, %d steps | %s | %s |" % (name, B, p.N, steps, stat(ts), stat(fs)))
        h.close(); plant.close()


if __name__ == "__main__":
    api = load_api()
    what = sys.argv[1:] or ["filter", "mpc", "host"]
    print("device: %s" % torch.cuda.get_device_name(0))
    for w in what:
        print("\n## %s" % w); sys.stdout.flush()
        {"filter": measure_filter, "mpc": measure_mpc, "host": measure_host}[w](api)
        sys.stdout.flush()
