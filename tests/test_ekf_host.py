"""The step bodies of the extended Kalman filter (cddp-cpp_amd/csrc/ekf.hpp) on the host, and the numpy restatement the GPU tests use.

1. tests/cpp/test_ekf.cpp, a stand-alone program, walks B = 3 trajectories over T = 3 steps through the bodies for the pendulum (nx = 2),
   the cart-pole (nx = 4) and the 7-joint arm (nx = 14), RK4, with ny = 1, nx, nx + 2 and 16: all four W / Wu combinations, a control box
   (ny = 1 and 16), two NaN drop-out rows (ny = nx) and a trajectory whose P0 = -I fails its first pivot (ny = nx + 2).  Built twice with
   g++ -ffp-contract=off -DCDDP_TRIG_SHARED=1: plainly, and with -fsanitize=address,undefined; each runs as its own process.  It writes
   every case's inputs and results to a file, and tests/plan_ekf_ref.py must reproduce the results from the inputs bit for bit -- with f
   and jac from the host build of the plant probe (tests/plant_probe.py: the same model structs in the kernels' own sin / cos, the
   arithmetic of the device; pyapi.model_eval keeps the host libm, whose sine may differ in the last place).
2. On the LTI model the EKF is the Kalman filter: P before and after every update is plan_kf_ref.kalman's SP / SF bit for bit, with
   K = 0 and the filter's own A = I + dt ((A - I) / dt), B = dt (B / dt), W and Wu.
3. A nonlinear case (pendulum, RK4, T = 20, ny = 1, W and Wu) against the same recursion in mpmath at 60 digits.  Measured: xh 1.698e-15
   relative to max |xh|, P 2.446e-15 relative to max |P| (plan_ekf_ref.MEASURED_REL_DEV_EKF holds the larger); 8 x that is allowed,
   floored at 1e-15: the margin is for the different conditioning of other seeds.
4. Consistency: an LTI loop simulated with true noise of the filter's W and v, B = 64, T = 200, ny = 2: the pooled mean of nis / ny lies
   within 6 standard errors (sqrt(2 / ny / n)) of 1.
No GPU; the library is used for model_eval (host code, case 3) only."""
import os
import subprocess

import numpy as np
import pytest

import plan_cov_ref as PC
import plan_ekf_ref as PE
import plan_kf_ref as PK

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
OUTPUTS = ("Xh", "P", "nis", "info")


def build_exe(kind):
    exe = os.path.join(BUILD, "test_ekf_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_ekf.cpp")
    csrc = os.path.join(REPO, "cddp-cpp_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("ekf.hpp", "plan_kf.hpp", "plan_cov.hpp", "dev_models.hpp", "dev_trig.hpp", "dev_linalg.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src, __file__] + hdrs):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-DCDDP_TRIG_SHARED=1", "-Wno-unknown-pragmas"] + FLAGS[kind] + [src, "-o", exe])
    return exe


def parse(path):
    cases = []
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if w[0] == "case":
                cases.append({"dims": tuple(int(x) for x in w[1:])})
            else:
                assert int(w[1]) == len(w) - 2, w[0]
                cases[-1][w[0]] = np.array([float.fromhex(x) for x in w[2:]])
    return cases


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_step_bodies_match_the_restatement(kind, tmp_path):
    import plant_probe as PP
    H = PP.host(tmp_path)
    out_file = str(tmp_path / ("ekf_%s.txt" % kind))
    out = subprocess.run([build_exe(kind), out_file], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ekf: ok (12 cases)" in out.stdout
    cases = parse(out_file)
    assert len(cases) == 12 and sorted({c["dims"][1] for c in cases}) == [2, 4, 14]
    seen_fail = seen_drop = 0
    for c in cases:
        model, nx, nu, ny, B, T, integ, have_w, have_wu, box, dropout, failing = c["dims"]
        assert ny in (1, nx, nx + 2, 16)
        tag = {0: "pendulum", 1: "cartpole", 7: "manip7"}[model]
        assert PP.BY_TAG[tag].dt == float(c["dt"][0]) and PP.BY_TAG[tag].id == model
        m = PE.ProbeModel(PP, H, tag, integ, list(c["params"]), c["lower"] if box else None, c["upper"] if box else None)
        f = PE.Filter(m, B, c["C"].reshape(ny, nx), c["v"], c["W"].reshape(nx, nx) if have_w else None, c["Wu"].reshape(nu, nu) if have_wu else None)
        P0 = c["P0"].reshape(B, nx, nx)
        assert not PE.same(PC.mirror(P0), P0)                              # junk above the diagonal
        f.reset(c["xh0"].reshape(B, nx), P0)
        r = f.run(c["Y"].reshape(B, T + 1, ny), c["U"].reshape(B, T, nu), skip_nan=bool(dropout))
        for k in OUTPUTS:
            assert PE.same(np.asarray(r[k], dtype=np.float64).reshape(-1), c[k]), (c["dims"], k)
        assert PE.same(f.xh.reshape(-1), c["xhN"]) and PE.same(f.P.reshape(-1), c["PN"]), c["dims"]
        assert PE.same(r["P"], np.swapaxes(r["P"], 2, 3))
        assert np.all(np.isfinite(r["Xh"][0])) and np.all(r["nis"][0] >= 0.0)
        if failing:
            seen_fail += 1
            assert list(r["info"]) == [0, 1, 0] and np.all(np.isnan(r["Xh"][1])) and np.all(np.isnan(r["P"][1])) and np.all(np.isnan(r["nis"][1]))
            assert np.all(np.isfinite(r["Xh"][2]))
        else:
            assert not r["info"].any() and np.all(np.isfinite(r["P"]))
        if dropout:
            seen_drop += 1
            assert np.isnan(c["Y"]).sum() == 2 and np.all(np.isfinite(r["nis"]))
            if ny == 1:                                                    # the one row is missing: the update is the identity
                assert PE.same(r["nis"][0, 1], 0.0)
    assert seen_fail == 3 and seen_drop == 3


LTI_A = np.array([[1.0, 0.1], [-0.2, 0.95]])
LTI_B = np.array([[0.005], [0.1]])


def test_on_the_lti_model_the_filter_is_the_kalman_filter():
    rng = np.random.default_rng(20261030)
    B, T, dt = 3, 6, 0.1
    for ny in (1, 2, 4):
        m = PE.LtiModel(LTI_A, LTI_B, dt)
        C = rng.standard_normal((ny, 2)); v = 0.05 + rng.random(ny)
        W = PC.spd(rng, 2, 0.05); Wu = PC.spd(rng, 1, 0.1); P0 = PC.spd(rng, 2)
        f = PE.Filter(m, B, C, v, W, Wu)
        f.reset(rng.standard_normal((B, 2)), P0)
        Y = rng.standard_normal((B, T + 1, ny)); U = rng.standard_normal((B, T, 1))
        before, after = [], []
        for t in range(T + 1):
            if t > 0:
                f.predict(U[:, t - 1])
            before.append(f.P.copy()); f.update(Y[:, t]); after.append(f.P.copy())
        Fx, Fu = m.jac(np.zeros((B, 2)), np.zeros((B, 1)))
        A = dt * Fx; A[:, [0, 1], [0, 1]] = A[:, [0, 1], [0, 1]] + 1.0
        Bm = dt * Fu
        stack = lambda M: np.ascontiguousarray(np.broadcast_to(M[:, None], (B, T) + M.shape[1:]))
        r = PK.kalman(stack(A), stack(Bm), np.zeros((B, T, 1, 2)), C, v, P0, W, Wu)
        assert not r["info"].any()
        assert PE.same(np.stack(before, axis=1), r["SP"]) and PE.same(np.stack(after, axis=1), r["SF"]), ny
        assert not PE.same(r["SP"], r["SF"])


def exact_pendulum_ekf(params, dt, xh0, P0, c, v, W, Wu, Y, U):
    """One trajectory, ny = 1, no box: the same recursion in mpmath at 60 digits (RK4 on the pendulum's f, A = I + dt Fx, B = dt Fu)."""
    import mpmath
    mpmath.mp.dps = 60
    mpf = lambda a: mpmath.mpf(float(a))
    length, mass, damping, gravity = (mpf(a) for a in params)
    inertia = mass * length * length
    h = mpf(dt)

    def f(x, u):
        return mpmath.matrix([x[1], (u - damping * x[1] + mass * gravity * length * mpmath.sin(x[0])) / inertia])

    x = mpmath.matrix([mpf(a) for a in xh0]); P = mpmath.matrix(np.asarray(P0).tolist())
    cm = mpmath.matrix([mpf(a) for a in c]).T; Wm = mpmath.matrix(np.asarray(W).tolist()); wu = mpf(Wu[0, 0]); vv = mpf(v)
    xs, Ps = [], []
    for t in range(len(Y)):
        if t > 0:
            u = mpf(U[t - 1])
            A = mpmath.matrix([[1, h], [h * (gravity / length) * mpmath.cos(x[0]), 1 + h * (-damping / inertia)]])
            Bm = mpmath.matrix([0, h / inertia])
            k1 = f(x, u); k2 = f(x + (h / 2) * k1, u); k3 = f(x + (h / 2) * k2, u); k4 = f(x + h * k3, u)
            x = x + (h / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
            P = A * P * A.T + Wm + Bm * wu * Bm.T
        hv = P * cm.T
        s = vv + (cm * hv)[0]
        g = hv / s
        x = x + g * (mpf(Y[t]) - (cm * x)[0])
        P = P - g * hv.T - hv * g.T + s * g * g.T
        xs.append(x.copy()); Ps.append(P.copy())
    return xs, Ps


def test_nonlinear_case_against_exact_evaluation(api):
    import mpmath
    rng = np.random.default_rng(20261031)
    params, dt, T = [0.5, 1.0, 0.01, 9.81], 0.02, 20
    m = PE.HostModel(api, api.MODEL_PENDULUM, api.RK4, dt, 2, 1, params)
    c = rng.standard_normal((1, 2)); v = np.array([0.07])
    W = PC.spd(rng, 2, 0.01); Wu = PC.spd(rng, 1, 0.05); P0 = PC.spd(rng, 2, 0.3)
    xh0 = np.array([[0.4, -0.2]]); Y = 0.3 * rng.standard_normal((1, T + 1, 1)); U = 0.5 * rng.standard_normal((1, T, 1))
    f = PE.Filter(m, 1, c, v, W, Wu)
    f.reset(xh0, P0)
    r = f.run(Y, U)
    assert r["info"][0] == 0
    xs, Ps = exact_pendulum_ekf(params, dt, xh0[0], P0, c[0], v[0], W, Wu, Y[0, :, 0], U[0, :, 0])
    dev = {}
    for name, got, ex in (("xh", r["Xh"][0], xs), ("P", r["P"][0].reshape(T + 1, 4), Ps)):
        worst = big = mpmath.mpf(0)
        for t in range(T + 1):
            flat = [ex[t][i, j] for i in range(ex[t].rows) for j in range(ex[t].cols)]
            for i, exact in enumerate(flat):
                worst = max(worst, abs(mpmath.mpf(float(got[t].reshape(-1)[i])) - exact)); big = max(big, abs(exact))
        dev[name] = float(worst / big)
    allowed = max(8.0 * PE.MEASURED_REL_DEV_EKF, 1e-15)
    print("exact: pendulum RK4 T = %d: xh %.3e  P %.3e  (recorded %.3e, allowed %.3e)" % (T, dev["xh"], dev["P"], PE.MEASURED_REL_DEV_EKF, allowed))
    assert max(dev.values()) <= allowed


def test_normalised_innovation_is_consistent():
    rng = np.random.default_rng(20261032)
    B, T, ny, dt = 64, 200, 2, 0.1
    m = PE.LtiModel(LTI_A, LTI_B, dt)
    C = np.array([[1.0, 0.0], [0.3, 1.0]]); v = np.array([0.04, 0.09])
    W = np.array([[0.02, 0.005], [0.005, 0.03]]); P0 = np.array([[0.5, 0.1], [0.1, 0.4]])
    Lw = np.linalg.cholesky(W); L0 = np.linalg.cholesky(P0)
    xh0 = rng.standard_normal((B, 2))
    x = xh0 + rng.standard_normal((B, 2)) @ L0.T
    U = 0.2 * rng.standard_normal((B, T, 1))
    Y = np.zeros((B, T + 1, ny))
    for t in range(T + 1):
        if t > 0:
            x = m.step(x, U[:, t - 1]) + rng.standard_normal((B, 2)) @ Lw.T
        Y[:, t] = x @ C.T + rng.standard_normal((B, ny)) * np.sqrt(v)
    f = PE.Filter(m, B, C, v, W)
    f.reset(xh0, P0)
    r = f.run(Y, U)
    assert not r["info"].any()
    n = r["nis"].size
    mean = float(np.mean(r["nis"] / ny)); se = float(np.sqrt(2.0 / ny / n))
    print("consistency: pooled mean of nis / ny = %.5f over %d samples, standard error %.5f: %.2f se from 1" % (mean, n, se, (mean - 1.0) / se))
    assert abs(mean - 1.0) <= 6.0 * se
