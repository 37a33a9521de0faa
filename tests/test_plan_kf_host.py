"""The step bodies of the filter kernel (cddp-cpp_amd/csrc/plan_kf.hpp) on the host, and the numpy restatement the GPU tests use.

1. tests/cpp/test_plan_kf.cpp, a stand-alone program, runs the bodies on fixed pseudo-random stacks for the pairs (1,1), (3,2), (4,1),
   (14,7), with shared inputs (ny = nx + 2), per-trajectory inputs (ny = 1) and per-trajectory inputs of which one trajectory's Sigma0
   is -I (the failure path), and compares bit for bit with the sums of include/cddp_hip.h written out longhand.  Built twice with
   g++ -ffp-contract=off: plainly, and with -fsanitize=address,undefined; each runs as its own process.  It writes every case's inputs
   and results to a file, and tests/plan_kf_ref.py must reproduce the results from the inputs bit for bit.
2. The restatement against exact evaluation: mpmath at 60 digits on the BATCH form -- L = Sm C^T (C Sm C^T + V)^-1, Sf = (I - L C) Sm,
   and the covariance of [dx; xhat] propagated as ONE 2 nx x 2 nx matrix, which assumes nothing about the estimate being orthogonal to
   its error -- on plan_cov_ref.contractive_stacks with spd Sigma0, W and Wu, N = 5, pairs (4,1), (3,2), (8,3), (14,7), ny in
   {1, nx, nx + 2}.  Measured (largest deviation relative to the exact maximum of the quantity; dcost relative to its exact value):
       L 4.447e-14 at (14,7) ny 1;  SX 2.555e-16 at (8,3) ny 10;  SU 4.307e-16 at (14,7) ny 14;  dcost 1.580e-16 at (4,1) ny 1
   (L = Sf C^T / v loses digits where v is small against c . h: the posterior is then a small difference of large terms).
   8 x the recorded value is allowed, and never more than 1e-12: a wrong formula is off by order one.
3. A single all-zero row of C: SF == SP == SX bitwise, SP is plan_cov_ref's SX with all gains zero, SU is Wu mirrored.
4. A perfect measurement (C = I, v = 1e-30, spd W): SX, SU and dcost agree with plan_cov_ref on the same stacks and gains.  Measured:
   3.450e-16 (SX, SU relative to their maxima, dcost relative to its value; the largest of the three over the four pairs).
5. Duality: SP of the filter on (A_t, C, W, diag v) without Wu is P of plan_lqr_ref.tvlqr on the transposed, time-reversed system
   (A^T, C^T, Qd = W, Rd = diag v, Qf = Sigma0).  Measured: 7.142e-17 relative to max |SP|.
6. Failure: a trajectory with Sigma0 = -I gets info = 1 and NaN from row 0; its neighbour is bitwise what it is without it.
No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import plan_cov_ref as PC
import plan_kf_ref as PK
import plan_lqr_ref as PL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
BODY_PAIRS = [(1, 1), (3, 2), (4, 1), (14, 7)]
PAIRS = [(4, 1), (3, 2), (8, 3), (14, 7)]
OUTPUTS = ("L", "SP", "SF", "SX", "SU", "dcost", "info")


def build_exe(kind):
    exe = os.path.join(BUILD, "test_plan_kf_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plan_kf.cpp")
    hdrs = [os.path.join(REPO, "cddp-cpp_amd", "csrc", h) for h in ("plan_kf.hpp", "plan_cov.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src, __file__] + hdrs):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"] + FLAGS[kind] + [src, "-o", exe])
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
def test_step_bodies_match_the_sums_written_out_and_the_restatement(kind, tmp_path):
    out_file = str(tmp_path / ("plan_kf_%s.txt" % kind))
    out = subprocess.run([build_exe(kind), out_file], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan kf: ok" in out.stdout
    cases = parse(out_file)
    assert len(cases) == 3 * len(BODY_PAIRS) and sorted({c["dims"][:2] for c in cases}) == BODY_PAIRS
    failed = 0
    for c in cases:
        nx, nu, ny, N, B, per, have_w, have_wu = c["dims"]
        lead = (B,) if per else ()
        A = c["A"].reshape(B, N, nx, nx); Bm = c["B"].reshape(B, N, nx, nu); K = c["K"].reshape(B, N, nu, nx)
        S0 = c["Sigma0"].reshape(lead + (nx, nx))
        assert nx == 1 or not PK.same(PC.mirror(S0), S0)                 # junk above the diagonal
        r = PK.kalman(A, Bm, K, c["C"].reshape(lead + (ny, nx)), c["v"].reshape(lead + (ny,)), S0,
                      c["W"].reshape(lead + (nx, nx)) if have_w else None, c["Wu"].reshape(lead + (nu, nu)) if have_wu else None,
                      c["Qdt"].reshape(nx, nx), c["Rdt"].reshape(nu, nu), c["Qf"].reshape(nx, nx))
        for k in OUTPUTS:
            assert PK.same(np.asarray(r[k], dtype=np.float64).reshape(-1), c[k]), (c["dims"], k)
        assert np.all(np.isfinite(r["SX"][0])) and np.abs(r["L"][0]).max() > 0
        assert PK.same(r["SX"], np.swapaxes(r["SX"], 2, 3)) and PK.same(r["SF"], np.swapaxes(r["SF"], 2, 3))
        if r["info"].any():
            failed += 1
            assert list(r["info"]) == [0, 1] and all(np.all(np.isnan(r[k][1])) for k in OUTPUTS[:6])
    assert failed == len(BODY_PAIRS)


def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def exact_batch_form(A, Bm, K, C, v, Sigma0, W, Wu, Qdt, Rdt, Qf):
    """One trajectory, symmetric inputs: (L_t, SX_t, SU_t lists, dcost) in mpmath at 60 digits, by the batch-form filter and the covariance
    of z = [dx; xhat] as one matrix: z_t = M_t z_t^- + [0; L_t] n_t, z_{t+1}^- = F_t z_t + [B eps + w; 0]."""
    mpmath = _mp()
    mp = lambda M: mpmath.matrix(np.asarray(M).tolist())
    N, nx, nu = A.shape[0], A.shape[1], Bm.shape[2]
    Cm, V = mp(C), mpmath.diag([mpmath.mpf(float(x)) for x in v])
    Wm = mp(W) if W is not None else mpmath.zeros(nx); Wum = mp(Wu) if Wu is not None else mpmath.zeros(nu)
    I = mpmath.eye(nx)

    def block(a, b, c, d):
        M = mpmath.zeros(2 * nx)
        M[:nx, :nx] = a; M[:nx, nx:] = b; M[nx:, :nx] = c; M[nx:, nx:] = d
        return M

    def tr(Q, M):
        return sum(mpmath.mpf(float(Q[i, j])) * M[i, j] for i in range(Q.shape[0]) for j in range(Q.shape[1]))

    Sm = mp(Sigma0)
    Pm = block(Sm, mpmath.zeros(nx), mpmath.zeros(nx), mpmath.zeros(nx))
    Ls, SXs, SUs, dcost = [], [], [], mpmath.mpf(0)
    for t in range(N + 1):
        L = Sm * Cm.T * mpmath.inverse(Cm * Sm * Cm.T + V)
        Sf = (I - L * Cm) * Sm
        M = block(I, mpmath.zeros(nx), L * Cm, I - L * Cm)
        P = M * Pm * M.T + block(mpmath.zeros(nx), mpmath.zeros(nx), mpmath.zeros(nx), L * V * L.T)
        Ls.append(L); SXs.append(P[:nx, :nx])
        if t == N:
            dcost += tr(Qf, P[:nx, :nx])
            break
        At, Bt, Kt = mp(A[t]), mp(Bm[t]), mp(K[t])
        SU = Kt * P[nx:, nx:] * Kt.T + Wum
        SUs.append(SU)
        dcost += tr(Qdt, P[:nx, :nx]) + tr(Rdt, SU)
        noise = Wm + Bt * Wum * Bt.T
        F = block(At, Bt * Kt, mpmath.zeros(nx), At + Bt * Kt)
        Pm = F * P * F.T + block(noise, mpmath.zeros(nx), mpmath.zeros(nx), mpmath.zeros(nx))
        Sm = At * Sf * At.T + noise
    return Ls, SXs, SUs, dcost


def synthetic(nx, nu, ny, N, seed):
    rng = np.random.default_rng(seed)
    A, Bm, K = PC.contractive_stacks(1, N, nx, nu, seed)
    C = rng.standard_normal((ny, nx)); v = 0.05 + rng.random(ny)
    Q = PC.spd(rng, nx, 0.1); R = PC.spd(rng, nu, 0.05); Qf = PC.spd(rng, nx, 3.0)
    return A, Bm, K, C, v, PC.spd(rng, nx), PC.spd(rng, nx, 0.05), PC.spd(rng, nu, 0.1), Q, R, Qf


def rel_dev(got, exact_list):
    """largest |got - exact| over all elements, relative to the exact maximum"""
    mpmath = _mp()
    worst = big = mpmath.mpf(0)
    for t, E in enumerate(exact_list):
        for i in range(E.rows):
            for j in range(E.cols):
                worst = max(worst, abs(mpmath.mpf(float(got[t, i, j])) - E[i, j])); big = max(big, abs(E[i, j]))
    return float(worst / big)


def allowed(measured):
    assert measured is not None and measured > 0
    return min(8.0 * measured, PK.CAP)


def test_restatement_against_exact_evaluation():
    mpmath = _mp()
    worst = {"L": 0.0, "SX": 0.0, "SU": 0.0, "dcost": 0.0}
    for nx, nu in PAIRS:
        for ny in (1, nx, nx + 2):
            A, Bm, K, C, v, S0, W, Wu, Q, R, Qf = synthetic(nx, nu, ny, 5, 20262100 + 64 * nx + 4 * nu + ny)
            r = PK.kalman(A, Bm, K, C, v, S0, W, Wu, Q, R, Qf)
            assert r["info"][0] == 0
            Le, SXe, SUe, dce = exact_batch_form(A[0], Bm[0], K[0], C, v, S0, W, Wu, Q, R, Qf)
            d = {"L": rel_dev(r["L"][0], Le), "SX": rel_dev(r["SX"][0], SXe), "SU": rel_dev(r["SU"][0], SUe),
                 "dcost": float(abs(mpmath.mpf(float(r["dcost"][0])) - dce) / abs(dce))}
            print("exact: (%d, %d) ny %d: " % (nx, nu, ny) + "  ".join("%s %.3e" % kv for kv in d.items()))
            for k in worst:
                worst[k] = max(worst[k], d[k])
    rec = {"L": PK.MEASURED_REL_DEV_L, "SX": PK.MEASURED_REL_DEV_SX, "SU": PK.MEASURED_REL_DEV_SU, "dcost": PK.MEASURED_REL_DEV_COST}
    print("exact: largest relative deviations: " + "  ".join("%s %.3e (allowed %.3e)" % (k, worst[k], allowed(rec[k])) for k in worst))
    for k in worst:
        assert worst[k] <= allowed(rec[k]), k


def test_zero_measurement_is_no_measurement():
    for nx, nu in PAIRS:
        A, Bm, K, _, _, S0, W, Wu, Q, R, Qf = synthetic(nx, nu, 1, 5, 20262300 + 16 * nx + nu)
        A = np.repeat(A, 2, axis=0); Bm = np.repeat(Bm, 2, axis=0); K = np.repeat(K, 2, axis=0)
        r = PK.kalman(A, Bm, K, np.zeros((1, nx)), np.array([0.3]), S0, W, Wu, Q, R, Qf)
        assert np.all(r["info"] == 0) and np.all(r["L"] == 0.0)
        assert PK.same(r["SF"], r["SP"]) and PK.same(r["SX"], r["SP"])
        open_loop = PC.covariance(A, Bm, np.zeros_like(K), S0, W, Wu)[0]
        assert PK.same(r["SP"], open_loop)
        assert PK.same(r["SU"], np.broadcast_to(PC.mirror(Wu), r["SU"].shape))


def test_perfect_measurement_is_state_feedback():
    worst = 0.0
    for nx, nu in PAIRS:
        A, Bm, K, _, _, S0, W, Wu, Q, R, Qf = synthetic(nx, nu, nx, 5, 20262400 + 16 * nx + nu)
        r = PK.kalman(A, Bm, K, np.eye(nx), np.full(nx, 1e-30), S0, W, Wu, Q, R, Qf)
        assert r["info"][0] == 0
        SX, SU, dc = PC.covariance(A, Bm, K, S0, W, Wu, Q, R, Qf)
        d = max(np.abs(r["SX"] - SX).max() / np.abs(SX).max(), np.abs(r["SU"] - SU).max() / np.abs(SU).max(), abs(r["dcost"][0] - dc[0]) / abs(dc[0]))
        print("perfect measurement: (%d, %d): %.3e" % (nx, nu, d))
        worst = max(worst, float(d))
    print("perfect measurement: largest relative deviation %.3e, allowed %.3e" % (worst, allowed(PK.MEASURED_REL_DEV_PERFECT)))
    assert worst <= allowed(PK.MEASURED_REL_DEV_PERFECT)


def test_duality_with_the_lqr_restatement():
    worst = 0.0
    for nx, nu in PAIRS:
        for ny in (1, nx, nx + 2):
            A, Bm, K, C, v, S0, W, _, _, _, _ = synthetic(nx, nu, ny, 5, 20262500 + 64 * nx + 4 * nu + ny)
            N = A.shape[1]
            SP = PK.kalman(A, Bm, K, C, v, S0, W, None)["SP"]
            At = np.ascontiguousarray(np.swapaxes(A[:, ::-1], 2, 3))                        # A_lqr[s] = A_{N-1-s}^T
            Ct = np.ascontiguousarray(np.broadcast_to(C.T, (1, N, nx, ny)))                 # B_lqr = C^T
            _, P, info = PL.tvlqr(At, Ct, W, np.diag(v), S0)
            assert info[0] == 0
            d = float(np.abs(SP[0] - P[0, ::-1]).max() / np.abs(SP).max())                  # SP_t = P_{N-t}: the sequence BEFORE the measurement
            print("duality: (%d, %d) ny %d: %.3e" % (nx, nu, ny, d))
            worst = max(worst, d)
    print("duality: largest relative deviation %.3e, allowed %.3e" % (worst, allowed(PK.MEASURED_REL_DEV_DUALITY)))
    assert worst <= allowed(PK.MEASURED_REL_DEV_DUALITY)


def test_failure_of_one_trajectory():
    nx, nu, ny, N = 4, 1, 3, 5
    A, Bm, K, C, v, S0, W, Wu, Q, R, Qf = synthetic(nx, nu, ny, N, 20262600)
    A = np.repeat(A, 2, axis=0); Bm = np.repeat(Bm, 2, axis=0); K = np.repeat(K, 2, axis=0)
    per = lambda M: np.ascontiguousarray(np.broadcast_to(M, (2,) + M.shape))
    good = PK.kalman(A, Bm, K, per(C), per(v), per(S0), per(W), per(Wu), Q, R, Qf)
    assert np.all(good["info"] == 0)
    S0b = per(S0).copy(); S0b[1] = -np.eye(nx)
    vb = per(v).copy(); vb[1] = 1e-3                                            # (s = v - |c|^2 < 0 for the first row)
    bad = PK.kalman(A, Bm, K, per(C), vb, S0b, per(W), per(Wu), Q, R, Qf)
    assert list(bad["info"]) == [0, 1]
    for k in OUTPUTS[:6]:
        assert np.all(np.isnan(bad[k][1])), k
        assert PK.same(bad[k][0], good[k][0]), k
