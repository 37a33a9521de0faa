"""The step bodies of the plan-covariance kernel (cddp-cpp_amd/csrc/plan_cov.hpp) on the host, and the numpy restatement the GPU tests use.

1. tests/cpp/test_plan_cov.cpp, a stand-alone program, runs the bodies on fixed pseudo-random stacks for the pairs (1,1), (3,2), (4,1),
   (14,7), with and without W / Wu, full and diagonal output, and compares bit for bit with the sums of include/cddp_hip.h written out
   longhand.  Built twice with g++ -ffp-contract=off: plainly, and with -fsanitize=address,undefined; each runs as its own process.  It
   writes every case's inputs and results to a file, and tests/plan_cov_ref.py must reproduce the results from the inputs bit for bit.
2. The restatement against exact evaluation: the closed form Sigma_t = Phi_t Sigma0 Phi_t^T + sum_s Phi_{t,s} (W + B_s Wu B_s^T) Phi_{t,s}^T
   and the trace formula of the expected cost increase, in mpmath at 60 digits, on contractive synthetic stacks.  The largest deviations
   over the four pairs were measured as plan_cov_ref.MEASURED_REL_DEV (Sigma_t, relative to max |Sigma_t|) and MEASURED_REL_DEV_COST (the
   cost, relative to the cost)
   (profiles/r17_plan_covariance.md); 8 x that is allowed -- the margin covers other seeds of the same generator, not an error in a
   formula, which shows as many orders of magnitude.
No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import plan_cov_ref as PC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
PAIRS = [(1, 1), (3, 2), (4, 1), (14, 7)]


def build_exe(kind):
    exe = os.path.join(BUILD, "test_plan_cov_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plan_cov.cpp")
    hdr = os.path.join(REPO, "cddp-cpp_amd", "csrc", "plan_cov.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in (src, hdr, __file__)):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + FLAGS[kind] + [src, "-o", exe])
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
    out_file = str(tmp_path / ("plan_cov_%s.txt" % kind))
    out = subprocess.run([build_exe(kind), out_file], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan cov: ok" in out.stdout
    cases = parse(out_file)
    assert len(cases) == 8 * len(PAIRS) and sorted({c["dims"][:2] for c in cases}) == PAIRS
    seen = set()
    for c in cases:
        nx, nu, N, have_w, have_wu, diag = c["dims"]
        seen.add((have_w, have_wu, diag))
        A = c["A"].reshape(1, N, nx, nx); Bm = c["B"].reshape(1, N, nx, nu); K = c["K"].reshape(1, N, nu, nx)
        SX, SU, dc = PC.covariance(A, Bm, K, c["S0"].reshape(nx, nx), c["W"].reshape(nx, nx) if have_w else None,
                                   c["Wu"].reshape(nu, nu) if have_wu else None, c["Q"].reshape(nx, nx), c["R"].reshape(nu, nu), c["Qf"].reshape(nx, nx),
                                   diag=bool(diag))
        assert PC.same(SX.reshape(-1), c["SX"]), (c["dims"], "SX")
        assert PC.same(SU.reshape(-1), c["SU"]), (c["dims"], "SU")
        assert PC.same(dc, c["dc"]), (c["dims"], "dcost")
        assert np.abs(c["SX"]).max() > 0 and np.abs(c["SU"]).max() > 0
    assert len(seen) == 8


def exact_deviation(nx, nu, N, seed, have_w, have_wu):
    """(largest |Sigma_t - exact| / max |Sigma_t|, |dcost - exact| / |exact|) of the restatement on one contractive trajectory"""
    import mpmath
    mpmath.mp.dps = 60
    rng = np.random.default_rng(seed)
    A, Bm, K = PC.contractive_stacks(1, N, nx, nu, seed)
    S0 = PC.spd(rng, nx); W = PC.spd(rng, nx, 0.05) if have_w else None; Wu = PC.spd(rng, nu, 0.1) if have_wu else None
    Q = PC.spd(rng, nx); R = PC.spd(rng, nu); Qf = PC.spd(rng, nx, 3.0)
    SX, SU, dc = PC.covariance(A, Bm, K, S0, W, Wu, Q, R, Qf)
    mp = lambda M: mpmath.matrix(np.asarray(M).tolist())
    Acl = [mp(A[0, t]) + mp(Bm[0, t]) * mp(K[0, t]) for t in range(N)]
    S0m = mp(PC.mirror(S0))
    noise = []
    for s in range(N):
        V = mpmath.zeros(nx, nx)
        if have_w:
            V = V + mp(PC.mirror(W))
        if have_wu:
            V = V + mp(Bm[0, s]) * mp(PC.mirror(Wu)) * mp(Bm[0, s]).T
        noise.append(V)
    exact = []
    for t in range(N + 1):
        Phi = mpmath.eye(nx)
        for s in range(t):
            Phi = Acl[s] * Phi
        Sig = Phi * S0m * Phi.T
        for s in range(t):                      # Phi_{t,s} = Acl_{t-1} ... Acl_{s+1}
            P = mpmath.eye(nx)
            for r in range(s + 1, t):
                P = Acl[r] * P
            Sig = Sig + P * noise[s] * P.T
        exact.append(Sig)
    scale = float(np.abs(SX).max())
    dev = 0.0
    for t in range(N + 1):
        for i in range(nx):
            for j in range(nx):
                dev = max(dev, float(abs(mpmath.mpf(float(SX[0, t, i, j])) - exact[t][i, j])) / scale)
    tr = lambda M, S: sum(M[i, j] * S[i, j] for i in range(M.rows) for j in range(M.cols))
    cost = mpmath.mpf(0)
    for t in range(N):
        SUt = mp(K[0, t]) * exact[t] * mp(K[0, t]).T
        if have_wu:
            SUt = SUt + mp(PC.mirror(Wu))
        cost += tr(mp(Q), exact[t]) + tr(mp(R), SUt)
    cost += tr(mp(Qf), exact[N])
    return dev, float(abs(mpmath.mpf(float(dc[0])) - cost) / abs(cost))


def test_restatement_against_exact_evaluation():
    worst = worst_cost = 0.0
    for nx, nu in PAIRS:
        for have_w, have_wu in ((False, False), (True, True)):
            dev, dcost_dev = exact_deviation(nx, nu, 5, 20261700 + 16 * nx + nu, have_w, have_wu)
            print("exact: (%d, %d) W %d Wu %d: Sigma %.3e  dcost %.3e" % (nx, nu, have_w, have_wu, dev, dcost_dev))
            worst = max(worst, dev); worst_cost = max(worst_cost, dcost_dev)
    print("exact: Sigma: largest deviation / max |Sigma_t| %.3e, allowed %.3e; dcost: largest relative deviation %.3e, allowed %.3e"
          % (worst, 8.0 * PC.MEASURED_REL_DEV, worst_cost, 8.0 * PC.MEASURED_REL_DEV_COST))
    assert worst <= 8.0 * PC.MEASURED_REL_DEV
    assert worst_cost <= 8.0 * PC.MEASURED_REL_DEV_COST
