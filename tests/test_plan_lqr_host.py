"""The step bodies of the gain-design kernel (cddp-cpp_amd/csrc/plan_lqr.hpp) on the host, and the numpy restatement the GPU tests use.

1. tests/cpp/test_plan_lqr.cpp, a stand-alone program, runs the bodies on fixed pseudo-random stacks for the pairs (1,1), (3,2), (4,1),
   (14,7), with shared and per-trajectory weights and with one trajectory whose R is negative definite (the failure path), and compares
   bit for bit with the sums of include/cddp_hip.h written out longhand.  Built twice with g++ -ffp-contract=off: plainly, and with
   -fsanitize=address,undefined; each runs as its own process.  It writes every case's inputs and results to a file, and
   tests/plan_lqr_ref.py must reproduce the results from the inputs bit for bit.
2. The restatement against exact evaluation: the same recursion in mpmath at 60 digits on plan_cov_ref.contractive_stacks with spd
   weights, N = 5.  The largest deviations over the four pairs were measured as plan_lqr_ref.MEASURED_REL_DEV_K (relative to max |K|) and
   MEASURED_REL_DEV_P (relative to max |P|) (profiles/r20_plan_tvlqr.md); 8 x that is allowed -- the margin covers other seeds of the same
   generator, not an error in a formula, which shows as many orders of magnitude.
3. Two identities on the restatements: dx0^T P_0 dx0 is the closed-loop quadratic cost of the plan_jvp recursion run with K_lqr, and
   tr(P_0 Sigma0) is plan_cov_ref.covariance's dcost without noise under the same gains and weights; on the synthetic stacks and on the
   constant stacks of the LTI problem of the GPU test.  MEASURED_REL_DEV_IDENTITY is the largest of |left - exact|, |right - exact| and
   |left - right| over both identities, relative to the exact (mpmath) value; 8 x that is allowed.
No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import plan_cov_ref as PC
import plan_lqr_ref as PL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
PAIRS = [(1, 1), (3, 2), (4, 1), (14, 7)]


def build_exe(kind):
    exe = os.path.join(BUILD, "test_plan_lqr_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plan_lqr.cpp")
    hdr = os.path.join(REPO, "cddp-cpp_amd", "csrc", "plan_lqr.hpp")
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
    out_file = str(tmp_path / ("plan_lqr_%s.txt" % kind))
    out = subprocess.run([build_exe(kind), out_file], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan lqr: ok" in out.stdout
    cases = parse(out_file)
    assert len(cases) == 3 * len(PAIRS) and sorted({c["dims"][:2] for c in cases}) == PAIRS
    failed = 0
    for c in cases:
        nx, nu, N, B, per = c["dims"]
        lead = (B,) if per else ()
        dt = float(c["dt"][0])
        A = c["A"].reshape(B, N, nx, nx); Bm = c["B"].reshape(B, N, nx, nu)
        Q = c["Q"].reshape(lead + (nx, nx)); R = c["R"].reshape(lead + (nu, nu)); Qf = c["Qf"].reshape(lead + (nx, nx))
        assert nx == 1 or not PL.same(PC.mirror(Q), Q)                 # junk above the diagonal
        K, P, info = PL.tvlqr(A, Bm, Q * dt, R * dt, Qf)
        assert PL.same(K.reshape(-1), c["K"]), (c["dims"], "K")
        assert PL.same(P.reshape(-1), c["P"]), (c["dims"], "P")
        assert PL.same(info.astype(np.float64), c["info"]), (c["dims"], "info")
        assert np.abs(K[0]).max() > 0 and np.all(np.isfinite(P[0]))
        if info.any():
            failed += 1
            assert list(info) == [0, N] and np.all(K[1] == 0.0) and np.all(np.isnan(P[1, :N])) and np.all(np.isfinite(P[1, N]))
    assert failed == len(PAIRS)


def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def exact_recursion(A, Bm, Qd, Rd, Qf):
    """One trajectory, A (N, nx, nx), Bm (N, nx, nu), symmetric weights: (K_t list, P_t list) in mpmath at 60 digits"""
    mpmath = _mp()
    mp = lambda M: mpmath.matrix(np.asarray(M).tolist())
    N = A.shape[0]
    Qd, Rd = mp(Qd), mp(Rd)
    P = [None] * (N + 1); K = [None] * N
    P[N] = mp(Qf)
    for t in range(N - 1, -1, -1):
        At, Bt = mp(A[t]), mp(Bm[t])
        K[t] = -(mpmath.inverse(Rd + Bt.T * P[t + 1] * Bt) * (Bt.T * P[t + 1] * At))
        Acl = At + Bt * K[t]
        P[t] = Qd + K[t].T * Rd * K[t] + Acl.T * P[t + 1] * Acl
    return K, P


def deviations(A, Bm, Qd, Rd, Qf, Sigma0, dx0):
    """(K, P, identity) deviations of the restatement on ONE trajectory: A (1, N, nx, nx), Bm (1, N, nx, nu)"""
    mpmath = _mp()
    nx, nu, N = A.shape[2], Bm.shape[3], A.shape[1]
    K, P, info = PL.tvlqr(A, Bm, Qd, Rd, Qf)
    assert info[0] == 0
    Ke, Pe = exact_recursion(A[0], Bm[0], PC.mirror(Qd), PC.mirror(Rd), PC.mirror(Qf))
    f = lambda x: mpmath.mpf(float(x))
    dK = max(float(abs(f(K[0, t, k, j]) - Ke[t][k, j])) for t in range(N) for k in range(nu) for j in range(nx)) / float(np.abs(K).max())
    dP = max(float(abs(f(P[0, t, i, j]) - Pe[t][i, j])) for t in range(N + 1) for i in range(nx) for j in range(nx)) / float(np.abs(P).max())
    # identity 1: dx0^T P_0 dx0 = the closed-loop cost from dx0
    exact1 = sum(f(dx0[i]) * Pe[0][i, j] * f(dx0[j]) for i in range(nx) for j in range(nx))
    left1 = float(dx0 @ P[0, 0] @ dx0)
    right1 = float(PL.closed_loop_cost(A, Bm, K, dx0[None], Qd, Rd, Qf)[0])
    # identity 2: tr(P_0 Sigma0) = the expected cost increase without noise
    S0 = PC.mirror(Sigma0)
    exact2 = sum(Pe[0][i, j] * f(S0[i, j]) for i in range(nx) for j in range(nx))
    left2 = float(np.sum(P[0, 0] * S0))
    right2 = float(PC.covariance(A, Bm, K, Sigma0, None, None, PC.mirror(Qd), PC.mirror(Rd), PC.mirror(Qf))[2][0])
    ident = 0.0
    for ex, l, r in ((exact1, left1, right1), (exact2, left2, right2)):
        ident = max(ident, float(abs(f(l) - ex) / abs(ex)), float(abs(f(r) - ex) / abs(ex)), float(abs(f(l) - f(r)) / abs(ex)))
    return dK, dP, ident


def synthetic(nx, nu, N, seed):
    rng = np.random.default_rng(seed)
    A, Bm, _ = PC.contractive_stacks(1, N, nx, nu, seed)
    return A, Bm, PC.spd(rng, nx), PC.spd(rng, nu), PC.spd(rng, nx, 3.0), PC.spd(rng, nx), rng.standard_normal(nx)


def lti_case(api, seed):
    from test_plan_sens import lti_problem
    p = lti_problem(api, 5, 5)
    rng = np.random.default_rng(seed)
    A, Bm = PL.lti_stacks(p, 1)
    Qd, Rd, Qf = PC.cost_matrices(p)
    return A, Bm, Qd, Rd, Qf, PC.spd(rng, p.nx), rng.standard_normal(p.nx)


def test_restatement_against_exact_evaluation():
    worst_k = worst_p = 0.0
    for nx, nu in PAIRS:
        dK, dP, _ = deviations(*synthetic(nx, nu, 5, 20262000 + 16 * nx + nu))
        print("exact: (%d, %d): K %.3e  P %.3e" % (nx, nu, dK, dP))
        worst_k = max(worst_k, dK); worst_p = max(worst_p, dP)
    print("exact: K: largest deviation / max |K| %.3e, allowed %.3e; P: largest deviation / max |P| %.3e, allowed %.3e"
          % (worst_k, 8.0 * PL.MEASURED_REL_DEV_K, worst_p, 8.0 * PL.MEASURED_REL_DEV_P))
    assert worst_k <= 8.0 * PL.MEASURED_REL_DEV_K
    assert worst_p <= 8.0 * PL.MEASURED_REL_DEV_P


def test_two_identities_on_the_restatements(api):
    worst = 0.0
    for nx, nu in PAIRS:
        _, _, ident = deviations(*synthetic(nx, nu, 5, 20262000 + 16 * nx + nu))
        print("identities: (%d, %d): %.3e" % (nx, nu, ident))
        worst = max(worst, ident)
    _, _, ident = deviations(*lti_case(api, 20262100))
    print("identities: LTI 2 x 1: %.3e" % ident)
    worst = max(worst, ident)
    print("identities: largest relative deviation %.3e, allowed %.3e" % (worst, 8.0 * PL.MEASURED_REL_DEV_IDENTITY))
    assert worst <= 8.0 * PL.MEASURED_REL_DEV_IDENTITY
