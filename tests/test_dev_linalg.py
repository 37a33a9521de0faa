"""The per-lane linear algebra of cddp-cpp_amd/csrc/dev_linalg.hpp and the lane-shared LDLT / Jacobi of kernels_te.hpp, each routine run BY
ITSELF on the GPU through the probe library (tests/hip/dev_probe.hip) and compared with references that share no code with it:
mpmath (60 digits, on the float64 inputs) for values, the numpy twin's EigenLDLT for pivot order, the info flag and D^+.

The case sets (tests/dev_probe.py, fixed seeds) are there for the branches the solver-level tests never reach: zero and sub-DBL_MIN
pivots, a non-zero pivot after a zero one, the all-zero-diagonal early return, pivot sequences that differ between the lane groups
of one wavefront, run-time sizes below NMAX, ragged last wavefronts.  Every set has a CPU test that runs the HOST build of the same
case bodies against the same references and bounds and asserts that the set reaches its branches (counts are printed).

What is exact: ok, the transpositions, signs, sign_of_reduction / dmax / dmin; every value between the device and the host build
(the routines use + - * / sqrt and comparisons only, both builds without contraction); the cooperative LDLT against
LDLTd<PM>, ldlt_lds_solve against LDLTs::solve and the singular-value instantiations against each other.  "Bit-equal" here is
dev_probe.same_numbers: the same bits for every non-zero number and infinity; -0.0 counts as +0.0 (-fno-signed-zeros) and any NaN
as any NaN.
What is bounded: values against mpmath, by 4 x the worst error the independent double-precision reference (twin EigenLDLT,
numpy.linalg.inv / eigvalsh / svd) reaches on the same committed case set; both numbers stand next to each constant."""
import math
from fractions import Fraction

import numpy as np
import pytest
import mpmath as mp

import dev_probe as P

NS = (1, 2, 3, 4, 7)                                        # the NU values the product instantiates
DYN = {8: (0, 1, 2, 5, 8), 16: (0, 1, 2, 9, 14, 16)}        # LDLTd<kPTS>, LDLTd<kPTMax> at run-time sizes
COOP = ((4, 2), (8, 6), (16, 14))                           # (G, PM): TeCfg of the pendulum, 3-DOF arm, 7-joint arm terminal layouts

# Normwise backward error of the solve, |Ax - b|_inf / (|A|_inf |x|_inf + |b|_inf), and of the factorisation,
# |P A P^T - L D L^T|_inf / |A|_inf, per family: (worst value of the twin's EigenLDLT over every case set of this module, bound = 4 x).
# Diagonal-pivoted LDLT is not backward stable on indefinite input, hence the larger figures there.
# (measured on the host build of the routines, for the record: solve 2.2e-14 / factor 1.8e-14 on "indefinite", <= 1.1e-16 elsewhere;
#  test_ldlt_reference_figures re-measures the twin's column)
LDLT_TWIN_SOLVE = {"spd": 9.27e-17, "indefinite": 1.60e-14, "illcond": 5.31e-17, "ties": 1.40e-16, "triangles": 6.26e-17,
                   "rankdef": 5.54e-17, "subnormal": 6.05e-17, "subnormal_above": 3.18e-17}
LDLT_TWIN_FACTOR = {"spd": 7.96e-17, "indefinite": 6.58e-15, "illcond": 7.41e-17, "ties": 9.79e-17, "triangles": 8.05e-17,
                    "rankdef": 7.04e-17, "subnormal": 6.46e-17, "subnormal_above": 0.0}     # (1 x 1: the factor is the entry)
LDLT_SOLVE_BOUND = {k: (v, 4.0 * v) for k, v in LDLT_TWIN_SOLVE.items()}
LDLT_FACTOR_BOUND = {k: (v, 4.0 * v) for k, v in LDLT_TWIN_FACTOR.items()}
EXACT_FAMILIES = ("zero", "rankdef_dense", "empty", "zerodiag_upper_only")         # integer data, every operation exact: factor and x equal the twin's bit for bit


def _seed(n):
    return 1000 + n


def _ldlt_sets():
    """(entry point, NMAX, n) -> cases.  LDLTs<N> and LDLTd<N> at n = N share a set; the cooperative shapes add LDLTd<PM> at every n."""
    sets = {}
    for N in NS:
        sets[("ldlts_%d" % N, N, N)] = P.ldlt_cases(N, _seed(N))
        sets[("ldltd_%d" % N, N, N)] = P.ldlt_cases(N, _seed(N))
    for nmax, ns in DYN.items():
        for n in ns:
            sets[("ldltd_%d" % nmax, nmax, n)] = P.ldlt_cases(n, _seed(n), reps=2)
    for G, PM in COOP:
        for n in range(PM + 1):
            sets[("ldltd_%d" % PM, PM, n)] = P.ldlt_cases(n, _seed(n), reps=2)
    return sets


def _branches(c, tw):
    """Which branches of the factorisation / solve a case takes, read from the twin's factor."""
    n = c["A"].shape[0]
    d = np.diag(tw.M) if n else np.zeros(0)
    early = n >= 2 and not np.any(np.diag(c["A"]) != 0.0)
    zero_then_valid = (not early) and any(d[i] == 0.0 and np.any(d[i + 1:] != 0.0) for i in range(n))
    return dict(early_return=early, d_plus_zero=bool(np.any(d == 0.0)), d_plus_subnormal=bool(np.any((d != 0.0) & (np.abs(d) <= P.DBL_MIN))),
                zero_then_valid=zero_then_valid, not_ok=not tw.ok, late_fail=(not tw.ok) and not early and not zero_then_valid,
                swap=bool(np.any(tw.tr != np.arange(n))), zero_after_valid_ok=tw.ok and n >= 2 and d[0] != 0.0 and bool(np.any(d == 0.0)))


def _check_ldlt(cases, Y, nmax, ld=None, worst=None):
    """Records Y of one LDLT entry point against the twin (exact: ok, transpositions) and mpmath (backward errors)."""
    for i, c in enumerate(cases):
        n = c["A"].shape[0]
        ok, tr, M, x = P.ldlt_unpack(Y, i, nmax, n, ld)
        tw = P.T.EigenLDLT(c["A"])
        assert ok == tw.ok, (c["fam"], n, i)
        assert np.array_equal(tr, tw.tr), (c["fam"], n, i, tr, tw.tr)
        fam, blk = c["fam"], c["blk"]
        if fam in EXACT_FAMILIES:
            assert np.array_equal(np.tril(M), np.tril(tw.M)) and (n == 0 or np.array_equal(x, tw.solve(c["b"]))), (fam, n, i)
            continue
        if blk is None:                                      # ok false: the caller drops the factor
            continue
        assert not np.any(np.isnan(M[np.tril_indices(n)])) and not np.any(np.isnan(x)), (fam, n, i)
        out = [j for j in range(n) if j not in blk]
        assert np.all(x[out] == 0.0), (fam, n, i, x)         # D^+: the components of a zero / sub-DBL_MIN pivot are exactly 0
        es = P.solve_backward_error(P.sym_lower(c["A"])[np.ix_(blk, blk)], x[blk], c["b"][blk])
        ef = P.factor_backward_error(c["A"], tr, M)
        if worst is not None:
            w = worst.setdefault(fam, [0.0, 0.0]); w[0] = max(w[0], es); w[1] = max(w[1], ef)
        else:
            assert es <= LDLT_SOLVE_BOUND[fam][1], (fam, n, i, es, LDLT_SOLVE_BOUND[fam])
            assert ef <= LDLT_FACTOR_BOUND[fam][1], (fam, n, i, ef, LDLT_FACTOR_BOUND[fam])


def _twin_records(cases, nmax):
    """The twin's EigenLDLT in the record layout of the probe, to measure the reference's own error with _check_ldlt."""
    Y = np.zeros((1 + nmax + nmax * nmax + nmax, len(cases)))
    for i, c in enumerate(cases):
        n = c["A"].shape[0]
        tw = P.T.EigenLDLT(c["A"])
        Mf = np.zeros((nmax, nmax)); Mf[:n, :n] = tw.M
        Y[0, i] = 1.0 if tw.ok else 0.0
        Y[1:1 + n, i] = tw.tr
        Y[1 + nmax:1 + nmax + nmax * nmax, i] = Mf.ravel()
        Y[1 + nmax + nmax * nmax:1 + nmax + nmax * nmax + n, i] = tw.solve(c["b"]) if n else []
    return Y


def measure_twin_ldlt():
    """The figures behind LDLT_TWIN_SOLVE / LDLT_TWIN_FACTOR: the twin's worst (solve, factor) backward error per family."""
    worst = {}
    for (name, nmax, n), cases in _ldlt_sets().items():
        _check_ldlt(cases, _twin_records(cases, nmax), nmax, worst=worst)
    return worst


def test_ldlt_reference_figures():
    """The twin's own errors on the case sets are the figures the bounds are built from."""
    worst = measure_twin_ldlt()
    print("twin EigenLDLT worst (solve, factor) backward error per family:", worst)
    for fam, (es, ef) in worst.items():
        assert es <= LDLT_TWIN_SOLVE[fam] and ef <= LDLT_TWIN_FACTOR[fam], (fam, es, ef)   # (from above only: numpy / BLAS may improve)


def test_ldlt_case_sets_reach_their_branches():
    count = {}
    for (name, nmax, n), cases in _ldlt_sets().items():
        if not name.startswith("ldltd"):
            continue
        for c in cases:
            for k, v in _branches(c, P.T.EigenLDLT(c["A"])).items():
                count[(k, nmax)] = count.get((k, nmax), 0) + int(v)
            if n < nmax:
                count[("n_below_nmax", nmax)] = count.get(("n_below_nmax", nmax), 0) + 1
    print("LDLT branch counts (branch, NMAX):", sorted(count.items()))
    for nmax in (3, 4, 7, 8, 16, 6, 14):
        for k in ("early_return", "d_plus_zero", "d_plus_subnormal", "zero_then_valid", "late_fail", "swap", "zero_after_valid_ok"):
            assert count[(k, nmax)] > 0, (k, nmax)
    for nmax in (2, 8, 16, 6, 14):
        assert count[("early_return", nmax)] > 0 and count[("d_plus_subnormal", nmax)] > 0 and count[("swap", nmax)] > 0
    for nmax in (8, 16, 2, 6, 14):
        assert count[("n_below_nmax", nmax)] > 0
    # one wavefront of the cooperative kernel holds 64 / G consecutive cases: every one holds at least two different pivot
    # sequences, the first one an early return next to a failure at a later pivot and a non-zero pivot after a zero one
    for G, PM in COOP:
        tpw = 64 // G
        for n in range(3, PM + 1):
            cases = P.ldlt_cases(n, _seed(n), reps=2)
            for w in range(0, len(cases) - tpw + 1, tpw):
                assert len({tuple(P.T.EigenLDLT(c["A"]).tr) for c in cases[w:w + tpw]}) >= 2, (G, PM, n, w)
            br = [_branches(c, P.T.EigenLDLT(c["A"])) for c in cases[:4]]
            assert all(any(b[k] for b in br) for k in ("early_return", "late_fail", "zero_then_valid")), (G, PM, n)


def test_ldlt_host_build_against_twin_and_mpmath(tmp_path):
    lib = P.host(tmp_path)
    for (name, nmax, n), cases in _ldlt_sets().items():
        Y = P.run(lib, name, P.ldlt_pack(cases, nmax))
        _check_ldlt(cases, Y, nmax)
    for N in NS:                                             # the two per-lane forms give the same bits (CPU finding the issue records)
        cases = P.ldlt_cases(N, _seed(N))
        X = P.ldlt_pack(cases, N)
        assert P.same_numbers(P.run(lib, "ldlts_%d" % N, X), P.run(lib, "ldltd_%d" % N, X)), N
    d = np.array([2.0, -3.0, 0.0, 1e-310, P.DBL_MIN, np.nextafter(P.DBL_MIN, 1.0), -1e-310, 5.0])
    Y = P.run(lib, "ldlt1", np.stack([d, np.full(d.size, 3.0)]))
    assert np.array_equal(Y[0], [1.5, -1.0, 0.0, 0.0, 0.0, 3.0 / np.nextafter(P.DBL_MIN, 1.0), 0.0, 0.6])


@pytest.mark.gpu
def test_ldlt_per_lane_forms_on_device(api, tmp_path):
    """LDLTs<N>, LDLTd<N> at n = N, LDLTd<8> / LDLTd<16> at run-time sizes, ldlt1_solve: exact flags and transpositions against the
    twin, backward errors against mpmath, every output bit-equal to the host build."""
    dev, hst = P.device(), P.host(tmp_path)
    for (name, nmax, n), cases in _ldlt_sets().items():
        X = P.ldlt_pack(cases, nmax)
        Y = P.run(dev, name, X)
        _check_ldlt(cases, Y, nmax)
        assert P.same_numbers(Y, P.run(hst, name, X)), (name, n)
    d = np.array([2.0, -3.0, 0.0, 1e-310, P.DBL_MIN, np.nextafter(P.DBL_MIN, 1.0), -1e-310, 5.0])
    X = np.stack([d, np.full(d.size, 3.0)])
    assert P.same_numbers(P.run(dev, "ldlt1", X), P.run(hst, "ldlt1", X))


@pytest.mark.gpu
@pytest.mark.parametrize("G,PM", COOP)
def test_cooperative_ldlt_equals_the_per_lane_form(api, G, PM):
    """ldlt_mem_compute_coop<G, PM> + ldlt_mem_solve (one factorisation on the G lanes of a group, system in LDS, leading dimension
    PM + 1) against LDLTd<PM> of the lane-per-item kernel: flag, transpositions, factor and solution, exactly.  Every n from 0 to
    PM; the 64 / G groups of a wavefront hold different families (different pivot sequences, the zero-diagonal early return, a
    failure at a later pivot); batches of one group, of a ragged last wavefront and of several wavefronts."""
    dev = P.device()
    name = "ldlt_coop_%d_%d" % (G, PM)
    tpw = 64 // G
    for n in range(PM + 1):
        cases = P.ldlt_cases(n, _seed(n), reps=2)
        cases = cases * (1 if len(cases) > 2 * tpw else (2 * tpw) // len(cases) + 1)
        assert len(cases) % tpw != 0 or n < 2                # ragged last wavefront
        for sub in (cases, cases[len(cases) // 2:len(cases) // 2 + 1], cases[:tpw + 1]):
            Yc = P.run(dev, name, P.ldlt_pack(sub, PM, ld=PM + 1))
            Yl = P.run(dev, "ldltd_%d" % PM, P.ldlt_pack(sub, PM))
            for i, c in enumerate(sub):
                a, b = P.ldlt_unpack(Yc, i, PM, n, PM + 1), P.ldlt_unpack(Yl, i, PM, n)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]), (c["fam"], n, i, a[:2], b[:2])
                if n >= 2:                                   # (for n <= 1 neither form touches the matrix)
                    assert P.same_numbers(np.tril(a[2]), np.tril(b[2])), (c["fam"], n, i)
                assert P.same_numbers(a[3], b[3]), (c["fam"], n, i, a[3], b[3])


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
def test_lds_solve_equals_ldlts_solve(api, N):
    """ldlt_lds_solve<N> on the factor as LDLTs<N> stores it (transpositions as doubles, read from LDS) against LDLTs<N>::solve."""
    dev = P.device()
    cases = P.ldlt_cases(N, _seed(N))
    X = P.ldlt_pack(cases, N)
    Y = P.run(dev, "ldlts_%d" % N, X)
    F = np.concatenate([Y[1 + N:1 + N + N * N], Y[1:1 + N], X[1 + N * N:]])
    Z = P.run(dev, "lds_solve_%d" % N, F)
    assert P.same_numbers(Z, Y[1 + N + N * N:])


# ---- inverse_pplu ---------------------------------------------------------------------------------------------------------------
# |inv - A^-1|_inf / |A^-1|_inf against mpmath: numpy.linalg.inv reaches INV_REF on the set, the bound is 4 x that.
INV_REF = 1.48e-15          # (the host build of inverse_pplu: 9.8e-16)
INV_BOUND = 4.0 * INV_REF


def _inverse_cases(N):
    rng = np.random.default_rng(2000 + N)
    out = []
    for _ in range(6):
        out.append(rng.normal(size=(N, N)) + N * np.eye(N))                  # well conditioned, non-symmetric
        out.append(rng.normal(size=(N, N)))                                  # general
        M = rng.normal(size=(N, N)); out.append(M @ M.T + 0.5 * np.eye(N))   # mass-matrix like
        A = rng.normal(size=(N, N)) + N * np.eye(N)
        out.append(A[::-1].copy())                                           # the large entries off the diagonal: every step swaps rows
    return out


def _inverse_error(A, inv):
    R = mp.inverse(P.mpf_mat(A))
    return float(P.mp_norminf(P.mpf_mat(inv) - R) / P.mp_norminf(R))


def _check_inverse(lib, measure=False):
    worst = 0.0
    for N in NS:
        cases = _inverse_cases(N)
        Y = P.run(lib, "inverse_%d" % N, np.stack([A.ravel() for A in cases], axis=1))
        for i, A in enumerate(cases):
            e = _inverse_error(A, np.linalg.inv(A) if measure else Y[:, i].reshape(N, N))
            worst = max(worst, e)
            assert measure or e <= INV_BOUND, (N, i, e, INV_BOUND)
    return worst


def test_inverse_host_build_against_mpmath(tmp_path):
    ref = _check_inverse(P.host(tmp_path), measure=True)
    assert ref <= INV_REF, ref
    print("inverse_pplu worst error (host build):", _check_inverse(P.host(tmp_path)))


@pytest.mark.gpu
def test_inverse_on_device(api, tmp_path):
    dev, hst = P.device(), P.host(tmp_path)
    _check_inverse(dev)
    for N in NS:
        X = np.stack([A.ravel() for A in _inverse_cases(N)], axis=1)
        assert P.same_numbers(P.run(dev, "inverse_%d" % N, X), P.run(hst, "inverse_%d" % N, X)), N


# ---- min_real_eig ---------------------------------------------------------------------------------------------------------------
# The callers use only `<= 0`.  Sign cases: symmetric, the smallest eigenvalue at least 1e-6 |S|_inf away from 0 on either side
# (the routine's early exits decide at 1e-8 of its scale; cases inside the 1e-6 band are excluded from the sign assertion, and the
# generator produces none: asserted below).  Value cases: singular PSD matrices, where neither early exit can fire and the Jacobi runs
# to its end; there the value is asserted, |value - lambda_min| / |S|_inf, against EIG_BOUND = 4 x numpy.linalg.eigvalsh's own
# worst error on the same matrices (EIG_REF).
EIG_REF = 1.83e-16          # (the host build of min_real_eig: 4.6e-17)
EIG_BOUND = 4.0 * EIG_REF


def _mineig_cases(N):
    rng = np.random.default_rng(3000 + N)
    sign, value = [], []
    for r in range(8):
        M = rng.normal(size=(N, N)); S = M @ M.T
        sign.append(S + 3.0 * N * np.eye(N))                                   # diagonally dominant: Gershgorin exit at once
        Q = P.rand_orth(rng, N)
        lam = rng.uniform(0.5, 2.0, size=N); lam[0] = -rng.uniform(0.01, 1.0)
        sign.append((Q * lam) @ Q.T)                                           # indefinite
        A = -S - 0.1 * np.eye(N); sign.append(A)                               # negative diagonal: Rayleigh exit at once
        lam = rng.uniform(0.01, 0.02, size=N); lam[-1] = 5.0
        Q = P.rand_orth(rng, N); sign.append((Q * lam) @ Q.T)                  # PD, far from diagonally dominant: exits after sweeps
        lam = rng.uniform(0.5, 2.0, size=N); lam[0] = -1e-4
        Q = P.rand_orth(rng, N); sign.append((Q * lam) @ Q.T)                  # barely indefinite, usually with a positive diagonal
        V = rng.integers(-3, 4, size=(N, N - 1)).astype(float)
        value.append(V @ V.T)                                                  # singular PSD, integer entries: lambda_min = 0
    sign = [0.5 * (S + S.T) for S in sign]
    return sign, value


def _check_mineig(lib, measure=False):
    count, worst, in_band = {}, 0.0, 0
    for N in (3, 4, 7):
        sign, value = _mineig_cases(N)
        Y = P.run(lib, "mineig_%d" % N, np.stack([S.ravel() for S in sign + value], axis=1))[0]
        for i, S in enumerate(sign):
            lmin = P.mp_eigvalsh_min(S)
            scale = np.max(np.sum(np.abs(S), axis=1))
            in_band += int(abs(lmin) < 1e-6 * scale)
            kind, sweep = P.mineig_exit(S)
            count[(kind, "sweep 0" if sweep == 0 else "later")] = count.get((kind, "sweep 0" if sweep == 0 else "later"), 0) + 1
            assert (Y[i] <= 0) == (lmin <= 0), (N, i, Y[i], float(lmin))
        for j, S in enumerate(value):
            lmin = P.mp_eigvalsh_min(S)
            scale = np.max(np.sum(np.abs(S), axis=1))
            kind, sweep = P.mineig_exit(S)
            count[("value:" + kind, "")] = count.get(("value:" + kind, ""), 0) + 1
            got = np.linalg.eigvalsh(S)[0] if measure else Y[len(sign) + j]
            if kind == "jacobi":
                e = float(abs(mp.mpf(float(got)) - lmin)) / scale
                worst = max(worst, e)
                assert measure or e <= EIG_BOUND, (N, j, e, EIG_BOUND)
    assert in_band == 0, "the sign cases keep 1e-6 of the matrix scale away from 0"
    return count, worst


def test_min_real_eig_host_build(tmp_path):
    lib = P.host(tmp_path)
    count, worst = _check_mineig(lib)
    ref = _check_mineig(lib, measure=True)[1]
    assert ref <= EIG_REF, ref
    print("min_real_eig exits (sign cases inside the 1e-6 band: 0):", sorted(count.items()), "worst value error", worst)
    assert count.get(("gershgorin", "sweep 0"), 0) > 0 and count.get(("rayleigh", "sweep 0"), 0) > 0
    assert count.get(("gershgorin", "later"), 0) > 0 and count.get(("rayleigh", "later"), 0) > 0
    assert count.get(("value:jacobi", ""), 0) >= 12          # neither exit: the Jacobi runs to its end
    X, ref = _mineig2_cases()
    Y = P.run(lib, "mineig_2", X)[0]
    _check_mineig2(X, Y, ref)
    e2 = _mineig2_error(X, np.array([np.min(np.linalg.eigvals(X[:, i].reshape(2, 2)).real) for i in range(X.shape[1])]), ref)
    print("numpy.linalg.eigvals worst error on the N = 2 set:", e2, "host build:", _mineig2_error(X, Y, ref))
    assert e2 <= EIG2_REF, e2
    assert P.run(lib, "mineig_1", np.array([[-2.5, 0.0, 3.0]]))[0].tolist() == [-2.5, 0.0, 3.0]


def _mineig2_cases():
    """N = 2, closed form for a GENERAL real matrix: symmetric, non-symmetric with real and with complex eigenvalues; the
    eigenvalues are kept apart (|disc| >= 1e-2 scale^2) so that the closed form's square root is well conditioned."""
    rng = np.random.default_rng(3002)
    mats, kinds = [], {"real": 0, "complex": 0, "symmetric": 0}
    while len(mats) < 60:
        M = rng.normal(size=(2, 2)) * 2.0
        if len(mats) % 3 == 0:
            M = 0.5 * (M + M.T)
        tr, det = M[0, 0] + M[1, 1], M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
        disc, scale = 0.25 * tr * tr - det, np.max(np.abs(M)) ** 2
        if abs(disc) < 1e-2 * scale:
            continue
        E = mp.eig(P.mpf_mat(M), left=False, right=False)
        ref = min(mp.re(v) for v in E)
        if abs(ref) < 1e-3:
            continue
        kinds["symmetric" if len(mats) % 3 == 0 else ("real" if disc > 0 else "complex")] += 1
        mats.append((M, float(ref)))
    assert min(kinds.values()) >= 10, kinds
    return np.stack([M.ravel() for M, _ in mats], axis=1), np.array([r for _, r in mats])


# N = 2: |value - min Re(eig)| / max|M_ij| against mpmath; numpy.linalg.eigvals reaches EIG2_REF on the set, the bound is 4 x that.
EIG2_REF = 2.84e-16
EIG2_BOUND = 4.0 * EIG2_REF


def _mineig2_error(X, got, ref):
    return float(np.max(np.abs(got - ref) / np.max(np.abs(X), axis=0)))


def _check_mineig2(X, Y, ref):
    assert np.array_equal(Y <= 0, ref <= 0)
    e = _mineig2_error(X, Y, ref)
    assert e <= EIG2_BOUND, (e, EIG2_BOUND)


@pytest.mark.gpu
def test_min_real_eig_on_device(api, tmp_path):
    dev, hst = P.device(), P.host(tmp_path)
    _check_mineig(dev)
    X, ref = _mineig2_cases()
    _check_mineig2(X, P.run(dev, "mineig_2", X)[0], ref)
    X1 = np.array([[-2.5, 0.0, 3.0, 1e-310, -np.inf]])
    assert P.run(dev, "mineig_1", X1)[0].tolist() == X1[0].tolist()
    for N in (3, 4, 7):
        sign, value = _mineig_cases(N)
        X = np.stack([S.ravel() for S in sign + value], axis=1)
        assert P.same_numbers(P.run(dev, "mineig_%d" % N, X), P.run(hst, "mineig_%d" % N, X)), N
    X, _ = _mineig2_cases()
    assert P.same_numbers(P.run(dev, "mineig_2", X), P.run(hst, "mineig_2", X))


# ---- singular values ------------------------------------------------------------------------------------------------------------
# |s - s_ref| / s_max against mpmath's SVD for the largest and the smallest singular value: numpy.linalg.svd reaches SVD_REF on the
# set, the bound is 4 x that.  The Jacobi has ONE text (dev_linalg.hpp::singular_minmax<NMAXP>) with two instantiations -- <16> in
# te_backward, <8> (leading dimension 8) in the stack-fed sweep -- and a copy on memory operands (kernels_te.hpp::singular_minmax_mem).
SVD_REF = 5.42e-16
SVD_BOUND = 4.0 * SVD_REF


def _singular_cases():
    rng = np.random.default_rng(4000)
    out = [np.zeros((0, 0)), np.array([[-3.0]]), np.array([[0.0]])]
    for n in (2, 3, 5, 8, 14, 16):
        out.append(rng.normal(size=(n, n)))
        A = rng.normal(size=(n, n)); A[:, -1] = A[:, 0]; out.append(A)        # rank deficient: two equal columns
        out.append(np.diag(rng.normal(size=n) * 3.0))                         # diagonal: no rotation at all
        out.append((P.rand_orth(rng, n) * np.logspace(-5, 1, n)) @ P.rand_orth(rng, n))
    return out


def _singular_ref(A):
    if A.shape[0] == 0:
        return 0.0, 0.0
    S = mp.svd_r(P.mpf_mat(A), compute_uv=False)
    return max(S), min(S)


def _singular_error(got_max, got_min, A):
    smax, smin = _singular_ref(A)
    den = smax if smax != 0 else mp.mpf(1)
    return float(max(abs(mp.mpf(float(got_max)) - smax), abs(mp.mpf(float(got_min)) - smin)) / den)


def test_singular_value_cases_and_reference_error():
    """The case set against mpmath with numpy's SVD standing in for the routine (the Jacobi copies are device-only): the set holds
    n = 0, n = 1, rank-deficient and diagonal matrices, and the reference error behind SVD_BOUND is what the module states."""
    worst = 0.0
    for A in _singular_cases():
        s = np.linalg.svd(A, compute_uv=False) if A.shape[0] else np.zeros(1)
        worst = max(worst, _singular_error(s.max(), s.min(), A))
    print("numpy.linalg.svd worst error on the set:", worst)
    assert worst <= SVD_REF
    ranks = [np.linalg.matrix_rank(A) < A.shape[0] for A in _singular_cases() if A.shape[0] > 1]
    assert sum(ranks) >= 6 and any(A.shape[0] == 0 for A in _singular_cases()) and any(A.shape[0] == 1 for A in _singular_cases())


@pytest.mark.gpu
def test_singular_value_copies_on_device(api):
    dev = P.device()
    cases = _singular_cases()
    X = np.full((1 + 256, len(cases)), P.NAN)
    for i, A in enumerate(cases):
        n = A.shape[0]
        F = np.full((16, 16), P.NAN); F[:n, :n] = A
        X[0, i] = n; X[1:, i] = F.ravel()
    Y = P.run(dev, "singular", X)
    assert P.same_numbers(Y[0:2], Y[2:4]), "singular_minmax<16> and singular_minmax_mem differ"
    small = np.array([A.shape[0] <= 8 for A in cases])
    assert small.sum() >= 15 and P.same_numbers(Y[0:2, small], Y[4:6, small]), "singular_minmax<16> and singular_minmax<8> differ"
    for i, A in enumerate(cases):
        for k in (0, 2) + ((4,) if small[i] else ()):
            e = _singular_error(Y[k, i], Y[k + 1, i], A)
            assert e <= SVD_BOUND, (i, k, A.shape, e, SVD_BOUND)


# ---- madd_2r, affine_2r, sign_of_reduction, dmax, dmin ---------------------------------------------------------------------------
def _fl(q):
    """Round an exact rational to the nearest float64 (ties to even): Fraction -> float does exactly that."""
    return float(q)


def _two_rounding_cases():
    """Operands for which a*b + c differs between one rounding (fused) and two: c = -fl(a*b), so the twice-rounded result is an exact
    0 and the fused one is the rounding error of the product.  Constructed and asserted in exact rational arithmetic."""
    rng = np.random.default_rng(5000)
    a = 1.0 + rng.random(200); b = 1.0 + rng.random(200)
    keep = [i for i in range(200) if Fraction(a[i]) * Fraction(b[i]) != Fraction(a[i] * b[i])]
    a, b = a[keep], b[keep]
    c = -(a * b)
    for i in range(a.size):
        exact = Fraction(a[i]) * Fraction(b[i]) + Fraction(c[i])
        assert _fl(exact) != 0.0 and _fl(Fraction(_fl(Fraction(a[i]) * Fraction(b[i]))) + Fraction(c[i])) == 0.0
    assert a.size > 100
    return a, b, c


def _check_two_roundings(lib):
    a, b, c = _two_rounding_cases()
    B = a.size
    assert np.array_equal(P.run(lib, "madd", np.stack([a, b, c]))[0], np.zeros(B))
    x = 1.0 + np.arange(B) / B
    assert np.array_equal(P.run(lib, "madd", np.stack([a, b, x]))[0], a * b + x)       # numpy: two roundings
    for N in (1, 2, 4):
        # base + a*k with base = -fl(a*k): 0 unless the product is fused into the sum
        X = np.zeros((3 + 2 * N, B)); X[0], X[1], X[2] = c, a, b
        assert np.array_equal(P.run(lib, "affine_%d" % N, X)[0], np.zeros(B)), N
        if N >= 2:
            # sum_j K_j dx_j with K_0 dx_0 = -fl(K_1 dx_1): 0 unless the second product is fused into the running sum
            X = np.zeros((3 + 2 * N, B)); X[3], X[3 + N] = c, 1.0; X[4], X[4 + N] = a, b
            assert np.array_equal(P.run(lib, "affine_%d" % N, X)[0], np.zeros(B)), N
        rng = np.random.default_rng(5001 + N)
        X = rng.normal(size=(3 + 2 * N, B))
        p = np.zeros(B)
        for j in range(N):
            p = p + X[3 + j] * X[3 + N + j]
        assert np.array_equal(P.run(lib, "affine_%d" % N, X)[0], (X[0] + X[1] * X[2]) + p), N


def _sign_cases():
    nnan = np.copysign(np.nan, -1.0)
    a = np.array([0.0, 5e-324, -5e-324, 1e-300, -1e-300, np.nan, nnan, 1.0, -1.0, np.inf, -np.inf, 3.0 - 3.0, np.nan, 1.0, np.nan, 2.0, 1.0])
    b = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, -2.0, 1.0, 1.0, 1.0, np.nan, np.nan, 7.0, 1.0, 2.0])
    return a, b


def _check_sign_min_max(lib):
    a, b = _sign_cases()
    Y = P.run(lib, "signminmax", np.stack([a, b]))
    for i in range(a.size):
        x, y = a[i], b[i]
        sgn = math.copysign(1.0, x) if x != x else (-1.0 if x < 0 else 1.0)
        assert Y[0, i] == sgn, (i, x, Y[0, i])
        mx = y if x < y else x                               # std::max(a, b): (a < b) ? b : a
        mn = y if y < x else x                               # std::min(a, b): (b < a) ? b : a
        assert P.same_numbers(Y[1, i], mx) and P.same_numbers(Y[2, i], mn), (i, x, y, Y[1, i], Y[2, i])
        cl = 1.0 if 1.0 < mx else mx                         # dclamp(a, b, 1) = dmin(dmax(a, b), 1) = std::min(max, 1): (1 < max) ? 1 : max
        assert P.same_numbers(Y[3, i], cl), (i, x, y, Y[3, i])
        assert Y[4, i] == (1.0 if math.isfinite(x) else 0.0)


def test_two_roundings_and_sign_min_max_host_build(tmp_path):
    _check_two_roundings(P.host(tmp_path))
    _check_sign_min_max(P.host(tmp_path))


@pytest.mark.gpu
def test_two_roundings_and_sign_min_max_on_device(api):
    """madd_2r / affine_2r return the TWICE-rounded value (operands built so that a fused multiply-add gives another one);
    sign_of_reduction at x - x, +-tiny and NaN of both signs; dmax / dmin with a NaN in either position, std::max / std::min order."""
    _check_two_roundings(P.device())
    _check_sign_min_max(P.device())
