"""Helper of tests/test_dev_linalg.py, tests/test_boxqp.py and tests/test_dev_elem_gpu.py: loads the device-routine probe
(tests/hip/dev_probe.hip, built by cddp-cpp_amd/csrc/Makefile into cddp-cpp_amd/lib/libcddp_hip_probe.so) and the host build of the
same case bodies (tests/hip/dev_probe_host.cpp, compiled here with g++), and owns the fixed-seed case generators and the references.

References are independent of the code under test: mpmath at 60 digits on the float64 inputs for values, the numpy twin
(oracle/twin/cddp_twin.py: EigenLDLT, boxqp) for decisions and structure.  Not a conftest: the test modules import it."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle", "twin"))
import cddp_twin as T  # noqa: E402

mp.mp.dps = 60
DEVICE_LIB = os.path.join(REPO, "cddp-cpp_amd", "lib", "libcddp_hip_probe.so")
DBL_MIN = np.finfo(np.float64).tiny
EPS = 2.0 ** -52
NAN = float("nan")

_host = None
_device = None


def host(tmp_path):
    """The case bodies compiled for the host with the product's -ffp-contract=off (once per process)."""
    global _host
    if _host is None:
        so = str(tmp_path / "libcddp_probe_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                               os.path.join(HERE, "hip", "dev_probe_host.cpp")])
        _host = ctypes.CDLL(so)
    return _host


def device():
    """The gfx950 probe library.  GPU tests take the `api` fixture first, so torch's ROCm runtime is bound before this loads."""
    global _device
    if _device is None:
        assert os.path.exists(DEVICE_LIB), "libcddp_hip_probe.so is missing: run make -C cddp-cpp_amd/csrc (build() does)"
        _device = ctypes.CDLL(DEVICE_LIB)
    return _device


def run(lib, name, X):
    """X: (NIN, B) float64, batch-minor.  Returns (NOUT, B)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    nin, nout = ctypes.c_int(), ctypes.c_int()
    getattr(lib, "probe_%s_dims" % name)(ctypes.byref(nin), ctypes.byref(nout))
    assert X.ndim == 2 and X.shape[0] == nin.value, (name, X.shape, nin.value)
    B = X.shape[1]
    out = np.full((nout.value, B), NAN)
    fn = getattr(lib, "probe_" + name)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    fn.restype = ctypes.c_int
    rc = fn(X.ctypes.data, out.ctypes.data, B)
    assert rc == 0, "probe_%s: hipError_t %d" % (name, rc)
    return out


def same_numbers(a, b):
    """Equality of two float64 arrays as NUMBERS: every finite or infinite value bit for bit, with two carve-outs -- -0.0 equals
    +0.0 (the library is built with -fno-signed-zeros, under which the sign of an exact zero is not defined) and every NaN equals
    every NaN (DESIGN.md section 5 documents NaN signs / payloads as not comparable between x86 and gfx950).  This is what the
    test modules mean by "bit-equal"."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def mpf_mat(A):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(A)])


def mp_norminf(M):
    return max([mp.fsum([abs(M[i, j]) for j in range(M.cols)]) for i in range(M.rows)] or [mp.mpf(0)])


def rand_orth(rng, n):
    Q, R = np.linalg.qr(rng.normal(size=(n, n)))
    return Q * np.sign(np.diag(R))


# -------------------------------------------------------------------------------------------------------------------------
# LDLT
# -------------------------------------------------------------------------------------------------------------------------
def ldlt_cases(n, seed, reps=3):
    """Fixed-seed matrices of size n, families interleaved (so neighbouring lanes / lane groups hold different pivot sequences and
    different exits).  Each case: fam, A (n x n; only the lower triangle may be read), b, blk = the indices of the non-singular
    block (x must solve A[blk, blk] x[blk] = b[blk] and be exactly 0 elsewhere) or None when x is not checked (ok false)."""
    rng = np.random.default_rng(seed)
    out = []
    full = list(range(n))

    def add(fam, A, b=None, blk=full):
        out.append(dict(fam=fam, A=np.array(A, dtype=np.float64), b=rng.normal(size=n) if b is None else np.array(b, dtype=np.float64), blk=blk))

    def spd(k):
        M = rng.normal(size=(k, k))
        return M @ M.T + 0.5 * np.eye(k)

    if n == 0:
        add("empty", np.zeros((0, 0)))
        return out
    if n == 1:
        for v in (2.0, -3.0, 1e-300):
            add("spd" if v > 0 else "indefinite", [[v]])
        add("zero", [[0.0]], blk=[])
        add("subnormal", [[1e-310]], blk=[])
        add("subnormal", [[DBL_MIN]], blk=[])                       # |d| > DBL_MIN is false AT DBL_MIN
        add("subnormal_above", [[np.nextafter(DBL_MIN, 1.0)]])
        return out
    # the structural cases first: the first four share a wavefront of the cooperative kernel even at 64 / G = 4
    add("zero", np.zeros((n, n)), blk=[])
    A = np.zeros((n, n)); A[1, 0] = A[0, 1] = 1.0
    add("zerodiag_offdiag", A, blk=None)
    if n >= 3:
        A = np.zeros((n, n)); A[:n - 2, :n - 2] = spd(n - 2) + 4.0 * np.eye(n - 2); A[n - 1, n - 2] = A[n - 2, n - 1] = 1.0
        add("late_fail", A, blk=None)
        A = np.eye(n); A[n - 2:, n - 2:] = 2.0                        # the largest diagonal last: transpositions, then 2 - 1 * 2 * 1 = 0
        add("zero_then_valid", A, blk=None)
    add("rankdef_dense", np.full((n, n), 2.0), b=np.arange(1, n + 1) * 2.0, blk="exact")
    # zero diagonal, the two triangles differ: only the LOWER one decides the early return's flag
    A = np.zeros((n, n)); A[n - 1, 0] = 3.0
    add("zerodiag_lower_only", A, b=np.arange(1, n + 1) * 1.0, blk=None)                      # ok false
    A = np.zeros((n, n)); A[0, n - 1] = 3.0
    add("zerodiag_upper_only", A, b=np.arange(1, n + 1) * 1.0, blk="exact")                   # ok true, x = 0
    for _ in range(reps):
        add("spd", spd(n))
        Q = rand_orth(rng, n)
        d = rng.uniform(0.5, 3.0, size=n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        S = (Q * d) @ Q.T
        add("indefinite", 0.5 * (S + S.T))
        Q = rand_orth(rng, n)
        S = (Q * np.logspace(-6, 2, n)) @ Q.T
        add("illcond", 0.5 * (S + S.T))
        O = rng.normal(size=(n, n)) * 0.3; O = 0.5 * (O + O.T); np.fill_diagonal(O, 0.0)
        sg = np.ones(n); sg[rng.integers(0, n)] = -1.0                # |diagonal| all equal, one of them negative: the first wins
        add("ties", O + np.diag(2.0 * sg))
        S = spd(n)
        add("triangles", np.tril(S) + np.triu(rng.normal(size=(n, n)) * 7.0, 1))
        k = max(1, n // 2)
        perm = rng.permutation(n)
        A = np.zeros((n, n)); A[:k, :k] = spd(k)
        A = A[np.ix_(np.argsort(perm), np.argsort(perm))]              # block rows land at perm[:k]
        add("rankdef", A, blk=sorted(perm[:k].tolist()))
        A = np.zeros((n, n)); A[:n - 1, :n - 1] = spd(n - 1); A[n - 1, n - 1] = 1e-310 if _ % 2 == 0 else DBL_MIN
        add("subnormal", A, blk=list(range(n - 1)))
    return out


def ldlt_pack(cases, nmax, ld=None):
    """Records of CaseLdltd / CaseLdlts / the cooperative kernel: n, A (leading dimension ld), b; NaN outside the n x n block and beyond b[n)."""
    ld = nmax if ld is None else ld
    B = len(cases)
    X = np.full((1 + nmax * ld + nmax, B), NAN)
    for i, c in enumerate(cases):
        k = c["A"].shape[0]
        X[0, i] = k
        A = np.full((nmax, ld), NAN); A[:k, :k] = c["A"]
        X[1:1 + nmax * ld, i] = A.ravel()
        X[1 + nmax * ld:1 + nmax * ld + k, i] = c["b"]
    return X


def ldlt_unpack(Y, i, nmax, n, ld=None):
    ld = nmax if ld is None else ld
    ok = Y[0, i] == 1.0
    tr = Y[1:1 + n, i].astype(int)
    M = Y[1 + nmax:1 + nmax + nmax * ld, i].reshape(nmax, ld)[:n, :n]
    x = Y[1 + nmax + nmax * ld:1 + nmax + nmax * ld + n, i]
    return ok, tr, M, x


def sym_lower(A):
    return np.tril(A) + np.tril(A, -1).T


def solve_backward_error(A, x, b):
    """Normwise backward error |Ax - b|_inf / (|A|_inf |x|_inf + |b|_inf), residual in mpmath."""
    if len(b) == 0:
        return 0.0
    Am, xm, bm = mpf_mat(A), mp.matrix([mp.mpf(float(v)) for v in x]), mp.matrix([mp.mpf(float(v)) for v in b])
    r = Am * xm - bm
    den = mp_norminf(Am) * max(abs(v) for v in xm) + max(abs(v) for v in bm)
    return float(max(abs(v) for v in r) / den) if den != 0 else float(max(abs(v) for v in r))


def factor_backward_error(A, tr, M):
    """|P A P^T - L D L^T|_inf / |A|_inf in mpmath, L / D read from the lower triangle of M."""
    n = A.shape[0]
    if n == 0:
        return 0.0
    P = list(range(n))
    for k in range(n):
        P[k], P[tr[k]] = P[tr[k]], P[k]
    Ap = mpf_mat(sym_lower(A)[np.ix_(P, P)])
    L = mp.matrix(n, n); D = mp.matrix(n, n)
    for i in range(n):
        L[i, i] = 1; D[i, i] = mp.mpf(float(M[i, i]))
        for j in range(i):
            L[i, j] = mp.mpf(float(M[i, j]))
    R = Ap - L * D * L.T
    na = mp_norminf(Ap)
    return float(mp_norminf(R) / na) if na != 0 else float(mp_norminf(R))


# -------------------------------------------------------------------------------------------------------------------------
# min_real_eig: which exit a symmetric matrix takes (a trace of the routine's decisions, used for the reach counts only)
# -------------------------------------------------------------------------------------------------------------------------
def mineig_exit(M):
    n = M.shape[0]
    S = 0.5 * (M + M.T)
    for sweep in range(60):   # (Python floats below: an overflowing theta^2 is inf, as in C)
        r = np.sum(np.abs(S), axis=1) - np.abs(np.diag(S))
        lo = np.min(np.diag(S) - r); dmn = np.min(np.diag(S)); scale = np.max(np.abs(np.diag(S)) + r)
        if lo > 1e-8 * scale:
            return "gershgorin", sweep
        if dmn < -1e-8 * scale:
            return "rayleigh", sweep
        if np.sum(np.triu(S, 1) ** 2) < 1e-300:
            break
        for p in range(n):
            for q in range(p + 1, n):
                if S[p, q] == 0.0:
                    continue
                theta = float(S[q, q] - S[p, p]) / float(2.0 * S[p, q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                cs = 1.0 / math.sqrt(t * t + 1.0); sn = t * cs
                J = np.eye(n); J[p, p] = cs; J[q, q] = cs; J[p, q] = sn; J[q, p] = -sn
                S = J.T @ S @ J
    return "jacobi", sweep


def mp_eigvalsh_min(S):
    E = mp.eigsy(mpf_mat(S), eigvals_only=True)
    return min(E)


# -------------------------------------------------------------------------------------------------------------------------
# BoxQP
# -------------------------------------------------------------------------------------------------------------------------
BQ = {"HESSIAN_NOT_PD": -1, "NO_DESCENT": 0, "MAX_ITER_EXCEEDED": 1, "MAX_LS_EXCEEDED": 2, "SUCCESS": 4, "ALL_CLAMPED": 5}


def boxqp_options(max_it=100):
    o = T.default_options()
    o["boxqp_max_iterations"] = int(max_it)
    return o


def boxqp_pack(cases, n):
    """Records of CaseBoxqp<n>: max_iterations, H, g, lower, upper, x0, r."""
    X = np.zeros((1 + n * n + 5 * n, len(cases)))
    for i, c in enumerate(cases):
        X[:, i] = np.concatenate([[c["max_it"]], c["H"].ravel(), c["g"], c["lo"], c["up"], c["x0"], c["r"]])
    return X


def boxqp_unpack(Y, i, n):
    status = int(Y[0, i]); free = Y[1:1 + n, i].astype(int); x = Y[1 + n:1 + 2 * n, i]
    nf = int(Y[1 + 2 * n, i]); y = Y[2 + 2 * n:2 + 2 * n + nf, i]
    return status, free, x, nf, y


def boxqp1_exit(H, g, lo, up, x0, max_it):
    """Which way a scalar BoxQP ends, in the letters of dev_boxqp.hpp's comment (A-E) or 'loop' for the ballot fallback: a trace of
    the twin's boxqp() decisions on Python floats (IEEE double, no contraction)."""
    o = boxqp_options(max_it)
    norm_ok = lambda ag: ag == 0.0 or (2.0 ** -500 < ag < 2.0 ** 500)
    obj = lambda z: 0.5 * (z * (H * z)) + g * z
    if max_it < 2:
        return "loop"
    x = min(max(x0, lo), up)
    grad = g + H * x
    if (x == lo and grad > 0) or (x == up and grad < 0):
        return "A"
    if not norm_ok(abs(grad)):
        return "loop"
    if abs(grad) < o["boxqp_min_gradient_norm"]:
        return "B"
    newton = -(g / H) if abs(H) > DBL_MIN else -0.0
    search = newton - x
    sdotg = search * grad
    if not sdotg < 0:
        return "loop"
    x1 = min(max(x + search, lo), up)
    v0, v1 = obj(x), obj(x1)
    if not (v1 - v0) <= o["boxqp_armijo_constant"] * sdotg:
        return "loop"
    if abs(v0 - v1) < o["boxqp_min_relative_improvement"] * abs(v0):
        return "C"
    grad1 = g + H * x1
    if (x1 == lo and grad1 > 0) or (x1 == up and grad1 < 0):
        return "D"
    if norm_ok(abs(grad1)) and abs(grad1) < o["boxqp_min_gradient_norm"]:
        return "E"
    return "loop"


# -------------------------------------------------------------------------------------------------------------------------
# ulp error against mpmath
# -------------------------------------------------------------------------------------------------------------------------
def ulp_of(v):
    a = abs(float(v))
    return 4.9e-324 if a == 0 else float(np.nextafter(a, np.inf) - a)


def max_ulp_error(f, xs, got):
    """max over the points of |got - f(x)| / ulp(f(x)), f an mpmath function of the exact float64 argument(s)."""
    worst, at = 0.0, None
    for k in range(len(got)):
        args = xs[k] if isinstance(xs[k], tuple) else (xs[k],)
        r = f(*[mp.mpf(float(a)) for a in args])
        e = float(abs(mp.mpf(float(got[k])) - r)) / ulp_of(r)
        if e > worst:
            worst, at = e, xs[k]
    return worst, at
