"""The filter recursion of include/cddp_hip.h ("Kalman filter gains and output-feedback covariance along a solved plan") restated in
numpy, one function per step body: the reference of the bitwise checks of tests/test_plan_kf.py and test_plan_kf_shapes.py (GPU) and of
tests/test_plan_kf_host.py (the C++ step bodies of csrc/plan_kf.hpp).

Vectorised over the batch and over the elements of a matrix; every accumulation loop is written out with its index ascending, from the
stated start value, and numpy rounds each product and each sum, as the library built with -ffp-contract=off does; / is IEEE's.
Comparisons are by value (np.array_equal with NaN = NaN): the header leaves the sign of an exact zero open.  Nothing here touches a
device."""
import numpy as np

from plan_cov_ref import mirror, same  # noqa: F401  (same: re-exported for the tests)


def h_vec(S, c):
    """step 1a: h[i] = sum_j S[i][j] * c[j] from 0, j ascending.  S (B, nx, nx), c (B, nx) -> (B, nx)"""
    h = np.zeros(S.shape[:2])
    for j in range(S.shape[2]):
        h = h + S[:, :, j] * c[:, None, j]
    return h


def innovation(v, c, h):
    """step 1b: s = v; s += c[j] * h[j], j ascending.  v (B,), c, h (B, nx) -> (B,)"""
    s = v.copy()
    for j in range(c.shape[1]):
        s = s + c[:, j] * h[:, j]
    return s


def joseph(S, G, h, s):
    """steps 1c - 1e: g = h / s; S[i][j] - g[i] h[j] - h[i] g[j] + (s g[i]) g[j] and G[i][j] + h[i] g[j] for j <= i, mirrored"""
    g = h / s[:, None]
    e = S - g[:, :, None] * h[:, None, :]
    e = e - h[:, :, None] * g[:, None, :]
    q = s[:, None] * g
    e = e + q[:, :, None] * g[:, None, :]
    return mirror(e), mirror(G + h[:, :, None] * g[:, None, :])


def update(Sm, C, v):
    """step 1, all rows.  Sm (B, nx, nx), C (B, ny, nx), v (B, ny) -> Sf, G, ok (B,) bool: every row passed s > 0"""
    S = Sm; G = np.zeros_like(Sm); ok = np.ones(Sm.shape[0], dtype=bool)
    for r in range(C.shape[1]):
        h = h_vec(S, C[:, r])
        s = innovation(v[:, r], C[:, r], h)
        ok = ok & (s > 0.0)
        S, G = joseph(S, G, h, s)
    return S, G, ok


def gain(Sf, C, v):
    """step 2: L[i][r] = (sum_j Sf[i][j] * C[r][j]) / v[r] -> (B, nx, ny)"""
    return np.stack([h_vec(Sf, C[:, r]) / v[:, r, None] for r in range(C.shape[1])], axis=2)


def acl_of(At, Bt, Kt):
    """plan_covariance step 1"""
    Acl = At.copy()
    for k in range(Bt.shape[2]):
        Acl = Acl + Bt[:, :, k, None] * Kt[:, None, k, :]
    return Acl


def control_cov(Kt, Xh, Wus):
    """plan_covariance steps 2 and 3 with Xh for Sigma"""
    B, nu, nx = Kt.shape
    Z = np.zeros((B, nu, nx))
    for l in range(nx):
        Z = Z + Kt[:, :, l, None] * Xh[:, None, l, :]
    S_u = np.zeros((B, nu, nu))
    for l in range(nx):
        S_u = S_u + Z[:, :, l, None] * Kt[:, None, :, l]
    if Wus is not None:
        S_u = S_u + Wus
    return mirror(S_u)


def propagate(M, Sig, Ws, Wus, Bt):
    """plan_covariance steps 4 and 5 with M for Acl: M Sig M^T (+ W) (+ B Wu B^T), the lower triangle mirrored"""
    B, nx = M.shape[0], M.shape[1]
    Y = np.zeros((B, nx, nx))
    for l in range(nx):
        Y = Y + M[:, :, l, None] * Sig[:, None, l, :]
    Nx = np.zeros((B, nx, nx))
    for l in range(nx):
        Nx = Nx + M[:, :, l, None] * Y[:, None, :, l]
    if Ws is not None:
        Nx = Nx + Ws
    if Wus is not None:
        nu = Bt.shape[2]
        G = np.zeros((B, nx, nu))
        for m in range(nu):
            G = G + Bt[:, :, m, None] * Wus[:, None, m, :]
        H = np.zeros((B, nx, nx))
        for k in range(nu):
            H = H + G[:, :, k, None] * Bt[:, None, :, k]
        Nx = Nx + H
    return mirror(Nx)


def trace_sum(Q, M):
    """plan_covariance step 6 for one matrix: r_i = sum_j Q[i][j] M[i][j]; c = sum_i r_i, both from 0 ascending -> (B,)"""
    n = M.shape[1]
    r = np.zeros((M.shape[0], n))
    for j in range(n):
        r = r + Q[None, :, j] * M[:, :, j]
    return r


def kalman(A, Bm, K, C, v, Sigma0, W=None, Wu=None, Qdt=None, Rdt=None, Qf=None, diag=False):
    """A (B, N, nx, nx), Bm (B, N, nx, nu), K (B, N, nu, nx); C (ny, nx) or (B, ny, nx), v (ny,) or (B, ny); Sigma0 / W (nx, nx) or
    (B, nx, nx), Wu (nu, nu) or (B, nu, nu), W and Wu may be None; Qdt, Rdt, Qf as plan_cov_ref.covariance's, or all None (no dcost).
    -> dict: L (B, N + 1, nx, ny), SP, SF, SX (B, N + 1, nx, nx), SU (B, N, nu, nu) (diag: the diagonals of SP, SF, SX, SU), dcost (B,) or
    None, info (B,) int32.  A trajectory whose row fails at step t: info = t + 1, NaN in every row s >= t and in dcost."""
    B, N, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]

    def batched(M, shape):
        return None if M is None else np.ascontiguousarray(np.broadcast_to(np.asarray(M, dtype=np.float64), (B,) + shape))

    def sym(M, n):
        return None if M is None else batched(mirror(np.asarray(M, dtype=np.float64)), (n, n))

    C = np.asarray(C, dtype=np.float64); ny = C.shape[-2]
    Cs = batched(C, (ny, nx)); vs = batched(v, (ny,))
    Sm = sym(Sigma0, nx); Ws = sym(W, nx); Wus = sym(Wu, nu)
    Xm = np.zeros((B, nx, nx))
    L = np.zeros((B, N + 1, nx, ny)); SP = np.zeros((B, N + 1, nx, nx)); SF = np.zeros_like(SP); SX = np.zeros_like(SP)
    SU = np.zeros((B, N, nu, nu)); info = np.zeros(B, dtype=np.int32)
    cost = Qdt is not None
    dcost = np.zeros(B) if cost else None
    dead = np.zeros(B, dtype=bool)
    nan3 = lambda M: np.where(dead[:, None, None], np.nan, M)
    with np.errstate(all="ignore"):                                   # (a dead trajectory walks on, on whatever it holds)
        for t in range(N + 1):
            Sf, G, ok = update(Sm, Cs, vs)
            info[~ok & ~dead] = t + 1
            dead = dead | ~ok
            Xh = mirror(Xm + G)
            Sx = Xh + Sf
            SP[:, t] = nan3(Sm); SF[:, t] = nan3(Sf); L[:, t] = nan3(gain(Sf, Cs, vs)); SX[:, t] = nan3(Sx)
            if t == N:
                break
            At, Bt, Kt = A[:, t], Bm[:, t], K[:, t]
            S_u = control_cov(Kt, Xh, Wus)
            SU[:, t] = nan3(S_u)
            if cost:
                c = np.zeros(B)
                r = trace_sum(Qdt, Sx)
                for i in range(nx):
                    c = c + r[:, i]
                r = trace_sum(Rdt, S_u)
                for i in range(nu):
                    c = c + r[:, i]
                dcost = dcost + c
            Sm = propagate(At, Sf, Ws, Wus, Bt)
            Xm = propagate(acl_of(At, Bt, Kt), Xh, None, None, Bt)
        if cost:
            c = np.zeros(B)
            r = trace_sum(Qf, Sx)
            for i in range(nx):
                c = c + r[:, i]
            dcost = np.where(dead, np.nan, dcost + c)
    d = (lambda M: np.ascontiguousarray(np.diagonal(M, axis1=2, axis2=3))) if diag else (lambda M: M)
    return {"L": L, "SP": d(SP), "SF": d(SF), "SX": d(SX), "SU": d(SU), "dcost": dcost, "info": info}


# The largest deviations of kalman() from exact (60-digit) evaluation of the BATCH form of the filter (L = Sm C^T (C Sm C^T + V)^-1,
# Sf = (I - L C) Sm, the covariance of [dx; xhat] propagated as one matrix) over the pairs (4,1), (3,2), (8,3), (14,7) with ny in
# {1, nx, nx + 2} at N = 5 on plan_cov_ref.contractive_stacks with spd Sigma0, W and Wu, as tests/test_plan_kf_host.py measures them: of
# L, SX, SU relative to the exact maximum of each, of dcost relative to the exact value.  Likewise the perfect-measurement and duality
# identities of that file.  Tests that are not bitwise allow 8 x the figure of the quantity they compare, capped at 1e-12.
MEASURED_REL_DEV_L = 4.447e-14      # at (14, 7), ny = 1: L = Sf C^T / v cancels where v is small against c . h
MEASURED_REL_DEV_SX = 2.555e-16     # at (8, 3), ny = 10
MEASURED_REL_DEV_SU = 4.307e-16     # at (14, 7), ny = 14
MEASURED_REL_DEV_COST = 1.580e-16   # at (4, 1), ny = 1
MEASURED_REL_DEV_PERFECT = 3.450e-16# at (4, 1)
MEASURED_REL_DEV_DUALITY = 7.142e-17# at (8, 3), ny = 10
CAP = 1e-12
