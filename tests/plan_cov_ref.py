"""The covariance recursion of include/cddp_hip.h ("state and control covariance along a solved plan") restated in numpy: the reference of
the bitwise checks of tests/test_plan_cov.py and test_plan_cov_shapes.py (GPU) and of tests/test_plan_cov_host.py (the C++ step bodies).

Vectorised over the batch and over the elements of a matrix; every accumulation loop is written out with its index ascending, from the
stated start value, and numpy rounds each product and each sum, as the library built with -ffp-contract=off does.  Comparisons are by
value (np.array_equal with NaN = NaN): the header leaves the sign of an exact zero open.  Nothing here touches a device."""
import numpy as np


def same(a, b):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    if hasattr(b, "detach"):
        b = b.detach().cpu().numpy()
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def mirror(M):
    """(..., n, n) -> the symmetric matrix whose lower triangle (j <= i) is M's: what is above the diagonal is never looked at"""
    L = np.tril(M)
    return L + np.swapaxes(np.tril(M, -1), -1, -2)


def covariance(A, Bm, K, Sigma0, W=None, Wu=None, Qdt=None, Rdt=None, Qf=None, diag=False):
    """A (B, N, nx, nx), Bm (B, N, nx, nu), K (B, N, nu, nx); Sigma0 / W (nx, nx) or (B, nx, nx), Wu (nu, nu) or (B, nu, nu), W and Wu
    may be None; Qdt = Q * dt (nx, nx), Rdt = R * dt (nu, nu), Qf (nx, nx), or all None (no dcost).
    -> SX (B, N + 1, nx, nx), SU (B, N, nu, nu) (diag: (B, N + 1, nx), (B, N, nu)), dcost (B,) or None"""
    B, N, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]

    def batched(M, n):
        return None if M is None else np.ascontiguousarray(np.broadcast_to(mirror(np.asarray(M, dtype=np.float64)), (B, n, n)))

    Sig = batched(Sigma0, nx); Ws = batched(W, nx); Wus = batched(Wu, nu)
    SX = np.zeros((B, N + 1, nx, nx)); SU = np.zeros((B, N, nu, nu))
    cost = Qdt is not None
    dcost = np.zeros(B) if cost else None

    def trace(Q, M, n):
        """c-terms: r_i = sum_j Q[i][j] M[i][j] (j ascending from 0), returned as (B, n)"""
        r = np.zeros((B, n))
        for j in range(n):
            r = r + Q[None, :, j] * M[:, :, j]
        return r

    for t in range(N):
        SX[:, t] = Sig
        At, Bt, Kt = A[:, t], Bm[:, t], K[:, t]
        Acl = At.copy()                                           # 1
        for k in range(nu):
            Acl = Acl + Bt[:, :, k, None] * Kt[:, None, k, :]
        Z = np.zeros((B, nu, nx))                                  # 2
        for l in range(nx):
            Z = Z + Kt[:, :, l, None] * Sig[:, None, l, :]
        S_u = np.zeros((B, nu, nu))                                # 3 (the lower triangle counts)
        for l in range(nx):
            S_u = S_u + Z[:, :, l, None] * Kt[:, None, :, l]
        if Wus is not None:
            S_u = S_u + Wus
        S_u = mirror(S_u)
        SU[:, t] = S_u
        Y = np.zeros((B, nx, nx))                                  # 4
        for l in range(nx):
            Y = Y + Acl[:, :, l, None] * Sig[:, None, l, :]
        Nx = np.zeros((B, nx, nx))                                 # 5 (the lower triangle counts)
        for l in range(nx):
            Nx = Nx + Acl[:, :, l, None] * Y[:, None, :, l]
        if Ws is not None:
            Nx = Nx + Ws
        if Wus is not None:
            G = np.zeros((B, nx, nu))
            for m in range(nu):
                G = G + Bt[:, :, m, None] * Wus[:, None, m, :]
            H = np.zeros((B, nx, nx))
            for k in range(nu):
                H = H + G[:, :, k, None] * Bt[:, None, :, k]
            Nx = Nx + H
        if cost:                                                   # 6
            c = np.zeros(B)
            r = trace(Qdt, Sig, nx)
            for i in range(nx):
                c = c + r[:, i]
            r = trace(Rdt, S_u, nu)
            for i in range(nu):
                c = c + r[:, i]
            dcost = dcost + c
        Sig = mirror(Nx)
    SX[:, N] = Sig
    if cost:
        c = np.zeros(B)
        r = trace(Qf, Sig, nx)
        for i in range(nx):
            c = c + r[:, i]
        dcost = dcost + c
    if diag:
        SX = np.ascontiguousarray(np.diagonal(SX, axis1=2, axis2=3)); SU = np.ascontiguousarray(np.diagonal(SU, axis1=2, axis2=3))
    return SX, SU, dcost


def cost_matrices(p):
    """(Q dt, R dt, Qf) of a pyapi.Problem, as the library's constant pool holds them"""
    Q = np.asarray(p.Q, dtype=np.float64).reshape(p.nx, p.nx); R = np.asarray(p.R, dtype=np.float64).reshape(p.nu, p.nu)
    return Q * p.dt, R * p.dt, np.asarray(p.Qf, dtype=np.float64).reshape(p.nx, p.nx)


def contractive_stacks(B, N, nx, nu, seed):
    """Synthetic stacks whose closed loop contracts: A = 0.5 * an orthogonal matrix + small noise, small B and K"""
    rng = np.random.default_rng(seed)
    A = np.zeros((B, N, nx, nx))
    for b in range(B):
        for t in range(N):
            q, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
            A[b, t] = 0.5 * q + 0.02 * rng.standard_normal((nx, nx))
    Bm = 0.2 * rng.standard_normal((B, N, nx, nu)); K = 0.2 * rng.standard_normal((B, N, nu, nx))
    return A, Bm, K


def spd(rng, n, scale=1.0, lead=()):
    M = rng.standard_normal(lead + (n, n))
    return scale * (M @ np.swapaxes(M, -1, -2) / n + 0.1 * np.eye(n))


# The largest deviations of covariance() from exact (60-digit) evaluation over the pairs (1,1), (3,2), (4,1), (14,7) at N = 5, as
# tests/test_plan_cov_host.py measures them (profiles/r17_plan_covariance.md): of Sigma_t against the closed form, relative to
# max |Sigma_t| (1.257e-16, at (14,7) with noise), and of dcost against the trace formula, relative to the cost (2.682e-16, at (4,1)).
# Tests that are not bitwise allow 8 x the figure of the quantity they compare.
MEASURED_REL_DEV = 1.257e-16
MEASURED_REL_DEV_COST = 2.682e-16
