"""The backward Riccati recursion of include/cddp_hip.h ("time-varying LQR tracking gains along a solved plan") restated in numpy: the
reference of the bitwise checks of tests/test_plan_lqr.py and test_plan_lqr_shapes.py (GPU) and of tests/test_plan_lqr_host.py (the C++
step bodies of csrc/plan_lqr.hpp).

Vectorised over the batch and over the elements of a matrix; every accumulation loop is written out with its index ascending, from the
stated start value, and numpy rounds each product and each sum, as the library built with -ffp-contract=off does; / and sqrt are IEEE's.
Comparisons are by value (np.array_equal with NaN = NaN): the header leaves the sign of an exact zero open.  Nothing here touches a
device."""
import numpy as np

from plan_cov_ref import mirror, same  # noqa: F401  (same: re-exported for the tests)


def tvlqr(A, Bm, Qd, Rd, Qf):
    """A (B, N, nx, nx), Bm (B, N, nx, nu); Qd = Q * dt and Qf (nx, nx) or (B, nx, nx), Rd = R * dt (nu, nu) or (B, nu, nu): only their
    lower triangles are looked at.  -> K (B, N, nu, nx), P (B, N + 1, nx, nx), info (B,) int32: 0, or t + 1 of the first step (walking
    backward: the largest t) whose pivot test failed; K_s = 0 and P_s = NaN for every s <= t of such a trajectory."""
    B, N, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]

    def batched(M, n):
        return np.ascontiguousarray(np.broadcast_to(mirror(np.asarray(M, dtype=np.float64)), (B, n, n)))

    Qd = batched(Qd, nx); Rd = batched(Rd, nu)
    P = batched(Qf, nx)
    Ks = np.zeros((B, N, nu, nx)); Ps = np.zeros((B, N + 1, nx, nx)); info = np.zeros(B, dtype=np.int32)
    Ps[:, N] = P
    dead = np.zeros(B, dtype=bool)
    with np.errstate(all="ignore"):                                   # (a dead trajectory walks on, on whatever it holds)
        for t in range(N - 1, -1, -1):
            At, Bt = A[:, t], Bm[:, t]
            M = np.zeros((B, nx, nu))                                  # 1: M[i][k] += P[i][l] * B[l][k]
            for l in range(nx):
                M = M + P[:, :, l, None] * Bt[:, None, l, :]
            Quu = np.zeros((B, nu, nu))                                # 2: Quu[r][c] += B[l][r] * M[l][c]; + Rd (the lower triangle counts)
            for l in range(nx):
                Quu = Quu + Bt[:, l, :, None] * M[:, None, l, :]
            Quu = Quu + Rd
            Qux = np.zeros((B, nu, nx))                                # 3: Qux[k][j] += M[l][k] * A[l][j]
            for l in range(nx):
                Qux = Qux + M[:, l, :, None] * At[:, None, l, :]
            L = np.zeros((B, nu, nu)); ok = np.ones(B, dtype=bool)     # 4
            for r in range(nu):
                for c in range(r):
                    s = Quu[:, r, c]
                    for m in range(c):
                        s = s - L[:, r, m] * L[:, c, m]
                    L[:, r, c] = s / L[:, c, c]
                s = Quu[:, r, r]
                for m in range(r):
                    s = s - L[:, r, m] * L[:, r, m]
                ok = ok & (s > 0.0)
                L[:, r, r] = np.sqrt(s)
            y = np.zeros((B, nu, nx)); z = np.zeros((B, nu, nx))       # 5, all columns at once
            for r in range(nu):
                s = Qux[:, r, :]
                for m in range(r):
                    s = s - L[:, r, m, None] * y[:, m, :]
                y[:, r, :] = s / L[:, r, r, None]
            for r in range(nu - 1, -1, -1):
                s = y[:, r, :]
                for m in range(r + 1, nu):
                    s = s - L[:, m, r, None] * z[:, m, :]
                z[:, r, :] = s / L[:, r, r, None]
            K = -z
            Acl = At.copy()                                            # 6
            for k in range(nu):
                Acl = Acl + Bt[:, :, k, None] * K[:, None, k, :]
            Y = np.zeros((B, nx, nx))                                  # 7: Y[i][j] += P[i][l] * Acl[l][j]
            for l in range(nx):
                Y = Y + P[:, :, l, None] * Acl[:, None, l, :]
            T = np.zeros((B, nu, nx))                                  # 8: T[k][j] += Rd[k][m] * K[m][j]
            for m in range(nu):
                T = T + Rd[:, :, m, None] * K[:, None, m, :]
            S = np.zeros((B, nx, nx))                                  # 9 (the lower triangle counts): S[i][j] += Acl[l][i] * Y[l][j]
            for l in range(nx):
                S = S + Acl[:, l, :, None] * Y[:, None, l, :]
            H = np.zeros((B, nx, nx))
            for k in range(nu):
                H = H + K[:, k, :, None] * T[:, None, k, :]
            S = S + H
            S = S + Qd
            P = mirror(S)
            info[~ok & ~dead] = t + 1
            dead = dead | ~ok
            Ks[:, t] = np.where(dead[:, None, None], 0.0, K)
            Ps[:, t] = np.where(dead[:, None, None], np.nan, P)
    return Ks, Ps, info


def closed_loop_cost(A, Bm, K, dx0, Qd, Rd, Qf):
    """sum_t dx_t^T Qd dx_t + du_t^T Rd du_t, plus dx_N^T Qf dx_N, along the recursion of cddp_hip_plan_jvp (tests/test_plan_sens.py::ref_jvp)
    with the gains K: dx0 (B, nx) -> (B,).  The weights are read through their lower triangles."""
    from test_plan_sens import ref_jvp
    B, N, nx, nu = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    dX, dU = ref_jvp(A, Bm, K, dx0[:, None, :])
    dX = dX[:, 0]; dU = dU[:, 0]
    bc = lambda M, n: np.broadcast_to(mirror(np.asarray(M, dtype=np.float64)), (B, n, n))
    Qd = bc(Qd, nx); Rd = bc(Rd, nu); Qf = bc(Qf, nx)
    c = np.zeros(B)
    for t in range(N):
        c = c + np.einsum("bi,bij,bj->b", dX[:, t], Qd, dX[:, t]) + np.einsum("bi,bij,bj->b", dU[:, t], Rd, dU[:, t])
    return c + np.einsum("bi,bij,bj->b", dX[:, N], Qf, dX[:, N])


def lti_stacks(p, B):
    """The constant stacks of an LTI problem (tests/test_plan_sens.py::lti_problem, Euler: the model's matrices are the step's)"""
    A = np.ascontiguousarray(np.broadcast_to(np.asarray(p.lti_A, dtype=np.float64), (B, p.N, p.nx, p.nx)))
    Bm = np.ascontiguousarray(np.broadcast_to(np.asarray(p.lti_B, dtype=np.float64).reshape(p.nx, p.nu), (B, p.N, p.nx, p.nu)))
    return A, Bm


# The largest deviations of tvlqr() from exact (60-digit) evaluation of the same recursion over the pairs (1,1), (3,2), (4,1), (14,7) at
# N = 5 on plan_cov_ref.contractive_stacks with spd weights, as tests/test_plan_lqr_host.py measures them (profiles/r20_plan_tvlqr.md):
# of K relative to max |K|, of P relative to max |P|, and of the two identities (dx0^T P_0 dx0 against the closed-loop cost of the
# plan_jvp recursion, tr(P_0 Sigma0) against plan_cov_ref.covariance's dcost; synthetic and LTI stacks) relative to their exact value.
# Tests that are not bitwise allow 8 x the figure of the quantity they compare.
MEASURED_REL_DEV_K = 7.662e-16          # at (14, 7)
MEASURED_REL_DEV_P = 4.825e-17          # at (4, 1)
MEASURED_REL_DEV_IDENTITY = 4.411e-16   # on the LTI stacks
