"""Helper of tests/test_plan_mc.py and tests/test_plan_mc_every_model.py: numpy restatements of the sums of cddp-cpp_amd/csrc/plan_mc.hpp (the
tree sum over the samples, the moments, stats), the closed loop written out over DevicePlant.step with explicit ascending loops, and the
per-step violation from the rows of tests/test_score_rollouts.py.  Nothing here is imported by the product."""
import numpy as np

from test_score_rollouts import dmax, rows_numpy, rows_probe

SEED = 20261018


def factors(nx, nu, scale=1.0):
    """lower-triangular factors with a full lower triangle: L0 (nx, nx), Lw (nx, nx), Lu (nu, nu)"""
    def tri(n, s, k):
        L = np.zeros((n, n))
        for i in range(n):
            for j in range(i + 1):
                L[i, j] = s * (1.0 if i == j else 0.3 * np.cos(1.0 + i + 2.0 * j + k))
        return L
    return tri(nx, 0.05 * scale, 0), tri(nx, 0.01 * scale, 1), tri(nu, 0.08 * scale, 2)


def tree_sum(v):
    """the tree sum of plan_mc.hpp over the LAST axis: chunks of 64 lanes, absent lanes 0.0, v[l] += v[l ^ m] for m = 1 .. 32, chunk totals
    added in ascending order from chunk 0's"""
    v = np.asarray(v, dtype=np.float64)
    S = v.shape[-1]
    nchunk = (S + 63) // 64
    w = np.zeros(v.shape[:-1] + (nchunk * 64,))
    w[..., :S] = v
    w = w.reshape(v.shape[:-1] + (nchunk, 64))
    lanes = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        w = w + w[..., lanes ^ m]
    total = w[..., 0, 0]
    for k in range(1, nchunk):
        total = total + w[..., k, 0]
    return total


def moments(D, diag=False):
    """D (B, S, T, n): the deviations of the samples -> mean (B, T, n), cov (B, T, n, n) (diag: (B, T, n)) by the header's formulas"""
    B, S, T, n = D.shape
    Dm = np.moveaxis(D, 1, -1)                                   # (B, T, n, S)
    with np.errstate(all="ignore"):
        m1 = tree_sum(Dm)
        mean = m1 / float(S)
        cov = np.zeros((B, T, n, n))
        for i in range(n):
            for j in range(i + 1):
                if S > 1:
                    q = tree_sum(Dm[:, :, i] * Dm[:, :, j])
                    c = (q - (m1[:, :, i] * m1[:, :, j]) / float(S)) / float(S - 1)
                else:
                    c = np.zeros((B, T))
                cov[:, :, i, j] = c; cov[:, :, j, i] = c
    if diag:
        cov = np.ascontiguousarray(np.diagonal(cov, axis1=2, axis2=3))
    return mean, cov


def stats(cost, viol, viol_tol):
    """stats (B, 8) of plan_mc.hpp from cost, viol (B, S)"""
    B, S = cost.shape
    out = np.zeros((B, 8))
    with np.errstate(all="ignore"):
        out[:, 0] = (np.isfinite(cost) & np.isfinite(viol)).sum(axis=1)
        out[:, 1] = (viol > viol_tol).sum(axis=1)
        mean = tree_sum(cost) / float(S)
        out[:, 2] = mean
        e = cost - mean[:, None]
        out[:, 3] = tree_sum(e * e) / float(S - 1) if S > 1 else 0.0
        out[:, 6] = tree_sum(viol) / float(S)
        for b in range(B):
            cmin = cmax = cost[b, 0]; vmax = viol[b, 0]
            for c in range(1, S):
                if cost[b, c] < cmin:
                    cmin = cost[b, c]
                if cmax < cost[b, c]:
                    cmax = cost[b, c]
                if vmax < viol[b, c]:
                    vmax = viol[b, c]
            out[b, 4] = cmin; out[b, 5] = cmax; out[b, 7] = vmax
    return out


def viol_steps(api, p, X, U):
    """v (B, S, N + 1): v_t = the path rows of step t folded from 0 (the stacked order: constraint objects sorted by name), v_N the
    terminal inequality rows -- the fold of test_score_rollouts.viol_reference taken per step"""
    B, S, N = U.shape[:3]
    v = np.zeros((B, S, N + 1))
    for c in sorted(p._cons, key=lambda c: c.name):
        rows = rows_numpy(api, p, c, X, U)
        if rows is None:
            rows = rows_probe(api, c, X, U)
        for g in rows:
            v[:, :, :N] = dmax(v[:, :, :N], g)
    for tc in sorted(p._terms, key=lambda c: c.name):
        if tc.kind != api.TERM_INEQUALITY:
            continue
        nx = X.shape[-1]
        for r in range(tc.dim):
            s = np.zeros((B, S))
            for j in range(nx):
                s = s + tc.A[r * nx + j] * X[:, :, -1, j]
            v[:, :, N] = dmax(v[:, :, N], s - tc.b[r])
    return v


def closed_loop(plant, Xp, Up, K, x0, Z0, E, Wn, box=None):
    """The rollout of the header written out: plant is a DevicePlant of batch B * S (trajectory b's block S times over, no box of its
    own: the clip is restated here), Xp (B, N + 1, nx), Up (B, N, nu), K (B, N, nu, nx) the plan, x0 (B, nx) the base state, Z0 / E / Wn
    the coloured noise (None: no such source).  -> X (B, S, N + 1, nx), U (B, S, N, nu) as applied"""
    B, N, nu = Up.shape
    nx = Xp.shape[2]
    S = next(a for a in (Z0, E, Wn) if a is not None).shape[1]
    x = np.repeat(x0[:, None, :], S, axis=1)
    if Z0 is not None:
        x = x + Z0
    X = np.zeros((B, S, N + 1, nx)); U = np.zeros((B, S, N, nu))
    X[:, :, 0] = x
    for t in range(N):
        uc = np.repeat(Up[:, None, t, :], S, axis=1)
        if E is not None:
            uc = uc + E[:, :, t]
        u = np.zeros((B, S, nu))
        for i in range(nu):
            s = np.zeros((B, S))
            for j in range(nx):
                s = s + K[:, None, t, i, j] * (x[:, :, j] - Xp[:, None, t, j])
            u[:, :, i] = uc[:, :, i] + s
        if box is not None:
            u = np.minimum(np.maximum(u, box[0]), box[1])
        U[:, :, t] = u
        w = None if Wn is None else np.ascontiguousarray(Wn[:, :, t].reshape(B * S, nx))
        x = plant.step(np.ascontiguousarray(x.reshape(B * S, nx)), np.ascontiguousarray(u.reshape(B * S, nu)), w).reshape(B, S, nx)
        X[:, :, t + 1] = x
    return X, U
