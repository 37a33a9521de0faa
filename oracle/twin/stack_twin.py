"""Stack-level numpy reference of the stack-fed sweeps (cddp-cpp_amd/csrc/stacks.hip, stacks_coop.hpp, stacks_te.hpp) -- TEST
INFRASTRUCTURE, never imported by the product.

Every function takes ONE trajectory's arrays exactly as a host plug-in hands them to HipStackSolver (float64, step-major: fx [N][nx][nx],
fu [N][nx][nu], lx [N][nx], lu [N][nu], lxx [N][nx][nx], luu [N][nu][nu], lux [N][nu][nx], VxN [nx], VxxN [nx][nx]; path rows y, s, g [N][m],
Gx [N][m][nx], Gu [N][m][nu]; Hessian stacks Fxx [N][nx][nx][nx], Fuu [N][nx][nu][nu], Fux [N][nx][nu][nx]; defects d [N][nx]) and returns
a dict with the outputs the handle downloads: ok, K, k, Vx, Vxx, dV, inf_du, inf_pr, inf_comp, step_norm, alpha_pr_max, alpha_du_max and,
on the path branches, ky, Ky, ks, Ks (and dX for IPDDP_PATH).

The recursions are the ones of oracle/twin/cddp_twin.py (Twin.clddp_backward, Twin.ipddp_backward, Twin.linear_rollout_directions,
Twin.max_step_sizes), msipddp_twin.py and cddp_twin_te.py, restated on stacks instead of a plant: the same expressions in the same order,
so that fed the stacks of a Twin iterate they reproduce Twin.backward() to rounding (tests/test_stack_twin.py pins that).  They are NOT a
restatement of the kernels."""
import numpy as np

import cddp_twin as T
import cddp_twin_te as TE
import logddp_twin as LG
import msipddp_twin as MS


def _tensor_terms(hess, t, w, Q_xx, Q_ux, Q_uu):
    """Twin.add_tensor_terms (ipddp_solver.cpp:1070-1082, 1396-1408) on the stacked dt-scaled tensors of step t."""
    Fxx, Fuu, Fux = hess[0][t], hess[1][t], hess[2][t]
    for i in range(len(w)):
        Q_xx = Q_xx + w[i] * Fxx[i]; Q_ux = Q_ux + w[i] * Fux[i]; Q_uu = Q_uu + w[i] * Fuu[i]
    return Q_xx, Q_ux, Q_uu


def _empty(N, nx, nu):
    return dict(ok=False, K=np.zeros((N, nu, nx)), k=np.zeros((N, nu)), Vx=np.zeros((N + 1, nx)), Vxx=np.zeros((N + 1, nx, nx)),
                dV=np.zeros(2), inf_du=0.0, inf_pr=0.0, inf_comp=0.0, step_norm=0.0, alpha_pr_max=1.0, alpha_du_max=1.0)


def clddp(st, reg, opt, box=None, U=None, k_warm=None):
    """CLDDPSolver::backwardPass (clddp_solver.cpp:79-204), Twin.clddp_backward: eigenvalue PD test, dense inverse, reg in the factor only,
    inf_du scaled by termination_scaling_max_factor.  box = (lower, upper) with the control stack U: BoxQP (boxqp.cpp:25-250) on
    [lower - u_t, upper - u_t], warm-started from k_warm [N][nu] (the previous sweep's k), which is updated in place step by step as the
    sweep writes it.  out["free"] [N][nu] marks the BoxQP's free rows."""
    fx, fu = st["fx"], st["fu"]
    N, nx, nu = fx.shape[0], fx.shape[1], fu.shape[2]
    out = _empty(N, nx, nu)
    free_rows = np.ones((N, nu), dtype=bool)
    V_x = np.array(st["VxN"], float); V_xx = np.array(st["VxxN"], float)
    out["Vx"][N], out["Vxx"][N] = V_x, V_xx
    dV = np.zeros(2); norm_Vx = float(np.sum(np.abs(V_x))); Qu_err = 0.0; step_norm = 0.0
    for t in range(N - 1, -1, -1):
        A, B = fx[t], fu[t]
        lx, lu, lxx, luu, lux = st["lx"][t], st["lu"][t], st["lxx"][t], st["luu"][t], st["lux"][t]
        Q_x = lx + A.T @ V_x; Q_u = lu + B.T @ V_x
        Q_xx = lxx + A.T @ V_xx @ A; Q_ux = lux + B.T @ V_xx @ A; Q_uu = luu + B.T @ V_xx @ B
        Q_uu_reg = Q_uu.copy(); Q_uu_reg[np.diag_indices(nu)] += reg
        if np.min(np.linalg.eigvals(Q_uu_reg).real) <= 0:     # EigenSolver, :133-140
            out["free"] = free_rows
            return out
        if box is None:
            H = np.linalg.inv(Q_uu_reg)
            k = -H @ Q_u; K = -H @ Q_ux
        else:
            lb = box[0] - U[t]; ub = box[1] - U[t]
            x, status, free, fac = T.boxqp(Q_uu_reg, Q_u, lb, ub, k_warm[t].copy(), opt)
            if status in ("HESSIAN_NOT_PD", "NO_DESCENT"):
                out["free"] = free_rows
                return out
            k = x; K = np.zeros((nu, nx))
            idx = np.where(free)[0]
            if idx.size > 0:
                K[idx, :] = -fac.solve(Q_ux[idx, :])
            free_rows[t] = free
            k_warm[t] = k
        out["k"][t], out["K"][t] = k, K
        dV += np.array([float(Q_u @ k), 0.5 * float(k @ (Q_uu @ k))])
        V_x = Q_x + K.T @ Q_uu @ k + Q_ux.T @ k + K.T @ Q_u
        V_xx = Q_xx + K.T @ Q_uu @ K + Q_ux.T @ K + K.T @ Q_ux
        V_xx = 0.5 * (V_xx + V_xx.T)
        out["Vx"][t], out["Vxx"][t] = V_x, V_xx
        norm_Vx += float(np.sum(np.abs(V_x))); Qu_err = max(Qu_err, float(np.max(np.abs(Q_u))))
        step_norm = max(step_norm, float(np.max(np.abs(k))))
    sf = opt["termination_scaling_max_factor"]
    sf = max(sf, norm_Vx / (N * nx)) / sf
    out.update(ok=True, dV=dV, inf_du=Qu_err / sf, step_norm=step_norm, free=free_rows)
    return out


def ipddp(st, reg, hess=None):
    """Unconstrained branch of IPDDPSolver::backwardPass (ipddp_solver.cpp:1048-1118), Twin.ipddp_backward with m = 0; hess: the
    F_xx / F_uu / F_ux terms weighted by V_x of step t + 1 (use_ilqr = false)."""
    fx, fu = st["fx"], st["fu"]
    N, nx, nu = fx.shape[0], fx.shape[1], fu.shape[2]
    out = _empty(N, nx, nu)
    V_x = np.array(st["VxN"], float); V_xx = T.sym(np.array(st["VxxN"], float))
    out["Vx"][N], out["Vxx"][N] = V_x, V_xx
    dV = np.zeros(2); inf_du = step_norm = 0.0
    for t in range(N - 1, -1, -1):
        A, B = fx[t], fu[t]
        lx, lu, lxx, luu, lux = st["lx"][t], st["lu"][t], st["lxx"][t], st["luu"][t], st["lux"][t]
        Q_x = lx + A.T @ V_x; Q_u = lu + B.T @ V_x
        Q_xx = lxx + A.T @ V_xx @ A; Q_ux = lux + B.T @ V_xx @ A; Q_uu = luu + B.T @ V_xx @ B
        if hess is not None:
            Q_xx, Q_ux, Q_uu = _tensor_terms(hess, t, V_x, Q_xx, Q_ux, Q_uu)
        Q_uu = T.sym(Q_uu); Q_uu[np.diag_indices(nu)] += reg
        f = T.EigenLDLT(Q_uu)
        if not f.ok:
            return out
        k = -f.solve(Q_u); K = -f.solve(Q_ux)
        out["k"][t], out["K"][t] = k, K
        V_x = Q_x + K.T @ Q_u + Q_ux.T @ k + K.T @ Q_uu @ k
        V_xx = T.sym(Q_xx + K.T @ Q_ux + Q_ux.T @ K + K.T @ Q_uu @ K)
        out["Vx"][t], out["Vxx"][t] = V_x, V_xx
        dV[0] += float(k @ Q_u); dV[1] += 0.5 * float(k @ (Q_uu @ k))
        inf_du = max(inf_du, float(np.max(np.abs(Q_u)))); step_norm = max(step_norm, float(np.max(np.abs(k))))
    out.update(ok=True, dV=dV, inf_du=inf_du, step_norm=step_norm)
    return out


def ipddp_path(st, reg, mu, opt, hess=None):
    """Path branch of IPDDPSolver::backwardPass (ipddp_solver.cpp:1355-1568, Twin.ipddp_backward), the linear-policy rollout from dx0 = 0
    with dS / dY (:1511-1532, Twin.linear_rollout_directions) and computeMaxStepSizes (:2939-2988, Twin.max_step_sizes)."""
    fx, fu = st["fx"], st["fu"]
    N, nx, nu = fx.shape[0], fx.shape[1], fu.shape[2]
    m = st["y"].shape[1]
    out = _empty(N, nx, nu)
    out.update(ky=np.zeros((N, m)), Ky=np.zeros((N, m, nx)), ks=np.zeros((N, m)), Ks=np.zeros((N, m, nx)), dX=np.zeros((N + 1, nx)))
    V_x = np.array(st["VxN"], float); V_xx = T.sym(np.array(st["VxxN"], float))
    out["Vx"][N], out["Vxx"][N] = V_x, V_xx
    dV = np.zeros(2); inf_du = inf_pr = inf_comp = step_norm = 0.0
    for t in range(N - 1, -1, -1):
        A, B = fx[t], fu[t]
        Q_yx, Q_yu = st["Gx"][t], st["Gu"][t]
        y, s, g = st["y"][t], st["s"][t], st["g"][t]
        lx, lu, lxx, luu, lux = st["lx"][t], st["lu"][t], st["lxx"][t], st["luu"][t], st["lux"][t]
        Q_x = lx + Q_yx.T @ y + A.T @ V_x
        Q_u = lu + Q_yu.T @ y + B.T @ V_x
        Q_xx = lxx + A.T @ V_xx @ A; Q_ux = lux + B.T @ V_xx @ A; Q_uu = luu + B.T @ V_xx @ B
        if hess is not None:
            Q_xx, Q_ux, Q_uu = _tensor_terms(hess, t, V_x, Q_xx, Q_ux, Q_uu)
        s_safe = np.maximum(s, max(mu * 1e-3, T.EPS_SLACK))
        YS = np.array([T.clip_pos(y[i], s_safe[i]) for i in range(m)])
        rp = g + s; rc = y * s - mu; rhat = y * rp - rc
        Q_uu_reg = T.sym(Q_uu) + Q_yu.T @ np.diag(YS) @ Q_yu
        Q_uu_reg[np.diag_indices(nu)] += reg
        f = T.EigenLDLT(Q_uu_reg)
        if not f.ok:
            return out
        Sir = np.array([T.clip_sgn(rhat[i], s_safe[i]) for i in range(m)])
        big = np.zeros((nu, 1 + nx))
        big[:, 0] = Q_u + Q_yu.T @ Sir
        big[:, 1:] = Q_ux + Q_yu.T @ np.diag(YS) @ Q_yx
        kK = -f.solve(big)
        k = kK[:, 0].copy(); K = kK[:, 1:].copy()
        out["k"][t], out["K"][t] = k, K
        temp = Q_yu @ k
        out["ky"][t] = np.array([T.clip_sgn(rhat[i] + y[i] * temp[i], s_safe[i]) for i in range(m)])
        out["Ky"][t] = np.clip(np.diag(YS) @ (Q_yx + Q_yu @ K), -T.MAX_BARRIER_RATIO, T.MAX_BARRIER_RATIO)
        out["ks"][t] = -rp - temp
        out["Ks"][t] = -Q_yx - Q_yu @ K
        Q_u = Q_u + Q_yu.T @ Sir; Q_x = Q_x + Q_yx.T @ Sir
        Q_xx = Q_xx + Q_yx.T @ np.diag(YS) @ Q_yx
        Q_ux = Q_ux + Q_yu.T @ np.diag(YS) @ Q_yx
        Q_uu = Q_uu + Q_yu.T @ np.diag(YS) @ Q_yu
        dV[0] += float(k @ Q_u); dV[1] += 0.5 * float(k @ (Q_uu @ k))
        V_x = Q_x + K.T @ Q_u + Q_ux.T @ k + K.T @ Q_uu @ k
        V_xx = T.sym(Q_xx + K.T @ Q_ux + Q_ux.T @ K + K.T @ Q_uu @ K)
        out["Vx"][t], out["Vxx"][t] = V_x, V_xx
        inf_du = max(inf_du, float(np.max(np.abs(Q_u))))
        inf_pr = max(inf_pr, float(np.max(np.abs(rp)))); inf_comp = max(inf_comp, float(np.max(np.abs(rc))))
        step_norm = max(step_norm, float(np.max(np.abs(k))))
    # rolloutLinearPolicy from dx0 = 0, dS / dY (Twin.linear_rollout_directions)
    dX = np.zeros((N + 1, nx)); dU = np.zeros((N, nu))
    for t in range(N):
        dU[t] = out["k"][t] + out["K"][t] @ dX[t]
        dX[t + 1] = fx[t] @ dX[t] + fu[t] @ dU[t] + np.zeros(nx)
    dS = np.zeros((N, m)); dY = np.zeros((N, m))
    for t in range(N):
        dS[t] = out["ks"][t] + out["Ks"][t] @ dX[t]
        dY[t] = np.clip(out["ky"][t] + out["Ky"][t] @ dX[t], -T.MAX_BARRIER_RATIO, T.MAX_BARRIER_RATIO)
    # computeMaxStepSizes (Twin.max_step_sizes)
    tau = max(opt["min_fraction_to_boundary"], 1.0 - mu)
    apr = adu = 1.0
    for t in range(N):
        for i in range(m):
            if dS[t, i] < 0.0:
                apr = min(apr, -tau * st["s"][t, i] / dS[t, i])
            if dY[t, i] < 0.0:
                adu = min(adu, -tau * st["y"][t, i] / dY[t, i])
    out.update(ok=True, dV=dV, inf_du=inf_du, inf_pr=inf_pr, inf_comp=inf_comp, step_norm=step_norm, dX=dX, dS=dS, dY=dY,
               alpha_pr_max=min(max(apr, 0.0), 1.0), alpha_du_max=min(max(adu, 0.0), 1.0))
    return out


def logddp(st, reg, hess=None):
    """LogDDPSolver::backwardPass (logddp_solver.cpp:470-575) on cost stacks that already carry the barrier terms: logddp_twin.backward
    with cons = [] (stack-level already)."""
    N, nx, nu = st["fx"].shape[0], st["fx"].shape[1], st["fu"].shape[2]
    H = None if hess is None else [(hess[0][t], hess[1][t], hess[2][t]) for t in range(N)]
    ok, K, k, Vx, Vxx, dV, qu_err = LG.backward(list(st["fx"]), list(st["fu"]), st["lx"], st["lu"], st["lxx"], st["luu"], st["lux"],
                                                 st["VxN"], st["VxxN"], [], None, None, 0.0, 0.0, reg, hess=H)
    out = _empty(N, nx, nu)
    if ok:
        out.update(ok=True, K=K, k=k, Vx=Vx, Vxx=Vxx, dV=dV, inf_du=qu_err, step_norm=float(np.max(np.abs(k))))
    return out


def msipddp(st, reg, d):
    """MSIPDDPSolver::backwardPass without path constraints (msipddp_solver.cpp:1112-1208): msipddp_twin.backward (stack-level already)."""
    N, nx, nu = st["fx"].shape[0], st["fx"].shape[1], st["fu"].shape[2]
    r = MS.backward(list(st["fx"]), list(st["fu"]), st["lx"], st["lu"], st["lxx"], st["luu"], st["lux"], st["VxN"], st["VxxN"], d,
                    np.zeros((N, nx)), reg)
    out = _empty(N, nx, nu)
    if r[0]:
        out.update(ok=True, K=r[1], k=r[2], Vx=r[3], Vxx=r[4], dV=r[5], inf_du=r[6], step_norm=r[7])
    return out


def msipddp_path(st, reg, mu, d):
    """The constrained branch of MSIPDDPSolver::backwardPass (msipddp_solver.cpp:1222-1420), restated from msipddp_twin.MSIPDDP.backward_pass
    on stacks: plain ratios y / s and rhat / s (no floor, no clip), the defects through V_x + V_xx d_t, and line 1398's (nx x nu) product
    added to Q_ux (transposed for nu = 1, elementwise for nx = nu).  inf_pr is max |g + s| (the solver class adds the defect norm on top)."""
    fx, fu = st["fx"], st["fu"]
    N, nx, nu = fx.shape[0], fx.shape[1], fu.shape[2]
    m = st["y"].shape[1]
    if not (nu == 1 or nx == nu):
        raise ValueError("msipddp_solver.cpp:1398 defines Q_ux only for nu = 1 or nx = nu")
    out = _empty(N, nx, nu)
    out.update(ky=np.zeros((N, m)), Ky=np.zeros((N, m, nx)), ks=np.zeros((N, m)), Ks=np.zeros((N, m, nx)))
    V_x = np.array(st["VxN"], float); V_xx = np.array(st["VxxN"], float); V_xx = 0.5 * (V_xx + V_xx.T)
    out["Vx"][N], out["Vxx"][N] = V_x, V_xx
    dV = np.zeros(2); idu = ipr = icomp = snorm = 0.0
    for t in range(N - 1, -1, -1):
        A, B = fx[t], fu[t]
        y, s, g = st["y"][t], st["s"][t], st["g"][t]
        Qyx, Qyu = st["Gx"][t], st["Gu"][t]
        w = V_x + V_xx @ d[t]
        Q_x = st["lx"][t] + Qyx.T @ y + A.T @ w
        Q_u = st["lu"][t] + Qyu.T @ y + B.T @ w
        Q_xx = st["lxx"][t] + A.T @ V_xx @ A
        Q_ux = st["lux"][t] + B.T @ V_xx @ A
        Q_uu = st["luu"][t] + B.T @ V_xx @ B
        ys = y / s
        pres = g + s; cres = y * s - mu; rhat = y * pres - cres
        Qr = 0.5 * (Q_uu + Q_uu.T)
        Qr = Qr + (Qyu.T * ys) @ Qyu
        Qr[np.diag_indices(nu)] += reg
        f = T.EigenLDLT(Qr)
        if not f.ok:
            return out
        sir = rhat / s
        rhs0 = Q_u + Qyu.T @ sir
        rhs1 = Q_ux + (Qyu.T * ys) @ Qyx
        k_u = -f.solve(rhs0); K_u = -f.solve(rhs1)
        out["k"][t], out["K"][t] = k_u, K_u
        temp = Qyu @ k_u
        out["ky"][t] = (rhat + y * temp) / s
        out["Ky"][t] = ys[:, None] * (Qyx + Qyu @ K_u)
        out["ks"][t] = -pres - temp
        out["Ks"][t] = -Qyx - Qyu @ K_u
        Q_u = Q_u + Qyu.T @ sir
        Q_x = Q_x + Qyx.T @ sir
        Q_xx = Q_xx + (Qyx.T * ys) @ Qyx
        P = (Qyx.T * ys) @ Qyu                   # :1398
        Q_ux = Q_ux + (P.T if nu == 1 else P)
        Q_uu = Q_uu + (Qyu.T * ys) @ Qyu
        dV = dV + np.array([float(k_u @ Q_u), 0.5 * float(k_u @ (Q_uu @ k_u))])
        V_x_n = Q_x + K_u.T @ Q_u + Q_ux.T @ k_u + K_u.T @ Q_uu @ k_u
        V_xx_n = Q_xx + K_u.T @ Q_ux + Q_ux.T @ K_u + K_u.T @ Q_uu @ K_u
        ipr = max(ipr, float(np.max(np.abs(pres)))); icomp = max(icomp, float(np.max(np.abs(cres))))
        V_x, V_xx = V_x_n, 0.5 * (V_xx_n + V_xx_n.T)
        out["Vx"][t], out["Vxx"][t] = V_x, V_xx
        idu = max(idu, float(np.max(np.abs(Q_u)))); snorm = max(snorm, float(np.max(np.abs(k_u))))
    out.update(ok=True, dV=dV, inf_du=idu, inf_pr=ipr, inf_comp=icomp, step_norm=snorm)
    return out


def term_eq(st, reg, HT, bT, lam_prev, mu, reg_scale, reg_exponent):
    """The reduced-LQR branch (ipddp_solver.cpp:478-639, 1252-1268) on the LQ stacks of the terminal-equality route (fx = A, fu = B,
    lx = q, lu = r, lxx = Q, luu = R without the regularisation, lux = M as [N][nx][nu], VxN = q_N, VxxN = Q_N):
    cddp_twin_te.terminal_equality_lqr + rollout_linear.  Returns K, k, Vxx (= P), Vx (= p), dlam, dX, inf_du, step_norm."""
    A, B = st["fx"], st["fu"]
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    Q = list(st["lxx"]) + [st["VxxN"]]; q = list(st["lx"]) + [st["VxN"]]
    R = [st["luu"][t] + reg * np.eye(nu) for t in range(N)]
    ok, K, k, P, p, _, lam_d = TE.terminal_equality_lqr(Q, q, R, list(st["lu"]), list(st["lux"]), list(A), list(B), [np.zeros(nx)] * N,
                                                        np.zeros(nx), HT, bT, mu, reg_scale, reg_exponent, lam_prev)
    out = _empty(N, nx, nu)
    if not ok:
        return out
    dX, _ = TE.rollout_linear(list(A), list(B), [np.zeros(nx)] * N, K, k, np.zeros(nx))
    inf_du = max(float(np.max(np.abs(st["lu"][t] + B[t].T @ p[t + 1]))) for t in range(N))
    out.update(ok=True, K=np.stack(K), k=np.stack(k), Vx=np.stack(p), Vxx=np.stack(P), dlam=lam_d, dX=np.stack(dX), inf_du=inf_du,
               step_norm=max(float(np.max(np.abs(v))) for v in k))
    return out


def retry(sweep, reg, opt):
    """The "increase the regularisation and retry" loop of CDDPSolverBase::solve (cddp_solver_base.cpp:93-111) around one sweep(reg) ->
    dict, with the kernels' rule: reg *= update_factor, a zero regularisation (a fixed point of the product) restarts at reg_min_value
    (reg_max_value when that is 0), capped at reg_max_value; the loop ends, unsuccessful, once reg reaches the cap.  Returns the last
    attempt's outputs with out["reg"] = the regularisation of that attempt and out["retries"] = the number of increases."""
    f, rmax = opt["reg_update_factor"], opt["reg_max_value"]
    n = 0
    while True:
        out = sweep(reg)
        if out["ok"] or not (f > 1.0):
            break
        reg = reg * f
        if not (reg > 0.0):
            reg = opt["reg_min_value"] if opt["reg_min_value"] > 0.0 else rmax
        reg = min(reg, rmax)
        n += 1
        if reg >= rmax:
            break
    out["reg"] = reg; out["retries"] = n
    return out
