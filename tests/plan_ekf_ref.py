"""The extended Kalman filter of include/cddp_hip.h ("extended Kalman filter on the device") restated in numpy: the reference of the
bitwise checks of tests/test_ekf.py, test_ekf_every_model.py, test_mpc_ekf.py (GPU) and of tests/test_ekf_host.py (the C++ step bodies
of csrc/ekf.hpp).

The covariance algebra is plan_kf_ref's (the row-at-a-time Joseph update) and plan_cov_ref's (A S A^T + W + B Wu B^T); f and jac come
from a model object: ProbeModel evaluates them through a build of the plant probe (its host build is the model structs in the kernels' own
sin / cos: the reference of every bitwise check), HostModel through pyapi.model_eval (the library's host build, host libm), LtiModel in numpy.
Vectorised over the batch; every accumulation loop is written out with its index ascending from the stated start value.  Comparisons
are by value (same(): NaN = NaN, -0.0 = 0.0).  Nothing here touches a device."""
import numpy as np

import plan_kf_ref as PK
from plan_cov_ref import mirror, same  # noqa: F401  (same: re-exported for the tests)


def clip(u, lower, upper):
    """fmin(fmax(u, lower), upper), only with a box"""
    return u if lower is None else np.minimum(np.maximum(u, lower), upper)


class HostModel:
    """f and jac of a built-in plant through pyapi.model_eval, one trajectory at a time.  params: (n,) shared or (B, n)."""

    def __init__(self, api, model, integrator, dt, nx, nu, params=(), lower=None, upper=None):
        self.api, self.model, self.integrator, self.dt, self.nx, self.nu = api, model, integrator, dt, nx, nu
        self.params = np.asarray(params, dtype=np.float64)
        self.lower = None if lower is None else np.asarray(lower, dtype=np.float64)
        self.upper = None if upper is None else np.asarray(upper, dtype=np.float64)

    def _p(self, b):
        return list(self.params[b] if self.params.ndim == 2 else self.params)

    def step(self, x, u):
        return np.stack([self.api.model_eval(self.model, self.integrator, self.dt, self._p(b), self.nx, self.nu, x[b], u[b], want=("step",))["step"]
                         for b in range(x.shape[0])])

    def jac(self, x, u):
        J = [self.api.model_eval(self.model, self.integrator, self.dt, self._p(b), self.nx, self.nu, x[b], u[b], want=("jac",))["jac"] for b in range(x.shape[0])]
        return np.stack([j[0] for j in J]), np.stack([j[1] for j in J])


class ProbeModel:
    """f and jac of a built-in plant through a build of the plant probe (tests/plant_probe.py): its HOST build, g++ with
    -DCDDP_TRIG_SHARED=1, is the same model structs in the kernels' own sin / cos (pyapi.model_eval keeps the host libm), so a reference
    made with it is bitwise what the device computes; its device build is the gfx950 code itself.  params: None = the probe table's,
    (n,) shared or (B, n) per trajectory (the derived block is plant_probe.p32's)."""

    def __init__(self, PP, lib, tag, integrator, params=None, lower=None, upper=None):
        import copy
        self.PP, self.lib, self.tag, self.integrator = PP, lib, tag, integrator
        pl = PP.BY_TAG[tag]
        self.nx, self.nu, self.dt = pl.nx, pl.nu, pl.dt
        pv = np.asarray(pl.params if params is None else params, dtype=np.float64)
        blocks = []
        for row in (pv if pv.ndim == 2 else pv[None]):
            q = copy.copy(pl); q.params = list(row)
            blocks.append(PP.p32(q))
        self.P = np.stack(blocks, axis=1)                                  # (32, 1) or (32, B)
        self.lower = None if lower is None else np.asarray(lower, dtype=np.float64)
        self.upper = None if upper is None else np.asarray(upper, dtype=np.float64)

    def _pack(self, x, u, step):
        B = x.shape[0]
        P = self.P if self.P.shape[1] == B else np.repeat(self.P[:, :1], B, axis=1)
        rows = ([np.full((1, B), float(self.integrator)), np.full((1, B), self.dt)] if step else []) + [P, x.T, u.T]
        return np.ascontiguousarray(np.vstack(rows))

    def step(self, x, u):
        return self.PP.run(self.lib, "step_" + self.tag, self._pack(x, u, True))[:self.nx].T.copy()

    def jac(self, x, u):
        J = self.PP.run(self.lib, "jac_" + self.tag, self._pack(x, u, False)).T
        nx, nu = self.nx, self.nu
        return J[:, :nx * nx].reshape(-1, nx, nx).copy(), J[:, nx * nx:].reshape(-1, nx, nu).copy()


class LtiModel:
    """x+ = A x + B u as LTIModel::step sums it (s over A x, t over B u, s + t), and its continuous-equivalent Jacobians (A - I) / dt, B / dt"""

    def __init__(self, A, Bm, dt, lower=None, upper=None):
        self.A, self.Bm, self.dt = np.asarray(A, dtype=np.float64), np.asarray(Bm, dtype=np.float64), dt
        self.nx, self.nu = self.Bm.shape
        self.lower = None if lower is None else np.asarray(lower, dtype=np.float64)
        self.upper = None if upper is None else np.asarray(upper, dtype=np.float64)

    def step(self, x, u):
        s = np.zeros_like(x); t = np.zeros_like(x)
        for j in range(self.nx):
            s = s + self.A[None, :, j] * x[:, None, j]
        for j in range(self.nu):
            t = t + self.Bm[None, :, j] * u[:, None, j]
        return s + t

    def jac(self, x, u):
        B = x.shape[0]
        Fx = (self.A - np.eye(self.nx)) / self.dt
        return np.broadcast_to(Fx, (B,) + Fx.shape).copy(), np.broadcast_to(self.Bm / self.dt, (B,) + self.Bm.shape).copy()


def batched(M, B, shape):
    return None if M is None else np.ascontiguousarray(np.broadcast_to(np.asarray(M, dtype=np.float64), (B,) + shape))


def measure(C, x, yn=None):
    """y[r] = m (+ yn[r]), m = sum_j C[r][j] x[j] from 0.  C (B, ny, nx), x (B, nx)"""
    m = np.zeros(C.shape[:2])
    for j in range(C.shape[2]):
        m = m + C[:, :, j] * x[:, None, j]
    return m if yn is None else m + yn


def update(xh, P, C, v, y, skip_nan=False):
    """All rows of one measurement.  xh (B, nx), P (B, nx, nx), C (B, ny, nx), v, y (B, ny) -> xh, P, nis (B,), failed (B,) bool"""
    B = xh.shape[0]
    nis = np.zeros(B); failed = np.zeros(B, dtype=bool)
    with np.errstate(all="ignore"):
        for r in range(C.shape[1]):
            c = C[:, r]
            h = PK.h_vec(P, c)
            s = PK.innovation(v[:, r], c, h)
            m = np.zeros(B)
            for j in range(c.shape[1]):
                m = m + c[:, j] * xh[:, j]
            e = y[:, r] - m
            g = h / s[:, None]
            skipped = np.isnan(y[:, r]) if skip_nan else np.zeros(B, dtype=bool)
            bad = ~skipped & ~(s > 0.0)
            go = ~skipped & ~bad
            Pn, _ = PK.joseph(P, np.zeros_like(P), h, s)
            xh = np.where(go[:, None], xh + g * e[:, None], xh)
            P = np.where(go[:, None, None], Pn, P)
            nis = np.where(go, nis + (e * e) / s, nis)
            failed = failed | bad
    return xh, P, nis, failed


def predict(model, xh, P, u, Ws=None, Wus=None):
    """u (B, nu) commanded; Ws / Wus (B, n, n) mirrored or None -> xh, P"""
    nx = xh.shape[1]
    with np.errstate(all="ignore"):
        us = clip(u, model.lower, model.upper)
        Fx, Fu = model.jac(xh, us)
        h = model.dt
        A = h * Fx
        idx = np.arange(nx)
        A[:, idx, idx] = A[:, idx, idx] + 1.0
        Bm = h * Fu
        return model.step(xh, us), PK.propagate(A, P, Ws, Wus, Bm)


class Filter:
    """The object: xh, P, info and the step count.  C (ny, nx) or (B, ny, nx), v likewise, W / Wu or None."""

    def __init__(self, model, B, C, v, W=None, Wu=None):
        self.model, self.B = model, B
        C = np.asarray(C, dtype=np.float64)
        self.ny = C.shape[-2]
        nx, nu = model.nx, model.nu
        self.C = batched(C, B, (self.ny, nx)); self.v = batched(v, B, (self.ny,))
        self.Ws = None if W is None else batched(mirror(np.asarray(W, dtype=np.float64)), B, (nx, nx))
        self.Wus = None if Wu is None else batched(mirror(np.asarray(Wu, dtype=np.float64)), B, (nu, nu))
        self.xh = np.zeros((B, nx)); self.P = np.zeros((B, nx, nx)); self.info = np.zeros(B, dtype=np.int32); self.t = 0

    def reset(self, xh0, P0):
        nx = self.model.nx
        self.xh = np.array(xh0, dtype=np.float64).reshape(self.B, nx)
        self.P = batched(mirror(np.asarray(P0, dtype=np.float64)), self.B, (nx, nx)).copy()
        self.info[:] = 0; self.t = 0

    def _poison(self):
        dead = self.info != 0
        self.xh = np.where(dead[:, None], np.nan, self.xh); self.P = np.where(dead[:, None, None], np.nan, self.P)
        return dead

    def update(self, y, skip_nan=False):
        self.xh, self.P, nis, failed = update(self.xh, self.P, self.C, self.v, np.asarray(y, dtype=np.float64).reshape(self.B, self.ny), skip_nan)
        self.info[failed & (self.info == 0)] = self.t + 1
        return np.where(self._poison(), np.nan, nis)

    def predict(self, u):
        self.xh, self.P = predict(self.model, self.xh, self.P, np.asarray(u, dtype=np.float64).reshape(self.B, self.model.nu), self.Ws, self.Wus)
        self._poison()
        self.t += 1

    def run(self, Y, U=None, skip_nan=False, diag=False):
        """Y (B, T + 1, ny), U (B, T, nu) -> dict Xh, P, nis, info: the loop over update / predict"""
        T = Y.shape[1] - 1
        Xh, Ps, nis = [], [], []
        for t in range(T + 1):
            if t > 0:
                self.predict(U[:, t - 1])
            nis.append(self.update(Y[:, t], skip_nan)); Xh.append(self.xh.copy()); Ps.append(self.P.copy())
        Pm = np.stack(Ps, axis=1)
        if diag:
            Pm = np.ascontiguousarray(np.diagonal(Pm, axis1=2, axis2=3))
        return {"Xh": np.stack(Xh, axis=1), "P": Pm, "nis": np.stack(nis, axis=1), "info": self.info.copy()}


# The largest deviation of Filter.run from the same recursion evaluated in mpmath at 60 digits (tests/test_ekf_host.py: pendulum, RK4,
# T = 20, ny = 1; xh relative to max |xh|, P relative to max |P|).  Tests that are not bitwise allow 8 x this, floored at 1e-15.
MEASURED_REL_DEV_EKF = 2.446e-15      # P; xh 1.698e-15
