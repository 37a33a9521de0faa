"""Numpy restatements of the five spacecraft plants of the reference (src/dynamics_model/{euler,quaternion,mrp}_attitude.cpp,
spacecraft_twobody.cpp, spacecraft_landing2d.cpp), written from those sources alone: no import of the product (pyapi, pycddp_amd)
or of the C++ oracle.  Each plant has the interface the numpy twin (oracle/twin/cddp_twin.py) takes: nx, nu, f(x, u, t), jac, hess.

Derivatives, as the reference takes them:
  * autodiff plants (the three attitude forms): Jacobians by complex-step differentiation of the autodiff expression (no
    subtraction, no truncation error: autodiff's value to rounding), Hessians by hyper-dual numbers (exact second derivatives);
  * finite-difference plants (two-body, 2-D lander): central differences, h = 2e-5 (helper.hpp:96), of this module's own f;
    the lander's cross Hessian is the base-class autodiff default on ITS autodiff expression (thrust = u0, no max_thrust factor).
"""
import math

import numpy as np


class HyperDual:
    """a + b e1 + c e2 + d e1 e2 with e1^2 = e2^2 = 0: d carries the exact mixed second derivative."""
    __slots__ = ("a", "b", "c", "d")

    def __init__(self, a, b=0.0, c=0.0, d=0.0):
        self.a, self.b, self.c, self.d = float(a), float(b), float(c), float(d)

    @staticmethod
    def lift(v):
        return v if isinstance(v, HyperDual) else HyperDual(v)

    def __add__(self, o):
        o = HyperDual.lift(o); return HyperDual(self.a + o.a, self.b + o.b, self.c + o.c, self.d + o.d)
    __radd__ = __add__

    def __neg__(self):
        return HyperDual(-self.a, -self.b, -self.c, -self.d)

    def __sub__(self, o):
        return self + (-HyperDual.lift(o))

    def __rsub__(self, o):
        return HyperDual.lift(o) - self

    def __mul__(self, o):
        o = HyperDual.lift(o)
        return HyperDual(self.a * o.a, self.a * o.b + self.b * o.a, self.a * o.c + self.c * o.a,
                         self.a * o.d + self.b * o.c + self.c * o.b + self.d * o.a)
    __rmul__ = __mul__

    def unary(self, g, g1, g2):
        return HyperDual(g, g1 * self.b, g1 * self.c, g1 * self.d + g2 * self.b * self.c)

    def __truediv__(self, o):
        o = HyperDual.lift(o)
        return self * o.unary(1.0 / o.a, -1.0 / o.a ** 2, 2.0 / o.a ** 3)

    def __rtruediv__(self, o):
        return HyperDual.lift(o) / self


def val(v):
    if isinstance(v, HyperDual):
        return v.a
    return v.real if isinstance(v, complex) or np.iscomplexobj(v) else v


def sin(v):
    if isinstance(v, HyperDual):
        return v.unary(math.sin(v.a), math.cos(v.a), -math.sin(v.a))
    return np.sin(v)


def cos(v):
    if isinstance(v, HyperDual):
        return v.unary(math.cos(v.a), -math.sin(v.a), -math.cos(v.a))
    return np.cos(v)


def tan(v):
    if isinstance(v, HyperDual):
        t = math.tan(v.a); return v.unary(t, 1.0 + t * t, 2.0 * t * (1.0 + t * t))
    return np.tan(v)


def sqrt(v):
    if isinstance(v, HyperDual):
        r = math.sqrt(v.a); return v.unary(r, 0.5 / r, -0.25 / (v.a * r))
    return np.sqrt(v)


def _mv(M, v):
    return [sum((M[i][j] * v[j] for j in range(len(v))), 0.0) for i in range(len(M))]


def cs_jacobian(f, z, h=1e-30):
    """Complex-step derivative: column j = Im f(z + i h e_j) / h."""
    z = np.asarray(z, dtype=np.float64)
    cols = []
    for j in range(z.size):
        zc = z.astype(np.complex128); zc[j] += 1j * h
        cols.append(np.array([complex(v).imag for v in f(list(zc))]) / h)
    return np.stack(cols, axis=1)


def hd_hessian(f, z):
    """Hessians of every output of f w.r.t. z by hyper-dual numbers: H[i] (n x n)."""
    z = [float(v) for v in z]; n = len(z)
    out = None
    for a in range(n):
        for b in range(a, n):
            zz = [HyperDual(v) for v in z]
            zz[a] = HyperDual(z[a], 1.0, 0.0, 0.0) if a != b else HyperDual(z[a], 1.0, 1.0, 0.0)
            if a != b:
                zz[b] = HyperDual(z[b], 0.0, 1.0, 0.0)
            r = f(zz)
            if out is None:
                out = np.zeros((len(r), n, n))
            for i, v in enumerate(r):
                out[i, a, b] = out[i, b, a] = HyperDual.lift(v).d
    return out


def fd_jacobian(f, z, h=2e-5):
    """helper.hpp:96 finite_difference_jacobian, central differences."""
    z = np.asarray(z, dtype=np.float64); zp = z.copy(); cols = []
    for i in range(z.size):
        zp[i] = z[i] + h; fp = np.asarray(f(zp), dtype=np.float64)
        zp[i] = z[i] - h; fm = np.asarray(f(zp), dtype=np.float64)
        cols.append((fp - fm) / (2.0 * h)); zp[i] = z[i]
    return np.stack(cols, axis=1)


class _Plant:
    """Plants whose Jacobians / Hessians are the autodiff of `_ad(x, u)` (a list expression on any scalar type)."""
    def _split(self, z):
        return z[:self.nx], z[self.nx:]

    def _adz(self, z):
        x, u = self._split(z); return self._ad(x, u)

    def jac(self, x, u, t):
        J = cs_jacobian(self._adz, np.concatenate([x, u]))
        return J[:, :self.nx], J[:, self.nx:]

    def hess(self, x, u, t):
        H = hd_hessian(self._adz, np.concatenate([x, u]))
        n = self.nx
        return H[:, :n, :n].copy(), H[:, n:, n:].copy(), H[:, n:, :n].copy()


class _Attitude(_Plant):
    def __init__(self, inertia):
        self.I = np.asarray(inertia, dtype=np.float64).reshape(3, 3)
        self.Iinv = np.linalg.inv(self.I)

    def _rates(self, w, tau):   # I^-1 (-skew(w) (I w) + tau)
        h = _mv(self.I.tolist(), w)
        v = [w[2] * h[1] - w[1] * h[2] + tau[0], w[0] * h[2] - w[2] * h[0] + tau[1], w[1] * h[0] - w[0] * h[1] + tau[2]]
        return _mv(self.Iinv.tolist(), v)

    def f(self, x, u, t):
        return np.array([val(v) for v in self._ad(list(x), list(u))], dtype=np.float64)


class EulerAttitude(_Attitude):   # euler_attitude.cpp:33-52 / .hpp:159-180, ZYX [psi, theta, phi]
    nx, nu = 6, 3

    def _ad(self, x, u):
        theta, phi = x[1], x[2]
        c_th = cos(theta)
        c_safe = c_th if abs(val(c_th)) >= 1e-9 else (1e-9 if val(c_th) >= 0 else -1e-9)
        E = [[0.0, sin(phi) / c_safe, cos(phi) / c_safe], [0.0, cos(phi), -sin(phi)], [1.0, sin(phi) * tan(theta), cos(phi) * tan(theta)]]
        return _mv(E, x[3:6]) + self._rates(x[3:6], u)


class QuaternionAttitude(_Attitude):   # quaternion_attitude.cpp:33-62 (value: normalised q), 159-183 (autodiff: un-normalised)
    nx, nu = 7, 3

    @staticmethod
    def _kin(q, w):
        O = [[0.0, -w[0], -w[1], -w[2]], [w[0], 0.0, w[2], -w[1]], [w[1], -w[2], 0.0, w[0]], [w[2], w[1], -w[0], 0.0]]
        return [0.5 * v for v in _mv(O, q)]

    def _ad(self, x, u):
        return self._kin(x[0:4], x[4:7]) + self._rates(x[4:7], u)

    def f(self, x, u, t):
        q = np.asarray(x[0:4], dtype=np.float64)
        n = float(np.linalg.norm(q))
        q = q / n if n > 1e-9 else np.array([1.0, 0.0, 0.0, 0.0])
        return np.array(self._kin(list(q), list(x[4:7])) + self._rates(list(x[4:7]), list(u)), dtype=np.float64)


class MrpAttitude(_Attitude):   # mrp_attitude.cpp:31-98 / .hpp:154+: 0.25 B(sigma) omega
    nx, nu = 6, 3

    def _ad(self, x, u):
        s = x[0:3]
        n2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2]
        S = [[0.0, -s[2], s[1]], [s[2], 0.0, -s[0]], [-s[1], s[0], 0.0]]
        B = [[(1.0 - n2) * (1.0 if i == j else 0.0) + 2.0 * S[i][j] + 2.0 * s[i] * s[j] for j in range(3)] for i in range(3)]
        return [0.25 * v for v in _mv(B, x[3:6])] + self._rates(x[3:6], u)


class SpacecraftTwobody:   # spacecraft_twobody.cpp:15-74
    nx, nu = 6, 3

    def __init__(self, mu, mass):
        self.mu, self.mass = float(mu), float(mass)

    def f(self, x, u, t):
        r = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        r3 = r * r * r
        return np.array([x[3], x[4], x[5]] + [-self.mu * x[i] / r3 + u[i] / self.mass for i in range(3)], dtype=np.float64)

    def jac(self, x, u, t):
        return fd_jacobian(lambda s: self.f(s, u, t), x), fd_jacobian(lambda c: self.f(x, c, t), u)

    def hess(self, x, u, t):
        raise RuntimeError("getContinuousDynamicsAutodiff must be overridden in the derived class to use Autodiff-based derivatives.")


class SpacecraftLanding2D(_Plant):   # spacecraft_landing2d.cpp:20-112, state [x, x_dot, y, y_dot, theta, theta_dot]
    nx, nu = 6, 2

    def __init__(self, mass=100000.0, length=50.0, width=10.0, min_thrust=880000.0, max_thrust=2210000.0, max_gimble=0.349066):
        self.mass, self.length, self.max_thrust = float(mass), float(length), float(max_thrust)
        self.inertia = (1.0 / 12.0) * self.mass * self.length * self.length
        self.g = 9.81

    def f(self, x, u, t):
        a = u[1] + x[4]
        thrust = self.max_thrust * u[0]
        T = -self.length / 2.0 * thrust * math.sin(u[1])
        return np.array([x[1], thrust * math.sin(a) / self.mass, x[3], thrust * math.cos(a) / self.mass - self.g, x[5], T / self.inertia])

    def _ad(self, x, u):   # :112+, the expression the base-class cross Hessian differentiates
        a = u[1] + x[4]
        T = -u[0] * (self.length / 2.0) * sin(u[1])
        return [x[1], u[0] * sin(a) / self.mass, x[3], u[0] * cos(a) / self.mass - self.g, x[5], T / self.inertia]

    def jac(self, x, u, t):
        return fd_jacobian(lambda s: self.f(s, u, t), x), fd_jacobian(lambda c: self.f(x, c, t), u)

    def hess(self, x, u, t):   # state / control Hessians: zero overrides (:100-110)
        _, _, Fux = _Plant.hess(self, x, u, t)
        return np.zeros((6, 6, 6)), np.zeros((6, 2, 2)), Fux
