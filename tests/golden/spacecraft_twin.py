"""Numpy restatements of the five spacecraft plants of the reference (src/dynamics_model/{euler,quaternion,mrp}_attitude.cpp,
spacecraft_twobody.cpp, spacecraft_landing2d.cpp), written from those sources alone: no import of the product (pyapi, pycddp_amd)
or of the C++ oracle.  Each plant has the interface the numpy twin (oracle/twin/cddp_twin.py) takes: nx, nu, f(x, u, t), jac, hess.

Derivatives, as the reference takes them:
  * autodiff plants (the three attitude forms): Jacobians by complex-step differentiation of the autodiff expression (no
    subtraction, no truncation error: autodiff's value to rounding), Hessians by hyper-dual numbers (exact second derivatives);
  * finite-difference plants (two-body, 2-D lander): central differences, h = 2e-5 (helper.hpp:96), of this module's own f;
    the lander's cross Hessian is the base-class autodiff default on ITS autodiff expression (thrust = u0, no max_thrust factor).
On mpmath numbers f, jac and hess give the same quantities at the working precision: the autodiff expression on Jets (second-order
Taylor numbers of mpmath components), the central differences at h = 1e-20, i.e. the derivative they approximate.
"""
import math

import numpy as np

try:   # the arbitrary-precision branch of the dispatch below (tests/plant_probe.py: the plants' values at 60 digits)
    import mpmath as _mp
    _MPF = _mp.mpf
except ImportError:   # the twin itself needs numpy only
    _mp, _MPF = None, ()


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


class Jet:
    """Value, gradient and Hessian of an expression carried forward together (second-order Taylor arithmetic), sparse: g and h hold
    only the variables an intermediate depends on, h the pairs (i, j) with i <= j.  The components are of any scalar type: on mpmath
    numbers one evaluation gives every first and second derivative at the working precision (the hyper-dual rules, all pairs at once)."""
    __slots__ = ("a", "g", "h")
    __array_ufunc__ = None

    def __init__(self, a, g=None, h=None):
        self.a, self.g, self.h = a, g or {}, h or {}

    @staticmethod
    def _sum(p, q):
        r = dict(p)
        for k, v in q.items():
            r[k] = r[k] + v if k in r else v
        return r

    def __add__(self, o):
        if not isinstance(o, Jet):
            return Jet(self.a + o, self.g, self.h)
        return Jet(self.a + o.a, Jet._sum(self.g, o.g), Jet._sum(self.h, o.h))
    __radd__ = __add__

    def __neg__(self):
        return Jet(-self.a, {k: -v for k, v in self.g.items()}, {k: -v for k, v in self.h.items()})

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Jet):
            return Jet(self.a * o, {k: v * o for k, v in self.g.items()}, {k: v * o for k, v in self.h.items()})
        g = Jet._sum({k: v * o.a for k, v in self.g.items()}, {k: self.a * v for k, v in o.g.items()})
        h = Jet._sum({k: v * o.a for k, v in self.h.items()}, {k: self.a * v for k, v in o.h.items()})
        for i, p in self.g.items():
            for j, q in o.g.items():
                k = (i, j) if i <= j else (j, i)
                t = 2.0 * (p * q) if i == j else p * q
                h[k] = h[k] + t if k in h else t
        return Jet(self.a * o.a, g, h)
    __rmul__ = __mul__

    def unary(self, f0, f1, f2):
        h = {k: f1 * v for k, v in self.h.items()}
        for i, p in self.g.items():
            for j, q in self.g.items():
                if i <= j:
                    t = f2 * (p * q)
                    h[(i, j)] = h[(i, j)] + t if (i, j) in h else t
        return Jet(f0, {k: f1 * v for k, v in self.g.items()}, h)

    def __truediv__(self, o):
        if not isinstance(o, Jet):
            return self * (1.0 / o)
        return self * o.unary(1.0 / o.a, -1.0 / (o.a * o.a), 2.0 / (o.a * o.a * o.a))

    def __rtruediv__(self, o):
        return self.unary(1.0 / self.a, -1.0 / (self.a * self.a), 2.0 / (self.a * self.a * self.a)) * o


def val(v):
    if isinstance(v, (HyperDual, Jet)):
        return v.a
    if isinstance(v, _MPF):
        return v
    return v.real if isinstance(v, complex) or np.iscomplexobj(v) else v


def sin(v):
    if isinstance(v, _MPF):
        return _mp.sin(v)
    if isinstance(v, Jet):
        s, c = msin(v.a), mcos(v.a); return v.unary(s, c, -s)
    if isinstance(v, HyperDual):
        return v.unary(math.sin(v.a), math.cos(v.a), -math.sin(v.a))
    return np.sin(v)


def cos(v):
    if isinstance(v, _MPF):
        return _mp.cos(v)
    if isinstance(v, Jet):
        s, c = msin(v.a), mcos(v.a); return v.unary(c, -s, -c)
    if isinstance(v, HyperDual):
        return v.unary(math.cos(v.a), -math.sin(v.a), -math.cos(v.a))
    return np.cos(v)


def tan(v):
    if isinstance(v, _MPF):
        return _mp.tan(v)
    if isinstance(v, Jet):
        t = mtan(v.a); return v.unary(t, 1.0 + t * t, 2.0 * t * (1.0 + t * t))
    if isinstance(v, HyperDual):
        t = math.tan(v.a); return v.unary(t, 1.0 + t * t, 2.0 * t * (1.0 + t * t))
    return np.tan(v)


def sqrt(v):
    if isinstance(v, _MPF):
        return _mp.sqrt(v)
    if isinstance(v, Jet):
        r = msqrt(v.a); return v.unary(r, 0.5 / r, -0.25 / (v.a * r))
    if isinstance(v, HyperDual):
        r = math.sqrt(v.a); return v.unary(r, 0.5 / r, -0.25 / (v.a * r))
    return np.sqrt(v)


def is_mpf(seq):
    return any(isinstance(val(v), _MPF) for v in seq)


def vec(vals):
    """The plants' return value: a float64 vector, or -- on mpmath numbers -- the list as it stands."""
    vals = [val(v) for v in vals]
    return vals if is_mpf(vals) else np.array(vals, dtype=np.float64)


# Two families on purpose: sin / cos / tan / sqrt above are what the autodiff expressions (_ad) are written in -- numpy's functions on
# float64 and complex128 (the complex step needs them), the derivative rules on HyperDual and Jet.  msin / mcos / mtan / msqrt / mpow15
# are what the plain value expressions (f of the finite-difference plants, originally math.sin ...) and the derivative rules themselves
# are written in: the C library's functions on a float, so that those values stay what they were, mpmath's on an mpf.
def msin(v):
    return _mp.sin(v) if isinstance(v, _MPF) else math.sin(v)


def mcos(v):
    return _mp.cos(v) if isinstance(v, _MPF) else math.cos(v)


def mtan(v):
    return _mp.tan(v) if isinstance(v, _MPF) else math.tan(v)


def msqrt(v):
    return _mp.sqrt(v) if isinstance(v, _MPF) else math.sqrt(v)


def mpow15(v):
    return v * _mp.sqrt(v) if isinstance(v, _MPF) else math.pow(v, 1.5)


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


def jet_derivs(f, z):
    """J[i, a] and H[i, a, b] of every output of f w.r.t. z from one evaluation on Jets, in the type of z's entries (object arrays of
    mpmath numbers, exact zeros as 0)."""
    n = len(z)
    r = [v if isinstance(v, Jet) else Jet(v) for v in f([Jet(v, {j: 1.0}) for j, v in enumerate(z)])]
    dt = object if is_mpf(z) else np.float64
    J, H = np.zeros((len(r), n), dtype=dt), np.zeros((len(r), n, n), dtype=dt)
    for i, v in enumerate(r):
        for a, d in v.g.items():
            J[i, a] = d
        for (a, b), d in v.h.items():
            H[i, a, b] = H[i, b, a] = d
    return J, H


def fd_jacobian(f, z, h=2e-5):
    """helper.hpp:96 finite_difference_jacobian, central differences.  On mpmath numbers: the derivative those differences approximate
    (h = 1e-20 at 60 digits: truncation and rounding both below 1e-38 of the function's scale)."""
    if is_mpf(z):
        z = list(z); h = _MPF(10) ** -20; cols = []
        for i in range(len(z)):
            fp = f(z[:i] + [z[i] + h] + z[i + 1:]); fm = f(z[:i] + [z[i] - h] + z[i + 1:])
            cols.append([(p - m) / (2 * h) for p, m in zip(fp, fm)])
        return np.array(cols, dtype=object).T
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
        z = list(x) + list(u)
        J = jet_derivs(self._adz, z)[0] if is_mpf(z) else cs_jacobian(self._adz, np.concatenate([x, u]))
        return J[:, :self.nx], J[:, self.nx:]

    def hess(self, x, u, t):
        z = list(x) + list(u)
        H = jet_derivs(self._adz, z)[1] if is_mpf(z) else hd_hessian(self._adz, np.concatenate([x, u]))
        n = self.nx
        return H[:, :n, :n].copy(), H[:, n:, n:].copy(), H[:, n:, :n].copy()


class _Attitude(_Plant):
    def __init__(self, inertia):
        self.I = np.asarray(inertia, dtype=np.float64).reshape(3, 3)
        self.Iinv = np.linalg.inv(self.I)

    def _rates(self, w, tau):   # I^-1 (-skew(w) (I w) + tau)
        if is_mpf(list(w) + list(tau)):   # 60 digits: the inverse of the float64 inertia itself, not its float64 rounding
            I = _mp.matrix(self.I.tolist()); h = _mv(I.tolist(), w)
            v = [w[2] * h[1] - w[1] * h[2] + tau[0], w[0] * h[2] - w[2] * h[0] + tau[1], w[1] * h[0] - w[0] * h[1] + tau[2]]
            return _mv((I ** -1).tolist(), v)
        h = _mv(self.I.tolist(), w)
        v = [w[2] * h[1] - w[1] * h[2] + tau[0], w[0] * h[2] - w[2] * h[0] + tau[1], w[1] * h[0] - w[0] * h[1] + tau[2]]
        return _mv(self.Iinv.tolist(), v)

    def f(self, x, u, t):
        return vec(self._ad(list(x), list(u)))


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
        if is_mpf(x):
            n = _mp.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3])
            q = [v / n for v in x[0:4]] if n > 1e-9 else [_MPF(1), _MPF(0), _MPF(0), _MPF(0)]
            return self._kin(q, list(x[4:7])) + self._rates(list(x[4:7]), list(u))
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
        r = msqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        r3 = r * r * r
        return vec([x[3], x[4], x[5]] + [-self.mu * x[i] / r3 + u[i] / self.mass for i in range(3)])

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
        T = -self.length / 2.0 * thrust * msin(u[1])
        return vec([x[1], thrust * msin(a) / self.mass, x[3], thrust * mcos(a) / self.mass - self.g, x[5], T / self.inertia])

    def _ad(self, x, u):   # :112+, the expression the base-class cross Hessian differentiates
        a = u[1] + x[4]
        T = -u[0] * (self.length / 2.0) * sin(u[1])
        return [x[1], u[0] * sin(a) / self.mass, x[3], u[0] * cos(a) / self.mass - self.g, x[5], T / self.inertia]

    def jac(self, x, u, t):
        return fd_jacobian(lambda s: self.f(s, u, t), x), fd_jacobian(lambda c: self.f(x, c, t), u)

    def hess(self, x, u, t):   # state / control Hessians: zero overrides (:100-110)
        _, _, Fux = _Plant.hess(self, x, u, t)
        return np.zeros((6, 6, 6)), np.zeros((6, 2, 2)), Fux
