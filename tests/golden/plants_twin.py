"""Numpy restatements of eight more plants of the reference (src/dynamics_model/{dubins_car,dreyfus_rocket,acrobot,usv_3dof,forklift,
quadrotor_rate,spacecraft_linear_fuel,spacecraft_nonlinear}.cpp), written from those sources alone: no import of the product (pyapi, pycddp_amd) or of the C++ oracle.
Each plant has the interface the numpy twin (oracle/twin/cddp_twin.py) takes: nx, nu, f(x, u, t) or step(x, u, t), jac, hess.  The
number types (hyper-dual numbers, complex step, central differences) are those of tests/golden/spacecraft_twin.py.

Derivatives, as the reference takes them:
  * DubinsCar, DreyfusRocket, Usv3Dof: hand-written Jacobians / some Hessian blocks there, autodiff for the rest.  Here every
    Jacobian is the complex-step derivative and every Hessian block the hyper-dual one of the plant's autodiff expression -- the
    hand-written blocks of the reference are derivatives of the same expression, so the two agree to rounding;
  * Acrobot, QuadrotorRate: autodiff throughout (the quadrotor's through the quaternion normalisation);
  * SpacecraftNonlinear: central differences of this module's own f; no autodiff expression, so its Hessians raise as the
    reference's cross Hessian does;
  * Forklift: a discrete plant; Jacobians = (d step - I) / timestep, Hessians = d2 step / timestep;
  * SpacecraftLinearFuel: central differences, h = 2e-5 (helper.hpp:96), of this module's own f; all Hessians are zero overrides.
"""
import math

import numpy as np

from spacecraft_twin import HyperDual, _Plant, _mp, _mv, cos, cs_jacobian, fd_jacobian, hd_hessian, is_mpf, mpow15, msqrt, sin, sqrt, tan, val, vec  # noqa: F401


class _AdPlant(_Plant):
    def f(self, x, u, t):
        return vec(self._ad(list(x), list(u)))


class DubinsCar(_AdPlant):   # dubins_car.cpp: state [x, y, theta], control [omega]
    nx, nu = 3, 1

    def __init__(self, speed):
        self.speed = float(speed)

    def _ad(self, x, u):
        return [self.speed * cos(x[2]), self.speed * sin(x[2]), u[0]]


class DreyfusRocket(_AdPlant):   # dreyfus_rocket.cpp: state [x, x_dot], control [theta]
    nx, nu = 2, 1

    def __init__(self, thrust_acceleration=64.0, gravity_acceleration=32.0):
        self.T, self.g = float(thrust_acceleration), float(gravity_acceleration)

    def _ad(self, x, u):
        return [x[1], self.T * cos(u[0]) - self.g]


class Acrobot(_AdPlant):   # acrobot.cpp:24-163: state [theta1, theta2, theta1_dot, theta2_dot], control [torque]
    nx, nu = 4, 1
    gravity, friction = 9.81, 1.0

    def __init__(self, l1=1.0, l2=1.0, m1=1.0, m2=1.0, J1=1.0, J2=1.0):
        self.l1, self.l2, self.m1, self.m2, self.J1, self.J2 = (float(v) for v in (l1, l2, m1, m2, J1, J2))

    def _ad(self, x, u):
        l1, l2, m1, m2, J1, J2 = self.l1, self.l2, self.m1, self.m2, self.J1, self.J2
        th1, th2, w1, w2 = x
        c1, s2, c2, c12 = cos(th1), sin(th2), cos(th2), cos(th1 + th2)
        m11 = m1 * l1 * l1 + J1 + m2 * (l1 * l1 + l2 * l2 + 2 * l1 * l2 * c2) + J2
        m12 = m2 * (l2 * l2 + l1 * l2 * c2) + J2
        m22 = l2 * l2 * m2 + J2
        tmp = l1 * l2 * m2 * s2
        b1 = -(2 * w1 * w2 + w2 * w2) * tmp
        b2 = tmp * w1 * w1
        g1 = ((m1 + m2) * l1 * c1 + m2 * l2 * c12) * self.gravity
        g2 = m2 * l2 * c12 * self.gravity
        r1 = 0.0 - b1 - g1 - self.friction * w1
        r2 = u[0] - b2 - g2 - self.friction * w2
        det = m11 * m22 - m12 * m12
        return [w1, w2, (m22 * r1 - m12 * r2) / det, (m11 * r2 - m12 * r1) / det]


class Usv3Dof(_AdPlant):   # usv_3dof.cpp: state [x, y, psi, u, v, r], control [tau_u, tau_v, tau_r]; the fixed vessel of :17-48
    nx, nu = 6, 3

    def __init__(self):
        m, Iz = 100.0, 10.0
        X_udot, Y_vdot, Y_rdot, N_vdot, N_rdot = -10.0, -50.0, -5.0, -5.0, -5.0
        X_u, Y_v, Y_r, N_v, N_r = -20.0, -100.0, 0.0, 0.0, -20.0
        M = np.diag([m, m, Iz]) + np.array([[-X_udot, 0.0, 0.0], [0.0, -Y_vdot, -Y_rdot], [0.0, -N_vdot, -N_rdot]])
        self.M = M
        self.Minv = np.linalg.inv(M).tolist()
        self.D = [[-X_u, 0.0, 0.0], [0.0, -Y_v, -Y_r], [0.0, -N_v, -N_r]]
        self.m_x, self.m_y, self.m_yr = m - X_udot, m - Y_vdot, -Y_rdot

    def _ad(self, x, tau):
        psi, u, v, r = x[2], x[3], x[4], x[5]
        c, s = cos(psi), sin(psi)
        nu = [u, v, r]
        C = [[0.0, 0.0, -self.m_y * v - self.m_yr * r], [0.0, 0.0, self.m_x * u], [self.m_y * v + self.m_yr * r, -self.m_x * u, 0.0]]
        Cnu, Dnu = _mv(C, nu), _mv(self.D, nu)
        Minv = (_mp.matrix(self.M.tolist()) ** -1).tolist() if is_mpf(list(x) + list(tau)) else self.Minv   # 60 digits: the exact inverse
        return [c * u - s * v, s * u + c * v, r] + _mv(Minv, [tau[i] - Cnu[i] - Dnu[i] for i in range(3)])

    def hess(self, x, u, t):   # the control Hessian is a zero override (:237-246)
        Fxx, _, Fux = _Plant.hess(self, x, u, t)
        return Fxx, np.zeros((6, 3, 3)), Fux


class Forklift(_Plant):   # forklift.cpp: DISCRETE; state [x, y, theta, v, delta], control [a, ddelta]
    nx, nu = 5, 2
    discrete = True

    def __init__(self, wheelbase=2.0, dt=0.01, rear_steer=True, max_steering_angle=0.785398):
        self.L, self.h, self.sign = float(wheelbase), float(dt), (-1.0 if rear_steer else 1.0)

    def _ad(self, x, u):   # the discrete map (:17-48 == :127-158)
        h, L = self.h, self.L
        v = x[3]
        return [x[0] + h * v * cos(x[2]), x[1] + h * v * sin(x[2]), x[2] + h * v * tan(self.sign * x[4]) / L, x[3] + h * u[0], x[4] + h * u[1]]

    def step(self, x, u, t):
        return vec(self._ad(list(x), list(u)))

    def jac(self, x, u, t):   # :50-87
        A, B = _Plant.jac(self, x, u, t)
        return (A - np.eye(5)) / self.h, B / self.h

    def hess(self, x, u, t):   # :89-125
        Fxx, Fuu, Fux = _Plant.hess(self, x, u, t)
        return Fxx / self.h, Fuu / self.h, Fux / self.h


class SpacecraftLinearFuel:   # spacecraft_linear_fuel.cpp: state [x, y, z, vx, vy, vz, mass, effort], control [Fx, Fy, Fz]
    nx, nu = 8, 3

    def __init__(self, mean_motion, isp, g0=9.80665):
        self.n, self.isp, self.g0, self.eps = float(mean_motion), float(isp), float(g0), 1e-8

    def f(self, x, u, t):
        n = self.n; n2 = n * n; mass = x[6]
        t2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
        return vec([x[3], x[4], x[5], 2.0 * n * x[4] + 3.0 * n2 * x[0] + u[0] / mass, -2.0 * n * x[3] + u[1] / mass,
                    -n2 * x[2] + u[2] / mass, -msqrt(t2 + self.eps) / (self.isp * self.g0), 0.5 * t2])

    def jac(self, x, u, t):
        return fd_jacobian(lambda s: self.f(s, u, t), x), fd_jacobian(lambda c: self.f(x, c, t), u)

    def hess(self, x, u, t):   # :141-158
        return np.zeros((8, 8, 8)), np.zeros((8, 3, 3)), np.zeros((8, 3, 8))


class QuadrotorRate(_AdPlant):   # quadrotor_rate.cpp: state [p, v, qw, qx, qy, qz], control [thrust, wx, wy, wz]
    nx, nu = 10, 4

    def __init__(self, mass, max_thrust, max_rate):
        for v, msg in ((mass, "Mass must be positive"), (max_thrust, "Maximum thrust must be positive"), (max_rate, "Maximum angular rate must be positive")):
            if not v > 0.0:
                raise ValueError(msg)
        self.mass, self.g = float(mass), 9.81

    def _ad(self, x, u):
        q = x[6:10]
        n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        qw, qx, qy, qz = (v / n for v in q)
        T, w = u[0], u[1:4]
        R = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)],
             [2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)],
             [2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)]]
        a = _mv(R, [0.0, 0.0, T])
        O = [[0.0, -w[0], -w[1], -w[2]], [w[0], 0.0, w[2], -w[1]], [w[1], -w[2], 0.0, w[0]], [w[2], w[1], -w[0], 0.0]]
        return [x[3], x[4], x[5], a[0] / self.mass, a[1] / self.mass, a[2] / self.mass - self.g] + [0.5 * v for v in _mv(O, [qw, qx, qy, qz])]


class SpacecraftNonlinear:   # spacecraft_nonlinear.cpp: state [p, v, r0, theta, dr0, dtheta], control [ux, uy, uz]
    nx, nu = 10, 3

    def __init__(self, mass=1.0, r_scale=1.0, v_scale=1.0, mu=1.0):
        self.mass, self.mu = float(mass), float(mu)

    def f(self, x, u, t):
        px, py, pz, vx, vy, vz, r0, _, dr0, dth = x if is_mpf(x) else (float(v) for v in x)
        mu = self.mu
        den = mpow15((r0 + px) ** 2 + py * py + pz * pz)
        ddr0 = -mu / (r0 * r0) + r0 * dth * dth
        ddth = -2.0 * dr0 * dth / r0
        return vec([vx, vy, vz,
                    2.0 * dth * vy + ddth * py + dth * dth * px - mu * (px + r0) / den + mu / (r0 * r0) + u[0] / self.mass,
                    -2.0 * dth * vx - ddth * px + dth * dth * py - mu * py / den + u[1] / self.mass,
                    -mu * pz / den + u[2] / self.mass, dr0, dth, ddr0, ddth])

    def jac(self, x, u, t):
        return fd_jacobian(lambda s: self.f(s, u, t), x), fd_jacobian(lambda c: self.f(x, c, t), u)

    def hess(self, x, u, t):
        raise RuntimeError("getContinuousDynamicsAutodiff must be overridden in the derived class to use Autodiff-based derivatives.")
