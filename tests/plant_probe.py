"""Helper of tests/test_plant_probe.py and tests/test_constraint_probe.py: loads the plant / constraint probe (tests/hip/plant_probe.hip,
linked by cddp-cpp_amd/csrc/Makefile into cddp-cpp_amd/lib/libcddp_hip_probe.so) and the host build of the plant cases
(tests/hip/plant_probe_host.cpp, compiled here with g++ -O2 -std=c++17 -ffp-contract=off -DCDDP_TRIG_SHARED=1: the plants of
dev_models.hpp in the kernels' own sin / cos), and owns the plant table, the fixed-seed point sets and the references.

References are independent of the code under test: the C++ oracle in its shared-trig mode for model ids 0-10, the numpy twins of
tests/golden/{spacecraft,plants}_twin.py -- evaluated in mpmath at 60 digits on the float64 inputs for values -- for ids 11-23, the
constraint classes of oracle/twin/cddp_twin.py.  Not a conftest: the test modules import it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import mpmath as mp

import dev_probe as D

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(REPO, "oracle", "twin"))
import cddp_twin as T  # noqa: E402
import spacecraft_twin as ST  # noqa: E402
import plants_twin as PT  # noqa: E402

mp.mp.dps = 60
NAN, INF = float("nan"), float("inf")
INTEGRATORS = ("euler", "heun", "rk3", "rk4")           # CDDP_HIP_EULER .. CDDP_HIP_RK4 = 0 .. 3
TRIG_LIMIT = 1.0e9                                       # dev_trig.hpp::kTrigFastLimit
B_SET = 3 * 64 + 37                                      # three wavefronts and a partial one

MEAN_MOTION = float(np.sqrt(3.986004418e14 / (6371e3 + 500e3) ** 3))
INERTIA = np.array([[1.0, 0.1, 0.0], [0.1, 1.5, 0.05], [0.0, 0.05, 2.0]])
LANDING = [100000.0, 50.0, 10.0, 880000.0, 2210000.0, 0.349066]
ACROBOT = [1.1, 0.9, 1.2, 0.8, 1.0, 0.7]
FORKLIFT = [2.0, 1.0, 0.785398]
QUADROTOR_RATE = [1.0, 20.0, 0.5]
QUAD = [1.0, 0.2, 0.01, 0.01, 0.02, 9.81]
LTI_A = np.array([[1.0, 0.1], [-0.2, 0.95]])
LTI_B = np.array([[0.005], [0.1]])


class Plant:
    def __init__(self, tag, mid, nx, nu, params, dt, ax=(), au=(), ref="oracle", discrete=False, hess="both", jacblk=False, quat=None,
                 builder=None, twin=None):
        self.tag, self.id, self.nx, self.nu, self.params, self.dt = tag, mid, nx, nu, list(params), dt
        self.ax, self.au = tuple(ax), tuple(au)      # the state / control slots the plant takes a sine, cosine or tangent of
        self.ref, self.discrete, self.hess, self.jacblk, self.quat = ref, discrete, hess, jacblk, quat
        self.builder, self.twin = builder, twin       # pyapi problem builder (oracle plants) / twin constructor


# The parameters are those of the project's problem builders (ids 0-10: tests/test_plant_probe.py asserts the equality) and of the
# twins' tables in tests/test_spacecraft_plants.py / tests/test_remaining_plants.py (ids 11-23).  hess: "both" = hess() in both
# builds, "blocked" = host hess() + the device's blocked contraction, None = the plant has no second-order terms in either build.
PLANTS = [
    Plant("pendulum", 0, 2, 1, [0.5, 1.0, 0.01, 9.81], 0.02, ax=(0,), builder=("pendulum_problem", ())),
    Plant("cartpole", 1, 4, 1, [1.0, 0.2, 0.5, 9.81, 0.0], 0.05, ax=(1,), builder=("cartpole_problem", ())),
    Plant("unicycle", 2, 3, 2, [], 0.03, ax=(2,), builder=("unicycle_problem", ())),
    Plant("lti21", 3, 2, 1, [], 0.1, discrete=True, builder=None),
    Plant("quadrotor", 4, 13, 4, QUAD, 0.02, hess="blocked", quat=3, builder=("quadrotor_problem", ())),
    Plant("manipulator", 5, 6, 3, [], 0.01, ax=(0, 1, 2), builder=("manipulator_problem", ())),
    Plant("quad12", 6, 12, 4, QUAD, 0.01, ax=(6, 7, 8), hess="blocked", builder=("quadrotor12_problem", ())),
    Plant("manip7", 7, 14, 7, [], 0.01, ax=tuple(range(7)), hess="blocked", builder=("manipulator7_problem", ())),
    Plant("bicycle", 8, 4, 2, [2.0], 0.05, ax=(2,), au=(1,), builder=("bicycle_problem", ())),
    Plant("car", 9, 4, 2, [2.0], 0.03, ax=(2,), au=(0,), discrete=True, builder=("car_problem", ())),
    Plant("hcw", 10, 6, 3, [MEAN_MOTION, 1.0], 10.0, builder=("hcw_problem", ())),
    Plant("euler", 11, 6, 3, INERTIA.ravel(), 0.1, ax=(1, 2), ref="twin", hess="blocked", jacblk=True, twin=lambda dt: ST.EulerAttitude(INERTIA)),
    Plant("quaternion", 12, 7, 3, INERTIA.ravel(), 0.1, ref="twin", hess="blocked", jacblk=True, quat=0, twin=lambda dt: ST.QuaternionAttitude(INERTIA)),
    Plant("mrp", 13, 6, 3, INERTIA.ravel(), 0.1, ref="twin", hess="blocked", jacblk=True, twin=lambda dt: ST.MrpAttitude(INERTIA)),
    Plant("twobody", 14, 6, 3, [1.0, 1.0], 0.05, ref="twin", hess=None, twin=lambda dt: ST.SpacecraftTwobody(1.0, 1.0)),
    Plant("landing2d", 15, 6, 2, LANDING, 0.1, ax=(4,), au=(1,), ref="twin", twin=lambda dt: ST.SpacecraftLanding2D(*LANDING)),
    Plant("dubins", 16, 3, 1, [1.3], 0.1, ax=(2,), ref="twin", twin=lambda dt: PT.DubinsCar(1.3)),
    Plant("dreyfus", 17, 2, 1, [64.0, 32.0], 0.01, au=(0,), ref="twin", twin=lambda dt: PT.DreyfusRocket(64.0, 32.0)),
    Plant("acrobot", 18, 4, 1, ACROBOT, 0.02, ax=(0, 1), ref="twin", twin=lambda dt: PT.Acrobot(*ACROBOT)),
    Plant("usv", 19, 6, 3, [], 0.1, ax=(2,), ref="twin", hess="blocked", twin=lambda dt: PT.Usv3Dof()),
    Plant("forklift", 20, 5, 2, FORKLIFT, 0.03, ax=(2, 4), ref="twin", discrete=True, jacblk=True, twin=lambda dt: PT.Forklift(2.0, dt, True, 0.785398)),
    Plant("quadrotorrate", 21, 10, 4, QUADROTOR_RATE, 0.05, ref="twin", hess="blocked", jacblk=True, quat=6, twin=lambda dt: PT.QuadrotorRate(*QUADROTOR_RATE)),
    Plant("linearfuel", 22, 8, 3, [MEAN_MOTION, 300.0, 9.80665], 10.0, ref="twin", twin=lambda dt: PT.SpacecraftLinearFuel(MEAN_MOTION, 300.0, 9.80665)),
    Plant("nonlinear", 23, 10, 3, [1.3, 1.0, 1.0, 0.9], 0.05, ref="twin", hess=None, twin=lambda dt: PT.SpacecraftNonlinear(1.3, 1.0, 1.0, 0.9)),
]
BY_TAG = {p.tag: p for p in PLANTS}
TAGS = [p.tag for p in PLANTS]
BLOCKED = [p.tag for p in PLANTS if p.hess == "blocked"]
HESS_BOTH = [p.tag for p in PLANTS if p.hess == "both"]
NO_HESS = [p.tag for p in PLANTS if p.hess is None]
JAC_BLOCKED = [p.tag for p in PLANTS if p.jacblk]
TRIG_POLICY = ("cartpole", "unicycle")                    # the plants whose f takes a Trig policy (dev_models.hpp: kTrigPolicy)

_host = None


def host(tmp_path):
    """The plant cases compiled for the host in the kernels' arithmetic (once per process)."""
    global _host
    if _host is None:
        so = str(tmp_path / "libcddp_plant_probe_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DCDDP_TRIG_SHARED=1", "-Wno-unknown-pragmas",
                               "-o", so, os.path.join(HERE, "hip", "plant_probe_host.cpp")])
        _host = ctypes.CDLL(so)
    return _host


device = D.device
run = D.run
same_numbers = D.same_numbers


def has_entry(lib, name):
    return hasattr(lib, "probe_" + name)


# ------------------------------------------------------------------------------------------------------------------------------------
# the parameter block the kernels read (ProblemDev::mp), restated from the descriptions in include/cddp_hip.h
# ------------------------------------------------------------------------------------------------------------------------------------
def inverse3_cofactor(M):
    """Eigen's fixed-size 3 x 3 inverse: cofactors times 1 / det, in float64 operation by operation."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    Cf = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            Cf[i, j] = M[i1, j1] * M[i2, j2] - M[i1, j2] * M[i2, j1]
    det = (M[0, 0] * Cf[0, 0] + M[0, 1] * Cf[0, 1]) + M[0, 2] * Cf[0, 2]
    return Cf.T * (1.0 / det)


def p32(pl, dt=None):
    dt = pl.dt if dt is None else dt
    p = np.zeros(32)
    p[:len(pl.params)] = pl.params
    if pl.tag == "lti21":
        p[:4] = LTI_A.ravel(); p[4:6] = LTI_B.ravel(); p[6] = dt
    elif pl.tag == "car":
        p[1] = dt
    elif pl.tag == "forklift":
        p[3] = dt
    elif pl.tag in ("euler", "quaternion", "mrp"):
        p[9:18] = inverse3_cofactor(pl.params).ravel()
    elif pl.tag == "usv":
        m, Iz, X_udot, Y_vdot, Y_rdot, N_vdot, N_rdot = 100.0, 10.0, -10.0, -50.0, -5.0, -5.0, -5.0
        X_u, Y_v, Y_r, N_v, N_r = -20.0, -100.0, 0.0, 0.0, -20.0
        M = [m - X_udot, 0.0, 0.0, 0.0, m - Y_vdot, 0.0 - Y_rdot, 0.0, 0.0 - N_vdot, Iz - N_rdot]
        p[:] = 0.0
        p[0:9] = inverse3_cofactor(M).ravel()
        p[9:18] = [-X_u, 0.0, 0.0, 0.0, -Y_v, -Y_r, 0.0, -N_v, -N_r]
        p[18:21] = [m - X_udot, m - Y_vdot, -Y_rdot]
    return p


# ------------------------------------------------------------------------------------------------------------------------------------
# point sets: (x (B, nx), u (B, nu)), fixed seeds
# ------------------------------------------------------------------------------------------------------------------------------------
def _seed(pl, salt):
    return 20261018 + 1000 * pl.id + salt


def _regular_raw(pl, rng, B):
    """x ~ N(0, 0.7), u ~ N(0, 1), as tests/test_host_models.py draws them; then the plant's own domain: a unit-dominant quaternion,
    and -- where a value is singular or meaningless at the origin of a coordinate (two-body radius, fuel mass, orbit radius, the
    Euler-angle pitch) -- that coordinate moved into the plant's working range."""
    x = rng.normal(0.0, 0.7, (B, pl.nx)); u = rng.normal(0.0, 1.0, (B, pl.nu))
    if pl.quat is not None:
        q = pl.quat
        x[:, q + 1:q + 4] *= 0.1; x[:, q] = 1.0
    if pl.tag == "euler":
        x[:, 1] *= 0.5                                   # pitch within +-1.05 at 3 sigma: away from the kinematic singularity
    if pl.tag == "twobody":
        x[:, :3] += np.where(x[:, :3] >= 0, 0.8, -0.8)   # |r| >= 1.38
    if pl.tag == "linearfuel":
        x[:, 6] = 1.0 + np.abs(x[:, 6])                  # a positive mass
    if pl.tag == "nonlinear":
        x[:, :6] *= 0.15; x[:, 6] = 1.0 + 0.1 * x[:, 6]; x[:, 9] = 1.0 + 0.1 * x[:, 9]   # a near-circular orbit, the chaser close to the target
    if pl.tag == "forklift":
        x[:, 4] *= 0.5                                   # steering angle: tan stays regular
    return x, u


def regular_set(pl, B=B_SET):
    return _regular_raw(pl, np.random.default_rng(_seed(pl, 1)), B)


def near_half_pi(rng, n):
    """Angles within a few ulp of multiples of pi / 2."""
    k = rng.integers(-4, 5, n).astype(np.float64)
    a = k * (np.pi / 2)
    for _ in range(3):
        step = rng.integers(-1, 2, n)
        a = np.where(step > 0, np.nextafter(a, INF), np.where(step < 0, np.nextafter(a, -INF), a))
    return a


def edge_set(pl, B=B_SET):
    """Families interleaved with period 8 (neighbouring lanes differ): zero | angles at multiples of pi / 2 | the plant's degenerate
    point (zero quaternion, r = 0) | magnitudes of 1e6 | regular | regular | angles at multiples of pi / 2, regular rest | regular.
    On top, per wavefront: lanes 5 and 37 hold |angle| >= 1e9 (the mixed wavefront: every other lane of it is in range unless its
    own family says otherwise), lane 17 a NaN and lane 41 an infinity, lane 23 exactly 1e9 and lane 24 the double below it.
    A plant without a trigonometric argument takes these values in its first state slot.  Returns x, u, fam (B,)."""
    rng = np.random.default_rng(_seed(pl, 2))
    x, u = _regular_raw(pl, rng, B)
    fam = np.empty(B, dtype=object)
    ax = pl.ax if (pl.ax or pl.au) else (0,)
    for i in range(B):
        k = i % 8
        f = ("zero", "halfpi", "degenerate", "big", "regular", "regular", "halfpi", "regular")[k]
        if f == "zero":
            x[i] = 0.0; u[i] = 0.0
        elif f == "halfpi":
            if k == 1:
                x[i] *= 0.0
            x[i, list(pl.ax)] = near_half_pi(rng, len(pl.ax)); u[i, list(pl.au)] = near_half_pi(rng, len(pl.au))
        elif f == "degenerate":
            if pl.quat is not None:
                x[i, pl.quat:pl.quat + 4] = 0.0
            elif pl.tag in ("twobody", "nonlinear"):
                x[i, :3] = 0.0
                if pl.tag == "nonlinear":
                    x[i, 6] = 0.0                       # r0 = 0 as well: (r0 + px)^2 + py^2 + pz^2 = 0
            elif pl.tag == "linearfuel":
                x[i, 6] = 0.0; u[i] = 0.0               # zero mass, zero thrust
            else:
                f = "regular"
        elif f == "big":
            x[i] *= 1e6; u[i] *= 1e6
        w = i % 64
        if w in (5, 37):
            f = "bigangle"
            big = (10.0 ** rng.uniform(9.0, 12.0)) * (1.0 if w == 5 else -1.0)
            x[i, list(ax)] = big; u[i, list(pl.au)] = -big
        elif w == 17:
            f = "nan"; x[i, ax[0] if ax else 0] = NAN
            if not pl.ax and pl.au:
                u[i, pl.au[0]] = NAN
        elif w == 41:
            f = "inf"; x[i, ax[0] if ax else 0] = INF
            if not pl.ax and pl.au:
                u[i, pl.au[0]] = -INF
        elif w == 23:
            f = "at_limit"; x[i, list(ax)] = TRIG_LIMIT; u[i, list(pl.au)] = -TRIG_LIMIT
        elif w == 24:
            f = "below_limit"; x[i, list(ax)] = np.nextafter(TRIG_LIMIT, 0.0); u[i, list(pl.au)] = -np.nextafter(TRIG_LIMIT, 0.0)
        fam[i] = f
    return x, u, fam


def pack(pl, x, u, dt=None, integ=None):
    """Records of CaseF / CaseJac / CaseHess / CaseJacBlocked (p, x, u) or, with integ, of CaseStep (integrator, dt, p, x, u)."""
    B = x.shape[0]
    dt = pl.dt if dt is None else dt
    P = np.repeat(p32(pl, dt)[:, None], B, axis=1)
    rows = [P, x.T, u.T]
    if integ is not None:
        rows = [np.full((1, B), float(integ)), np.full((1, B), dt)] + rows
    return np.ascontiguousarray(np.vstack(rows))


def pack_tensor(pl, x, u, w, Q, dt=None):
    """Records of CaseTensor: p, dt, x, u, w, Q_xx | Q_ux | Q_uu."""
    B = x.shape[0]
    dt = pl.dt if dt is None else dt
    return np.ascontiguousarray(np.vstack([np.repeat(p32(pl, dt)[:, None], B, axis=1), np.full((1, B), dt), x.T, u.T, w.T, Q.T]))


def tensor_inputs(pl, B, salt=3):
    rng = np.random.default_rng(_seed(pl, salt))
    nq = pl.nx * pl.nx + pl.nu * pl.nx + pl.nu * pl.nu
    return rng.normal(0.0, 1.0, (B, pl.nx)), rng.normal(0.0, 1.0, (B, nq))


def split_hess(pl, Y):
    """(NOUT, B) of CaseHess -> F_xx (B, nx, nx, nx), F_uu (B, nx, nu, nu), F_ux (B, nx, nu, nx)."""
    nx, nu = pl.nx, pl.nu
    B = Y.shape[1]
    a, b = nx * nx * nx, nx * nu * nu
    return (Y[:a].T.reshape(B, nx, nx, nx), Y[a:a + b].T.reshape(B, nx, nu, nu), Y[a + b:].T.reshape(B, nx, nu, nx))


def contract(pl, H, w, Q, dt=None):
    """The solver's contraction of the full tensors, in its order: for i ascending, Q[e] = Q[e] + w[i] * (dt * F[i][e])."""
    dt = pl.dt if dt is None else dt
    nx, nu = pl.nx, pl.nu
    Fxx, Fuu, Fux = H
    B = w.shape[0]
    Qxx = Q[:, :nx * nx].reshape(B, nx, nx).copy()
    Qux = Q[:, nx * nx:nx * nx + nu * nx].reshape(B, nu, nx).copy()
    Quu = Q[:, nx * nx + nu * nx:].reshape(B, nu, nu).copy()
    with np.errstate(all="ignore"):
        for i in range(nx):
            wi = w[:, i][:, None, None]
            Qxx = Qxx + wi * (dt * Fxx[:, i]); Qux = Qux + wi * (dt * Fux[:, i]); Quu = Quu + wi * (dt * Fuu[:, i])
    return np.concatenate([Qxx.reshape(B, -1), Qux.reshape(B, -1), Quu.reshape(B, -1)], axis=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the integrators from the probe's own f, in numpy (oracle/twin/cddp_twin.py::discrete_step holds the formulas): every stage state
# ------------------------------------------------------------------------------------------------------------------------------------
class ProbeF:
    """f(x, u, t) on whole batches through the f case of a probe library; records the state every stage was evaluated at."""
    def __init__(self, lib, pl, dt=None):
        self.lib, self.pl, self.dt, self.stages = lib, pl, dt, []
        self.discrete = pl.discrete

    def f(self, x, u, t):
        self.stages.append(x.copy())
        return run(self.lib, "f_" + self.pl.tag, pack(self.pl, x, u, self.dt)).T
    step = f


def numpy_step(lib, pl, integ, x, u, dt=None):
    """x_next (B, nx) and the list of stage states."""
    m = ProbeF(lib, pl, dt)
    with np.errstate(all="ignore"):
        xn = T.discrete_step(m, INTEGRATORS[integ], pl.dt if dt is None else dt, x, u, 0.0)
    return xn, m.stages


def out_of_range(a):
    return ~(np.abs(a) < TRIG_LIMIT)          # also true for NaN / inf, as the routines test it


def angle_flags(pl, stages, u):
    """Per lane: did any stage evaluate a sine / cosine / tangent at an angle outside the fast range (or a non-finite one)?"""
    flag = np.zeros(u.shape[0], dtype=bool)
    for s in stages:
        for j in pl.ax:
            flag |= out_of_range(s[:, j])
    for j in pl.au:
        flag |= out_of_range(u[:, j])
    return flag


def wild_lanes(pl, stages, u):
    """A superset of the lanes that can have taken the libm fallback, whatever the plant does with its arguments: any stage state
    or control entry that is non-finite or of magnitude >= 1e9 / n, n = the number of slots the plant takes angles from (a plant may
    take the sine of a SUM of its angles: the 3-DOF arm's q1 + q2, the 7-joint arm's cumulative angles, the lander's gimbal + pitch)."""
    lim = TRIG_LIMIT / max(1, len(pl.ax) + len(pl.au))
    flag = np.any(~(np.abs(u) < lim), axis=1)
    for s in stages:
        flag |= np.any(~(np.abs(s) < lim), axis=1)
    return flag


# ------------------------------------------------------------------------------------------------------------------------------------
# mpmath: the twins' f at 60 digits on the float64 inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def twin_f_mp(tw, x, u):
    xm = [mp.mpf(float(v)) for v in x]; um = [mp.mpf(float(v)) for v in u]
    r = tw.step(xm, um, 0.0) if getattr(tw, "discrete", False) else tw.f(xm, um, 0.0)
    return [mp.mpf(v) for v in r]


def twin_f(tw, x, u):
    return np.asarray(tw.step(x, u, 0.0) if getattr(tw, "discrete", False) else tw.f(x, u, 0.0), dtype=np.float64)


def err_vs_mp(got, ref):
    """max over the components of |got - ref| / max(1, |ref|), the measure of the existing plant tests (rel_err), against mpmath."""
    return max(float(abs(mp.mpf(float(g)) - r) / max(mp.mpf(1), abs(r))) for g, r in zip(got, ref))


def twin_derivs_mp(tw, x, u, hess):
    """The twin's own jac / hess on the float64 inputs as 60-digit numbers (Jets through its autodiff expression, or the limit of its
    central differences), each block split into a float64 pair (hi, lo) with hi + lo the value to 32 digits."""
    xm = [mp.mpf(float(v)) for v in x]; um = [mp.mpf(float(v)) for v in u]
    blocks = list(tw.jac(xm, um, 0.0)) + (list(tw.hess(xm, um, 0.0)) if hess else [])
    out = []
    for A in blocks:
        A = np.asarray(A, dtype=object)
        hi = A.astype(np.float64)
        out.append((hi, (A - hi).astype(np.float64)))
    return out


def err_vs_pair(got, ref):
    """max |got - (hi + lo)| / max(1, |hi|): got - hi is exact in float64 wherever the two are close."""
    hi, lo = ref
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs((got - hi) - lo) / np.maximum(1.0, np.abs(hi)))) if got.size else 0.0


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# constraints (device only)
# ------------------------------------------------------------------------------------------------------------------------------------
CON_NX, CON_NU = 4, 3
KIND = {"ctrlbox": 0, "statebox": 1, "ball": 2, "linear": 3, "soc": 4, "thrust2": 5, "thrust1": 6}


class Pool:
    """ConDev descriptors and the pool they point into, laid out as capi.hip's flatten() does: consecutive blocks."""
    def __init__(self):
        self.pool, self.cons, self.twins, self.off = [], [], [], 0

    def _put(self, v):
        at = len(self.pool)
        self.pool += [float(a) for a in np.asarray(v, dtype=np.float64).ravel()]
        return at

    def _con(self, kind, dim, dual, tw, lower=0, upper=0, center=0, A=0, b=0, scale=0.0, radius=0.0):
        self.cons.append([KIND[kind], dim, dual, self.off, lower, upper, center, A, b, scale, radius])
        self.twins.append(tw); self.off += dual

    def ctrlbox(self, lo, up, scale=1.0):
        self._con("ctrlbox", len(lo), 2 * len(lo), _Leading(T.ControlBox(lo, up, scale), len(lo), "u"), lower=self._put(lo), upper=self._put(up), scale=scale)

    def statebox(self, lo, up, scale=1.0):
        self._con("statebox", len(lo), 2 * len(lo), _Leading(T.StateBox(lo, up, scale), len(lo), "x"), lower=self._put(lo), upper=self._put(up), scale=scale)

    def ball(self, radius, center, scale=1.0):
        self._con("ball", len(center), 1, T.Ball(radius, center, scale), center=self._put(center), scale=scale, radius=radius)

    def linear(self, A, b):
        self._con("linear", len(b), len(b), T.Linear(A, b), A=self._put(A), b=self._put(b))

    def soc(self, origin, direction, fov, eps):
        tw = T.SecondOrderCone(origin, direction, fov, 1e-6)
        tw.eps = eps                                     # (the constructor refuses eps = 0; the evaluation is what is compared)
        self._con("soc", 3, 1, tw, center=self._put(origin), lower=self._put(tw.ax), scale=eps, radius=tw.cosf)

    def thrust(self, mn, mx, eps, D=CON_NU):
        if mn is None:
            self._con("thrust1", D, 1, T.ThrustMagnitude(None, mx, eps), scale=eps, radius=mx)
        else:
            self._con("thrust2", D, 2, T.ThrustMagnitude(mn, mx, eps), lower=self._put([mn]), scale=eps, radius=mx)

    @property
    def m(self):
        return self.off


class _Leading:
    """The twin's boxes span the whole state / control; the device's StateBox<D> / CtrlBox<D> the leading D entries."""
    def __init__(self, tw, d, which):
        self.tw, self.d, self.dim, self.which = tw, d, tw.dim, which

    def g(self, x, u):
        return self.tw.g(x[:self.d], u[:self.d])

    def jac(self, x, u):
        Gx = np.zeros((self.dim, x.size)); Gu = np.zeros((self.dim, u.size))
        jx, ju = self.tw.jac(x[:self.d], u[:self.d])
        if self.which == "x":
            Gx[:, :self.d] = jx
        else:
            Gu[:, :self.d] = ju
        return Gx, Gu


def run_con(lib, name, pool, x, u):
    """-> (form A, form B), each a dict g (B, m), Gx (B, m, nx), Gu (B, m, nu)."""
    dims = [ctypes.c_int() for _ in range(5)]
    getattr(lib, "probe_con_%s_dims" % name)(*[ctypes.byref(d) for d in dims])
    nin, nout, m, nx, nu = (d.value for d in dims)
    assert (nx, nu) == (CON_NX, CON_NU) and m == pool.m and nin == nx + nu, (name, nin, nout, m, nx, nu, pool.m)
    B = x.shape[0]
    X = np.ascontiguousarray(np.vstack([x.T, u.T]), dtype=np.float64)
    out = np.full((nout, B), NAN)
    cons = np.ascontiguousarray(np.array(pool.cons, dtype=np.float64))
    pl = np.ascontiguousarray(np.array(pool.pool + [0.0], dtype=np.float64))
    fn = getattr(lib, "probe_con_" + name)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    fn.restype = ctypes.c_int
    rc = fn(X.ctypes.data, out.ctypes.data, B, cons.ctypes.data, len(pool.cons), pl.ctypes.data, len(pool.pool))
    assert rc == 0, "probe_con_%s: hipError_t %d" % (name, rc)
    nrec = m + m * nx + m * nu
    forms = []
    for k in range(2):
        Y = out[k * nrec:(k + 1) * nrec]
        forms.append(dict(g=Y[:m].T.copy(), Gx=Y[m:m + m * nx].T.reshape(B, m, nx).copy(), Gu=Y[m + m * nx:].T.reshape(B, m, nu).copy()))
    return forms


def twin_con(pool, x, u):
    """The twin's stacked g, Gx, Gu (constraint objects in list order, rows at the stacked offsets)."""
    with np.errstate(all="ignore"):
        g = np.concatenate([tw.g(x, u) for tw in pool.twins])
        J = [tw.jac(x, u) for tw in pool.twins]
    return g, np.vstack([j[0] for j in J]), np.vstack([j[1] for j in J])


def mpf_con(pool, x, u):
    """g, G_x, G_u of every constraint at 60 digits (rows stacked in list order), from the formulas of constraint.hpp as the twin's
    classes state them, guards included (decided at 60 digits)."""
    xm = [mp.mpf(float(v)) for v in x]; um = [mp.mpf(float(v)) for v in u]
    nx, nu = len(xm), len(um)
    g, Gx, Gu = [], [], []
    zx = lambda: [mp.mpf(0)] * nx
    zu = lambda: [mp.mpf(0)] * nu

    def unit(n, i, v):
        r = [mp.mpf(0)] * n; r[i] = v
        return r
    for c, tw in zip(pool.cons, pool.twins):
        kind = c[0]
        if kind in (0, 1):
            b = tw.tw if isinstance(tw, _Leading) else tw
            v = um if kind == 0 else xm
            s = mp.mpf(b.scale)
            g += [(-v[i]) * s - (-mp.mpf(b.lo[i])) * s for i in range(b.n)] + [v[i] * s - mp.mpf(b.up[i]) * s for i in range(b.n)]
            for sg in (-s, s):
                for i in range(b.n):
                    Gx.append(unit(nx, i, sg) if kind == 1 else zx()); Gu.append(unit(nu, i, sg) if kind == 0 else zu())
        elif kind == 2:
            d = [xm[i] - mp.mpf(tw.c[i]) for i in range(tw.c.size)]
            g.append(-(mp.mpf(tw.scale) * mp.fsum([a * a for a in d])) + mp.mpf(tw.r) ** 2 * mp.mpf(tw.scale))
            Gx.append([-2 * mp.mpf(tw.scale) * a for a in d] + [mp.mpf(0)] * (nx - len(d))); Gu.append(zu())
        elif kind == 3:
            g += [mp.fsum([mp.mpf(tw.A[r, j]) * xm[j] for j in range(nx)]) - mp.mpf(tw.b[r]) for r in range(tw.dim)]
            for r in range(tw.dim):
                Gx.append([mp.mpf(tw.A[r, j]) for j in range(nx)]); Gu.append(zu())
        elif kind == 4:
            v = [xm[i] - mp.mpf(tw.o[i]) for i in range(3)]
            rn = mp.sqrt(mp.fsum([a * a for a in v]) + mp.mpf(tw.eps))
            g.append(rn * mp.mpf(tw.cosf) - mp.fsum([v[i] * mp.mpf(tw.ax[i]) for i in range(3)]))
            Gx.append([(mp.mpf(tw.cosf) * (v[i] / rn) if rn > mp.mpf(1e-9) else 0) - mp.mpf(tw.ax[i]) for i in range(3)] + [mp.mpf(0)] * (nx - 3)); Gu.append(zu())
        else:
            sq = mp.fsum([a * a for a in um])
            n, rn = mp.sqrt(sq), mp.sqrt(sq + mp.mpf(tw.eps))
            live = (rn > mp.mpf(sys.float_info.min)) if tw.mn is None else not (rn < mp.mpf(tw.eps))     # the rows are zeroed behind the guard
            row = [a / rn if live and rn != 0 else (mp.mpf(0) if not live else mp.nan) for a in um]
            if tw.mn is None:
                g.append(n - mp.mpf(tw.mx)); Gx.append(zx()); Gu.append(row)
            else:
                g += [mp.mpf(tw.mn) - n, n - mp.mpf(tw.mx)]
                Gx += [zx(), zx()]; Gu += [[-a for a in row], row]
    return g, Gx, Gu


def mp_err(got, ref):
    """max |got - ref| / max(1, |ref|) over a float64 array and the same-shaped nest of mpmath numbers."""
    got = np.asarray(got, dtype=np.float64).ravel()
    flat = [v for row in ref for v in (row if isinstance(row, list) else [row])]
    assert got.size == len(flat)
    return max([float(abs(mp.mpf(float(a)) - r) / max(mp.mpf(1), abs(r))) for a, r in zip(got, flat)] or [0.0])
