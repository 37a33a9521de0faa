"""Device-resident DubinsCar, DreyfusRocket, Acrobot, Usv3Dof, Forklift, QuadrotorRate, SpacecraftLinearFuel and SpacecraftNonlinear --
cddp_hip_model ids 16-23.

CPU: the library's host build of the plants (cddp_hip_model_eval: the kernels' own source, csrc/dev_models.hpp) against the numpy
restatements of tests/golden/plants_twin.py, which share no code with the product -- step values with every integrator, Jacobians
against complex step (finite differences for the fuel-state HCW plant), Hessians against hyper-dual numbers and against central
differences of the library's own Jacobians; the known answers of the reference's tests/dynamics_model/test_*.cpp files restated as
numbers; the refusals; the facade classes and their kept numpy methods; and the twin against a subset of its committed fixtures
(tests/golden/plants/*.json, tests/golden/make_plants_golden.py).  Tolerances are those of tests/test_spacecraft_plants.py.

GPU: the resident solves against the numpy twin: one sweep (K, k, V_x, V_xx, dV, every line-search trial) at 1e-8, the whole solve
in iterations, status and sweep / rollout counts; full DDP at step level; one LogDDP and one MSIPDDP solve against their twins;
batch independence; the facade's solve_batch; and the plug-in route for Python subclasses of the restated plants (model = None)."""
import glob
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(REPO, "oracle", "twin"))
import plants_twin as P  # noqa: E402

MEAN_MOTION = float(np.sqrt(3.986004418e14 / (6371e3 + 500e3) ** 3))
ACROBOT = [1.1, 0.9, 1.2, 0.8, 1.0, 0.7]
FORKLIFT = [2.0, 1.0, 0.785398]
INTEGRATORS = {"euler": 0, "heun": 1, "rk3": 2, "rk4": 3}
KINDS = ["dubins", "dreyfus", "acrobot", "usv", "forklift", "quadrotorrate", "linearfuel", "nonlinear"]
QUADROTOR_RATE = [1.0, 20.0, 0.5]
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "plants", "*.json")))
FIXTURE_NAMES = [os.path.basename(f)[:-len(".json")] for f in FIXTURES]
EXPECTED_FIXTURES = sorted("%s_%s_box" % (k, s) for k in KINDS for s in ("clddp", "ipddp"))


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def plants(api):
    """name -> (model id, parameters handed to the library, twin plant, dt, sampler of (x, u))"""
    def uniform(nx, nu):
        return lambda rng: (rng.uniform(-0.8, 0.8, nx), rng.uniform(-1.0, 1.0, nu))
    def fuel(rng):
        x = rng.uniform(-0.8, 0.8, 8); x[6] = rng.uniform(0.5, 2.0)      # a positive mass
        return x, rng.uniform(-1.0, 1.0, 3)
    def quad(rng):
        x = rng.uniform(-0.8, 0.8, 10); x[6:10] = rng.uniform(-1.0, 1.0, 4) + np.array([1.5, 0, 0, 0])   # an un-normalised quaternion on purpose
        return x, np.concatenate([rng.uniform(5.0, 15.0, 1), rng.uniform(-0.5, 0.5, 3)])
    def orbit(rng):
        return np.concatenate([rng.uniform(-0.1, 0.1, 6), [rng.uniform(0.9, 1.1), rng.uniform(-1, 1), rng.uniform(-0.1, 0.1), rng.uniform(0.9, 1.1)]]), rng.uniform(-0.2, 0.2, 3)
    return {
        "quadrotorrate": (api.MODEL_QUADROTOR_RATE, QUADROTOR_RATE, P.QuadrotorRate(*QUADROTOR_RATE), 0.05, quad),
        "nonlinear": (api.MODEL_SPACECRAFT_NONLINEAR, [1.3, 1.0, 1.0, 0.9], P.SpacecraftNonlinear(1.3, 1.0, 1.0, 0.9), 0.05, orbit),
        "dubins": (api.MODEL_DUBINS_CAR, [1.3], P.DubinsCar(1.3), 0.1, uniform(3, 1)),
        "dreyfus": (api.MODEL_DREYFUS_ROCKET, [64.0, 32.0], P.DreyfusRocket(64.0, 32.0), 0.01, uniform(2, 1)),
        "acrobot": (api.MODEL_ACROBOT, ACROBOT, P.Acrobot(*ACROBOT), 0.02, uniform(4, 1)),
        "usv": (api.MODEL_USV_3DOF, [], P.Usv3Dof(), 0.1, uniform(6, 3)),
        "forklift": (api.MODEL_FORKLIFT, FORKLIFT, P.Forklift(2.0, 0.03, True, 0.785398), 0.03, uniform(5, 2)),
        "linearfuel": (api.MODEL_SPACECRAFT_LINEAR_FUEL, [MEAN_MOTION, 300.0, 9.80665], P.SpacecraftLinearFuel(MEAN_MOTION, 300.0, 9.80665), 10.0, fuel),
    }


EXACT = ["dubins", "dreyfus", "acrobot", "usv", "forklift", "quadrotorrate"]     # autodiff / analytic Jacobians
FD = ["linearfuel", "nonlinear"]


def _twin_step(tw, integ, dt, x, u):
    import cddp_twin as T
    return T.discrete_step(tw, integ, dt, x, u, 0.0)


def _eval(api, name, x, u, want, integ="euler", dt=None):
    mid, prm, tw, dt0, _ = plants(api)[name]
    return api.model_eval(mid, INTEGRATORS[integ], dt0 if dt is None else dt, prm, tw.nx, tw.nu, x, u, want=want)


# ================================================================================ CPU: the plants
@pytest.mark.parametrize("integ", list(INTEGRATORS))
@pytest.mark.parametrize("name", KINDS)
def test_step_matches_the_numpy_restatement(api, name, integ):
    mid, prm, tw, dt, sample = plants(api)[name]
    rng = np.random.default_rng(20261016)
    for _ in range(8):
        x, u = sample(rng)
        got = _eval(api, name, x, u, ("step",), integ)["step"]
        assert rel_err(got, _twin_step(tw, integ, dt, x, u)) < 1e-13, (name, integ, x, u)


@pytest.mark.parametrize("name", EXACT)
def test_jacobians_match_complex_step(api, name):
    _, _, tw, _, sample = plants(api)[name]
    rng = np.random.default_rng(11)
    for _ in range(8):
        x, u = sample(rng)
        fx, fu = _eval(api, name, x, u, ("jac",))["jac"]
        cx, cu = tw.jac(x, u, 0.0)
        assert rel_err(fx, cx) < 1e-12 and rel_err(fu, cu) < 1e-12, name


@pytest.mark.parametrize("name", FD)
def test_finite_difference_jacobians_match_the_twins_own(api, name):
    _, _, tw, _, sample = plants(api)[name]
    rng = np.random.default_rng(12)
    for _ in range(8):
        x, u = sample(rng)
        fx, fu = _eval(api, name, x, u, ("jac",))["jac"]
        cx, cu = tw.jac(x, u, 0.0)
        assert rel_err(fx, cx) < 1e-9 and rel_err(fu, cu) < 1e-9, name


@pytest.mark.parametrize("name", EXACT)
def test_hessians_match_hyper_duals_and_finite_differences_of_the_jacobians(api, name):
    """(Forklift: both sides carry the 1 / timestep of forklift.cpp:89-125 -- the Jacobians differenced here are (d step - I) / timestep.)"""
    _, _, tw, _, sample = plants(api)[name]
    nx, nu = tw.nx, tw.nu
    rng = np.random.default_rng(13)
    for _ in range(3):
        x, u = sample(rng)
        fxx, fuu, fux = _eval(api, name, x, u, ("hess",))["hess"]
        hx, hu, hux = tw.hess(x, u, 0.0)          # hyper-dual numbers on the twin's autodiff expression: exact
        assert rel_err(fxx, hx) < 1e-10 and rel_err(fuu, hu) < 1e-10 and rel_err(fux, hux) < 1e-10, name
        h = 1e-5
        for j in range(nx + nu):   # central differences of the library's own Jacobians
            dz = np.zeros(nx + nu); dz[j] = h
            jp = _eval(api, name, x + dz[:nx], u + dz[nx:], ("jac",))["jac"]; jm = _eval(api, name, x - dz[:nx], u - dz[nx:], ("jac",))["jac"]
            dfx = (jp[0] - jm[0]) / (2 * h); dfu = (jp[1] - jm[1]) / (2 * h)
            if j < nx:
                assert rel_err(fxx[:, :, j], dfx) < 1e-6, (name, j)
            else:
                assert rel_err(fuu[:, :, j - nx], dfu) < 1e-6, (name, j)
                assert rel_err(fux[:, j - nx, :], dfx) < 1e-6, (name, j)


def test_forklift_hessians_carry_the_timestep(api):
    """forklift.cpp:89-125: hessian of the DISCRETE map / timestep, so d2 theta+ / dv d delta = -sec^2(delta) / L whatever the timestep."""
    x = np.array([0.1, -0.2, 0.3, 0.7, 0.2]); u = np.array([0.1, 0.05])
    for dt in (0.01, 0.05):
        fxx, fuu, fux = api.model_eval(api.MODEL_FORKLIFT, api.EULER, dt, FORKLIFT, 5, 2, x, u, want=("hess",))["hess"]
        assert abs(fxx[2, 3, 4] - (-1.0 / np.cos(0.2) ** 2 / 2.0)) < 1e-12 and np.all(fuu == 0.0) and np.all(fux == 0.0)
        assert abs(fxx[0, 2, 2] - (-0.7 * np.cos(0.3))) < 1e-12


def test_linear_fuel_hessians_are_exactly_zero(api):
    x, u = plants(api)["linearfuel"][4](np.random.default_rng(3))
    for block in _eval(api, "linearfuel", x, u, ("hess",))["hess"]:
        assert np.all(block == 0.0)


def test_usv_control_hessian_is_zero_and_the_others_are_not(api):
    x, u = plants(api)["usv"][4](np.random.default_rng(5))
    fxx, fuu, fux = _eval(api, "usv", x, u, ("hess",))["hess"]
    assert np.all(fuu == 0.0) and np.all(fux == 0.0) and np.max(np.abs(fxx)) > 0.1


# ---- the known answers the reference's tests/dynamics_model/test_*.cpp hold, restated as numbers
def test_forklift_known_answers_of_the_reference(api):
    """test_forklift.cpp:28-91: dt 0.01, wheelbase 2; a straight step, the steering and speed integrators, rear against front steering."""
    ev = lambda prm, x, u: api.model_eval(api.MODEL_FORKLIFT, api.EULER, 0.01, prm, 5, 2, np.array(x, float), np.array(u, float))["step"]
    n = ev(FORKLIFT, [0, 0, 0, 1.0, 0], [0, 0])
    assert np.max(np.abs(n - np.array([0.01, 0.0, 0.0, 1.0, 0.0]))) < 1e-6
    assert abs(ev(FORKLIFT, [0] * 5, [0.0, 0.5])[4] - 0.005) < 1e-6 and abs(ev(FORKLIFT, [0] * 5, [2.0, 0.0])[3] - 0.02) < 1e-6
    rear = ev([2.0, 1.0, 0.785398], [0, 0, 0, 1.0, np.pi / 6], [0, 0]); front = ev([2.0, 0.0, 0.785398], [0, 0, 0, 1.0, np.pi / 6], [0, 0])
    assert abs(rear[2] + front[2]) < 1e-6 and rear[2] < 0.0 < front[2]
    # :93-150: the Jacobians are finite and equal a numerical derivative of the continuous form (x+ - x) / dt at 1e-4
    x = np.array([0.0, 0.0, 0.0, 1.0, 0.1]); u = np.array([0.1, 0.05])
    A, B = api.model_eval(api.MODEL_FORKLIFT, api.EULER, 0.01, FORKLIFT, 5, 2, x, u, want=("jac",))["jac"]
    f = lambda z: (ev(FORKLIFT, z, u) - z) / 0.01
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(B)) and np.max(np.abs(A - P.fd_jacobian(f, x, 1e-7))) < 1e-4


def test_dubins_and_dreyfus_known_answers_of_the_reference(api):
    """test_dubins_car.cpp:28-58 (speed 1, dt 0.1, turn rate 0.5 for 50 Euler steps: the heading is 0.5 * 5 s, the path has unit speed) and
    test_dreyfus_rocket.cpp:27-68 (dt 0.05, RK4, thrust angle pi / 4 for 100 steps: the rocket has climbed and still climbs)."""
    x = np.zeros(3)
    for _ in range(50):
        xn = api.model_eval(api.MODEL_DUBINS_CAR, api.EULER, 0.1, [1.0], 3, 1, x, np.array([0.5]))["step"]
        assert abs(np.hypot(xn[0] - x[0], xn[1] - x[1]) - 0.1) < 1e-12
        x = xn
    assert abs(x[2] - 2.5) < 1e-12
    s = np.zeros(2)
    for _ in range(100):
        s = api.model_eval(api.MODEL_DREYFUS_ROCKET, api.RK4, 0.05, [64.0, 32.0], 2, 1, s, np.array([np.pi / 4]))["step"]
    acc = 64.0 * np.cos(np.pi / 4) - 32.0          # constant acceleration: RK4 is exact
    assert s[0] > 0.0 and s[1] > 0.0 and abs(s[1] - acc * 5.0) < 1e-9 and abs(s[0] - 0.5 * acc * 25.0) < 1e-9


def test_acrobot_known_answers_of_the_reference(api):
    """test_acrobot.cpp:104-187 (unit parameters): the torque enters the two accelerations only; rest at theta1 = pi stays at rest in the
    angle rows; a small offset accelerates; the torque's sign moves the accelerations and not the angle rates."""
    one = [1.0] * 6
    f = lambda x, u: api.model_eval(api.MODEL_ACROBOT, api.EULER, 1.0, one, 4, 1, np.array(x, float), np.array(u, float))["step"] - np.array(x, float)
    _, B = api.model_eval(api.MODEL_ACROBOT, api.RK4, 0.01, one, 4, 1, np.array([np.pi / 6, -np.pi / 8, 0.1, -0.1]), np.array([1.0]), want=("jac",))["jac"]
    assert B.shape == (4, 1) and B[0, 0] == 0.0 and B[1, 0] == 0.0 and B[2, 0] != 0.0 and B[3, 0] != 0.0
    sd = f([np.pi, 0.0, 0.0, 0.0], [0.0])
    assert abs(sd[0]) < 1e-10 and abs(sd[1]) < 1e-10
    assert abs(f([0.01, 0.0, 0.0, 0.0], [0.0])[2]) > 1e-6
    pos = f([np.pi / 4, -np.pi / 6, 0.0, 0.0], [1.0]); neg = f([np.pi / 4, -np.pi / 6, 0.0, 0.0], [-1.0])
    assert pos[0] == neg[0] and pos[1] == neg[1] and pos[2] != neg[2] and pos[3] != neg[3]


def test_usv_and_linear_fuel_known_answers_of_the_reference(api):
    """test_usv_3dof.cpp:30-90 (dt 0.05: the state moves under a surge force, shapes, a zero control Hessian) and
    test_spacecraft_linear_fuel.cpp:30-82 (dt 1, Isp 300, g0 9.81: without thrust the mass changes only by the epsilon under the norm,
    the effort state not at all, and the position rows are the HCW drift)."""
    x0 = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0]); u0 = np.array([10.0, 0.0, 1.0])
    r = api.model_eval(api.MODEL_USV_3DOF, api.EULER, 0.05, [], 6, 3, x0, u0, want=("step", "jac", "hess"))
    assert not np.allclose(r["step"], x0) and r["jac"][0].shape == (6, 6) and r["jac"][1].shape == (6, 3)
    assert r["hess"][0].shape == (6, 6, 6) and r["hess"][1].shape == (6, 3, 3) and np.max(np.abs(r["hess"][1])) < 1e-9
    assert abs(r["step"][3] - (1.0 + 0.05 * (10.0 - 20.0 * 1.0) / 110.0)) < 1e-12      # surge: (tau_u - X_u-damping) / (m - X_udot)
    x = np.array([-37.59664132226163, 27.312455860666148, 13.656227930333074, 0.015161970413423813, 0.08348413138390476, 0.04174206569195238, 100.0, 0.0])
    n = 0.0011
    s = api.model_eval(api.MODEL_SPACECRAFT_LINEAR_FUEL, api.EULER, 1.0, [n, 300.0, 9.81], 8, 3, x, np.zeros(3))["step"]
    assert np.max(np.abs(s[:3] - (x[:3] + x[3:6]))) < 1e-12 and s[7] == 0.0 and abs(s[6] - (100.0 - 1e-4 / (300.0 * 9.81))) < 1e-12
    assert abs(s[3] - (x[3] + 2.0 * n * x[4] + 3.0 * n * n * x[0])) < 1e-15


def test_quadrotor_rate_known_answers_of_the_reference(api):
    """test_quadrotor_rate.cpp:72-140 (mass 1, max thrust 20, max rate 0.5): hover thrust at the identity attitude is an equilibrium at
    1e-10; a roll rate of 0.1 moves qx at 0.05 per second and nothing else in the quaternion."""
    x = np.array([0.0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
    f = lambda u: api.model_eval(api.MODEL_QUADROTOR_RATE, api.EULER, 1.0, QUADROTOR_RATE, 10, 4, x, np.array(u, float))["step"] - x
    assert np.max(np.abs(f([9.81, 0, 0, 0]))) < 1e-10
    sd = f([9.81, 0.1, 0, 0])
    assert abs(sd[7] - 0.05) < 1e-12 and abs(sd[6]) < 0.01 and abs(sd[8]) < 1e-10 and abs(sd[9]) < 1e-10
    # the value normalises q: a scaled quaternion gives the same accelerations
    x2 = x.copy(); x2[6:10] = [2.0, 0.4, -0.6, 0.8]; x3 = x2.copy(); x3[6:10] /= np.linalg.norm(x3[6:10])
    g = lambda z: api.model_eval(api.MODEL_QUADROTOR_RATE, api.EULER, 1.0, QUADROTOR_RATE, 10, 4, z, np.array([12.0, 0.1, -0.2, 0.3]))["step"] - z
    assert np.max(np.abs(g(x2) - g(x3))) < 1e-14


def test_spacecraft_nonlinear_known_answers_of_the_reference(api):
    """spacecraft_nonlinear.cpp:37-62 with the normalised constants of test_spacecraft_nonlinear.cpp:66-72 (mu = 1, mass 1): a deputy on
    the chief's circular orbit of radius 1 does not move relative to it, the orbit angle advances at rate 1; a radial offset is pulled by
    the tidal term 3 px to first order; the state stays finite over a step (:61)."""
    ev = lambda x, u: api.model_eval(api.MODEL_SPACECRAFT_NONLINEAR, api.EULER, 1.0, [1.0, 1.0, 1.0, 1.0], 10, 3, np.array(x, float), np.array(u, float))["step"] - np.array(x, float)
    sd = ev([0, 0, 0, 0, 0, 0, 1.0, 0.3, 0.0, 1.0], [0, 0, 0])
    assert np.max(np.abs(sd - np.array([0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0]))) < 1e-15
    sd = ev([1e-4, 0, 0, 0, 0, 0, 1.0, 0.0, 0.0, 1.0], [0.01, -0.02, 0.03])
    assert abs(sd[3] - (3e-4 + 0.01)) < 1e-7 and abs(sd[4] + 0.02) < 1e-12 and abs(sd[5] - 0.03) < 1e-12
    st = api.model_eval(api.MODEL_SPACECRAFT_NONLINEAR, api.RK4, 0.01, [1.0, 1.0, 1.0, 1.0], 10, 3,
                        np.array([-0.01127, 0.0, 0.1, 0.02, 0.02, 0.0, 0.9, 0.0, 0.0, 1.2]), np.zeros(3))["step"]
    assert np.all(np.isfinite(st))


# ================================================================================ CPU: refusals
@pytest.mark.parametrize("prm,msg", [([0.0, 20.0, 0.5], "Mass must be positive"), ([1.0, -1.0, 0.5], "Maximum thrust must be positive"),
                                     ([1.0, 20.0, 0.0], "Maximum angular rate must be positive")])
def test_quadrotor_rate_parameters_must_be_positive(api, prm, msg):
    """quadrotor_rate.cpp:28-36, the reference's three messages: from the library, the facade and the twin alike."""
    with pytest.raises(api.HipError, match=msg):
        api.model_eval(api.MODEL_QUADROTOR_RATE, api.EULER, 0.1, prm, 10, 4, np.r_[np.zeros(6), 1.0, 0, 0, 0], np.zeros(4))
    with pytest.raises(ValueError, match=msg):
        _facade().QuadrotorRate(0.01, *prm)
    with pytest.raises(ValueError, match=msg):
        P.QuadrotorRate(*prm)


def test_spacecraft_nonlinear_second_derivatives_are_refused_with_the_reference_message(api):
    with pytest.raises(api.HipError, match="getContinuousDynamicsAutodiff must be overridden"):
        api.model_eval(api.MODEL_SPACECRAFT_NONLINEAR, api.EULER, 0.1, [1.0, 1.0, 1.0, 1.0], 10, 3, np.r_[np.zeros(6), 1.0, 0, 0, 1.0], np.zeros(3), want=("hess",))
    with pytest.raises(RuntimeError, match="getContinuousDynamicsAutodiff"):
        _facade().SpacecraftNonlinear(0.01).get_state_hessian(np.r_[np.zeros(6), 1.0, 0, 0, 1.0], np.zeros(3))


@pytest.mark.parametrize("mid_name,nx,nu", [("MODEL_DUBINS_CAR", 3, 2), ("MODEL_DREYFUS_ROCKET", 3, 1), ("MODEL_ACROBOT", 4, 2), ("MODEL_USV_3DOF", 6, 2),
                                            ("MODEL_FORKLIFT", 4, 2), ("MODEL_SPACECRAFT_LINEAR_FUEL", 6, 3), ("MODEL_QUADROTOR_RATE", 13, 4),
                                            ("MODEL_SPACECRAFT_NONLINEAR", 10, 4)])
def test_wrong_dimensions_are_refused(api, mid_name, nx, nu):
    with pytest.raises(api.HipError, match="has nx = "):
        api.model_eval(getattr(api, mid_name), api.EULER, 0.1, [1.0, 1.0, 1.0], nx, nu, np.ones(nx), np.zeros(nu))


# ================================================================================ CPU: the facade
def _facade():
    import importlib.util
    name = "pycddp_amd"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return sys.modules[name]


def _facade_plants(pc):
    """name -> the facade object that describes the plant of plants(api)[name]"""
    return {"dubins": pc.DubinsCar(1.3, 0.1), "dreyfus": pc.DreyfusRocket(0.01), "acrobot": pc.Acrobot(0.02, *ACROBOT, integration_type="rk4"),
            "usv": pc.Usv3Dof(0.1, "heun"), "forklift": pc.Forklift(0.03), "linearfuel": pc.SpacecraftLinearFuel(10.0, MEAN_MOTION, 300.0),
            "quadrotorrate": pc.QuadrotorRate(0.05, *QUADROTOR_RATE, integration_type="rk4"), "nonlinear": pc.SpacecraftNonlinear(0.05, "heun", 1.3, 1.0, 1.0, 0.9)}


def test_facade_classes_take_the_reference_signatures(api):
    pc = _facade()
    d = pc.DubinsCar(speed=1.0, timestep=0.1)
    assert (d.integration_type, d.params, d.model) == ("euler", [1.0], api.MODEL_DUBINS_CAR)
    r = pc.DreyfusRocket(timestep=0.05)
    assert (r.integration_type, r.params, r.model) == ("rk4", [64.0, 32.0], api.MODEL_DREYFUS_ROCKET)
    a = pc.Acrobot(timestep=0.01)
    assert (a.integration_type, a.params, a.model) == ("euler", [1.0] * 6, api.MODEL_ACROBOT)
    u = pc.Usv3Dof(timestep=0.1)
    assert (u.integration_type, u.params, u.model) == ("euler", [], api.MODEL_USV_3DOF)
    f = pc.Forklift()
    assert (f.timestep, f.integration_type, f.params, f.model) == (0.01, "euler", FORKLIFT, api.MODEL_FORKLIFT)
    assert pc.Forklift(0.02, 1.5, "euler", False, 0.5).params == [1.5, 0.0, 0.5]
    s = pc.SpacecraftLinearFuel(timestep=1.0, mean_motion=0.001, isp=300.0)
    assert (s.integration_type, s.params, s.model) == ("euler", [0.001, 300.0, 9.80665], api.MODEL_SPACECRAFT_LINEAR_FUEL)
    q = pc.QuadrotorRate(timestep=0.01, mass=1.0, max_thrust=20.0, max_rate=0.5)
    assert (q.integration_type, q.params, q.model, q.state_dim, q.control_dim) == ("euler", QUADROTOR_RATE, api.MODEL_QUADROTOR_RATE, 10, 4)
    n = pc.SpacecraftNonlinear(timestep=0.01)
    assert (n.integration_type, n.params, n.model, n.state_dim, n.control_dim) == ("rk4", [1.0, 1.0, 1.0, 1.0], api.MODEL_SPACECRAFT_NONLINEAR, 10, 3)
    assert pc.SpacecraftNonlinear(0.01, "euler", 2.0, 3.0, 4.0, 5.0).params == [2.0, 3.0, 4.0, 5.0]
    rng = np.random.default_rng(14)
    P_ = plants(api)
    for name, obj in _facade_plants(pc).items():
        tw, sample = P_[name][2], P_[name][4]
        x, c = sample(rng)
        assert (obj.state_dim, obj.control_dim) == (tw.nx, tw.nu)
        assert rel_err(obj.get_discrete_dynamics(x, c), _twin_step(tw, obj.integration_type, obj.timestep, x, c)) < 1e-13
        assert rel_err(obj.get_state_jacobian(x, c), tw.jac(x, c, 0.0)[0]) < 1e-9


def test_a_subclass_with_model_none_is_a_host_plant():
    pc = _facade()
    class HostDubins(pc.DubinsCar):
        model = None
    assert HostDubins(1.0, 0.1).model is None and pc.DubinsCar(1.0, 0.1).model is not None


@pytest.mark.parametrize("name", ["dubins", "dreyfus", "acrobot", "usv", "linearfuel"])
def test_model_eval_equals_the_kept_numpy_methods(api, name):
    """The five classes that had a host restatement keep it (get_continuous_dynamics and the numpy Jacobians); the library's plant
    evaluates to the same numbers: 1e-12, 1e-9 for the finite differences of SpacecraftLinearFuel."""
    pc = _facade()
    obj = _facade_plants(pc)[name]
    mid, prm, tw, _, sample = plants(api)[name]
    tol = 1e-9 if name == "linearfuel" else 1e-12
    rng = np.random.default_rng(15)
    for _ in range(4):
        x, u = sample(rng)
        r = api.model_eval(mid, api.EULER, 1.0, prm, tw.nx, tw.nu, x, u, want=("step", "jac", "hess"))
        assert rel_err(r["step"] - x, obj.get_continuous_dynamics(x, u)) < 1e-12
        assert rel_err(r["jac"][0], obj.get_state_jacobian(x, u)) < tol and rel_err(r["jac"][1], obj.get_control_jacobian(x, u)) < tol
        for got, kept in zip(r["hess"], (obj.get_state_hessian(x, u), obj.get_control_hessian(x, u), obj.get_cross_hessian(x, u))):
            assert rel_err(got, np.stack(kept)) < 1e-12
    if name == "usv":
        H = obj.get_control_hessian(np.zeros(6), np.zeros(3))
        assert len(H) == 6 and all(h.shape == (3, 3) and np.all(h == 0.0) for h in H)


# ================================================================================ CPU: the fixtures
def _load(name):
    with open(os.path.join(HERE, "golden", "plants", name + ".json")) as f:
        return json.load(f)


def test_fixtures_present():
    assert FIXTURE_NAMES == EXPECTED_FIXTURES, FIXTURE_NAMES


@pytest.mark.parametrize("name", ["acrobot_ipddp_box", "forklift_clddp_box", "usv_ipddp_box", "quadrotorrate_ipddp_box", "nonlinear_clddp_box"])
def test_twin_reproduces_its_fixtures(name):
    import make_plants_golden as MG
    fx = _load(name)
    out = MG.run_case(name, with_solve=False)
    assert out["sweep"]["ok"] == fx["sweep"]["ok"] and out["sweep"]["reg"] == fx["sweep"]["reg"]
    for key in ("K", "k", "Vx", "Vxx", "dV"):
        assert rel_err(out["sweep"][key], fx["sweep"][key]) < 1e-12, key
    assert [t["success"] for t in out["trials"]] == [t["success"] for t in fx["trials"]]


# ================================================================================ GPU
def _problem(api, name, solver=None, **kw):
    kind, solv, _ = name.split("_")
    s = {"clddp": api.SOLVER_CLDDP, "ipddp": api.SOLVER_IPDDP}[solv] if solver is None else solver
    build = {"dubins": api.dubins_problem, "dreyfus": api.dreyfus_problem, "acrobot": api.acrobot_problem, "usv": api.usv_problem,
             "forklift": api.forklift_problem, "linearfuel": api.linear_fuel_problem, "quadrotorrate": api.quadrotor_rate_problem,
             "nonlinear": api.spacecraft_nonlinear_problem}[kind]
    return build(s, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXPECTED_FIXTURES)
def test_hip_matches_twin(api, name):
    """One sweep at 1e-8 (gains, value expansion, dV, every trial), then the whole solve (counts equal, objective at 1e-6)."""
    fx = _load(name)
    p = _problem(api, name)
    U0 = api.batch_U0(p, 1)
    hs = api.HipBatchSolver(p, 1)
    hs.set_initial(p.x0[None, :], U0)
    hs.initialize()
    ok = hs.backward()
    sw = fx["sweep"]
    assert bool(ok[0]) == sw["ok"]
    K, k = hs.gains(); Vx, Vxx = hs.value(); dV, reg = hs.backward_scalars()
    assert reg[0] == sw["reg"]
    for i, t in enumerate(sw["t"]):
        errs = (rel_err(K[0, t], sw["K"][i]), rel_err(k[0, t], sw["k"][i]), rel_err(Vx[0, t], sw["Vx"][i]), rel_err(Vxx[0, t], sw["Vxx"][i]))
        print(name, "t", t, "K %.2e k %.2e Vx %.2e Vxx %.2e" % errs)
        assert max(errs) < 1e-8, (name, t)
    print(name, "dV %.2e" % rel_err(dV[0], sw["dV"]))
    assert rel_err(dV[0], sw["dV"]) < 1e-8
    trials = hs.forward(np.array(fx["alphas"]))
    for a, tr in enumerate(fx["trials"]):
        g = trials[0, a]
        assert bool(g["success"]) == tr["success"], (name, tr["alpha"])
        if tr["success"]:
            assert rel_err(g["cost"], tr["cost"]) < 1e-8 and rel_err(g["merit_function"], tr["merit"]) < 1e-8
    hs.close()
    p2 = _problem(api, name)
    hs = api.HipBatchSolver(p2, 1)
    hs.set_initial(p2.x0[None, :], U0)
    hs.solve()
    r = hs.results()[0]
    fs = fx["solve"]
    print(name, "solve", int(r["iterations"]), int(r["status"]), int(r["n_backward"]), int(r["n_forward"]), float(r["final_objective"]), "twin",
          fs["iterations"], fs["status"], fs["n_backward"], fs["n_forward"], fs["final_objective"])
    assert (int(r["iterations"]), int(r["status"]), int(r["n_backward"]), int(r["n_forward"])) == (fs["iterations"], fs["status"], fs["n_backward"], fs["n_forward"]), (name, r)
    assert rel_err(r["final_objective"], fs["final_objective"]) < 1e-6
    hs.close()


DDP_HORIZON = 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dubins_ipddp_box", "dreyfus_ipddp_box", "acrobot_ipddp_box", "usv_ipddp_box", "forklift_ipddp_box", "linearfuel_ipddp_box",
                                  "quadrotorrate_ipddp_box"])
def test_hip_full_ddp_step_level(api, name):
    """use_ilqr = 0: the second-order dynamics terms in the sweep (explicit tensors; blocked duals on the surface vessel; zero on the
    fuel-state HCW plant) against the twin with its hyper-dual Hessians.  On a horizon of 20 steps: at the first iterate the tensor
    terms make Q_xx indefinite on the vessel and the forklift, and the value recursion then amplifies a perturbation with every step --
    in the twin itself a 1e-13 change of x0 moves the vessel's gains by 1e+2 over its 80 steps and the forklift's by 2e-6 over its 100,
    against 2e-9 / 2e-12 over 20 steps -- so the whole horizon would compare rounding, not the tensor terms."""
    import make_plants_golden as MG
    kind = name.split("_")[0]
    spec = MG.BUILDERS[kind]("IPDDP", N=DDP_HORIZON); spec["options"]["use_ilqr"] = False
    tw = MG.G.T.Twin(spec)
    tw.set_initial(np.array(spec["x0"], float), spec.get("U0")); tw.initialize()
    ok = tw.backward()
    p = _problem(api, name, horizon=DDP_HORIZON); p.options.use_ilqr = 0
    U0 = api.batch_U0(p, 1)
    hs = api.HipBatchSolver(p, 1)
    hs.set_initial(p.x0[None, :], U0); hs.initialize()
    hok = hs.backward()
    assert bool(ok) and bool(hok[0])
    K, k = hs.gains(); Vx, Vxx = hs.value()
    errs = (rel_err(K[0], tw.K_u), rel_err(k[0], tw.k_u), rel_err(Vx[0], tw.Vx), rel_err(Vxx[0], tw.Vxx))
    print(name, "full DDP K %.2e k %.2e Vx %.2e Vxx %.2e" % errs)
    assert max(errs) < 1e-8
    hs.close()


@pytest.mark.gpu
def test_spacecraft_nonlinear_full_ddp_is_refused(api):
    p = api.spacecraft_nonlinear_problem(api.SOLVER_IPDDP); p.options.use_ilqr = 0
    with pytest.raises(api.HipError, match="getContinuousDynamicsAutodiff must be overridden"):
        api.HipBatchSolver(p, 4)


@pytest.mark.gpu
def test_hip_logddp_solve_matches_its_twin(api):
    import logddp_twin as L
    import make_plants_golden as MG
    spec = MG.CASES["usv_ipddp_box"]()
    tw = L.LogDDP(spec); tw.set_initial(spec["x0"], spec.get("U0")); r = tw.solve()
    p = api.usv_problem(api.SOLVER_LOGDDP)
    hs = api.HipBatchSolver(p, 1); hs.set_initial(p.x0[None, :]); hs.solve()
    res = hs.results()[0]; X, U = hs.trajectory(); hs.close()
    print("logddp", dict(zip(res.dtype.names, res)), r)
    assert (int(res["iterations"]), api.STATUS_STRINGS[int(res["status"])], int(res["n_backward"]), int(res["n_forward"])) == \
        (r["iterations"], r["status"], r["n_backward"], r["n_forward"]), r
    assert rel_err(res["final_objective"], r["final_objective"]) < 1e-6
    assert np.max(np.abs(X[0] - tw.X)) < 1e-6 and np.max(np.abs(U[0] - tw.U)) < 1e-6


@pytest.mark.gpu
def test_hip_msipddp_solve_matches_its_twin(api):
    """The Dubins car WITH its turn-rate box: nu = 1, the shape for which MSIPDDP with path rows is defined."""
    import msipddp_twin as M
    import make_plants_golden as MG
    spec = MG.CASES["dubins_ipddp_box"]()
    spec["options"].update(ms_rollout_type="nonlinear", ms_segment_length=5, warm_start=False)
    tw = M.MSIPDDP(spec); tw.set_initial(np.array(spec["x0"], float), spec.get("U0"), None); r = tw.solve()
    p = api.dubins_problem(api.SOLVER_MSIPDDP)
    p.options.msipddp_segment_length = 5; p.options.warm_start = 0
    hs = api.HipBatchSolver(p, 1); hs.set_initial(p.x0[None, :], api.batch_U0(p, 1)); hs.solve()
    res = hs.results()[0]; X, U = hs.trajectory(); hs.close()
    print("msipddp", dict(zip(res.dtype.names, res)), r)
    assert (int(res["iterations"]), api.STATUS_STRINGS[int(res["status"])], int(res["n_backward"]), int(res["n_forward"])) == \
        (r["iterations"], r["status"], r["n_backward"], r["n_forward"]), r
    assert rel_err(res["final_objective"], r["final_objective"]) < 1e-6
    assert np.max(np.abs(U[0] - tw.U)) < 1e-6


SPREAD = {"dubins": [0.05, 0.05, 0.02], "dreyfus": [0.02, 0.05], "acrobot": [0.02] * 4, "usv": [0.05] * 6, "forklift": [0.05, 0.05, 0.02, 0.02, 0.01],
          "linearfuel": [0.5, 0.5, 0.5, 0.002, 0.002, 0.002, 0.01, 0.0], "quadrotorrate": [0.05] * 6 + [0.0, 0.02, 0.02, 0.02],
          "nonlinear": [0.002] * 6 + [0.0] * 4}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batch_members_equal_their_single_solves(api, kind):
    """B = 1024 distinct initial states: four members (first, two inside, last) equal their B = 1 solves bit for bit."""
    p = _problem(api, kind + "_ipddp_box")
    B = 1024
    x0 = api.batch_x0(p, B, 20261016, SPREAD[kind])
    U0 = api.batch_U0(p, B)
    hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0); hs.solve()
    res = hs.results(); X, U = hs.trajectory(); hs.close()
    for b in (0, 333, 700, B - 1):
        h1 = api.HipBatchSolver(p, 1); h1.set_initial(x0[b:b + 1], None if U0 is None else U0[b:b + 1]); h1.solve()
        r1 = h1.results(); X1, U1 = h1.trajectory(); h1.close()
        for f in r1.dtype.names:
            assert np.array_equal(res[f][b:b + 1], r1[f], equal_nan=True), (kind, b, f)
        assert np.array_equal(X[b], X1[0]) and np.array_equal(U[b], U1[0]), (kind, b)


def _facade_solver(pc, api, p, sys_):
    opt = pc.CDDPOptions(); opt.verbose = False; opt.print_solver_header = False
    opt.max_iterations = p.options.max_iterations; opt.tolerance = p.options.tolerance; opt.acceptable_tolerance = p.options.acceptable_tolerance
    opt.regularization.initial_value = p.options.reg_initial_value
    solver = pc.CDDP(p.x0, p.x_ref, p.N, p.dt, opt)
    solver.set_dynamical_system(sys_)
    solver.set_objective(pc.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    c = p._cons[0]
    solver.add_constraint("ControlConstraint", pc.ControlConstraint(np.array(c.lower[:c.dim]), np.array(c.upper[:c.dim])))
    return solver


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_facade_solve_batch_is_resident_and_equals_the_handle(api, kind):
    pc = _facade()
    p = _problem(api, kind + "_ipddp_box")
    sys_ = {"dubins": lambda: pc.DubinsCar(1.0, p.dt), "dreyfus": lambda: pc.DreyfusRocket(p.dt), "acrobot": lambda: pc.Acrobot(p.dt, integration_type="rk4"),
            "usv": lambda: pc.Usv3Dof(p.dt, "rk4"), "forklift": lambda: pc.Forklift(p.dt),
            "linearfuel": lambda: pc.SpacecraftLinearFuel(p.dt, MEAN_MOTION, 300.0, integration_type="rk4"),
            "quadrotorrate": lambda: pc.QuadrotorRate(p.dt, *QUADROTOR_RATE, integration_type="rk4"), "nonlinear": lambda: pc.SpacecraftNonlinear(p.dt)}[kind]()
    solver = _facade_solver(pc, api, p, sys_)
    U0 = api.batch_U0(p, 8)
    if U0 is not None:
        solver.set_initial_trajectory([p.x0] * (p.N + 1), list(U0[0]))
    x0s = api.batch_x0(p, 8, 7, SPREAD[kind])
    sols = solver.solve_batch(list(x0s), pc.SolverType.IPDDP)
    assert all(s.route == "resident" for s in sols), [s.route for s in sols]
    ph = solver._problem(api.SOLVER_IPDDP)    # the descriptor the facade hands to the library
    hs = api.HipBatchSolver(ph, 8); hs.set_initial(x0s, U0); hs.solve()
    res = hs.results(); X, U = hs.trajectory(); hs.close()
    for b, s in enumerate(sols):
        assert (s.iterations_completed, s.status_message) == (int(res["iterations"][b]), api.STATUS_STRINGS[int(res["status"][b])])
        assert np.array_equal(np.stack(s.control_trajectory), U[b]) and np.array_equal(np.stack(s.state_trajectory), X[b]), (kind, b)


@pytest.mark.gpu
@pytest.mark.parametrize("plant", ["dubins_car", "spacecraft_linear_fuel"])
def test_python_subclass_of_a_restated_plant_solves_through_the_plugin_route(api, plant):
    """What tests/test_pycddp_reference_api.py::test_host_only_plant_solves_through_the_plugin_route covered before these plants had
    kernels: a Python subclass (model = None) of the Dubins car and of the fuel-aware HCW spacecraft, by CLDDP and IPDDP with a control
    box -- GPU backward passes on the stack-fed sweeps of shapes (3, 1, .) and (8, 3, .), host rollouts of the numpy restatements."""
    pc = _facade()

    class HostDubinsCar(pc.DubinsCar):
        model = None

    class HostSpacecraftLinearFuel(pc.SpacecraftLinearFuel):
        model = None

    dub = dict(make=lambda dt: HostDubinsCar(1.0, dt), dt=0.1, N=40, x0=np.zeros(3), goal=np.array([2.0, 1.0, 0.5]), Qf=50.0 * np.eye(3),
               R=0.1 * np.eye(1), box=1.5)
    sc = dict(make=lambda dt: HostSpacecraftLinearFuel(dt, mean_motion=0.001, isp=300.0), dt=1.0, N=30,
              x0=np.array([10.0, 5.0, 2.0, 0.0, 0.0, 0.0, 50.0, 0.0]), goal=np.r_[np.zeros(6), 50.0, 0.0], Qf=np.diag([50.0] * 6 + [0.0, 0.0]),
              R=0.1 * np.eye(3), box=2.0)
    c = {"dubins_car": dub, "spacecraft_linear_fuel": sc}[plant]
    dt, N, x0, goal = c["dt"], c["N"], c["x0"], c["goal"]
    nu = c["R"].shape[0]
    stand_still = float((x0 - goal) @ c["Qf"] @ (x0 - goal))
    for stype in (pc.SolverType.CLDDP, pc.SolverType.IPDDP):
        opts = pc.CDDPOptions(); opts.max_iterations = 60; opts.verbose = False; opts.print_solver_header = False
        solver = pc.CDDP(x0, goal, N, dt, opts)
        solver.set_dynamical_system(c["make"](dt))
        solver.set_objective(pc.QuadraticObjective(np.zeros((x0.size, x0.size)), c["R"], c["Qf"], goal, [], dt))
        solver.add_constraint("ControlConstraint", pc.ControlConstraint(-c["box"] * np.ones(nu), c["box"] * np.ones(nu)))
        sol = solver.solve(stype)
        assert sol.route == "plugin", sol.route
        X = np.stack(sol.state_trajectory); U = np.stack(sol.control_trajectory)
        print(plant, stype, sol.route, sol.status_message, sol.iterations_completed, sol.final_objective, stand_still)
        assert sol.status_message and np.all(np.isfinite(X)) and np.max(np.abs(U)) <= c["box"] + 1e-9
        assert sol.final_objective < 0.5 * stand_still          # well below the cost of standing still
        x = x0.copy(); model = c["make"](dt)
        for t in range(N):                                      # the returned trajectory is a rollout of the plant
            x = model.get_discrete_dynamics(x, U[t])
            assert np.max(np.abs(x - X[t + 1])) < 1e-9 * max(1.0, float(np.max(np.abs(x))))
