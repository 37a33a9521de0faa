"""The extended Kalman filter kernel on every model struct of PLANT_MODEL_LIST (csrc/plant_models.hpp): cddp_hip_ekf_run over T = 3 steps
with ny = 2, W and Wu, at B = 65 (a full 64-wide tile and a ragged one) and, for nx >= 10, B = 33 (the 32-wide tile edge), bitwise equal
to tests/plan_ekf_ref.py with f and jac as the DEVICE gives them: the step from DevicePlant.step, the Jacobians from the plant probe
(tests/hip/plant_probe.hip, the gfx950 build of the same Model::jac) -- so the comparison does not depend on a host libm.  The plants,
their parameters and their working ranges are those of tests/plant_probe.py (24 plants: test_model_cases.py holds that table to the list);
the 25th struct, the 1 x 1 LTI plant, has no probe entry and is evaluated in numpy, which is exact for it."""
import numpy as np
import pytest

import plan_cov_ref as PC
import plan_ekf_ref as PE

pytestmark = pytest.mark.gpu

T, NY = 3, 2


def tags():
    import plant_probe as PP
    return PP.TAGS + ["lti11"]


class DeviceModel:
    """f through a DevicePlant without a box (the reference clips before it calls), jac through the probe"""

    def __init__(self, api, PP, pl, B, integ, lower, upper):
        self.PP, self.pl, self.nx, self.nu, self.dt = PP, pl, pl.nx, pl.nu, pl.dt
        self.lower, self.upper = lower, upper
        kw = dict(lti_A=PP.LTI_A, lti_B=PP.LTI_B) if pl.tag == "lti21" else {}
        self.plant = api.DevicePlant(pl.id, integ, pl.dt, pl.nx, pl.nu, B, params=pl.params, **kw)

    def step(self, x, u):
        return self.plant.step(x, u)

    def jac(self, x, u):
        J = self.PP.run(self.PP.device(), "jac_" + self.pl.tag, self.PP.pack(self.pl, x, u)).T
        nx, nu = self.nx, self.nu
        return J[:, :nx * nx].reshape(-1, nx, nx).copy(), J[:, nx * nx:].reshape(-1, nx, nu).copy()


@pytest.mark.parametrize("tag", tags())
def test_run_on_every_model(api, tag):
    import plant_probe as PP
    rng = np.random.default_rng(20261080 + sum(ord(c) for c in tag))
    if tag == "lti11":
        nx, nu, dt, B, integ = 1, 1, 0.1, 65, api.EULER
        A, Bm = np.array([[0.9]]), np.array([[0.5]])
        lower, upper = np.array([-0.3]), np.array([0.4])
        model = PE.LtiModel(A, Bm, dt, lower, upper)
        plant = api.DevicePlant(api.MODEL_LTI, integ, dt, 1, 1, B, lti_A=A, lti_B=Bm, u_lower=lower, u_upper=upper)
        x0 = rng.standard_normal((B, 1))
        ident = 1
    else:
        pl = PP.BY_TAG[tag]
        nx, nu, dt = pl.nx, pl.nu, pl.dt
        B = 33 if nx >= 10 else 65
        integ = api.RK4
        lower, upper = -0.5 - 0.1 * np.arange(nu), 0.4 + 0.1 * np.arange(nu)
        kw = dict(lti_A=PP.LTI_A, lti_B=PP.LTI_B) if tag == "lti21" else {}
        plant = api.DevicePlant(pl.id, integ, dt, nx, nu, B, params=pl.params, u_lower=lower, u_upper=upper, **kw)
        model = DeviceModel(api, PP, pl, B, integ, lower, upper)
        x0 = PP.regular_set(pl, B)[0]
        ident = pl.id
    C = rng.standard_normal((NY, nx)); v = 0.05 + rng.random(NY)
    W = PC.spd(rng, nx, 1e-4); Wu = PC.spd(rng, nu, 1e-3); P0 = PC.spd(rng, nx, 1e-3)
    U = 0.6 * rng.standard_normal((B, T, nu))                                    # some entries beyond the box: the clip is exercised
    Y = (x0 @ C.T)[:, None, :] + 0.01 * rng.standard_normal((B, T + 1, NY))     # measurements near the estimate: it stays in the plant's range
    ref = PE.Filter(model, B, C, v, W, Wu)
    ref.reset(x0, P0)
    want = ref.run(Y, U)
    assert not want["info"].any() and np.all(np.isfinite(want["Xh"])) and np.all(np.isfinite(want["P"])), ident
    assert np.any(np.minimum(np.maximum(U, lower), upper) != U)
    ekf = api.DeviceEkf(plant, C, v, W, Wu)
    ekf.reset(x0, P0)
    got = ekf.run(Y, U)
    for k in ("Xh", "P", "nis", "info"):
        assert PE.same(got[k], want[k]), (tag, k, int(np.sum(got[k] != want[k])))
    xh, P, info = ekf.get()
    assert PE.same(xh, want["Xh"][:, -1]) and PE.same(P, want["P"][:, -1]) and not info.any()
    assert not PE.same(want["Xh"][:, 0], want["Xh"][:, -1])
    ekf.close(); plant.close()
    if tag != "lti11":
        model.plant.close()
