"""The device-resident extended Kalman filter (cddp_hip_ekf_*; include/cddp_hip.h "extended Kalman filter on the device").  The header
fixes the arithmetic, so every comparison is bitwise (plan_ekf_ref.same: NaN = NaN, -0.0 = 0.0) against tests/plan_ekf_ref.py, whose f
and jac are the host build of the same model structs in the kernels' own sin / cos (the plant probe's host library; numpy for the LTI
plant):
  1. run, and the loop over update / predict / get, on pendulum, cart-pole, unicycle and LTI: B = 1, 64, 65; T = 1, 3; ny = 1, nx, nx + 2;
     shared and per-trajectory plant parameters, sensors and P0; host and device pointers; full and DIAG output; W / Wu absent or given;
     a control box.  The object is left at the final posterior, and a second run continues from it;
  2. a NaN drop-out with CDDP_HIP_EKF_SKIP_NAN;
  3. one trajectory of the batch with a failing pivot: info, NaN from that step on, its neighbours bitwise what they are without it;
  4. the refusals that need a plant, each with its message, and that they change nothing."""
import numpy as np
import pytest

import plan_cov_ref as PC
import plan_ekf_ref as PE

pytestmark = pytest.mark.gpu

LTI_A = np.array([[1.0, 0.1], [-0.2, 0.95]])
LTI_B = np.array([[0.005], [0.1]])
PLANTS = {   # name: model id name, integrator name, dt, nx, nu, params, box
    "pendulum": ("MODEL_PENDULUM", "RK4", 0.02, 2, 1, [0.5, 1.0, 0.01, 9.81], ([-0.6], [0.4])),
    "cartpole": ("MODEL_CARTPOLE", "RK4", 0.05, 4, 1, [1.0, 0.2, 0.5, 9.81, 0.0], None),
    "unicycle": ("MODEL_UNICYCLE", "HEUN", 0.03, 3, 2, [], ([-0.5, -0.7], [0.8, 0.3])),
    "lti": ("MODEL_LTI", "EULER", 0.1, 2, 1, [], None),
}


def make(api, name, B, per_params=False, seed=0, tmp_path=None):
    """-> (DevicePlant, reference model)"""
    import plant_probe as PP
    mid, integ, dt, nx, nu, params, box = PLANTS[name]
    mid, integ = getattr(api, mid), getattr(api, integ)
    lo, up = box if box else (None, None)
    if name == "lti":
        return (api.DevicePlant(mid, integ, dt, nx, nu, B, lti_A=LTI_A, lti_B=LTI_B, u_lower=lo, u_upper=up), PE.LtiModel(LTI_A, LTI_B, dt, lo, up))
    pv = np.asarray(params, dtype=np.float64)
    if per_params:
        rng = np.random.default_rng(20261040 + seed)
        pv = pv[None, :] * rng.uniform(0.9, 1.1, (B, pv.size))
    assert PP.BY_TAG[name].dt == dt and PP.BY_TAG[name].id == mid
    return (api.DevicePlant(mid, integ, dt, nx, nu, B, params=pv, u_lower=lo, u_upper=up), PE.ProbeModel(PP, PP.host(tmp_path), name, integ, pv, lo, up))


def draw(name, B, T, ny, per_sensor, per_P0, have_w, have_wu, seed):
    _, _, _, nx, nu, _, _ = PLANTS[name]
    rng = np.random.default_rng(seed)
    lead = (B,) if per_sensor else ()
    d = dict(C=rng.standard_normal(lead + (ny, nx)), v=0.05 + rng.random(lead + (ny,)),
             W=PC.spd(rng, nx, 0.01, lead) if have_w else None, Wu=PC.spd(rng, nu, 0.05, lead) if have_wu else None,
             xh0=0.3 * rng.standard_normal((B, nx)), P0=PC.spd(rng, nx, 0.5, (B,) if per_P0 else ()),
             Y=0.5 * rng.standard_normal((B, T + 1, ny)), U=rng.standard_normal((B, T, nu)))
    P0 = d["P0"]
    if nx > 1:
        P0[..., 0, nx - 1] = 9.0           # junk above the diagonal: only the lower triangle is read
    return d


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


#        plant       B   T  ny      per_params per_sensor per_P0 device diag   W      Wu
CASES = [
    ("pendulum", 1, 1, "1", False, False, False, False, False, False, False),
    ("pendulum", 65, 3, "nx", True, False, True, False, False, True, True),
    ("pendulum", 64, 3, "nx+2", False, True, False, True, True, True, False),
    ("cartpole", 64, 3, "nx+2", False, False, False, True, True, True, False),
    ("cartpole", 65, 1, "1", True, True, True, False, False, False, True),
    ("cartpole", 1, 3, "nx", False, False, False, False, False, True, True),
    ("unicycle", 65, 3, "nx", False, False, True, True, False, True, True),
    ("unicycle", 64, 1, "nx+2", False, False, False, False, True, False, False),
    ("unicycle", 1, 3, "1", False, True, True, False, False, False, True),
    ("lti", 65, 3, "1", False, False, False, False, False, True, True),
    ("lti", 1, 3, "nx+2", False, False, True, True, False, True, False),
    ("lti", 64, 1, "nx", False, True, False, False, True, False, False),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:4]) + "".join("1" if x else "0" for x in c[4:]))
def test_run_and_the_step_loop_are_the_restatement(api, case, tmp_path):
    name, B, T, nyk, per_params, per_sensor, per_P0, device, diag, have_w, have_wu = case
    nx = PLANTS[name][3]
    ny = {"1": 1, "nx": nx, "nx+2": nx + 2}[nyk]
    plant, model = make(api, name, B, per_params, seed=B + T, tmp_path=tmp_path)
    d = draw(name, B, T, ny, per_sensor, per_P0, have_w, have_wu, 20261050 + 16 * B + T + 100 * nx + ny)
    ref = PE.Filter(model, B, d["C"], d["v"], d["W"], d["Wu"])
    ref.reset(d["xh0"], d["P0"])
    want = ref.run(d["Y"], d["U"], diag=diag)
    assert not want["info"].any() and np.all(np.isfinite(want["Xh"])) and np.all(want["nis"] >= 0.0)
    wrap = dev if device else (lambda a: a)
    ekf = api.DeviceEkf(plant, d["C"], d["v"], d["W"], d["Wu"])
    # 1. one launch
    ekf.reset(wrap(d["xh0"]), wrap(d["P0"]))
    got = ekf.run(wrap(d["Y"]), wrap(d["U"]), diag=diag)
    for k in ("Xh", "P", "nis", "info"):
        assert PE.same(host(got[k]), want[k]), (case, k, int(np.sum(host(got[k]) != want[k])))
    xh, P, info = ekf.get(device=device)
    assert PE.same(host(xh), ref.xh) and PE.same(host(P), ref.P) and not host(info).any()       # left at the final posterior
    # 2. the loop over the step entries, from a fresh reset
    ekf.reset(wrap(d["xh0"]), wrap(d["P0"]))
    full = ref.P.shape
    ref.reset(d["xh0"], d["P0"])
    wantf = ref.run(d["Y"], d["U"])
    for t in range(T + 1):
        if t > 0:
            ekf.predict(wrap(d["U"][:, t - 1]))
        nis = ekf.update(wrap(d["Y"][:, t]))
        xh, P, info = ekf.get(device=device)
        assert PE.same(host(nis), wantf["nis"][:, t]) and PE.same(host(xh), wantf["Xh"][:, t]) and PE.same(host(P), wantf["P"][:, t]), (case, t)
    assert host(P).shape == full
    # 3. a second run continues from the object's state: the two halves of a log are the whole log
    if T == 3:
        ekf.reset(wrap(d["xh0"]), wrap(d["P0"]))
        a = ekf.run(wrap(d["Y"][:, :2]), wrap(d["U"][:, :1]))
        ekf.predict(wrap(d["U"][:, 1]))
        b = ekf.run(wrap(d["Y"][:, 2:]), wrap(d["U"][:, 2:]))
        assert PE.same(np.concatenate([host(a["Xh"]), host(b["Xh"])], axis=1), wantf["Xh"])
        assert PE.same(np.concatenate([host(a["P"]), host(b["P"])], axis=1), wantf["P"])
    ekf.close(); plant.close()


def test_nan_is_a_dropout_with_the_flag(api, tmp_path):
    name, B, T, ny = "cartpole", 65, 3, 4
    plant, model = make(api, name, B, tmp_path=tmp_path)
    d = draw(name, B, T, ny, False, False, True, True, 20261060)
    Y = d["Y"].copy()
    Y[3, 1, 2] = np.nan; Y[64, 0, :] = np.nan; Y[10, 3, 0] = np.nan
    ref = PE.Filter(model, B, d["C"], d["v"], d["W"], d["Wu"])
    ref.reset(d["xh0"], d["P0"])
    want = ref.run(Y, d["U"], skip_nan=True)
    assert not want["info"].any() and np.all(np.isfinite(want["Xh"])) and want["nis"][64, 0] == 0.0
    ekf = api.DeviceEkf(plant, d["C"], d["v"], d["W"], d["Wu"])
    ekf.reset(d["xh0"], d["P0"])
    got = ekf.run(Y, d["U"], skip_nan=True)
    for k in ("Xh", "P", "nis", "info"):
        assert PE.same(got[k], want[k]), k
    # the trajectories without a missing row are what they are on the full log
    ekf.reset(d["xh0"], d["P0"])
    full = ekf.run(d["Y"], d["U"])
    keep = np.ones(B, dtype=bool); keep[[3, 64, 10]] = False
    assert PE.same(full["Xh"][keep], got["Xh"][keep]) and not PE.same(full["Xh"][3], got["Xh"][3])
    # without the flag a host NaN is refused, and the object is untouched
    before = ekf.get()
    with pytest.raises(api.HipError, match="only with CDDP_HIP_EKF_SKIP_NAN"):
        ekf.run(Y, d["U"])
    with pytest.raises(api.HipError, match="only with CDDP_HIP_EKF_SKIP_NAN"):
        ekf.update(Y[:, 0])
    assert all(PE.same(a, b) for a, b in zip(before, ekf.get()))
    ekf.close(); plant.close()


def test_failing_pivot_of_one_trajectory(api, tmp_path):
    name, B, T, ny = "unicycle", 65, 3, 3
    plant, model = make(api, name, B, tmp_path=tmp_path)
    d = draw(name, B, T, ny, True, True, True, True, 20261070)
    ekf = api.DeviceEkf(plant, d["C"], d["v"], d["W"], d["Wu"])
    ekf.reset(d["xh0"], d["P0"])
    good = ekf.run(d["Y"], d["U"])
    assert not good["info"].any()
    # trajectory 40: a prior of -I with a small v fails its first row at once; trajectory 7: fine at step 0 and 1, its v turns the pivot
    # negative only when W = -I has entered P, at step 1 + 1
    P0 = d["P0"].copy(); v = d["v"].copy(); W = d["W"].copy()
    P0[40] = -np.eye(3); v[40] = 1e-3
    W[7] = -4.0 * np.eye(3)
    ref = PE.Filter(model, B, d["C"], v, W, d["Wu"])
    ref.reset(d["xh0"], P0)
    want = ref.run(d["Y"], d["U"])
    assert want["info"][40] == 1 and want["info"][7] >= 2 and int(np.count_nonzero(want["info"])) == 2
    bad_ekf = api.DeviceEkf(plant, d["C"], v, W, d["Wu"])
    bad_ekf.reset(d["xh0"], P0)
    bad = bad_ekf.run(d["Y"], d["U"])
    for k in ("Xh", "P", "nis", "info"):
        assert PE.same(bad[k], want[k]), k
    t7 = int(want["info"][7]) - 1
    assert np.all(np.isnan(bad["Xh"][40])) and np.all(np.isfinite(bad["Xh"][7, :t7])) and np.all(np.isnan(bad["Xh"][7, t7:])) and np.all(np.isnan(bad["nis"][7, t7:]))
    keep = np.ones(B, dtype=bool); keep[[7, 40]] = False
    for k in ("Xh", "P", "nis"):
        assert PE.same(bad[k][keep], good[k][keep]), k                     # the neighbours are bitwise unchanged
    xh, P, info = bad_ekf.get()
    assert np.all(np.isnan(xh[40])) and np.all(np.isnan(P[7])) and PE.same(info, want["info"])
    # the step entries agree, and the dead trajectory stays dead
    bad_ekf.reset(d["xh0"], P0)
    for t in range(T + 1):
        if t > 0:
            bad_ekf.predict(d["U"][:, t - 1])
        nis = bad_ekf.update(d["Y"][:, t])
        assert PE.same(nis, want["nis"][:, t]) and PE.same(bad_ekf.get()[0], want["Xh"][:, t]), t
    assert PE.same(bad_ekf.get()[2], want["info"])
    ekf.close(); bad_ekf.close(); plant.close()


def test_refusals_that_need_a_plant(api, tmp_path):
    B = 3
    plant, _ = make(api, "cartpole", B, tmp_path=tmp_path)
    C0 = np.ones((2, 4)); v0 = np.array([0.1, 0.2])
    for kw, msg in ((dict(v=np.array([0.1, 0.0])), "v holds an entry that is not finite and > 0"), (dict(v=np.array([np.inf, 0.1])), "v holds an entry"),
                    (dict(C_=np.full((2, 4), np.nan)), "C holds a non-finite value"), (dict(W=np.full((4, 4), np.inf)), "W holds a non-finite value"),
                    (dict(Wu=np.full((1, 1), np.nan)), "Wu holds a non-finite value")):
        args = dict(C_=C0, v=v0); args.update(kw)
        with pytest.raises(api.HipError, match=msg):
            api.DeviceEkf(plant, **args)
    mid, integ, dt, nx, nu, params, _ = PLANTS["cartpole"]
    sub = api.DevicePlant(getattr(api, mid), getattr(api, integ), dt, nx, nu, B, params=params, substeps=2)
    with pytest.raises(api.HipError, match="takes 2 substeps per control interval"):
        api.DeviceEkf(sub, C0, v0)
    sub.close()
    ekf = api.DeviceEkf(plant, C0, v0)
    ekf.reset(np.zeros((B, 4)), np.eye(4))
    before = ekf.get()
    lib = ekf.lib
    y = np.zeros((B, 2)); nis = np.zeros(B)
    assert lib.cddp_hip_ekf_update(ekf.h, 64, y.ctypes.data, nis.ctypes.data) == -2 and b"unknown flag bits 0x40" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_ekf_update(ekf.h, 0, None, None) == -1 and b"null y pointer" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_ekf_run(ekf.h, 0, -1, y.ctypes.data, None, None, None, None, None) == -1 and b"T must not be negative" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_ekf_run(ekf.h, 0, 2, y.ctypes.data, None, None, None, None, None) == -1 and b"null U pointer" in lib.cddp_hip_last_error()
    with pytest.raises(api.HipError, match="u holds a non-finite value"):
        ekf.predict(np.full((B, 1), np.nan))
    with pytest.raises(api.HipError, match="P0 holds a non-finite value"):
        ekf.reset(np.zeros((B, 4)), np.full((4, 4), np.nan))
    # device form: a host address is refused
    assert lib.cddp_hip_ekf_update(ekf.h, api.EKF_DEVICE, y.ctypes.data, None) == -2 and b"y is not device memory" in lib.cddp_hip_last_error()
    assert all(PE.same(a, b) for a, b in zip(before, ekf.get()))
    ekf.close(); plant.close()
