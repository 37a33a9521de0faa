"""Monte-Carlo evaluation of a solved plan with the estimator in the loop (cddp_hip_mc_sample_meas_noise, cddp_hip_plan_montecarlo_of;
csrc/inst_mcof.hip, csrc/plan_mcof.hpp).

The header fixes the arithmetic, so every check but one is BITWISE (np.array_equal with NaN = NaN; values, so -0.0 == 0.0).  References:
the host program over plan_mcof.hpp (the measurement noise), the loop written out over DevicePlant.step with the estimator's lines of
tests/plan_mcof_ref.py, the noise of mc_sample_noise / mc_sample_meas_noise and the stacks of field_device (the per-sample outputs), and
the numpy restatement of the tree sum applied to the per-sample outputs of the same call (every reduction).  The one toleranced test holds
the pooled sample moments of an LTI loop against cddp_hip_plan_kalman on the same handle inside 6 standard errors, at the seed
tests/test_plan_mcof_host.py has shown to pass on the host."""
import ctypes as C

import numpy as np
import pytest

import model_cases as MC
import plan_mc_ref as MR
import plan_mcof_ref as R
from plan_mcof_ref import SEED
from test_plan_sens import lti_problem, lti_seed, solved
from test_score_rollouts import case as score_case, dev, objective_numpy, same, same_record, same_snapshot, snapshot, solve_record, viol_reference

pytestmark = pytest.mark.gpu

MC_REDUCED = ("stats", "nviol_step", "dXmean", "SX", "dUmean", "SU")
REDUCED = MC_REDUCED + ("dEmean", "SE")
PER_SAMPLE = ("cost", "viol", "X", "U", "Xh")


def torch_():
    import torch
    return torch


def plan_of(h):
    Xp, Up = h.trajectory()
    return Xp, Up


def stacks_of(h):
    """A (B, N, nx, nx), Bm (B, N, nx, nu), K (B, N, nu, nx) as cddp_hip_get_field_device decodes them"""
    B, N, nx, nu = h.B, h.p.N, h.p.nx, h.p.nu
    f = lambda name, r, c: h.field_device(name).cpu().numpy().reshape(B, N, r, c)
    return f("A", nx, nx), f("B", nx, nu), f("K", nu, nx)


def sensors(nx, ny, scale=0.02):
    """C (ny, nx) with every entry non-zero, v (ny,) unequal variances"""
    i, j = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    Cm = np.where((i % nx) == j, 1.0, 0.2 * np.cos(1.0 + 2.0 * i + j))
    return np.ascontiguousarray(Cm), (scale * (1.0 + 0.25 * np.arange(ny))) ** 2


def design(h, Cm, v, L0, Lw, Lu):
    """the filter gains of the handle's own stacks for these sensors and noises"""
    cov = lambda L: None if L is None else L @ L.T
    kf = h.plan_kalman(Cm, v, cov(L0), cov(Lw), cov(Lu), want=("L", "info"))
    assert (kf["info"] == 0).all() and np.isfinite(kf["L"]).all()
    return kf["L"]


def mcof(h, Cm, v, L, L0, Lw, Lu, S, **kw):
    return h.plan_montecarlo_of(Cm, v, L, L0, Lw, Lu, nsamp=S, factors=True, **kw)


def written_out(api, h, Cm, v, L, L0, Lw, Lu, S, seed, stream, x0=None, keep=False, plant_kw=None, box=None, params=None):
    """the loop of the header over DevicePlant.step, with the library's own noise arrays and stacks"""
    p, B = h.p, h.B
    noise = h.mc_sample_noise(L0, Lw, Lu, nsamp=S, seed=seed, stream=stream, keep_nominal=keep, factors=True)
    Yn = h.mc_sample_meas_noise(v, nsamp=S, seed=seed, stream=stream, keep_nominal=keep)
    Xp, Up = plan_of(h)
    A, Bm, K = stacks_of(h)
    kw = dict(plant_kw or {})
    if params is not None:
        kw["params"] = np.repeat(params, S, axis=0)
    big = api.DevicePlant.of_problem(p, B * S, **kw)
    X, U, Xh = R.closed_loop(big.step, Xp, Up, K, A, Bm, Cm, L, Xp[:, 0] if x0 is None else x0, noise["Z0"] if L0 is not None else None,
                             noise["E"] if Lu is not None else None, noise["Wn"] if Lw is not None else None, Yn, box=box)
    big.close()
    return X, U, Xh


def reduced_reference(api, h, out, viol_tol, diag=False):
    """every reduced output from the per-sample outputs of the same call"""
    Xp, Up = plan_of(h)
    ref = {}
    dX = out["X"] - Xp[:, None]
    ref["dXmean"], ref["SX"] = MR.moments(dX, diag)
    ref["dUmean"], ref["SU"] = MR.moments(out["U"] - Up[:, None], diag)
    ref["dEmean"], ref["SE"] = MR.moments(dX - out["Xh"], diag)
    ref["stats"] = MR.stats(out["cost"], out["viol"], viol_tol)
    v = MR.viol_steps(api, h.p, out["X"], out["U"])
    ref["nviol_step"] = (v > viol_tol).sum(axis=1).astype(np.int32)
    ref["viol"] = v.max(axis=2)
    return ref


# ---- 1. the measurement noise is the host program's
@pytest.mark.parametrize("pair", [(2, 1), (3, 2)])
def test_meas_noise_is_the_host_programs(api, pair, tmp_path):
    import test_plan_mcof_host as H
    nx, nu = pair
    B, N = 3, 6
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=N) if pair == (2, 1) else api.unicycle_problem(api.SOLVER_IPDDP, horizon=N)
    assert (p.nx, p.nu) == pair
    h = api.HipBatchSolver(p, B)                            # (the noise needs no solve)
    exe = H.build_exe("plain")
    for ny in (1, 16):
        v = 0.01 * (1.0 + np.arange(ny))
        for S in (1, 65):
            for keep, stream in ((False, 0), (True, 2)):
                Yn = H.meas_noise_file(exe, tmp_path, v, 0x1234567890, stream, B, S, N, nx, nu, keep)
                got = h.mc_sample_meas_noise(v, nsamp=S, seed=0x1234567890, stream=stream, keep_nominal=keep)
                assert same(got, Yn), (pair, ny, S, keep)
                assert np.isfinite(Yn).all() and (Yn[:, 1:] != 0).all() and (bool((Yn[:, 0] == 0).all()) == keep)
                d = h.mc_sample_meas_noise(v, nsamp=S, seed=0x1234567890, stream=stream, keep_nominal=keep, device=True)
                assert d.is_cuda and same(d, got)
    h.close()


# ---- 2. per-sample outputs against the loop written out
def _pendulum(api, N):
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=N)
    p.options.max_iterations = 3
    return p, solved(api, p, 5, 20261801, [0.5, 0.5]), 1


def _unicycle(api, N):
    p, x0, _ = score_case(api, "unicycle_box_ball", seed=13)
    p.options.max_iterations = 3
    return p, solved(api, p, 5, 0, x0=np.ascontiguousarray(x0[:5])), 4


def _nx10(api, N):
    p, spread = MC.sens_problem(api, (10, 4))
    return p, solved(api, p, 5, 20262901, np.asarray(spread)), 3


CASES = {"pendulum": (_pendulum, None), "unicycle": (_unicycle, None), "nx10-default": (_nx10, None), "nx10-t4=0": (_nx10, {"CDDP_HIP_T4": "0"})}


@pytest.mark.parametrize("name", list(CASES))
def test_per_sample_outputs_are_the_loop_written_out(api, monkeypatch, name):
    build, env = CASES[name]
    for k, val in (env or {}).items():
        monkeypatch.setenv(k, val)                             # read at handle creation
    p, h, ny = build(api, 6)
    B, S = h.B, 65
    Cm, v = sensors(p.nx, ny)
    if name.startswith("nx10"):
        row = MC.MODELS[MC.KEYS[MC.SENS_MODELS[(10, 4)]]]
        sx = np.asarray(row.spread, dtype=np.float64)
        L0, Lw, Lu = MR.factors(p.nx, p.nu)
        L0, Lw = L0 / 0.05 * 0.1 * sx[:, None], Lw / 0.01 * 0.02 * sx[:, None]
        lo, up = MC.control_box(api, p)
        Lu = Lu / 0.08 * 0.3 * (0.5 * (up - lo))[:, None]
        plo, pup = MC.plant_box(api, p)
        v = v * (sx[np.arange(ny) % p.nx] / 0.2) ** 2
    else:
        L0, Lw, Lu = MR.factors(p.nx, p.nu, 2.0)
        Lu = Lu * 8.0                                          # the control noise reaches the plant's box
        plo, pup = (np.array([-3.0]), np.array([2.5])) if p.nu == 1 else (np.array([-0.8, -0.6]), np.array([0.9, 0.5]))
    L = design(h, Cm, v, L0, Lw, Lu)
    Xp, Up = plan_of(h)
    x0 = np.ascontiguousarray(Xp[:, 0] + 0.01)                 # a base state of the caller's, on the plant run
    # the handle's own model
    X, U, Xh = written_out(api, h, Cm, v, L, L0, Lw, Lu, S, SEED, 4)
    got = mcof(h, Cm, v, L, L0, Lw, Lu, S, seed=SEED, stream=4, want=PER_SAMPLE)
    assert np.isfinite(X).all() and np.isfinite(Xh).all(), name
    for k, ref in (("X", X), ("U", U), ("Xh", Xh)):
        assert same(got[k], ref), (name, "own", k, np.abs(got[k] - ref).max())
    assert same(got["cost"], objective_numpy(p, X, U)), name
    vref, lo_, hi_ = viol_reference(api, p, X, U)
    assert same(got["viol"], vref), name
    assert (Xh[:, :, 1:] != 0).all() and not same(Xh, X - Xp[:, None])            # an estimate, not the state
    # a plant with a box and two substeps, from a base state
    dp = api.DevicePlant.of_problem(p, B, substeps=2, u_lower=plo, u_upper=pup)
    X, U, Xh = written_out(api, h, Cm, v, L, L0, Lw, Lu, S, SEED, 5, x0=x0, plant_kw={"substeps": 2}, box=(plo, pup))
    got = mcof(h, Cm, v, L, L0, Lw, Lu, S, seed=SEED, stream=5, plant=dp, x0=x0, want=PER_SAMPLE)
    for k, ref in (("X", X), ("U", U), ("Xh", Xh)):
        assert same(got[k], ref), (name, "plant", k, np.abs(got[k] - ref).max())
    assert same(got["cost"], objective_numpy(p, X, U)) and same(got["viol"], viol_reference(api, p, X, U)[0]), name
    assert ((U == plo) | (U == pup)).any() and ((U > plo) & (U < pup)).any(), name  # the box is met and is not everything
    # common random numbers: the initial state of every sample is cddp_hip_plan_montecarlo's at the same (seed, stream)
    sf = h.plan_montecarlo(L0, Lw, Lu, nsamp=S, seed=SEED, stream=5, plant=dp, x0=x0, factors=True, want=("X",))["X"]
    assert same(got["X"][:, :, 0], sf[:, :, 0]) and not same(got["X"][:, :, 1:], sf[:, :, 1:]), name
    dp.close(); h.close()


# ---- 2b. sixteen wavefronts on the largest plant: the kernel whose static LDS (72 KB at (14, 7)) no other test launches
def test_more_than_256_samples_on_the_largest_plant(api):
    """manip7 (14, 7), S = 257: k_mcof<Manip7Model, *, 16>, five wavefronts of which the last holds one live lane.  Per-sample outputs
    against the loop written out, the reductions against the tree sum of them."""
    from test_plan_mc_every_model import noise_scale
    p, spread = MC.sens_problem(api, (14, 7))
    B, S, ny = 2, 257, 2
    h = solved(api, p, B, 20262914, np.asarray(spread))
    L0, Lw, Lu = noise_scale(p, spread)
    lo, up = MC.control_box(api, p)
    Lu = Lu / 0.08 * 0.3 * (0.5 * (up - lo))[:, None]
    Cm, v = sensors(p.nx, ny)
    sx = np.asarray(spread, dtype=np.float64)
    v = v * (sx[np.arange(ny) % p.nx] / 0.2) ** 2
    L = design(h, Cm, v, L0, Lw, Lu)
    X, U, Xh = written_out(api, h, Cm, v, L, L0, Lw, Lu, S, SEED, 11)
    got = mcof(h, Cm, v, L, L0, Lw, Lu, S, seed=SEED, stream=11, want=PER_SAMPLE + REDUCED)
    assert np.isfinite(X).all() and np.isfinite(Xh).all()
    for k, ref in (("X", X), ("U", U), ("Xh", Xh)):
        assert same(got[k], ref), (k, np.abs(got[k] - ref).max())
    ref = reduced_reference(api, h, got, 0.0)
    for k in REDUCED:
        assert same(got[k], ref[k]), (k, np.abs(np.asarray(got[k], dtype=float) - ref[k]).max())
    assert (got["SE"][:, :, 0, 0] > 0).all()
    h.close()


# ---- 3. the reductions are the tree applied to the per-sample outputs of the same call
@pytest.mark.parametrize("B", [1, 64, 65])
def test_reductions_are_the_tree_sum(api, B):
    p, x0, _ = score_case(api, "unicycle_box_ball", seed=17)
    p.options.max_iterations = 2
    rng = np.random.default_rng(B)
    x0 = p.x0[None, :] + np.array([0.3, 0.3, 0.4]) * rng.uniform(-1.0, 1.0, (B, p.nx))
    h = solved(api, p, B, 0, x0=np.ascontiguousarray(x0))
    L0, Lw, Lu = MR.factors(p.nx, p.nu, 2.0)
    Cm, v = sensors(p.nx, 2)
    L = design(h, Cm, v, L0, Lw, Lu)
    tol = 0.01
    for S in (1, 63, 65, 130):
        out = mcof(h, Cm, v, L, L0, Lw, Lu, S, seed=SEED, stream=S, viol_tol=tol, want=PER_SAMPLE + REDUCED)
        ref = reduced_reference(api, h, out, tol)
        assert same(out["viol"], ref["viol"]), (B, S)
        for k in REDUCED:
            assert same(out[k], ref[k]), (B, S, k, np.abs(np.asarray(out[k], dtype=float) - ref[k]).max())
        for k in ("SX", "SU", "SE"):
            assert same(out[k], np.swapaxes(out[k], 2, 3)), k
        dg = mcof(h, Cm, v, L, L0, Lw, Lu, S, seed=SEED, stream=S, viol_tol=tol, diag=True, want=("SX", "SU", "SE", "dEmean"))
        for k in ("SX", "SU", "SE"):
            assert same(dg[k], np.diagonal(out[k], axis1=2, axis2=3)), (k, S)
        assert same(dg["dEmean"], out["dEmean"])
        if S == 1:
            assert (out["SE"] == 0).all() and (out["SX"] == 0).all() and (out["stats"][:, 3] == 0).all()
        if S >= 63:
            n = out["nviol_step"]
            assert (out["SE"][:, :, 0, 0] > 0).all() and (n > 0).any() and (n < S).any()
    h.close()


# ---- 4. keep_nominal
def test_keep_nominal_sample_is_the_plan(api):
    p = lti_problem(api, 8, 30)
    B, S = 5, 65
    x0 = api.batch_x0(p, B, 20261811, [0.3, 0.3])
    U0, X0 = lti_seed(p, x0)
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0, X0); h.solve()
    assert (h.results()["status"] == h.results()["status"][0]).all()
    h.backward()
    c = R.LTI
    L = design(h, c["C"], c["v"], c["L0"], c["Lw"], c["Lu"])
    out = mcof(h, c["C"], c["v"], L, c["L0"], c["Lw"], c["Lu"], S, seed=SEED, stream=9, keep_nominal=True, want=("X", "U", "Xh", "dEmean"))
    dp = api.DevicePlant.of_problem(p, B)
    Xt, Ut = h.track_plan(dp)
    assert (out["Xh"][:, 0] == 0).all() and same(out["X"][:, 0], Xt) and same(out["U"][:, 0], Ut)
    assert (out["Xh"][:, 1:, 1:] != 0).all()
    free = mcof(h, c["C"], c["v"], L, c["L0"], c["Lw"], c["Lu"], S, seed=SEED, stream=9, want=("Xh",))["Xh"]
    assert (free[:, 0] != 0).any() and same(free[:, 1:], out["Xh"][:, 1:])
    dp.close(); h.close()


# ---- 5. pointers, tile groups, the handle is left alone
def test_host_and_device_pointers_agree(api):
    p, h, ny = _unicycle(api, 6)
    S = 65
    L0, Lw, Lu = MR.factors(p.nx, p.nu, 2.0)
    Cm, v = sensors(p.nx, ny)
    L = design(h, Cm, v, L0, Lw, Lu)
    allw = PER_SAMPLE + REDUCED
    x0 = np.ascontiguousarray(h.trajectory()[0][:, 0] + 0.02)
    kw = dict(seed=SEED, stream=9, keep_nominal=True, viol_tol=0.0)
    host = mcof(h, Cm, v, L, L0, Lw, Lu, S, want=allw, x0=x0, **kw)
    d = mcof(h, Cm, v, dev(L), L0, Lw, Lu, S, want=allw, x0=dev(x0), **kw)
    for k in allw:
        assert d[k].is_cuda and same(d[k], host[k]), k
    assert d["nviol_step"].dtype == torch_().int32
    for k in allw:                                         # every output alone
        assert same(mcof(h, Cm, v, L, L0, Lw, Lu, S, want=(k,), x0=x0, **kw)[k], host[k]), k
    h.close()


def test_two_tile_groups(api, monkeypatch):
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=6)
    p.options.max_iterations = 3
    b, S = 130, 65
    x0 = api.batch_x0(p, b, 20261780, np.array([1.0, 1.0])); U0 = api.batch_U0(p, b)
    one = api.HipBatchSolver(p, b); one.set_initial(x0, U0); one.solve()
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    two = api.HipBatchSolver(p, b); two.set_initial(x0, U0); two.solve()
    assert two.num_groups() == 2 and one.num_groups() == 1
    L0, Lw, Lu = MR.factors(p.nx, p.nu, 4.0)
    Cm, v = sensors(p.nx, 2)
    L = design(one, Cm, v, L0, Lw, Lu)
    assert same(L, design(two, Cm, v, L0, Lw, Lu))
    allw = PER_SAMPLE + REDUCED
    a = mcof(one, Cm, v, L, L0, Lw, Lu, S, seed=SEED, want=allw)
    for conv in (lambda x: x, dev):
        g = mcof(two, Cm, v, conv(L), L0, Lw, Lu, S, seed=SEED, x0=conv(np.ascontiguousarray(one.trajectory()[0][:, 0])), want=allw)
        for k in allw:
            assert same(g[k], a[k]), k
    n1 = one.mc_sample_meas_noise(v, nsamp=S, seed=SEED)
    assert same(n1, two.mc_sample_meas_noise(v, nsamp=S, seed=SEED)) and not same(n1[128], n1[0])
    one.close(); two.close()


@pytest.mark.parametrize("solver", ["IPDDP", "CLDDP"])
def test_handle_state_is_untouched(api, solver):
    p, x0, U = score_case(api, "unicycle_box_ball", solver=getattr(api, "SOLVER_" + solver), seed=13)
    p.options.max_iterations = 4
    B = x0.shape[0]
    U0 = np.ascontiguousarray(U[:, 0])
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0); h.solve()
    L0, Lw, Lu = MR.factors(p.nx, p.nu)
    Cm, v = sensors(p.nx, 2)
    L = design(h, Cm, v, L0, Lw, Lu)
    before = snapshot(api, h)
    dp = api.DevicePlant.of_problem(p, B, substeps=2)
    mcof(h, Cm, v, L, L0, Lw, Lu, 65, seed=1, want=PER_SAMPLE + REDUCED)
    mcof(h, Cm, v, dev(L), L0, Lw, Lu, 130, seed=2, plant=dp, want=REDUCED)
    h.mc_sample_meas_noise(v, nsamp=3)
    assert same_snapshot(before, snapshot(api, h)) is None
    again = solve_record(h)
    twin = api.HipBatchSolver(p, B); twin.set_initial(x0, U0); twin.solve()
    assert same_record(again, solve_record(twin))
    h.close(); twin.close(); dp.close()


# ---- 6. refusals
def test_refusals(api):
    t = torch_()
    B, S = 5, 4
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=5)
    p.options.max_iterations = 3
    h = solved(api, p, B, 20261801, [0.1, 0.3, 0.1, 0.1])
    ref = solve_record(h)
    fresh = api.HipBatchSolver(p, B)
    import test_msipddp_device as MS
    pm = MS.make(api, "pendulum_box")[0]
    pm.options.max_iterations = 2
    ms = solved(api, pm, B, 20261801, [0.1, 0.1])
    other = api.DevicePlant.of_problem(api.pendulum_problem(), B)
    small = api.DevicePlant.of_problem(p, B + 1)
    L0, Lw, Lu = MR.factors(p.nx, p.nu)
    ny = 2
    Cm, v = sensors(p.nx, ny)
    L = design(h, Cm, v, L0, Lw, Lu)
    Lms = np.zeros((B, pm.N + 1, pm.nx, ny)); Cms, _ = sensors(pm.nx, ny)
    lib = h.lib
    cost = np.full((B, S), -7.0); dcost = t.full((B, S), -7.0, dtype=t.float64, device="cuda")

    def desc(hh=None, Cd=Cm, vd=v, **kw):
        d, keep = (hh or h)._mcof_desc("test", Cd, vd, L0 if hh is None else None, Lw if hh is None else None, Lu if hh is None else None, S, factors=True)
        for k, val in kw.items():
            if k in ("ny", "C", "v"):
                setattr(d, k, val)
            else:
                setattr(d.mc, k, val)
        return d, keep

    ptr = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())

    def call(hh, flags, d, plant=None, x0=None, Lg=L, outs=(cost,)):
        args = [ptr(o) for o in outs] + [None] * (13 - len(outs))
        return lib.cddp_hip_plan_montecarlo_of(hh.h if hh is not None else None, plant.h if plant is not None else None, flags,
                                               C.addressof(d[0]) if d is not None else None, ptr(x0), ptr(Lg), *args)

    def refused(rc, *needles):
        msg = lib.cddp_hip_last_error().decode()
        assert rc < 0, msg
        for n in needles:
            assert n in msg, (n, msg)
        assert (cost == -7.0).all() and bool((dcost == -7.0).all())       # nothing written
        t.cuda.synchronize()
        assert float((dcost + 1.0).sum().item()) == -6.0 * B * S          # the device still works: no error is left behind
        assert call(h, 0, desc()) == 0 and (cost != -7.0).all()           # and the next call works
        cost[:] = -7.0

    me = "cddp_hip_plan_montecarlo_of"
    # everything cddp_hip_plan_montecarlo refuses
    refused(call(None, 0, desc()), me, "null handle")
    refused(call(h, 0, None), me, "null descriptor")
    refused(call(h, 4, desc()), "unknown flag bits 0x4")
    refused(call(h, 0, desc(nsamp=0)), "nsamp = 0")
    refused(call(h, 0, desc(nsamp=1025)), "nsamp = 1025", "at most 1024")
    refused(call(h, 0, desc(viol_tol=float("nan"))), "viol_tol is NaN")
    bad = L0.copy(); bad[1, 0] = np.inf
    refused(call(h, 0, desc(L0=api._ptr(bad))), "L0[1][0]", "not finite")
    refused(call(h, 0, desc(), outs=()), "every output is NULL")
    refused(call(ms, 0, desc(ms, Cms), Lg=Lms), "MSIPDDP")
    refused(call(fresh, 0, desc()), "needs a solved handle")
    refused(call(h, 0, desc(), plant=other), "the plant has nx = 2")
    refused(call(h, 0, desc(), plant=small), "batch of %d" % (B + 1))
    refused(call(h, api.MC_DEVICE, desc(), Lg=dev(L)), "cost is not device memory")
    refused(call(h, api.MC_DEVICE, desc(), Lg=dev(L), x0=np.zeros((B, p.nx)), outs=(dcost,)), "x0 is not device memory")
    # the sensor model and the gains
    refused(call(h, 0, desc(), Lg=None), me, "null L pointer")
    refused(call(h, 0, desc(C=None)), "null C pointer")
    refused(call(h, 0, desc(v=None)), "null v pointer")
    refused(call(h, 0, desc(ny=0)), "ny = 0", "1 .. 16")
    refused(call(h, 0, desc(ny=17)), "ny = 17", "1 .. 16")
    for badv in (0.0, -1.0, np.inf, np.nan):
        vb = v.copy(); vb[1] = badv
        refused(call(h, 0, desc(v=api._ptr(vb))), "v[1]", "not finite and > 0")
    Cb = Cm.copy(); Cb[1, 2] = np.nan
    refused(call(h, 0, desc(C=api._ptr(Cb))), "C holds a non-finite value")
    Lb = L.copy(); Lb[B - 1, p.N, p.nx - 1, ny - 1] = np.inf
    refused(call(h, 0, desc(), Lg=Lb), "L holds a non-finite value")
    refused(call(h, api.MC_DEVICE, desc(), Lg=L, outs=(dcost,)), "L is not device memory")
    # the noise entry
    y = np.full((B, S, p.N + 1, ny), -7.0)
    sn = lambda hh, flags, d, Y: lib.cddp_hip_mc_sample_meas_noise(hh.h if hh is not None else None, flags, C.addressof(d[0]) if d is not None else None, ptr(Y))
    me = "cddp_hip_mc_sample_meas_noise"
    refused(sn(None, 0, desc(), y), me, "null handle")
    refused(sn(h, 2, desc(), y), "unknown flag bits 0x2")
    refused(sn(h, 0, desc(), None), "Yn is NULL")
    refused(sn(h, 0, desc(ny=17), y), "ny = 17")
    refused(sn(h, 0, desc(v=None), y), "null v pointer")
    refused(sn(h, api.MC_DEVICE, desc(), y), "Yn is not device memory")
    assert (y == -7.0).all()
    assert sn(h, 0, desc(C=None), y) == 0 and (y != -7.0).all()            # the noise does not read C
    assert same_record(solve_record(h), ref)
    h.close(); fresh.close(); ms.close(); other.close(); small.close()


# ---- 7. statistics: the one toleranced test
def test_statistics_against_plan_kalman(api):
    """LTI (2, 1) unconstrained, N = 12, ny = 1 (the position), B = 64, S = 1024, all four noises: the case and the seed of
    tests/test_plan_mcof_host.py::test_statistics_on_the_cpu, which gave there, as fractions of the bounds: SE 0.503, SU 0.325, SX 0.357,
    dEmean 0.359.  The gains are the same for every trajectory, so the per-trajectory moments are independent estimates of one filter; the
    yardstick is cddp_hip_plan_kalman on the same handle and stacks.  Bounds: 6 standard errors -- of a sample covariance
    sqrt((S_ii S_jj + S_ij^2) / (B (S - 1))), of a sample mean sqrt(S_ii / (B S)).  This is the claim that the pair of calls validates an
    LQG design: the sample covariance of the estimation error on the plant is the filter's Sf_t, and the spread of states and controls
    under output feedback is the one the filter predicts."""
    c = R.LTI
    N, B, S = c["N"], c["B"], c["S"]
    p = lti_problem(api, N, 20)
    x0 = api.batch_x0(p, B, 20261811, [0.3, 0.3])
    U0, X0 = lti_seed(p, x0)
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0, X0); h.solve()
    h.backward()                                             # the stacks at the returned plan (see cddp_hip_plan_kalman, WHICH SWEEP)
    cov = lambda L: L @ L.T
    kf = h.plan_kalman(c["C"], c["v"], cov(c["L0"]), cov(c["Lw"]), cov(c["Lu"]), want=("L", "SF", "SX", "SU", "info"))
    assert (kf["info"] == 0).all()
    for k in ("SF", "SX", "SU", "L"):
        assert np.abs(kf[k] - kf[k][:1]).max() <= 1e-12 * np.abs(kf[k]).max(), k          # one filter for the batch
    out = h.plan_montecarlo_of(c["C"], c["v"], kf["L"], c["L0"], c["Lw"], c["Lu"], nsamp=S, seed=SEED, stream=0, factors=True, want=("SX", "SU", "SE", "dEmean"))
    ratios = R.statistics_ratios(out["SX"], out["SU"], out["SE"], out["dEmean"], {k: kf[k][0] for k in ("SX", "SU", "SF")}, B, S)
    print("statistics, seed %d: largest |pooled - filter| / (6 standard errors): %s" % (SEED, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)
    h.close()


# ---- 8. the facade
def test_solve_batch_lqg_mc_is_the_two_calls(api):
    """CDDP.solve_batch_lqg_mc = solve_batch_lqg + plan_montecarlo_of with the gains it returned, on a handle solved alike"""
    import os, sys, importlib.util
    name = "pycddp_amd"
    if name in sys.modules:
        pycddp = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py"))
        pycddp = importlib.util.module_from_spec(spec); sys.modules[name] = pycddp; spec.loader.exec_module(pycddp)
    p = lti_problem(api, 6, 5)
    b, S = 64, 65
    x0n = api.batch_x0(p, b, 20261820, [1.0, 1.0]); U0n, X0n = lti_seed(p, x0n)
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 5
    sv = pycddp.CDDP(x0n[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.LTISystem(p.lti_A, p.lti_B, p.dt, "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    c = R.LTI
    cov = lambda L: L @ L.T
    S0, W, Wu = cov(c["L0"]), cov(c["Lw"]), cov(c["Lu"])
    want = ("stats", "SX", "SE", "dEmean", "cost")
    out = sv.solve_batch_lqg_mc(dev(x0n), dev(c["C"]), dev(c["v"]), dev(S0), dev(W), dev(Wu), nsamp=S, seed=SEED, stream=3, keep_nominal=True, mc_want=want,
                                U0=dev(U0n), X0=dev(X0n), solver_type=pycddp.SolverType.CLDDP)
    plain = sv.solve_batch_lqg(dev(x0n), dev(c["C"]), dev(c["v"]), dev(S0), dev(W), dev(Wu), U0=dev(U0n), X0=dev(X0n), solver_type=pycddp.SolverType.CLDDP,
                               kf_want=("L", "SF", "SX", "SU", "dcost", "info"))
    assert same(out["X"], plain["X"]) and same(out["U"], plain["U"])
    for k in plain["kalman"]:
        assert same(out["kalman"][k], plain["kalman"][k]), k
    h = api.HipBatchSolver(p, b); h.set_initial(x0n, U0n, X0n); h.solve()
    L = h.plan_kalman(c["C"], c["v"], S0, W, Wu, want=("L",))["L"]
    assert same(L, out["kalman"]["L"])
    ref = h.plan_montecarlo_of(c["C"], c["v"], L, S0, W, Wu, nsamp=S, seed=SEED, stream=3, keep_nominal=True, want=want)
    for k in want:
        assert out["mc"][k].is_cuda and same(out["mc"][k], ref[k]), k
    h.close()
