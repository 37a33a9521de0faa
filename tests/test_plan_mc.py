"""Monte-Carlo closed-loop evaluation of a solved plan under noise (cddp_hip_mc_sample_noise, cddp_hip_plan_montecarlo; csrc/inst_mc.hip,
csrc/plan_mc.hpp).

The header fixes the arithmetic, so every check but one is BITWISE (np.array_equal with NaN = NaN; values, so -0.0 == 0.0: the library is
built with -fno-signed-zeros).  References: the host program over plan_mc.hpp (the noise), cddp_hip_score_rollouts fed that noise (the
per-sample outputs without process noise), a loop over DevicePlant.step with the feedback line in numpy (all three noises), and a numpy
restatement of the tree sum applied to the per-sample outputs of the same call (every reduction).  The one toleranced test holds the
sample moments of an LTI loop against cddp_hip_plan_covariance inside 6 standard errors, at the seed tests/test_plan_mc_cpu.py has shown to
pass on the host."""
import ctypes as C

import numpy as np
import pytest

import plan_mc_ref as R
from plan_mc_ref import SEED
from test_plan_sens import solved
from test_score_rollouts import case as score_case, dev, objective_numpy, same, same_record, same_snapshot, snapshot, solve_record, viol_reference

pytestmark = pytest.mark.gpu

REDUCED = ("stats", "nviol_step", "dXmean", "SX", "dUmean", "SU")
PER_SAMPLE = ("cost", "viol", "X", "U")


def torch_():
    import torch
    return torch


def cov_of(L):
    return None if L is None else L @ L.T


def mc(h, L0, Lw, Lu, S, **kw):
    return h.plan_montecarlo(L0, Lw, Lu, nsamp=S, factors=True, **kw)


def plan_of(h):
    Xp, Up = h.trajectory()
    K = h.gains()[0].reshape(h.B, h.p.N, h.p.nu, h.p.nx)
    return Xp, Up, K


def cartpole_handle(api, B, N=5, seed=20261801):
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N)
    p.options.max_iterations = 3
    return solved(api, p, B, seed, [0.1, 0.3, 0.1, 0.1])


def reduced_reference(api, h, out, S, viol_tol, diag=False):
    """every reduced output from the per-sample outputs of the same call"""
    Xp, Up, K = plan_of(h)
    ref = {}
    ref["dXmean"], ref["SX"] = R.moments(out["X"] - Xp[:, None], diag)
    ref["dUmean"], ref["SU"] = R.moments(out["U"] - Up[:, None], diag)
    ref["stats"] = R.stats(out["cost"], out["viol"], viol_tol)
    v = R.viol_steps(api, h.p, out["X"], out["U"])
    ref["nviol_step"] = (v > viol_tol).sum(axis=1).astype(np.int32)
    ref["viol"] = v.max(axis=2)
    return ref


# ---- 1. the noise is the host program's
@pytest.mark.parametrize("pair", [(2, 1), (3, 2)])
def test_noise_is_the_host_programs(api, pair, tmp_path):
    import test_plan_mc_cpu as H
    nx, nu = pair
    B, S, N = 3, 65, 3
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=N) if pair == (2, 1) else api.unicycle_problem(api.SOLVER_IPDDP, horizon=N)
    assert (p.nx, p.nu) == pair
    h = api.HipBatchSolver(p, B)
    L0, Lw, Lu = H.factors(nx, nu, 5)
    exe = H.build_exe("plain")
    for keep, stream in ((False, 0), (True, 2)):
        Z0, E, Wn = H.noise_files(exe, tmp_path, L0, Lw, Lu, 0x1234567890, stream, B, S, N, keep)
        got = h.mc_sample_noise(L0, Lw, Lu, nsamp=S, seed=0x1234567890, stream=stream, keep_nominal=keep, factors=True)
        assert same(got["Z0"], Z0) and same(got["E"], E) and same(got["Wn"], Wn), (pair, keep)
        assert np.isfinite(E).all() and (E[:, 1:] != 0).all() and (bool((E[:, 0] == 0).all()) == keep)
        d = h.mc_sample_noise(L0, Lw, Lu, nsamp=S, seed=0x1234567890, stream=stream, keep_nominal=keep, factors=True, device=True)
        assert all(d[k].is_cuda and same(d[k], got[k]) for k in got)
        # a source switched off is zero and leaves the others where they are; covariances are factored on the host
        off = h.mc_sample_noise(L0, None, Lu, nsamp=S, seed=0x1234567890, stream=stream, keep_nominal=keep, factors=True)
        assert same(off["Z0"], Z0) and same(off["E"], E) and (off["Wn"] == 0).all()
        one = h.mc_sample_noise(None, Lw, None, nsamp=S, seed=0x1234567890, stream=stream, keep_nominal=keep, factors=True, want=("Wn",))
        assert same(one["Wn"], Wn)
    Lc = np.linalg.cholesky(L0 @ L0.T)
    a = h.mc_sample_noise(L0 @ L0.T, nsamp=4, seed=3, want=("Z0",))["Z0"]
    assert same(a, h.mc_sample_noise(Lc, nsamp=4, seed=3, factors=True, want=("Z0",))["Z0"])
    h.close()


# ---- 2. per-sample outputs without process noise are score_rollouts' on the same noise
@pytest.mark.parametrize("plant", ["own", "plant"])
def test_per_sample_outputs_are_score_rollouts(api, plant):
    B, S, N = 5, 65, 5
    h = cartpole_handle(api, B, N)
    p = h.p
    dp = None
    if plant == "plant":
        rng = np.random.default_rng(3)
        params = np.tile(np.array(list(p.c.model_params)[:5]), (B, 1))
        params[:, 1] *= rng.uniform(0.8, 1.3, B)
        dp = api.DevicePlant.of_problem(p, B, params=params, substeps=2, u_lower=[-3.0], u_upper=[2.5])
    L0, Lw, Lu = R.factors(p.nx, p.nu)
    Lu = Lu * 20.0                                        # the control noise reaches the plant's box
    noise = h.mc_sample_noise(L0, None, Lu, nsamp=S, seed=SEED, stream=1, factors=True)
    Xp, Up, K = plan_of(h)
    x0 = np.ascontiguousarray(Xp[:, 0] + 0.01)            # a base state of the caller's
    for base in (None, x0):
        xb = Xp[:, 0] if base is None else base
        ref = h.score_rollouts(np.ascontiguousarray(Up[:, None] + noise["E"]), x0=np.ascontiguousarray(xb[:, None] + noise["Z0"]), plant=dp, feedback=True,
                               want=PER_SAMPLE)
        got = mc(h, L0, None, Lu, S, seed=SEED, stream=1, plant=dp, x0=base, want=PER_SAMPLE)
        for k in PER_SAMPLE:
            assert same(got[k], ref[k]), (plant, k, base is None)
    assert np.isfinite(ref["cost"]).all() and len(np.unique(ref["cost"])) == B * S
    if dp is not None:
        assert (ref["U"] == -3.0).any() or (ref["U"] == 2.5).any()
        dp.close()
    h.close()


# ---- 3. all three noises against the loop written out
def test_all_three_noises_are_the_loop_written_out(api):
    B, S = 5, 65
    p, x0, _ = score_case(api, "unicycle_box_ball", seed=13)
    p.options.max_iterations = 3
    h = solved(api, p, B, 0, x0=np.ascontiguousarray(x0[:B]))
    L0, Lw, Lu = R.factors(p.nx, p.nu, 2.0)
    noise = h.mc_sample_noise(L0, Lw, Lu, nsamp=S, seed=SEED, stream=4, factors=True)
    Xp, Up, K = plan_of(h)
    big = api.DevicePlant.of_problem(p, B * S)
    X, U = R.closed_loop(big, Xp, Up, K, Xp[:, 0], noise["Z0"], noise["E"], noise["Wn"])
    big.close()
    got = mc(h, L0, Lw, Lu, S, seed=SEED, stream=4, want=PER_SAMPLE)
    assert same(got["X"], X) and same(got["U"], U)
    assert same(got["cost"], objective_numpy(p, X, U))
    ref, lo, hi = viol_reference(api, p, X, U)
    assert same(got["viol"], ref) and lo < 0 < hi and (ref > 0).any() and (ref == 0).any()
    # process noise alone changes what the other two sources do not: the draws of the others stay where they are
    only_w = mc(h, None, Lw, None, S, seed=SEED, stream=4, want=("X",))["X"]
    big = api.DevicePlant.of_problem(p, B * S)
    Xw, _ = R.closed_loop(big, Xp, Up, K, Xp[:, 0], None, None, noise["Wn"])
    big.close()
    assert same(only_w, Xw)
    h.close()


# ---- 4. the reductions are the tree applied to the per-sample outputs of the same call
@pytest.mark.parametrize("B", [1, 64, 65])
def test_reductions_are_the_tree_sum(api, B):
    p, x0, _ = score_case(api, "unicycle_box_ball", seed=17)
    p.options.max_iterations = 2
    rng = np.random.default_rng(B)
    x0 = p.x0[None, :] + np.array([0.3, 0.3, 0.4]) * rng.uniform(-1.0, 1.0, (B, p.nx))
    h = solved(api, p, B, 0, x0=np.ascontiguousarray(x0))
    L0, Lw, Lu = R.factors(p.nx, p.nu, 2.0)
    tol = 0.01
    for S in (1, 2, 63, 64, 65, 130):
        out = mc(h, L0, Lw, Lu, S, seed=SEED, stream=S, viol_tol=tol, want=PER_SAMPLE + REDUCED)
        ref = reduced_reference(api, h, out, S, tol)
        assert same(out["viol"], ref["viol"]), (B, S)
        for k in REDUCED:
            assert same(out[k], ref[k]), (B, S, k, np.abs(np.asarray(out[k], dtype=float) - ref[k]).max())
        assert same(out["SX"], np.swapaxes(out["SX"], 2, 3)) and same(out["SU"], np.swapaxes(out["SU"], 2, 3))
        dg = mc(h, L0, Lw, Lu, S, seed=SEED, stream=S, viol_tol=tol, diag=True, want=("SX", "SU", "dXmean"))
        assert same(dg["SX"], np.diagonal(out["SX"], axis1=2, axis2=3)) and same(dg["SU"], np.diagonal(out["SU"], axis1=2, axis2=3))
        assert same(dg["dXmean"], out["dXmean"])
        if S == 1:
            assert (out["SX"] == 0).all() and (out["stats"][:, 3] == 0).all()
        if S >= 63:
            n = out["nviol_step"]
            assert (out["SX"][:, 1:, 0, 0] > 0).all() and (n > 0).any() and (n < S).any() and (out["stats"][:, 1] <= S).all()
    h.close()


# ---- 5. keep_nominal, output subsets, pointers
def test_keep_nominal_subsets_and_pointers(api):
    t = torch_()
    B, S = 5, 65
    h = cartpole_handle(api, B)
    p = h.p
    L0, Lw, Lu = R.factors(p.nx, p.nu)
    kw = dict(seed=SEED, stream=9, keep_nominal=True, viol_tol=0.0)
    allw = PER_SAMPLE + REDUCED
    full = mc(h, L0, Lw, Lu, S, want=allw, **kw)
    nominal = h.score_rollouts(None, feedback=True, want=PER_SAMPLE)
    for k in PER_SAMPLE:
        assert same(full[k][:, 0], nominal[k][:, 0]), k
    free = mc(h, L0, Lw, Lu, S, want=("cost",), seed=SEED, stream=9)
    assert not same(free["cost"][:, 0], full["cost"][:, 0]) and same(free["cost"][:, 1:], full["cost"][:, 1:])
    # every output alone, and all of them without the two large ones
    for k in allw:
        assert same(mc(h, L0, Lw, Lu, S, want=(k,), **kw)[k], full[k]), k
    small = mc(h, L0, Lw, Lu, S, want=("cost", "viol") + REDUCED, **kw)
    for k in small:
        assert same(small[k], full[k]), k
    # device pointers, with a base state; then on a user stream
    x0 = np.ascontiguousarray(h.trajectory()[0][:, 0] + 0.02)
    host = mc(h, L0, Lw, Lu, S, want=allw, x0=x0, **kw)
    d = mc(h, L0, Lw, Lu, S, want=allw, x0=dev(x0), **kw)
    for k in allw:
        assert d[k].is_cuda and same(d[k], host[k]), k
    assert d["nviol_step"].dtype == t.int32
    s = t.cuda.Stream()
    h.set_stream(s.cuda_stream)
    half = t.from_numpy(0.5 * x0).cuda()
    big = t.zeros((1024, 1024), dtype=t.float64, device="cuda")
    t.cuda.synchronize()
    with t.cuda.stream(s):
        for _ in range(4):
            big = big @ big                                # work in front of the input on the stream: an unordered read would see zeros
        xin = t.zeros_like(half)
        xin += half; xin += half
        u = mc(h, L0, Lw, Lu, S, want=allw, x0=xin, **kw)
        twice = {k: u[k] + u[k] for k in ("cost", "SX")}    # queued right behind the call
    s.synchronize()
    for k in allw:
        assert same(u[k], host[k]), ("stream", k)
    assert same(twice["cost"], 2.0 * host["cost"]) and same(twice["SX"], 2.0 * host["SX"])
    h.set_stream(0)
    h.close()


# ---- 6. two tile groups draw what one group draws
def test_two_tile_groups(api, monkeypatch):
    """B = 130 in two groups (trajectories 0..127 and 128..129) against one group: the counter carries the trajectory's index in the batch,
    the pointers are offset per group"""
    p = api.pendulum_problem(api.SOLVER_IPDDP, True, horizon=5)
    p.options.max_iterations = 3
    b, S = 130, 65
    x0 = api.batch_x0(p, b, 20261780, np.array([1.0, 1.0])); U0 = api.batch_U0(p, b)
    one = api.HipBatchSolver(p, b); one.set_initial(x0, U0); one.solve()
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    two = api.HipBatchSolver(p, b); two.set_initial(x0, U0); two.solve()
    assert two.num_groups() == 2 and one.num_groups() == 1
    L0, Lw, Lu = R.factors(p.nx, p.nu, 4.0)
    allw = PER_SAMPLE + REDUCED
    params = np.tile(np.array(list(p.c.model_params)[:4]), (b, 1)) * np.random.default_rng(1).uniform(0.9, 1.1, (b, 1))
    dp = api.DevicePlant.of_problem(p, b, params=params)
    for plant in (None, dp):
        a = mc(one, L0, Lw, Lu, S, seed=SEED, plant=plant, want=allw)
        for conv in (lambda v: v, dev):
            g = mc(two, L0, Lw, Lu, S, seed=SEED, plant=plant, x0=conv(np.ascontiguousarray(one.trajectory()[0][:, 0])), want=allw)
            for k in allw:
                assert same(g[k], a[k]), (k, plant is not None)
    n1 = one.mc_sample_noise(L0, Lw, Lu, nsamp=S, seed=SEED, factors=True)
    n2 = two.mc_sample_noise(L0, Lw, Lu, nsamp=S, seed=SEED, factors=True)
    assert all(same(n1[k], n2[k]) for k in n1) and not same(n1["E"][128], n1["E"][0])
    one.close(); two.close(); dp.close()


# ---- 7. the handle is left alone
def test_handle_state_is_untouched(api):
    p, x0, U = score_case(api, "unicycle_box_ball", seed=13)
    p.options.max_iterations = 4
    B = x0.shape[0]
    U0 = np.ascontiguousarray(U[:, 0])
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0); h.solve()
    before = snapshot(api, h)
    L0, Lw, Lu = R.factors(p.nx, p.nu)
    dp = api.DevicePlant.of_problem(p, B, substeps=2)
    mc(h, L0, Lw, Lu, 65, seed=1, want=PER_SAMPLE + REDUCED)
    mc(h, L0, Lw, Lu, 130, seed=2, plant=dp, device=True, want=REDUCED)
    h.mc_sample_noise(L0, Lw, Lu, nsamp=3, factors=True)
    assert same_snapshot(before, snapshot(api, h)) is None
    again = solve_record(h)
    twin = api.HipBatchSolver(p, B); twin.set_initial(x0, U0); twin.solve()
    assert same_record(again, solve_record(twin))
    h.close(); twin.close(); dp.close()


# ---- 8. refusals
def test_refusals(api):
    t = torch_()
    B, S = 5, 4
    h = cartpole_handle(api, B)
    p = h.p
    ref = solve_record(h)
    fresh = api.HipBatchSolver(p, B)
    import test_msipddp_device as MS
    pm = MS.make(api, "pendulum_box")[0]
    pm.options.max_iterations = 2
    ms = solved(api, pm, B, 20261801, [0.1, 0.1])
    other = api.DevicePlant.of_problem(api.pendulum_problem(), B)
    small = api.DevicePlant.of_problem(p, B + 1)
    L0, Lw, Lu = R.factors(p.nx, p.nu)
    lib = h.lib
    cost = np.full((B, S), -7.0); dcost = t.full((B, S), -7.0, dtype=t.float64, device="cuda")

    def desc(**kw):
        d, keep = h._mc_desc("test", L0, Lw, Lu, S, factors=True)
        for k, v in kw.items():
            setattr(d, k, v)
        return d, keep

    def call(hh, flags, d, plant=None, x0=None, outs=(cost,)):
        ptr = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
        args = [ptr(o) for o in outs] + [None] * (10 - len(outs))
        return lib.cddp_hip_plan_montecarlo(hh.h if hh is not None else None, plant.h if plant is not None else None, flags,
                                            C.addressof(d[0]) if d is not None else None, ptr(x0), *args)

    def refused(rc, *needles):
        msg = lib.cddp_hip_last_error().decode()
        assert rc < 0, msg
        for n in needles:
            assert n in msg, (n, msg)
        assert (cost == -7.0).all() and bool((dcost == -7.0).all())       # nothing written
        t.cuda.synchronize()
        assert float((dcost + 1.0).sum().item()) == -6.0 * B * S          # the device still works: no error is left behind
        assert same_record(solve_record(h), ref), msg

    me = "cddp_hip_plan_montecarlo"
    refused(call(None, 0, desc()), me, "null handle")
    refused(call(h, 0, None), me, "null descriptor")
    refused(call(h, 4, desc()), "unknown flag bits 0x4")
    refused(call(h, 0, desc(nsamp=0)), "nsamp = 0")
    refused(call(h, 0, desc(nsamp=1025)), "nsamp = 1025", "at most 1024")
    refused(call(h, 0, desc(viol_tol=float("nan"))), "viol_tol is NaN")
    bad = L0.copy(); bad[1, 0] = np.inf
    refused(call(h, 0, desc(L0=api._ptr(bad))), "L0[1][0]", "not finite")
    junk = Lw.copy(); junk[0, 1] = np.nan                                  # above the diagonal: not read, not refused
    assert call(h, 0, desc(Lw=api._ptr(junk))) == 0 and (cost != -7.0).all()
    cost[:] = -7.0
    refused(call(h, 0, desc(), outs=()), "every output is NULL")
    refused(call(ms, 0, desc()), "MSIPDDP")
    refused(call(fresh, 0, desc()), "needs a solved handle")
    refused(call(h, 0, desc(), plant=other), "the plant has nx = 2")
    refused(call(h, 0, desc(), plant=small), "batch of %d" % (B + 1))
    refused(call(h, api.MC_DEVICE, desc()), "cost is not device memory")
    refused(call(h, api.MC_DEVICE, desc(), x0=np.zeros((B, p.nx)), outs=(dcost,)), "x0 is not device memory")
    short = t.full((B * S - 1,), -7.0, dtype=t.float64, device="cuda")
    rc = call(h, api.MC_DEVICE, desc(), outs=(short,))
    if rc < 0:                                                             # (torch sub-allocates: a short tensor inside a larger block passes the range check)
        refused(rc, "cost needs")
    # the noise entry
    z = np.full((B, S, p.nx), -7.0)
    sn = lambda hh, flags, d, Z: lib.cddp_hip_mc_sample_noise(hh.h if hh is not None else None, flags, C.addressof(d[0]) if d is not None else None,
                                                               Z.ctypes.data if Z is not None else None, None, None)
    refused(sn(None, 0, desc(), z), "cddp_hip_mc_sample_noise", "null handle")
    refused(sn(h, 2, desc(), z), "unknown flag bits 0x2")
    refused(sn(h, 0, desc(), None), "all NULL")
    refused(sn(h, api.MC_DEVICE, desc(), z), "Z0 is not device memory")
    assert (z == -7.0).all()
    # the binding's own
    with pytest.raises(ValueError, match="nsamp"):
        h.plan_montecarlo(L0 @ L0.T, nsamp=0)
    h.close(); fresh.close(); ms.close(); other.close(); small.close()


# ---- 9. statistics: the one toleranced test
def test_statistics_against_plan_covariance(api):
    """LTI (2, 1) unconstrained, N = 20, B = 64, S = 1024, all three noises.  The gains are the same for every trajectory, so the SX_b are
    independent estimates of one Sigma_t; the yardstick is cddp_hip_plan_covariance on the same handle and stacks.  Bounds: 6 standard
    errors -- of a sample covariance sqrt((S_ii S_jj + S_ij^2) / (B (S - 1))), of a sample mean sqrt(S_ii / (B S)), of the mean cost excess
    the one computed from cost_var -- a margin over the sampling error that covers the few hundred comparisons made at one fixed seed
    (tests/cpp/test_plan_mc.cpp runs the same loop on the host with this seed)."""
    from test_plan_sens import lti_problem, lti_seed
    N, B, S = 20, 64, 1024
    p = lti_problem(api, N, 20)
    x0 = api.batch_x0(p, B, 20261811, [0.3, 0.3])
    U0, X0 = lti_seed(p, x0)
    h = api.HipBatchSolver(p, B); h.set_initial(x0, U0, X0); h.solve()
    h.backward()                                             # the stacks at the returned plan (see cddp_hip_plan_covariance, WHICH SWEEP)
    L0 = np.array([[0.05, 0.0], [0.01, 0.04]]); Lw = np.array([[0.01, 0.0], [0.002, 0.015]]); Lu = np.array([[0.05]])
    cov = h.plan_covariance(L0 @ L0.T, Lw @ Lw.T, Lu @ Lu.T)
    Sig = cov["SX"]
    assert same(Sig, np.repeat(Sig[:1], B, axis=0)) or np.abs(Sig - Sig[:1]).max() <= 1e-12 * np.abs(Sig).max()   # one Sigma_t for the batch
    Sig = Sig[0]
    out = mc(h, L0, Lw, Lu, S, seed=SEED, stream=0, keep_nominal=False, want=("SX", "dXmean", "stats", "cost"))
    nom = mc(h, L0, Lw, Lu, 1, seed=SEED, stream=0, keep_nominal=True, want=("cost",))["cost"][:, 0]
    mSX = out["SX"].mean(axis=0); mM = out["dXmean"].mean(axis=0)
    worst = worst_m = 0.0
    for t in range(N + 1):
        for i in range(2):
            bm = 6.0 * np.sqrt(Sig[t, i, i] / (B * S))
            worst_m = max(worst_m, abs(mM[t, i]) / bm)
            assert abs(mM[t, i]) <= bm, ("mean", t, i, mM[t, i], bm)
            for j in range(2):
                bound = 6.0 * np.sqrt((Sig[t, i, i] * Sig[t, j, j] + Sig[t, i, j] ** 2) / (B * (S - 1)))
                worst = max(worst, abs(mSX[t, i, j] - Sig[t, i, j]) / bound)
                assert abs(mSX[t, i, j] - Sig[t, i, j]) <= bound, ("cov", t, i, j, mSX[t, i, j], Sig[t, i, j], bound)
    excess = out["stats"][:, 2] - nom
    se = np.sqrt((out["stats"][:, 3] / S).sum()) / B          # of the mean over b of cost_mean: the trajectories are independent
    got, want = excess.mean(), cov["dcost"].mean()
    print("statistics: |mean SX - Sigma| / bound %.3f, |mean dX| / bound %.3f, cost excess %.6e vs dcost %.6e, %.3f standard errors"
          % (worst, worst_m, got, want, abs(got - want) / se))
    assert abs(got - want) <= 6.0 * se
    h.close()


# ---- 10. the facade
def test_solve_batch_mc_is_the_two_calls(api):
    """CDDP.solve_batch_mc = solve_batch_device + plan_montecarlo on a handle solved alike"""
    import os, sys, importlib.util
    name = "pycddp_amd"
    if name in sys.modules:
        pycddp = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cddp-cpp_amd", "pycddp_amd.py"))
        pycddp = importlib.util.module_from_spec(spec); sys.modules[name] = pycddp; spec.loader.exec_module(pycddp)
    from test_plan_sens import lti_problem, lti_seed
    p = lti_problem(api, 5, 5)
    b, S = 64, 65
    x0n = api.batch_x0(p, b, 20261820, [1.0, 1.0]); U0n, X0n = lti_seed(p, x0n)
    o = pycddp.CDDPOptions(); o.verbose = False; o.print_solver_header = False; o.max_iterations = 5
    sv = pycddp.CDDP(x0n[0], p.x_ref, p.N, p.dt, o)
    sv.set_dynamical_system(pycddp.LTISystem(p.lti_A, p.lti_B, p.dt, "euler"))
    sv.set_objective(pycddp.QuadraticObjective(p.Q, p.R, p.Qf, p.x_ref, [], p.dt))
    L0, Lw, Lu = R.factors(p.nx, p.nu)
    want = ("stats", "SX", "dXmean", "cost")
    out = sv.solve_batch_mc(dev(x0n), L0 @ L0.T, Lw @ Lw.T, Lu @ Lu.T, nsamp=S, seed=SEED, stream=3, keep_nominal=True, mc_want=want, U0=dev(U0n), X0=dev(X0n),
                            solver_type=pycddp.SolverType.CLDDP)
    plain = sv.solve_batch_device(dev(x0n), dev(U0n), dev(X0n), solver_type=pycddp.SolverType.CLDDP)
    assert same(out["X"], plain["X"]) and same(out["U"], plain["U"])
    h = api.HipBatchSolver(p, b); h.set_initial(x0n, U0n, X0n); h.solve()
    assert same(h.trajectory()[0], out["X"])
    ref = h.plan_montecarlo(L0 @ L0.T, Lw @ Lw.T, Lu @ Lu.T, nsamp=S, seed=SEED, stream=3, keep_nominal=True, want=want)
    for k in want:
        assert out["mc"][k].is_cuda and same(out["mc"][k], ref[k]), k
    h.close()
