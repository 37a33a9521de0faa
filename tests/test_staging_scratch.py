"""The staging scratch one handle's host-pointer entries share (csrc/capi.hip, struct Staging): eight calls of different entries in a
row on ONE handle, their needs going up and down, so the buffer is regrown, re-carved and re-used while it is larger than the call
needs.  Every host-form result is held, BITWISE, to the device form of the same call on the same handle with the same inputs as
torch.float64 tensors -- which stages nothing.  B = 65 in two tile groups: one full tile and a group of a single trajectory, so every
group offset and the partial tile are live."""
import numpy as np
import pytest

from test_plan_sens import dev, same, solved

pytestmark = pytest.mark.gpu

B, N = 65, 8


def same_all(a, b, where):
    """two tuples or dicts of results; the device side has to be device tensors"""
    if isinstance(a, dict):
        assert set(a) == set(b), where
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(b)]
    a = a if isinstance(a, (tuple, list)) else (a,)
    b = b if isinstance(b, (tuple, list)) else (b,)
    assert len(a) == len(b) and len(a) > 0, where
    for x, y in zip(a, b):
        assert y.is_cuda and same(x, y), where
        assert np.any(np.asarray(x) != 0), where                         # the call has written something (the arrays start as zeros)


def test_eight_entries_share_one_scratch(api, monkeypatch):
    monkeypatch.setenv("CDDP_HIP_GROUPS", "2")
    p = api.cartpole_problem(api.SOLVER_IPDDP, True, horizon=N)          # nx 4, nu 1, control box
    p.options.max_iterations = 4
    h = solved(api, p, B, 20262001, [0.1, 0.3, 0.1, 0.1])
    assert h.num_groups() == 2 and (p.nx, p.nu) == (4, 1)
    nx, nu = p.nx, p.nu
    rng = np.random.default_rng(20262002)
    Xp, Up = h.trajectory()

    # 1. plan_jvp, one vector
    dx1 = np.ascontiguousarray(rng.standard_normal((B, 1, nx)))
    first = h.plan_jvp(dx1)
    same_all(first, h.plan_jvp(dev(dx1)), "1 plan_jvp nvec = 1")

    # 2. score_rollouts, three candidates, with the X and U outputs
    S = 3
    x0 = np.ascontiguousarray(Xp[:, 0] + 0.01 * rng.standard_normal((B, nx)))
    Uc = np.ascontiguousarray(Up[:, None] + 0.5 * rng.standard_normal((B, S, N, nu)))
    want = ("cost", "viol", "X", "U")
    sc = h.score_rollouts(Uc, x0=x0, want=want)
    same_all(sc, h.score_rollouts(dev(Uc), x0=dev(x0), want=want), "2 score_rollouts")

    # 3. plan_covariance, full matrices, W and Wu given
    def spd(n):
        a = rng.standard_normal((n, n))
        return np.ascontiguousarray(a @ a.T + n * np.eye(n))
    S0, W, Wu = 0.01 * spd(nx), 0.001 * spd(nx), 0.1 * spd(nu)
    same_all(h.plan_covariance(S0, W, Wu), h.plan_covariance(dev(S0), dev(W), dev(Wu)), "3 plan_covariance")

    # 4. plan_jvp, four vectors: more than the buffer holds by now
    dx4 = np.ascontiguousarray(rng.standard_normal((B, 4, nx)))
    same_all(h.plan_jvp(dx4), h.plan_jvp(dev(dx4)), "4 plan_jvp nvec = 4")

    # 5. mc_sample_noise, five samples, all three outputs
    L0, Lw, Lu = np.linalg.cholesky(S0), np.linalg.cholesky(W), np.linalg.cholesky(Wu)
    draw = dict(nsamp=5, seed=20262003, stream=1, factors=True)
    same_all(h.mc_sample_noise(L0, Lw, Lu, **draw), h.mc_sample_noise(L0, Lw, Lu, device=True, **draw), "5 mc_sample_noise")

    # 6. plan_montecarlo, five samples: the int32 block (65 * 9 counts: no multiple of 8 bytes) and two moments
    mc_want = ("cost", "stats", "nviol_step", "dXmean", "SU")
    mc_h = h.plan_montecarlo(L0, Lw, Lu, x0=x0, viol_tol=-1.0, want=mc_want, **draw)          # (viol_tol < 0: every sample counts at every step)
    same_all(mc_h, h.plan_montecarlo(L0, Lw, Lu, x0=dev(x0), viol_tol=-1.0, want=mc_want, **draw), "6 plan_montecarlo")
    assert mc_h["nviol_step"].dtype == np.int32

    # 7. seed_best with the winner: the device form first, so the seed that stays is the host form's
    wd = h.seed_best(dev(Uc), dev(sc["cost"]), dev(sc["viol"]), x0=dev(x0))
    w = h.seed_best(Uc, sc["cost"], sc["viol"], x0=x0)
    assert w.dtype == np.int32 and wd.is_cuda and same(w, wd) and (w >= 0).all() and len(set(w.tolist())) > 1

    # 8. plan_vjp, one vector: less than the buffer holds (the seed does not touch the plan's stacks)
    gX = np.ascontiguousarray(rng.standard_normal((B, 1, N + 1, nx)))
    gU = np.ascontiguousarray(rng.standard_normal((B, 1, N, nu)))
    same_all(h.plan_vjp(gX, gU), h.plan_vjp(dev(gX), dev(gU)), "8 plan_vjp")

    # the first call again
    again = h.plan_jvp(dx1)
    assert same(again[0], first[0]) and same(again[1], first[1])

    # what the host form of seed_best left behind: the seed of set_initial_device(x0, the winners' controls)
    twin = api.HipBatchSolver(p, B)
    twin.set_initial_device(dev(x0), dev(np.ascontiguousarray(Uc[np.arange(B), w])))
    h.initialize(); twin.initialize()
    for a, b in zip(h.trajectory(), twin.trajectory()):
        assert same(a, b)
    h.close(); twin.close()
