"""Sampling-based plan refinement on every model it is compiled for (k_mppi_score<M, PER> over PLANT_MODEL_LIST, csrc/inst_mppi.hip) and at odd
nu: k_mppi_score carries the odd Box-Muller normal across the step boundary there, and draw_pair / k_mppi_blend index sigma and the box by
e % nu -- with nu in {1, 2, 4} and a scalar sigma (tests/test_mppi.py) an index that is wrong only where nu does not divide 2 passes.

Here sigma and the box are vectors with a distinct ratio per control (tests/model_cases.py: 0.75 of the half-width times 1 + 0.25 i), the
box follows test_mppi.setup's rule (centre - 0.8 sigma, centre + 1.1 sigma), and B, S, N are those of tests/test_score_every_model.py.
That box overhangs the problem's control box on the controls with the larger ratios, so viol_tol is set to the overhang: a candidate the
sampling box admits is not made inadmissible by the control-box rows alone, and trajectories keep two or more admissible candidates.
lambda is the median over the batch of the spread of the candidates' costs on the host rollout.  Every comparison is BITWISE."""
import numpy as np
import pytest

import model_cases as MC
import test_mppi as TM
from test_mppi import SEED, boxkw, host_blend, host_controls, refine_written_out
from test_score_rollouts import dev, objective_numpy, same

pytestmark = pytest.mark.gpu

B, S = MC.B, MC.S
ODD = {3: "hcw", 7: "manip7"}
REFINE_KEYS = [k for k in MC.MODEL_KEYS if k not in ("pendulum", "cartpole", "unicycle", "quad12")]      # those four: test_mppi.PLANTS
PLANT_KEYS = ("hcw", "manip7", "quaternion_attitude")      # nu = 3, nu = 7, and one of ids 11-23 (an inertia and its inverse per trajectory)


def setup(api, key, N=None, seed=7):
    """-> problem, x0, mean (B, N, nu), sigma (nu,), box, viol_tol, lambda"""
    p, x0, U, centre, sigma = MC.model_case(api, key, seed=seed, N=N)
    mean = np.ascontiguousarray(U[:, 0])                                           # the tame candidate: a quarter of the scale
    box = (np.ascontiguousarray(centre - 0.8 * sigma), np.ascontiguousarray(centre + 1.1 * sigma))
    lo, up = MC.control_box(api, p)
    assert all(c.scale == 1.0 for c in p._cons)
    tol = float(max(0.0, (box[1] - up).max(), (lo - box[0]).max()))                # the rows of a control at the sampling box's edge, as the header forms them
    cost = objective_numpy(p, MC.rollout_host(api, p, x0, U), U)
    lam = float(max(np.median(cost.max(axis=1) - cost.min(axis=1)), 1e-6))
    return p, x0, mean, sigma, box, tol, lam


def distinct(v):
    return len(set(np.round(v, 12).tolist())) == len(v)


# ---- 1. the candidates at odd nu are the host program's
@pytest.mark.parametrize("nu", sorted(ODD))
def test_sample_controls_is_the_host_programs(api, nu, tmp_path):
    """N = 5 on both models (the 7-link arm too): N * nu is odd, a pair straddles every step boundary and the last pair is half used"""
    p, x0, mean, sigma, box, tol, lam = setup(api, ODD[nu], N=5)
    assert p.nu == nu and (p.N * nu) % 2 == 1
    assert distinct(sigma) and distinct(box[0]) and distinct(box[1]) and distinct(box[1] - box[0])      # no two controls share sigma or a bound
    h = api.HipBatchSolver(p, B)
    for bx, keep, stream in ((box, True, 5), (box, False, 5), (None, True, 0), (None, False, 0)):
        z, ref = host_controls(tmp_path, mean, sigma, bx, SEED, stream, 0, S, keep)
        got = h.sample_controls(sigma, S, U_mean=mean, seed=SEED, stream=stream, keep_mean=keep, **boxkw(bx))
        assert np.isfinite(ref).all()
        assert same(got, ref), (nu, bx is not None, keep, stream, np.abs(got - ref).max())
        if bx is not None:
            for i in range(nu):      # every control meets both of its own bounds and the inside
                assert (ref[..., i] == bx[0][i]).any() and (ref[..., i] == bx[1][i]).any() and ((ref[..., i] > bx[0][i]) & (ref[..., i] < bx[1][i])).any(), (nu, i)
        elif not keep:
            # the reference itself tells the controls apart: element e of a candidate is mean + sigma[e % nu] z
            assert np.array_equal(ref, mean[:, None] + sigma * z)
        gd = h.sample_controls(sigma, S, U_mean=dev(mean), seed=SEED, stream=stream, keep_mean=keep, **boxkw(bx))
        assert gd.is_cuda and same(gd, ref), (nu, "device")
    h.close()


@pytest.fixture(scope="module")
def drawn(api):
    """per odd-nu model: candidates of the library's own draw, scored by score_rollouts; computed once, shared, never modified"""
    cache = {}

    def get(nu):
        if nu not in cache:
            p, x0, mean, sigma, box, tol, lam = setup(api, ODD[nu], N=5)
            h = api.HipBatchSolver(p, B)
            U = h.sample_controls(sigma, S, U_mean=mean, seed=SEED, stream=0, **boxkw(box))
            sc = h.score_rollouts(U, x0=x0)
            h.close()
            for v in (U, sc["cost"], sc["viol"]):
                v.setflags(write=False)
            cache[nu] = (p, mean, box, tol, lam, U, sc["cost"], sc["viol"])
        return cache[nu]
    return get


@pytest.mark.parametrize("nu", sorted(ODD))
def test_blend_is_the_host_programs(api, drawn, nu, tmp_path):
    p, mean, box, tol, lam, U, cost, viol = drawn(nu)
    cost = cost.copy(); viol = viol.copy()
    cost[1, 0] = np.nan; viol[2, :] = np.inf                    # a NaN cost is inadmissible; trajectory 2 has no admissible candidate
    cost[3, :] = cost[3, 0]; viol[3, :] = 0.0                   # ties
    assert np.isfinite(np.delete(cost, 1, axis=0)).all()
    # a box of the blend's own, so narrow that the blend meets it: the clip of blend_end is indexed by e % nu too
    rng = np.random.default_rng(nu)
    narrow = (np.ascontiguousarray(mean.min(axis=(0, 1)) + rng.uniform(0.3, 0.5, nu) * np.ptp(mean, axis=(0, 1))),
              np.ascontiguousarray(mean.max(axis=(0, 1)) - rng.uniform(0.1, 0.3, nu) * np.ptp(mean, axis=(0, 1))))
    h = api.HipBatchSolver(p, B)
    for bx, t in ((box, tol), (narrow, tol), (None, 0.0)):
        w, st, ref = host_blend(tmp_path, mean, U, cost, viol, bx, lam, t)
        out, stats = h.mppi_blend(mean, U, cost, viol, lam=lam, viol_tol=t, **boxkw(bx))
        assert same(out, ref), (nu, np.abs(out - ref).max())
        assert same(stats, st), nu
        assert st[2, 0] == 0 and same(out[2], mean[2]) and st[3, 0] == S
        if bx is not None:
            assert (st[:, 0] >= 2).sum() >= B / 2 and not same(ref, mean), nu
        if bx is narrow:
            for i in range(nu):
                assert (ref[..., i] == bx[0][i]).any() and (ref[..., i] == bx[1][i]).any(), (nu, i)
        od, sd = h.mppi_blend(dev(mean), dev(np.array(U)), dev(cost), dev(viol), lam=lam, viol_tol=t, **boxkw(bx))
        assert od.is_cuda and sd.is_cuda and same(od, ref) and same(sd, st), (nu, "device")
    h.close()


# ---- 2. a refinement is the loop written out, on every model test_mppi.py does not run
def check_refine_inputs(ref, mean, where):
    """the conditions on the inputs, on the loop written out (the reference): two or more admissible candidates on at least half the
    trajectories, a blend that is not the mean, everything finite"""
    n_adm = ref["stats"][:, 0]
    print(where, "admissible candidates per trajectory: none on %d, two or more on %d of %d" % ((n_adm == 0).sum(), (n_adm >= 2).sum(), len(n_adm)))
    assert all(np.isfinite(ref[k]).all() for k in ref), where
    assert (n_adm >= 2).sum() >= len(n_adm) / 2, where
    assert not same(ref["U"], mean), where


@pytest.mark.parametrize("model", REFINE_KEYS)
def test_refine_is_the_loop_written_out(api, model):
    p, x0, mean, sigma, box, tol, lam = setup(api, model)
    assert p.nu == 1 or distinct(sigma)
    h = api.HipBatchSolver(p, B)
    kw = dict(lam=lam, viol_tol=tol, keep_mean=True, seed=SEED, stream=11)
    ref = refine_written_out(h, p, x0, mean, sigma, S, box, lam, tol, True, SEED, 11, 2)
    check_refine_inputs(ref, mean, model)
    got = h.mppi_refine(sigma, S, x0=x0, U_mean=mean, iters=2, **kw, **boxkw(box))
    for k in ref:
        assert same(got[k], ref[k]), (model, k)
    d = h.mppi_refine(sigma, S, x0=dev(x0), U_mean=dev(mean), iters=2, **kw, **boxkw(box))
    for k in ref:
        assert d[k].is_cuda and same(d[k], ref[k]), (model, k, "device")
    if model in PLANT_KEYS:
        # one round on a plant with a parameter block per trajectory, two substeps and a box of its own
        row = MC.MODELS[MC.KEYS[model]]
        plo, pup = MC.plant_box(api, p)
        dp = api.DevicePlant.of_problem(p, B, params=MC.plant_params(row, p, 3), substeps=2, u_lower=plo, u_upper=pup)
        assert dp.desc.params_per_trajectory
        ref1 = refine_written_out(h, p, x0, mean, sigma, S, box, lam, tol, True, SEED, 4, 1, plant=dp)
        check_refine_inputs(ref1, mean, model + " on a plant")
        own1 = refine_written_out(h, p, x0, mean, sigma, S, box, lam, tol, True, SEED, 4, 1)
        assert not same(ref1["cost"], own1["cost"])                                # the plant is not the model
        for conv in (lambda a: a, dev):
            got1 = h.mppi_refine(sigma, S, x0=conv(x0), U_mean=conv(mean), plant=dp, iters=1, lam=lam, viol_tol=tol, keep_mean=True, seed=SEED, stream=4,
                                 **boxkw(box))
            for k in ref1:
                assert same(got1[k], ref1[k]), (model, k, "plant")
        dp.close()
    h.close()


def test_the_refine_cases_and_test_mppis_are_every_model():
    assert len(REFINE_KEYS) == 21 and len(TM.PLANTS) == 4 and set(PLANT_KEYS) <= set(REFINE_KEYS)
