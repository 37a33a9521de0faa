"""The Monte-Carlo plan evaluation on every model it is compiled for (k_mc<M, PER, NW> over PLANT_MODEL_LIST, csrc/inst_mc.hip) and on every
registered kernel set that carries a constraint.

Every model: IPDDP with the model's control box, two iterations, the horizon of tests/model_cases.py, B = 3, S = 65 (a trajectory's samples
lie in two wavefronts), all three noises with full lower-triangular factors, on a plant with a parameter block per trajectory (where the
plant takes one) and a box of its own inside the problem's.  The per-sample states and applied controls are those of the loop written out:
DevicePlant.step of a plant of batch B * S, the feedback line and the clip in numpy with ascending loops.
Every constrained set: viol and nviol_step against the rows of tests/test_score_rollouts.py folded per step.  BITWISE throughout."""
import numpy as np
import pytest

import model_cases as MC
import plan_mc_ref as R
from plan_mc_ref import SEED
from test_plan_sens import solved
from test_score_rollouts import same, viol_reference

pytestmark = pytest.mark.gpu

B, S = 3, 65


def plan_of(h):
    Xp, Up = h.trajectory()
    return Xp, Up, h.gains()[0].reshape(h.B, h.p.N, h.p.nu, h.p.nx)


def noise_scale(p, spread):
    """factors scaled to the model: a tenth of the x0 spread of its row for the states, a twentieth of the box half-width for the controls"""
    L0, Lw, Lu = R.factors(p.nx, p.nu)
    sx = np.asarray(spread, dtype=np.float64)
    return L0 / 0.05 * 0.1 * sx[:, None], Lw / 0.01 * 0.02 * sx[:, None], Lu


@pytest.mark.parametrize("key", MC.MODEL_KEYS)
def test_every_model_is_the_loop_written_out(api, key):
    row = MC.MODELS[MC.KEYS[key]]
    p = MC.build_row(api, row)
    assert p.N == MC.horizon(p.nx)
    p.options.max_iterations = 2
    h = solved(api, p, B, 20261840, row.spread)
    lo, up = MC.control_box(api, p)
    L0, Lw, Lu = noise_scale(p, row.spread)
    Lu = Lu / 0.08 * 0.6 * (0.5 * (up - lo))[:, None]                  # wide enough for the plant's box to be met on every model
    plo, pup = MC.plant_box(api, p)
    params = MC.plant_params(row, p, 3, b=B)
    kw = {} if params is None else {"params": params}
    dp = api.DevicePlant.of_problem(p, B, u_lower=plo, u_upper=pup, **kw)
    assert bool(dp.desc.params_per_trajectory) == row.per_traj
    big = api.DevicePlant.of_problem(p, B * S, **({} if params is None else {"params": np.repeat(params, S, axis=0)}))
    noise = h.mc_sample_noise(L0, Lw, Lu, nsamp=S, seed=SEED, stream=7, keep_nominal=True, factors=True)
    Xp, Up, K = plan_of(h)
    X, U = R.closed_loop(big, Xp, Up, K, Xp[:, 0], noise["Z0"], noise["E"], noise["Wn"], box=(plo, pup))
    got = h.plan_montecarlo(L0, Lw, Lu, nsamp=S, seed=SEED, stream=7, keep_nominal=True, factors=True, plant=dp, want=("X", "U", "dXmean", "SX", "SU"))
    assert np.isfinite(X).all() and np.isfinite(U).all(), key
    assert same(got["X"], X), (key, np.abs(got["X"] - X).max())
    assert same(got["U"], U), (key, np.abs(got["U"] - U).max())
    assert ((U == plo) | (U == pup)).any() and ((U > plo) & (U < pup)).any(), key          # the plant's box is met and is not everything
    m, c = R.moments(got["X"] - Xp[:, None])
    assert same(got["dXmean"], m) and same(got["SX"], c), key
    assert same(got["SU"], R.moments(got["U"] - Up[:, None])[1]), key
    h.close(); dp.close(); big.close()


@pytest.mark.parametrize("name", MC.SET_NAMES)
def test_every_constrained_set(api, name):
    p, x0, _ = MC.set_case(api, name)
    p.options.max_iterations = 2
    h = solved(api, p, B, 0, x0=np.ascontiguousarray(x0[:B]))
    assert MC.set_of(api, p) == name
    spread = np.abs(x0 - p.x0[None, :]).max(axis=0) + 1e-3
    L0, Lw, Lu = noise_scale(p, spread)
    Lu = Lu * 5.0
    tol = 1e-3
    got = h.plan_montecarlo(L0 * 3.0, Lw * 3.0, Lu, nsamp=S, seed=SEED, stream=8, factors=True, viol_tol=tol, want=("viol", "nviol_step", "X", "U", "stats"))
    ref, lo_, hi_ = viol_reference(api, p, got["X"], got["U"])
    assert np.isfinite(got["X"]).all(), name
    assert same(got["viol"], ref), (name, np.abs(got["viol"] - ref).max())
    v = R.viol_steps(api, p, got["X"], got["U"])
    assert same(v.max(axis=2), ref)
    assert same(got["nviol_step"], (v > tol).sum(axis=1).astype(np.int32)), name
    assert same(got["stats"][:, 1], (ref > tol).sum(axis=1).astype(np.float64)), name
    print(name, "rows in [%g, %g]; samples over the tolerance per step: %s" % (lo_, hi_, got["nviol_step"].sum(axis=0).tolist()))
    assert lo_ < 0, name
    h.close()


def test_the_cases_are_every_model_and_set():
    assert len(MC.MODEL_KEYS) == len(MC.plant_model_list()) == 25
    assert set(MC.SET_NAMES) >= {"unicycle/ctrlbox+ball", "lti1x1/ctrlbox+terminal", "manip7/ctrlbox+terminal"}
