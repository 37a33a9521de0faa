"""The output-feedback Monte-Carlo evaluation on every model it is compiled for (k_mcof<M, PER, NW> over PLANT_MODEL_LIST,
csrc/inst_mcof.hip): the per-sample check of tests/test_plan_mcof.py at B = 2, S = 3, N = 4, ny = 2 on every case of tests/model_cases.py.

Every model: IPDDP with the model's control box, two iterations, all four noises, on a plant with a parameter block per trajectory (where
the plant takes one) and a box of its own inside the problem's.  The per-sample states, applied controls and estimates are those of the
loop written out over DevicePlant.step with the estimator's lines of tests/plan_mcof_ref.py, the library's own noise arrays and the
stacks of field_device; the moments of the estimation error are the tree sum of them.  BITWISE throughout."""
import numpy as np
import pytest

import model_cases as MC
import plan_mc_ref as MR
from plan_mcof_ref import SEED
from test_plan_mc_every_model import noise_scale
from test_plan_mcof import design, mcof, plan_of, sensors, written_out
from test_plan_sens import solved
from test_score_rollouts import same

pytestmark = pytest.mark.gpu

B, S, N, NY = 2, 3, 4, 2


@pytest.mark.parametrize("key", MC.MODEL_KEYS)
def test_every_model_is_the_loop_written_out(api, key):
    row = MC.MODELS[MC.KEYS[key]]
    p = MC.build_row(api, row, N)
    assert p.N == N
    p.options.max_iterations = 2
    h = solved(api, p, B, 20261840, row.spread)
    lo, up = MC.control_box(api, p)
    L0, Lw, Lu = noise_scale(p, row.spread)
    Lu = Lu / 0.08 * 0.6 * (0.5 * (up - lo))[:, None]                  # wide enough for the plant's box to be met
    plo, pup = MC.plant_box(api, p)
    params = MC.plant_params(row, p, 3, b=B)
    dp = api.DevicePlant.of_problem(p, B, u_lower=plo, u_upper=pup, **({} if params is None else {"params": params}))
    Cm, v = sensors(p.nx, NY)
    sx = np.asarray(row.spread, dtype=np.float64)
    v = v * (sx[np.arange(NY) % p.nx] / 0.2) ** 2                      # measurement noise on the scale of the state it reads
    L = design(h, Cm, v, L0, Lw, Lu)
    X, U, Xh = written_out(api, h, Cm, v, L, L0, Lw, Lu, S, SEED, 7, keep=True, box=(plo, pup), params=params)
    got = mcof(h, Cm, v, L, L0, Lw, Lu, S, seed=SEED, stream=7, keep_nominal=True, plant=dp, want=("X", "U", "Xh", "dEmean", "SE"))
    assert np.isfinite(X).all() and np.isfinite(U).all() and np.isfinite(Xh).all(), key
    for k, ref in (("X", X), ("U", U), ("Xh", Xh)):
        assert same(got[k], ref), (key, k, np.abs(got[k] - ref).max())
    assert (Xh[:, 1:, 1:] != 0).any(), key
    m, c = MR.moments(got["X"] - plan_of(h)[0][:, None] - got["Xh"])
    assert same(got["dEmean"], m) and same(got["SE"], c), key
    h.close(); dp.close()


def test_the_cases_are_every_model():
    assert len(MC.MODEL_KEYS) == len(MC.plant_model_list()) == 25
