"""cddp_hip_plan_kalman on every (nx, nu) pair it is compiled for (KF_PAIR_LIST of csrc/inst_kf.hip = SENS_PAIR_LIST), one model per pair
(tests/model_cases.py::SENS_MODELS), against tests/plan_kf_ref.py, BITWISE: ny = max(1, nx // 2) per trajectory through host pointers,
ny = nx + 2 shared through device pointers, every output, info == 0 and all outputs finite.

What the pairs reach that the cart-pole, the unicycle and the pendulum of tests/test_plan_kf.py do not: one owner per wavefront up to
nx = 8 and two from nx = 10 on (32 trajectories per workgroup, the last wavefront half empty at nx = 13); the product buffer that is
larger than nx x nx at (1, 1); the 150.5 KB of LDS of (14, 7); and the sub-tile-minor layout of the A / Bm stacks on the pairs with
nx > 8.  B = 70 (a full tile and a ragged one), N = 4, IPDDP with the control box, two iterations."""
import numpy as np
import pytest

import model_cases as MC
from test_plan_kf import ALL, check, inputs
from test_plan_sens import solved

pytestmark = pytest.mark.gpu

B = MC.B
PAIRS = sorted(MC.SENS_MODELS)
CASES = [(pair, "default") for pair in PAIRS] + [(pair, "t4=0") for pair in PAIRS if pair[0] > 8]


@pytest.mark.parametrize("pair,layout", CASES, ids=["%dx%d-%s" % (p[0], p[1], l) for p, l in CASES])
def test_pair_bitwise(api, monkeypatch, pair, layout):
    """nx > 8: the IPDDP handle runs the G = 16 cooperative sweep, whose A / Bm stacks are sub-tile-minor (launch.hpp: route.t4).  The
    library exposes no getter of the route, so, as tests/test_plan_cov_shapes.py does, the same problem also runs under CDDP_HIP_T4=0,
    which keeps the stacks wave-tiled: both maps are walked whichever is the default."""
    if layout == "t4=0":
        monkeypatch.setenv("CDDP_HIP_T4", "0")
    p, spread = MC.sens_problem(api, pair)
    h = solved(api, p, B, 20262900 + 16 * pair[0] + pair[1], np.asarray(spread))
    assert h.field_shape("A") == (p.N, p.nx * p.nx) and h.field_shape("B") == (p.N, p.nx * p.nu) and h.field_shape("K") == (p.N, p.nu * p.nx)
    seed = 20263100 + 16 * pair[0] + pair[1]
    r = check(h, inputs(p, max(1, p.nx // 2), seed, True, B), (pair, layout, "per-trajectory"), kinds=("host",))
    assert np.all(r["info"] == 0) and all(np.all(np.isfinite(r[k])) for k in ALL) and np.abs(r["L"]).max() > 0
    r = check(h, inputs(p, p.nx + 2, seed + 1, False, B), (pair, layout, "shared"), kinds=("device",))
    assert np.all(r["info"] == 0) and all(np.all(np.isfinite(r[k])) for k in ALL)
    h.close()
