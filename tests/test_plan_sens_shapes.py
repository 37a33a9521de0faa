"""cddp_hip_plan_jvp / cddp_hip_plan_vjp on every (nx, nu) pair they are compiled for (SENS_PAIR_LIST, csrc/inst_sens.hip), one model per pair
(tests/model_cases.py::SENS_MODELS), against the numpy recursions of tests/test_plan_sens.py, BITWISE, through host and device pointers.

What the pairs reach that the cart-pole, the pendulum and the quadrotor of tests/test_plan_sens.py do not: the accessor kernels (nx^2 + 2 nx nu
> 64) with four vectors per lane -- (6,3), (7,3), (8,3), (10,3), (10,4), read through Strided with no register copy; the sub-tile-minor
layout on the pairs with nx > 8, whose wide form exists for (10,3) and (10,4) alone; the largest prefetching pair (6,2) staged through LDS,
where four vectors per lane leave room for runs of two steps only; and the three other HAVE_GX / HAVE_GU instantiations of the adjoint on a
prefetching and on an accessor pair.  B = 70 (a full tile and a ragged one), N = 4, IPDDP with the control box, two iterations, so that the
gain stack is not that of an unsolved plan: check_both_entries asserts max |A|, |B|, |K| > 0 on every handle."""
import numpy as np
import pytest

import model_cases as MC
from test_plan_sens import check_both_entries, dev, ref_vjp, same, solved, stacks, vectors

pytestmark = pytest.mark.gpu

B = MC.B
PAIRS = sorted(MC.SENS_MODELS)
CASES = [(pair, "default") for pair in PAIRS] + [(pair, "t4=0") for pair in PAIRS if pair[0] > 8]


def handle(api, pair, seed):
    p, spread = MC.sens_problem(api, pair)
    return solved(api, p, B, seed, np.asarray(spread))


@pytest.mark.parametrize("pair,layout", CASES, ids=["%dx%d-%s" % (p[0], p[1], l) for p, l in CASES])
def test_pair_bitwise(api, monkeypatch, pair, layout):
    """R = 1; R = 5 as the library chooses (one vector per lane and pass at two tiles); R = 5 with CDDP_HIP_SENS_RV=4: one full chunk of
    Dims::kWide vectors and a partial one (nx > 10: kWide = 1, the switch changes nothing and the same kernel runs again).

    nx > 8: the IPDDP handle runs the G = 16 cooperative sweep, whose A / Bm stacks are sub-tile-minor (launch.hpp: route.t4).  The library
    exposes no getter of the route, so, as tests/test_plan_sens.py::test_quadrotor_sub_tile_minor_bitwise does, the same problem also runs
    under CDDP_HIP_T4=0, which keeps the stacks wave-tiled: both maps are walked whichever is the default."""
    monkeypatch.delenv("CDDP_HIP_SENS_RV", raising=False); monkeypatch.delenv("CDDP_HIP_SENS_IO", raising=False)
    if layout == "t4=0":
        monkeypatch.setenv("CDDP_HIP_T4", "0")
    h = handle(api, pair, 20261600 + 16 * pair[0] + pair[1])
    p = h.p
    assert h.field_shape("A") == (p.N, p.nx * p.nx) and h.field_shape("B") == (p.N, p.nx * p.nu) and h.field_shape("K") == (p.N, p.nu * p.nx)
    seed = 20261700 + 16 * pair[0] + pair[1]
    check_both_entries(h, 1, seed, (pair, layout, 1))
    check_both_entries(h, 5, seed + 1, (pair, layout, 5))
    monkeypatch.setenv("CDDP_HIP_SENS_RV", "4")
    check_both_entries(h, 5, seed + 2, (pair, layout, 5, "RV=4"))
    h.close()


@pytest.mark.parametrize("pair", [(5, 2), (8, 3)], ids=["5x2-prefetch", "8x3-accessor"])
@pytest.mark.parametrize("chunks", ["default", "4"])
def test_adjoint_with_one_cotangent_or_none(api, monkeypatch, pair, chunks):
    """gX only, gU only, neither: the three other HAVE_GX / HAVE_GU instantiations, with one and with four vectors per lane"""
    monkeypatch.delenv("CDDP_HIP_SENS_IO", raising=False)
    if chunks == "4":
        monkeypatch.setenv("CDDP_HIP_SENS_RV", "4")
    else:
        monkeypatch.delenv("CDDP_HIP_SENS_RV", raising=False)
    h = handle(api, pair, 20261800 + pair[0])
    A, Bm, K = stacks(h)
    assert np.abs(A).max() > 0 and np.abs(Bm).max() > 0 and np.abs(K).max() > 0
    R = 5
    dx0, gX, gU = vectors(h, R, 20261810 + pair[0])
    rX = ref_vjp(A, Bm, K, gX, None, R); rU = ref_vjp(A, Bm, K, None, gU, R)
    assert not same(rX, rU) and np.abs(rX).max() > 0 and np.abs(rU).max() > 0
    for conv in (lambda a: a, dev):
        assert same(h.plan_vjp(conv(gX), None), rX), (pair, "gX only")
        assert same(h.plan_vjp(None, conv(gU)), rU), (pair, "gU only")
    lib = api.load_hip()
    buf = np.full((B, R, h.p.nx), 7.0)
    assert lib.cddp_hip_plan_vjp(h.h, 0, R, None, None, buf.ctypes.data) == 0      # both NULL: the zero gradient, written
    assert np.all(buf == 0.0)
    h.close()


@pytest.mark.parametrize("rv", ["default", "4"])
def test_staged_rows_on_the_largest_prefetching_pair(api, monkeypatch, rv):
    """(6,2) under CDDP_HIP_SENS_IO=staged: with four vectors per lane rv (nx + nu) = 32 > 24, so Dims::stage drops to runs of two steps
    (N = 4: two full runs); with one vector per lane the runs are of four steps (one full run).  The cart-pole of tests/test_plan_sens.py
    stays at four either way."""
    monkeypatch.setenv("CDDP_HIP_SENS_IO", "staged")
    if rv == "4":
        monkeypatch.setenv("CDDP_HIP_SENS_RV", "4")
    else:
        monkeypatch.delenv("CDDP_HIP_SENS_RV", raising=False)
    h = handle(api, (6, 2), 20261900)
    for R in (1, 5):
        check_both_entries(h, R, 20261910 + R, ("6x2 staged", rv, R))
    A, Bm, K = stacks(h)
    dx0, gX, gU = vectors(h, 4, 20261920)
    assert same(h.plan_vjp(dev(gX), None), ref_vjp(A, Bm, K, gX, None, 4))
    assert same(h.plan_vjp(None, dev(gU)), ref_vjp(A, Bm, K, None, gU, 4))
    h.close()
