"""Every constraint struct of cddp-cpp_amd/csrc/dev_constraints.hpp on the device, one evaluation per lane (tests/hip/plant_probe.hip:
CaseCon).  Each case writes g, G_x, G_u twice -- from the ConDev / pool form and from the load + K (hoisted) form -- against a
ProblemDev of which only cons[], n_cons and pool are filled, G_x and G_u zero-filled beforehand as the call sites do.  nx = 4, nu = 3:
CtrlBox<2>, StateBox<2>, Ball<2>, Linear<2>, SecondOrderCone, ThrustMagnitude<3, true / false>, and two three-segment lists,
ConList<CtrlBox<2>, Ball<2>, ThrustMagnitude<3, true>> (the state-dependent segment in the middle) and
ConList<SecondOrderCone, CtrlBox<3>, ThrustMagnitude<3, false>> (the state-dependent segment first).  The header does not compile
for the host (Objective reads through an address-space pointer), so there is no host build: the references are the twin's classes
(oracle/twin/cddp_twin.py) and their formulas at 60 digits in mpmath.

Points: 229 per run (three wavefronts and a partial one), x ~ N(0, 0.7), u ~ N(0, 1); every 8th lane (lane 3 of each group of 8)
holds one of the case's special points: a point exactly on each bound (g == 0 exactly), the cone's apex, zero thrust.  Descriptor
variants per case carry the regularisation: eps = 0, 1e-20 and 1e-6 for the cone (regularised norm 0, 1e-10, 1e-3 at the apex: both
sides of reg_norm > 1e-9), eps = 0, 1e-6 and 4 for the thrust rows (two-sided: rn < eps false, false, true at zero thrust; one-sided:
rn > DBL_MIN false, true, true).

CPU: the twin's own float64 error against mpmath on the regular lanes is re-measured and held within a factor of the committed figures
(TWIN_ERR: g, G_x, G_u per case; bound for the device = 4 x the committed figure or the one re-measured on the GPU machine, whichever
is smaller); the special points reach both sides of every guard (counts printed) and sit exactly on
their bounds.
GPU: the two forms equal each other bit for bit; on regular lanes both are within 4 x TWIN_ERR of mpmath (a figure of 0 demands the
exact value: box and linear Jacobians, structural zeros); on every lane they match the twin in structure -- exactly zero where the
twin is zero, NaN where it is NaN (0 / 0 at zero thrust with eps = 0) -- which for the lists means every row sits at the twin's
stacked offset and every entry outside a segment's rows and columns stays zero; every segment of both lists, at every descriptor
variant, equals its single-constraint case (CtrlBox<3> included) at that offset, bit for bit.

Measured twin figures (max |value - mpmath| / max(1, |mpmath|) over the regular lanes of every variant):
  case       g          G_x        G_u
  ctrlbox      3.33e-16   0          0
  statebox     3.33e-16   0          0
  ball         3.21e-16   1.11e-16   0
  linear       2.23e-16   0          0
  soc          2.93e-16   1.91e-16   0
  soc_aligned  2.96e-16   1.84e-16   0
  thrust2      3.79e-16   0          1.70e-16
  thrust1      3.79e-16   0          1.70e-16
  list_a       3.79e-16   1.11e-16   1.70e-16
  list_b       3.79e-16   1.91e-16   1.70e-16
Reached by the special points (lanes over all variants): cone reg_norm > 1e-9 true 1519 / false 84; two-sided thrust rn < eps true 458 /
false 916; one-sided thrust rn > DBL_MIN true 1353 / false 21; g == 0 exactly on a bound 657 times; 26 NaN rows (0 / 0).
"""
import sys

import numpy as np
import pytest

import plant_probe as P

DBL_MIN = sys.float_info.min
B = P.B_SET
TWIN_ERR = {"ctrlbox": (3.34e-16, 0.0, 0.0), "statebox": (3.34e-16, 0.0, 0.0), "ball": (3.22e-16, 1.12e-16, 0.0), "linear": (2.24e-16, 0.0, 0.0),
            "soc": (2.94e-16, 1.92e-16, 0.0), "soc_aligned": (2.97e-16, 1.85e-16, 0.0), "thrust2": (3.80e-16, 0.0, 1.71e-16),
            "thrust1": (3.80e-16, 0.0, 1.71e-16), "list_a": (3.80e-16, 1.12e-16, 1.71e-16), "list_b": (3.80e-16, 1.92e-16, 1.71e-16)}

ORIGIN, AXIS, FOV = [0.125, -0.25, 0.375], [0.2, 0.3, 1.0], 0.5
BALL_C, BALL_R = [0.25, -0.5], 0.5
LIN_A, LIN_B = [[1.0, 2.0, 0.0, -1.0], [0.5, 0.0, 1.0, 0.0]], [1.0, 3.5]       # A [1, 2, 3, 4] == b exactly
T_MIN, T_MAX = 0.5, 2.0
EPS_CONE, EPS_THRUST = (0.0, 1e-20, 1e-6), (0.0, 1e-6, 4.0)


def _regular():
    rng = np.random.default_rng(20261019)
    return rng.normal(0.0, 0.7, (B, P.CON_NX)), rng.normal(0.0, 1.0, (B, P.CON_NU))


def _x(v):
    return np.array(list(v) + [0.3] * (P.CON_NX - len(v)))


U0 = np.array([0.2, -0.4, 0.1])
X0 = np.array([0.3, -0.1, 0.2, 0.4])
SP_CTRL2 = [("onbound", X0, np.array([-0.5, 1.5, 0.7])), ("onbound", X0, np.array([0.75, -1.0, -0.2]))]
SP_STATE = [("onbound", _x([-0.5, 1.5]), U0), ("onbound", _x([0.75, -1.0]), U0)]
SP_BALL = [("onbound", _x([0.75, -0.5]), U0), ("onbound", _x([0.25, -1.0]), U0), ("centre", _x(BALL_C), U0)]
SP_LIN = [("onbound", np.array([1.0, 2.0, 3.0, 4.0]), U0)]
SP_CONE = [("apex", _x(ORIGIN), U0)]
SP_THRUST = [("zero", X0, np.zeros(3)), ("onbound", X0, np.array([T_MAX, 0.0, 0.0])), ("onbound", X0, np.array([0.0, -T_MIN, 0.0]))]
SP_THRUST1 = SP_THRUST[:2]
SP_CTRL3 = [("onbound", X0, np.array([-0.5, 1.5, 0.25])), ("onbound", X0, np.array([0.75, -1.0, -2.0]))]


def _cone_axis_aligned(pool):   # cos(fov) = 1, axis e_z, eps = 0: the point (0, 0, 2) lies exactly on the cone, g == 0
    pool.soc([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 0.0, 0.0)


# case -> (entry point, [(variant name, pool builder)], special points)
def _cases():
    out = {}

    def add(name, entry, variants, special):
        out[name] = (entry, variants, special)
    add("ctrlbox", "ctrlbox", [("scale %g" % s, (lambda s: lambda p: p.ctrlbox([-0.5, -1.0], [0.75, 1.5], s))(s)) for s in (1.0, 2.5)], SP_CTRL2)
    add("statebox", "statebox", [("scale %g" % s, (lambda s: lambda p: p.statebox([-0.5, -1.0], [0.75, 1.5], s))(s)) for s in (1.0, 2.5)], SP_STATE)
    add("ball", "ball", [("scale %g" % s, (lambda s: lambda p: p.ball(BALL_R, BALL_C, s))(s)) for s in (1.0, 2.0)], SP_BALL)
    add("linear", "linear", [("rows", lambda p: p.linear(LIN_A, LIN_B))], SP_LIN)
    add("soc", "soc", [("eps %g" % e, (lambda e: lambda p: p.soc(ORIGIN, AXIS, FOV, e))(e)) for e in EPS_CONE], SP_CONE)
    add("soc_aligned", "soc", [("eps 0", _cone_axis_aligned)], [("onbound", _x([0.0, 0.0, 2.0]), U0), ("apex", _x([0.0, 0.0, 0.0]), U0)])
    add("thrust2", "thrust2", [("eps %g" % e, (lambda e: lambda p: p.thrust(T_MIN, T_MAX, e))(e)) for e in EPS_THRUST], SP_THRUST)
    add("thrust1", "thrust1", [("eps %g" % e, (lambda e: lambda p: p.thrust(None, T_MAX, e))(e)) for e in EPS_THRUST], SP_THRUST1)

    def list_a(e):
        def build(p):
            p.ctrlbox([-0.5, -1.0], [0.75, 1.5], 2.5); p.ball(BALL_R, BALL_C, 2.0); p.thrust(T_MIN, T_MAX, e)
        return build

    def list_b(ec, et):
        def build(p):
            p.soc(ORIGIN, AXIS, FOV, ec); p.ctrlbox([-0.5, -1.0, -2.0], [0.75, 1.5, 0.25], 1.0); p.thrust(None, T_MAX, et)
        return build
    add("list_a", "list_a", [("eps %g" % e, list_a(e)) for e in EPS_THRUST], SP_CTRL2 + SP_BALL + SP_THRUST)
    add("list_b", "list_b", [("eps %g / %g" % (ec, et), list_b(ec, et)) for ec, et in zip(EPS_CONE, EPS_THRUST)], SP_CONE + SP_CTRL3 + SP_THRUST1)
    return out


CASES = _cases()


def _points(case):
    """x, u, label (B,): the regular set with the case's special points on lane 3 of every group of 8, in turn."""
    x, u = _regular()
    label = np.array(["regular"] * B, dtype=object)
    sp = CASES[case][2]
    for k, i in enumerate(range(3, B, 8)):
        lb, xs, us = sp[k % len(sp)]
        x[i], u[i], label[i] = xs, us, lb
    return x, u, label


def _pool(build):
    p = P.Pool(); build(p)
    return p


def _twin_all(pool, x, u):
    g, Gx, Gu = [], [], []
    for i in range(x.shape[0]):
        a, b, c = P.twin_con(pool, x[i], u[i])
        g.append(a); Gx.append(b); Gu.append(c)
    return np.array(g), np.array(Gx), np.array(Gu)


def _errors(sets, pool, x, u, lanes):
    """worst error against mpmath of each (g, Gx, Gu) triple of arrays in sets over the given lanes (one reference per lane)"""
    e = [[0.0, 0.0, 0.0] for _ in sets]
    for i in lanes:
        ref = P.mpf_con(pool, x[i], u[i])
        for s, vals in enumerate(sets):
            for k in range(3):
                e[s][k] = max(e[s][k], P.mp_err(vals[k][i], ref[k]))
    return e


# ================================================================================ CPU
@pytest.mark.parametrize("case", list(CASES))
def test_twin_figures_on_the_regular_lanes(case):
    entry, variants, _ = CASES[case]
    x, u, label = _points(case)
    lanes = np.flatnonzero(label == "regular")
    assert lanes.size >= 200
    worst = [0.0, 0.0, 0.0]
    for vname, build in variants:
        pool = _pool(build)
        e = _errors([_twin_all(pool, x, u)], pool, x, u, lanes)[0]
        worst = [max(a, b) for a, b in zip(worst, e)]
    print("twin vs mpmath: %-12s g %.2e  Gx %.2e  Gu %.2e   (committed %s)" % ((case,) + tuple(worst) + (TWIN_ERR[case],)))
    # the committed figures describe the twin: the same up to what another machine's libm (the square roots are exact, the cone's
    # cosine is not) can move them by; an exact zero stays one.  The device's bound takes the smaller of the two (GPU test below).
    for a, b in zip(worst, TWIN_ERR[case]):
        assert (a == 0.0) == (b == 0.0) and 0.5 * b <= a <= 1.5 * b, (case, worst)


def test_special_points_reach_both_sides_of_every_guard_and_sit_on_their_bounds():
    counts = {"cone rn > 1e-9": [0, 0], "thrust2 rn < eps": [0, 0], "thrust1 rn > DBL_MIN": [0, 0], "g == 0 on a bound": 0, "NaN rows (0 / 0)": 0}
    for case, (entry, variants, _) in CASES.items():
        x, u, label = _points(case)
        for vname, build in variants:
            pool = _pool(build)
            g, Gx, Gu = _twin_all(pool, x, u)
            for tw in pool.twins:
                if isinstance(tw, P.T.SecondOrderCone):
                    rn = np.sqrt(np.sum((x[:, :3] - tw.o) ** 2, axis=1) + tw.eps)
                    counts["cone rn > 1e-9"][0] += int(np.sum(rn > 1e-9)); counts["cone rn > 1e-9"][1] += int(np.sum(~(rn > 1e-9)))
                if isinstance(tw, P.T.ThrustMagnitude):
                    rn = np.sqrt(np.sum(u * u, axis=1) + tw.eps)
                    if tw.mn is None:
                        counts["thrust1 rn > DBL_MIN"][0] += int(np.sum(rn > DBL_MIN)); counts["thrust1 rn > DBL_MIN"][1] += int(np.sum(~(rn > DBL_MIN)))
                    else:
                        counts["thrust2 rn < eps"][0] += int(np.sum(rn < tw.eps)); counts["thrust2 rn < eps"][1] += int(np.sum(~(rn < tw.eps)))
            on = np.flatnonzero(label == "onbound")
            assert (on.size or case == "soc") and np.all(np.any(g[on] == 0.0, axis=1)), (case, vname)   # every such point lies exactly on one of its bounds
            # (the general cone has no exactly representable boundary point: case soc_aligned carries it)
            counts["g == 0 on a bound"] += int(np.sum(g[on] == 0.0))
            counts["NaN rows (0 / 0)"] += int(np.sum(np.any(np.isnan(Gu), axis=2)))
            assert np.all(np.isfinite(g[label == "regular"]))
    print("reach:", counts)
    for k in ("cone rn > 1e-9", "thrust2 rn < eps", "thrust1 rn > DBL_MIN"):
        assert counts[k][0] > 0 and counts[k][1] > 0, (k, counts[k])
    assert counts["NaN rows (0 / 0)"] > 0


# ================================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_constraint_forms_on_the_device(api, case):
    G = P.device()
    entry, variants, _ = CASES[case]
    x, u, label = _points(case)
    lanes = np.flatnonzero(label == "regular")
    bad, measured = [], []
    for vname, build in variants:
        pool = _pool(build)
        A, Bf = P.run_con(G, entry, pool, x, u)
        tg, tGx, tGu = _twin_all(pool, x, u)
        for k, tw in (("g", tg), ("Gx", tGx), ("Gu", tGu)):
            if not P.same_numbers(A[k], Bf[k]):
                bad.append((case, vname, k, "the ConDev / pool form and the hoisted form differ"))
            for form, V in (("pool", A), ("hoisted", Bf)):
                d = V[k]
                if not (np.array_equal(d == 0.0, tw == 0.0) and np.array_equal(np.isnan(d), np.isnan(tw)) and np.array_equal(np.isinf(d), np.isinf(tw))):
                    at = np.argwhere((d == 0.0) != (tw == 0.0)) if not np.array_equal(d == 0.0, tw == 0.0) else np.argwhere(np.isnan(d) != np.isnan(tw))
                    bad.append((case, vname, k, form, "structure differs from the twin's", at[:4].tolist(), label[at[0][0]] if len(at) else None))
                sp = np.flatnonzero(label != "regular")
                with np.errstate(all="ignore"):
                    ok = np.isclose(d[sp], tw[sp], rtol=1e-14, atol=0.0, equal_nan=True)
                if not np.all(ok):
                    bad.append((case, vname, k, form, "special points: value off the twin's by more than 1e-14 relative", float(np.nanmax(np.abs(d[sp] - tw[sp])))))
        measured.append((vname,) + tuple(_errors([(tg, tGx, tGu)] + [(V["g"], V["Gx"], V["Gu"]) for V in (A, Bf)], pool, x, u, lanes)))
    # the twin's figure is its worst over the variants, as committed; on this machine it may be smaller, and then that holds
    here = [max(m[1][k] for m in measured) for k in range(3)]
    twin = [min(a, b) for a, b in zip(here, TWIN_ERR[case])]
    for vname, _, e_a, e_b in measured:
        for form, e in (("pool", e_a), ("hoisted", e_b)):
            print("device vs mpmath: %-12s %-14s %-8s g %.2e  Gx %.2e  Gu %.2e   (twin here %s, committed %s, bound 4 x)" % ((case, vname, form) + tuple(e) + (tuple(float("%.3g" % v) for v in here), TWIN_ERR[case])))
            for k, (a, b) in enumerate(zip(e, twin)):
                if a > 4.0 * b:
                    bad.append((case, vname, form, ("g", "Gx", "Gu")[k], "error %.3e above 4 x the twin's %.3e" % (a, b)))
    for b in bad:
        print("MISMATCH", b)
    assert not bad, bad[:4]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("list_a", "list_b"))
def test_list_rows_land_at_the_stacked_offsets(api, case):
    """Each segment of a three-constraint list alone (its own single-constraint case, the same descriptor) gives the rows the list has
    at that segment's offset, bit for bit; everything else in those columns of the list is exactly zero."""
    G = P.device()
    entry, variants, _ = CASES[case]
    x, u, _ = _points(case)
    singles = {(0, 2): "ctrlbox", (0, 3): "ctrlbox3", (2, 2): "ball", (4, 3): "soc", (5, 3): "thrust2", (6, 3): "thrust1"}   # (kind, dim)
    for vname, build in variants:
        pool = _pool(build)
        A, _ = P.run_con(G, entry, pool, x, u)
        off = 0
        for c, tw in zip(pool.cons, pool.twins):
            dual = c[2]
            one = P.Pool(); one.pool = list(pool.pool); one.cons = [list(c)]; one.cons[0][3] = 0; one.twins = [tw]; one.off = dual
            S, _ = P.run_con(G, singles[(c[0], c[1])], one, x, u)
            for k in ("g", "Gx", "Gu"):
                assert P.same_numbers(A[k][:, off:off + dual], S[k]), (case, vname, c[0], k)
            off += dual
        assert off == pool.m
