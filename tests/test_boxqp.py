"""The device BoxQP of cddp-cpp_amd/csrc/dev_boxqp.hpp run by itself through the probe library (tests/hip/dev_probe.hip):
boxqp_solve<N> for N in {2, 3, 4, 7}, and the three forms of the scalar problem -- boxqp_solve<1>, its written-out trace boxqp_solve1
and boxqp_solve1_fast, whose wavefront falls back to the loop through a ballot as soon as one lane leaves the five common traces.

References: the numpy twin's boxqp() (oracle/twin/cddp_twin.py) for status, free mask and x; KKT sign conditions and a
projected-gradient brute force where the status is SUCCESS or ALL_CLAMPED.  Status, free mask and the agreement of the scalar forms
are exact.  The CPU tests run the host build of the same case bodies (boxqp_solve1_fast is device-only) and assert that the case
sets reach every status, every exit A-E of boxqp_solve1_fast and its fallback; the counts are printed."""
import json
import os

import numpy as np
import pytest

import dev_probe as P

NS = (2, 3, 4, 7)
GOLDEN = os.path.join(P.HERE, "golden", "ref_boxqp_inputs.json")


def _status(name):
    return P.BQ[name]


# ---- boxqp_solve<N> -------------------------------------------------------------------------------------------------------------
def _cases(N):
    rng = np.random.default_rng(6000 + N)
    out = []

    def add(kind, H, g, lo, up, x0, max_it=100):
        out.append(dict(kind=kind, H=np.array(H, dtype=np.float64), g=np.array(g, dtype=np.float64), lo=np.array(lo, dtype=np.float64),
                        up=np.array(up, dtype=np.float64), x0=np.array(x0, dtype=np.float64), r=rng.normal(size=N), max_it=max_it))

    def spd():
        M = rng.normal(size=(N, N))
        return M @ M.T + 0.5 * np.eye(N)

    for rep in range(6):
        H = spd(); g = rng.normal(size=N) * 3
        lo = -np.abs(rng.normal(size=N)); up = np.abs(rng.normal(size=N))
        inside = lo + (up - lo) * rng.random(N)
        on = np.where(rng.random(N) < 0.5, lo, up)
        outside = np.where(rng.random(N) < 0.5, lo - 1.0, up + 2.0)
        add("all_free", H, g, lo * 100, up * 100, inside)
        add("some_clamped", H, g, lo, up, inside)
        add("some_clamped", H, g, lo, up, on)                 # warm start on the box
        add("some_clamped", H, g, lo, up, outside)            # ... and outside it
        add("all_clamped", H, 50.0 + np.abs(g), lo, up, lo)   # held at the lower bounds by the gradient
        add("all_clamped", H, -50.0 - np.abs(g), lo * 0.01, up * 0.01, inside * 0.01)
        lo2, up2 = lo.copy(), up.copy(); j = rep % N; up2[j] = lo2[j]
        add("lo_eq_up", H, g, lo2, up2, np.clip(inside, lo2, up2))
        add("max_it_1", H, g, lo, up, inside, max_it=1)
        add("max_it_2", H, g, lo, up, outside, max_it=2)
        # a free block the LDLT rejects: zero diagonal with a non-zero entry below it
        Hb = np.eye(N); Hb[0, 0] = Hb[1, 1] = 0.0; Hb[0, 1] = Hb[1, 0] = 1.0 + rep
        add("not_pd", Hb, g, lo * 100, up * 100, inside)
        # indefinite (the LDLT accepts it), drawn until the Newton direction is no descent direction at the warm start; and a
        # negative definite one, where it never is
        while True:
            Q = P.rand_orth(rng, N)
            lam = rng.uniform(0.5, 3.0, size=N) * np.where(np.arange(N) == 0, 1.0, -1.0)
            Hi = (Q * lam) @ Q.T; Hi = 0.5 * (Hi + Hi.T)
            if P.T.boxqp(Hi, g, lo * 100, up * 100, inside, P.boxqp_options())[1] == "NO_DESCENT":
                break
        add("no_descent", Hi, g, lo * 100, up * 100, inside)
        add("no_descent", -spd(), g, lo * 100, up * 100, inside)
    return out


def _check(cases, Y, N, count=None):
    for i, c in enumerate(cases):
        status, free, x, nf, y = P.boxqp_unpack(Y, i, N)
        xt, st, ft, fac = P.T.boxqp(c["H"], c["g"], c["lo"], c["up"], c["x0"], P.boxqp_options(c["max_it"]))
        if count is not None:
            count[st] = count.get(st, 0) + 1
            count["clamped rows"] = count.get("clamped rows", 0) + int(np.sum(~ft))
            count["free rows"] = count.get("free rows", 0) + int(np.sum(ft))
            if fac is not None and fac.n < N:
                count["factor of size nf < N"] = count.get("factor of size nf < N", 0) + 1
        assert status == _status(st), (c["kind"], i, status, st)
        assert np.array_equal(free, ft.astype(int)), (c["kind"], i, free, ft)
        # x and the factor's solve are compared with the TWIN, the reference the issue names for them.  This bound is reasoned, not
        # measured as 4 x a reference's error: the twin is the only independent statement of the iteration (an mpmath BoxQP would
        # take other line-search decisions on a knife-edge and end at another iterate), so there is no third party whose error on
        # the set could be measured.  Same algorithm, same decisions (asserted above); the twin's sums go through numpy's dot
        # (other order, possibly fused), so values differ by rounding, amplified at most by the conditioning of the Newton
        # solve: 16 n eps cond(H) max(1, |x|).  (The device against the host build is asserted bit-equal, with no tolerance.)
        tol = 16 * N * P.EPS * np.linalg.cond(c["H"]) * max(1.0, np.max(np.abs(xt)))
        assert np.max(np.abs(x - xt)) <= tol, (c["kind"], i, x, xt, tol)
        assert np.all(x >= c["lo"]) and np.all(x <= c["up"])
        # the final factor of the free block, used by solving one right-hand side with it
        assert nf == (0 if fac is None else fac.n), (c["kind"], i, nf)
        if fac is not None and fac.ok and nf > 0:
            yt = fac.solve(c["r"][:nf])
            assert np.max(np.abs(y - yt)) <= 16 * N * P.EPS * np.linalg.cond(c["H"]) * max(1.0, np.max(np.abs(yt))), (c["kind"], i, y, yt)
        if st in ("SUCCESS", "ALL_CLAMPED") and c["kind"] not in ("not_pd", "no_descent"):
            grad = c["g"] + c["H"] @ x
            for j in range(N):                               # KKT sign conditions (test_oracle_pins.py::test_boxqp_against_bruteforce)
                if free[j]:
                    assert abs(grad[j]) < 1e-6, (c["kind"], i, j, grad)
                else:
                    assert (x[j] == c["lo"][j] and grad[j] > 0) or (x[j] == c["up"][j] and grad[j] < 0), (c["kind"], i, j)
            ev = np.linalg.eigvalsh(c["H"])
            if i % 4 == 0 and ev[-1] / ev[0] <= 200.0:       # projected-gradient brute force on a quarter of them: (1 - 1/200)^5000 < 1e-10
                L = ev[-1]
                z = np.clip(np.zeros(N), c["lo"], c["up"])
                for _ in range(5000):
                    z = np.clip(z - (c["g"] + c["H"] @ z) / L, c["lo"], c["up"])
                assert np.allclose(x, z, atol=1e-6), (c["kind"], i, x, z)


def test_boxqp_host_build_against_twin(tmp_path):
    lib = P.host(tmp_path)
    count = {}
    for N in NS:
        cases = _cases(N)
        _check(cases, P.run(lib, "boxqp_%d" % N, P.boxqp_pack(cases, N)), N, count)
    print("boxqp_solve<N> case set:", sorted(count.items()))
    for st in ("SUCCESS", "ALL_CLAMPED", "HESSIAN_NOT_PD", "NO_DESCENT", "MAX_ITER_EXCEEDED"):
        assert count.get(st, 0) >= 4, (st, count)
    assert count["clamped rows"] > 50 and count["free rows"] > 50 and count["factor of size nf < N"] >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
def test_boxqp_on_device(api, tmp_path, N):
    """boxqp_solve<N>: status and free mask exact against the twin, x and the final Hfree factor against the twin, KKT and brute
    force where it converged; every output bit-equal to the host build (+ - * /, comparisons and one square root)."""
    cases = _cases(N)
    X = P.boxqp_pack(cases, N)
    Y = P.run(P.device(), "boxqp_%d" % N, X)
    _check(cases, Y, N)
    assert P.same_numbers(Y, P.run(P.host(tmp_path), "boxqp_%d" % N, X))


# ---- the scalar forms -----------------------------------------------------------------------------------------------------------
def _scalar_cases():
    """H <= 0, denormal and tiny H (the gradient's square underflows), g = 0, lo = up, warm starts inside, on and outside the
    bounds, iteration caps 1, 2, 3; plus the reference-held inputs of tests/golden/ref_boxqp_inputs.json reduced to their diagonal
    scalars.  Columns: max_iterations, H, g, lo, up, x0, (unused)."""
    rng = np.random.default_rng(6001)
    rows = []
    Hs = [lambda: 10.0 ** rng.uniform(-3, 3), lambda: 10.0 ** rng.uniform(-3, 3), lambda: 10.0 ** rng.uniform(-3, 3),
          lambda: -10.0 ** rng.uniform(-3, 3), lambda: 0.0, lambda: 1e-310, lambda: -1e-310, lambda: 1e-200, lambda: 1e200, lambda: P.DBL_MIN]
    gs = [lambda: rng.normal() * 3, lambda: rng.normal() * 3, lambda: 0.0, lambda: rng.normal() * 1e-9, lambda: rng.normal() * 1e-300,
          lambda: rng.normal() * 1e200, lambda: rng.normal() * 1e3]
    for k in range(2600):
        H, g = Hs[rng.integers(len(Hs))](), gs[rng.integers(len(gs))]()
        lo = -abs(rng.normal()) * 10.0 ** rng.integers(-1, 3); up = abs(rng.normal()) * 10.0 ** rng.integers(-1, 3)
        if k % 11 == 0:
            up = lo
        w = rng.integers(6)
        x0 = [lo + (up - lo) * rng.random(), lo, up, lo - 1.0, up + 1.0, 0.0][w]
        if k % 7 == 0 and H > 0 and abs(H) > 1e-100 and abs(H) < 1e100:
            x0 = -g / H                                       # the warm start is the unconstrained minimiser (gradient ~ 0: exit B)
        if k % 4 == 1 and 1.0 < H < 1e100 and abs(g) > 1e-3 and abs(g) < 1e100:
            x0 = (-g / H) * (1.0 + 1e-6); lo, up = -1e6 - abs(x0), 1e6 + abs(x0)   # one tiny Newton step: relative improvement (exit C)
        max_it = [100, 100, 100, 100, 1, 2, 3][rng.integers(7)]
        rows.append([max_it, H, g, lo, up, x0, 0.0])
    with open(GOLDEN) as f:
        for c in json.load(f)["cases"]:
            n = c["n"]; Q = np.array(c["Q"]).reshape(n, n)
            for j in range(n):
                for x0 in (0.0, 0.5 * (c["lower"][j] + c["upper"][j]), c["upper"][j] + 1.0):
                    rows.append([100, Q[j, j], c["q"][j], c["lower"][j], c["upper"][j], x0, 0.0])
    return np.array(rows).T.copy()


def _scalar_twin(X):
    st, fr, xs = [], [], []
    with np.errstate(all="ignore"):
        for i in range(X.shape[1]):
            m, H, g, lo, up, x0 = X[:6, i]
            x, s, f, _ = P.T.boxqp(np.array([[H]]), np.array([g]), np.array([lo]), np.array([up]), np.array([x0]), P.boxqp_options(m))
            st.append(_status(s)); fr.append(int(f[0])); xs.append(x[0])
    return np.array(st, dtype=float), np.array(fr, dtype=float), np.array(xs)


def _scalar_exits(X):
    with np.errstate(all="ignore"):
        return np.array([P.boxqp1_exit(*[float(v) for v in X[1:6, i]], int(X[0, i])) for i in range(X.shape[1])])


def test_scalar_boxqp_host_build_and_reach(tmp_path):
    lib = P.host(tmp_path)
    X = _scalar_cases()
    Y1, Yg = P.run(lib, "boxqp1", X), P.run(lib, "boxqp_1", X)
    assert P.same_numbers(Y1[:3], Yg[:3]), "boxqp_solve1 and boxqp_solve<1> differ"
    st, fr, xs = _scalar_twin(X)
    assert np.array_equal(Y1[0], st) and np.array_equal(Y1[1], fr) and P.same_numbers(Y1[2], xs)   # (1 x 1 sums: nothing to reorder)
    exits = _scalar_exits(X)
    count = {k: int(np.sum(exits == k)) for k in ("A", "B", "C", "D", "E", "loop")}
    stc = {k: int(np.sum(st == v)) for k, v in P.BQ.items()}
    print("scalar BoxQP: exits of boxqp_solve1_fast", count, "statuses", stc)
    assert all(v >= 20 for v in count.values()), count
    for k in ("NO_DESCENT", "MAX_ITER_EXCEEDED", "MAX_LS_EXCEEDED", "SUCCESS", "ALL_CLAMPED"):
        assert stc[k] >= 5, stc
    # the exits are traces of the loop: a fast lane's result is what the twin gives
    fast = exits != "loop"
    assert np.all(np.isin(st[fast], [4.0, 5.0]))
    assert np.all(st[np.isin(exits, ["A", "D"])] == 5.0) and np.all(st[np.isin(exits, ["B", "C", "E"])] == 4.0)


def _orderings(X, exits):
    """The batches of the boxqp_solve1_fast test: every lane on a fast trace, none, fast and slow interleaved in every wavefront,
    exactly one slow lane in a wavefront (first, middle and last lane; and in the second wavefront only), B = 1 and B = 67."""
    F, S = np.where(exits != "loop")[0], np.where(exits == "loop")[0]
    k = min(F.size, S.size)
    inter = np.empty(2 * k, dtype=int); inter[0::2] = F[:k]; inter[1::2] = S[:k]
    out = {"all fast": F, "all slow": S, "interleaved": inter, "all cases": np.arange(X.shape[1])}
    for lane in (0, 37, 63):
        idx = F[:64].copy(); idx[lane] = S[lane]
        out["one slow lane at %d" % lane] = idx
    idx = F[:128].copy(); idx[64 + 5] = S[5]
    out["one slow lane in the second wavefront"] = idx
    out["B = 1 fast"] = F[3:4]; out["B = 1 slow"] = S[3:4]
    out["B = 67"] = inter[:67]
    out["B = 67 fast but the last lane"] = np.concatenate([F[100:166], S[7:8]])
    return out


def test_scalar_orderings_are_what_they_say():
    X = _scalar_cases()
    exits = _scalar_exits(X)
    o = _orderings(X, exits)
    assert np.all(exits[o["all fast"]] != "loop") and np.all(exits[o["all slow"]] == "loop")
    inter = exits[o["interleaved"]] == "loop"
    assert all(0 < np.sum(inter[w:w + 64]) < min(64, inter.size - w) for w in range(0, inter.size, 64))
    for k, idx in o.items():
        if k.startswith("one slow lane"):
            assert np.sum(exits[idx] == "loop") == 1
    assert o["B = 67"].size == 67 and o["B = 1 fast"].size == 1 and np.sum(exits[o["B = 67 fast but the last lane"]] == "loop") == 1


@pytest.mark.gpu
def test_scalar_boxqp_forms_agree_on_device(api, tmp_path):
    """boxqp_solve<1>, boxqp_solve1 and boxqp_solve1_fast on the device: status, free flag and x agree exactly, with each other, with
    the host build and with the twin, in every ordering of fast and slow lanes."""
    dev, hst = P.device(), P.host(tmp_path)
    X = _scalar_cases()
    exits = _scalar_exits(X)
    st, fr, xs = _scalar_twin(X)
    Yl = P.run(dev, "boxqp1", X)
    assert P.same_numbers(Yl, P.run(hst, "boxqp1", X))
    assert P.same_numbers(Yl[:3], P.run(dev, "boxqp_1", X)[:3])
    assert np.array_equal(Yl[0], st) and np.array_equal(Yl[1], fr) and P.same_numbers(Yl[2], xs)
    for name, idx in _orderings(X, exits).items():
        Yf = P.run(dev, "boxqp1_fast", X[:, idx])
        bad = np.where(~((Yf[:3] == Yl[:3, idx]) | (np.isnan(Yf[:3]) & np.isnan(Yl[:3, idx]))).all(axis=0))[0]
        assert bad.size == 0, (name, bad[:8], Yf[:3, bad[:4]], Yl[:3, idx[bad[:4]]], exits[idx[bad[:4]]])
