"""The elementary routines of cddp-cpp_amd/csrc/dev_trig.hpp (sincos_fast / sincos_n<1>, log_shared, exp_fast, pow_shared, asin_shared)
ON THE DEVICE, through the probe library (tests/hip/dev_probe.hip); tests/test_dev_trig.py compiles the header for the host only.

Arguments: the sets of tests/cpp/test_dev_trig.cpp and test_dev_elem.cpp, about 40 000 points in all.  In range: the ulp
bounds those host tests assert (sin, cos < 0.85; log < 0.9; exp < 0.95; asin < 0.8; pow < 64), here against mpmath at 60 digits,
and bit equality with the host build of the same source (straight-line code of IEEE basic operations and explicit fma, both
builds without contraction).  Fallback arguments (out of range, zero, negative, infinite, NaN) reach the device libm, whose
accuracy is not this project's code: semantics only -- sign, NaN-ness, infinities, exact values such as log 1 = 0.  Where a fallback
returns a finite inexact number (sin / cos of 1e12, asin 0.75) the test only asks that it IS that function's value, to 1e-14 /
1e-15 absolute on results of magnitude <= pi / 2, i.e. some tens of ulp: deliberately not a measured bound, a device libm within
its documented few ulp passes and a wrong branch (another function, a wrong quadrant, a dropped sign) does not."""
import numpy as np
import pytest
import mpmath as mp

import dev_probe as P

BOUND = {"sin": 0.85, "cos": 0.85, "log": 0.9, "exp": 0.95, "asin": 0.8, "pow": 64.0}
_cache = {}


def _args():
    if _cache:
        return _cache
    rng = np.random.default_rng(7000)
    n = 1500
    sc = [(2.0 * rng.random(n) - 1.0) * R for R in (0.8, 3.2, 7.0, 30.0, 1000.0, 1.0e6, 9.9e8)]
    near = []
    # neighbourhoods of the multiples of pi/2 over the host test's range k = -4000 .. 4000: every k up to 100, every 7th beyond
    for k in sorted(set(range(-100, 101)) | set(range(-4000, 4001, 7)) | {4000}):
        for j in (-8, -3, -1, 0, 1, 2, 8):
            x = np.float64(k * 1.5707963267948966)
            for _ in range(abs(j)):
                x = np.nextafter(x, -np.inf if j < 0 else np.inf)
            near.append(x)
    tiny = [np.ldexp(1.1, e) for e in range(-300, 0, 3)] + [-np.ldexp(1.7, e) for e in range(-300, 0, 3)]
    _cache["sincos"] = np.concatenate(sc + [near, tiny])
    _cache["log"] = np.concatenate([10.0 ** (-10.0 + 16.0 * rng.random(n)), 0.5 + 1.5 * rng.random(n),
                                    np.ldexp(1.0 + rng.random(n), rng.integers(-1020, 1021, size=n))])
    _cache["exp"] = np.concatenate([(2.0 * rng.random(2 * n) - 1.0) * 700.0, (2.0 * rng.random(n) - 1.0) * 2.0, [700.0, -700.0, 0.0]])
    _cache["asin"] = np.concatenate([(2.0 * rng.random(2 * n) - 1.0) * 0.4999999,
                                     10.0 ** (-12.0 + 11.7 * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)])
    mu = 10.0 ** (-10.0 + 11.0 * rng.random(n))
    _cache["pow"] = np.stack([np.concatenate([mu, mu, mu]), np.concatenate([np.full(n, 1.2), np.full(n, 0.25), 2.0 * rng.random(n)])])
    return _cache


def _run_in_range(lib):
    a = _args()
    Y = P.run(lib, "sincos", a["sincos"][None, :])
    return {"sincos": Y, "log": P.run(lib, "log", a["log"][None, :]), "exp": P.run(lib, "exp", a["exp"][None, :]),
            "asin": P.run(lib, "asin", a["asin"][None, :]), "pow": P.run(lib, "pow", a["pow"])}


def _check_in_range(R):
    a = _args()
    assert P.same_numbers(R["sincos"][0:2], R["sincos"][2:4]), "sincos_n<1> and sincos_fast differ inside the fast range"
    err = {
        "sin": P.max_ulp_error(mp.sin, a["sincos"], R["sincos"][0]), "cos": P.max_ulp_error(mp.cos, a["sincos"], R["sincos"][1]),
        "log": P.max_ulp_error(mp.log, a["log"], R["log"][0]), "exp": P.max_ulp_error(mp.exp, a["exp"], R["exp"][0]),
        "asin": P.max_ulp_error(mp.asin, a["asin"], R["asin"][0]),
        "pow": P.max_ulp_error(mp.power, [(x, y) for x, y in a["pow"].T], R["pow"][0]),
    }
    print("max ulp error against mpmath (value, argument):", err)
    for k, (e, at) in err.items():
        assert e < BOUND[k], (k, e, at)
    return err


def _fallback(lib):
    """Semantics of the out-of-range paths."""
    inf, nan = np.inf, np.nan
    x = np.array([1.0e12, -3.0e15, inf, -inf, nan, 0.0, 1.0e9, -1.0e9])
    Y = P.run(lib, "sincos", x[None, :])
    s, c = Y[0], Y[1]
    assert np.all(np.isnan(s[2:5])) and np.all(np.isnan(c[2:5]))
    assert s[5] == 0.0 and c[5] == 1.0
    for i in (0, 1, 6, 7):                                   # libm on a huge finite argument: a sine and a cosine of the same angle
        assert abs(s[i]) <= 1.0 and abs(c[i]) <= 1.0 and abs(s[i] * s[i] + c[i] * c[i] - 1.0) < 1e-14
        assert abs(s[i] - float(mp.sin(mp.mpf(float(x[i]))))) < 1e-14 and abs(c[i] - float(mp.cos(mp.mpf(float(x[i]))))) < 1e-14
    x = np.array([0.0, -1.0, inf, nan, 1.0, 4.9e-324, 1e-310, -inf, 2.2250738585072014e-308])
    L = P.run(lib, "log", x[None, :])[0]
    assert L[0] == -inf and np.isnan(L[1]) and L[2] == inf and np.isnan(L[3]) and L[4] == 0.0 and np.isnan(L[7])
    e, at = P.max_ulp_error(mp.log, x[[5, 6, 8]], L[[5, 6, 8]])       # subnormal arguments are log_shared's own code (scaled by 2^54)
    assert e < BOUND["log"], (e, at)
    x = np.array([0.75, 1.0, -1.0, 1.5, 0.0, nan, 0.5, -0.5])
    A = P.run(lib, "asin", x[None, :])[0]
    assert abs(A[0] - np.arcsin(0.75)) < 1e-15 and abs(A[1] - np.pi / 2) < 1e-15 and abs(A[2] + np.pi / 2) < 1e-15
    assert np.isnan(A[3]) and A[4] == 0.0 and np.isnan(A[5]) and abs(A[6] - np.pi / 6) < 1e-15 and abs(A[7] + np.pi / 6) < 1e-15
    xy = np.array([[0.0, 1.0, 1e300, 1e-300, 2.0, -2.0, -8.0, inf, nan, 4.0], [0.25, 1.2, 3.0, 3.0, 0.0, 2.0, 1.0 / 3.0, 0.5, 1.0, 0.5]])
    W = P.run(lib, "pow", xy)[0]
    assert W[0] == 0.0 and W[1] == 1.0 and W[2] == inf and W[3] == 0.0 and W[4] == 1.0 and W[5] == 4.0
    assert np.isnan(W[6]) and W[7] == inf and np.isnan(W[8]) and abs(W[9] - 2.0) <= 64 * P.EPS * 2.0


def test_elementary_routines_host_build(tmp_path):
    """The argument sets and bounds of the GPU test below, validated on the host build of the same source."""
    lib = P.host(tmp_path)
    _check_in_range(_run_in_range(lib))
    _fallback(lib)


@pytest.mark.gpu
def test_elementary_routines_on_device(api, tmp_path):
    R = _run_in_range(P.device())
    _check_in_range(R)
    H = _run_in_range(P.host(tmp_path))
    for k in R:
        bad = np.where(~((R[k] == H[k]) | (np.isnan(R[k]) & np.isnan(H[k]))).all(axis=0))[0]
        assert bad.size == 0, (k, bad.size, bad[:5], R[k][:, bad[:5]], H[k][:, bad[:5]])


@pytest.mark.gpu
def test_elementary_fallbacks_on_device(api):
    _fallback(P.device())
