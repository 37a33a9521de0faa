"""CPU-side checks of the boundary of the output-feedback Monte-Carlo entries (cddp_hip_mc_sample_meas_noise, cddp_hip_plan_montecarlo_of):
exported by the built library, declared in include/cddp_hip.h with the documented signature, descriptor and arithmetic, bound in pyapi with
matching argtypes and a descriptor of the stated size, each refusal that needs no device answered with its own message instead of a crash,
the Python binding's own refusals raised before the library is called, offered by HipBatchSolver, the facade and the C++ mirror, and
instantiated over every plant -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import model_cases as MC
from test_plan_kf_abi import _NoLibrary, declaration, header, lib  # noqa: F401  (lib: the fixture that builds the library when it is missing)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cddp_hip_mc_sample_meas_noise", "cddp_hip_plan_montecarlo_of")


def test_symbols_are_exported(api, lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), "libcddp_hip.so does not export %s" % s
        assert s in api.EXPORTED_SYMBOLS


def test_header_declares_the_documented_signature():
    assert declaration(SYMBOLS[0]) == ["cddp_hip_handle *h", "int flags", "const cddp_hip_mcof_desc *desc", "double *Yn"]
    assert declaration(SYMBOLS[1]) == ["cddp_hip_handle *h", "cddp_hip_plant *plant", "int flags", "const cddp_hip_mcof_desc *desc", "const double *x0",
                                       "const double *L", "double *cost", "double *viol", "double *stats", "int32_t *nviol_step", "double *dXmean",
                                       "double *SX", "double *dUmean", "double *SU", "double *X_out", "double *U_out", "double *dEmean", "double *SE",
                                       "double *Xh_out"]
    m = re.search(r"typedef struct cddp_hip_mcof_desc \{(.*?)\} cddp_hip_mcof_desc;", header(), flags=re.S)
    assert m and [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()] == [
        "cddp_hip_mc_desc mc", "int32_t ny", "int32_t _pad", "const double *C", "const double *v"]
    raw = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", raw)                     # new entry points only
    doc = re.sub(r"\s+", " ", raw[raw.index("Monte-Carlo evaluation of a solved plan under output feedback"):raw.index("typedef struct cddp_hip_mcof_desc")])
    for needle in ("e = nx + N (nu + nx) + t ny + r", "s += C[r][j] * dx[j]", "p += C[r][j] * xh[j]", "before step 4 changes any of it",
                   "s += L_t[i][r] * inn[r]", "e[i] = dx[i] - xh[i]", "s += K_t[i][j] * xh[j]", "s += A_t[i][j] * xh[j]", "s += B_t[i][j] * fb[j]",
                   "unclipped, noise-free fb", "keep_nominal zeroes the measurement noise of sample 0 too", "sqrt(v[r]), correctly rounded",
                   "Not covered: nonlinear (EKF) or saturation-aware prediction", "intermittent", "NEES or quantiles"):
        assert needle in doc, needle
    hpp = open(os.path.join(MC.CSRC, "plan_mcof.hpp")).read()
    assert "xp[i] = s, s = 0; s += A_t[i][j] * xh[j] (j ascending), then s += B_t[i][j] * fb[j]" in hpp


def test_binding_matches_the_header(api, lib):
    assert C.sizeof(api.McofDesc) == 80 and api.McofDesc.mc.offset == 0 and api.McofDesc.ny.offset == 56 and api.McofDesc.C.offset == 64 and api.McofDesc.v.offset == 72
    fn = getattr(lib, SYMBOLS[0])
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] and fn.restype is C.c_int
    fn = getattr(lib, SYMBOLS[1])
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 15 and fn.restype is C.c_int
    assert len(fn.argtypes) == len(declaration(SYMBOLS[1]))
    assert api.MCOF_OUTPUTS == api.MC_OUTPUTS + ("dEmean", "SE", "Xh")
    assert lib.cddp_hip_abi_version() == 5


def test_refusals_that_need_no_device_have_their_own_messages(api, lib):
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    d = api.McofDesc()
    d.mc.nsamp = 4; d.ny = 1; d.C = C.cast(p, C.POINTER(C.c_double)); d.v = C.cast(p, C.POINTER(C.c_double))
    outs = (p,) * 13
    f = lib.cddp_hip_plan_montecarlo_of
    g = lib.cddp_hip_mc_sample_meas_noise
    fake = C.c_void_p(8)       # never dereferenced: every refusal below comes before the handle is looked into
    cases = [
        (lambda: f(None, None, 0, C.addressof(d), None, p, *outs), -1, b"cddp_hip_plan_montecarlo_of: null handle"),
        (lambda: f(fake, None, 0, None, None, p, *outs), -1, b"cddp_hip_plan_montecarlo_of: null descriptor"),
        (lambda: f(fake, None, 4, C.addressof(d), None, p, *outs), -2, b"cddp_hip_plan_montecarlo_of: unknown flag bits 0x4"),
        (lambda: g(None, 0, C.addressof(d), p), -1, b"cddp_hip_mc_sample_meas_noise: null handle"),
        (lambda: g(fake, 0, None, p), -1, b"cddp_hip_mc_sample_meas_noise: null descriptor"),
        (lambda: g(fake, 2, C.addressof(d), p), -2, b"cddp_hip_mc_sample_meas_noise: unknown flag bits 0x2"),
    ]
    for call, code, message in cases:
        lib.cddp_hip_mpc_advance(None, 7, 0, None)           # (another message in between: each entry sets its own)
        assert call() == code
        assert message in lib.cddp_hip_last_error(), (message, lib.cddp_hip_last_error())
    d.mc.nsamp = 0
    assert f(fake, None, 0, C.addressof(d), None, p, *outs) == -2 and b"nsamp = 0" in lib.cddp_hip_last_error()
    assert list(buf) == [0.0] * 8


def test_binding_refuses_before_the_library_is_called(api):
    import types
    h = object.__new__(api.HipBatchSolver)
    h.p = types.SimpleNamespace(N=5, nx=4, nu=2); h.B = 3; h.lib = _NoLibrary(); h.h = None
    Cm = np.ones((2, 4)); v = np.ones(2); L = np.zeros((3, 6, 4, 2))
    with pytest.raises(ValueError, match="want"):
        h.plan_montecarlo_of(Cm, v, L, want=())
    with pytest.raises(ValueError, match="want"):
        h.plan_montecarlo_of(Cm, v, L, want=("SE", "SF"))
    with pytest.raises(ValueError, match="gains L must be given"):
        h.plan_montecarlo_of(Cm, v, None)
    with pytest.raises(ValueError, match="C and v must be given"):
        h.plan_montecarlo_of(None, v, L)
    with pytest.raises(ValueError, match="C and v must be given"):
        h.plan_montecarlo_of(Cm, None, L)
    with pytest.raises(ValueError, match="measurement rows"):
        h.plan_montecarlo_of(np.ones((17, 4)), np.ones(17), np.zeros((3, 6, 4, 17)))
    with pytest.raises(ValueError, match="measurement rows"):
        h.mc_sample_meas_noise(np.ones(0))
    with pytest.raises(ValueError, match="variances > 0"):
        h.plan_montecarlo_of(Cm, np.array([1.0, 0.0]), L)
    with pytest.raises(ValueError, match="variances > 0"):
        h.mc_sample_meas_noise(np.array([1.0, np.inf]))
    with pytest.raises(ValueError, match="C: a finite matrix"):
        h.plan_montecarlo_of(np.ones((2, 3)), v, L)
    with pytest.raises(ValueError, match="C: a finite matrix"):
        h.plan_montecarlo_of(np.full((2, 4), np.nan), v, L)
    with pytest.raises(ValueError, match="shape"):
        h.plan_montecarlo_of(Cm, v, np.zeros((3, 5, 4, 2)))              # L without the row of step N
    with pytest.raises(ValueError, match="nsamp"):
        h.plan_montecarlo_of(Cm, v, L, nsamp=1025)
    with pytest.raises(ValueError, match="Sigma0"):
        h.plan_montecarlo_of(Cm, v, L, Sigma0=np.eye(3))
    d, keep = h._mcof_desc("t", Cm, np.array([4.0, 9.0]), None, None, None, 7)
    assert d.ny == 2 and d.mc.nsamp == 7 and d.v[1] == 9.0 and d.C[7] == 1.0 and not d.mc.L0


def test_solver_facade_and_mirror_offer_the_methods(api):
    assert callable(api.HipBatchSolver.plan_montecarlo_of) and callable(api.HipBatchSolver.mc_sample_meas_noise)
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    assert callable(mod.CDDP.solve_batch_lqg_mc)
    sv = mod.CDDP([0.0, 0.0], [0.0, 0.0], 10, 0.02)
    with pytest.raises(RuntimeError):
        sv.solve_batch_lqg_mc(None, None, None, None)            # no dynamical system yet: refused before anything else is looked at
    txt = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    assert re.search(r"\bplanMonteCarloOf\s*\(", txt) and "cddp_hip_plan_montecarlo_of(h_" in txt
    assert re.search(r"\bmcSampleMeasNoise\s*\(", txt) and "cddp_hip_mc_sample_meas_noise(h_" in txt


def test_kernel_is_a_unit_of_its_own_over_every_plant():
    mk = open(os.path.join(MC.CSRC, "Makefile")).read()
    assert re.search(r"\binst_mcof\.hip\b", mk)
    src = open(os.path.join(MC.CSRC, "inst_mcof.hip")).read()
    assert "PLANT_MODEL_LIST(Y)" in src and '#include "plan_mcof.hpp"' in src and '#include "mc_reduce.hpp"' in src
    assert '#include "mc_reduce.hpp"' in open(os.path.join(MC.CSRC, "inst_mc.hip")).read()       # the two units share the sums over the samples
