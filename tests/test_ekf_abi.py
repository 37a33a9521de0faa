"""CPU-side checks of the boundary of the extended Kalman filter entries (cddp_hip_ekf_*, cddp_hip_mpc_run_ekf): exported by the built
library, declared in include/cddp_hip.h with the documented signatures, descriptor and arithmetic, bound in pyapi with matching argtypes and
a descriptor of the stated size and offsets, every refusal that needs neither a device nor a plant answered with its own message instead
of a crash (those that read the plant's dimensions -- v, C, W, Wu, substeps -- are exercised on the GPU by tests/test_ekf.py), offered by
HipBatchSolver, the facade and the C++ mirror, and instantiated over every plant -- no GPU needed."""
import ctypes as C
import os
import re

import model_cases as MC
from test_plan_kf_abi import declaration, header, lib  # noqa: F401  (lib: the fixture that builds the library when it is missing)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cddp_hip_ekf_create", "cddp_hip_ekf_destroy", "cddp_hip_ekf_reset", "cddp_hip_ekf_update", "cddp_hip_ekf_predict", "cddp_hip_ekf_get",
           "cddp_hip_ekf_run", "cddp_hip_mpc_run_ekf")


def test_symbols_are_exported(api, lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), "libcddp_hip.so does not export %s" % s
        assert s in api.EXPORTED_SYMBOLS


def test_header_declares_the_documented_signatures():
    assert declaration("cddp_hip_ekf_create") == ["cddp_hip_plant *model", "const cddp_hip_ekf_desc *desc", "cddp_hip_ekf **out"]
    assert declaration("cddp_hip_ekf_destroy") == ["cddp_hip_ekf *ekf"]
    assert declaration("cddp_hip_ekf_reset") == ["cddp_hip_ekf *ekf", "int flags", "const double *xh0", "const double *P0"]
    assert declaration("cddp_hip_ekf_update") == ["cddp_hip_ekf *ekf", "int flags", "const double *y", "double *nis"]
    assert declaration("cddp_hip_ekf_predict") == ["cddp_hip_ekf *ekf", "int flags", "const double *u"]
    assert declaration("cddp_hip_ekf_get") == ["cddp_hip_ekf *ekf", "int flags", "double *xh", "double *P", "int32_t *info"]
    assert declaration("cddp_hip_ekf_run") == ["cddp_hip_ekf *ekf", "int flags", "int T", "const double *Y", "const double *U", "double *Xh_out",
                                               "double *P_out", "double *nis_out", "int32_t *info"]
    assert declaration("cddp_hip_mpc_run_ekf") == ["cddp_hip_handle *h", "cddp_hip_plant *plant", "cddp_hip_ekf *ekf", "int steps", "int mode", "int flags",
                                                   "const double *x0_true", "const double *W", "const double *Yn", "double *U_applied", "double *X_visited",
                                                   "double *Xh_visited", "double *nis", "int32_t *iterations", "int32_t *status", "cddp_hip_stats *stats_sum"]
    m = re.search(r"typedef struct cddp_hip_ekf_desc \{(.*?)\} cddp_hip_ekf_desc;", header(), flags=re.S)
    assert m and [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()] == [
        "int32_t abi_version", "int32_t ny", "int32_t per_trajectory", "int32_t _pad", "const double *C", "const double *v", "const double *W", "const double *Wu"]
    raw = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", raw)                     # new entry points only
    doc = re.sub(r"\s+", " ", raw[raw.index("extended Kalman filter on the device; the MPC loop closed through it"):raw.index("typedef struct cddp_hip_ekf_desc")])
    for needle in ("h[i] = sum_j P[i][j] * c[j], from 0.0", "s = v[r]; s += c[j] * h[j]", "m = sum_j c[j] * xh[j], from 0.0", "e = y[r] - m", "g[i] = h[i] / s",
                   "xh[i] = xh[i] + g[i] * e", "q += (s * g[i]) * g[j]", "nis += (e * e) / s", "CDDP_HIP_EKF_SKIP_NAN", "info = t + 1",
                   "A[i][j] = h * Fx[i][j], then += 1.0 where i == j", "Bm = h * Fu", "P <- A P A^T + W + Bm Wu Bm^T", "triangles of W and Wu are read",
                   "Not covered: sub-stepped estimator models"):
        assert needle in doc, needle
    for flag, value in (("CDDP_HIP_EKF_DEVICE", 1), ("CDDP_HIP_EKF_SKIP_NAN", 2), ("CDDP_HIP_EKF_PER_TRAJ", 4), ("CDDP_HIP_EKF_DIAG", 8), ("CDDP_HIP_MPC_EKF_SKIP_NAN", 256)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (flag, value), header()), flag


def test_binding_matches_the_header(api, lib):
    D = api.EkfDesc
    assert C.sizeof(D) == 48
    assert [getattr(D, f).offset for f in ("abi_version", "ny", "per_trajectory", "_pad", "C", "v", "W", "Wu")] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert (api.EKF_DEVICE, api.EKF_SKIP_NAN, api.EKF_PER_TRAJ, api.EKF_DIAG, api.MPC_EKF_SKIP_NAN) == (1, 2, 4, 8, 256)
    for s in SYMBOLS:
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(declaration(s)), s
    assert lib.cddp_hip_abi_version() == 5


def test_refusals_that_need_no_device_have_their_own_messages(api, lib):
    buf = (C.c_double * 8)(*([1.0] * 8))
    p = C.addressof(buf)
    dp = C.cast(p, C.POINTER(C.c_double))
    out = C.c_void_p()

    def desc(**kw):
        d = api.EkfDesc()
        d.abi_version = api.ABI_VERSION; d.ny = 1; d.C = dp; d.v = dp
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    mk = lib.cddp_hip_ekf_create
    none = C.POINTER(C.c_double)()
    cases = [
        (lambda: mk(None, None, C.byref(out)), -1, b"cddp_hip_ekf_create: null argument"),
        (lambda: mk(None, C.byref(desc()), None), -1, b"cddp_hip_ekf_create: null argument"),
        (lambda: mk(None, C.byref(desc(abi_version=4)), C.byref(out)), -2, b"cddp_hip_ekf_create: ABI version mismatch: got 4 want 5"),
        (lambda: mk(None, C.byref(desc(ny=0)), C.byref(out)), -2, b"cddp_hip_ekf_create: ny = 0, 1 .. 16 measurement rows are expected"),
        (lambda: mk(None, C.byref(desc(ny=17)), C.byref(out)), -2, b"cddp_hip_ekf_create: ny = 17, 1 .. 16 measurement rows are expected"),
        (lambda: mk(None, C.byref(desc(C=none)), C.byref(out)), -1, b"cddp_hip_ekf_create: null C pointer"),
        (lambda: mk(None, C.byref(desc(v=none)), C.byref(out)), -1, b"cddp_hip_ekf_create: null v pointer"),
        (lambda: mk(None, C.byref(desc()), C.byref(out)), -1, b"cddp_hip_ekf_create: null model plant"),
        (lambda: lib.cddp_hip_ekf_reset(None, 0, p, p), -1, b"cddp_hip_ekf_reset: null estimator"),
        (lambda: lib.cddp_hip_ekf_update(None, 0, p, None), -1, b"cddp_hip_ekf_update: null estimator"),
        (lambda: lib.cddp_hip_ekf_predict(None, 0, p), -1, b"cddp_hip_ekf_predict: null estimator"),
        (lambda: lib.cddp_hip_ekf_get(None, 0, p, None, None), -1, b"cddp_hip_ekf_get: null estimator"),
        (lambda: lib.cddp_hip_ekf_run(None, 0, 1, p, p, p, None, None, None), -1, b"cddp_hip_ekf_run: null estimator"),
        (lambda: lib.cddp_hip_mpc_run_ekf(None, None, None, 1, 0, 0, dp, None, None, None, None, None, None, None, None, None), -1,
         b"cddp_hip_mpc_run_ekf: null handle"),
    ]
    for call, code, message in cases:
        lib.cddp_hip_mpc_advance(None, 7, 0, None)           # (another message in between: each entry sets its own)
        assert call() == code, message
        assert message in lib.cddp_hip_last_error(), (message, lib.cddp_hip_last_error())
    assert not out.value and list(buf) == [1.0] * 8
    assert lib.cddp_hip_ekf_destroy(None) == 0


def test_solver_facade_and_mirror_offer_the_methods(api):
    assert callable(api.HipBatchSolver.mpc_run_ekf)
    for m in ("reset", "update", "predict", "get", "run", "close"):
        assert callable(getattr(api.DeviceEkf, m)), m
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    import inspect
    sig = inspect.signature(mod.CDDP.solve_mpc_batch)
    assert "estimator" in sig.parameters and "meas_noise" in sig.parameters
    txt = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    assert re.search(r"\bclass Ekf\b", txt) and "cddp_hip_ekf_create(" in txt and "cddp_hip_ekf_run(" in txt
    assert re.search(r"\bmpcRunEkf\s*\(", txt) and "cddp_hip_mpc_run_ekf(h_" in txt


def test_kernel_is_a_unit_of_its_own_over_every_plant():
    mk = open(os.path.join(MC.CSRC, "Makefile")).read()
    assert re.search(r"\binst_ekf\.hip\b", mk)
    src = open(os.path.join(MC.CSRC, "inst_ekf.hip")).read()
    assert "PLANT_MODEL_LIST(Y)" in src and '#include "ekf.hpp"' in src and "KernelSet" not in src.replace("no KernelSet", "") and "atomic" not in src.replace("no atomics", "")
    hpp = open(os.path.join(MC.CSRC, "ekf.hpp")).read()
    assert '#include "plan_kf.hpp"' in hpp and "cddp_kf::joseph_row" in hpp and "cddp_cov::next_rows_to" in hpp and "hip_runtime" not in hpp
