"""CPU-side checks of the boundary of the filter entry (cddp_hip_plan_kalman): exported by the built library, declared in
include/cddp_hip.h with the documented signature and flags, bound in pyapi with matching argtypes, each refusal that needs no device
answered with its own message instead of a crash, the Python binding's own refusals raised before the library is called, offered by
HipBatchSolver, the facade and the C++ mirror, and instantiated over the pairs of the plan sensitivities -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import model_cases as MC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "cddp_hip_plan_kalman"


@pytest.fixture(scope="module")
def lib(api):
    if not os.path.exists(api.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return api.load_hip()


def header():
    txt = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)      # comments out (the parameter list carries size comments)


def declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, "%s is not declared in include/cddp_hip.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_symbol_is_exported(api, lib):
    assert hasattr(lib, SYMBOL), "libcddp_hip.so does not export %s" % SYMBOL
    assert SYMBOL in api.EXPORTED_SYMBOLS


def test_header_declares_the_documented_signature():
    assert declaration(SYMBOL) == ["cddp_hip_handle *h", "int flags", "int ny", "const double *C", "const double *v", "const double *Sigma0",
                                   "const double *W", "const double *Wu", "double *L_out", "double *SP_out", "double *SF_out", "double *SX",
                                   "double *SU", "double *dcost", "int32_t *info"]
    assert re.search(r"enum\s*\{\s*CDDP_HIP_KF_DEVICE\s*=\s*1\s*,\s*CDDP_HIP_KF_DIAG\s*=\s*2\s*,\s*CDDP_HIP_KF_PER_TRAJ\s*=\s*4\s*\}", header())
    raw = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    assert re.search(r"#define\s+CDDP_HIP_KF_MAX_NY\s+16\b", raw)
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", raw)                     # a new entry point only
    doc = re.sub(r"\s+", " ", raw[raw.index("Kalman filter gains and output-feedback covariance along a solved plan"):raw.index("int cddp_hip_plan_kalman")])
    assert "LAST BACKWARD SWEEP" in doc and "cddp_hip_backward first" in doc           # which sweep the stacks belong to
    assert "CDDP_HIP_LQR_INSTALL the recursion sees the installed gains" in doc
    assert "The row FAILS unless sr > 0" in doc and "info[b] = t + 1" in doc
    assert "the caller's to whiten" in doc                                             # correlated measurement noise


def test_binding_argtypes_match_the_header(api, lib):
    fn = getattr(lib, SYMBOL)
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 12 and fn.restype is C.c_int
    assert len(fn.argtypes) == len(declaration(SYMBOL))
    assert (api.KF_DEVICE, api.KF_DIAG, api.KF_PER_TRAJ, api.KF_MAX_NY) == (1, 2, 4, 16)
    assert lib.cddp_hip_abi_version() == 5


def test_refusals_that_need_no_device_have_their_own_messages(api, lib):
    buf = (C.c_double * 8)()
    fake = C.c_void_p(8)       # never dereferenced: every refusal below comes before the handle is looked into
    p = C.addressof(buf)
    f = lib.cddp_hip_plan_kalman
    outs = (p,) * 7
    cases = [
        (lambda: f(None, 0, 1, p, p, p, p, p, *outs), -1, b"cddp_hip_plan_kalman: null handle"),
        (lambda: f(fake, 8, 1, p, p, p, p, p, *outs), -2, b"cddp_hip_plan_kalman: unknown flag bits 0x8"),
        (lambda: f(fake, 7 | 48, 1, p, p, p, p, p, *outs), -2, b"cddp_hip_plan_kalman: unknown flag bits 0x30"),
        (lambda: f(fake, 0, 0, p, p, p, p, p, *outs), -2, b"cddp_hip_plan_kalman: ny = 0, 1 .. 16 measurement rows are expected"),
        (lambda: f(fake, 0, 17, p, p, p, p, p, *outs), -2, b"cddp_hip_plan_kalman: ny = 17, 1 .. 16 measurement rows are expected"),
        (lambda: f(fake, 0, 1, None, p, p, p, p, *outs), -1, b"cddp_hip_plan_kalman: null C pointer"),
        (lambda: f(fake, 0, 1, p, None, p, p, p, *outs), -1, b"cddp_hip_plan_kalman: null v pointer"),
        (lambda: f(fake, 0, 1, p, p, None, p, p, *outs), -1, b"cddp_hip_plan_kalman: null Sigma0 pointer"),
        (lambda: f(fake, 7, 1, p, p, p, p, p, *((None,) * 7)), -1, b"cddp_hip_plan_kalman: all six outputs and info are null"),
    ]
    for call, code, message in cases:
        lib.cddp_hip_mpc_advance(None, 7, 0, None)           # (another message in between: each entry sets its own)
        assert call() == code
        assert message in lib.cddp_hip_last_error(), (message, lib.cddp_hip_last_error())
    assert list(buf) == [0.0] * 8


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s): the binding must refuse before" % name)


def test_binding_refuses_before_the_library_is_called(api):
    """empty or unknown want, missing inputs, mixed host / device arguments, wrong shapes, ny out of range and float32: ValueError from
    HipBatchSolver.plan_kalman itself.  The solver object is made without a handle, and its library raises when touched."""
    import types
    torch = pytest.importorskip("torch")
    h = object.__new__(api.HipBatchSolver)
    h.p = types.SimpleNamespace(N=5, nx=4, nu=2); h.B = 3; h.lib = _NoLibrary(); h.h = None
    Cm = np.ones((2, 4)); v = np.ones(2); S0 = np.eye(4)
    with pytest.raises(ValueError, match="want"):
        h.plan_kalman(Cm, v, S0, want=())
    with pytest.raises(ValueError, match="want"):
        h.plan_kalman(Cm, v, S0, want=("L", "K"))
    with pytest.raises(ValueError, match="must be given"):
        h.plan_kalman(Cm, None, S0)
    with pytest.raises(ValueError, match="all be numpy arrays or all be device tensors"):
        h.plan_kalman(Cm, torch.ones(2, dtype=torch.float64), S0)
    with pytest.raises(ValueError, match="shape"):
        h.plan_kalman(np.ones((2, 3)), v, S0)                    # C of another nx
    with pytest.raises(ValueError, match="shape"):
        h.plan_kalman(Cm, np.ones(3), S0)                        # v of another ny
    with pytest.raises(ValueError, match="shape"):
        h.plan_kalman(Cm, v, np.eye(3))
    with pytest.raises(ValueError, match="shape"):
        h.plan_kalman(Cm, v, S0, Wu=np.eye(4))                   # Wu of W's size
    with pytest.raises(ValueError, match="shape"):
        h.plan_kalman(np.broadcast_to(Cm, (3, 2, 4)).copy(), v, S0)   # C per trajectory, v and Sigma0 shared
    with pytest.raises(ValueError, match="shape"):
        h.plan_kalman(np.broadcast_to(Cm, (2, 2, 4)).copy(), v, S0)   # a leading axis that is not B
    with pytest.raises(ValueError, match="measurement rows"):
        h.plan_kalman(np.ones((17, 4)), np.ones(17), S0)
    with pytest.raises(ValueError, match="measurement rows"):
        h.plan_kalman(np.ones((0, 4)), np.ones(0), S0)
    with pytest.raises(ValueError, match="float64"):
        h.plan_kalman(Cm.astype(np.float32), v, S0)
    with pytest.raises(ValueError, match="device"):
        h.plan_kalman(Cm, v, S0, device=True)


def test_solver_facade_and_mirror_offer_the_method(api):
    assert callable(api.HipBatchSolver.plan_kalman)
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    assert callable(mod.CDDP.solve_batch_lqg)
    sv = mod.CDDP([0.0, 0.0], [0.0, 0.0], 10, 0.02)
    with pytest.raises(RuntimeError):
        sv.solve_batch_lqg(None, None, None, None)               # no dynamical system yet: refused before anything else is looked at
    txt = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    assert re.search(r"\bplanKalman\s*\(", txt) and "cddp_hip_plan_kalman(h_" in txt


def kf_pair_list():
    """The (nx, nu) pairs in KF_PAIR_LIST of csrc/inst_kf.hip, in order."""
    with open(os.path.join(MC.CSRC, "inst_kf.hip")) as fh:
        text = fh.read()
    m = re.search(r"#define\s+KF_PAIR_LIST\(Y\)((?:[^\n]*\\\n)*[^\n]*)", text)
    return [(int(a), int(b)) for a, b in re.findall(r"Y\((\d+),\s*(\d+)\)", m.group(1))]


def test_filter_is_instantiated_over_the_sensitivity_pairs():
    assert kf_pair_list() == MC.sens_pair_list()
    assert sorted(MC.SENS_MODELS) == sorted(kf_pair_list())
    mk = open(os.path.join(MC.CSRC, "Makefile")).read()
    assert re.search(r"\binst_kf\.hip\b", mk)
