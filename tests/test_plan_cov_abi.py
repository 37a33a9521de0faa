"""CPU-side checks of the boundary of the plan covariance (cddp_hip_plan_covariance): exported by the built library, declared in
include/cddp_hip.h with the documented signature and flags, bound in pyapi with matching argtypes, each refusal that needs no device
answered with its own message instead of a crash, offered by HipBatchSolver, the facade and the C++ mirror, and instantiated over the
pairs of the plan sensitivities -- no GPU needed."""
import ctypes as C
import os
import re

import pytest

import model_cases as MC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "cddp_hip_plan_covariance"


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
    assert declaration(SYMBOL) == ["cddp_hip_handle *h", "int flags", "const double *Sigma0", "const double *W", "const double *Wu", "double *SX",
                                   "double *SU", "double *dcost"]
    assert re.search(r"enum\s*\{\s*CDDP_HIP_COV_DEVICE\s*=\s*1\s*,\s*CDDP_HIP_COV_DIAG\s*=\s*2\s*,\s*CDDP_HIP_COV_PER_TRAJ\s*=\s*4\s*\}", header())
    raw = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", raw)                     # a new entry point only
    doc = re.sub(r"\s+", " ", raw[raw.index("state and control covariance along a solved plan"):raw.index("int cddp_hip_plan_covariance")])
    assert "LAST BACKWARD SWEEP" in doc and "cddp_hip_backward first" in doc           # which sweep the stacks belong to


def test_binding_argtypes_match_the_header(api, lib):
    fn = getattr(lib, SYMBOL)
    assert list(fn.argtypes) == [C.c_void_p, C.c_int] + [C.c_void_p] * 6 and fn.restype is C.c_int
    assert len(fn.argtypes) == len(declaration(SYMBOL))
    assert (api.COV_DEVICE, api.COV_DIAG, api.COV_PER_TRAJ) == (1, 2, 4)
    assert lib.cddp_hip_abi_version() == 5


def test_refusals_that_need_no_device_have_their_own_messages(api, lib):
    buf = (C.c_double * 8)()
    fake = C.c_void_p(8)       # never dereferenced: every refusal below comes before the handle is looked into
    p = C.addressof(buf)
    f = lib.cddp_hip_plan_covariance
    cases = [
        (lambda: f(None, 0, p, p, p, p, p, p), b"cddp_hip_plan_covariance: null handle"),
        (lambda: f(fake, 8, p, p, p, p, p, p), b"cddp_hip_plan_covariance: unknown flag bits 0x8"),
        (lambda: f(fake, 7 | 48, p, p, p, p, p, p), b"cddp_hip_plan_covariance: unknown flag bits 0x30"),
        (lambda: f(fake, 0, None, p, p, p, p, p), b"cddp_hip_plan_covariance: null Sigma0 pointer"),
        (lambda: f(fake, 2, p, None, None, None, None, None), b"cddp_hip_plan_covariance: SX, SU and dcost are all null"),
    ]
    for call, message in cases:
        lib.cddp_hip_mpc_advance(None, 7, 0, None)           # (another message in between: each entry sets its own)
        assert call() != 0
        assert message in lib.cddp_hip_last_error(), (message, lib.cddp_hip_last_error())
    assert list(buf) == [0.0] * 8


def test_solver_facade_and_mirror_offer_the_method(api):
    assert callable(api.HipBatchSolver.plan_covariance)
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    assert callable(mod.CDDP.solve_batch_cov)
    sv = mod.CDDP([0.0, 0.0], [0.0, 0.0], 10, 0.02)
    with pytest.raises(RuntimeError):
        sv.solve_batch_cov(None, None)                       # no dynamical system yet: refused before anything else is looked at
    txt = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    assert re.search(r"\bplanCovariance\s*\(", txt) and "cddp_hip_plan_covariance(h_" in txt


def cov_pair_list():
    """The (nx, nu) pairs in COV_PAIR_LIST of csrc/inst_cov.hip, in order."""
    with open(os.path.join(MC.CSRC, "inst_cov.hip")) as fh:
        text = fh.read()
    m = re.search(r"#define\s+COV_PAIR_LIST\(Y\)((?:[^\n]*\\\n)*[^\n]*)", text)
    return [(int(a), int(b)) for a, b in re.findall(r"Y\((\d+),\s*(\d+)\)", m.group(1))]


def test_covariance_is_instantiated_over_the_sensitivity_pairs():
    assert cov_pair_list() == MC.sens_pair_list()
    assert sorted(MC.SENS_MODELS) == sorted(cov_pair_list())
    mk = open(os.path.join(MC.CSRC, "Makefile")).read()
    assert re.search(r"\binst_cov\.hip\b", mk)
