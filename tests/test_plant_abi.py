"""CPU-side checks of the device-resident plant's boundary (cddp_hip_plant_create / _destroy / _step, cddp_hip_mpc_run_plant,
cddp_hip_track_plan): exported by the built library, declared in include/cddp_hip.h with the documented signatures, bound in pyapi with
matching argtypes, refusing NULL handles with a message -- and every descriptor refusal of cddp_hip_plant_create, which validates the
descriptor before it looks at a device: each returns its own message, and a fully valid descriptor gets as far as the "no HIP device"
refusal on a machine without one.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cddp_hip_plant_create", "cddp_hip_plant_destroy", "cddp_hip_plant_step", "cddp_hip_mpc_run_plant", "cddp_hip_track_plan")
INERTIA = [1.0, 0.1, 0.0, 0.1, 1.5, 0.05, 0.0, 0.05, 2.0]


@pytest.fixture(scope="module")
def lib(api):
    if not os.path.exists(api.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return api.load_hip()


def header():
    txt = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, "%s is not declared in include/cddp_hip.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_symbols_are_exported(api, lib):
    for s in ENTRIES:
        assert hasattr(lib, s), "libcddp_hip.so does not export %s" % s
        assert s in api.EXPORTED_SYMBOLS


def test_header_declares_the_documented_signatures():
    assert declaration("cddp_hip_plant_create") == ["const cddp_hip_plant_desc *desc", "int batch", "int device", "cddp_hip_plant **out"]
    assert declaration("cddp_hip_plant_destroy") == ["cddp_hip_plant *p"]
    assert declaration("cddp_hip_plant_step") == ["cddp_hip_plant *p", "int flags", "const double *x", "const double *u", "const double *w", "double *x_next"]
    assert declaration("cddp_hip_mpc_run_plant") == ["cddp_hip_handle *h", "cddp_hip_plant *plant", "int steps", "int mode", "int flags", "const double *W",
                                                     "double *U_applied", "double *X_visited", "int32_t *iterations", "int32_t *status",
                                                     "cddp_hip_stats *stats_sum"]
    assert declaration("cddp_hip_track_plan") == ["cddp_hip_handle *h", "cddp_hip_plant *plant", "const double *x0", "const double *W", "double *X_out",
                                                  "double *U_out"]
    h = header()
    m = re.search(r"typedef\s+struct\s+cddp_hip_plant_desc\s*\{([^}]*)\}\s*cddp_hip_plant_desc\s*;", h)
    assert m, "cddp_hip_plant_desc is not declared"
    fields = [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t abi_version", "int32_t model, integrator", "int32_t substeps", "int32_t nx, nu", "int32_t params_per_trajectory",
                      "int32_t _pad", "double dt", "const double *model_params", "const double *lti_A, *lti_B", "const double *u_lower, *u_upper"]
    assert re.search(r"CDDP_HIP_PLANT_DEVICE\s*=\s*1\b", h)
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", open(os.path.join(REPO, "include", "cddp_hip.h")).read())   # new entry points only


def test_binding_argtypes_match_the_header(api, lib):
    i32 = C.POINTER(C.c_int32); dp = C.POINTER(C.c_double)
    assert list(lib.cddp_hip_plant_create.argtypes) == [C.POINTER(api.PlantDesc), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    assert list(lib.cddp_hip_plant_destroy.argtypes) == [C.c_void_p]
    assert list(lib.cddp_hip_plant_step.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert list(lib.cddp_hip_mpc_run_plant.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, dp, i32, i32, C.POINTER(api.Stats)]
    assert list(lib.cddp_hip_track_plan.argtypes) == [C.c_void_p, C.c_void_p, dp, dp, dp, dp]
    for s in ENTRIES:
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(declaration(s)), s
    assert api.PLANT_DEVICE == 1
    # the structure's layout is the header's: eight int32, a double, five pointers
    assert [n for n, _ in api.PlantDesc._fields_] == ["abi_version", "model", "integrator", "substeps", "nx", "nu", "params_per_trajectory", "_pad", "dt",
                                                     "model_params", "lti_A", "lti_B", "u_lower", "u_upper"]
    assert C.sizeof(api.PlantDesc) == 8 * 4 + 8 + 5 * C.sizeof(C.c_void_p) and api.PlantDesc.dt.offset == 32
    assert callable(api.DevicePlant.step) and callable(api.DevicePlant.close)
    for name in ("mpc_run_plant", "track_plan"):
        assert callable(getattr(api.HipBatchSolver, name))


def test_null_handles_are_refused_with_a_message(api, lib):
    x = np.zeros(4)
    assert lib.cddp_hip_plant_step(None, 0, x.ctypes.data, x.ctypes.data, None, x.ctypes.data) != 0
    assert b"null plant" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_mpc_run_plant(None, None, 3, api.MPC_SHIFT_PROVIDED, 0, None, None, None, None, None, None) != 0
    assert b"null handle" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_track_plan(None, None, None, None, None, None) != 0
    assert b"null handle" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_plant_create(None, 4, 0, None) != 0
    assert b"null argument" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_plant_destroy(None) == 0


# ---- the descriptor refusals -------------------------------------------------------------------------------------------------------
class Desc:
    """A valid pendulum descriptor (RK4, two substeps, a control box) whose fields a case overrides."""
    def __init__(self, api, batch=3, **over):
        self.keep = {}
        d = api.PlantDesc()
        d.abi_version = api.ABI_VERSION; d.model = api.MODEL_PENDULUM; d.integrator = api.RK4; d.substeps = 2
        d.nx = 2; d.nu = 1; d.params_per_trajectory = 0; d.dt = 0.02
        self.d = d
        self.set("model_params", np.zeros(api.MAX_MODEL_PARAMS)); self.keep["model_params"][:4] = [0.5, 1.0, 0.01, 9.81]
        self.set("u_lower", [-2.0]); self.set("u_upper", [2.0])
        self.batch = batch
        for k, v in over.items():
            if k in ("model_params", "lti_A", "lti_B", "u_lower", "u_upper"):
                self.set(k, v)
            else:
                setattr(d, k, v)

    def set(self, name, v):
        if v is None:
            setattr(self.d, name, None); return
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64)); self.keep[name] = a
        setattr(self.d, name, a.ctypes.data_as(C.POINTER(C.c_double)))


def create(lib, desc):
    out = C.c_void_p()
    rc = lib.cddp_hip_plant_create(C.byref(desc.d), desc.batch, 0, C.byref(out))
    msg = lib.cddp_hip_last_error().decode() if rc else ""
    if rc == 0:
        lib.cddp_hip_plant_destroy(out)
    return rc, msg


def params24(api, rows):
    a = np.zeros((len(rows), api.MAX_MODEL_PARAMS))
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a


def refusal_cases(api):
    """(name, descriptor, the words its message must carry)."""
    singular = [1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 0.0, 1.0]
    att = dict(model=api.MODEL_EULER_ATTITUDE, nx=6, nu=3, u_lower=None, u_upper=None)
    lti = dict(model=api.MODEL_LTI, nx=2, nu=1, substeps=1, lti_A=[1.0, 0.1, -0.2, 0.95], lti_B=[0.005, 0.1])
    return [
        ("abi", Desc(api, abi_version=api.ABI_VERSION + 1), ["ABI version mismatch"]),
        ("model", Desc(api, model=24), ["unknown model id 24"]),
        ("model_negative", Desc(api, model=-1), ["unknown model id -1"]),
        ("integrator", Desc(api, integrator=4), ["unknown integrator 4"]),
        ("nx", Desc(api, nx=3), ["has nx = 2, nu = 1", "got nx = 3, nu = 1"]),
        ("nu", Desc(api, nu=2), ["has nx = 2, nu = 1", "got nx = 2, nu = 2"]),
        ("lti_dims", Desc(api, **dict(lti, nx=3)), ["LTI plant exists for"]),
        ("substeps", Desc(api, substeps=0), ["substeps must be at least 1 (got 0)"]),
        ("substeps_car", Desc(api, model=api.MODEL_CAR, nx=4, nu=2, substeps=2, u_lower=None, u_upper=None), ["discrete plant", "h = dt"]),
        ("substeps_forklift", Desc(api, model=api.MODEL_FORKLIFT, nx=5, nu=2, substeps=3, u_lower=None, u_upper=None), ["discrete plant"]),
        ("substeps_lti", Desc(api, **dict(lti, substeps=2)), ["discrete plant"]),
        ("dt_zero", Desc(api, dt=0.0), ["dt must be positive"]),
        ("dt_negative", Desc(api, dt=-0.02), ["dt must be positive"]),
        ("dt_nan", Desc(api, dt=float("nan")), ["dt must be positive"]),
        ("lower_null", Desc(api, u_lower=None), ["come as a pair", "u_lower is NULL"]),
        ("upper_null", Desc(api, u_upper=None), ["come as a pair", "u_upper is NULL"]),
        ("lower_above_upper", Desc(api, u_lower=[2.5]), ["u_lower[0] = 2.5", "u_upper[0] = 2"]),
        ("lti_no_A", Desc(api, **dict(lti, lti_A=None)), ["LTI plant needs lti_A and lti_B"]),
        ("lti_no_B", Desc(api, **dict(lti, lti_B=None)), ["LTI plant needs lti_A and lti_B"]),
        ("lti_per_trajectory", Desc(api, **dict(lti, params_per_trajectory=1)), ["shared by the batch"]),
        ("singular_inertia", Desc(api, model_params=params24(api, [singular]), **att), ["inertia matrix is singular"]),
        ("singular_inertia_trajectory", Desc(api, params_per_trajectory=1, model_params=params24(api, [INERTIA, INERTIA, singular]), **att),
         ["trajectory 2:", "inertia matrix is singular"]),
        ("mass", Desc(api, model=api.MODEL_QUADROTOR_RATE, nx=10, nu=4, u_lower=None, u_upper=None, model_params=params24(api, [[0.0, 20.0, 0.5]])),
         ["Mass must be positive"]),
        ("mass_trajectory", Desc(api, model=api.MODEL_QUADROTOR_RATE, nx=10, nu=4, u_lower=None, u_upper=None, params_per_trajectory=1,
                                 model_params=params24(api, [[1.0, 20.0, 0.5], [-1.0, 20.0, 0.5], [1.0, 20.0, 0.5]])), ["trajectory 1:", "Mass must be positive"]),
    ]


def test_every_descriptor_refusal_has_its_own_message(api, lib):
    seen = {}
    for name, desc, words in refusal_cases(api):
        rc, msg = create(lib, desc)
        assert rc != 0 and rc != -20, (name, rc, msg)
        assert msg.startswith("cddp_hip_plant_create:"), (name, msg)
        for w in words:
            assert w in msg, (name, w, msg)
        seen[name] = msg
    # distinct refusals, distinct messages
    kinds = ["abi", "model", "integrator", "nx", "lti_dims", "substeps", "substeps_car", "dt_zero", "lower_null", "lower_above_upper", "lti_no_A",
             "lti_per_trajectory", "singular_inertia", "mass"]
    assert len({seen[k] for k in kinds}) == len(kinds)


def test_a_valid_descriptor_reaches_the_device_check(api, lib):
    """Validation comes first: every valid descriptor -- shared and per-trajectory parameters, a discrete plant, LTI -- gets as far as
    the device, which this machine may not have."""
    have = lib.cddp_hip_device_count() > 0
    valid = [
        Desc(api),
        Desc(api, u_lower=None, u_upper=None, substeps=1),
        Desc(api, params_per_trajectory=1, model_params=params24(api, [[0.5, 1.0, 0.01, 9.81], [0.6, 1.2, 0.01, 9.81], [0.4, 0.8, 0.0, 9.81]])),
        Desc(api, model=api.MODEL_EULER_ATTITUDE, nx=6, nu=3, u_lower=None, u_upper=None, model_params=params24(api, [INERTIA])),
        Desc(api, model=api.MODEL_CAR, nx=4, nu=2, substeps=1, u_lower=[-0.5, -2.0], u_upper=[0.5, 2.0], model_params=params24(api, [[2.0]])),
        Desc(api, model=api.MODEL_LTI, nx=2, nu=1, substeps=1, lti_A=[1.0, 0.1, -0.2, 0.95], lti_B=[0.005, 0.1], model_params=None),
        Desc(api, model=api.MODEL_LTI, nx=1, nu=1, substeps=1, lti_A=[0.9], lti_B=[0.1]),
    ]
    for i, desc in enumerate(valid):
        rc, msg = create(lib, desc)
        if have:
            assert rc == 0, (i, rc, msg)
        else:
            assert rc == -20 and "no HIP device" in msg, (i, rc, msg)
    # and an invalid one is refused for its own reason even where there is no device: the order is descriptor, then device
    rc, msg = create(lib, Desc(api, substeps=0))
    assert rc == -2 and "substeps" in msg


def test_batch_must_be_positive(api, lib):
    rc, msg = create(lib, Desc(api, batch=0))
    assert rc != 0 and "batch must be positive" in msg


def test_python_plant_raises_the_refusal(api, lib):
    with pytest.raises(api.HipError, match="substeps must be at least 1"):
        api.DevicePlant(api.MODEL_PENDULUM, api.RK4, 0.02, 2, 1, 4, params=[0.5, 1.0, 0.01, 9.81], substeps=0)
    p = api.pendulum_problem()
    with pytest.raises(api.HipError, match="trajectory 1: .*singular"):
        api.DevicePlant(api.MODEL_MRP_ATTITUDE, api.EULER, 0.1, 6, 3, 2, params=np.array([INERTIA, [0.0] * 9]))
    if lib.cddp_hip_device_count() == 0:
        with pytest.raises(api.HipError, match="no HIP device"):
            api.DevicePlant.of_problem(p, 4, substeps=3, integrator=api.RK4)


def test_facade_takes_a_plant(api):
    import importlib.util, inspect, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    sig = inspect.signature(mod.CDDP.solve_mpc_batch)
    assert sig.parameters["plant"].default is None and sig.parameters["disturbances"].default is None
    sv = mod.CDDP([0.0, 0.0], [0.0, 0.0], 10, 0.02)
    with pytest.raises(ValueError):
        sv.solve_mpc_batch([[0.0, 0.0]], 2, disturbances=np.zeros((1, 2, 2)))     # disturbances need a plant
    with pytest.raises(ValueError):
        sv.solve_mpc_batch([[0.0, 0.0]], 2, plant={"no_such_key": 1})
