"""ctypes binding of the C-ABI in include/cddp_hip.h.

Builds `cddp_hip_problem` descriptors (the POD twin of cddp::CDDP, reference
include/cddp-cpp/cddp_core/cddp_core.hpp:215-423) and calls cddp-cpp_amd/lib/libcddp_hip.so (`HipBatchSolver`; fails
loudly if the library or a GPU is missing).  It contains no solver arithmetic and knows nothing about the CPU checker:
the tests / bench.py's cpu_baseline hang that on this namespace themselves.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
HIP_LIB_PATH = os.environ.get("CDDP_HIP_LIB") or os.path.join(_HERE, "lib", "libcddp_hip.so")   # override: kernel experiments

ABI_VERSION = 5          # CDDP_HIP_ABI_VERSION of include/cddp_hip.h
MAX_MODEL_PARAMS = 24
NAME_LEN = 48

# enums (include/cddp_hip.h)
MODEL_PENDULUM, MODEL_CARTPOLE, MODEL_UNICYCLE, MODEL_LTI = 0, 1, 2, 3
MODEL_QUADROTOR, MODEL_MANIPULATOR, MODEL_QUADROTOR_EULER12, MODEL_MANIPULATOR7 = 4, 5, 6, 7
MODEL_BICYCLE, MODEL_CAR, MODEL_HCW = 8, 9, 10
MODEL_EULER_ATTITUDE, MODEL_QUATERNION_ATTITUDE, MODEL_MRP_ATTITUDE = 11, 12, 13
MODEL_SPACECRAFT_TWOBODY, MODEL_SPACECRAFT_LANDING2D = 14, 15
MODEL_DUBINS_CAR, MODEL_DREYFUS_ROCKET, MODEL_ACROBOT, MODEL_USV_3DOF, MODEL_FORKLIFT = 16, 17, 18, 19, 20
MODEL_QUADROTOR_RATE, MODEL_SPACECRAFT_LINEAR_FUEL, MODEL_SPACECRAFT_NONLINEAR = 21, 22, 23
EULER, HEUN, RK3, RK4 = 0, 1, 2, 3
SOLVER_CLDDP, SOLVER_IPDDP, SOLVER_LOGDDP, SOLVER_MSIPDDP = 0, 1, 2, 3
CON_CONTROL_BOX, CON_STATE_BOX, CON_BALL, CON_LINEAR = 0, 1, 2, 3
CON_SOC, CON_THRUST, CON_MAX_THRUST = 4, 5, 6
TERM_EQUALITY, TERM_INEQUALITY = 0, 1
STATUS_RUNNING, STATUS_OPTIMAL, STATUS_ACCEPTABLE, STATUS_MAX_ITERATIONS, STATUS_REG_LIMIT, STATUS_MAX_CPU_TIME, STATUS_REG_LIMIT_CONVERGED = range(7)
STATUS_STRINGS = [
    "Running", "OptimalSolutionFound", "AcceptableSolutionFound", "MaxIterationsReached",
    "RegularizationLimitReached_NotConverged", "MaxCpuTimeReached", "RegularizationLimitReached_Converged",
]

_dp = C.POINTER(C.c_double)


class Options(C.Structure):
    _fields_ = [
        ("tolerance", C.c_double), ("acceptable_tolerance", C.c_double),
        ("max_iterations", C.c_int32), ("use_ilqr", C.c_int32), ("enable_parallel", C.c_int32),
        ("return_iteration_info", C.c_int32), ("warm_start", C.c_int32), ("_pad0", C.c_int32),
        ("termination_scaling_max_factor", C.c_double),
        ("ls_max_iterations", C.c_int32), ("_pad1", C.c_int32),
        ("ls_initial_step_size", C.c_double), ("ls_min_step_size", C.c_double),
        ("ls_step_reduction_factor", C.c_double),
        ("reg_initial_value", C.c_double), ("reg_update_factor", C.c_double),
        ("reg_max_value", C.c_double), ("reg_min_value", C.c_double),
        ("boxqp_max_iterations", C.c_int32), ("_pad2", C.c_int32),
        ("boxqp_min_gradient_norm", C.c_double), ("boxqp_min_relative_improvement", C.c_double),
        ("boxqp_step_decrease_factor", C.c_double), ("boxqp_min_step_size", C.c_double),
        ("boxqp_armijo_constant", C.c_double),
        ("filter_merit_acceptance_threshold", C.c_double),
        ("filter_violation_acceptance_threshold", C.c_double),
        ("filter_max_violation_threshold", C.c_double),
        ("filter_min_violation_for_armijo_check", C.c_double),
        ("filter_armijo_constant", C.c_double),
        ("ipddp_dual_var_init_scale", C.c_double), ("ipddp_slack_var_init_scale", C.c_double),
        ("ipddp_barrier_tol_mult", C.c_double), ("ipddp_barrier_update_dual_weight", C.c_double),
        ("ipddp_mu_kappa_epsilon", C.c_double),
        ("ipddp_check_state_stationarity", C.c_int32), ("ipddp_theta_norm_l2", C.c_int32),
        ("ipddp_max_filter_size", C.c_int32), ("ipddp_warmstart_repair", C.c_int32),
        ("ipddp_theta_0_floor", C.c_double), ("ipddp_warmstart_s_min", C.c_double),
        ("ipddp_warmstart_y_min", C.c_double), ("ipddp_warmstart_interior_factor", C.c_double),
        ("ipddp_jacobian_regularization_value", C.c_double),
        ("ipddp_jacobian_regularization_exponent", C.c_double),
        ("barrier_mu_initial", C.c_double), ("barrier_mu_min_value", C.c_double),
        ("barrier_mu_update_factor", C.c_double), ("barrier_mu_update_power", C.c_double),
        ("barrier_min_fraction_to_boundary", C.c_double),
        ("barrier_strategy", C.c_int32), ("_pad3", C.c_int32),
        ("max_cpu_time", C.c_double),
        ("logddp_mu_initial", C.c_double), ("logddp_mu_min_value", C.c_double), ("logddp_mu_update_factor", C.c_double),
        ("logddp_relaxed_delta", C.c_double),
        ("msipddp_costate_var_init_scale", C.c_double), ("msipddp_segment_length", C.c_int32), ("msipddp_rollout_type", C.c_int32),
        ("msipddp_use_controlled_rollout", C.c_int32), ("_pad4", C.c_int32),
    ]


def default_options():
    """Reference defaults: include/cddp-cpp/cddp_core/options.hpp:41-251, boxqp.hpp:30-41."""
    o = Options()
    o.tolerance = 1e-5; o.acceptable_tolerance = 1e-6; o.max_iterations = 1; o.use_ilqr = 1
    o.enable_parallel = 0; o.return_iteration_info = 0; o.warm_start = 0
    o.termination_scaling_max_factor = 100.0
    o.ls_max_iterations = 11; o.ls_initial_step_size = 1.0; o.ls_min_step_size = 1e-8
    o.ls_step_reduction_factor = 0.5
    o.reg_initial_value = 1e-6; o.reg_update_factor = 10.0; o.reg_max_value = 1e7; o.reg_min_value = 1e-10
    o.boxqp_max_iterations = 100; o.boxqp_min_gradient_norm = 1e-8
    o.boxqp_min_relative_improvement = 1e-8; o.boxqp_step_decrease_factor = 0.6
    o.boxqp_min_step_size = 1e-22; o.boxqp_armijo_constant = 0.1
    o.filter_merit_acceptance_threshold = 1e-6; o.filter_violation_acceptance_threshold = 1e-6
    o.filter_max_violation_threshold = 1e4; o.filter_min_violation_for_armijo_check = 1e-7
    o.filter_armijo_constant = 1e-4
    o.ipddp_dual_var_init_scale = 0.1; o.ipddp_slack_var_init_scale = 1e-2
    o.ipddp_barrier_tol_mult = 0.1; o.ipddp_barrier_update_dual_weight = 0.01
    o.ipddp_mu_kappa_epsilon = 10.0; o.ipddp_check_state_stationarity = 0; o.ipddp_theta_norm_l2 = 0
    o.ipddp_max_filter_size = 5; o.ipddp_warmstart_repair = 0; o.ipddp_theta_0_floor = 1.0
    o.ipddp_warmstart_s_min = 1e-4; o.ipddp_warmstart_y_min = 1e-4
    o.ipddp_warmstart_interior_factor = 1.1
    o.ipddp_jacobian_regularization_value = 1e-8; o.ipddp_jacobian_regularization_exponent = 0.25
    o.barrier_mu_initial = 1.0; o.barrier_mu_min_value = 1e-10; o.barrier_mu_update_factor = 0.5
    o.barrier_mu_update_power = 1.2; o.barrier_min_fraction_to_boundary = 0.99; o.barrier_strategy = 0
    o.max_cpu_time = 0.0
    o.logddp_mu_initial = 1.0; o.logddp_mu_min_value = 1e-10; o.logddp_mu_update_factor = 0.5; o.logddp_relaxed_delta = 1e-10
    o.msipddp_costate_var_init_scale = 1e-6; o.msipddp_segment_length = 5; o.msipddp_rollout_type = 0; o.msipddp_use_controlled_rollout = 0
    return o


class Constraint(C.Structure):
    _fields_ = [
        ("name", C.c_char * NAME_LEN), ("kind", C.c_int32), ("dim", C.c_int32),
        ("lower", _dp), ("upper", _dp), ("center", _dp), ("A", _dp), ("b", _dp),
        ("radius", C.c_double), ("scale", C.c_double),
    ]


class TerminalConstraint(C.Structure):
    _fields_ = [
        ("name", C.c_char * NAME_LEN), ("kind", C.c_int32), ("dim", C.c_int32),
        ("target", _dp), ("A", _dp), ("b", _dp),
    ]


class ProblemStruct(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("solver", C.c_int32), ("model", C.c_int32), ("integrator", C.c_int32),
        ("nx", C.c_int32), ("nu", C.c_int32), ("horizon", C.c_int32), ("_pad0", C.c_int32),
        ("dt", C.c_double), ("model_params", C.c_double * MAX_MODEL_PARAMS),
        ("lti_A", _dp), ("lti_B", _dp),
        ("Q", _dp), ("R", _dp), ("Qf", _dp), ("x_ref", _dp), ("x_ref_traj", _dp),
        ("n_constraints", C.c_int32), ("n_terminal", C.c_int32),
        ("constraints", C.POINTER(Constraint)), ("terminal", C.POINTER(TerminalConstraint)),
        ("options", Options),
    ]


class Result(C.Structure):
    _fields_ = [
        ("final_objective", C.c_double), ("merit_function", C.c_double),
        ("inf_pr", C.c_double), ("inf_du", C.c_double), ("inf_comp", C.c_double),
        ("barrier_mu", C.c_double), ("regularization", C.c_double),
        ("alpha_pr", C.c_double), ("alpha_du", C.c_double), ("step_norm", C.c_double),
        ("iterations", C.c_int32), ("status", C.c_int32), ("n_backward", C.c_int32), ("n_forward", C.c_int32),
    ]


RESULT_DTYPE = np.dtype([
    ("final_objective", "f8"), ("merit_function", "f8"), ("inf_pr", "f8"), ("inf_du", "f8"),
    ("inf_comp", "f8"), ("barrier_mu", "f8"), ("regularization", "f8"), ("alpha_pr", "f8"),
    ("alpha_du", "f8"), ("step_norm", "f8"), ("iterations", "i4"), ("status", "i4"),
    ("n_backward", "i4"), ("n_forward", "i4"),
])
TRIAL_DTYPE = np.dtype([
    ("alpha", "f8"), ("alpha_pr", "f8"), ("alpha_du", "f8"), ("cost", "f8"), ("merit_function", "f8"),
    ("theta", "f8"), ("inf_pr", "f8"), ("inf_comp", "f8"), ("success", "i4"), ("_pad", "i4"),
])
GATHER_DTYPE = np.dtype([("final_objective", "f8"), ("iterations", "i4"), ("status", "i4")])


TIMING_ROLLOUT, TIMING_ALL, TIMING_SWEEP = 0, 1, 2
# cddp_hip_mpc_advance / cddp_hip_mpc_run (include/cddp_hip.h, "device-resident MPC step")
MPC_KEEP_PLAN, MPC_SHIFT_EXISTING, MPC_SHIFT_PROVIDED = 0, 1, 2
MPC_SHIFT_DUALS, MPC_X_DEVICE = 1, 2
# cddp_hip_plan_jvp / cddp_hip_plan_vjp (include/cddp_hip.h, "linear response of a solved plan to its initial state")
SENS_DEVICE = 1
# cddp_hip_plan_covariance (include/cddp_hip.h, "state and control covariance along a solved plan")
COV_DEVICE, COV_DIAG, COV_PER_TRAJ = 1, 2, 4
# cddp_hip_plan_tvlqr (include/cddp_hip.h, "time-varying LQR tracking gains along a solved plan")
LQR_DEVICE, LQR_PER_TRAJ, LQR_INSTALL = 1, 2, 4
# cddp_hip_plan_kalman (include/cddp_hip.h, "Kalman filter gains and output-feedback covariance along a solved plan")
KF_DEVICE, KF_DIAG, KF_PER_TRAJ = 1, 2, 4
KF_MAX_NY = 16
# cddp_hip_score_rollouts / cddp_hip_seed_best (include/cddp_hip.h, "scoring candidate control sequences and seeding from the best")
SCORE_DEVICE = 1
SCORE_FEEDBACK = 2
SCORE_X0_PER_CANDIDATE = 4
# cddp_hip_sample_controls / cddp_hip_mppi_blend / cddp_hip_mppi_refine (include/cddp_hip.h, "sampling-based plan refinement")
MPPI_SEED = 8
# cddp_hip_mc_sample_noise / cddp_hip_plan_montecarlo (include/cddp_hip.h, "Monte-Carlo evaluation of a solved plan under noise")
MC_DEVICE, MC_DIAG = 1, 2
MC_MAX_SAMPLES = 1024
MC_STATS = ("n_finite", "n_viol", "cost_mean", "cost_var", "cost_min", "cost_max", "viol_mean", "viol_max")
MC_OUTPUTS = ("cost", "viol", "stats", "nviol_step", "dXmean", "SX", "dUmean", "SU", "X", "U")
# cddp_hip_mc_sample_meas_noise / cddp_hip_plan_montecarlo_of (include/cddp_hip.h, "Monte-Carlo evaluation of a solved plan under output feedback")
MCOF_OUTPUTS = MC_OUTPUTS + ("dEmean", "SE", "Xh")
# cddp_hip_get_field_device / cddp_hip_field_shape (include/cddp_hip.h, "device-resident inputs and outputs"): enum cddp_hip_field
FIELD_NAMES = ("X", "U", "K", "KFF", "VX", "VXX", "A", "B", "S", "Y", "G", "LAMBDA")
FIELD_IDS = {name: i for i, name in enumerate(FIELD_NAMES)}
# the columns of cddp_hip_get_results_device, in the order of cddp_hip_result
RESULT_DEVICE_COLS = ("final_objective", "merit_function", "inf_pr", "inf_du", "inf_comp", "barrier_mu", "regularization", "alpha_pr", "alpha_du", "step_norm")
RESULT_DEVICE_ICOLS = ("iterations", "status", "n_backward", "n_forward")


# cddp_hip_plant_* / cddp_hip_mpc_run_plant / cddp_hip_track_plan (include/cddp_hip.h, "closed loop against a separate plant")
PLANT_DEVICE = 1


class PlantDesc(C.Structure):   # cddp_hip_plant_desc
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32), ("integrator", C.c_int32), ("substeps", C.c_int32),
        ("nx", C.c_int32), ("nu", C.c_int32), ("params_per_trajectory", C.c_int32), ("_pad", C.c_int32),
        ("dt", C.c_double), ("model_params", _dp), ("lti_A", _dp), ("lti_B", _dp), ("u_lower", _dp), ("u_upper", _dp),
    ]


# cddp_hip_set_reference / cddp_hip_mpc_set_reference_path (include/cddp_hip.h, "moving the goal and the per-step reference of a live handle")
REF_DEVICE, REF_CLEAR_TRAJ = 1, 2


class RefPathDesc(C.Structure):   # cddp_hip_ref_path
    _fields_ = [
        ("abi_version", C.c_int32), ("flags", C.c_int32), ("rows", C.c_int64), ("start", C.c_int64),
        ("rows_per_step", C.c_double), ("path", C.c_void_p),   # (a host OR a device address, by the flag: a plain pointer value)
    ]


class MppiDesc(C.Structure):   # cddp_hip_mppi_desc
    _fields_ = [
        ("seed", C.c_uint64), ("stream", C.c_uint32), ("iters", C.c_int32), ("ncand", C.c_int32), ("keep_mean", C.c_int32),
        ("lam", C.c_double), ("viol_tol", C.c_double), ("sigma", _dp), ("u_lower", _dp), ("u_upper", _dp),
    ]


class McDesc(C.Structure):   # cddp_hip_mc_desc
    _fields_ = [
        ("seed", C.c_uint64), ("stream", C.c_uint32), ("nsamp", C.c_int32), ("keep_nominal", C.c_int32), ("_pad", C.c_int32),
        ("viol_tol", C.c_double), ("L0", _dp), ("Lw", _dp), ("Lu", _dp),
    ]


class McofDesc(C.Structure):   # cddp_hip_mcof_desc
    _fields_ = [("mc", McDesc), ("ny", C.c_int32), ("_pad", C.c_int32), ("C", _dp), ("v", _dp)]


# cddp_hip_ekf_* / cddp_hip_mpc_run_ekf (include/cddp_hip.h, "extended Kalman filter on the device; the MPC loop closed through it")
EKF_DEVICE, EKF_SKIP_NAN, EKF_PER_TRAJ, EKF_DIAG = 1, 2, 4, 8
MPC_EKF_SKIP_NAN = 256


class EkfDesc(C.Structure):   # cddp_hip_ekf_desc
    _fields_ = [("abi_version", C.c_int32), ("ny", C.c_int32), ("per_trajectory", C.c_int32), ("_pad", C.c_int32),
                ("C", _dp), ("v", _dp), ("W", _dp), ("Wu", _dp)]


class Stats(C.Structure):
    _fields_ = [
        ("solve_ms", C.c_double), ("backward_ms", C.c_double), ("forward_ms", C.c_double),
        ("update_ms", C.c_double), ("sweeps", C.c_int64), ("rollouts", C.c_int64),
        ("rollouts_launched", C.c_int64), ("traj_iterations", C.c_int64),
        ("outer_iterations", C.c_int32), ("n_converged", C.c_int32), ("kernel_launches", C.c_int32),
        ("timing_detail", C.c_int32), ("rollout_steps", C.c_int64),
    ]


def _arr(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


class Problem:
    """Python-side owner of a cddp_hip_problem descriptor (keeps the numpy buffers alive)."""

    def __init__(self, solver, model, integrator, nx, nu, horizon, dt, Q, R, Qf, x_ref,
                 model_params=(), lti_A=None, lti_B=None, x_ref_traj=None, options=None):
        self.keep = []
        self.c = ProblemStruct()
        self.c.abi_version = ABI_VERSION
        self.c.solver = solver; self.c.model = model; self.c.integrator = integrator
        self.c.nx = nx; self.c.nu = nu; self.c.horizon = horizon; self.c.dt = dt
        for i, v in enumerate(model_params):
            self.c.model_params[i] = float(v)
        self.Q = _arr(Q).reshape(nx, nx); self.R = _arr(R).reshape(nu, nu); self.Qf = _arr(Qf).reshape(nx, nx)
        self.x_ref = _arr(x_ref).reshape(nx)
        self.c.Q = _ptr(self.Q); self.c.R = _ptr(self.R); self.c.Qf = _ptr(self.Qf); self.c.x_ref = _ptr(self.x_ref)
        if lti_A is not None:
            self.lti_A = _arr(lti_A).reshape(nx, nx); self.lti_B = _arr(lti_B).reshape(nx, nu)
            self.c.lti_A = _ptr(self.lti_A); self.c.lti_B = _ptr(self.lti_B)
        if x_ref_traj is not None:
            self.x_ref_traj = _arr(x_ref_traj).reshape(horizon + 1, nx)
            self.c.x_ref_traj = _ptr(self.x_ref_traj)
        self.c.options = options if options is not None else default_options()
        self._cons = []
        self._terms = []
        self.nx, self.nu, self.N, self.dt = nx, nu, horizon, dt

    @property
    def options(self):
        return self.c.options

    def _rebuild(self):
        if self._cons:
            arr = (Constraint * len(self._cons))(*self._cons)
            self._cons_arr = arr
            self.c.constraints = C.cast(arr, C.POINTER(Constraint)); self.c.n_constraints = len(self._cons)
        else:
            self.c.n_constraints = 0
        if self._terms:
            arr = (TerminalConstraint * len(self._terms))(*self._terms)
            self._terms_arr = arr
            self.c.terminal = C.cast(arr, C.POINTER(TerminalConstraint)); self.c.n_terminal = len(self._terms)
        else:
            self.c.n_terminal = 0

    def add_control_box(self, name, lower, upper, scale=1.0):
        lo, up = _arr(lower), _arr(upper); self.keep += [lo, up]
        c = Constraint(); c.name = name.encode(); c.kind = CON_CONTROL_BOX; c.dim = lo.size
        c.lower = _ptr(lo); c.upper = _ptr(up); c.scale = scale
        self._cons.append(c); self._rebuild(); return self

    def add_state_box(self, name, lower, upper, scale=1.0):
        lo, up = _arr(lower), _arr(upper); self.keep += [lo, up]
        c = Constraint(); c.name = name.encode(); c.kind = CON_STATE_BOX; c.dim = lo.size
        c.lower = _ptr(lo); c.upper = _ptr(up); c.scale = scale
        self._cons.append(c); self._rebuild(); return self

    def add_ball(self, name, radius, center, scale=1.0):
        ce = _arr(center); self.keep += [ce]
        c = Constraint(); c.name = name.encode(); c.kind = CON_BALL; c.dim = ce.size
        c.center = _ptr(ce); c.radius = radius; c.scale = scale
        self._cons.append(c); self._rebuild(); return self

    def add_linear(self, name, A, b):
        A_, b_ = _arr(A), _arr(b); self.keep += [A_, b_]
        c = Constraint(); c.name = name.encode(); c.kind = CON_LINEAR; c.dim = b_.size
        c.A = _ptr(A_); c.b = _ptr(b_); c.scale = 1.0
        self._cons.append(c); self._rebuild(); return self

    def add_second_order_cone(self, name, cone_origin, opening_direction, cone_angle_fov, regularization_epsilon=1e-6):
        """SecondOrderConeConstraint (constraint.hpp:626-668): the constructor's checks and normalisation happen here."""
        if cone_angle_fov < 0 or cone_angle_fov > np.pi:
            raise ValueError("SecondOrderConeConstraint: Cone angle must be between 0 and PI.")
        if regularization_epsilon <= 0:
            raise ValueError("SecondOrderConeConstraint: Regularization epsilon must be positive.")
        o = _arr(cone_origin).reshape(3); a = _arr(opening_direction).reshape(3)
        n = float(np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))
        if n == 0.0:
            raise ValueError("SecondOrderConeConstraint: Opening direction cannot be zero vector.")
        a = a / n
        self.keep += [o, a]
        c = Constraint(); c.name = name.encode(); c.kind = CON_SOC; c.dim = 3
        c.center = _ptr(o); c.lower = _ptr(a); c.radius = float(np.cos(cone_angle_fov)); c.scale = regularization_epsilon
        self._cons.append(c); self._rebuild(); return self

    def add_thrust_magnitude(self, name, min_thrust_norm, max_thrust_norm, epsilon=1e-6):
        """ThrustMagnitudeConstraint (constraint.hpp:802-838)."""
        if min_thrust_norm < 0.0:
            raise ValueError("ThrustMagnitudeConstraint: min_thrust_norm must be non-negative.")
        if max_thrust_norm < min_thrust_norm:
            raise ValueError("ThrustMagnitudeConstraint: max_thrust_norm must be greater than or equal to min_thrust_norm.")
        if epsilon <= 0.0:
            raise ValueError("ThrustMagnitudeConstraint: epsilon must be positive.")
        mn = _arr([min_thrust_norm]); self.keep += [mn]
        c = Constraint(); c.name = name.encode(); c.kind = CON_THRUST; c.dim = self.nu
        c.lower = _ptr(mn); c.radius = max_thrust_norm; c.scale = epsilon
        self._cons.append(c); self._rebuild(); return self

    def add_max_thrust_magnitude(self, name, max_thrust_norm, epsilon=1e-6):
        """MaxThrustMagnitudeConstraint (constraint.hpp:929-953)."""
        if max_thrust_norm < 0.0:
            raise ValueError("MaxThrustMagnitudeConstraint: max_thrust_norm must be non-negative.")
        if epsilon <= 0.0:
            raise ValueError("MaxThrustMagnitudeConstraint: epsilon must be positive.")
        c = Constraint(); c.name = name.encode(); c.kind = CON_MAX_THRUST; c.dim = self.nu
        c.radius = max_thrust_norm; c.scale = epsilon
        self._cons.append(c); self._rebuild(); return self

    def add_terminal_equality(self, name, target):
        t_ = _arr(target); self.keep += [t_]
        c = TerminalConstraint(); c.name = name.encode(); c.kind = TERM_EQUALITY; c.dim = t_.size; c.target = _ptr(t_)
        self._terms.append(c); self._rebuild(); return self

    def add_terminal_inequality(self, name, A, b):
        A_, b_ = _arr(A), _arr(b); self.keep += [A_, b_]
        c = TerminalConstraint(); c.name = name.encode(); c.kind = TERM_INEQUALITY; c.dim = b_.size
        c.A = _ptr(A_); c.b = _ptr(b_)
        self._terms.append(c); self._rebuild(); return self

    def dual_dim(self):
        m = 0
        for c in self._cons:
            m += {CON_CONTROL_BOX: 2 * c.dim, CON_STATE_BOX: 2 * c.dim, CON_BALL: 1, CON_LINEAR: c.dim, CON_SOC: 1, CON_THRUST: 2, CON_MAX_THRUST: 1}[c.kind]
        return m


# ----------------------------------------------------------------------------------------------
# Problem builders for the BASELINE configs; constants from the
# reference examples (examples/cddp_pendulum.cpp:24-65, cddp_cartpole.cpp:24-66,
# cddp_unicycle.cpp / python_portfolio_lib.py:374-446, cddp_quadrotor_point.cpp:22-96,
# cddp_manipulator.cpp:22-68).
# ----------------------------------------------------------------------------------------------
def pendulum_problem(solver=SOLVER_IPDDP, constrained=True, horizon=100):
    o = default_options(); o.max_iterations = 30; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-5
    o.reg_initial_value = 1e-6
    dt = 0.02
    p = Problem(solver, MODEL_PENDULUM, EULER, 2, 1, horizon, dt, np.zeros((2, 2)), 0.1 * np.eye(1),
                100.0 * np.eye(2), [0.0, 0.0], model_params=[0.5, 1.0, 0.01, 9.81], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-20.0], [20.0])
    p.x0 = np.array([np.pi, 0.0])
    return p


def cartpole_problem(solver=SOLVER_IPDDP, constrained=True, horizon=100):
    o = default_options(); o.max_iterations = 80; o.tolerance = 1e-6; o.acceptable_tolerance = 1e-5
    o.reg_initial_value = 1e-5
    dt = 0.05
    p = Problem(solver, MODEL_CARTPOLE, RK4, 4, 1, horizon, dt, np.zeros((4, 4)), 0.1 * np.eye(1),
                100.0 * np.eye(4), [0.0, np.pi, 0.0, 0.0], model_params=[1.0, 0.2, 0.5, 9.81, 0.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-5.0], [5.0])
    p.x0 = np.zeros(4)
    return p


def unicycle_problem(solver=SOLVER_IPDDP, horizon=200, obstacle=True):
    o = default_options(); o.max_iterations = 100; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.03
    p = Problem(solver, MODEL_UNICYCLE, EULER, 3, 2, horizon, dt, np.zeros((3, 3)), 0.05 * np.eye(2),
                np.diag([100.0, 100.0, 50.0]), [2.0, 2.0, np.pi / 2], options=o)
    p.add_control_box("control_limits", [-1.1, -np.pi], [1.1, np.pi])
    if obstacle:
        p.add_ball("obstacle", 0.4, [1.0, 1.0])
    p.x0 = np.array([0.0, 0.0, np.pi / 4])
    p.U0_const = np.array([0.5, 0.1])
    return p


def hcw_problem(solver=SOLVER_IPDDP, horizon=80, constrained=True, integrator=None):
    """Hill-Clohessy-Wiltshire rendezvous (src/dynamics_model/spacecraft_linear.cpp; orbit of tests/dynamics_model/test_spacecraft_linear.cpp:
    500 km altitude, dt = 10 s, m = 1 kg as its DiscreteDynamics case): from its drifting initial state to the origin, thrust box."""
    o = default_options(); o.max_iterations = 40; o.tolerance = 1e-5; o.acceptable_tolerance = 1e-6; o.reg_initial_value = 1e-6
    n = float(np.sqrt(3.986004418e14 / (6371e3 + 500e3) ** 3))
    dt = 10.0
    p = Problem(solver, MODEL_HCW, RK4 if integrator is None else integrator, 6, 3, horizon, dt, np.diag([1e-4] * 3 + [1e-2] * 3), 1.0 * np.eye(3),
                np.diag([10.0] * 3 + [100.0] * 3), np.zeros(6), model_params=[n, 1.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", -0.5 * np.ones(3), 0.5 * np.ones(3))
    p.x0 = np.array([-37.59664132226163, 27.312455860666148, 13.656227930333074, 0.015161970413423813, 0.08348413138390476, 0.04174206569195238])
    return p


def bicycle_problem(solver=SOLVER_IPDDP, horizon=100, constrained=True, integrator=None):
    """Kinematic bicycle (src/dynamics_model/bicycle.cpp; constants of tests/dynamics_model/test_bicycle.cpp:28-40: dt 0.05, wheelbase
    2): drive from the origin to (2, 1, pi/4) at rest; state [x, y, theta, v], control [a, delta]."""
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.05
    p = Problem(solver, MODEL_BICYCLE, EULER if integrator is None else integrator, 4, 2, horizon, dt, np.zeros((4, 4)), np.diag([0.05, 0.5]),
                np.diag([100.0, 100.0, 50.0, 10.0]), [2.0, 1.0, np.pi / 4, 0.0], model_params=[2.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-2.0, -0.5], [2.0, 0.5])
    p.x0 = np.array([0.0, 0.0, 0.0, 0.5])
    p.U0_const = np.array([0.1, 0.05])
    return p


def car_problem(solver=SOLVER_IPDDP, horizon=100, constrained=True):
    """The reference's car (src/dynamics_model/car.cpp, a DISCRETE plant; dt 0.03, wheelbase 2, control box +-[0.5, 2] of
    tests/cddp_core/test_ipddp_solver.cpp:686-750) with a QUADRATIC parking cost, so that the device-resident solve can be compared with
    the oracle (the reference's own test pairs it with a user NonlinearObjective: that shape runs through the plug-in solve)."""
    o = default_options(); o.max_iterations = 80; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    o.reg_initial_value = 1e-2
    dt = 0.03
    p = Problem(solver, MODEL_CAR, EULER, 4, 2, horizon, dt, np.diag([1e-2, 1e-2, 0.0, 0.0]), np.diag([1e-2, 1e-4]),
                np.diag([10.0, 10.0, 10.0, 3.0]), [0.0, 0.0, 0.0, 0.0], model_params=[2.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-0.5, -2.0], [0.5, 2.0])
    p.x0 = np.array([1.0, 1.0, 1.5 * np.pi, 0.0])
    p.U0_const = np.array([0.01, 0.1])
    return p


def unicycle_cone_problem(solver=SOLVER_IPDDP, horizon=100):
    """Unicycle with a control box and a SecondOrderConeConstraint on (x, y, theta) (constraint.hpp:626-800; geometry of
    tests/cddp_core/test_constraint.cpp:236-243: a 45-degree cone opening along +y from below the start), m = 5."""
    p = unicycle_problem(solver, horizon, obstacle=False)
    p._cons[0].name = b"ControlConstraint"; p._rebuild()   # std::map order: "ControlConstraint" < "SecondOrderConeConstraint" (the device layout); 'S' < 'c'
    p.add_second_order_cone("SecondOrderConeConstraint", [0.0, -0.5, 0.0], [0.0, 1.0, 0.0], np.pi / 4.0 + 0.35, 1e-6)
    return p


def unicycle_thrust_problem(solver=SOLVER_IPDDP, horizon=100, two_sided=True):
    """Unicycle whose control norm |(v, omega)| is bounded by the thrust-magnitude rows (constraint.hpp:802-1048): the two-sided
    ThrustMagnitudeConstraint (m = 2) or MaxThrustMagnitudeConstraint (m = 1) under the reference names.  Weights chosen so that the
    reference algorithm converges: IPDDP linearises path constraints to first order only (no constraint Hessians in
    ipddp_solver.cpp), and with a norm bound that ends up ACTIVE its iterates do not settle (oracle and twin agree on that)."""
    o = default_options(); o.max_iterations = 100; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.03
    p = Problem(solver, MODEL_UNICYCLE, EULER, 3, 2, horizon, dt, np.zeros((3, 3)), (0.5 if two_sided else 2.0) * np.eye(2),
                np.diag([10.0, 10.0, 5.0]), [2.0, 2.0, np.pi / 2], options=o)
    if two_sided:
        p.add_thrust_magnitude("ThrustMagnitudeConstraint", 0.3, 2.0, 1e-6)
    else:
        p.add_max_thrust_magnitude("MaxThrustMagnitudeConstraint", 2.0, 1e-6)
    p.x0 = np.array([0.0, 0.0, np.pi / 4])
    p.U0_const = np.array([0.5, 0.1])
    return p


def scalar_integrator_problem(horizon=8, path_constraint=False, terminal_inequality=False,
                              terminal_equality=False, options=None, solver=SOLVER_IPDDP):
    """LTI A=B=1 problems of tests/cddp_core/test_ipddp_solver.cpp:137-242, 1147-1637."""
    o = options if options is not None else default_options()
    p = Problem(solver, MODEL_LTI, EULER, 1, 1, horizon, 1.0, np.zeros((1, 1)), 1e-2 * np.eye(1),
                100.0 * np.eye(1), [1.0], lti_A=np.eye(1), lti_B=np.eye(1), options=o)
    if path_constraint:
        p.add_control_box("ControlConstraint", [-0.5], [0.5])
    if terminal_inequality:
        p.add_terminal_inequality("TerminalUpperBound", np.eye(1), np.zeros(1))
    if terminal_equality:
        p.add_terminal_equality("TerminalEquality", [0.0])
    p.x0 = np.zeros(1)
    return p


def quadrotor_problem(solver=SOLVER_IPDDP, horizon=120, constrained=True):
    o = default_options(); o.max_iterations = 120; o.ls_max_iterations = 15; o.reg_initial_value = 1e-4
    dt = 0.02
    Q = np.zeros((13, 13)); Q[4, 4] = Q[5, 5] = Q[6, 6] = 0.1
    R = 0.1 * np.eye(4)
    Qf = np.zeros((13, 13))
    for i in range(3): Qf[i, i] = 500.0
    for i in range(3, 7): Qf[i, i] = 1.0
    for i in range(7, 10): Qf[i, i] = 10.0
    goal = np.zeros(13); goal[0] = 3.0; goal[2] = 2.0; goal[3] = 1.0
    p = Problem(solver, MODEL_QUADROTOR, RK4, 13, 4, horizon, dt, Q, R, Qf, goal,
                model_params=[1.0, 0.2, 0.01, 0.01, 0.02, 9.81], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", np.zeros(4), 5.0 * np.ones(4))
    x0 = np.zeros(13); x0[3] = 1.0
    p.x0 = x0
    p.U0_const = (1.0 * 9.81 / 4.0) * np.ones(4)
    return p


def quadrotor_figure8_problem(solver=SOLVER_IPDDP, horizon=400):
    """The reference's own N = 400 quadrotor case: figure-8 tracking with per-step reference states
    (tests/cddp_core/test_ipddp_solver.cpp:887-1080, test_clddp_solver.cpp:570-763): m = 1.2, arm = 0.165, u in [0, 4]^4,
    Q = Qf = diag(1 x 7, 0 x 6), R = 0.01 I, hover U0, X0 = hover rollout.  It exercises the time-varying-reference branch of
    QuadraticObjective (objective.cpp:83-88)."""
    o = default_options(); o.tolerance = 1e-6; o.reg_initial_value = 1e-4; o.return_iteration_info = 1
    if solver == SOLVER_IPDDP:
        o.max_iterations = 500; o.acceptable_tolerance = 1e-5
    else:
        o.max_iterations = 200; o.acceptable_tolerance = 1e-6
    dt = 0.02
    Q = np.zeros((13, 13))
    for i in range(7): Q[i, i] = 1.0
    R = 0.01 * np.eye(4); Qf = Q.copy()
    omega = 2.0 * np.pi / (horizon * dt)
    ref = np.zeros((horizon + 1, 13))
    for i in range(horizon + 1):
        a = omega * (i * dt)
        ref[i, 0] = 3.0 * np.cos(a); ref[i, 1] = 3.0 * np.sin(a) * np.cos(a); ref[i, 2] = 2.0; ref[i, 3] = 1.0
    goal = np.zeros(13); goal[0] = 3.0; goal[2] = 2.0; goal[3] = 1.0
    p = Problem(solver, MODEL_QUADROTOR, RK4, 13, 4, horizon, dt, Q, R, Qf, goal,
                model_params=[1.2, 0.165, 7.782e-3, 7.782e-3, 1.439e-2, 9.81], x_ref_traj=ref, options=o)
    p.add_control_box("ControlConstraint", np.zeros(4), 4.0 * np.ones(4))
    p.x0 = goal.copy()
    p.U0_const = (1.2 * 9.81 / 4.0) * np.ones(4)
    return p


def quadrotor12_problem(solver=SOLVER_IPDDP, horizon=400, constrained=True):
    """SYNTHETIC throughput shape of BASELINE config 4 (nx=12, nu=4, N=400)."""
    o = default_options(); o.max_iterations = 120; o.ls_max_iterations = 15; o.reg_initial_value = 1e-4
    dt = 0.02
    Q = np.zeros((12, 12)); Q[6, 6] = Q[7, 7] = Q[8, 8] = 0.1
    R = 0.1 * np.eye(4)
    Qf = np.diag([500.0] * 3 + [10.0] * 3 + [1.0] * 3 + [0.0] * 3)
    goal = np.zeros(12); goal[0] = 3.0; goal[2] = 2.0
    p = Problem(solver, MODEL_QUADROTOR_EULER12, RK4, 12, 4, horizon, dt, Q, R, Qf, goal,
                model_params=[1.0, 0.2, 0.01, 0.01, 0.02, 9.81], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", np.zeros(4), 5.0 * np.ones(4))
    p.x0 = np.zeros(12)
    p.U0_const = (1.0 * 9.81 / 4.0) * np.ones(4)
    return p


def manipulator_problem(solver=SOLVER_IPDDP, horizon=160, terminal_equality=False, constrained=True):
    """examples/cddp_manipulator.cpp:22-68 (3-DOF, rk4, FD Jacobians; X0 = linear interpolation)."""
    o = default_options(); o.max_iterations = 80; o.ls_max_iterations = 20
    dt = 0.01
    goal = np.array([np.pi, -np.pi / 6, -np.pi / 3, 0.0, 0.0, 0.0])
    Q = np.diag([1.0, 1.0, 1.0, 0.1, 0.1, 0.1]); R = 0.1 * np.eye(3); Qf = 100.0 * Q
    p = Problem(solver, MODEL_MANIPULATOR, RK4, 6, 3, horizon, dt, Q, R, Qf, goal, options=o)
    if constrained:
        p.add_control_box("ControlConstraint", -50.0 * np.ones(3), 50.0 * np.ones(3))
    if terminal_equality:
        p.add_terminal_equality("TerminalEquality", goal)
    p.x0 = np.array([0.0, -np.pi / 2, np.pi, 0.0, 0.0, 0.0])
    al = np.linspace(0.0, 1.0, horizon + 1)[:, None]
    p.X0_single = (1.0 - al) * p.x0[None, :] + al * goal[None, :]
    return p


def manipulator7_problem(solver=SOLVER_IPDDP, horizon=150, terminal_equality=True, n_alphas=16):
    """SYNTHETIC throughput shape of BASELINE config 5 (nx=14, nu=7, N=150)."""
    o = default_options(); o.max_iterations = 80; o.tolerance = 1e-5; o.acceptable_tolerance = 1e-5
    o.ls_max_iterations = n_alphas; o.enable_parallel = 1
    dt = 0.01
    goal = np.concatenate([np.array([0.6, -0.4, 0.5, -0.3, 0.4, -0.2, 0.3]), np.zeros(7)])
    Q = np.zeros((14, 14)); R = 0.01 * np.eye(7); Qf = 100.0 * np.eye(14)
    p = Problem(solver, MODEL_MANIPULATOR7, RK4, 14, 7, horizon, dt, Q, R, Qf, goal, options=o)
    p.add_control_box("ControlConstraint", -50.0 * np.ones(7), 50.0 * np.ones(7))
    if terminal_equality:
        p.add_terminal_equality("TerminalEquality", goal)
    p.x0 = np.zeros(14)
    return p


# ---- spacecraft plants (src/dynamics_model/{euler,quaternion,mrp}_attitude.cpp, spacecraft_twobody.cpp, spacecraft_landing2d.cpp)
ATTITUDE_INERTIA = ((1.0, 0.1, 0.0), (0.1, 1.5, 0.05), (0.0, 0.05, 2.0))   # a full (non-diagonal) inertia: every entry of I^-1 matters
_ATTITUDE = {"euler": (MODEL_EULER_ATTITUDE, 6), "quaternion": (MODEL_QUATERNION_ATTITUDE, 7), "mrp": (MODEL_MRP_ATTITUDE, 6)}


def attitude_problem(kind="euler", solver=SOLVER_IPDDP, horizon=60, constrained=True, integrator=None, inertia=ATTITUDE_INERTIA):
    """Rest-to-rest slew of a rigid body to the identity attitude, torque box +-1.  kind: "euler" (ZYX angles), "quaternion"
    ([qw, qx, qy, qz]) or "mrp"; the three start from the same rotation (yaw 0.3, pitch -0.2, roll 0.4).  model_params: the inertia
    matrix, row-major (the library appends its inverse)."""
    model, nx = _ATTITUDE[kind]
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-5; o.acceptable_tolerance = 1e-6
    dt = 0.1
    ypr = (0.3, -0.2, 0.4)
    cy, sy, cp, sp, cr, sr = (f(0.5 * a) for a in ypr for f in (np.cos, np.sin))
    q = np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])
    att = {"euler": np.array(ypr), "quaternion": q, "mrp": q[1:] / (1.0 + q[0])}[kind]
    goal = np.zeros(nx)
    if kind == "quaternion":
        goal[0] = 1.0
    Qf = np.diag([100.0] * (nx - 3) + [10.0] * 3)
    p = Problem(solver, model, RK4 if integrator is None else integrator, nx, 3, horizon, dt, np.zeros((nx, nx)), 0.1 * np.eye(3), Qf, goal,
                model_params=np.asarray(inertia, dtype=np.float64).reshape(9), options=o)
    if constrained:
        p.add_control_box("ControlConstraint", -np.ones(3), np.ones(3))
    p.x0 = np.concatenate([att, [0.0, 0.0, 0.0]])
    return p


def twobody_problem(solver=SOLVER_IPDDP, horizon=60, constrained=True, integrator=None):
    """Orbit correction about a central body in canonical units (mu = 1, mass 1, circular orbit of radius 1): from a perturbed state to
    the circular orbit's state at t = N dt, thrust box +-0.2."""
    o = default_options(); o.max_iterations = 40; o.tolerance = 1e-5; o.acceptable_tolerance = 1e-6
    dt = 0.05
    T = horizon * dt
    goal = np.array([np.cos(T), np.sin(T), 0.0, -np.sin(T), np.cos(T), 0.0])
    p = Problem(solver, MODEL_SPACECRAFT_TWOBODY, EULER if integrator is None else integrator, 6, 3, horizon, dt, np.zeros((6, 6)), np.eye(3),
                100.0 * np.eye(6), goal, model_params=[1.0, 1.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", -0.2 * np.ones(3), 0.2 * np.ones(3))
    p.x0 = np.array([1.02, -0.01, 0.01, 0.0, 0.98, 0.02])
    return p


LANDING2D_PARAMS = (100000.0, 50.0, 10.0, 880000.0, 2210000.0, 0.349066)   # spacecraft_landing2d.hpp:38-45 defaults


def landing2d_problem(solver=SOLVER_IPDDP, horizon=80, constrained=True, integrator=None):
    """Powered descent of the planar lander (state [x, x_dot, y, y_dot, theta, theta_dot], control [thrust fraction, gimbal angle]) to rest
    at the origin; box: thrust fraction in [min_thrust / max_thrust, 1], gimbal within +-max_gimble; starts from hover thrust."""
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.1
    mass, _, _, tmin, tmax, gmax = LANDING2D_PARAMS
    p = Problem(solver, MODEL_SPACECRAFT_LANDING2D, RK4 if integrator is None else integrator, 6, 2, horizon, dt, np.zeros((6, 6)),
                np.diag([1.0, 1.0]), np.diag([1e-2, 1e-1, 1e-2, 1e-1, 10.0, 10.0]), np.zeros(6), model_params=LANDING2D_PARAMS, options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [tmin / tmax, -gmax], [1.0, gmax])
    p.x0 = np.array([20.0, -2.0, 150.0, -15.0, 0.05, 0.0])
    p.U0_const = np.array([9.81 * mass / tmax, 0.0])
    return p


# ---- the remaining small plants (src/dynamics_model/{dubins_car,dreyfus_rocket,acrobot,usv_3dof,forklift,spacecraft_linear_fuel}.cpp)
def dubins_problem(solver=SOLVER_IPDDP, horizon=60, constrained=True, integrator=None):
    """Constant-speed Dubins car (state [x, y, theta], control [omega]; speed 1): a quarter turn to (3.8, 3.8, pi / 2), turn-rate box +-1;
    starts from a constant turn rate."""
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-5; o.acceptable_tolerance = 1e-6
    dt = 0.1
    p = Problem(solver, MODEL_DUBINS_CAR, EULER if integrator is None else integrator, 3, 1, horizon, dt, np.zeros((3, 3)), 0.1 * np.eye(1),
                np.diag([100.0, 100.0, 50.0]), [3.8, 3.8, np.pi / 2], model_params=[1.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-1.0], [1.0])
    p.x0 = np.zeros(3)
    p.U0_const = np.array([0.2])
    return p


def dreyfus_problem(solver=SOLVER_IPDDP, horizon=50, constrained=True, integrator=None):
    """Dreyfus rocket (state [x, x_dot], control [thrust angle]; thrust 64, gravity 32 as the reference's defaults): climb one unit and
    stop, thrust angle within [0.05, 3]; starts from the hover angle pi / 3."""
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-5; o.acceptable_tolerance = 1e-6
    dt = 0.01
    p = Problem(solver, MODEL_DREYFUS_ROCKET, RK4 if integrator is None else integrator, 2, 1, horizon, dt, np.zeros((2, 2)), 0.1 * np.eye(1),
                np.diag([100.0, 10.0]), [1.0, 0.0], model_params=[64.0, 32.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [0.05], [3.0])
    p.x0 = np.zeros(2)
    p.U0_const = np.array([np.pi / 3])
    return p


ACROBOT_PARAMS = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)   # acrobot.hpp:46-50 defaults: l1, l2, m1, m2, J1, J2


def acrobot_problem(solver=SOLVER_IPDDP, horizon=80, constrained=True, integrator=None):
    """Acrobot (state [theta1, theta2, theta1_dot, theta2_dot], torque on the second joint) from its hanging rest to a bent elbow,
    torque box +-10."""
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.02
    p = Problem(solver, MODEL_ACROBOT, RK4 if integrator is None else integrator, 4, 1, horizon, dt, np.zeros((4, 4)), 0.01 * np.eye(1),
                np.diag([100.0, 100.0, 10.0, 10.0]), [-np.pi / 2, 0.5, 0.0, 0.0], model_params=ACROBOT_PARAMS, options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-10.0], [10.0])
    p.x0 = np.array([-np.pi / 2, 0.0, 0.0, 0.0])
    return p


def usv_problem(solver=SOLVER_IPDDP, horizon=80, constrained=True, integrator=None):
    """3-DOF surface vessel (state [x, y, psi, u, v, r], control [tau_u, tau_v, tau_r]; the reference's fixed vessel, no parameters): from
    rest to (3, 2) with heading 0.3, force / moment box +-200.  (Under use_ilqr = 0 the tensor terms make Q_xx indefinite at the
    first iterate of this problem and the value recursion over 80 steps amplifies rounding: use a short horizon for full DDP.)"""
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.1
    p = Problem(solver, MODEL_USV_3DOF, RK4 if integrator is None else integrator, 6, 3, horizon, dt, np.zeros((6, 6)), 1e-4 * np.eye(3),
                np.diag([100.0, 100.0, 100.0, 10.0, 10.0, 10.0]), [3.0, 2.0, 0.3, 0.0, 0.0, 0.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-200.0] * 3, [200.0] * 3)
    p.x0 = np.zeros(6)
    return p


FORKLIFT_PARAMS = (2.0, 1.0, 0.785398)   # forklift.hpp:54-58 defaults: wheelbase, rear_steer, max_steering_angle


def forklift_problem(solver=SOLVER_IPDDP, horizon=100, constrained=True):
    """The reference's rear-steered forklift (a DISCRETE plant; state [x, y, theta, v, steering angle], control [acceleration, steering
    rate]): a lane change to (2, 1) with heading 0.5 at rest, box +-[1, 1].  (Under use_ilqr = 0 the first sweep over the 100 steps is
    ill-conditioned in the same way as usv_problem's, more mildly.)"""
    o = default_options(); o.max_iterations = 80; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.03
    p = Problem(solver, MODEL_FORKLIFT, EULER, 5, 2, horizon, dt, np.zeros((5, 5)), np.diag([0.1, 1.0]),
                np.diag([100.0, 100.0, 50.0, 10.0, 10.0]), [2.0, 1.0, 0.5, 0.0, 0.0], model_params=FORKLIFT_PARAMS, options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [-1.0, -1.0], [1.0, 1.0])
    p.x0 = np.array([0.0, 0.0, 0.0, 0.5, 0.0])
    p.U0_const = np.array([0.1, -0.05])
    return p


def linear_fuel_problem(solver=SOLVER_IPDDP, horizon=80, constrained=True, integrator=None):
    """The HCW rendezvous of hcw_problem with a mass state (state [x, y, z, vx, vy, vz, mass, accumulated control effort]; 1 kg, Isp 300 s):
    the mass and effort states carry no cost."""
    o = default_options(); o.max_iterations = 40; o.tolerance = 1e-5; o.acceptable_tolerance = 1e-6; o.reg_initial_value = 1e-6
    n = float(np.sqrt(3.986004418e14 / (6371e3 + 500e3) ** 3))
    dt = 10.0
    p = Problem(solver, MODEL_SPACECRAFT_LINEAR_FUEL, RK4 if integrator is None else integrator, 8, 3, horizon, dt,
                np.diag([1e-4] * 3 + [1e-2] * 3 + [0.0, 0.0]), 1.0 * np.eye(3), np.diag([10.0] * 3 + [100.0] * 3 + [0.0, 0.0]), np.zeros(8),
                model_params=[n, 300.0, 9.80665], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", -0.5 * np.ones(3), 0.5 * np.ones(3))
    p.x0 = np.array([-37.59664132226163, 27.312455860666148, 13.656227930333074, 0.015161970413423813, 0.08348413138390476, 0.04174206569195238,
                     1.0, 0.0])
    return p


QUADROTOR_RATE_PARAMS = (1.0, 20.0, 0.5)   # mass, max_thrust, max_rate (the constants of the reference's own test of the plant)


def quadrotor_rate_problem(solver=SOLVER_IPDDP, horizon=60, constrained=True, integrator=None):
    """Rate-controlled quadrotor (state [p, v, q = (qw, qx, qy, qz)], control [thrust, wx, wy, wz]): from hover at the origin to hover at
    (0.5, 0.3, 0.5), thrust within [0, max_thrust], body rates within +-max_rate; starts from the hover thrust."""
    o = default_options(); o.max_iterations = 60; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.05
    mass, max_thrust, max_rate = QUADROTOR_RATE_PARAMS
    goal = np.array([0.5, 0.3, 0.5, 0, 0, 0, 1.0, 0, 0, 0])
    p = Problem(solver, MODEL_QUADROTOR_RATE, RK4 if integrator is None else integrator, 10, 4, horizon, dt, np.zeros((10, 10)),
                np.diag([0.01, 0.1, 0.1, 0.1]), np.diag([100.0] * 3 + [10.0] * 3 + [10.0] * 4), goal, model_params=QUADROTOR_RATE_PARAMS, options=o)
    if constrained:
        p.add_control_box("ControlConstraint", [0.0, -max_rate, -max_rate, -max_rate], [max_thrust, max_rate, max_rate, max_rate])
    p.x0 = np.array([0.0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0])
    p.U0_const = np.array([mass * 9.81, 0.0, 0.0, 0.0])
    return p


def spacecraft_nonlinear_problem(solver=SOLVER_IPDDP, horizon=40, constrained=True, integrator=None):
    """Nonlinear relative motion in canonical units (mu = 1, circular reference orbit of radius 1, mass 1; state [p, v, r0, theta, dr0,
    dtheta]): null a small offset from the reference orbit, acceleration box +-0.3.  The four orbit states carry no cost.  No full DDP:
    use_ilqr = 0 is refused for this plant."""
    o = default_options(); o.max_iterations = 40; o.tolerance = 1e-4; o.acceptable_tolerance = 1e-6
    dt = 0.05
    p = Problem(solver, MODEL_SPACECRAFT_NONLINEAR, RK4 if integrator is None else integrator, 10, 3, horizon, dt, np.zeros((10, 10)), 0.1 * np.eye(3),
                np.diag([100.0] * 6 + [0.0] * 4), np.array([0.0] * 6 + [1.0, 0.0, 0.0, 1.0]), model_params=[1.0, 1.0, 1.0, 1.0], options=o)
    if constrained:
        p.add_control_box("ControlConstraint", -0.3 * np.ones(3), 0.3 * np.ones(3))
    p.x0 = np.array([0.02, -0.01, 0.01, 0.0, 0.01, 0.0, 1.0, 0.0, 0.0, 1.0])
    return p


def batch_x0(problem, batch, seed, spread=None):
    """Seeded per-trajectory x0 perturbations; trajectory 0 is the example."""
    rng = np.random.default_rng(seed)
    x0 = np.tile(problem.x0, (batch, 1)).astype(np.float64)
    if spread is None:
        spread = 0.1 * np.ones(problem.nx)
    pert = rng.uniform(-1.0, 1.0, size=(batch, problem.nx)) * np.asarray(spread)[None, :]
    pert[0] = 0.0
    return np.ascontiguousarray(x0 + pert)


def batch_U0(problem, batch):
    if hasattr(problem, "U0_const"):
        return np.ascontiguousarray(np.tile(problem.U0_const, (batch, problem.N, 1)).astype(np.float64))
    return None


# ----------------------------------------------------------------------------------------------
# Product binding
# ----------------------------------------------------------------------------------------------
_hip_libs = {}
# ONE library since round 4 (csrc/Makefile: every translation unit with -DCDDP_TRIG_SHARED): the plants' sin / cos / asin / tan and
# the solver core's log / pow are the straight-line routines of dev_trig.hpp -- the routines the CPU checker can run too (its
# trig_mode 1), which makes accept / reject decisions bit-comparable.  The `trig` arguments below are kept for callers written
# against rounds 1-3 (two libraries): None and "shared" name the library; "libm" is refused unless CDDP_HIP_LIB points at a
# hand-made device-libm experiment build (cddp_hip_trig_shared() == 0).


def default_trig():
    # (CDDP_HIP_LIB + CDDP_HIP_TRIG=libm: the hand-made device-libm comparison build of profiles/r04_trig_ab.md)
    return "libm" if (os.environ.get("CDDP_HIP_LIB") and os.environ.get("CDDP_HIP_TRIG") == "libm") else "shared"


def load_hip(trig=None):
    """Load the HIP C-ABI library.  Raises if it is missing: there is no fallback path."""
    trig = trig or default_trig()
    if trig not in ("shared", "libm"):
        raise ValueError("trig must be None, 'shared' or 'libm'")
    if "lib" not in _hip_libs:
        path = HIP_LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError("HIP library missing: %s -- run __graft_entry__.build(); "
                               "the product has no CPU fallback" % path)
        lib = C.CDLL(path)
        lib.cddp_hip_last_error.restype = C.c_char_p
        lib.cddp_hip_status_string.restype = C.c_char_p
        lib.cddp_hip_create.argtypes = [C.POINTER(ProblemStruct), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        lib.cddp_hip_mpc_advance.argtypes = MPC_ADVANCE_ARGTYPES; lib.cddp_hip_mpc_advance.restype = C.c_int
        lib.cddp_hip_mpc_run.argtypes = MPC_RUN_ARGTYPES; lib.cddp_hip_mpc_run.restype = C.c_int
        for name, at in list(PLANT_ARGTYPES.items()) + list(DEVICE_IO_ARGTYPES.items()):
            fn = getattr(lib, name); fn.argtypes = at; fn.restype = C.c_int
        _hip_libs["lib"] = lib
    lib = _hip_libs["lib"]
    if (trig == "shared") != bool(lib.cddp_hip_trig_shared()):
        raise RuntimeError("trig=%r asked for, but %s was built %s -DCDDP_TRIG_SHARED" %
                           (trig, HIP_LIB_PATH, "with" if lib.cddp_hip_trig_shared() else "without"))
    return lib


# (x_next is a host OR a device address: passed as a plain pointer value)
MPC_ADVANCE_ARGTYPES = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
MPC_RUN_ARGTYPES = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(Stats)]
# (cddp_hip_plant_step: x, u, w, x_next are host OR device addresses: plain pointer values)
PLANT_ARGTYPES = {
    "cddp_hip_plant_create": [C.POINTER(PlantDesc), C.c_int, C.c_int, C.POINTER(C.c_void_p)],
    "cddp_hip_plant_destroy": [C.c_void_p],
    "cddp_hip_plant_step": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_mpc_run_plant": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(Stats)],
    "cddp_hip_track_plan": [C.c_void_p, C.c_void_p, _dp, _dp, _dp, _dp],
    # (the arrays of the step entries are host OR device addresses, by the flag: plain pointer values)
    "cddp_hip_ekf_create": [C.c_void_p, C.POINTER(EkfDesc), C.POINTER(C.c_void_p)],
    "cddp_hip_ekf_destroy": [C.c_void_p],
    "cddp_hip_ekf_reset": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "cddp_hip_ekf_update": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "cddp_hip_ekf_predict": [C.c_void_p, C.c_int, C.c_void_p],
    "cddp_hip_ekf_get": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_ekf_run": [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6,
    "cddp_hip_mpc_run_ekf": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(Stats)],
}
# (device addresses: plain pointer values)
DEVICE_IO_ARGTYPES = {
    "cddp_hip_field_shape": [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "cddp_hip_get_field_device": [C.c_void_p, C.c_int, C.c_void_p],
    "cddp_hip_get_results_device": [C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_set_initial_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_get_live_slots": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    # (host or device addresses, by the flag: plain pointer values)
    "cddp_hip_plan_jvp": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_plan_vjp": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_plan_covariance": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_plan_tvlqr": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_plan_kalman": [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 12,
    "cddp_hip_score_rollouts": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_seed_best": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p],
    "cddp_hip_sample_controls": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_mppi_blend": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_mppi_refine": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_mc_sample_noise": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cddp_hip_plan_montecarlo": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 11,
    "cddp_hip_mc_sample_meas_noise": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "cddp_hip_plan_montecarlo_of": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 15,
    "cddp_hip_set_reference": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "cddp_hip_get_reference": [C.c_void_p, _dp, _dp, C.POINTER(C.c_int32)],
    "cddp_hip_mpc_set_reference_path": [C.c_void_p, C.POINTER(RefPathDesc)],
    "cddp_hip_mpc_reference_cursor": [C.c_void_p, C.POINTER(C.c_int64)],
}

EXPORTED_SYMBOLS = [
    "cddp_hip_default_options", "cddp_hip_abi_version", "cddp_hip_trig_shared", "cddp_hip_last_error", "cddp_hip_device_count",
    "cddp_hip_status_string", "cddp_hip_build_alphas", "cddp_hip_create", "cddp_hip_destroy",
    "cddp_hip_set_stream", "cddp_hip_set_initial", "cddp_hip_initialize", "cddp_hip_backward",
    "cddp_hip_forward", "cddp_hip_solve", "cddp_hip_get_results", "cddp_hip_get_trajectory",
    "cddp_hip_get_gains", "cddp_hip_get_value", "cddp_hip_get_linearization", "cddp_hip_get_duals", "cddp_hip_get_costates", "cddp_hip_get_backward_scalars",
    "cddp_hip_get_history", "cddp_hip_get_terminal", "cddp_hip_write_gather_records_device", "cddp_hip_dual_dim", "cddp_hip_batch",
    "cddp_hip_set_timing_detail", "cddp_hip_history_capacity", "cddp_hip_set_barrier_state", "cddp_hip_num_groups", "cddp_hip_concurrency", "cddp_hip_comm_unique_id", "cddp_hip_comm_init", "cddp_hip_comm_destroy", "cddp_hip_comm_info", "cddp_hip_get_plan_head", "cddp_hip_allgather_results",
    "cddp_hip_backward_stacks", "cddp_hip_stacks_create_abi", "cddp_hip_stacks_destroy", "cddp_hip_set_stacks", "cddp_hip_set_defect_stack", "cddp_hip_set_control_box", "cddp_hip_set_hessian_stacks", "cddp_hip_set_constraint_stacks",
    "cddp_hip_stacks_backward", "cddp_hip_stacks_last_kernel_ms", "cddp_hip_stacks_last_sweep_form", "cddp_hip_stacks_factor_cache", "cddp_hip_stacks_get_gains", "cddp_hip_stacks_get_constraint_gains",
    "cddp_hip_stacks_get_scalars", "cddp_hip_set_terminal_equality", "cddp_hip_stacks_get_terminal", "cddp_hip_plugin_solve", "cddp_hip_plugin_solve_terminal", "cddp_hip_plugin_set_host_threads", "cddp_hip_plugin_last_stats", "cddp_hip_model_eval", "cddp_hip_set_options", "cddp_hip_set_initial_state", "cddp_hip_forget_solver_state", "cddp_hip_set_duals", "cddp_hip_set_terminal",
    "cddp_hip_costate_mode", "cddp_hip_costate_redos", "cddp_hip_ls_stage_counts", "cddp_hip_mpc_advance", "cddp_hip_mpc_run",
    "cddp_hip_plant_create", "cddp_hip_plant_destroy", "cddp_hip_plant_step", "cddp_hip_mpc_run_plant", "cddp_hip_track_plan",
    "cddp_hip_field_shape", "cddp_hip_get_field_device", "cddp_hip_get_results_device", "cddp_hip_set_initial_device", "cddp_hip_get_live_slots",
    "cddp_hip_plan_jvp", "cddp_hip_plan_vjp", "cddp_hip_plan_covariance", "cddp_hip_plan_tvlqr", "cddp_hip_plan_kalman",
    "cddp_hip_score_rollouts", "cddp_hip_seed_best",
    "cddp_hip_sample_controls", "cddp_hip_mppi_blend", "cddp_hip_mppi_refine",
    "cddp_hip_mc_sample_noise", "cddp_hip_plan_montecarlo", "cddp_hip_mc_sample_meas_noise", "cddp_hip_plan_montecarlo_of",
    "cddp_hip_set_reference", "cddp_hip_get_reference", "cddp_hip_mpc_set_reference_path", "cddp_hip_mpc_reference_cursor",
    "cddp_hip_ekf_create", "cddp_hip_ekf_destroy", "cddp_hip_ekf_reset", "cddp_hip_ekf_update", "cddp_hip_ekf_predict", "cddp_hip_ekf_get",
    "cddp_hip_ekf_run", "cddp_hip_mpc_run_ekf",
]


class HipError(RuntimeError):
    pass


class HipBatchSolver:
    """Batch of independent trajectories of one problem on one GPU (C-ABI handle)."""

    def __init__(self, problem, batch, device=0, trig=None):
        self.lib = load_hip(trig)
        self.p = problem; self.B = batch
        self.h = C.c_void_p()
        rc = self.lib.cddp_hip_create(C.byref(problem.c), batch, device, C.byref(self.h))
        self._check(rc)
        self.m = self.lib.cddp_hip_dual_dim(self.h)
        self._user_stream = False; self._device = int(device)
        self.plan_epoch = 0      # counts the calls that rewrite the A / B / K stacks (sweeps): what plan_jvp / plan_vjp read belongs to the last of them

    def _check(self, rc):
        if rc != 0:
            raise HipError("cddp_hip error %d: %s" % (rc, self.lib.cddp_hip_last_error().decode()))

    def close(self):
        if self.h:
            self.lib.cddp_hip_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_groups(self):
        return int(self.lib.cddp_hip_num_groups(self.h))

    def concurrency(self):
        """Groups cddp_hip_solve keeps in flight at once (2 = the static two-way CU partition of round 5)."""
        return int(self.lib.cddp_hip_concurrency(self.h))

    def costate_mode(self):
        """1: the last solve (before the first: the next) evaluates the IPDDP costate trial in the shadow of the next sweep launch; 0: on the chain."""
        return int(self.lib.cddp_hip_costate_mode(self.h))

    def costate_redos(self):
        """Shadow solves of this handle that were discarded (non-finite deferred costate) and run again on the chain."""
        return int(self.lib.cddp_hip_costate_redos(self.h))

    def ls_stage_counts(self):
        """(ran, returned, gave_up): second-stage (tile, step size) workgroups of the last solve's two-stage iterations that ran inside
        the first stage's rollout launch -- ran a trial, returned at once, gave the wait for the first stage's masks up.  All 0 when the
        solve used two launches per such iteration (CDDP_HIP_LS_INKERNEL=0, costate on the chain, other solvers)."""
        c = (C.c_longlong * 3)()
        self.lib.cddp_hip_ls_stage_counts.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        rc = self.lib.cddp_hip_ls_stage_counts(self.h, c)
        if rc != 0:
            raise HipError("cddp_hip_ls_stage_counts failed: %d" % rc)
        return int(c[0]), int(c[1]), int(c[2])

    def set_stream(self, stream_ptr):
        self._check(self.lib.cddp_hip_set_stream(self.h, C.c_void_p(stream_ptr)))
        self._user_stream = True

    def set_timing_detail(self, detail):
        """TIMING_ROLLOUT (default): solve() brackets the rollout launches only; TIMING_ALL: every class;
        TIMING_SWEEP: derivative fill + sweep only (each event costs ~5 us of queue time)."""
        self._check(self.lib.cddp_hip_set_timing_detail(self.h, int(detail)))

    def set_initial(self, x0, U0=None, X0=None):
        x0 = _arr(x0); assert x0.shape == (self.B, self.p.nx)
        U0 = _arr(U0) if U0 is not None else None; X0 = _arr(X0) if X0 is not None else None
        self._check(self.lib.cddp_hip_set_initial(self.h, _ptr(x0), _ptr(U0), _ptr(X0)))

    def initialize(self):
        self.plan_epoch += 1
        self._check(self.lib.cddp_hip_initialize(self.h))

    # ---- warm start / MPC restarts
    def set_options(self, options):
        self._check(self.lib.cddp_hip_set_options(self.h, C.byref(options)))

    def set_warm_start(self, flag=True):
        self.p.options.warm_start = 1 if flag else 0
        self.set_options(self.p.options)

    def set_initial_state(self, x0):
        x0 = _arr(x0).reshape(self.B, self.p.nx)
        self._check(self.lib.cddp_hip_set_initial_state(self.h, _ptr(x0)))

    def forget_solver_state(self):
        """As if the reference's solver object were new: the next warm-started initialize takes the "provided trajectory" branch."""
        self._check(self.lib.cddp_hip_forget_solver_state(self.h))

    def set_duals(self, S=None, Y=None):
        S = _arr(S) if S is not None else None; Y = _arr(Y) if Y is not None else None
        self._check(self.lib.cddp_hip_set_duals(self.h, _ptr(S), _ptr(Y)))

    def set_barrier_state(self, mu=None, reg=None):
        mu = _arr(mu).reshape(self.B) if mu is not None else None
        reg = _arr(reg).reshape(self.B) if reg is not None else None
        self._check(self.lib.cddp_hip_set_barrier_state(self.h, _ptr(mu), _ptr(reg)))

    def set_terminal_state(self, S_T=None, Y_T=None, Lambda_T=None):
        a = [(_arr(v) if v is not None else None) for v in (S_T, Y_T, Lambda_T)]
        self._check(self.lib.cddp_hip_set_terminal(self.h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2])))

    def backward(self):
        self.plan_epoch += 1
        ok = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.cddp_hip_backward(self.h, ok.ctypes.data_as(C.POINTER(C.c_int32))))
        return ok

    def forward(self, alphas):
        a = _arr(alphas); t = np.zeros((self.B, a.size), dtype=TRIAL_DTYPE)
        self._check(self.lib.cddp_hip_forward(self.h, _ptr(a), a.size, t.ctypes.data_as(C.c_void_p)))
        return t

    def solve(self):
        self.plan_epoch += 1
        st = Stats()
        self._check(self.lib.cddp_hip_solve(self.h, C.byref(st)))
        return st

    def results(self):
        r = np.zeros(self.B, dtype=RESULT_DTYPE)
        self._check(self.lib.cddp_hip_get_results(self.h, r.ctypes.data_as(C.c_void_p)))
        return r

    def trajectory(self):
        X = np.zeros((self.B, self.p.N + 1, self.p.nx)); U = np.zeros((self.B, self.p.N, self.p.nu))
        self._check(self.lib.cddp_hip_get_trajectory(self.h, _ptr(X), _ptr(U)))
        return X, U

    def plan_head(self):
        """(u_0, x_1) of every trajectory's current iterate: what an MPC loop reads back (cddp_hip_get_plan_head)."""
        u0 = np.zeros((self.B, self.p.nu)); x1 = np.zeros((self.B, self.p.nx))
        self._check(self.lib.cddp_hip_get_plan_head(self.h, _ptr(u0), _ptr(x1)))
        return u0, x1

    def mpc_advance(self, mode, x_next=None, shift_duals=False):
        """One MPC step on the device (cddp_hip_mpc_advance): the seed of the next solve from the current plan, without a host copy of it.
        mode: MPC_KEEP_PLAN (== set_initial_state(x_next)), MPC_SHIFT_EXISTING (== set_initial(x_next, U shifted, X shifted)) or
        MPC_SHIFT_PROVIDED (== forget_solver_state + the same).  x_next: None = x_1 of the plan; a numpy array (B, nx) = the measured state,
        uploaded (the step's only transfer); a torch tensor on the handle's device = read in place (float64, contiguous), ordered on the
        stream given to set_stream, or after a synchronisation of the tensor's current stream when there is none."""
        flags = MPC_SHIFT_DUALS if shift_duals else 0
        keep = None
        if x_next is None:
            ptr = None
        elif isinstance(x_next, np.ndarray) or not hasattr(x_next, "data_ptr"):
            keep = _arr(x_next).reshape(self.B, self.p.nx); ptr = keep.ctypes.data
        else:
            import torch
            if not x_next.is_cuda or x_next.dtype != torch.float64 or tuple(x_next.shape) != (self.B, self.p.nx):
                raise ValueError("x_next: a float64 device tensor of shape (%d, %d) is expected" % (self.B, self.p.nx))
            if x_next.device.index != self._device:   # its address would be read as one of the handle's device
                raise ValueError("x_next lives on device %s, the handle on device %d" % (x_next.device.index, self._device))
            keep = x_next.contiguous(); ptr = keep.data_ptr(); flags |= MPC_X_DEVICE
            if not self._user_stream:
                torch.cuda.current_stream(keep.device).synchronize()
        self._check(self.lib.cddp_hip_mpc_advance(self.h, int(mode), flags, ptr))

    def mpc_run(self, steps, mode, shift_duals=False):
        """`steps` closed-loop MPC steps with the model as the plant (cddp_hip_mpc_run): solve, record, advance -- one call, one copy per
        output.  Returns a dict: U_applied (B, steps, nu), X_visited (B, steps + 1, nx), iterations and status (B, steps, int32), stats
        (the per-solve Stats added up)."""
        steps = int(steps); self.plan_epoch += 1
        U = np.zeros((self.B, max(steps, 0), self.p.nu)); X = np.zeros((self.B, max(steps, 0) + 1, self.p.nx))
        it = np.zeros((self.B, max(steps, 0)), dtype=np.int32); st = np.zeros((self.B, max(steps, 0)), dtype=np.int32)
        stats = Stats()
        i32 = C.POINTER(C.c_int32)
        self._check(self.lib.cddp_hip_mpc_run(self.h, steps, int(mode), MPC_SHIFT_DUALS if shift_duals else 0, _ptr(U), _ptr(X),
                                              it.ctypes.data_as(i32), st.ctypes.data_as(i32), C.byref(stats)))
        return {"U_applied": U, "X_visited": X, "iterations": it, "status": st, "stats": stats}

    def mpc_run_plant(self, plant, steps, mode, shift_duals=False, W=None):
        """`steps` closed-loop MPC steps against a DevicePlant (cddp_hip_mpc_run_plant): solve, plant step on the device from row 0 of the
        plan and its u_0 (saturated, disturbed by W[:, k]), advance from the plant's state.  W: None or (B, steps, nx), uploaded once.
        Returns the dict of mpc_run; U_applied holds the saturated controls, X_visited the plant's states."""
        steps = int(steps); self.plan_epoch += 1
        U = np.zeros((self.B, max(steps, 0), self.p.nu)); X = np.zeros((self.B, max(steps, 0) + 1, self.p.nx))
        it = np.zeros((self.B, max(steps, 0)), dtype=np.int32); st = np.zeros((self.B, max(steps, 0)), dtype=np.int32)
        Wa = _arr(W).reshape(self.B, max(steps, 0), self.p.nx) if W is not None else None
        stats = Stats()
        i32 = C.POINTER(C.c_int32)
        self._check(self.lib.cddp_hip_mpc_run_plant(self.h, plant.h if plant is not None else None, steps, int(mode), MPC_SHIFT_DUALS if shift_duals else 0,
                                                    _ptr(Wa), _ptr(U), _ptr(X), it.ctypes.data_as(i32), st.ctypes.data_as(i32), C.byref(stats)))
        return {"U_applied": U, "X_visited": X, "iterations": it, "status": st, "stats": stats}

    def mpc_run_ekf(self, plant, ekf, steps, mode, x0_true, W=None, Yn=None, shift_duals=False, skip_nan=False):
        """`steps` closed-loop MPC steps against a DevicePlant with a controller that sees only y = C x + Yn (cddp_hip_mpc_run_ekf): per step
        the DeviceEkf's update, the advance from its estimate, the solve, the plant step on the TRUE state (which starts at x0_true (B, nx)),
        the prediction with the commanded u_0.  W: None or (B, steps, nx); Yn: None or (B, steps + 1, ny); both uploaded once.  The handle
        needs a current plan (set_initial and initialize or solve).  Returns the dict of mpc_run_plant plus Xh_visited (B, steps, nx), the
        estimate each solve started from, and nis (B, steps)."""
        steps = int(steps); self.plan_epoch += 1
        n = max(steps, 0); nx, nu = self.p.nx, self.p.nu
        U = np.zeros((self.B, n, nu)); X = np.zeros((self.B, n + 1, nx)); Xh = np.zeros((self.B, n, nx)); nis = np.zeros((self.B, n))
        it = np.zeros((self.B, n), dtype=np.int32); st = np.zeros((self.B, n), dtype=np.int32)
        x0a = _arr(x0_true).reshape(self.B, nx) if x0_true is not None else None
        Wa = _arr(W).reshape(self.B, n, nx) if W is not None else None
        Ya = _arr(Yn).reshape(self.B, n + 1, ekf.ny) if Yn is not None else None
        stats = Stats()
        i32 = C.POINTER(C.c_int32)
        flags = (MPC_SHIFT_DUALS if shift_duals else 0) | (MPC_EKF_SKIP_NAN if skip_nan else 0)
        self._check(self.lib.cddp_hip_mpc_run_ekf(self.h, plant.h if plant is not None else None, ekf.h if ekf is not None else None, steps, int(mode),
                                                  flags, _ptr(x0a), _ptr(Wa), _ptr(Ya), _ptr(U), _ptr(X), _ptr(Xh), _ptr(nis),
                                                  it.ctypes.data_as(i32), st.ctypes.data_as(i32), C.byref(stats)))
        return {"U_applied": U, "X_visited": X, "Xh_visited": Xh, "nis": nis, "iterations": it, "status": st, "stats": stats}

    def track_plan(self, plant, x0=None, W=None):
        """The solved plan's feedback policy u_t = U_t + K_t (x_t - X_t) rolled out on a DevicePlant over the horizon (cddp_hip_track_plan).
        x0: None = row 0 of the plan, or (B, nx); W: None or (B, N, nx).  Returns (X (B, N + 1, nx), U (B, N, nu), the saturated controls);
        the handle's state is not modified."""
        x0a = _arr(x0).reshape(self.B, self.p.nx) if x0 is not None else None
        Wa = _arr(W).reshape(self.B, self.p.N, self.p.nx) if W is not None else None
        X = np.zeros((self.B, self.p.N + 1, self.p.nx)); U = np.zeros((self.B, self.p.N, self.p.nu))
        self._check(self.lib.cddp_hip_track_plan(self.h, plant.h if plant is not None else None, _ptr(x0a), _ptr(Wa), _ptr(X), _ptr(U)))
        return X, U

    # ---- moving the goal and the per-step reference of the live handle
    def _ref_arg(self, name, a, shape, device):
        """A reference array as a plain address: a numpy array (host) or a float64 tensor on the handle's device."""
        if a is None:
            return None, None
        if device:
            t = self._device_tensor(name, a, shape)
            return t, t.data_ptr()
        k = _arr(a).reshape(shape)
        return k, k.ctypes.data

    def set_reference(self, x_ref=None, x_ref_traj=None, clear_traj=False):
        """Replace the goal x_ref (nx,) and / or the per-step reference x_ref_traj (N + 1, nx) of the live handle (cddp_hip_set_reference);
        None keeps what the handle has, clear_traj drops the per-step reference.  numpy arrays are uploaded (finite values and the rule
        |x_ref_traj[N] - x_ref| <= 1e-6 are checked); float64 tensors on the handle's device are read in place, ordered on the stream given to
        set_stream or after a synchronisation of torch's current stream -- all arrays of one call are of one kind.  Takes effect from the next
        initialize / solve; score_rollouts, mppi_refine, plan_montecarlo and forward use it at once.  Refused while a reference path is bound."""
        nx, N = self.p.nx, self.p.N
        given = [a for a in (x_ref, x_ref_traj) if a is not None]
        device = any(hasattr(a, "data_ptr") for a in given)
        if device and not all(hasattr(a, "data_ptr") for a in given):
            raise ValueError("set_reference: x_ref and x_ref_traj must both be numpy arrays or both be device tensors")
        k0, p0 = self._ref_arg("x_ref", x_ref, (nx,), device)
        k1, p1 = self._ref_arg("x_ref_traj", x_ref_traj, (N + 1, nx), device)
        if device:
            self._order_device_io()
        flags = (REF_DEVICE if device else 0) | (REF_CLEAR_TRAJ if clear_traj else 0)
        self._check(self.lib.cddp_hip_set_reference(self.h, flags, p0, p1))

    def get_reference(self):
        """(x_ref (nx,), x_ref_traj (N + 1, nx) or None): the goal and the per-step reference as the device holds them, what the kernels
        of the next launch read (cddp_hip_get_reference)."""
        x = np.zeros(self.p.nx); T = np.zeros((self.p.N + 1, self.p.nx)); has = C.c_int32(0)
        self._check(self.lib.cddp_hip_get_reference(self.h, _ptr(x), _ptr(T), C.byref(has)))
        return x, (T if has.value else None)

    def mpc_set_reference_path(self, path, start=0, rows_per_step=1.0):
        """Bind a path (L, nx) to the handle (cddp_hip_mpc_set_reference_path): the window of cursor `start` becomes the per-step reference
        and its last row the goal at once, and every mpc_advance -- mpc_run and mpc_run_plant included -- moves the cursor by one and installs
        the next window on the device.  Window row t of cursor k is the path at (k + t) * rows_per_step, linearly interpolated between rows,
        the last row past the end.  path: a numpy array (copied) or a float64 device tensor (copied on the device); None unbinds and leaves
        the reference as it stands."""
        if path is None:
            self._check(self.lib.cddp_hip_mpc_set_reference_path(self.h, None))
            return
        d = RefPathDesc()
        d.abi_version = ABI_VERSION; d.start = int(start); d.rows_per_step = float(rows_per_step)
        if hasattr(path, "data_ptr"):
            if path.dim() != 2:
                raise ValueError("path: shape (L, %d) is expected, got %s" % (self.p.nx, tuple(path.shape)))
            keep = self._device_tensor("path", path, (path.shape[0], self.p.nx))
            d.flags = REF_DEVICE; d.rows = int(keep.shape[0]); d.path = keep.data_ptr()
            self._order_device_io()
        else:
            keep = _arr(path)
            if keep.ndim != 2 or keep.shape[1] != self.p.nx:
                raise ValueError("path: shape (L, %d) is expected, got %s" % (self.p.nx, keep.shape))
            d.flags = 0; d.rows = int(keep.shape[0]); d.path = keep.ctypes.data if keep.size else None
        self._check(self.lib.cddp_hip_mpc_set_reference_path(self.h, C.byref(d)))

    def mpc_reference_cursor(self):
        """The cursor of the window now installed (start + the advances since the path was bound); -1 without a path."""
        c = C.c_int64(0)
        self._check(self.lib.cddp_hip_mpc_reference_cursor(self.h, C.byref(c)))
        return int(c.value)

    def gains(self):
        K = np.zeros((self.B, self.p.N, self.p.nu, self.p.nx)); k = np.zeros((self.B, self.p.N, self.p.nu))
        self._check(self.lib.cddp_hip_get_gains(self.h, _ptr(K), _ptr(k)))
        return K, k

    def value(self):
        Vx = np.zeros((self.B, self.p.N + 1, self.p.nx)); Vxx = np.zeros((self.B, self.p.N + 1, self.p.nx, self.p.nx))
        self._check(self.lib.cddp_hip_get_value(self.h, _ptr(Vx), _ptr(Vxx)))
        return Vx, Vxx

    def linearization(self):
        """A_t = I + dt f_x, B_t = dt f_u of the last backward pass (F_x_, F_u_ of cddp_solver_base.cpp:319-394)."""
        A = np.zeros((self.B, self.p.N, self.p.nx, self.p.nx)); Bm = np.zeros((self.B, self.p.N, self.p.nx, self.p.nu))
        self._check(self.lib.cddp_hip_get_linearization(self.h, _ptr(A), _ptr(Bm)))
        return A, Bm

    def duals(self):
        S = np.zeros((self.B, self.p.N, self.m)); Y = np.zeros_like(S); G = np.zeros_like(S)
        if self.m:
            self._check(self.lib.cddp_hip_get_duals(self.h, _ptr(S), _ptr(Y), _ptr(G)))
        return S, Y, G

    def costates(self):
        """Costate trajectory Lambda of the current iterate, (B, rows, nx): rows = N + 1 (IPDDP) or N (MSIPDDP) (cddp_hip_get_costates)."""
        rows = C.c_int32(0)
        self._check(self.lib.cddp_hip_get_costates(self.h, None, C.byref(rows)))
        L = np.zeros((self.B, rows.value, self.p.nx))
        self._check(self.lib.cddp_hip_get_costates(self.h, _ptr(L), C.byref(rows)))
        return L

    def terminal(self):
        dims = np.zeros(2, dtype=np.int32)
        self._check(self.lib.cddp_hip_get_terminal(self.h, None, None, None, None, dims.ctypes.data_as(C.POINTER(C.c_int32))))
        mT, pT = int(dims[0]), int(dims[1])
        S = np.zeros((self.B, mT)); Y = np.zeros((self.B, mT)); G = np.zeros((self.B, mT)); L = np.zeros((self.B, pT))
        self._check(self.lib.cddp_hip_get_terminal(self.h, _ptr(S), _ptr(Y), _ptr(G), _ptr(L), None))
        return S, Y, G, L

    def backward_scalars(self):
        dV = np.zeros((self.B, 2)); reg = np.zeros(self.B)
        self._check(self.lib.cddp_hip_get_backward_scalars(self.h, _ptr(dV), _ptr(reg)))
        return dV, reg

    def history(self, hist_batch=1):
        cap = self.lib.cddp_hip_history_capacity(self.h)   # fixed at create time (set_options may lower max_iterations)
        h = np.zeros((hist_batch, cap, 9)); cnt = np.zeros(hist_batch, dtype=np.int32)
        self._check(self.lib.cddp_hip_get_history(self.h, hist_batch, _ptr(h), cnt.ctypes.data_as(C.POINTER(C.c_int32))))
        return [h[b, :cnt[b]].copy() for b in range(hist_batch)]

    def allgather_results(self, comm, world, shard_capacity, recv_device_ptr):
        """The path's single collective through the C-ABI (RCCL all-gather of the 16-byte records); comm = a
        communicator from `comm_init` (or None for world == 1)."""
        self._check(self.lib.cddp_hip_allgather_results(self.h, C.c_void_p(comm), int(world), int(shard_capacity), C.c_void_p(recv_device_ptr)))

    def write_gather_records_device(self, device_ptr):
        self._check(self.lib.cddp_hip_write_gather_records_device(self.h, C.c_void_p(device_ptr)))

    # ---- device-resident inputs and outputs: torch.float64 tensors on the handle's device, batch-major as the numpy entries
    def _torch_device(self):
        import torch
        return torch.device("cuda", self._device)

    def _device_tensor(self, name, t, shape):
        """The checks of a tensor handed to the C entry: refused here with ValueError, before the call."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: a torch tensor is expected, got %s" % (name, type(t).__name__))
        if not t.is_cuda:
            raise ValueError("%s lives on %s, the handle on device %d" % (name, t.device, self._device))
        if t.device.index != self._device:
            raise ValueError("%s lives on device %s, the handle on device %d" % (name, t.device.index, self._device))
        if t.dtype != torch.float64:
            raise ValueError("%s: dtype torch.float64 is expected, got %s" % (name, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s: shape %s is expected, got %s" % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous (batch-major)" % name)
        return t

    def _order_device_io(self):
        """Without a stream from set_stream the handle's streams know nothing of torch's: what torch has queued for the tensors is finished first."""
        if not self._user_stream:
            import torch
            torch.cuda.current_stream(self._torch_device()).synchronize()

    def set_initial_device(self, x0, U0=None, X0=None):
        """set_initial from tensors on the handle's device (cddp_hip_set_initial_device): x0 (B, nx), U0 (B, N, nu) or None (zeros), X0
        (B, N + 1, nx) or None (x0 along the horizon); row 0 of the seed is x0.  float64, contiguous.  Nothing crosses the bus; the handle is
        left as set_initial leaves it.  Ordered on the stream given to set_stream, or after a synchronisation of torch's current stream."""
        x0 = self._device_tensor("x0", x0, (self.B, self.p.nx))
        if U0 is not None:
            U0 = self._device_tensor("U0", U0, (self.B, self.p.N, self.p.nu))
        if X0 is not None:
            X0 = self._device_tensor("X0", X0, (self.B, self.p.N + 1, self.p.nx))
        self._order_device_io()
        self._check(self.lib.cddp_hip_set_initial_device(self.h, x0.data_ptr(), U0.data_ptr() if U0 is not None else None,
                                                         X0.data_ptr() if X0 is not None else None))

    def live_slots(self):
        """The plane of the slotted fields that holds every trajectory's current iterate, (B,) int32 (cddp_hip_get_live_slots)."""
        s = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.cddp_hip_get_live_slots(self.h, s.ctypes.data_as(C.POINTER(C.c_int32)), None))
        return s

    def field_shape(self, name):
        """(T, E) of the (B, T, E) array of a field of FIELD_NAMES (cddp_hip_field_shape)."""
        if name not in FIELD_IDS:
            raise ValueError("unknown field %r (one of %s)" % (name, ", ".join(FIELD_NAMES)))
        rows = C.c_int32(0); cols = C.c_int32(0)
        self._check(self.lib.cddp_hip_field_shape(self.h, FIELD_IDS[name], C.byref(rows), C.byref(cols)))
        return int(rows.value), int(cols.value)

    def field_device(self, name, out=None):
        """One field of FIELD_NAMES as a (B, T, E) float64 tensor on the handle's device, bit for bit what its numpy getter returns
        (cddp_hip_get_field_device).  out: a tensor to fill instead of a new one.  With a stream from set_stream the tensor is complete for
        work queued on that stream; otherwise on return."""
        import torch
        T, E = self.field_shape(name)
        if out is None:
            out = torch.empty((self.B, T, E), dtype=torch.float64, device=self._torch_device())
        else:
            out = self._device_tensor("out", out, (self.B, T, E))
        self._order_device_io()
        self._check(self.lib.cddp_hip_get_field_device(self.h, FIELD_IDS[name], out.data_ptr()))
        return out

    def trajectory_device(self):
        return self.field_device("X"), self.field_device("U")

    def gains_device(self):
        nx, nu = self.p.nx, self.p.nu
        return self.field_device("K").view(self.B, self.p.N, nu, nx), self.field_device("KFF")

    def value_device(self):
        nx = self.p.nx
        return self.field_device("VX"), self.field_device("VXX").view(self.B, self.p.N + 1, nx, nx)

    def linearization_device(self):
        nx, nu = self.p.nx, self.p.nu
        return self.field_device("A").view(self.B, self.p.N, nx, nx), self.field_device("B").view(self.B, self.p.N, nx, nu)

    def duals_device(self):
        """(S, Y, G), each (B, N, m); refused as duals' C entry refuses a problem without slack / dual rows."""
        return self.field_device("S"), self.field_device("Y"), self.field_device("G")

    def costates_device(self):
        return self.field_device("LAMBDA")

    def results_device(self):
        """results() on the device (cddp_hip_get_results_device): a dict of per-trajectory column views, named as RESULT_DTYPE, over one
        (B, 10) float64 and one (B, 4) int32 tensor (also returned, as "cols" and "icols")."""
        import torch
        dev = self._torch_device()
        cols = torch.empty((self.B, 10), dtype=torch.float64, device=dev); icols = torch.empty((self.B, 4), dtype=torch.int32, device=dev)
        self._order_device_io()
        self._check(self.lib.cddp_hip_get_results_device(self.h, cols.data_ptr(), icols.data_ptr()))
        out = {name: cols[:, i] for i, name in enumerate(RESULT_DEVICE_COLS)}
        out.update({name: icols[:, i] for i, name in enumerate(RESULT_DEVICE_ICOLS)})
        out["cols"] = cols; out["icols"] = icols
        return out


    # ---- linear response of the plan to its initial state (cddp_hip_plan_jvp / cddp_hip_plan_vjp): numpy arrays take the host path,
    # torch.float64 tensors on the handle's device the device path; the result is of the kind of the input
    def _sens_arg(self, name, a, tail, nvec=None, squeeze=None):
        """One array argument, (B,) + tail or (B, R) + tail -> (the contiguous (B, R) + tail array, R, whether the vector axis was absent)."""
        is_t = hasattr(a, "data_ptr")
        shape = tuple(a.shape)
        if shape == (self.B,) + tuple(tail):
            R, sq = 1, True
        elif len(shape) == len(tail) + 2 and shape[0] == self.B and shape[2:] == tuple(tail) and shape[1] >= 1:
            R, sq = int(shape[1]), False
        else:
            raise ValueError("%s: shape %s or %s is expected, got %s" % (name, (self.B,) + tuple(tail), (self.B, "R") + tuple(tail), shape))
        if nvec is not None and (R != nvec or sq != squeeze):
            raise ValueError("%s: %d vector(s) per trajectory, the other argument has %d (or only one of them has the vector axis)" % (name, R, nvec))
        full = (self.B, R) + tuple(tail)
        if is_t:
            a = self._device_tensor(name, a.reshape(full) if a.is_contiguous() else a, full)
        else:
            a = _arr(a).reshape(full)
        return a, R, sq

    def plan_jvp(self, dx0, want=("dX", "dU")):
        """The first-order response of the closed-loop plan to a change dx0 of its initial state (cddp_hip_plan_jvp): dx_{t+1} = A_t dx_t +
        B_t du_t, du_t = K_t dx_t over the stacks of the last backward sweep.  dx0: (B, nx) or (B, R, nx), a numpy array or a torch.float64
        tensor on the handle's device.  Returns (dX, dU) of shape (B, [R,] N + 1, nx) and (B, [R,] N, nu), of dx0's kind; an output that
        `want` does not name is None.  The handle's state is not modified."""
        want = tuple(want)
        if not want or any(w not in ("dX", "dU") for w in want):
            raise ValueError("want: a non-empty subset of ('dX', 'dU') is expected, got %r" % (want,))
        N, nx, nu = self.p.N, self.p.nx, self.p.nu
        d, R, sq = self._sens_arg("dx0", dx0, (nx,))
        sx = (self.B, N + 1, nx) if sq else (self.B, R, N + 1, nx)
        su = (self.B, N, nu) if sq else (self.B, R, N, nu)
        if hasattr(d, "data_ptr"):
            import torch
            dev = self._torch_device()
            dX = torch.empty(sx, dtype=torch.float64, device=dev) if "dX" in want else None
            dU = torch.empty(su, dtype=torch.float64, device=dev) if "dU" in want else None
            self._order_device_io()
            self._check(self.lib.cddp_hip_plan_jvp(self.h, SENS_DEVICE, R, d.data_ptr(), dX.data_ptr() if dX is not None else None,
                                                   dU.data_ptr() if dU is not None else None))
        else:
            dX = np.zeros(sx) if "dX" in want else None
            dU = np.zeros(su) if "dU" in want else None
            self._check(self.lib.cddp_hip_plan_jvp(self.h, 0, R, d.ctypes.data, dX.ctypes.data if dX is not None else None,
                                                   dU.ctypes.data if dU is not None else None))
        return dX, dU

    def plan_vjp(self, gX=None, gU=None):
        """The gradient with respect to x_0 of a loss on the plan, from its gradients gX (B, [R,] N + 1, nx) and gU (B, [R,] N, nu) with
        respect to (X, U); None = zeros (cddp_hip_plan_vjp: the adjoint of plan_jvp's recursion).  numpy arrays or torch.float64 tensors on
        the handle's device, both of one kind.  Returns (B, [R,] nx) of that kind."""
        N, nx, nu = self.p.N, self.p.nx, self.p.nu
        if gX is None and gU is None:
            raise ValueError("plan_vjp: gX and gU are both None (the gradient would be zero)")
        gx = gu = None; R = sq = None
        if gX is not None:
            gx, R, sq = self._sens_arg("gX", gX, (N + 1, nx))
        if gU is not None:
            gu, R, sq = self._sens_arg("gU", gU, (N, nu), R, sq)
        kinds = {hasattr(a, "data_ptr") for a in (gx, gu) if a is not None}
        if len(kinds) != 1:
            raise ValueError("plan_vjp: gX and gU must both be numpy arrays or both be device tensors")
        s0 = (self.B, nx) if sq else (self.B, R, nx)
        if kinds.pop():
            import torch
            g0 = torch.empty(s0, dtype=torch.float64, device=self._torch_device())
            self._order_device_io()
            self._check(self.lib.cddp_hip_plan_vjp(self.h, SENS_DEVICE, R, gx.data_ptr() if gx is not None else None,
                                                   gu.data_ptr() if gu is not None else None, g0.data_ptr()))
        else:
            g0 = np.zeros(s0)
            self._check(self.lib.cddp_hip_plan_vjp(self.h, 0, R, gx.ctypes.data if gx is not None else None,
                                                   gu.ctypes.data if gu is not None else None, g0.ctypes.data))
        return g0

    def plan_jacobian_device(self):
        """(dX/dx0 (B, N + 1, nx, nx), dU/dx0 (B, N, nu, nx)) as device tensors, from ONE plan_jvp with the nx unit vectors: entry
        [b, t, i, j] is the response of X[b, t, i] (U[b, t, i]) to x0[b, j]."""
        import torch
        nx = self.p.nx
        eye = torch.eye(nx, dtype=torch.float64, device=self._torch_device()).expand(self.B, nx, nx).contiguous()
        dX, dU = self.plan_jvp(eye)
        return dX.permute(0, 2, 3, 1).contiguous(), dU.permute(0, 2, 3, 1).contiguous()

    # ---- state and control covariance along the plan (cddp_hip_plan_covariance): numpy arrays take the host path, torch.float64 tensors on
    # the handle's device the device path; every argument of a call is of one kind, and so is the result
    def plan_covariance(self, Sigma0, W=None, Wu=None, diag=False, want=("SX", "SU", "dcost")):
        """Covariance of the plan's states and controls under its own feedback gains (cddp_hip_plan_covariance): Sigma_{t+1} = Acl_t Sigma_t
        Acl_t^T + W + B_t Wu B_t^T with Acl_t = A_t + B_t K_t over the stacks of the last backward sweep, cov(du_t) = K_t Sigma_t K_t^T + Wu,
        and the expected increase of the quadratic objective.  Sigma0: (nx, nx) for the whole batch or (B, nx, nx) per trajectory; W
        (process noise) and Wu (actuator noise, nu x nu) are None or of Sigma0's kind and batching.  Only the lower triangles are read.
        numpy arrays or torch.float64 tensors on the handle's device.  Returns a dict of Sigma0's kind with the entries `want` names: "SX"
        (B, N + 1, nx, nx), "SU" (B, N, nu, nu) -- diag=True: their diagonals, (B, N + 1, nx) and (B, N, nu) -- and "dcost" (B,).  The
        handle's state is not modified."""
        want = tuple(want)
        if not want or any(w not in ("SX", "SU", "dcost") for w in want):
            raise ValueError("want: a non-empty subset of ('SX', 'SU', 'dcost') is expected, got %r" % (want,))
        if Sigma0 is None:
            raise ValueError("plan_covariance: Sigma0 is None")
        N, nx, nu, B = self.p.N, self.p.nx, self.p.nu, self.B
        device = hasattr(Sigma0, "data_ptr") and not isinstance(Sigma0, np.ndarray)
        if not device:
            if isinstance(Sigma0, np.ndarray) and Sigma0.dtype != np.float64:
                raise ValueError("plan_covariance: Sigma0: dtype float64 is expected, got %s" % Sigma0.dtype)
            Sigma0 = np.ascontiguousarray(Sigma0, dtype=np.float64)      # (a list, as the other arguments may be)
        ndim = len(tuple(Sigma0.shape))
        if ndim not in (2, 3):
            raise ValueError("plan_covariance: Sigma0: shape %s or %s is expected, got %s" % ((nx, nx), (B, nx, nx), tuple(Sigma0.shape)))
        per = ndim == 3
        lead = (B,) if per else ()
        args = []
        for name, a, n in (("Sigma0", Sigma0, nx), ("W", W, nx), ("Wu", Wu, nu)):
            args.append(None if a is None else self._score_arg("plan_covariance", name, a, (lead + (n, n),), device))
        s0, w, wu = args
        flags = (COV_DEVICE if device else 0) | (COV_DIAG if diag else 0) | (COV_PER_TRAJ if per else 0)
        shapes = {"SX": (B, N + 1, nx) if diag else (B, N + 1, nx, nx), "SU": (B, N, nu) if diag else (B, N, nu, nu), "dcost": (B,)}
        if device:
            import torch
            dev = self._torch_device()
            out = {k: torch.empty(shapes[k], dtype=torch.float64, device=dev) for k in want}
            self._order_device_io()
            ptr = lambda a: a.data_ptr() if a is not None else None
        else:
            out = {k: np.zeros(shapes[k]) for k in want}
            ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self.lib.cddp_hip_plan_covariance(self.h, flags, ptr(s0), ptr(w), ptr(wu), ptr(out.get("SX")), ptr(out.get("SU")), ptr(out.get("dcost"))))
        return out

    # ---- time-varying LQR gains along the plan (cddp_hip_plan_tvlqr): numpy arrays take the host path, torch.float64 tensors on the
    # handle's device the device path; every argument of a call is of one kind, and so is the result (no weight given: numpy)
    def plan_tvlqr(self, Q=None, R=None, Qf=None, install=False, want=("K", "P"), device=None):
        """The finite-horizon LQR of the plan's linearisation for the caller's tracking weights (cddp_hip_plan_tvlqr): the backward
        Riccati recursion over the A / B stacks of the last backward sweep.  Q (nx, nx) and R (nu, nu) are unscaled (the library multiplies
        by dt), Qf (nx, nx) is used as given; None = the handle's own.  A weight with a leading B axis is per trajectory, and then every
        weight that is given must be.  Only the lower triangles are read.  numpy arrays or torch.float64 tensors on the handle's device.
        Returns a dict of the arguments' kind with the entries `want` names -- "K" (B, N, nu, nx), "P" (B, N + 1, nx, nx) -- and "info"
        (B,) int32: 0, or t + 1 of the step whose factorisation failed (K = 0 and P = NaN from there down).  install=True also writes K
        into the handle's gain stack: until the next backward sweep gains(), field_device("K"), track_plan, plan_jvp / plan_vjp,
        plan_covariance, plan_montecarlo and the feedback scoring read the designed gains; want may then be empty.  device: with no
        weight given, whether the results are device tensors (default: numpy arrays)."""
        want = tuple(want)
        if any(w not in ("K", "P") for w in want) or (not want and not install):
            raise ValueError("want: a subset of ('K', 'P') is expected, non-empty unless install=True, got %r" % (want,))
        N, nx, nu, B = self.p.N, self.p.nx, self.p.nu, self.B
        given = [(name, a, n) for name, a, n in (("Q", Q, nx), ("R", R, nu), ("Qf", Qf, nx)) if a is not None]
        kinds = {hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) for _, a, _ in given}
        if len(kinds) > 1:
            raise ValueError("plan_tvlqr: Q, R and Qf must all be numpy arrays or all be device tensors")
        if kinds:
            kind = kinds.pop()
            if device is not None and bool(device) != kind:
                raise ValueError("plan_tvlqr: device=%r, but the weights are %s" % (device, "device tensors" if kind else "numpy arrays"))
            device = kind
        device = bool(device)
        conv = {}
        for name, a, n in given:
            if not device:
                if isinstance(a, np.ndarray) and a.dtype != np.float64:
                    raise ValueError("plan_tvlqr: %s: dtype float64 is expected, got %s" % (name, a.dtype))
                a = np.ascontiguousarray(a, dtype=np.float64)
            conv[name] = a
        ndims = {len(tuple(a.shape)) for a in conv.values()}
        if ndims - {2, 3} or len(ndims) > 1:
            raise ValueError("plan_tvlqr: the weights that are given must all have shape (n, n) or all have shape %s, got %s"
                             % ((B, "n", "n"), ", ".join("%s %s" % (k, tuple(a.shape)) for k, a in conv.items())))
        per = ndims == {3}
        lead = (B,) if per else ()
        args = {name: None for name in ("Q", "R", "Qf")}
        for name, a, n in given:
            args[name] = self._score_arg("plan_tvlqr", name, conv[name], (lead + (n, n),), device)
        flags = (LQR_DEVICE if device else 0) | (LQR_PER_TRAJ if per else 0) | (LQR_INSTALL if install else 0)
        shapes = {"K": (B, N, nu, nx), "P": (B, N + 1, nx, nx)}
        if device:
            import torch
            dev = self._torch_device()
            out = {k: torch.empty(shapes[k], dtype=torch.float64, device=dev) for k in want}
            out["info"] = torch.empty((B,), dtype=torch.int32, device=dev)
            self._order_device_io()
            ptr = lambda a: a.data_ptr() if a is not None else None
        else:
            out = {k: np.zeros(shapes[k]) for k in want}
            out["info"] = np.zeros((B,), dtype=np.int32)
            ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self.lib.cddp_hip_plan_tvlqr(self.h, flags, ptr(args["Q"]), ptr(args["R"]), ptr(args["Qf"]), ptr(out.get("K")), ptr(out.get("P")),
                                                 ptr(out["info"])))
        return out

    # ---- Kalman filter gains and output-feedback covariance along the plan (cddp_hip_plan_kalman): numpy arrays take the host path,
    # torch.float64 tensors on the handle's device the device path; every argument of a call is of one kind, and so is the result
    def plan_kalman(self, C, v, Sigma0, W=None, Wu=None, diag=False, want=("L", "SX", "SU", "dcost"), device=None):
        """The Kalman filter of the plan's linearisation for the sensors y_t = C dx_t + n_t, cov(n_t) = diag(v), and the covariance of
        states and controls when the handle's gains act on the filtered estimate (cddp_hip_plan_kalman), over the stacks of the last
        backward sweep; after plan_tvlqr(install=True) the gains are the installed ones.  C: (ny, nx) with 1 <= ny <= KF_MAX_NY, v: (ny,)
        measurement variances, Sigma0 (nx, nx), W (nx, nx) and Wu (nu, nu) or None; with a leading B axis on C every input is per
        trajectory.  Only the lower triangles of Sigma0, W and Wu are read.  numpy arrays or torch.float64 tensors on the handle's device,
        never mixed.  Returns a dict of the arguments' kind with the entries `want` names: "L" (B, N + 1, nx, ny) the filter gains, "SP"
        and "SF" (B, N + 1, nx, nx) the error covariance before and after the measurement, "SX" (B, N + 1, nx, nx) and "SU" (B, N, nu, nu)
        the covariance of states and controls under output feedback -- diag=True: the diagonals of SP, SF, SX and SU -- "dcost" (B,) and
        "info" (B,) int32: 0, or t + 1 of the step at which a measurement row failed (NaN from that row on).  device: must agree with
        the arguments' kind if given.  The handle's state is not modified."""
        names = ("L", "SP", "SF", "SX", "SU", "dcost", "info")
        want = tuple(want)
        if not want or any(w not in names for w in want):
            raise ValueError("want: a non-empty subset of %r is expected, got %r" % (names, want))
        if C is None or v is None or Sigma0 is None:
            raise ValueError("plan_kalman: C, v and Sigma0 must be given")
        N, nx, nu, B = self.p.N, self.p.nx, self.p.nu, self.B
        given = [(name, a) for name, a in (("C", C), ("v", v), ("Sigma0", Sigma0), ("W", W), ("Wu", Wu)) if a is not None]
        kinds = {hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) for _, a in given}
        if len(kinds) > 1:
            raise ValueError("plan_kalman: C, v, Sigma0, W and Wu must all be numpy arrays or all be device tensors")
        kind = kinds.pop()
        if device is not None and bool(device) != kind:
            raise ValueError("plan_kalman: device=%r, but the arguments are %s" % (device, "device tensors" if kind else "numpy arrays"))
        device = kind
        conv = {}
        for name, a in given:
            if not device:
                if isinstance(a, np.ndarray) and a.dtype != np.float64:
                    raise ValueError("plan_kalman: %s: dtype float64 is expected, got %s" % (name, a.dtype))
                a = np.ascontiguousarray(a, dtype=np.float64)
            conv[name] = a
        cs = tuple(conv["C"].shape)
        if len(cs) not in (2, 3) or cs[-1] != nx or (len(cs) == 3 and cs[0] != B):
            raise ValueError("plan_kalman: C: shape %s or %s is expected, got %s" % (("ny", nx), (B, "ny", nx), cs))
        ny = int(cs[-2])
        if not 1 <= ny <= KF_MAX_NY:
            raise ValueError("plan_kalman: C has %d rows, 1 .. %d measurement rows are expected" % (ny, KF_MAX_NY))
        per = len(cs) == 3
        lead = (B,) if per else ()
        tails = {"C": (ny, nx), "v": (ny,), "Sigma0": (nx, nx), "W": (nx, nx), "Wu": (nu, nu)}
        args = {name: None for name in tails}
        for name, _ in given:
            args[name] = self._score_arg("plan_kalman", name, conv[name], (lead + tails[name],), device)
        flags = (KF_DEVICE if device else 0) | (KF_DIAG if diag else 0) | (KF_PER_TRAJ if per else 0)
        sx = (B, N + 1, nx) if diag else (B, N + 1, nx, nx)
        shapes = {"L": (B, N + 1, nx, ny), "SP": sx, "SF": sx, "SX": sx, "SU": (B, N, nu) if diag else (B, N, nu, nu), "dcost": (B,), "info": (B,)}
        if device:
            import torch
            dev = self._torch_device()
            out = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "info" else torch.float64, device=dev) for k in want}
            self._order_device_io()
            ptr = lambda a: a.data_ptr() if a is not None else None
        else:
            out = {k: np.zeros(shapes[k], dtype=np.int32 if k == "info" else np.float64) for k in want}
            ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self.lib.cddp_hip_plan_kalman(self.h, flags, ny, ptr(args["C"]), ptr(args["v"]), ptr(args["Sigma0"]), ptr(args["W"]), ptr(args["Wu"]),
                                                  *[ptr(out.get(k)) for k in names]))
        return out

    # ---- scoring candidate control sequences and seeding from the best (cddp_hip_score_rollouts / cddp_hip_seed_best): numpy arrays take
    # the host path, torch.float64 tensors on the handle's device the device path; every argument of a call is of one kind
    def _score_arg(self, who, name, a, shapes, device):
        """One array argument whose shape must be one of `shapes`: a contiguous float64 numpy array, or the checked device tensor."""
        if hasattr(a, "data_ptr") and not isinstance(a, np.ndarray):
            if not device:
                raise ValueError("%s: %s is a device tensor, the other arguments are numpy arrays" % (who, name))
            if tuple(a.shape) not in shapes:
                raise ValueError("%s: %s: shape %s is expected, got %s" % (who, name, " or ".join(str(x) for x in shapes), tuple(a.shape)))
            return self._device_tensor(name, a, tuple(a.shape))
        if device:
            raise ValueError("%s: %s is not a device tensor, the other arguments are" % (who, name))
        if isinstance(a, np.ndarray) and a.dtype != np.float64:
            raise ValueError("%s: %s: dtype float64 is expected, got %s" % (who, name, a.dtype))
        a = np.ascontiguousarray(a, dtype=np.float64)
        if tuple(a.shape) not in shapes:
            raise ValueError("%s: %s: shape %s is expected, got %s" % (who, name, " or ".join(str(x) for x in shapes), tuple(a.shape)))
        return a

    @staticmethod
    def _addr(a):
        return None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())

    def score_rollouts(self, U, x0=None, plant=None, feedback=False, want=("cost", "viol"), ncand=None):
        """What S candidate control sequences per trajectory are worth, in one launch (cddp_hip_score_rollouts): U (B, S, N, nu), or None
        with feedback=True (the plan's own U); x0 (B, nx), (B, S, nx) or None (row 0 of the live plan); plant: a DevicePlant or None (the
        handle's own model).  feedback=True applies u_t = U_t + K_t (x_t - X_t) around the live plan.  numpy arrays, or torch.float64
        tensors on the handle's device (device path, device tensors back).  want: any of "cost" (B, S), "viol" (B, S), "X" (B, S, N + 1,
        nx), "U" (B, S, N, nu: the controls as applied); returns a dict.  With U None the number of candidates is x0's S, or ncand, or 1.
        The handle's solver state is not modified."""
        who = "score_rollouts"
        want = tuple(want)
        if any(w not in ("cost", "viol", "X", "U") for w in want):
            raise ValueError("%s: want: a subset of ('cost', 'viol', 'X', 'U') is expected, got %r" % (who, want))
        B, N, nx, nu = self.B, self.p.N, self.p.nx, self.p.nu
        if U is None and not feedback:
            raise ValueError("%s: U is None without feedback=True: there is nothing to roll out" % who)
        given = [a for a in (U, x0) if a is not None]
        device = any(hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) for a in given)
        S = None
        if U is not None:
            if len(tuple(U.shape) if hasattr(U, "shape") else np.shape(U)) != 4:
                raise ValueError("%s: U: shape (%d, S, %d, %d) is expected, got %s" % (who, B, N, nu, tuple(np.shape(U))))
            S = int(np.shape(U)[1])
            if S < 1:
                raise ValueError("%s: U: at least one candidate is expected" % who)
            U = self._score_arg(who, "U", U, [(B, S, N, nu)], device)
        flags = SCORE_FEEDBACK if feedback else 0
        if x0 is not None:
            shp = tuple(np.shape(x0))
            if S is None:
                S = int(shp[1]) if len(shp) == 3 else (int(ncand) if ncand is not None else 1)
            x0 = self._score_arg(who, "x0", x0, [(B, nx), (B, S, nx)], device)
            if len(shp) == 3:
                flags |= SCORE_X0_PER_CANDIDATE
        if S is None:
            S = int(ncand) if ncand is not None else 1
        if ncand is not None and int(ncand) != S:
            raise ValueError("%s: ncand = %d, the arrays hold %d candidates" % (who, int(ncand), S))
        if S < 1:
            raise ValueError("%s: at least one candidate is expected" % who)
        shapes = {"cost": (B, S), "viol": (B, S), "X": (B, S, N + 1, nx), "U": (B, S, N, nu)}
        out = {}
        if device:
            import torch
            dev = self._torch_device()
            for w in ("cost",) + tuple(w for w in want if w != "cost"):
                out[w] = torch.empty(shapes[w], dtype=torch.float64, device=dev)
            self._order_device_io()
            flags |= SCORE_DEVICE
        else:
            for w in ("cost",) + tuple(w for w in want if w != "cost"):
                out[w] = np.zeros(shapes[w])
        self._check(self.lib.cddp_hip_score_rollouts(self.h, plant.h if plant is not None else None, flags, S, self._addr(x0), self._addr(U),
                                                     self._addr(out["cost"]), self._addr(out.get("viol")), self._addr(out.get("X")), self._addr(out.get("U"))))
        return {w: out[w] for w in want}

    def seed_best(self, U, cost, viol=None, x0=None, viol_tol=0.0):
        """Seed the handle from the best of S candidates per trajectory (cddp_hip_seed_best): the admissible (finite, viol <= viol_tol)
        candidate of lowest cost, else the finite one of lowest viol then cost, ties to the lowest index, else candidate 0 with winner -1.
        U (B, S, N, nu), cost (B, S), viol (B, S) or None (all 0), x0 (B, nx) or None (keep the handle's x0); numpy arrays or
        torch.float64 device tensors, all of one kind.  Returns winner (B,) int32 of that kind.  The handle is left exactly as
        set_initial_device(x0, U[arange(B), winner]) leaves it."""
        who = "seed_best"
        B, N, nx, nu = self.B, self.p.N, self.p.nx, self.p.nu
        if U is None or cost is None:
            raise ValueError("%s: U and cost are required" % who)
        device = hasattr(U, "data_ptr") and not isinstance(U, np.ndarray)
        if len(tuple(np.shape(U))) != 4 or int(np.shape(U)[1]) < 1:
            raise ValueError("%s: U: shape (%d, S, %d, %d) with S >= 1 is expected, got %s" % (who, B, N, nu, tuple(np.shape(U))))
        S = int(np.shape(U)[1])
        U = self._score_arg(who, "U", U, [(B, S, N, nu)], device)
        cost = self._score_arg(who, "cost", cost, [(B, S)], device)
        if viol is not None:
            viol = self._score_arg(who, "viol", viol, [(B, S)], device)
        if x0 is not None:
            x0 = self._score_arg(who, "x0", x0, [(B, nx)], device)
        viol_tol = float(viol_tol)
        if device:
            import torch
            winner = torch.empty((B,), dtype=torch.int32, device=self._torch_device())
            self._order_device_io()
        else:
            winner = np.zeros(B, dtype=np.int32)
        self._check(self.lib.cddp_hip_seed_best(self.h, SCORE_DEVICE if device else 0, S, self._addr(x0), self._addr(U), self._addr(cost),
                                                self._addr(viol), viol_tol, self._addr(winner)))
        return winner

    # ---- sampling-based plan refinement (cddp_hip_sample_controls / cddp_hip_mppi_blend / cddp_hip_mppi_refine): the conventions of
    # score_rollouts -- numpy arrays take the host path, torch.float64 tensors on the handle's device the device path, one kind per call
    def _mppi_desc(self, who, sigma, ncand, lam=1.0, seed=0, stream=0, iters=1, keep_mean=False, viol_tol=0.0, u_lower=None, u_upper=None):
        """-> (MppiDesc, the arrays it points into).  What can be refused without the library is refused here with ValueError."""
        nu = self.p.nu
        ncand = int(ncand); iters = int(iters); lam = float(lam); viol_tol = float(viol_tol); seed = int(seed); stream = int(stream)
        if ncand < 1:
            raise ValueError("%s: ncand: at least one candidate is expected, got %d" % (who, ncand))
        if iters < 1:
            raise ValueError("%s: iters: at least one round is expected, got %d" % (who, iters))
        if not (lam > 0.0 and np.isfinite(lam)):
            raise ValueError("%s: lam: a positive finite temperature is expected, got %r" % (who, lam))
        if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 32:
            raise ValueError("%s: seed is a 64-bit and stream a 32-bit unsigned number, got %r and %r" % (who, seed, stream))
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (nu,)) if np.ndim(sigma) == 0 else np.asarray(sigma, dtype=np.float64))
        if sg.shape != (nu,) or not (np.isfinite(sg).all() and (sg > 0.0).all()):
            raise ValueError("%s: sigma: %d positive finite entries (or one scalar) are expected, got %r" % (who, nu, sigma))
        if (u_lower is None) != (u_upper is None):
            raise ValueError("%s: u_lower and u_upper are both given or both None" % who)
        d = MppiDesc()
        d.seed = seed; d.stream = stream; d.iters = iters; d.ncand = ncand; d.keep_mean = 1 if keep_mean else 0; d.lam = lam; d.viol_tol = viol_tol
        keep = [sg]
        d.sigma = _ptr(sg)
        if u_lower is not None:
            lo = np.ascontiguousarray(np.asarray(u_lower, dtype=np.float64)); up = np.ascontiguousarray(np.asarray(u_upper, dtype=np.float64))
            if lo.shape != (nu,) or up.shape != (nu,) or not (lo <= up).all():
                raise ValueError("%s: u_lower, u_upper: %d entries each with u_lower <= u_upper are expected" % (who, nu))
            keep += [lo, up]
            d.u_lower = _ptr(lo); d.u_upper = _ptr(up)
        return d, keep

    def _is_device(self, *arrays):
        return any(hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) for a in arrays if a is not None)

    def _mppi_out(self, shape, device):
        if device:
            import torch
            return torch.empty(shape, dtype=torch.float64, device=self._torch_device())
        return np.zeros(shape)

    def sample_controls(self, sigma, ncand, U_mean=None, device=None, **draw):
        """The S = ncand candidate controls the refinement draws around U_mean (B, N, nu), or around the live plan's U when it is None
        (cddp_hip_sample_controls): (B, S, N, nu), u = U_mean + sigma * z clipped to [u_lower, u_upper], z a standard normal that is a
        function of (seed, stream, trajectory, candidate, element) alone.  draw: seed, stream, keep_mean, u_lower, u_upper.  numpy in, numpy
        out; a device tensor in (or device=True with U_mean None), a device tensor out."""
        who = "sample_controls"
        B, N, nu = self.B, self.p.N, self.p.nu
        d, keep = self._mppi_desc(who, sigma, ncand, **draw)
        dev = self._is_device(U_mean) if device is None else bool(device)
        if U_mean is not None:
            U_mean = self._score_arg(who, "U_mean", U_mean, [(B, N, nu)], dev)
        out = self._mppi_out((B, d.ncand, N, nu), dev)
        if dev:
            self._order_device_io()
        self._check(self.lib.cddp_hip_sample_controls(self.h, SCORE_DEVICE if dev else 0, C.addressof(d), self._addr(U_mean), self._addr(out)))
        return out

    def mppi_blend(self, U_mean, U_cand, cost, viol=None, lam=1.0, viol_tol=0.0, u_lower=None, u_upper=None):
        """Softmin weights and blend over candidates the caller supplies (cddp_hip_mppi_blend): U_mean (B, N, nu), U_cand (B, S, N, nu),
        cost and viol (B, S) (viol None: all 0).  Admissible = finite with viol <= viol_tol; w_c = exp(-(cost_c - rho) / lam) / eta over the
        admissible candidates, rho their lowest cost; U' = U_mean + sum_c w_c (U_c - U_mean), clipped to the box.  Returns (U', stats), stats
        (B, 3) = n_adm, rho, ess; a trajectory without an admissible candidate keeps its mean.  numpy arrays or device tensors, of one kind."""
        who = "mppi_blend"
        B, N, nu = self.B, self.p.N, self.p.nu
        if U_mean is None or U_cand is None or cost is None:
            raise ValueError("%s: U_mean, U_cand and cost are required" % who)
        if len(tuple(np.shape(U_cand))) != 4 or int(np.shape(U_cand)[1]) < 1:
            raise ValueError("%s: U_cand: shape (%d, S, %d, %d) with S >= 1 is expected, got %s" % (who, B, N, nu, tuple(np.shape(U_cand))))
        S = int(np.shape(U_cand)[1])
        d, keep = self._mppi_desc(who, 1.0, S, lam=lam, viol_tol=viol_tol, u_lower=u_lower, u_upper=u_upper)
        dev = self._is_device(U_cand)
        U_mean = self._score_arg(who, "U_mean", U_mean, [(B, N, nu)], dev)
        U_cand = self._score_arg(who, "U_cand", U_cand, [(B, S, N, nu)], dev)
        cost = self._score_arg(who, "cost", cost, [(B, S)], dev)
        if viol is not None:
            viol = self._score_arg(who, "viol", viol, [(B, S)], dev)
        out = self._mppi_out((B, N, nu), dev); stats = self._mppi_out((B, 3), dev)
        if dev:
            self._order_device_io()
        self._check(self.lib.cddp_hip_mppi_blend(self.h, SCORE_DEVICE if dev else 0, C.addressof(d), self._addr(U_mean), self._addr(U_cand),
                                                 self._addr(cost), self._addr(viol), self._addr(out), self._addr(stats)))
        return out, stats

    def mppi_refine(self, sigma, ncand, x0=None, U_mean=None, plant=None, seed_handle=False, device=None, **draw):
        """`iters` rounds of draw -> roll out -> softmin weights -> blend around U_mean (B, N, nu; None: the live plan's U), from x0 (B, nx;
        None: row 0 of the live plan), on the handle's model or a DevicePlant (cddp_hip_mppi_refine).  The candidates are drawn inside the
        kernels: no (B, S, N, nu) array exists.  draw: lam, seed, stream, iters, keep_mean, viol_tol, u_lower, u_upper; round k draws from
        stream + k.  Returns a dict: "U" (B, N, nu) the refined mean, "cost" and "viol" (B, S) and "stats" (B, 3) = n_adm, rho, ess of the
        last round.  seed_handle=True leaves the handle as set_initial_device(x0, U) leaves it.  numpy arrays or device tensors (device=True
        when both arrays are None); the handle's solver state is otherwise untouched."""
        who = "mppi_refine"
        B, N, nx, nu = self.B, self.p.N, self.p.nx, self.p.nu
        d, keep = self._mppi_desc(who, sigma, ncand, **draw)
        dev = self._is_device(x0, U_mean) if device is None else bool(device)
        if x0 is not None:
            x0 = self._score_arg(who, "x0", x0, [(B, nx)], dev)
        if U_mean is not None:
            U_mean = self._score_arg(who, "U_mean", U_mean, [(B, N, nu)], dev)
        S = d.ncand
        out = {"U": self._mppi_out((B, N, nu), dev), "cost": self._mppi_out((B, S), dev), "viol": self._mppi_out((B, S), dev),
               "stats": self._mppi_out((B, 3), dev)}
        flags = (SCORE_DEVICE if dev else 0) | (MPPI_SEED if seed_handle else 0)
        if dev:
            self._order_device_io()
        self._check(self.lib.cddp_hip_mppi_refine(self.h, plant.h if plant is not None else None, flags, C.addressof(d), self._addr(x0),
                                                  self._addr(U_mean), self._addr(out["U"]), self._addr(out["cost"]), self._addr(out["viol"]),
                                                  self._addr(out["stats"])))
        return out

    # ---- Monte-Carlo evaluation of the plan under noise (cddp_hip_mc_sample_noise / cddp_hip_plan_montecarlo): the conventions of
    # score_rollouts for the arrays; the covariances (or their factors) are small host arrays
    def _mc_desc(self, who, Sigma0, W, Wu, nsamp, seed=0, stream=0, keep_nominal=False, viol_tol=0.0, factors=False):
        """-> (McDesc, the arrays it points into).  Covariances are factored on the host with numpy.linalg.cholesky; factors=True takes the
        lower-triangular factors themselves.  What can be refused without the library is refused here with ValueError."""
        nx, nu = self.p.nx, self.p.nu
        nsamp = int(nsamp); seed = int(seed); stream = int(stream); viol_tol = float(viol_tol)
        if not 1 <= nsamp <= MC_MAX_SAMPLES:
            raise ValueError("%s: nsamp: 1 to %d samples are expected, got %d" % (who, MC_MAX_SAMPLES, nsamp))
        if not 0 <= seed < 2 ** 64 or not 0 <= stream < 2 ** 32:
            raise ValueError("%s: seed is a 64-bit and stream a 32-bit unsigned number, got %r and %r" % (who, seed, stream))
        if viol_tol != viol_tol:
            raise ValueError("%s: viol_tol is NaN" % who)
        d = McDesc()
        d.seed = seed; d.stream = stream; d.nsamp = nsamp; d.keep_nominal = 1 if keep_nominal else 0; d.viol_tol = viol_tol
        keep = []
        for field, name, a, n in (("L0", "Sigma0", Sigma0, nx), ("Lw", "W", W, nx), ("Lu", "Wu", Wu, nu)):
            if a is None:
                continue
            if hasattr(a, "data_ptr") and not isinstance(a, np.ndarray):
                a = a.detach().cpu().numpy()     # (nx x nx at most: the factors are host arrays of the C entry)
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (n, n) or not np.isfinite(a).all():
                raise ValueError("%s: %s: a finite (%d, %d) matrix is expected, got shape %s" % (who, name, n, n, a.shape))
            if not factors:
                try:
                    a = np.linalg.cholesky(a)
                except np.linalg.LinAlgError:
                    raise ValueError("%s: %s is not positive definite (pass a factor with factors=True for a semidefinite one)" % (who, name))
            L = np.ascontiguousarray(np.tril(a))
            keep.append(L)
            setattr(d, field, _ptr(L))
        return d, keep

    def mc_sample_noise(self, Sigma0=None, W=None, Wu=None, nsamp=1, device=False, want=("Z0", "E", "Wn"), **draw):
        """The coloured noise plan_montecarlo draws (cddp_hip_mc_sample_noise): a dict of "Z0" (B, S, nx), "E" (B, S, N, nu), "Wn" (B, S, N,
        nx), each L z with z a standard normal that is a function of (seed, stream, trajectory, sample, element) alone; a source whose
        covariance is None is all zeros.  draw: seed, stream, keep_nominal, factors.  numpy arrays, or device tensors with device=True."""
        who = "mc_sample_noise"
        want = tuple(want)
        if not want or any(w not in ("Z0", "E", "Wn") for w in want):
            raise ValueError("%s: want: a non-empty subset of ('Z0', 'E', 'Wn') is expected, got %r" % (who, want))
        B, N, nx, nu = self.B, self.p.N, self.p.nx, self.p.nu
        d, keep = self._mc_desc(who, Sigma0, W, Wu, nsamp, **draw)
        S = d.nsamp
        shapes = {"Z0": (B, S, nx), "E": (B, S, N, nu), "Wn": (B, S, N, nx)}
        out = {k: self._mppi_out(shapes[k], device) for k in want}
        if device:
            self._order_device_io()
        self._check(self.lib.cddp_hip_mc_sample_noise(self.h, MC_DEVICE if device else 0, C.addressof(d), self._addr(out.get("Z0")),
                                                      self._addr(out.get("E")), self._addr(out.get("Wn"))))
        return out

    def plan_montecarlo(self, Sigma0=None, W=None, Wu=None, nsamp=64, seed=0, stream=0, keep_nominal=False, plant=None, x0=None, viol_tol=0.0,
                        diag=False, factors=False, want=("stats", "nviol_step", "dXmean", "SX", "dUmean", "SU"), device=None):
        """S = nsamp noisy closed-loop rollouts per trajectory around the live plan, reduced on the device (cddp_hip_plan_montecarlo):
        x_0 = x0 + L0 z, u_t = clip(U_t + Lu z + K_t (x_t - X_t)), x_{t+1} = f(x_t, u_t) + Lw z on the handle's model or a DevicePlant, with
        Sigma0 = L0 L0^T, W = Lw Lw^T, Wu = Lu Lu^T (None: no such noise; factors=True: the arguments are the lower-triangular factors).
        x0: (B, nx) or None (row 0 of the live plan), a numpy array or a torch.float64 tensor on the handle's device; device tensors in (or
        device=True) give device tensors back.  want: any of MC_OUTPUTS -- "cost", "viol" (B, S); "stats" (B, 8) in the order of MC_STATS;
        "nviol_step" (B, N + 1) int32, the samples whose rows of step t exceed viol_tol; "dXmean" (B, N + 1, nx), "SX" (B, N + 1, nx, nx),
        "dUmean" (B, N, nu), "SU" (B, N, nu, nu): sample mean and covariance of x - X_t and of the applied control minus U_t (diag=True:
        the diagonals, (B, N + 1, nx) and (B, N, nu)); "X" (B, S, N + 1, nx) and "U" (B, S, N, nu), the only outputs of that size.  The
        noise is a function of (seed, stream, trajectory, sample, element) alone; keep_nominal makes sample 0 noise-free.  The handle's
        solver state is not modified."""
        who = "plan_montecarlo"
        want = tuple(want)
        if not want or any(w not in MC_OUTPUTS for w in want):
            raise ValueError("%s: want: a non-empty subset of %r is expected, got %r" % (who, MC_OUTPUTS, want))
        B, N, nx, nu = self.B, self.p.N, self.p.nx, self.p.nu
        d, keep = self._mc_desc(who, Sigma0, W, Wu, nsamp, seed=seed, stream=stream, keep_nominal=keep_nominal, viol_tol=viol_tol, factors=factors)
        S = d.nsamp
        dev = self._is_device(x0) if device is None else bool(device)
        if x0 is not None:
            x0 = self._score_arg(who, "x0", x0, [(B, nx)], dev)
        shapes = {"cost": (B, S), "viol": (B, S), "stats": (B, 8), "nviol_step": (B, N + 1), "dXmean": (B, N + 1, nx),
                  "SX": (B, N + 1, nx) if diag else (B, N + 1, nx, nx), "dUmean": (B, N, nu), "SU": (B, N, nu) if diag else (B, N, nu, nu),
                  "X": (B, S, N + 1, nx), "U": (B, S, N, nu)}
        out = {}
        for k in want:
            if k == "nviol_step":
                if dev:
                    import torch
                    out[k] = torch.empty(shapes[k], dtype=torch.int32, device=self._torch_device())
                else:
                    out[k] = np.zeros(shapes[k], dtype=np.int32)
            else:
                out[k] = self._mppi_out(shapes[k], dev)
        if dev:
            self._order_device_io()
        flags = (MC_DEVICE if dev else 0) | (MC_DIAG if diag else 0)
        self._check(self.lib.cddp_hip_plan_montecarlo(self.h, plant.h if plant is not None else None, flags, C.addressof(d), self._addr(x0),
                                                      *[self._addr(out.get(k)) for k in MC_OUTPUTS]))
        return out

    # ---- Monte-Carlo evaluation under output feedback (cddp_hip_mc_sample_meas_noise / cddp_hip_plan_montecarlo_of): plan_montecarlo's
    # conventions; C and v are small host arrays as the factors are, the gains L follow the pointer kind of the call
    def _mcof_desc(self, who, Cm, v, Sigma0, W, Wu, nsamp, need_C=True, **draw):
        """-> (McofDesc, the arrays it points into): _mc_desc's descriptor with the sensor model C (ny, nx), v (ny,) behind it."""
        mc, keep = self._mc_desc(who, Sigma0, W, Wu, nsamp, **draw)
        host = lambda a: a.detach().cpu().numpy() if hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) else a
        if v is None or (need_C and Cm is None):
            raise ValueError("%s: C and v must be given" % who)
        v = np.ascontiguousarray(host(v), dtype=np.float64)
        if v.ndim != 1 or not 1 <= v.shape[0] <= KF_MAX_NY:
            raise ValueError("%s: v: 1 .. %d measurement rows are expected, got shape %s" % (who, KF_MAX_NY, v.shape))
        if not (np.isfinite(v).all() and (v > 0).all()):
            raise ValueError("%s: v: finite variances > 0 are expected" % who)
        d = McofDesc()
        d.mc = mc
        d.ny = int(v.shape[0])
        d.v = _ptr(v)
        keep.append(v)
        if Cm is not None:
            Cm = np.ascontiguousarray(host(Cm), dtype=np.float64)
            if Cm.shape != (d.ny, self.p.nx) or not np.isfinite(Cm).all():
                raise ValueError("%s: C: a finite matrix of shape %s is expected, got shape %s" % (who, (d.ny, self.p.nx), Cm.shape))
            d.C = _ptr(Cm)
            keep.append(Cm)
        return d, keep

    def mc_sample_meas_noise(self, v, nsamp=1, device=False, **draw):
        """The measurement noise plan_montecarlo_of draws (cddp_hip_mc_sample_meas_noise): (B, S, N + 1, ny), sqrt(v[r]) * z with z the
        standard normal of element nx + N (nu + nx) + t ny + r of plan_montecarlo's generator.  draw: seed, stream, keep_nominal.  A numpy
        array, or a device tensor with device=True."""
        who = "mc_sample_meas_noise"
        d, keep = self._mcof_desc(who, None, v, None, None, None, nsamp, need_C=False, **draw)
        out = self._mppi_out((self.B, d.mc.nsamp, self.p.N + 1, d.ny), device)
        if device:
            self._order_device_io()
        self._check(self.lib.cddp_hip_mc_sample_meas_noise(self.h, MC_DEVICE if device else 0, C.addressof(d), self._addr(out)))
        return out

    def plan_montecarlo_of(self, C_, v, L, Sigma0=None, W=None, Wu=None, nsamp=64, seed=0, stream=0, keep_nominal=False, plant=None, x0=None,
                           viol_tol=0.0, diag=False, factors=False, want=("stats", "nviol_step", "dXmean", "SX", "dUmean", "SU", "dEmean", "SE"),
                           device=None):
        """plan_montecarlo with the controller seeing only y_t = C dx_t + n_t, cov(n_t) = diag(v) (cddp_hip_plan_montecarlo_of): every
        sample carries the estimate xh of x - X_t of a linearised Kalman filter with the gains L (B, N + 1, nx, ny) -- plan_kalman's "L", or
        any gains -- updated by the measurement at every step, fed back as u_t = clip(U_t + Lu z + K_t xh) and predicted with A_t, B_t of
        the handle's stacks.  C_ (ny, nx) and v (ny,) are small host arrays (tensors are copied to the host); Sigma0, W, Wu, nsamp, seed,
        stream, keep_nominal, plant, x0, viol_tol, diag, factors as in plan_montecarlo, and the initial, actuator and process noise of a
        sample are plan_montecarlo's at the same (seed, stream).  L and x0: numpy arrays, or torch.float64 tensors on the handle's device
        (device tensors back), never mixed.  want: any of MCOF_OUTPUTS -- plan_montecarlo's, "dEmean" (B, N + 1, nx) and "SE" (B, N + 1, nx,
        nx; diag=True: (B, N + 1, nx)), sample mean and covariance of the estimation error (x - X_t) - xh after the measurement of step t,
        and "Xh" (B, S, N + 1, nx), the estimates.  The handle's state is not modified."""
        who = "plan_montecarlo_of"
        want = tuple(want)
        if not want or any(w not in MCOF_OUTPUTS for w in want):
            raise ValueError("%s: want: a non-empty subset of %r is expected, got %r" % (who, MCOF_OUTPUTS, want))
        if L is None:
            raise ValueError("%s: the filter gains L must be given" % who)
        B, N, nx, nu = self.B, self.p.N, self.p.nx, self.p.nu
        d, keep = self._mcof_desc(who, C_, v, Sigma0, W, Wu, nsamp, seed=seed, stream=stream, keep_nominal=keep_nominal, viol_tol=viol_tol, factors=factors)
        S, ny = d.mc.nsamp, d.ny
        dev = self._is_device(L, x0) if device is None else bool(device)
        L = self._score_arg(who, "L", L, [(B, N + 1, nx, ny)], dev)
        if x0 is not None:
            x0 = self._score_arg(who, "x0", x0, [(B, nx)], dev)
        sx = (B, N + 1, nx) if diag else (B, N + 1, nx, nx)
        shapes = {"cost": (B, S), "viol": (B, S), "stats": (B, 8), "nviol_step": (B, N + 1), "dXmean": (B, N + 1, nx), "SX": sx,
                  "dUmean": (B, N, nu), "SU": (B, N, nu) if diag else (B, N, nu, nu), "X": (B, S, N + 1, nx), "U": (B, S, N, nu),
                  "dEmean": (B, N + 1, nx), "SE": sx, "Xh": (B, S, N + 1, nx)}
        out = {}
        for k in want:
            if k == "nviol_step":
                if dev:
                    import torch
                    out[k] = torch.empty(shapes[k], dtype=torch.int32, device=self._torch_device())
                else:
                    out[k] = np.zeros(shapes[k], dtype=np.int32)
            else:
                out[k] = self._mppi_out(shapes[k], dev)
        if dev:
            self._order_device_io()
        flags = (MC_DEVICE if dev else 0) | (MC_DIAG if diag else 0)
        self._check(self.lib.cddp_hip_plan_montecarlo_of(self.h, plant.h if plant is not None else None, flags, C.addressof(d), self._addr(x0),
                                                         self._addr(L), *[self._addr(out.get(k)) for k in MCOF_OUTPUTS]))
        return out


class DevicePlant:
    """A device-resident plant for a batch of trajectories (cddp_hip_plant): a built-in model with its own parameters (shared, or one row
    per trajectory: params of shape (batch, n)), integrator, `substeps` steps of dt / substeps per control interval, and an optional
    control box the commanded control is clipped to.  Used by HipBatchSolver.mpc_run_plant / track_plan, or stepped directly."""

    def __init__(self, model, integrator, dt, nx, nu, batch, params=(), substeps=1, u_lower=None, u_upper=None, lti_A=None, lti_B=None,
                 device=0, trig=None):
        self.lib = load_hip(trig)
        self.B, self.nx, self.nu, self._device = int(batch), int(nx), int(nu), int(device)
        pv = np.asarray(params, dtype=np.float64)
        per = pv.ndim == 2
        mp = np.zeros((self.B if per else 1, MAX_MODEL_PARAMS))
        if pv.size:
            mp[:, :pv.shape[-1]] = pv
        self.keep = [np.ascontiguousarray(mp)]
        d = PlantDesc()
        d.abi_version = ABI_VERSION; d.model = int(model); d.integrator = int(integrator); d.substeps = int(substeps)
        d.nx = self.nx; d.nu = self.nu; d.params_per_trajectory = 1 if per else 0; d.dt = float(dt)
        d.model_params = _ptr(self.keep[0])
        for name, v in (("lti_A", lti_A), ("lti_B", lti_B), ("u_lower", u_lower), ("u_upper", u_upper)):
            if v is not None:
                a = _arr(v); self.keep.append(a); setattr(d, name, _ptr(a))
        self.desc = d
        self.h = C.c_void_p()
        rc = self.lib.cddp_hip_plant_create(C.byref(d), self.B, self._device, C.byref(self.h))
        if rc != 0:
            raise HipError("cddp_hip error %d: %s" % (rc, self.lib.cddp_hip_last_error().decode()))

    @classmethod
    def of_problem(cls, problem, batch, **over):
        """The plant of a Problem -- its model, parameters, integrator, dt (and LTI matrices) --, with any of them overridden by keyword."""
        c = problem.c
        kw = dict(model=c.model, integrator=c.integrator, dt=c.dt, nx=c.nx, nu=c.nu, params=list(c.model_params),
                  lti_A=getattr(problem, "lti_A", None), lti_B=getattr(problem, "lti_B", None))
        kw.update(over)
        return cls(batch=batch, **kw)

    def _check(self, rc):
        if rc != 0:
            raise HipError("cddp_hip error %d: %s" % (rc, self.lib.cddp_hip_last_error().decode()))

    def step(self, x, u, w=None):
        """x_next = plant(x, u) + w for every trajectory.  numpy arrays (B, nx), (B, nu), (B, nx): uploaded, computed, returned as numpy.
        torch tensors on the plant's device (float64): read and written in place on the device, after a synchronisation of their
        current stream (as HipBatchSolver.mpc_advance treats a device x_next); a torch tensor is returned."""
        if hasattr(x, "data_ptr") and not isinstance(x, np.ndarray):
            import torch
            ts = [("x", x, self.nx), ("u", u, self.nu)] + ([("w", w, self.nx)] if w is not None else [])
            keep = []
            for name, t, n in ts:
                if not hasattr(t, "data_ptr") or not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != (self.B, n):
                    raise ValueError("%s: a float64 device tensor of shape (%d, %d) is expected" % (name, self.B, n))
                if t.device.index != self._device:
                    raise ValueError("%s lives on device %s, the plant on device %d" % (name, t.device.index, self._device))
                keep.append(t.contiguous())
            out = torch.empty_like(keep[0])
            torch.cuda.current_stream(out.device).synchronize()
            self._check(self.lib.cddp_hip_plant_step(self.h, PLANT_DEVICE, keep[0].data_ptr(), keep[1].data_ptr(),
                                                     keep[2].data_ptr() if w is not None else None, out.data_ptr()))
            return out
        xa = _arr(x).reshape(self.B, self.nx); ua = _arr(u).reshape(self.B, self.nu)
        wa = _arr(w).reshape(self.B, self.nx) if w is not None else None
        out = np.zeros((self.B, self.nx))
        self._check(self.lib.cddp_hip_plant_step(self.h, 0, xa.ctypes.data, ua.ctypes.data, wa.ctypes.data if wa is not None else None, out.ctypes.data))
        return out

    def close(self):
        if self.h:
            self.lib.cddp_hip_plant_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceEkf:
    """A device-resident extended Kalman filter for a batch of trajectories (cddp_hip_ekf) with a DevicePlant as its model: sensors
    y = C x + n, cov(n) = diag(v); C (ny, nx) and v (ny,) shared by the batch, or (B, ny, nx) and (B, ny) -- then W (nx, nx) and Wu (nu, nu),
    where given, carry the batch axis too.  reset / update / predict / get / run take numpy arrays (uploaded, computed, returned as numpy)
    or float64 torch tensors on the plant's device (read and written in place, after a synchronisation of their current stream; torch
    tensors are returned).  The plant must outlive the filter: the object keeps a reference to it."""

    def __init__(self, plant, C_, v, W=None, Wu=None):
        self.lib = plant.lib
        self.plant = plant
        self.B, self.nx, self.nu, self._device = plant.B, plant.nx, plant.nu, plant._device
        Ca = _arr(C_); va = _arr(v)
        per = Ca.ndim == 3
        self.ny = int(Ca.shape[-2]) if Ca.ndim >= 2 else 0
        lead = (self.B,) if per else ()
        self.keep = [Ca.reshape(lead + (self.ny, self.nx)), va.reshape(lead + (self.ny,))]
        d = EkfDesc()
        d.abi_version = ABI_VERSION; d.ny = self.ny; d.per_trajectory = 1 if per else 0
        d.C = _ptr(self.keep[0]); d.v = _ptr(self.keep[1])
        for name, M, n in (("W", W, self.nx), ("Wu", Wu, self.nu)):
            if M is not None:
                a = _arr(M).reshape(lead + (n, n)); self.keep.append(a); setattr(d, name, _ptr(a))
        self.desc = d
        self.h = C.c_void_p()
        self._check(self.lib.cddp_hip_ekf_create(plant.h, C.byref(d), C.byref(self.h)))

    def _check(self, rc):
        if rc != 0:
            raise HipError("cddp_hip error %d: %s" % (rc, self.lib.cddp_hip_last_error().decode()))

    @staticmethod
    def _is_torch(a):
        return a is not None and hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)

    def _args(self, named):
        """named: (name, array or None, shape) triples, all numpy-like or all device tensors -> (device?, the arrays kept, their addresses)"""
        dev = any(self._is_torch(a) for _, a, _ in named)
        keep, ptrs = [], []
        for name, a, shape in named:
            if a is None:
                keep.append(None); ptrs.append(None); continue
            if dev:
                import torch
                if not self._is_torch(a) or not a.is_cuda or a.dtype != torch.float64 or tuple(a.shape) != tuple(shape):
                    raise ValueError("%s: a float64 device tensor of shape %s is expected" % (name, tuple(shape)))
                if a.device.index != self._device:
                    raise ValueError("%s lives on device %s, the estimator on device %d" % (name, a.device.index, self._device))
                t = a.contiguous(); keep.append(t); ptrs.append(t.data_ptr())
            else:
                t = _arr(a).reshape(shape); keep.append(t); ptrs.append(t.ctypes.data)
        if dev:
            import torch
            torch.cuda.current_stream(torch.device("cuda", self._device)).synchronize()
        return dev, keep, ptrs

    def _out(self, dev, shape, dtype=np.float64):
        if dev:
            import torch
            return torch.empty(shape, dtype=torch.float64 if dtype == np.float64 else torch.int32, device=torch.device("cuda", self._device))
        return np.zeros(shape, dtype=dtype)

    @staticmethod
    def _addr(a):
        return None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)

    def reset(self, xh0, P0):
        """xh <- xh0 (B, nx); P <- P0 (nx, nx) for the batch or (B, nx, nx), its lower triangle mirrored; info and the step count <- 0"""
        per = len(P0.shape) == 3 if hasattr(P0, "shape") else np.asarray(P0).ndim == 3
        dev, keep, ptrs = self._args([("xh0", xh0, (self.B, self.nx)), ("P0", P0, ((self.B,) if per else ()) + (self.nx, self.nx))])
        self._check(self.lib.cddp_hip_ekf_reset(self.h, (EKF_DEVICE if dev else 0) | (EKF_PER_TRAJ if per else 0), ptrs[0], ptrs[1]))

    def update(self, y, skip_nan=False):
        """The measurement update with y (B, ny) -> nis (B,).  skip_nan: a NaN in y is a missing measurement."""
        dev, keep, ptrs = self._args([("y", y, (self.B, self.ny))])
        nis = self._out(dev, (self.B,))
        self._check(self.lib.cddp_hip_ekf_update(self.h, (EKF_DEVICE if dev else 0) | (EKF_SKIP_NAN if skip_nan else 0), ptrs[0], self._addr(nis)))
        return nis

    def predict(self, u):
        """The prediction with the commanded control u (B, nu): the model plant clips it."""
        dev, keep, ptrs = self._args([("u", u, (self.B, self.nu))])
        self._check(self.lib.cddp_hip_ekf_predict(self.h, EKF_DEVICE if dev else 0, ptrs[0]))

    def get(self, device=False):
        """(xh (B, nx), P (B, nx, nx), info (B,) int32) of the object, as numpy arrays or (device=True) torch tensors"""
        xh = self._out(device, (self.B, self.nx)); P = self._out(device, (self.B, self.nx, self.nx)); info = self._out(device, (self.B,), np.int32)
        self._check(self.lib.cddp_hip_ekf_get(self.h, EKF_DEVICE if device else 0, self._addr(xh), self._addr(P), self._addr(info)))
        return xh, P, info

    def run(self, Y, U=None, skip_nan=False, diag=False, want=("Xh", "P", "nis", "info")):
        """A whole log in one launch from the object's state: Y (B, T + 1, ny), U (B, T, nu) (None at T = 0) -> dict of the wanted
        Xh (B, T + 1, nx), P (B, T + 1, nx, nx) (diag: (B, T + 1, nx)), nis (B, T + 1), info (B,)."""
        T = int(Y.shape[1]) - 1
        dev, keep, ptrs = self._args([("Y", Y, (self.B, T + 1, self.ny)), ("U", U if T > 0 else None, (self.B, T, self.nu))])
        shapes = {"Xh": (self.B, T + 1, self.nx), "P": (self.B, T + 1, self.nx) + (() if diag else (self.nx,)), "nis": (self.B, T + 1), "info": (self.B,)}
        out = {k: self._out(dev, shapes[k], np.int32 if k == "info" else np.float64) for k in want}
        flags = (EKF_DEVICE if dev else 0) | (EKF_SKIP_NAN if skip_nan else 0) | (EKF_DIAG if diag else 0)
        self._check(self.lib.cddp_hip_ekf_run(self.h, flags, T, ptrs[0], ptrs[1], *[self._addr(out.get(k)) for k in ("Xh", "P", "nis", "info")]))
        return out

    def close(self):
        if self.h:
            self.lib.cddp_hip_ekf_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def model_eval(model, integrator, dt, params, nx, nu, x, u, want=("step",), trig=None):
    """cddp_hip_model_eval: host evaluation of a built-in plant at one (x, u).  want: any of "step" (x_next), "jac" (f_x, f_u
    continuous-time), "hess" (f_xx[nx][nx][nx], f_uu[nx][nu][nu], f_ux[nx][nu][nx]).  Returns a dict."""
    lib = load_hip(trig)
    pv = np.zeros(MAX_MODEL_PARAMS); pv[:len(params)] = params
    x = _arr(x).reshape(nx); u = _arr(u).reshape(nu)
    out = {}
    xn = np.empty(nx) if "step" in want else None
    fx = np.empty((nx, nx)) if "jac" in want else None; fu = np.empty((nx, nu)) if "jac" in want else None
    fxx = np.empty((nx, nx, nx)) if "hess" in want else None; fuu = np.empty((nx, nu, nu)) if "hess" in want else None
    fux = np.empty((nx, nu, nx)) if "hess" in want else None
    lib.cddp_hip_model_eval.restype = C.c_int
    rc = lib.cddp_hip_model_eval(int(model), int(integrator), C.c_double(dt), _ptr(pv), int(nx), int(nu), _ptr(x), _ptr(u),
                                 _ptr(xn), _ptr(fx), _ptr(fu), _ptr(fxx), _ptr(fuu), _ptr(fux))
    if rc != 0:
        lib.cddp_hip_last_error.restype = C.c_char_p
        raise HipError(lib.cddp_hip_last_error().decode())
    if xn is not None: out["step"] = xn
    if fx is not None: out["jac"] = (fx, fu)
    if fxx is not None: out["hess"] = (fxx, fuu, fux)
    return out


# ---- host plug-in solve (include/cddp_hip.h: cddp_hip_plugin / cddp_hip_plugin_solve) ----------------------------------------
PLUGIN_MAX_CONSTRAINTS = 8
_F_DYN = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, C.c_double, _dp)
_F_JAC = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, C.c_double, _dp, _dp)
_F_HES = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, C.c_double, _dp, _dp, _dp)
_F_RC = C.CFUNCTYPE(C.c_double, C.c_void_p, _dp, _dp, C.c_int)
_F_TC = C.CFUNCTYPE(C.c_double, C.c_void_p, _dp)
_F_RCD = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp)
_F_TCD = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, _dp)
_F_CON = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp)
_F_CHS = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp)


class PluginStruct(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("options_bytes", C.c_int32), ("abort_flag", C.POINTER(C.c_int32)),
        ("user", C.c_void_p), ("nx", C.c_int32), ("nu", C.c_int32), ("n_constraints", C.c_int32),
        ("constraint_dims", C.c_int32 * PLUGIN_MAX_CONSTRAINTS),
        ("discrete_dynamics", _F_DYN), ("jacobians", _F_JAC), ("hessians", _F_HES),
        ("running_cost", _F_RC), ("terminal_cost", _F_TC), ("running_cost_derivatives", _F_RCD),
        ("terminal_cost_derivatives", _F_TCD), ("constraints", _F_CON),
        ("control_lower", _dp), ("control_upper", _dp), ("constraint_hessians", _F_CHS),
    ]


_F_TERM = C.CFUNCTYPE(None, C.c_void_p, _dp, _dp, _dp)


class PluginTerminalStruct(C.Structure):   # cddp_hip_plugin_terminal
    _fields_ = [("n_terminal", C.c_int32), ("dims", C.c_int32 * PLUGIN_MAX_CONSTRAINTS), ("equality", C.c_int32 * PLUGIN_MAX_CONSTRAINTS), ("evaluate", _F_TERM)]


def plugin_solve(solver, nx, nu, horizon, dt, options, x0, U0=None, X0=None, *, discrete_dynamics, jacobians, running_cost, terminal_cost,
                 running_cost_derivatives, terminal_cost_derivatives, hessians=None, constraints=None, constraint_dims=(),
                 control_lower=None, control_upper=None, constraint_hessians=None, device=0, trig=None,
                 terminal=None, terminal_dims=(), terminal_equality=(), want_terminal=False):
    """CDDP::solve() for HOST plug-ins through the C-ABI (cddp_hip_plugin_solve): the callables are the reference's virtual functions
    on numpy vectors -- discrete_dynamics(x, u, t) -> x_next; jacobians(x, u, t) -> (f_x, f_u) continuous-time;
    hessians(x, u, t) -> (f_xx[nx][nx][nx], f_uu[nx][nu][nu], f_ux[nx][nu][nx]); running_cost(x, u, index) -> float;
    terminal_cost(x) -> float; running_cost_derivatives(x, u, index) -> (l_x, l_u, l_xx, l_uu, l_ux); terminal_cost_derivatives(x)
    -> (l_x, l_xx); constraints(x, u, index, want_jacobians) -> (g - upper, G_x, G_u) stacked in name order.  The GPU runs the
    batched backward passes, the host the forward passes.  An exception raised by a callable stops the solve and is re-raised here.
    solver = SOLVER_LOGDDP runs the reference's LogDDP on the same callbacks; constraint_hessians(x, u, index) -> (g_xx[m][nx][nx],
    g_uu[m][nu][nu], g_ux[m][nu][nx]) or None supplies constraint curvature to its relaxed log barrier.  Returns (results, X, U, K).
    terminal(x_N, want_jacobian) -> (r, r_x) with the residual rows of every terminal-constraint object stacked in name order (terminal_dims,
    terminal_equality: 1 = TerminalEqualityConstraint-like, 0 = inequality g_T <= 0) runs cddp_hip_plugin_solve_terminal; want_terminal adds a
    fifth return value, the dict {S_T, Y_T, Lambda_T} of the final iterate."""
    lib = load_hip(trig)
    x0 = _arr(x0).reshape(-1, nx); B = x0.shape[0]; N = int(horizon)
    U0 = _arr(U0).reshape(B, N, nu) if U0 is not None else None
    X0 = _arr(X0).reshape(B, N + 1, nx) if X0 is not None else None
    m = int(sum(constraint_dims))
    err = []

    def vec(ptr, n):
        return np.ctypeslib.as_array(ptr, shape=(n,))

    abort = C.c_int32(0)

    def guard(fn, default=None):
        def w(*a):
            if err:
                return default
            try:
                return fn(*a)
            except BaseException as e:   # noqa: B902 -- re-raised by the caller thread after the C call returns
                err.append(e)
                abort.value = 1      # cddp_hip_plugin::abort_flag: the C solve returns at its next check instead of iterating on stale data
                return default
        return w

    def _dyn(_, x, u, t, out):
        vec(out, nx)[:] = np.asarray(discrete_dynamics(vec(x, nx).copy(), vec(u, nu).copy(), t), dtype=np.float64).reshape(nx)

    def _jac(_, x, u, t, fx, fu):
        a, b = jacobians(vec(x, nx).copy(), vec(u, nu).copy(), t)
        vec(fx, nx * nx)[:] = np.asarray(a, dtype=np.float64).reshape(nx * nx); vec(fu, nx * nu)[:] = np.asarray(b, dtype=np.float64).reshape(nx * nu)

    def _hes(_, x, u, t, fxx, fuu, fux):
        a, b, c2 = hessians(vec(x, nx).copy(), vec(u, nu).copy(), t)
        vec(fxx, nx * nx * nx)[:] = np.asarray(a, dtype=np.float64).reshape(-1); vec(fuu, nx * nu * nu)[:] = np.asarray(b, dtype=np.float64).reshape(-1)
        vec(fux, nx * nu * nx)[:] = np.asarray(c2, dtype=np.float64).reshape(-1)

    def _rc(_, x, u, idx):
        return float(running_cost(vec(x, nx).copy(), vec(u, nu).copy(), idx))

    def _tc(_, x):
        return float(terminal_cost(vec(x, nx).copy()))

    def _rcd(_, x, u, idx, lx, lu, lxx, luu, lux):
        a = running_cost_derivatives(vec(x, nx).copy(), vec(u, nu).copy(), idx)
        for dst, src, n in ((lx, a[0], nx), (lu, a[1], nu), (lxx, a[2], nx * nx), (luu, a[3], nu * nu), (lux, a[4], nu * nx)):
            vec(dst, n)[:] = np.asarray(src, dtype=np.float64).reshape(n)

    def _tcd(_, x, lx, lxx):
        a, b = terminal_cost_derivatives(vec(x, nx).copy())
        vec(lx, nx)[:] = np.asarray(a, dtype=np.float64).reshape(nx); vec(lxx, nx * nx)[:] = np.asarray(b, dtype=np.float64).reshape(nx * nx)

    def _con(_, x, u, idx, g, gx, gu):
        want = bool(gx) or bool(gu)
        gv, Gx, Gu = constraints(vec(x, nx).copy(), vec(u, nu).copy(), idx, want)
        vec(g, m)[:] = np.asarray(gv, dtype=np.float64).reshape(m)
        if gx: vec(gx, m * nx)[:] = np.asarray(Gx, dtype=np.float64).reshape(m * nx)
        if gu: vec(gu, m * nu)[:] = np.asarray(Gu, dtype=np.float64).reshape(m * nu)

    def _chs(_, x, u, idx, gxx, guu, gux):
        r = constraint_hessians(vec(x, nx).copy(), vec(u, nu).copy(), idx)
        if r is None:
            return
        vec(gxx, m * nx * nx)[:] = np.asarray(r[0], dtype=np.float64).reshape(-1); vec(guu, m * nu * nu)[:] = np.asarray(r[1], dtype=np.float64).reshape(-1)
        vec(gux, m * nu * nx)[:] = np.asarray(r[2], dtype=np.float64).reshape(-1)

    ps = PluginStruct()
    ps.nx, ps.nu, ps.n_constraints = nx, nu, len(constraint_dims)
    for i, dmy in enumerate(constraint_dims):
        ps.constraint_dims[i] = int(dmy)
    keep = [_F_DYN(guard(_dyn)), _F_JAC(guard(_jac)), _F_RC(guard(_rc, 0.0)), _F_TC(guard(_tc, 0.0)), _F_RCD(guard(_rcd)), _F_TCD(guard(_tcd))]
    ps.discrete_dynamics, ps.jacobians, ps.running_cost, ps.terminal_cost, ps.running_cost_derivatives, ps.terminal_cost_derivatives = keep
    if hessians is not None:
        keep.append(_F_HES(guard(_hes))); ps.hessians = keep[-1]
    if constraints is not None and m > 0:
        keep.append(_F_CON(guard(_con))); ps.constraints = keep[-1]
    if constraint_hessians is not None and m > 0:
        keep.append(_F_CHS(guard(_chs))); ps.constraint_hessians = keep[-1]
    lo = _arr(control_lower) if control_lower is not None else None
    up = _arr(control_upper) if control_upper is not None else None
    ps.control_lower, ps.control_upper = _ptr(lo), _ptr(up)
    ps.abi_version = ABI_VERSION; ps.options_bytes = C.sizeof(Options); ps.abort_flag = C.pointer(abort)
    res = np.zeros(B, dtype=RESULT_DTYPE)
    X = np.zeros((B, N + 1, nx)); U = np.zeros((B, N, nu)); K = np.zeros((B, N, nu, nx))
    tout = None
    if terminal is not None and len(terminal_dims) > 0:
        rows = int(sum(terminal_dims))
        mT = int(sum(d for d, e in zip(terminal_dims, terminal_equality) if not e)); pT = rows - mT

        def _term(_, x, r, rx):
            rv, Rx = terminal(vec(x, nx).copy(), bool(rx))
            vec(r, rows)[:] = np.asarray(rv, dtype=np.float64).reshape(rows)
            if rx: vec(rx, rows * nx)[:] = np.asarray(Rx, dtype=np.float64).reshape(rows * nx)

        ts = PluginTerminalStruct()
        ts.n_terminal = len(terminal_dims)
        for i, (dmy, e) in enumerate(zip(terminal_dims, terminal_equality)):
            ts.dims[i] = int(dmy); ts.equality[i] = 1 if e else 0
        keep.append(_F_TERM(guard(_term))); ts.evaluate = keep[-1]
        tbuf = np.zeros((B, max(1, 2 * mT + pT)))
        rc = lib.cddp_hip_plugin_solve_terminal(C.byref(ps), C.byref(ts), int(solver), N, C.c_double(dt), C.byref(options), int(device), B, _ptr(x0), _ptr(U0), _ptr(X0),
                                                res.ctypes.data_as(C.c_void_p), _ptr(X), _ptr(U), _ptr(K), _ptr(tbuf))
        tout = {"S_T": tbuf[:, :mT].copy(), "Y_T": tbuf[:, mT:2 * mT].copy(), "Lambda_T": tbuf[:, 2 * mT:2 * mT + pT].copy()}
    else:
        rc = lib.cddp_hip_plugin_solve(C.byref(ps), int(solver), N, C.c_double(dt), C.byref(options), int(device), B, _ptr(x0), _ptr(U0), _ptr(X0),
                                       res.ctypes.data_as(C.c_void_p), _ptr(X), _ptr(U), _ptr(K))
    if err:
        raise err[0]
    if rc != 0:
        raise HipError("cddp_hip error %d: %s" % (rc, lib.cddp_hip_last_error().decode()))
    if want_terminal:
        return res, X, U, K, tout
    return res, X, U, K


STACKS_CLDDP, STACKS_IPDDP, STACKS_IPDDP_PATH, STACKS_LOGDDP, STACKS_MSIPDDP, STACKS_MSIPDDP_PATH, STACKS_IPDDP_TERM_EQ = 0, 1, 2, 3, 4, 5, 6


class HipStackSolver:
    """Stack-fed backward pass bound to a handle (include/cddp_hip.h, "stack-fed mode"): the caller's host plugins fill the
    (N x batch) derivative stacks, the GPU sweeps them.  Arrays are batch-major numpy: fx (B,N,nx,nx), fu (B,N,nx,nu), lx (B,N,nx),
    lu (B,N,nu), lxx (B,N,nx,nx), luu (B,N,nu,nu), lux (B,N,nu,nx), VxN (B,nx), VxxN (B,nx,nx); y, s, g (B,N,m), Gx (B,N,m,nx),
    Gu (B,N,m,nu)."""

    def __init__(self, batch, nx, nu, m, horizon, device=0):
        self.lib = load_hip()
        self.B, self.nx, self.nu, self.m, self.N = batch, nx, nu, m, horizon
        self.h = C.c_void_p()
        self.lib.cddp_hip_stacks_last_kernel_ms.restype = C.c_double
        self._check(self.lib.cddp_hip_stacks_create_abi(ABI_VERSION, C.sizeof(Options), device, batch, nx, nu, m, horizon, C.byref(self.h)))

    def _check(self, rc):
        if rc != 0:
            raise HipError("cddp_hip error %d: %s" % (rc, self.lib.cddp_hip_last_error().decode()))

    def close(self):
        if self.h:
            self.lib.cddp_hip_stacks_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stacks(self, fx=None, fu=None, lx=None, lu=None, lxx=None, luu=None, lux=None, VxN=None, VxxN=None):
        a = [(_arr(v) if v is not None else None) for v in (fx, fu, lx, lu, lxx, luu, lux, VxN, VxxN)]
        self._check(self.lib.cddp_hip_set_stacks(self.h, *[_ptr(v) for v in a]))

    def set_defect_stack(self, defects=None):
        """Multiple-shooting defects f(x_t, u_t) - x_{t+1}, [B][N][nx] (MSIPDDP branch); None drops them."""
        a = _arr(defects) if defects is not None else None
        self._check(self.lib.cddp_hip_set_defect_stack(self.h, _ptr(a)))

    def set_control_box(self, lower=None, upper=None, U=None):
        """CLDDP branch: control bounds (nu each) and the current controls [B][N][nu]; all None removes the box."""
        a = [(_arr(v) if v is not None else None) for v in (lower, upper, U)]
        self._check(self.lib.cddp_hip_set_control_box(self.h, *[_ptr(v) for v in a]))

    def set_hessian_stacks(self, Fxx=None, Fuu=None, Fux=None):
        """dt-scaled dynamics Hessian tensors [B][N][nx][...] (full DDP); all None returns to Gauss-Newton."""
        a = [(_arr(v) if v is not None else None) for v in (Fxx, Fuu, Fux)]
        self._check(self.lib.cddp_hip_set_hessian_stacks(self.h, *[_ptr(v) for v in a]))

    def factor_cache(self, enable=True):
        """MSIPDDP's per-step factor cache (msipddp_solver.cpp:1169-1185): enable=True allocates / CLEARS it (start of a solve)."""
        self._check(self.lib.cddp_hip_stacks_factor_cache(self.h, 1 if enable else 0))

    def set_constraint_stacks(self, y=None, s=None, g=None, Gx=None, Gu=None):
        a = [(_arr(v) if v is not None else None) for v in (y, s, g, Gx, Gu)]
        self._check(self.lib.cddp_hip_set_constraint_stacks(self.h, *[_ptr(v) for v in a]))

    def set_terminal_equality(self, H_T, b_T, lambda_prev, reg_floor):
        """Terminal-equality branch (STACKS_IPDDP_TERM_EQ): H_T (B,pT,nx), b_T = -h_T (B,pT), lambda_prev (B,pT), reg_floor (B,)."""
        H = _arr(H_T); pT = H.shape[1]
        a = [_arr(b_T).reshape(self.B, pT), _arr(lambda_prev).reshape(self.B, pT), _arr(np.broadcast_to(np.asarray(reg_floor, dtype=np.float64), (self.B,)))]
        self.pT = pT
        self._check(self.lib.cddp_hip_set_terminal_equality(self.h, pT, _ptr(H), _ptr(a[0]), _ptr(a[1]), _ptr(a[2])))

    def terminal(self):
        dlam = np.zeros((self.B, self.pT)); dX = np.zeros((self.B, self.N + 1, self.nx))
        self._check(self.lib.cddp_hip_stacks_get_terminal(self.h, _ptr(dlam), _ptr(dX)))
        return dlam, dX

    def backward(self, branch, options, reg, mu=None, retry=False):
        reg = _arr(np.broadcast_to(np.asarray(reg, dtype=np.float64), (self.B,)))
        mu = _arr(np.broadcast_to(np.asarray(mu, dtype=np.float64), (self.B,))) if mu is not None else None
        ok = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.cddp_hip_stacks_backward(self.h, int(branch), C.byref(options), _ptr(reg), _ptr(mu), 1 if retry else 0,
                                                      ok.ctypes.data_as(C.POINTER(C.c_int32))))
        return ok

    def kernel_ms(self):
        return float(self.lib.cddp_hip_stacks_last_kernel_ms(self.h))

    def sweep_form(self):
        """0 = one lane per trajectory, 1 = lane-cooperative (the default for nx > 8)."""
        return int(self.lib.cddp_hip_stacks_last_sweep_form(self.h))

    def gains(self):
        B, N, nx, nu = self.B, self.N, self.nx, self.nu
        K = np.zeros((B, N, nu, nx)); k = np.zeros((B, N, nu)); Vx = np.zeros((B, N + 1, nx)); Vxx = np.zeros((B, N + 1, nx, nx)); dV = np.zeros((B, 2))
        self._check(self.lib.cddp_hip_stacks_get_gains(self.h, _ptr(K), _ptr(k), _ptr(Vx), _ptr(Vxx), _ptr(dV)))
        return K, k, Vx, Vxx, dV

    def constraint_gains(self):
        B, N, nx, m = self.B, self.N, self.nx, self.m
        ky = np.zeros((B, N, m)); Ky = np.zeros((B, N, m, nx)); ks = np.zeros((B, N, m)); Ks = np.zeros((B, N, m, nx)); dX = np.zeros((B, N + 1, nx))
        self._check(self.lib.cddp_hip_stacks_get_constraint_gains(self.h, _ptr(ky), _ptr(Ky), _ptr(ks), _ptr(Ks), _ptr(dX)))
        return ky, Ky, ks, Ks, dX

    def scalars(self):
        names = ("reg", "inf_du", "inf_pr", "inf_comp", "step_norm", "alpha_pr_max", "alpha_du_max")
        a = [np.zeros(self.B) for _ in names]
        self._check(self.lib.cddp_hip_stacks_get_scalars(self.h, *[_ptr(v) for v in a]))
        return dict(zip(names, a))


def hip_backward_stacks(fx, fu, lx, lu, lxx, luu, lux, VxN, VxxN, reg, reg_in_value, device=0):
    lib = load_hip()
    fx = _arr(fx); B, N, nx, _ = fx.shape; nu = _arr(fu).shape[3]
    args = [_arr(a) for a in (fx, fu, lx, lu, lxx, luu, lux, VxN, VxxN)]
    K = np.zeros((B, N, nu, nx)); k = np.zeros((B, N, nu)); Vx = np.zeros((B, N + 1, nx)); Vxx = np.zeros((B, N + 1, nx, nx))
    dV = np.zeros((B, 2)); ok = np.zeros(B, dtype=np.int32); ms = C.c_double(0.0)
    rc = lib.cddp_hip_backward_stacks(device, B, nx, nu, N, *[_ptr(a) for a in args], C.c_double(reg), int(reg_in_value),
                                      _ptr(K), _ptr(k), _ptr(Vx), _ptr(Vxx), _ptr(dV),
                                      ok.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms))
    if rc != 0:
        raise HipError("cddp_hip error %d: %s" % (rc, lib.cddp_hip_last_error().decode()))
    return K, k, Vx, Vxx, dV, ok, ms.value


# ---- RCCL communicator helpers of the C-ABI (include/cddp_hip.h, "multi-GPU") -------------------------------------
COMM_ID_BYTES = 128


def comm_unique_id():
    lib = load_hip()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib.cddp_hip_comm_unique_id(buf)
    if rc != 0:
        raise HipError("cddp_hip error %d: %s" % (rc, lib.cddp_hip_last_error().decode()))
    return buf.raw


def comm_init(unique_id, world, rank, device):
    lib = load_hip()
    comm = C.c_void_p()
    rc = lib.cddp_hip_comm_init(C.c_char_p(bytes(unique_id)), int(world), int(rank), int(device), C.byref(comm))
    if rc != 0:
        raise HipError("cddp_hip error %d: %s" % (rc, lib.cddp_hip_last_error().decode()))
    return comm.value


def comm_info(comm):
    """(ranks RCCL sees behind the communicator, this process's rank)"""
    lib = load_hip()
    n = C.c_int(); r = C.c_int()
    rc = lib.cddp_hip_comm_info(C.c_void_p(comm), C.byref(n), C.byref(r))
    if rc != 0:
        raise HipError("cddp_hip error %d: %s" % (rc, lib.cddp_hip_last_error().decode()))
    return n.value, r.value


def comm_destroy(comm):
    if comm:
        load_hip().cddp_hip_comm_destroy(C.c_void_p(comm))
