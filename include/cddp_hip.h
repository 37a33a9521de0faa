/*
 * cddp_hip.h -- C-ABI of the MI355X-native batched CLDDP / IPDDP solver core.
 *
 * This is the drop-in boundary for the hot path of astomodynamics/cddp-cpp:
 * everything cddp::ISolverAlgorithm::{initialize,solve} does for the "CLDDP"
 * and "IPDDP" solvers (reference include/cddp-cpp/cddp_core/cddp_core.hpp:186-210,
 * src/cddp_core/cddp_solver_base.cpp:29-186, clddp_solver.cpp, ipddp_solver.cpp,
 * boxqp.cpp), executed for a whole BATCH of independent trajectories on one GPU.
 *
 * Conventions (nothing like this exists in the reference):
 *   - extern "C", plain pointers and sizes, no exceptions / STL / Eigen / torch.
 *   - every entry point returns 0 on success, <0 on error;
 *     cddp_hip_last_error() returns a thread-local message.
 *   - all matrices are ROW-MAJOR doubles; trajectories handed over the boundary
 *     are batch-major: X[b][t][i], U[b][t][j], K[b][t][j][i].
 *   - host buffers are caller-owned, device buffers are library-owned (unless a
 *     *_device entry point says the pointer is a device pointer).
 *   - a handle is bound to (device, stream) and is NOT thread-safe; distinct
 *     handles are independent.
 *
 * The reference-side binding a maintainer adds is shown in INTEGRATION.md.
 */
#ifndef CDDP_HIP_H
#define CDDP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cddp_hip_options gained max_cpu_time (shifts cddp_hip_problem's tail), cddp_hip_stats gained rollout_steps (80 -> 88 bytes).
 * A host built against version 1 is refused by cddp_hip_create instead of being read at shifted offsets.
 * 3: cddp_hip_options gained the LogDDP barrier fields, cddp_hip_plugin gained constraint_hessians.
 * 4: cddp_hip_options gained the MSIPDDP multi-shooting fields. */
#define CDDP_HIP_ABI_VERSION 5
#define CDDP_HIP_MAX_MODEL_PARAMS 24
#define CDDP_HIP_NAME_LEN 48
#define CDDP_HIP_MAX_ALPHAS 32

/* ---- enumerations -------------------------------------------------------- */

/* Built-in plants with device-side dynamics + derivatives
 * (reference src/dynamics_model/{pendulum,cartpole,unicycle,lti_system,quadrotor,
 *  manipulator,bicycle,car,spacecraft_linear,euler_attitude,quaternion_attitude,mrp_attitude,
 *  spacecraft_twobody,spacecraft_landing2d,dubins_car,dreyfus_rocket,acrobot,usv_3dof,forklift,
 *  quadrotor_rate,spacecraft_linear_fuel,spacecraft_nonlinear}.cpp).  model_params layout is documented per entry. */
enum cddp_hip_model {
  CDDP_HIP_MODEL_PENDULUM = 0,   /* params: length, mass, damping, gravity                     */
  CDDP_HIP_MODEL_CARTPOLE = 1,   /* params: cart_mass, pole_mass, pole_length, gravity, damping */
  CDDP_HIP_MODEL_UNICYCLE = 2,   /* params: (none)                                              */
  CDDP_HIP_MODEL_LTI = 3,        /* discrete x+ = A x + B u; A,B via lti_A / lti_B              */
  CDDP_HIP_MODEL_QUADROTOR = 4,  /* nx=13 quaternion; params: mass, arm, Ixx,Iyy,Izz, gravity   */
  CDDP_HIP_MODEL_MANIPULATOR = 5,/* 3-DOF, central-FD Jacobians h=2e-5; params: (none)          */
  CDDP_HIP_MODEL_QUADROTOR_EULER12 = 6, /* SYNTHETIC nx=12 (BASELINE config 4 shape)            */
  CDDP_HIP_MODEL_MANIPULATOR7 = 7,      /* SYNTHETIC nx=14/nu=7 (BASELINE config 5 shape)       */
  CDDP_HIP_MODEL_BICYCLE = 8,    /* kinematic bicycle [x,y,theta,v] / [a,delta] (bicycle.cpp); params: wheelbase            */
  CDDP_HIP_MODEL_CAR = 9,        /* DISCRETE car [x,y,theta,v] / [delta,a] (car.cpp:24-60, h = dt); params: wheelbase      */
  CDDP_HIP_MODEL_HCW = 10,       /* Hill-Clohessy-Wiltshire relative motion [x,y,z,vx,vy,vz] / [Fx,Fy,Fz] (spacecraft_linear.cpp:24-120);
                                    params: mean_motion, mass                                                                  */
  /* rigid-body attitude plants, control [tau_x, tau_y, tau_z]; params [0..8]: the inertia matrix, row-major.  The library fills
     [9..17] with its inverse itself (cofactors times 1 / det, as Eigen's fixed-size inverse) and refuses a singular matrix. */
  CDDP_HIP_MODEL_EULER_ATTITUDE = 11,      /* nx=6 [psi,theta,phi,wx,wy,wz] ZYX angles (euler_attitude.cpp)                  */
  CDDP_HIP_MODEL_QUATERNION_ATTITUDE = 12, /* nx=7 [qw,qx,qy,qz,wx,wy,wz]; the step normalises q, the Jacobians do not
                                              (quaternion_attitude.cpp)                                                      */
  CDDP_HIP_MODEL_MRP_ATTITUDE = 13,        /* nx=6 [s1,s2,s3,wx,wy,wz] modified Rodrigues parameters (mrp_attitude.cpp)       */
  CDDP_HIP_MODEL_SPACECRAFT_TWOBODY = 14,  /* nx=6 [x,y,z,vx,vy,vz] / [ux,uy,uz] point mass about a central body
                                              (spacecraft_twobody.cpp); params: mu, mass.  Central-FD Jacobians; no full DDP
                                              (use_ilqr = 0 is refused: the reference's cross Hessian throws)               */
  CDDP_HIP_MODEL_SPACECRAFT_LANDING2D = 15,/* nx=6 [x,x_dot,y,y_dot,theta,theta_dot] / [thrust fraction, gimbal angle]
                                              (spacecraft_landing2d.cpp); params: mass, length, width, min_thrust,
                                              max_thrust, max_gimble (gravity 9.81, inertia mass * length^2 / 12)          */
  CDDP_HIP_MODEL_DUBINS_CAR = 16,          /* nx=3 [x,y,theta] / [omega], constant speed (dubins_car.cpp); params: speed       */
  CDDP_HIP_MODEL_DREYFUS_ROCKET = 17,      /* nx=2 [x,x_dot] / [theta] (dreyfus_rocket.cpp); params: thrust_acceleration,
                                              gravity_acceleration                                                            */
  CDDP_HIP_MODEL_ACROBOT = 18,             /* nx=4 [theta1,theta2,theta1_dot,theta2_dot] / [torque] (acrobot.cpp); params: l1, l2,
                                              m1, m2, J1, J2 (gravity 9.81 and friction 1.0 are fixed); autodiff derivatives      */
  CDDP_HIP_MODEL_USV_3DOF = 19,            /* nx=6 [x,y,psi,u,v,r] / [tau_u,tau_v,tau_r] surface vessel (usv_3dof.cpp); params:
                                              none from the caller.  The library fills [0..8] = M^-1, [9..17] = D_L (row-major),
                                              [18..20] = m_x, m_y, m_yr of the reference's fixed vessel                          */
  CDDP_HIP_MODEL_FORKLIFT = 20,            /* DISCRETE nx=5 [x,y,theta,v,delta] / [a, steering rate] (forklift.cpp, h = dt; the
                                              integrator is ignored); params: wheelbase, rear_steer (0 / 1), max_steering_angle
                                              (carried, unused by the dynamics); the library fills [3] = dt                     */
  CDDP_HIP_MODEL_QUADROTOR_RATE = 21,      /* nx=10 [px,py,pz,vx,vy,vz,qw,qx,qy,qz] / [thrust,wx,wy,wz] (quadrotor_rate.cpp); params: mass,
                                              max_thrust, max_rate (each must be positive; the last two are carried, unused by the
                                              dynamics); gravity 9.81; autodiff derivatives through the quaternion normalisation   */
  CDDP_HIP_MODEL_SPACECRAFT_LINEAR_FUEL = 22,/* nx=8 [x,y,z,vx,vy,vz,mass,accumulated control effort] / [Fx,Fy,Fz]
                                              (spacecraft_linear_fuel.cpp); params: mean_motion, isp, g0 (epsilon 1e-8 under the
                                              thrust norm is fixed).  Central-FD Jacobians; all Hessians are zero                */
  CDDP_HIP_MODEL_SPACECRAFT_NONLINEAR = 23 /* nx=10 [px,py,pz,vx,vy,vz,r0,theta,dr0,dtheta] / [ux,uy,uz] (spacecraft_nonlinear.cpp); params:
                                              mass, r_scale, v_scale (carried, unused by the dynamics), mu.  Central-FD Jacobians; no full
                                              DDP (use_ilqr = 0 is refused: the reference's cross Hessian throws)                  */
};

/* reference src/cddp_core/dynamical_system.cpp:28-83 */
enum cddp_hip_integrator {
  CDDP_HIP_EULER = 0, CDDP_HIP_HEUN = 1, CDDP_HIP_RK3 = 2, CDDP_HIP_RK4 = 3
};

/* Which reference solver core is replaced (cddp_core.cpp:213-233). */
enum cddp_hip_solver {
  CDDP_HIP_SOLVER_CLDDP = 0, CDDP_HIP_SOLVER_IPDDP = 1,
  CDDP_HIP_SOLVER_LOGDDP = 2,  /* logddp_solver.cpp:43-707 + barrier.hpp:37-296: single-shooting relaxed-log-barrier DDP.  Device-resident
                                  through cddp_hip_create / cddp_hip_solve for the built-in plants (round 4; register-resident up to nx = 8,
                                  csrc/kernels_logddp.hpp: every path constraint of the problem enters the barrier; options logddp_*,
                                  filter_*, regularisation and line-search fields; terminal constraints are ignored as the reference's
                                  LogDDP ignores them; result.barrier_mu = mu, result.inf_pr = the violation of the last resetFilter);
                                  scratch-backed above; full DDP only for plants with explicit Hessian tensors); user plug-ins:
                                  cddp_hip_plugin_solve (host loop + stack-fed GPU sweeps) */
  CDDP_HIP_SOLVER_MSIPDDP = 3  /* msipddp_solver.cpp:33-1930: multiple-shooting interior-point DDP (costates, dynamics defects at segment
                                  boundaries, three gap-closing rollout rules, multi-point filter).  Device-resident through cddp_hip_create /
                                  cddp_hip_solve for the built-in plants with nx <= 8 and no terminal set (round 4, csrc/kernels_msipddp.hpp;
                                  options msipddp_*, ipddp_slack / dual init scales, barrier_*, filter_*, regularisation and line-search
                                  fields; warm_start with a state guess in cddp_hip_set_initial is the multiple-shooting start: the guess
                                  is NOT rolled out; result.barrier_mu = mu; cddp_hip_get_duals returns its slacks / duals); user
                                  plug-ins, nx > 8 and terminal sets: cddp_hip_plugin_solve (host loop + stack-fed GPU sweeps).  Path
                                  constraints with nu > 1 and nx != nu are refused by both routes: the reference adds an (nx x nu) product
                                  to its (nu x nx) block Q_ux there (msipddp_solver.cpp:1398), which is only defined for nu = 1 (same
                                  linear layout) or nx = nu.  The unconstrained branch keeps the reference's per-step factor cache
                                  (msipddp_solver.cpp:1169-1185) for the lifetime of the handle */
};

/* Path-constraint kinds (reference include/cddp-cpp/cddp_core/constraint.hpp:144-404). */
enum cddp_hip_constraint_kind {
  CDDP_HIP_CON_CONTROL_BOX = 0, /* BoxConstraint<Control>: g=[-u;u]*s, upper=[-lb;ub]*s  */
  CDDP_HIP_CON_STATE_BOX = 1,   /* BoxConstraint<State>                                   */
  CDDP_HIP_CON_BALL = 2,        /* BallConstraint: g=-s*|x[:d]-c|^2, upper=-s*r^2         */
  CDDP_HIP_CON_LINEAR = 3,      /* LinearConstraint: g=A x, upper=b                       */
  CDDP_HIP_CON_SOC = 4,         /* SecondOrderConeConstraint (constraint.hpp:626-800): g = cos(fov) sqrt(|x[:3]-o|^2+eps) - (x[:3]-o).axis;
                                   center = origin o (3), lower = UNIT opening direction (3), radius = cos(fov), scale = eps, dim = 3 */
  CDDP_HIP_CON_THRUST = 5,      /* ThrustMagnitudeConstraint (:802-927): g = [min-|u|, |u|-max]; lower[0] = min, radius = max, scale = eps, dim = nu */
  CDDP_HIP_CON_MAX_THRUST = 6   /* MaxThrustMagnitudeConstraint (:929-1048): g = |u|-max; radius = max, scale = eps, dim = nu */
};

/* reference include/cddp-cpp/cddp_core/terminal_constraint.hpp:62-263 */
enum cddp_hip_terminal_kind { CDDP_HIP_TERM_EQUALITY = 0, CDDP_HIP_TERM_INEQUALITY = 1 };

/* status_message strings of the reference (cddp_solver_base.cpp:69,82,202,210;
 * clddp_solver.cpp:209,270,274; ipddp_solver.cpp:941,1968,1985,2070). */
enum cddp_hip_status {
  CDDP_HIP_STATUS_RUNNING = 0,
  CDDP_HIP_STATUS_OPTIMAL = 1,            /* "OptimalSolutionFound"                       */
  CDDP_HIP_STATUS_ACCEPTABLE = 2,         /* "AcceptableSolutionFound"                    */
  CDDP_HIP_STATUS_MAX_ITERATIONS = 3,     /* "MaxIterationsReached"                       */
  CDDP_HIP_STATUS_REG_LIMIT = 4,          /* "RegularizationLimitReached_NotConverged"    */
  CDDP_HIP_STATUS_MAX_CPU_TIME = 5,       /* "MaxCpuTimeReached"                          */
  CDDP_HIP_STATUS_REG_LIMIT_CONVERGED = 6 /* "RegularizationLimitReached_Converged" (LogDDP, logddp_solver.cpp:216-222) */
};

/* Line-search selection rule (cddp_solver_base.cpp:255-263 vs :264-314). */
enum cddp_hip_linesearch_rule {
  CDDP_HIP_LS_FIRST_SUCCESS = 0, /* enable_parallel=false: first successful alpha wins      */
  CDDP_HIP_LS_BEST_MERIT = 1     /* enable_parallel=true : lowest merit among successes     */
};

enum cddp_hip_barrier_strategy { CDDP_HIP_BARRIER_ADAPTIVE = 0, CDDP_HIP_BARRIER_MONOTONIC = 1,
                                 CDDP_HIP_BARRIER_IPOPT = 2 };

/* ---- option POD (field-for-field twin of cddp::CDDPOptions, options.hpp:41-251) */
typedef struct cddp_hip_options {
  double tolerance;              /* 1e-5 */
  double acceptable_tolerance;   /* 1e-6 */
  int32_t max_iterations;        /* 1    */
  int32_t use_ilqr;              /* 1; 0 = full DDP (second-order dynamics terms, ipddp_solver.cpp:1070-1082, 1160-1178,
                                  * 1396-1408): pendulum, cart-pole, unicycle, LTI; refused for the other plants        */
  int32_t enable_parallel;       /* 0 -> CDDP_HIP_LS_FIRST_SUCCESS, 1 -> BEST_MERIT        */
  int32_t return_iteration_info; /* 0 */
  int32_t warm_start;            /* 0 */
  int32_t _pad0;
  double termination_scaling_max_factor; /* 100 */
  /* LineSearchOptions */
  int32_t ls_max_iterations;     /* 11; a ladder of more than CDDP_HIP_MAX_ALPHAS step sizes is refused by cddp_hip_create and
                                  * cddp_hip_set_options (the reference walks all of it; cddp_hip_plugin_solve does too) */
  int32_t _pad1;
  double ls_initial_step_size;   /* 1.0 */
  double ls_min_step_size;       /* 1e-8 */
  double ls_step_reduction_factor; /* 0.5 */
  /* RegularizationOptions */
  double reg_initial_value;      /* 1e-6 */
  double reg_update_factor;      /* 10 */
  double reg_max_value;          /* 1e7 */
  double reg_min_value;          /* 1e-10 */
  /* BoxQPOptions (boxqp.hpp:30-41) */
  int32_t boxqp_max_iterations;  /* 100 */
  int32_t _pad2;
  double boxqp_min_gradient_norm;        /* 1e-8 */
  double boxqp_min_relative_improvement; /* 1e-8 */
  double boxqp_step_decrease_factor;     /* 0.6 */
  double boxqp_min_step_size;            /* 1e-22 */
  double boxqp_armijo_constant;          /* 0.1 */
  /* SolverSpecificFilterOptions */
  double filter_merit_acceptance_threshold;     /* 1e-6 */
  double filter_violation_acceptance_threshold; /* 1e-6 */
  double filter_max_violation_threshold;        /* 1e4 */
  double filter_min_violation_for_armijo_check; /* 1e-7 */
  double filter_armijo_constant;                /* 1e-4 */
  /* IPDDPAlgorithmOptions */
  double ipddp_dual_var_init_scale;   /* 0.1 */
  double ipddp_slack_var_init_scale;  /* 1e-2 */
  double ipddp_barrier_tol_mult;      /* 0.1 */
  double ipddp_barrier_update_dual_weight; /* 0.01 */
  double ipddp_mu_kappa_epsilon;      /* 10 */
  int32_t ipddp_check_state_stationarity; /* 0 */
  int32_t ipddp_theta_norm_l2;        /* 0 = "l1" */
  int32_t ipddp_max_filter_size;      /* 5; IPDDP handles take at most 7: the filter holds max_filter_size + 1 points between an accept
                                       * and the prune, in eight slots.  Larger values are refused, not truncated (MSIPDDP does not read it) */
  int32_t ipddp_warmstart_repair;     /* 0 */
  double ipddp_theta_0_floor;         /* 1.0 */
  double ipddp_warmstart_s_min;       /* 1e-4 */
  double ipddp_warmstart_y_min;       /* 1e-4 */
  double ipddp_warmstart_interior_factor; /* 1.1 */
  double ipddp_jacobian_regularization_value;    /* 1e-8 */
  double ipddp_jacobian_regularization_exponent; /* 0.25 */
  /* SolverSpecificBarrierOptions */
  double barrier_mu_initial;          /* 1.0 */
  double barrier_mu_min_value;        /* 1e-10 */
  double barrier_mu_update_factor;    /* 0.5 */
  double barrier_mu_update_power;     /* 1.2 */
  double barrier_min_fraction_to_boundary; /* 0.99 */
  int32_t barrier_strategy;           /* CDDP_HIP_BARRIER_ADAPTIVE */
  int32_t _pad3;
  /* CDDPOptions::max_cpu_time [s], 0 = unlimited (options.hpp:212; checked at the top of every iteration,
   * cddp_solver_base.cpp:77-90).  One clock for the batch: when it expires, every trajectory still running
   * terminates with "MaxCpuTimeReached" and iterations = the iteration the check fired in. */
  double max_cpu_time;                /* 0 */
  /* LogBarrierOptions (options.hpp:135-143; LogDDP only): log_barrier.barrier.{mu_initial, mu_min_value, mu_update_factor} and
   * log_barrier.relaxed_log_barrier_delta */
  double logddp_mu_initial;           /* 1.0 */
  double logddp_mu_min_value;         /* 1e-10 */
  double logddp_mu_update_factor;     /* 0.5 */
  double logddp_relaxed_delta;        /* 1e-10 */
  /* MultiShootingOptions (options.hpp:120-130; MSIPDDP only).  With solver = MSIPDDP the InteriorPointOptions half of options.msipddp
   * (dual_var_init_scale, slack_var_init_scale, barrier.*) travels in ipddp_dual_var_init_scale / ipddp_slack_var_init_scale /
   * barrier_* above -- the mirrors copy options.msipddp there instead of options.ipddp. */
  double msipddp_costate_var_init_scale;  /* 1e-6 */
  int32_t msipddp_segment_length;         /* 5 */
  int32_t msipddp_rollout_type;           /* 0 = "nonlinear", 2 = "hybrid", 1 = any other string (plain rollout at the boundary) */
  int32_t msipddp_use_controlled_rollout; /* 0 */
  int32_t _pad4;
} cddp_hip_options;

/* Fill *opt with the reference defaults (options.hpp in-class initialisers). */
void cddp_hip_default_options(cddp_hip_options *opt);

/* ---- constraint descriptors --------------------------------------------- */

/* One entry of CDDP::path_constraint_set_ (std::map<std::string, unique_ptr<Constraint>>,
 * cddp_core.hpp:422).  The library sorts entries by `name` (lexicographic, as std::map
 * iterates) to reproduce the reference's dual stacking order (ipddp_solver.cpp:1371-1384).
 * CLDDP only honours a CONTROL_BOX whose name is exactly "ControlConstraint"
 * (clddp_solver.cpp:85-86). */
typedef struct cddp_hip_constraint {
  char name[CDDP_HIP_NAME_LEN];
  int32_t kind;        /* cddp_hip_constraint_kind */
  int32_t dim;         /* box: #variables (dual dim = 2*dim); ball: center size; linear: #rows */
  const double *lower; /* box: dim */
  const double *upper; /* box: dim */
  const double *center;/* ball: dim */
  const double *A;     /* linear: dim x nx row-major */
  const double *b;     /* linear: dim */
  double radius;       /* ball */
  double scale;        /* scale_factor (box, ball); 1.0 default */
} cddp_hip_constraint;

/* One entry of CDDP::terminal_constraint_set_. */
typedef struct cddp_hip_terminal_constraint {
  char name[CDDP_HIP_NAME_LEN];
  int32_t kind;         /* cddp_hip_terminal_kind */
  int32_t dim;          /* equality: nx; inequality: #rows of A_N */
  const double *target; /* equality: nx   (h = x_N - target)   */
  const double *A;      /* inequality: dim x nx (g = A x_N - b) */
  const double *b;      /* inequality: dim */
} cddp_hip_terminal_constraint;

/* ---- problem descriptor -------------------------------------------------- */

/* Everything cddp::CDDP holds for one problem (cddp_core.hpp:215-423), as a POD.
 * All trajectories of a batch share this descriptor; they differ in x0 / U0 only. */
typedef struct cddp_hip_problem {
  int32_t abi_version;  /* CDDP_HIP_ABI_VERSION */
  int32_t solver;       /* cddp_hip_solver */
  int32_t model;        /* cddp_hip_model */
  int32_t integrator;   /* cddp_hip_integrator */
  int32_t nx, nu, horizon;
  int32_t _pad0;
  double dt;
  double model_params[CDDP_HIP_MAX_MODEL_PARAMS];
  const double *lti_A;  /* CDDP_HIP_MODEL_LTI: nx*nx (discrete A) */
  const double *lti_B;  /* CDDP_HIP_MODEL_LTI: nx*nu (discrete B) */
  /* QuadraticObjective(Q, R, Qf, x_ref, reference_states, dt) -- objective.cpp:30-65.
   * Q and R are given UNSCALED; the library multiplies them by dt as the ctor does. */
  const double *Q;      /* nx*nx */
  const double *R;      /* nu*nu */
  const double *Qf;     /* nx*nx */
  const double *x_ref;  /* nx    */
  const double *x_ref_traj; /* (horizon+1)*nx per-step references or NULL (objective.cpp:83-88) */
  int32_t n_constraints;
  int32_t n_terminal;
  const cddp_hip_constraint *constraints;
  const cddp_hip_terminal_constraint *terminal;
  cddp_hip_options options;
} cddp_hip_problem;

/* ---- per-trajectory result record --------------------------------------- */

/* Twin of cddp::CDDPSolution scalars (cddp_core.hpp:54-76) plus work counters used
 * for the roofline accounting. 96 bytes. */
typedef struct cddp_hip_result {
  double final_objective;
  double merit_function;
  double inf_pr, inf_du, inf_comp;
  double barrier_mu;
  double regularization;
  double alpha_pr, alpha_du;
  double step_norm;
  int32_t iterations;
  int32_t status;          /* cddp_hip_status */
  int32_t n_backward;      /* backward sweeps executed (incl. regularisation retries) */
  int32_t n_forward;       /* forward rollouts required by the sequential rule        */
} cddp_hip_result;

/* The 16-byte record that is all-gathered across GPUs. */
typedef struct cddp_hip_gather_record {
  double final_objective;
  int32_t iterations;
  int32_t status;
} cddp_hip_gather_record;

/* Result of one line-search trial (twin of ForwardPassResult scalars, cddp_core.hpp:105-145). */
typedef struct cddp_hip_trial {
  double alpha, alpha_pr, alpha_du;
  double cost, merit_function, theta, inf_pr, inf_comp;
  int32_t success;
  int32_t _pad;
} cddp_hip_trial;

/* Timing / work summary of one cddp_hip_solve call. */
typedef struct cddp_hip_stats {
  double solve_ms;          /* hipEvent time of the device-resident loop           */
  double backward_ms;       /* sum of K1+K2 kernel time (hipEvent); 0 unless the timing detail covers it */
  double forward_ms;        /* sum of K4 (rollout) kernel time; 0 unless covered   */
  double update_ms;         /* sum of K4b (costate) + K5 kernel time; 0 unless covered */
  int64_t sweeps;           /* sum over trajectories of n_backward                 */
  int64_t rollouts;         /* sum over trajectories of n_forward                  */
  int64_t rollouts_launched;/* rollouts actually executed (speculative alphas too) */
  int64_t traj_iterations;  /* sum over trajectories of iterations                 */
  int32_t outer_iterations; /* host loop trips                                     */
  int32_t n_converged;      /* status OPTIMAL or ACCEPTABLE                        */
  int32_t kernel_launches;
  int32_t timing_detail;    /* CDDP_HIP_TIMING_* the class times were taken with   */
  int64_t rollout_steps;    /* time steps the credited rollouts (`rollouts`) actually traversed: a trial the
                             * reference abandons at its first fraction-to-boundary violation
                             * (ipddp_solver.cpp:1632-1645) counts the steps completed before it, not N */
} cddp_hip_stats;

/* Which kernel classes cddp_hip_solve brackets with hipEvents when a stats block is requested.  An event costs
 * about 5 us of queue time, i.e. bracketing every class of every iteration adds ~5 % to a C2 solve; the default
 * brackets the rollout launches only (2 events per iteration). */
enum {
  CDDP_HIP_TIMING_ROLLOUT = 0,   /* forward_ms only                       */
  CDDP_HIP_TIMING_ALL = 1,       /* backward_ms, forward_ms, update_ms    */
  CDDP_HIP_TIMING_SWEEP = 2      /* backward_ms only                      */
};

typedef struct cddp_hip_handle cddp_hip_handle;

/* ---- entry points -------------------------------------------------------- */

int cddp_hip_abi_version(void);
/* 0: the reference's plants evaluate sin / cos with the device libm (lib/libcddp_hip.so, the product build); 1: with the
 * branch-free routine of csrc/dev_trig.hpp (lib/libcddp_hip_sharedtrig.so, the parity build a host selects with
 * CDDP_HIP_TRIG=shared): same C-ABI, same kernels; a CPU checker can run that routine too, which makes plants whose accept /
 * reject decisions hinge on the last bit of a sine bit-comparable (tests/test_shared_trig_parity.py). */
int cddp_hip_trig_shared(void);
const char *cddp_hip_last_error(void);
/* Number of visible HIP devices (0 when the runtime finds none). */
int cddp_hip_device_count(void);
const char *cddp_hip_status_string(int status);

/* Build line-search ladder exactly as detail::buildLineSearchAlphas
 * (cddp_context_utils.cpp:37-57). Returns the number of alphas written (<= cap); with alphas == NULL
 * the ladder's own length, which may exceed CDDP_HIP_MAX_ALPHAS.  This is the ladder of CLDDP, IPDDP and
 * MSIPDDP; LogDDP walks ls_max_iterations plain geometric steps (logddp_solver.cpp:177-182). */
int cddp_hip_build_alphas(const cddp_hip_options *opt, double *alphas, int cap);

/* Create a solver instance for `batch` independent trajectories of `problem` on `device`.
 * Replaces CDDP::createSolver + ISolverAlgorithm construction (cddp_core.cpp:213-241).
 * Fails (returns <0) when no GPU/HIP runtime is available -- there is no CPU fallback. */
int cddp_hip_create(const cddp_hip_problem *problem, int batch, int device,
                    cddp_hip_handle **out);
int cddp_hip_destroy(cddp_hip_handle *h);

/* Run all subsequent work of this handle on an existing hipStream_t (e.g. torch's). */
int cddp_hip_set_stream(cddp_hip_handle *h, void *hip_stream);

/* Select the class-timing detail (CDDP_HIP_TIMING_*) of later cddp_hip_solve calls that pass a stats block. */
int cddp_hip_set_timing_detail(cddp_hip_handle *h, int detail);

/* CDDP::setInitialState / setInitialTrajectory for the whole batch (cddp_core.cpp:66-140).
 * x0: batch*nx. U0: batch*N*nu or NULL (zeros). X0: batch*(N+1)*nx or NULL (x0 replicated,
 * as cddp::example::makeInitialTrajectory does). CLDDP linearises X0 as given
 * (clddp_solver.cpp:68-74); IPDDP re-rolls X from U (ipddp_solver.cpp:868-874). */
int cddp_hip_set_initial(cddp_hip_handle *h, const double *x0, const double *U0,
                         const double *X0);

/* ISolverAlgorithm::initialize for the batch (clddp_solver.cpp:28-75, ipddp_solver.cpp:644-914).
 * The handle is the solver object: with options.warm_start the first call takes the reference's "warm start
 * with provided trajectory" branch (ipddp_solver.cpp:733-816; CLDDP falls back to its cold start), every later
 * call the "existing solver state" branch (ipddp_solver.cpp:675-731, clddp_solver.cpp:51-60): gains, slack /
 * dual / costate / terminal variables, regularisation and step lengths persist on the device, X is re-rolled
 * out from the current (or newly supplied) controls.  Without warm_start every call is a cold start from the
 * trajectory of the last cddp_hip_set_initial. */
int cddp_hip_initialize(cddp_hip_handle *h);

/* CDDP::setOptions on a live handle (e.g. to switch warm_start on between two solves).  The line-search
 * ladder size is fixed at create time. */
int cddp_hip_set_options(cddp_hip_handle *h, const cddp_hip_options *options);

/* CDDP::setInitialState for the batch: x0[b][i] only; controls, duals and gains on the device are kept
 * (the MPC restart of SURVEY.md 8(f1)).  cddp_hip_set_initial additionally replaces the trajectory
 * (CDDP::setInitialTrajectory). */
int cddp_hip_set_initial_state(cddp_hip_handle *h, const double *x0);

/* Forget the solver state of the handle -- gains, slack / dual / costate / terminal variables, regularisation -- as if the reference's
 * solver OBJECT were constructed anew, without re-allocating anything: with options.warm_start the next initialize / solve then takes the
 * reference's "warm start with provided trajectory" branch (ipddp_solver.cpp:733-816, clddp_solver.cpp:35-60: the trajectory of the last
 * cddp_hip_set_initial, barrier parameter from its largest violation, duals re-initialised) instead of "existing solver state"
 * (:653-731).  The MPC caller that builds a fresh problem per step (examples/ipddp_mpcc_rc.py:649-705, test_ipddp_solver.cpp's warm-start
 * tests) is cddp_hip_forget_solver_state + cddp_hip_set_initial(x0, shifted U, shifted X) + cddp_hip_solve on one long-lived handle. */
int cddp_hip_forget_solver_state(cddp_hip_handle *h);

/* Overwrite the path slack / dual variables S[b][t][m], Y[b][t][m] (either may be NULL) and the terminal
 * slack / dual / multipliers S_T[b][mT], Y_T[b][mT], Lambda_T[b][pT] of an initialised handle: the
 * reference's IPDDPSolverTestAccess::setPathInterior / setTerminalInterior / setTerminalEqualityMultiplier,
 * and the hook for callers that shift duals between MPC solves. */
int cddp_hip_set_duals(cddp_hip_handle *h, const double *S, const double *Y);
int cddp_hip_set_terminal(cddp_hip_handle *h, const double *S_T, const double *Y_T, const double *Lambda_T);
/* Overwrite the per-trajectory barrier parameter mu_[b] (IPDDP; mu_ of ipddp_solver.hpp) and / or the
 * regularisation context.regularization_[b] of an initialised handle (either may be NULL): with
 * cddp_hip_set_initial + cddp_hip_set_duals this installs an arbitrary iterate (X, U, S, Y, mu, reg), e.g. a late
 * iterate of another solve, for one cddp_hip_backward / cddp_hip_forward -- the role of the reference's
 * IPDDPSolverTestAccess (tests/cddp_core/test_ipddp_solver.cpp:30-135). */
int cddp_hip_set_barrier_state(cddp_hip_handle *h, const double *mu, const double *reg);

/* One backwardPass for every trajectory (clddp_solver.cpp:79-204 / ipddp_solver.cpp:960-1569),
 * including the "retry with larger regularisation" loop of cddp_solver_base.cpp:93-111.
 * ok[b] (optional, batch ints) receives 1 when the sweep succeeded. */
int cddp_hip_backward(cddp_hip_handle *h, int32_t *ok);

/* forwardPass for every trajectory and every given alpha
 * (clddp_solver.cpp:215-262 / ipddp_solver.cpp:1571-1876).  trials: batch*n_alphas records,
 * trials[b*n_alphas + a]. Does not commit anything. */
int cddp_hip_forward(cddp_hip_handle *h, const double *alphas, int n_alphas,
                     cddp_hip_trial *trials);

/* ISolverAlgorithm::solve for the batch: cddp_solver_base.cpp:29-186 as a per-trajectory
 * device state machine.  Calls cddp_hip_initialize first.  stats may be NULL. */
int cddp_hip_solve(cddp_hip_handle *h, cddp_hip_stats *stats);
/* How the last cddp_hip_solve scheduled the IPDDP costate trial (before the first solve: how the next one would): 1 = deferred into the
 * next sweep launch ("shadow": path-constrained IPDDP on the role-split sweep, no terminal set, Gauss-Newton, first-success rule, a
 * restartable solve), 0 = on the iteration's chain.  CDDP_HIP_COSTATE=sync | shadow (read at create) overrides the default.  Results
 * are bitwise the same either way. */
int cddp_hip_costate_mode(cddp_hip_handle *h);
/* Deferred solves of this handle that met a non-finite costate row, were discarded and run again on the chain (0 on healthy problems). */
int cddp_hip_costate_redos(cddp_hip_handle *h);
/* Two-stage line-search iterations of the last cddp_hip_solve that ran both stages in ONE rollout launch (deferred costate, first-success
 * rule, two-role rollout; CDDP_HIP_LS_INKERNEL=0 turns the form off): counts[0] = second-stage (tile, step size) workgroups that ran a
 * trial, counts[1] = those that returned at once because the first stage had served every lane of their tile, counts[2] = those that
 * gave up waiting for the first stage's masks and ran the trial for every lane in phase (correct, and 0 unless the device dispatched a
 * second stage without its first).  All 0 when no launch took the form.  Summed over the handle's tile groups. */
int cddp_hip_ls_stage_counts(cddp_hip_handle *h, long long *counts);

/* ---- device-resident MPC step --------------------------------------------
 * Between two solves of a receding-horizon loop the plan does not leave the device: cddp_hip_mpc_advance makes the seed of the next
 * solve from every trajectory's CURRENT iterate where it lies (a row permutation of the wave-tiled stacks), with no host copy of a
 * trajectory and no host transposition.  Each mode is, bit for bit, the host sequence named next to it -- the next cddp_hip_solve's
 * results, trajectory, duals and work counters; in between, cddp_hip_get_trajectory returns the shifted plan (the seed the host sequence
 * uploads) and, with CDDP_HIP_MPC_SHIFT_DUALS, cddp_hip_get_duals the shifted rows.  An advance is meant to be FOLLOWED BY A SOLVE: the
 * shift is made in place in every trajectory's live slot, so a second advance without a solve in between shifts the plan a second
 * time, where the host sequence run twice (it reads the live slot, which only the solve rewrites) would seed the same plan twice.
 * With x_next NULL, or a device x_next on a stream given by cddp_hip_set_stream, the call returns once its kernels are enqueued on the
 * handle's stream; the next solve and the getters are ordered behind them as behind every other setter.
 * "Shifted", per trajectory: X_shifted[t] = X[t+1] (t < N), X_shifted[N] = X[N]; U_shifted[t] = U[t+1] (t < N-1), U_shifted[N-1] = U[N-1];
 * S and Y like U.  x_next: NULL = X[1] of the current plan (the plant is the model); otherwise the measured state, batch*nx, which
 * replaces row 0 as cddp_hip_set_initial writes X_[0] = initial_state -- a host pointer (the step's only upload, batch*nx doubles) or,
 * with CDDP_HIP_MPC_X_DEVICE, a device pointer read on the handle's stream.
 * Refused, with nothing launched and nothing changed: a handle without a current plan (no cddp_hip_set_initial, or never initialised /
 * solved), an unknown mode or flag, CDDP_HIP_MPC_SHIFT_DUALS outside CDDP_HIP_MPC_SHIFT_EXISTING or on a problem without path duals.
 * Not shifted: gains, costates, the MSIPDDP factor cache, filter entries.  (Added after cddp_hip_get_costates; ABI version unchanged.) */
enum cddp_hip_mpc_mode {
  CDDP_HIP_MPC_KEEP_PLAN = 0,      /* == cddp_hip_set_initial_state(x_next): plan, duals, gains untouched                    */
  CDDP_HIP_MPC_SHIFT_EXISTING = 1, /* == cddp_hip_set_initial(x_next, U_shifted, X_shifted): solver state kept               */
  CDDP_HIP_MPC_SHIFT_PROVIDED = 2  /* == cddp_hip_forget_solver_state + cddp_hip_set_initial(x_next, U_shifted, X_shifted)   */
};
enum { CDDP_HIP_MPC_SHIFT_DUALS = 1,   /* SHIFT_EXISTING, IPDDP with path rows: also == cddp_hip_set_duals(S_shifted, Y_shifted) */
       CDDP_HIP_MPC_X_DEVICE   = 2 };  /* x_next is a DEVICE pointer (batch-major, batch*nx), read on the handle's stream   */
int cddp_hip_mpc_advance(cddp_hip_handle *h, int mode, int flags, const double *x_next /* batch*nx or NULL */);
/* The closed loop with the model as the plant: `steps` times { cddp_hip_solve; record u_0, x_1, iterations, status of every trajectory;
 * cddp_hip_mpc_advance(mode, flags, NULL) }.  The records accumulate in a device log and come back in one copy per output at the end
 * (any output may be NULL): U_applied[b][k][nu], X_visited[b][k][nx] with X_visited[b][0] the initial state of the first solve and
 * X_visited[b][k+1] the x_1 of solve k, iterations[b][k], status[b][k].  stats_sum (optional) adds up the per-solve counters and times.
 * Bitwise the hand-written loop over cddp_hip_solve, cddp_hip_get_plan_head and cddp_hip_mpc_advance.  An error from a solve ends the
 * run and is returned; the steps completed so far stay in the outputs. */
int cddp_hip_mpc_run(cddp_hip_handle *h, int steps, int mode, int flags,
                     double *U_applied /* B*steps*nu */, double *X_visited /* B*(steps+1)*nx */,
                     int32_t *iterations /* B*steps */, int32_t *status /* B*steps */, cddp_hip_stats *stats_sum);

/* ---- closed loop against a separate plant --------------------------------
 * A cddp_hip_plant is a device-resident plant for a batch of trajectories: one of the built-in models with its OWN parameters (shared by
 * the batch or one block per trajectory), integrator, integration step (dt / substeps under a zero-order hold of u), actuator
 * saturation and an additive disturbance.  It closes the MPC loop on the device (cddp_hip_mpc_run_plant), rolls a solved plan's
 * feedback policy out on the true plant (cddp_hip_track_plan) and can be driven directly (cddp_hip_plant_step).
 * (New entry points; ABI version unchanged; the descriptor carries its own abi_version, checked as cddp_hip_plugin's is.)
 *
 * Arithmetic (the library is built without FMA contraction; the tests of these entries are bitwise):
 *  - parameters: trajectory b reads its own DERIVED block -- what cddp_hip_create derives from cddp_hip_problem::model_params (inverse
 *    inertia, the USV matrices, ...) applied to its CDDP_HIP_MAX_MODEL_PARAMS caller entries when the plant is created; for the car and
 *    the forklift the timestep slot is the plant's dt; LTI: lti_A | lti_B | dt;
 *  - h = dt / substeps is divided once on the host, in double;
 *  - one step: u_s[i] = fmin(fmax(u[i], u_lower[i]), u_upper[i]) (only with a box); `substeps` times x <- step(integrator, h, params_b,
 *    x, u_s), the explicit integrators of the solver's own rollout; x_next[i] = x[i] + w[i] (only with w). */
typedef struct cddp_hip_plant_desc {
  int32_t abi_version;           /* CDDP_HIP_ABI_VERSION */
  int32_t model, integrator;     /* cddp_hip_model, cddp_hip_integrator */
  int32_t substeps;              /* >= 1: the plant takes `substeps` steps of dt / substeps under a zero-order hold of u */
  int32_t nx, nu;
  int32_t params_per_trajectory; /* 0: model_params is CDDP_HIP_MAX_MODEL_PARAMS doubles; 1: batch * CDDP_HIP_MAX_MODEL_PARAMS, batch-major */
  int32_t _pad;
  double dt;                     /* control interval */
  const double *model_params;    /* caller's parameters, laid out as cddp_hip_problem::model_params; derived entries are the library's */
  const double *lti_A, *lti_B;   /* CDDP_HIP_MODEL_LTI only, shared by the batch */
  const double *u_lower, *u_upper; /* nu each, or both NULL: the plant receives min(max(u, lower), upper) */
} cddp_hip_plant_desc;
typedef struct cddp_hip_plant cddp_hip_plant;
enum { CDDP_HIP_PLANT_DEVICE = 1 };   /* x, u, w, x_next are device pointers, batch-major as below */

/* The descriptor is checked BEFORE the device is looked at, each refusal with its own message: wrong abi_version; unknown model or
 * integrator; nx / nu not the model's; substeps < 1; substeps > 1 on a discrete plant (car, forklift, LTI: their step is h = dt by
 * definition); dt <= 0; one of u_lower / u_upper NULL or lower > upper in a slot; LTI without lti_A / lti_B or with
 * params_per_trajectory; a parameter block the model refuses (with per-trajectory parameters the message names the trajectory).  Only
 * then: -20, no HIP device.  The arrays of the descriptor are copied; they need not outlive the call. */
int cddp_hip_plant_create(const cddp_hip_plant_desc *desc, int batch, int device, cddp_hip_plant **out);
int cddp_hip_plant_destroy(cddp_hip_plant *p);
/* One control interval of every trajectory: x_next = plant(x, u) + w.  flags = 0: host pointers (uploaded, computed, downloaded);
 * CDDP_HIP_PLANT_DEVICE: device pointers of the plant's device, whose contents must be complete when the call is made.  Either way the
 * call returns after x_next has been written.  x_next may be x. */
int cddp_hip_plant_step(cddp_hip_plant *p, int flags, const double *x /* B*nx */, const double *u /* B*nu */,
                        const double *w /* B*nx or NULL */, double *x_next /* B*nx */);
/* cddp_hip_mpc_run with the plant in the loop: `steps` times { cddp_hip_solve; record iterations and status; x_next = plant(row 0 of every
 * trajectory's live slot, u_0 of the plan, W[:, k]); record the SATURATED u_0 and x_next; the equivalent of cddp_hip_mpc_advance(mode,
 * flags | CDDP_HIP_MPC_X_DEVICE, x_next) }.  Outputs, the behaviour on an error (the steps completed so far come back) and stats_sum as
 * cddp_hip_mpc_run.  W (host, B*steps*nx, W[b][k][nx]) is uploaded once before the first solve; nothing but the final logs crosses the
 * bus afterwards.  Bitwise the hand-written loop over cddp_hip_solve, cddp_hip_plant_step on row 0 of cddp_hip_get_trajectory and
 * cddp_hip_mpc_advance.  A handle of several tile groups runs the plant per group, on the group's stream.
 * Refused, with nothing launched and nothing changed: a NULL handle or plant; nx, nu or batch differing between plant and handle; a
 * plant on another device; everything cddp_hip_mpc_run refuses. */
int cddp_hip_mpc_run_plant(cddp_hip_handle *h, cddp_hip_plant *plant, int steps, int mode, int flags,
                           const double *W /* B*steps*nx or NULL, host */,
                           double *U_applied, double *X_visited, int32_t *iterations, int32_t *status, cddp_hip_stats *stats_sum);
/* The solved plan's feedback policy on the plant, over the horizon.  X, U: the live slot of the handle's current plan; K: the stack
 * cddp_hip_get_gains reads.  Per step t: dx[j] = x_t[j] - X_t[j]; s = 0, for j ascending s += K_t[i][j] * dx[j]; u[i] = U_t[i] + s;
 * then the plant step as above with W[b][t].  U_out holds the saturated controls; X_out[:, 0] is x0, or row 0 of the plan.  Host
 * pointers.  The handle's state is not modified.  Refused as cddp_hip_mpc_run_plant refuses a mismatched plant, and on a handle that was
 * never initialised or solved. */
int cddp_hip_track_plan(cddp_hip_handle *h, cddp_hip_plant *plant, const double *x0 /* B*nx or NULL = row 0 of the plan */,
                        const double *W /* B*N*nx or NULL */, double *X_out /* B*(N+1)*nx */, double *U_out /* B*N*nu */);

/* ---- moving the goal and the per-step reference of a live handle ------------
 * The objective's goal x_ref and per-step reference x_ref_traj (shared by the batch) can be replaced on a live handle, so a receding-
 * horizon caller follows a moving set-point or a path without re-creating the handle: the device-resident plan, the solver state and
 * captured iteration windows stay.  (New entry points; ABI version unchanged; the path descriptor carries its own abi_version.)
 *
 * cddp_hip_set_reference replaces the goal (x_ref, nx doubles, NULL = keep) and / or the per-step reference (x_ref_traj, (N+1)*nx doubles,
 * NULL = keep) in every tile group.  A handle created without a per-step reference gets its buffer on first use and keeps it;
 * CDDP_HIP_REF_CLEAR_TRAJ puts the running cost back on x_ref.  Semantics:
 *  - the change takes effect from the next cddp_hip_initialize / cddp_hip_solve, which then equals, bit for bit, the same call on a handle
 *    created with the new reference and brought to the same state; the scalars of the current iterate (cost, merit) stay those evaluated
 *    under the old reference until then;
 *  - entries that evaluate the objective on the spot use the new reference at once: cddp_hip_score_rollouts, cddp_hip_mppi_refine,
 *    cddp_hip_plan_montecarlo, cddp_hip_forward;
 *  - terminal-constraint targets are separate data and are not touched;
 *  - ordering: as every other setter, on the handle's stream.  Host pointers: the call returns after the upload.  CDDP_HIP_REF_DEVICE:
 *    device pointers, checked and ordered as cddp_hip_set_initial_device's -- on a stream given by cddp_hip_set_stream the call does not block;
 *  - the reference's constructor rule (objective.cpp:55-63), || x_ref_traj[N] - x_ref ||_2 <= 1e-6, is enforced on the state the call would
 *    leave behind when the pointers are host pointers.  With CDDP_HIP_REF_DEVICE the contents are not read by the host: the rule, and finite
 *    values, are the caller's responsibility.
 * Refused, each with its own message, nothing launched and nothing changed: a NULL handle; an unknown flag; CDDP_HIP_REF_CLEAR_TRAJ together
 * with an x_ref_traj; a call that changes nothing (no x_ref, no x_ref_traj, no CDDP_HIP_REF_CLEAR_TRAJ); a device pointer that is not memory
 * of the handle's device or too short; a non-finite host value; the last-row rule; a handle with a reference path bound (unbind first).
 *
 * cddp_hip_get_reference reads back from the device exactly what the kernels will read: x_ref (nx), x_ref_traj ((N+1)*nx, left untouched
 * when the handle has no per-step reference) and *has_traj (1 / 0).  Any output may be NULL.  Host pointers.
 *
 * cddp_hip_mpc_set_reference_path binds a path of L rows to the handle: the rows are copied into device memory the handle owns, the window
 * of cursor `start` is installed at once, and from then on EVERY cddp_hip_mpc_advance (all three modes; cddp_hip_mpc_run and
 * cddp_hip_mpc_run_plant go through it) moves the cursor by one and installs the next window before it returns -- one small kernel per tile
 * group on the group's stream, no upload.  Window of cursor k, rows t = 0 .. N (the library is built without FMA contraction):
 *     pos = (double)(k + t) * rows_per_step;  i = floor(pos);  a = pos - i;
 *     row t = path[L-1]                                  when i >= L-1  (past the end of the path the window holds the last row),
 *     row t[e] = p_i[e] + a * (p_{i+1}[e] - p_i[e])        otherwise      (with a == 0 this is p_i[e]);
 *     the goal x_ref becomes row N of the window (the last-row rule holds exactly).
 * Every element is blended alike: wrapping angles is the caller's business.  desc == NULL unbinds: the reference is left as it stands and
 * cddp_hip_set_reference is accepted again.  Binding again replaces the path and the cursor.  With host rows the call returns after the
 * upload and refuses non-finite values; with CDDP_HIP_REF_DEVICE the rows are checked as a device pointer and copied on the handle's stream.
 * Refused: a NULL handle; a wrong abi_version; an unknown flag; rows < 1; start < 0; rows_per_step not finite or <= 0; a NULL path.
 * cddp_hip_mpc_reference_cursor: the cursor of the window now installed (start + the advances since), -1 when no path is bound. */
enum { CDDP_HIP_REF_DEVICE = 1,      /* pointers are device pointers, checked and ordered as cddp_hip_set_initial_device's */
       CDDP_HIP_REF_CLEAR_TRAJ = 2 };/* drop the per-step reference: running cost back on x_ref (x_ref_traj must be NULL) */
int cddp_hip_set_reference(cddp_hip_handle *h, int flags, const double *x_ref /* nx or NULL = keep */,
                           const double *x_ref_traj /* (N+1)*nx or NULL = keep */);
int cddp_hip_get_reference(cddp_hip_handle *h, double *x_ref /* nx */, double *x_ref_traj /* (N+1)*nx */, int32_t *has_traj);
typedef struct cddp_hip_ref_path {
  int32_t abi_version, flags;   /* CDDP_HIP_ABI_VERSION; CDDP_HIP_REF_DEVICE or 0 */
  int64_t rows;                 /* L >= 1 */
  int64_t start;                /* cursor k0 >= 0 */
  double rows_per_step;         /* > 0, finite; 1.0: window row t of step k is path row k + t exactly */
  const double *path;           /* [L][nx]; copied, need not outlive the call */
} cddp_hip_ref_path;            /* 40 bytes */
int cddp_hip_mpc_set_reference_path(cddp_hip_handle *h, const cddp_hip_ref_path *desc /* NULL: unbind, reference left as it stands */);
int cddp_hip_mpc_reference_cursor(cddp_hip_handle *h, int64_t *cursor /* -1: no path bound */);

/* ---- getters (host buffers, batch-major) -------------------------------- */
int cddp_hip_get_results(cddp_hip_handle *h, cddp_hip_result *results /* batch */);
/* Head of the plan (round 4): u_0[batch][nu] and x_1[batch][nx] of every trajectory's current iterate -- what a receding-horizon
 * caller applies / re-starts from (examples/ipddp_mpcc_rc.py:649-705 reads sol.control_trajectory[0]); one small gather + one
 * copy instead of the whole (N + 1) x nx x batch trajectory.  Either pointer may be NULL. */
int cddp_hip_get_plan_head(cddp_hip_handle *h, double *u0, double *x1);
int cddp_hip_get_trajectory(cddp_hip_handle *h, double *X /* B*(N+1)*nx */, double *U /* B*N*nu */);
/* feedback_gains K_u (B*N*nu*nx) and feed-forward k_u (B*N*nu); either may be NULL. */
int cddp_hip_get_gains(cddp_hip_handle *h, double *K, double *k);
/* Value-function expansion along the horizon: Vx B*(N+1)*nx, Vxx B*(N+1)*nx*nx
 * (k_lambda_/K_lambda_ of ipddp_solver.cpp:1050-1104; V_x/V_xx of clddp_solver.cpp:188-192). */
int cddp_hip_get_value(cddp_hip_handle *h, double *Vx, double *Vxx);
/* The dynamics linearisation of the last backward pass, i.e. what precomputeDynamicsDerivatives leaves in F_x_ / F_u_
 * (cddp_solver_base.cpp:319-394): A[b][t] = I + dt f_x(x_t, u_t) (nx x nx, row-major), B[b][t] = dt f_u (nx x nu).  Either may be NULL. */
int cddp_hip_get_linearization(cddp_hip_handle *h, double *A /* B*N*nx*nx */, double *Bm /* B*N*nx*nu */);
/* Slack / dual / constraint residual trajectories, B*N*m each (m = total path dual dim). */
int cddp_hip_get_duals(cddp_hip_handle *h, double *S, double *Y, double *G);
/* Costate trajectory of the current iterate: Lambda_[t] = Lambda_[t] + alpha_pr k_lambda[t] + K_lambda[t] dx_t of the accepted forward pass
 * (ipddp_solver.cpp:1613-1616, 1660-1663: N + 1 rows; msipddp_solver.cpp:1466-1467, 1639-1641: N rows).  *rows receives the row count,
 * Lambda (B * rows * nx, may be NULL to query the count) the rows.  IPDDP and MSIPDDP handles only (added in round 5; ABI version unchanged). */
int cddp_hip_get_costates(cddp_hip_handle *h, double *Lambda, int32_t *rows);
/* Terminal-constraint state (IPDDP): stacked terminal-inequality slack / dual / residual
 * S_T, Y_T, G_T (B*mT each) and terminal-equality multipliers Lambda_T (B*pT); any may be NULL.
 * dims[0] = mT, dims[1] = pT (S_T_, Y_T_, G_T_, Lambda_T_eq_ of ipddp_solver.hpp). */
int cddp_hip_get_terminal(cddp_hip_handle *h, double *S_T, double *Y_T, double *G_T, double *Lambda_T, int32_t *dims);
/* Scalars of the last backward pass: dV (B*2), and per-trajectory regularisation (B). */
int cddp_hip_get_backward_scalars(cddp_hip_handle *h, double *dV, double *reg);
/* CDDPSolution::History for the first `hist_batch` trajectories (requires
 * options.return_iteration_info): hist[b][it][9] = {objective, merit, alpha_pr, alpha_du,
 * inf_du, inf_pr, inf_comp, mu, regularization}; counts[b] = entries; the `it` extent of the block is
 * cddp_hip_history_capacity(h) rows. */
int cddp_hip_get_history(cddp_hip_handle *h, int hist_batch, double *hist, int32_t *counts);
/* Rows per trajectory of the history block above: max_iterations + 1 of the options the handle was CREATED with
 * (cddp_hip_set_options may lower max_iterations afterwards; the row stride does not follow). */
int cddp_hip_history_capacity(cddp_hip_handle *h);

/* Write the 16-byte gather records of this handle's batch into a DEVICE buffer
 * (batch * sizeof(cddp_hip_gather_record)), on the handle's stream: the send buffer of the
 * single RCCL all-gather of SURVEY.md section 8(e). */
int cddp_hip_write_gather_records_device(cddp_hip_handle *h, void *device_ptr);

/* ---- device-resident inputs and outputs ----------------------------------
 * A solve can start from DEVICE arrays and return DEVICE arrays: a seed proposed by a policy network, a plan consumed by a training loop
 * or shifted by the caller's own kernel never crosses the bus and is never transposed on the host.  The arrays are batch-major, exactly
 * what the host entries take and return ([b][t][e], contiguous doubles); kernels convert to and from the handle's internal layouts
 * (csrc/inst_io.hip).  Pure data movement: every call is, bit for bit, its host counterpart.
 *  - cddp_hip_field_shape: rows T and columns E of the [batch][T][E] array of a field (K: nu*nx, VXX / A: nx*nx, B: nx*nu, LAMBDA: the rows
 *    cddp_hip_get_costates reports); no device work.  Either output may be NULL.
 *  - cddp_hip_get_field_device: the field as its host getter returns it (cddp_hip_get_trajectory, _get_gains, _get_value,
 *    _get_linearization, _get_duals, _get_costates), with the same refusals (no slack / dual rows, no costate trajectory).
 *  - cddp_hip_get_results_device: cddp_hip_get_results as columns in struct order -- cols[b][10] = final_objective, merit_function, inf_pr,
 *    inf_du, inf_comp, barrier_mu, regularization, alpha_pr, alpha_du, step_norm; icols[b][4] = iterations, status, n_backward, n_forward.
 *  - cddp_hip_set_initial_device: cddp_hip_set_initial from device arrays (U0_dev, X0_dev may be NULL with the same meaning; row 0 of the
 *    seed is x0 either way); the handle is left exactly as cddp_hip_set_initial leaves it.
 * Ordering, as cddp_hip_mpc_advance with CDDP_HIP_MPC_X_DEVICE: on a handle with a stream from cddp_hip_set_stream the kernels are ordered
 * on that stream (inputs written by work queued on it before the call are read, outputs are complete for work queued on it after) and the
 * call does not block; otherwise the call returns after the kernels have run: outputs complete, inputs free.
 * Refused before anything is launched, each with its own message, nothing changed: a NULL handle, an unknown field id, a NULL required
 * pointer, a pointer that is not device memory of the handle's device (a host address, pinned or not, never reaches a kernel), a pointer
 * whose allocation ends before the bytes the call touches.  A handle of several tile groups offsets the pointers per group.
 * (New entry points; ABI version unchanged.) */
enum cddp_hip_field { CDDP_HIP_FIELD_X = 0, CDDP_HIP_FIELD_U, CDDP_HIP_FIELD_K, CDDP_HIP_FIELD_KFF,
                      CDDP_HIP_FIELD_VX, CDDP_HIP_FIELD_VXX, CDDP_HIP_FIELD_A, CDDP_HIP_FIELD_B,
                      CDDP_HIP_FIELD_S, CDDP_HIP_FIELD_Y, CDDP_HIP_FIELD_G, CDDP_HIP_FIELD_LAMBDA };
int cddp_hip_field_shape(cddp_hip_handle *h, int field, int32_t *rows, int32_t *cols);   /* T and E of [B][T][E]; no device work */
int cddp_hip_get_field_device(cddp_hip_handle *h, int field, double *out_dev);           /* B*T*E doubles, batch-major */
int cddp_hip_get_results_device(cddp_hip_handle *h, double *cols_dev /* B*10 */, int32_t *icols_dev /* B*4 */);
int cddp_hip_set_initial_device(cddp_hip_handle *h, const double *x0_dev, const double *U0_dev, const double *X0_dev);
/* The plane of the slotted fields (X, U, S, Y, G, Lambda) that holds every trajectory's current iterate, slots[batch] (host, may be NULL),
 * and the number of planes: the slot rule the getters of those fields follow.  For tests and diagnosis. */
int cddp_hip_get_live_slots(cddp_hip_handle *h, int32_t *slots, int32_t *n_slots);

/* ---- linear response of a solved plan to its initial state -----------------
 * The first-order response of the closed-loop plan to a change of x_0 is the recursion dx_{t+1} = A_t dx_t + B_t du_t, du_t = K_t dx_t; the
 * gradient of a loss on (X, U) with respect to x_0 is its adjoint.  Both run on the device over the stacks where the sweep left them
 * (csrc/inst_sens.hip): no stack is copied or un-tiled.  With CLDDP K_t carries the clamped rows of the BoxQP (the active-set derivative),
 * with IPDDP it is the condensed interior-point gain.  Run forward, the recursion is the neighbouring-extremal correction of a plan for a
 * measured state.
 * WHICH SWEEP: K_t, A_t, B_t are the stacks cddp_hip_get_gains and cddp_hip_get_linearization read at the time of the call.  They belong to
 * the LAST BACKWARD SWEEP, which ran at the iterate BEFORE the last accepted step, not at the returned plan; at a converged solve the
 * difference is of the size of the last step.  A caller who wants them at the returned plan calls cddp_hip_backward first.
 * Arrays: batch-major, then the vector index, then time, then the element: [b][r][t][e], contiguous doubles, nvec vectors per trajectory.
 * flags = 0: host pointers; the call uploads, computes, downloads and returns when the outputs are written.  CDDP_HIP_SENS_DEVICE: every
 * array argument is a device pointer of the handle's device, checked and ordered as cddp_hip_get_field_device checks and orders its own
 * (see "device-resident inputs and outputs"); a handle of several tile groups offsets the pointers per group.  The handle's state is not
 * modified.
 * Arithmetic (the library is built with -ffp-contract=off: every product is rounded before it is added), per trajectory and per vector:
 *  - cddp_hip_plan_jvp: dx_0 = dx0.  For t = 0 .. N-1, first du_t: s = 0; for j ascending s += K_t[i][j] * dx_t[j]; du_t[i] = s.  Then
 *    dx_{t+1}: s = 0; for j ascending s += A_t[i][j] * dx_t[j]; for k ascending, on the same accumulator, s += B_t[i][k] * du_t[k];
 *    dx_{t+1}[i] = s.  dX rows are dx_0 .. dx_N, dU rows du_0 .. du_{N-1}; either output may be NULL, not both.
 *  - cddp_hip_plan_vjp: lam = gX_N (zeros when gX is NULL).  For t = N-1 .. 0, first mu: s = 0; for i ascending s += B_t[i][k] * lam[i];
 *    mu[k] = gU_t[k] + s (mu[k] = s when gU is NULL).  Then lam': s = 0; for i ascending s += A_t[i][j] * lam[i]; for k ascending
 *    s += K_t[k][j] * mu[k]; lam'[j] = gX_t[j] + s (lam'[j] = s when gX is NULL); lam = lam'.  gx0 = lam after t = 0.
 *  Non-finite stack rows propagate; nothing is special-cased.  (The sign of an exact zero is not specified.)
 * Refused before anything is launched, each with its own message, nothing changed: a NULL handle, unknown flag bits, nvec < 1, a NULL dx0
 * or gx0, dX and dU both NULL, a handle that was never solved or swept, an MSIPDDP handle (its plan carries defects and its gains belong to
 * the gap-closing recursion, so this recursion is not its response), and with CDDP_HIP_SENS_DEVICE a pointer cddp_hip_get_field_device
 * would refuse.  (New entry points; ABI version unchanged.) */
enum { CDDP_HIP_SENS_DEVICE = 1 };   /* all array arguments are device pointers of the handle's device */
int cddp_hip_plan_jvp(cddp_hip_handle *h, int flags, int nvec,
                      const double *dx0 /* B*nvec*nx */,
                      double *dX /* B*nvec*(N+1)*nx or NULL */, double *dU /* B*nvec*N*nu or NULL */);
int cddp_hip_plan_vjp(cddp_hip_handle *h, int flags, int nvec,
                      const double *gX /* B*nvec*(N+1)*nx or NULL = zeros */,
                      const double *gU /* B*nvec*N*nu or NULL = zeros */,
                      double *gx0 /* B*nvec*nx */);

/* ---- state and control covariance along a solved plan ----------------------
 * Given an uncertain initial state, process noise and actuator noise, how uncertain are the states and controls of the plan under its own
 * feedback gains, and what does that uncertainty cost?  The perturbation follows dx_{t+1} = (A_t + B_t K_t) dx_t + B_t eps_t + w_t with
 * cov(dx_0) = Sigma0, cov(w_t) = W, cov(eps_t) = Wu, white in time.  cddp_hip_plan_covariance runs the covariance recursion on the device
 * over the stacks where the sweep left them (csrc/inst_cov.hip: one workgroup per 64-trajectory tile, Sigma_t in LDS): no stack is copied or
 * un-tiled.  SX rows are Sigma_0 .. Sigma_N, SU rows cov(du_t) = K_t Sigma_t K_t^T + Wu for t = 0 .. N-1, and dcost is the expected increase
 * of the quadratic objective under that uncertainty, sum_t tr(Q dt Sigma_t) + tr(R dt SU_t), plus tr(Qf Sigma_N) (the objective has no 1/2).
 * WHICH SWEEP: K_t, A_t, B_t are the stacks cddp_hip_get_gains and cddp_hip_get_linearization read at the time of the call.  They belong to
 * the LAST BACKWARD SWEEP, which ran at the iterate BEFORE the last accepted step, not at the returned plan; at a converged solve the
 * difference is of the size of the last step.  A caller who wants them at the returned plan calls cddp_hip_backward first.
 * Arrays: batch-major, contiguous doubles, matrices row-major.  Sigma0, W and Wu are ONE matrix each for the whole batch (nx*nx, nx*nx,
 * nu*nu), or with CDDP_HIP_COV_PER_TRAJ one per trajectory, all three together (B*nx*nx, B*nx*nx, B*nu*nu); W and Wu may be NULL (no such
 * noise).  SX is [b][t][i][j] and SU [b][t][i][j]; with CDDP_HIP_COV_DIAG only the diagonals are written, SX [b][t][i] and SU [b][t][i]
 * (the recursion itself is the full one).  Any output may be NULL, not all.
 * flags without CDDP_HIP_COV_DEVICE: host pointers; the call uploads, computes, downloads and returns when the outputs are written.
 * CDDP_HIP_COV_DEVICE: every array argument is a device pointer of the handle's device, checked and ordered as cddp_hip_plan_jvp checks
 * and orders its own; a handle of several tile groups offsets the pointers per group.  The handle's state is not modified.
 * Arithmetic (the library is built with -ffp-contract=off: every product is rounded before it is added).  Every sum starts at the stated
 * value and runs with the index ascending, so the result does not depend on how the work is spread over lanes.  Only the lower triangle
 * (j <= i) of Sigma0, W and Wu is read: element [i][j] with j > i stands for element [j][i] wherever it appears below.  Every covariance
 * is computed for j <= i and mirrored, so the outputs are exactly symmetric.  Sigma_0 = Sigma0 (mirrored).  Per trajectory, for
 * t = 0 .. N-1:
 *  1. Acl[i][j]: s = A_t[i][j]; for k ascending s += B_t[i][k] * K_t[k][j].
 *  2. Z[i][j] (nu x nx): s = 0; for l ascending s += K_t[i][l] * Sigma_t[l][j].
 *  3. SU_t[i][j]: s = 0; for l ascending s += Z[i][l] * K_t[j][l]; then s += Wu[i][j] if Wu is given.
 *  4. Y[i][j]: s = 0; for l ascending s += Acl[i][l] * Sigma_t[l][j].
 *  5. Sigma_{t+1}[i][j]: s = 0; for l ascending s += Acl[i][l] * Y[j][l].  If W is given: s += W[i][j].  If Wu is given: G[i][k]:
 *     g = 0; for m ascending g += B_t[i][m] * Wu[m][k]; then h = 0; for k ascending h += G[i][k] * B_t[j][k]; s += h.
 *  6. the cost of step t: r_i = 0; for j ascending r_i += Qdt[i][j] * Sigma_t[i][j] (Qdt = Q * dt, as the solver holds it); c = 0; for i
 *     ascending c += r_i; then the same with Rdt = R * dt and SU_t, for i ascending added on the same c; dcost += c, with t ascending
 *     from dcost = 0.
 * After the loop the term of Qf and Sigma_N is formed the same way (r_i, then c from 0) and added last.
 * Non-finite stack rows propagate; nothing is special-cased.  (The sign of an exact zero is not specified.)
 * Refused before anything is launched, each with its own message, nothing changed: a NULL handle, unknown flag bits, a NULL Sigma0, SX, SU
 * and dcost all NULL, a handle that was never solved or swept, an MSIPDDP handle (its plan carries defects and its gains belong to the
 * gap-closing recursion, so this recursion is not its response), and with CDDP_HIP_COV_DEVICE a pointer cddp_hip_get_field_device would
 * refuse.  (New entry point; ABI version unchanged.) */
enum { CDDP_HIP_COV_DEVICE = 1, CDDP_HIP_COV_DIAG = 2, CDDP_HIP_COV_PER_TRAJ = 4 };
int cddp_hip_plan_covariance(cddp_hip_handle *h, int flags,
                             const double *Sigma0 /* nx*nx, or B*nx*nx with PER_TRAJ */,
                             const double *W      /* process noise, nx*nx | B*nx*nx, or NULL */,
                             const double *Wu     /* actuator noise, nu*nu | B*nu*nu, or NULL */,
                             double *SX    /* B*(N+1)*nx*nx (DIAG: B*(N+1)*nx) or NULL */,
                             double *SU    /* B*N*nu*nu     (DIAG: B*N*nu)     or NULL */,
                             double *dcost /* B or NULL */);

/* ---- time-varying LQR tracking gains along a solved plan --------------------
 * The gain stack a solve leaves behind is a by-product of the optimiser: rows of a clamped control are zero (CLDDP), the gains carry the
 * barrier curvature at the last mu (IPDDP), and they belong to the regularised Quu of the last sweep.  cddp_hip_plan_tvlqr designs the
 * controller a caller would stabilise the plan with instead: the finite-horizon LQR of the plan's linearisation (A_t, B_t) for the
 * caller's own tracking weights, du_t = K_t dx_t minimising sum_t dx_t^T Qd dx_t + du_t^T Rd du_t, plus dx_N^T Qf dx_N, with its
 * cost-to-go matrices P_t (dx_t^T P_t dx_t is the cost from step t on).  The recursion runs on the device over the stacks where the sweep
 * left them (csrc/inst_lqr.hip: one workgroup per tile of trajectories walks the horizon backward, P_t in LDS).
 * WHICH SWEEP: A_t, B_t are the stacks cddp_hip_get_linearization reads at the time of the call.  They belong to the LAST BACKWARD SWEEP,
 * which ran at the iterate before the last accepted step; a caller who wants them at the returned plan calls cddp_hip_backward first.
 * Weights: Q (nx*nx) and R (nu*nu) are unscaled, as in cddp_hip_problem: Qd[i][j] = Q[i][j] * dt and Rd[i][j] = R[i][j] * dt, one rounded product per element (formed where the element is read);
 * Qf (nx*nx) is used as given.  A NULL weight means the handle's own Q dt / R dt / Qf, as cddp_hip_plan_covariance reads them for dcost.
 * With CDDP_HIP_LQR_PER_TRAJ every weight that is given is one matrix per trajectory, batch-major (B*nx*nx, B*nu*nu, B*nx*nx); weights
 * that are not given stay the handle's.  Only the lower triangles (j <= i) are read: element [i][j] with j > i stands for element [j][i].
 * Outputs: K_out [b][t][k][j] for t = 0 .. N-1, P_out [b][t][i][j] for t = 0 .. N (row N is Qf's lower triangle mirrored; every P_t is
 * exactly symmetric), info [b]; any may be NULL.  Batch-major, contiguous, matrices row-major.
 * flags without CDDP_HIP_LQR_DEVICE: host pointers; the call uploads, computes, downloads and returns when the outputs are written.
 * CDDP_HIP_LQR_DEVICE: every array argument is a device pointer of the handle's device, checked and ordered as
 * cddp_hip_plan_covariance checks and orders its own; a handle of several tile groups offsets the pointers per group.
 * The handle's plan, duals and solver state are not modified.
 * CDDP_HIP_LQR_INSTALL additionally writes K_t into the handle's gain stack; the feedforward k_t is left alone.  From then until the next
 * backward sweep (cddp_hip_backward, cddp_hip_solve, an MPC step) the installed gains are what cddp_hip_get_gains and CDDP_HIP_FIELD_K
 * return and what cddp_hip_track_plan, cddp_hip_plan_jvp / _vjp, cddp_hip_plan_covariance, cddp_hip_plan_montecarlo and
 * cddp_hip_score_rollouts(CDDP_HIP_SCORE_FEEDBACK) read: they evaluate the designed controller.  The gain stack is dead state at the
 * start of a solve (every iteration sweeps before it rolls out, and cddp_hip_mpc_advance moves X | U | S | Y only): a later solve is bit
 * for bit the solve of a handle that never installed anything.  cddp_hip_forward is a single step of the solver, not one of the entries
 * above: it rolls out with the gains of its own route, which need not be the installed ones; call cddp_hip_backward before it.
 * Arithmetic (the library is built with -ffp-contract=off: every product is rounded before it is added; true division and square root,
 * no reciprocals).  Every sum starts at the stated value and runs with the index ascending.  Per trajectory P_N = Qf mirrored; for
 * t = N-1 .. 0, with P = P_{t+1}, A = A_t, B = B_t:
 *  1. M[i][k] (nx x nu): s = 0; for l ascending s += P[i][l] * B[l][k].
 *  2. Quu[r][c] for c <= r: s = 0; for l ascending s += B[l][r] * M[l][c]; then s += Rd[r][c].
 *  3. Qux[k][j] (nu x nx): s = 0; for l ascending s += M[l][k] * A[l][j].
 *  4. Quu = L L^T, rows r ascending.  For c < r: s = Quu[r][c]; for m < c ascending s -= L[r][m] * L[c][m]; L[r][c] = s / L[c][c].
 *     Diagonal: s = Quu[r][r]; for m < r ascending s -= L[r][m] * L[r][m]; the step FAILS unless s > 0; L[r][r] = sqrt(s).
 *  5. For every column j.  Forward, r ascending: s = Qux[r][j]; for m < r ascending s -= L[r][m] * y[m]; y[r] = s / L[r][r].
 *     Backward, r descending: s = y[r]; for m > r ascending s -= L[m][r] * z[m]; z[r] = s / L[r][r].  K_t[r][j] = -z[r].
 *  6. Acl[i][j]: s = A[i][j]; for k ascending s += B[i][k] * K_t[k][j].
 *  7. Y[i][j]: s = 0; for l ascending s += P[i][l] * Acl[l][j].
 *  8. T[k][j] (nu x nx): s = 0; for m ascending s += Rd[k][m] * K_t[m][j].
 *  9. P_t[i][j] for j <= i: s = 0; for l ascending s += Acl[l][i] * Y[l][j]; h = 0; for k ascending h += K_t[k][i] * T[k][j]; s += h;
 *     s += Qd[i][j].  Mirrored.  (The Joseph form P_t = Qd + K^T Rd K + Acl^T P Acl: symmetric by construction.)
 * Failure of one trajectory: the walk goes backward, so the first failed step met is the largest such t.  Then info[b] = t + 1, and
 * K_s = 0 (also in the installed stack) and P_s = NaN for every s <= t; rows s > t are those computed.  Otherwise info[b] = 0.  Other
 * trajectories are unaffected.  Non-finite stack rows end in a failed pivot (NaN > 0 is false).  (The sign of an exact zero is not
 * specified.)
 * Refused before anything is launched, each with its own message, nothing changed: a NULL handle, unknown flag bits, K_out and P_out NULL
 * without CDDP_HIP_LQR_INSTALL (nothing to compute), a handle that was never solved or swept, an MSIPDDP handle, a non-finite value in a
 * host weight, and with CDDP_HIP_LQR_DEVICE a pointer cddp_hip_get_field_device would refuse.  (New entry point; ABI version unchanged.) */
enum { CDDP_HIP_LQR_DEVICE = 1, CDDP_HIP_LQR_PER_TRAJ = 2, CDDP_HIP_LQR_INSTALL = 4 };
int cddp_hip_plan_tvlqr(cddp_hip_handle *h, int flags,
                        const double *Q  /* nx*nx | B*nx*nx with PER_TRAJ, or NULL */,
                        const double *R  /* nu*nu | B*nu*nu, or NULL */,
                        const double *Qf /* nx*nx | B*nx*nx, or NULL */,
                        double *K_out    /* B*N*nu*nx or NULL */,
                        double *P_out    /* B*(N+1)*nx*nx or NULL */,
                        int32_t *info    /* B or NULL */);

/* ---- Kalman filter gains and output-feedback covariance along a solved plan --
 * The entries above assume the controller sees the state.  With sensors, which estimator gains go with the plan, and how uncertain are
 * states and controls when the feedback acts on the estimate?  The perturbation model is that of cddp_hip_plan_covariance,
 * dx_{t+1} = A_t dx_t + B_t (du_t + eps_t) + w_t, cov(dx_0) = Sigma0, cov(w_t) = W, cov(eps_t) = Wu, white in time, with a measurement at
 * every step t = 0 .. N, taken before u_t is applied: y_t = C dx_t + n_t, cov(n_t) = diag(v), C ny x nx with 1 <= ny <= CDDP_HIP_KF_MAX_NY
 * (ny may exceed nx).  The feedback acts on the filtered estimate, du_t = K_t xhat_t|t, with K_t the handle's gain stack at the time of the
 * call.  cddp_hip_plan_kalman runs the filter and the covariance recursion on the device over the stacks where the sweep left them
 * (csrc/inst_kf.hip: one workgroup per tile of trajectories walks the horizon forward, the two covariances in LDS).
 * Measurement noise is DIAGONAL on purpose: the rows of a step are then processed one at a time, with no factorisation, and ny is a
 * run-time number.  Correlated measurement noise is the caller's to whiten (C <- V^-1/2 C, v <- 1).  C, v, W and Wu do not vary in time.
 * WHICH SWEEP: K_t, A_t, B_t are the stacks cddp_hip_get_gains and cddp_hip_get_linearization read at the time of the call.  They belong to
 * the LAST BACKWARD SWEEP, which ran at the iterate before the last accepted step; a caller who wants them at the returned plan calls
 * cddp_hip_backward first.  After cddp_hip_plan_tvlqr with CDDP_HIP_LQR_INSTALL the recursion sees the installed gains.
 * Arrays: batch-major, contiguous doubles, matrices row-major.  C (ny*nx), v (ny), Sigma0, W (nx*nx) and Wu (nu*nu) are ONE array each
 * for the whole batch, or with CDDP_HIP_KF_PER_TRAJ one per trajectory, every given input together (B*ny*nx, B*ny, ...); W and Wu may be
 * NULL (no such noise).  Only the lower triangles (j <= i) of Sigma0, W and Wu are read.  Outputs, any may be NULL, not all with info:
 * L_out [b][t][i][r] the filter gain of step t (xhat_t|t = xhat_t|t-1 + L_t (y_t - C xhat_t|t-1)), SP_out [b][t][i][j] the error
 * covariance Sm_t before the measurement of step t, SF_out the one after it (Sf_t), SX [b][t][i][j] the covariance of the true state
 * under output feedback, all for t = 0 .. N; SU [b][t][i][j] = cov(du_t) for t = 0 .. N-1; dcost [b] as cddp_hip_plan_covariance's, with
 * these SX and SU; info [b].  With CDDP_HIP_KF_DIAG only the diagonals of SP_out, SF_out, SX and SU are written ([b][t][i]); L_out is
 * always full, and the recursion itself is the full one.
 * flags without CDDP_HIP_KF_DEVICE: host pointers; the call uploads, computes, downloads and returns when the outputs are written.
 * CDDP_HIP_KF_DEVICE: every array argument is a device pointer of the handle's device, checked and ordered as
 * cddp_hip_plan_covariance checks and orders its own; a handle of several tile groups offsets the pointers per group.
 * The handle's plan, gains, duals and solver state are not modified.
 * Arithmetic (the library is built with -ffp-contract=off: every product is rounded before it is added; true division, no reciprocals).
 * Every sum starts at the stated value and runs with the index ascending; every symmetric quantity is computed for j <= i and mirrored.
 * Per trajectory Sm_0 = Sigma0 (mirrored) and Xm_0 = 0 (the covariance of the predicted estimate).  For t = 0 .. N:
 *  1. The update.  S = Sm_t, G = 0; for the rows r = 0 .. ny-1 of C ascending, with c = C[r]:
 *     a. h[i]: s = 0; for j ascending s += S[i][j] * c[j].
 *     b. sr: s = v[r]; for j ascending s += c[j] * h[j].  The row FAILS unless sr > 0.
 *     c. g[i] = h[i] / sr.
 *     d. S[i][j] for j <= i: e = S[i][j]; e -= g[i] * h[j]; e -= h[i] * g[j]; q = sr * g[i]; e += q * g[j].  Mirrored.  (The symmetric
 *        Joseph form S - g h^T - h g^T + sr g g^T.  An all-zero row of C leaves S unchanged: h = 0, g = 0.)
 *     e. G[i][j] for j <= i: G[i][j] += h[i] * g[j].  Mirrored.  (A sum of rank-one terms: no covariance is subtracted from another.)
 *     Sf_t = S after the last row.
 *  2. L_t[i][r]: s = 0; for j ascending s += Sf_t[i][j] * C[r][j]; L_t[i][r] = s / v[r].  (Equal to Sm C^T (C Sm C^T + V)^-1.)
 *  3. Xh_t[i][j] = Xm_t[i][j] + G[i][j] (the covariance of the filtered estimate), and SX_t[i][j] = Xh_t[i][j] + Sf_t[i][j].
 *  4. For t < N, in the steps of cddp_hip_plan_covariance's arithmetic: Acl by its step 1; SU_t by its steps 2 and 3 with Xh_t in the place
 *     of Sigma_t; Sm_{t+1} by its steps 4 and 5 with A_t in the place of Acl and Sf_t in the place of Sigma_t (W and Wu added as there);
 *     Xm_{t+1} by its steps 4 and 5 with Xh_t in the place of Sigma_t and neither W nor Wu.
 *  5. dcost by its step 6 with SX_t and SU_t, the term of Qf and SX_N added last.
 * Failure of one trajectory: the walk goes forward; the first failed row, at step t, gives info[b] = t + 1, every output row s >= t of
 * that trajectory is NaN (rows before it are those computed) and its dcost is NaN.  Otherwise info[b] = 0.  Other trajectories are
 * unaffected.  Non-finite stack rows end in a failed row (NaN > 0 is false).  (The sign of an exact zero is not specified.)
 * Not covered: correlated measurement noise, time-varying C, v or W, intermittent measurements, an estimator inside cddp_hip_track_plan
 * or the MPC loop (cddp_hip_plan_montecarlo_of below carries one through the Monte-Carlo evaluation), and the relinearisation of an
 * extended Kalman filter.
 * Refused before anything is launched, each with its own message, nothing changed: a NULL handle, unknown flag bits, ny outside
 * 1 .. CDDP_HIP_KF_MAX_NY, a NULL C, v or Sigma0, all six outputs and info NULL, a handle that was never solved or swept, an MSIPDDP
 * handle, a host v with an entry that is not finite or not > 0, a non-finite value in any other host input, and with CDDP_HIP_KF_DEVICE a
 * pointer cddp_hip_get_field_device would refuse.  (New entry point; ABI version unchanged.) */
enum { CDDP_HIP_KF_DEVICE = 1, CDDP_HIP_KF_DIAG = 2, CDDP_HIP_KF_PER_TRAJ = 4 };
#define CDDP_HIP_KF_MAX_NY 16
int cddp_hip_plan_kalman(cddp_hip_handle *h, int flags, int ny,
                         const double *C      /* ny*nx | B*ny*nx with PER_TRAJ */,
                         const double *v      /* ny | B*ny: measurement variances */,
                         const double *Sigma0 /* nx*nx | B*nx*nx */,
                         const double *W      /* nx*nx | B*nx*nx, or NULL */,
                         const double *Wu     /* nu*nu | B*nu*nu, or NULL */,
                         double *L_out  /* B*(N+1)*nx*ny or NULL */,
                         double *SP_out /* prior Sm_t:     B*(N+1)*nx*nx (DIAG: B*(N+1)*nx) or NULL */,
                         double *SF_out /* posterior Sf_t: same shape, or NULL */,
                         double *SX     /* as cddp_hip_plan_covariance's, or NULL */,
                         double *SU     /* B*N*nu*nu (DIAG: B*N*nu) or NULL */,
                         double *dcost  /* B or NULL */,
                         int32_t *info  /* B or NULL */);

/* ---- scoring candidate control sequences and seeding from the best -----------
 * The plan a nonconvex solve ends in depends on the control sequence it starts from.  cddp_hip_score_rollouts rolls S candidate control
 * sequences per trajectory out in ONE launch (csrc/inst_score.hip, one lane per trajectory and candidate) and returns what each is worth:
 * its objective and its largest constraint violation, optionally the states and the applied controls.  cddp_hip_seed_best picks a winner
 * per trajectory and seeds the handle from it on the device.  The same rollout scores the plan's feedback policy from a cloud of
 * initial states (CDDP_HIP_SCORE_FEEDBACK) and a candidate on a mismatched plant (plant != NULL).  Candidates are the caller's here:
 * these two entries draw no noise and blend nothing ("sampling-based plan refinement" below does).
 * Arrays: batch-major, then the candidate, then time, then the element, contiguous doubles.  flags without CDDP_HIP_SCORE_DEVICE: host
 * pointers, staged through device scratch the handle owns (grown on demand, freed with the handle); the call returns when the outputs
 * are written.  CDDP_HIP_SCORE_DEVICE: every pointer is device memory of the handle's device, checked and ordered as
 * cddp_hip_get_field_device checks and orders its own; a handle of several tile groups offsets the pointers per group.
 * Arithmetic (the library is built with -ffp-contract=off; the tests are bitwise), per trajectory b and candidate c:
 *   x = x0 (x0[b], x0[b][c] with CDDP_HIP_SCORE_X0_PER_CANDIDATE, row 0 of the live plan when x0 is NULL); cost = 0.0; viol = 0.0;
 *   for t = 0 .. N-1, in this order:
 *    - u = U[b][c][t].  With CDDP_HIP_SCORE_FEEDBACK u[i] = U[b][c][t][i] + s, s = 0; for j ascending s += K_t[i][j] * (x[j] - X_t[j]):
 *      the line of cddp_hip_track_plan, X_t and K_t read from the live slot and the gain stack; U == NULL then means the plan's own U_t.
 *    - with a plant: u[i] = fmin(fmax(u[i], u_lower[i]), u_upper[i]) (only with a box); u is the saturated control from here on.
 *    - cost += (e^T (Q dt)) e + (u^T (R dt)) u, e = x - x_ref (x - x_ref_traj[t] when the problem has a per-step reference): for every
 *      column j a zero accumulator r += e[i] * Qdt[i][j], i ascending, then sx += r * e[j]; likewise su; the step adds sx + su.
 *    - every path row g_i = g(x, u) - upper in the problem's stacked order (the constraint objects sorted by name), as the solver
 *      evaluates it; viol = max(viol, g_i) for i ascending, written (viol < g_i) ? g_i : viol.
 *    - x <- step(integrator, dt, params, x, u) of the handle's own model; with a plant `substeps` steps of dt / substeps with the plant's
 *      parameter block of trajectory b (see "closed loop against a separate plant").
 *   then cost += (e_N^T Qf) e_N and the terminal INEQUALITY rows A_N x_N - b_N are folded into viol the same way (IPDDP handles; the
 *   other solvers ignore the terminal set).  Terminal EQUALITIES are not part of viol.
 *  Cost and rows are evaluated on x_t BEFORE the step: the order of cddp_hip_initialize, whose final_objective a candidate's cost equals
 *  bit for bit.  viol > 0 means some row is violated by that much; a feasible rollout has viol = 0.  A non-finite state makes cost
 *  non-finite (0 * NaN is NaN); a NaN row alone is not seen by max().  X_out rows are x_0 .. x_N, U_out rows the controls as applied.
 *  The handle's solver state is not modified.
 * cddp_hip_seed_best, per trajectory (csrc/score_select.hpp): a candidate is FINITE when cost and viol are both finite, ADMISSIBLE when
 * it is finite and viol <= viol_tol.  The winner is the admissible candidate of lowest cost; when none is admissible, the finite
 * candidate of lowest viol, then of lowest cost; ties go to the lowest c.  When no candidate is finite winner[b] = -1, the trajectory
 * is seeded from c = 0 and the call still succeeds.  The handle is then left bit for bit as
 * cddp_hip_set_initial_device(h, x0, U[:, winner], NULL) leaves it (x0 == NULL: the seed's x0 and state rows stay as they are, which
 * needs an earlier cddp_hip_set_initial); nothing else of the handle changes.
 * Refused before anything is launched, each with its own message, nothing changed: a NULL handle, unknown flag bits, ncand < 1, a NULL
 * cost, a NULL U without CDDP_HIP_SCORE_FEEDBACK (seed_best: a NULL U), CDDP_HIP_SCORE_X0_PER_CANDIDATE or a handle without a plan
 * with a NULL x0, CDDP_HIP_SCORE_FEEDBACK on a handle cddp_hip_track_plan would refuse, a plant cddp_hip_track_plan would refuse, and
 * with CDDP_HIP_SCORE_DEVICE a pointer cddp_hip_get_field_device would refuse.  (New entry points; ABI version unchanged.) */
enum { CDDP_HIP_SCORE_DEVICE = 1,            /* every pointer is device memory of the handle's device */
       CDDP_HIP_SCORE_FEEDBACK = 2,          /* u_t = U_c,t + K_t (x_t - X_t) around the handle's live plan; U == NULL then means the plan's own U */
       CDDP_HIP_SCORE_X0_PER_CANDIDATE = 4 };/* x0 is [B][S][nx] instead of [B][nx] */
int cddp_hip_score_rollouts(cddp_hip_handle *h, cddp_hip_plant *plant /* NULL: the handle's own model, integrator, dt, parameters */,
                            int flags, int ncand /* S >= 1 */,
                            const double *x0   /* [B][nx] | [B][S][nx] | NULL = row 0 of the live plan */,
                            const double *U    /* [B][S][N][nu] */,
                            double *cost       /* [B][S] */,
                            double *viol       /* [B][S] or NULL */,
                            double *X_out      /* [B][S][N+1][nx] or NULL */,
                            double *U_out      /* [B][S][N][nu] applied controls, or NULL */);
int cddp_hip_seed_best(cddp_hip_handle *h, int flags /* CDDP_HIP_SCORE_DEVICE or 0 */, int ncand,
                       const double *x0 /* [B][nx] or NULL = keep the handle's x0 */, const double *U /* [B][S][N][nu] */,
                       const double *cost /* [B][S] */, const double *viol /* [B][S] or NULL = all 0 */, double viol_tol,
                       int32_t *winner /* [B] or NULL */);

/* ---- sampling-based plan refinement (MPPI) with candidates drawn in the kernel -----------
 * The sampling front end of a nonconvex solve: perturb the current plan, roll the candidates out, weight them by a softmin of their cost,
 * blend, repeat, then seed the solver.  The candidates come from a counter-based generator, so the lane that scores a candidate and the
 * lane that blends it draw the same numbers and no [B][S][N][nu] array lies between them (cddp_hip_mppi_refine allocates none); results
 * are a function of (seed, stream) alone, and a tile group draws what the whole batch would draw because the counter carries the
 * trajectory's index in the batch.  csrc/mppi.hpp is the normative statement (host and device compile it), restated here; the library is
 * built with -ffp-contract=off and the tests are bitwise.
 * Generator: Philox4x32-10, multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85.
 * Normal pair: element e = t * nu + i of candidate c of trajectory b lies in pair j = e >> 1.  Counter = (j, c, b, stream), key = (seed
 *  low word, seed high word), output words r0..r3; m1 = ((u64)r1 << 32 | r0) >> 11, m2 = ((u64)r3 << 32 | r2) >> 11,
 *  u1 = ((double)m1 + 1.0) * 0x1p-53, u2 = (double)m2 * 0x1p-53, rad = sqrt(-2.0 * log_fast(u1)),
 *  (s, co) = sincos_fast(0x1.921fb54442d18p+2 * u2); z = rad * co for even e, rad * s for odd e (log_fast, sincos_fast: csrc/dev_trig.hpp,
 *  always inside their fast range; sqrt correctly rounded).
 * Candidate: u_c[t][i] = mean[t][i] + sigma[i] * z, then fmin(fmax(u, u_lower[i]), u_upper[i]) with a box; with keep_mean candidate 0
 *  takes z = 0.
 * Weights, per trajectory over c ascending: a candidate is admissible when cost and viol are finite and viol <= viol_tol (the predicate of
 *  cddp_hip_seed_best).  rho = the lowest admissible cost, q = (cost_c - rho) / lambda, a_c = q <= 700.0 ? exp_fast(-q) : 0.0 (0 when
 *  inadmissible), eta = sum a_c, w_c = a_c / eta, ess = 1 / sum w_c^2.  When no candidate is admissible every w_c = 0, the trajectory's
 *  mean is left as it is and n_adm = rho = ess = 0.
 * Blend, per element: s = 0; for c ascending s += w_c * (u_c[t][i] - mean[t][i]); mean' = mean + s, clipped to the box when there is one.
 * cddp_hip_sample_controls writes the candidates of desc->stream around U_mean (NULL: the live plan's U, which needs a plan).
 * cddp_hip_mppi_blend weighs and blends candidates the caller supplies as they lie (viol NULL = all 0); only lambda, viol_tol, ncand and the
 *  box of the descriptor matter to it.  stats is [B][3] = n_adm, rho, ess.
 * cddp_hip_mppi_refine runs desc->iters rounds of score -> weights -> blend, round k with stream desc->stream + k.  Scoring is
 *  cddp_hip_score_rollouts' arithmetic and order without feedback, on the handle's model or on `plant`, whose own box is applied after the
 *  descriptor's (the blend uses the control as drawn and clipped by the descriptor's box).  x0 NULL: row 0 of the live plan.  U_out is the
 *  mean after the last round; cost_out, viol_out [B][S] and stats [B][3] (each may be NULL) are those of the last round.  With
 *  CDDP_HIP_MPPI_SEED the handle is then left bit for bit as cddp_hip_set_initial_device(h, x0, U_out, NULL) leaves it (x0 NULL: the seed's
 *  x0 and state rows stay as they are, which needs an earlier cddp_hip_set_initial); otherwise the handle's solver state is untouched.
 * Flags, pointer checks, stream ordering, tile-group offsets and the handle-owned scratch are those of cddp_hip_score_rollouts: host
 * pointers by default, CDDP_HIP_SCORE_DEVICE for device pointers (sigma and the box are always host arrays, read during the call).
 * Refused before anything is launched, each with its own message: a NULL handle or descriptor, unknown flag bits, iters < 1, ncand < 1, a
 * lambda that is not positive and finite, a NaN viol_tol, a NULL sigma or an entry that is not positive and finite, a half-given box or
 * lower > upper, a NULL U_mean on a handle without a plan, a NULL output, what cddp_hip_score_rollouts refuses of x0 and the plant, what
 * cddp_hip_seed_best refuses of a NULL x0 (CDDP_HIP_MPPI_SEED), and with CDDP_HIP_SCORE_DEVICE a pointer cddp_hip_get_field_device would
 * refuse.  (New entry points; ABI version unchanged.) */
typedef struct cddp_hip_mppi_desc {
  uint64_t seed;
  uint32_t stream;                     /* the noise stream; refinement round k draws from stream + k */
  int32_t iters;                       /* rounds of cddp_hip_mppi_refine (>= 1; the other entries ignore it but check it) */
  int32_t ncand;                       /* S >= 1 */
  int32_t keep_mean;                   /* nonzero: candidate 0 is the mean itself */
  double lambda;                       /* temperature of the softmin, positive */
  double viol_tol;
  const double *sigma;                 /* [nu], host */
  const double *u_lower, *u_upper;     /* [nu], host; both set or both NULL */
} cddp_hip_mppi_desc;                  /* 64 bytes */
enum { CDDP_HIP_MPPI_SEED = 8 };       /* cddp_hip_mppi_refine: seed the handle from the refined mean (with CDDP_HIP_SCORE_DEVICE or without) */
int cddp_hip_sample_controls(cddp_hip_handle *h, int flags, const cddp_hip_mppi_desc *desc,
                             const double *U_mean /* [B][N][nu] or NULL = the live plan's U */, double *U_out /* [B][S][N][nu] */);
int cddp_hip_mppi_blend(cddp_hip_handle *h, int flags, const cddp_hip_mppi_desc *desc, const double *U_mean /* [B][N][nu] */,
                        const double *U_cand /* [B][S][N][nu] */, const double *cost /* [B][S] */, const double *viol /* [B][S] or NULL */,
                        double *U_out /* [B][N][nu] */, double *stats /* [B][3] or NULL */);
int cddp_hip_mppi_refine(cddp_hip_handle *h, cddp_hip_plant *plant /* or NULL */, int flags, const cddp_hip_mppi_desc *desc,
                         const double *x0 /* [B][nx] or NULL */, const double *U_mean /* [B][N][nu] or NULL = the live plan's U */,
                         double *U_out /* [B][N][nu] */, double *cost_out /* [B][S] or NULL */, double *viol_out /* [B][S] or NULL */,
                         double *stats /* [B][3] or NULL */);

/* ---- Monte-Carlo evaluation of a solved plan under noise --------------------------------
 * What do the true nonlinear plant, the actuator box and the constraint rows do to the Gaussian picture of cddp_hip_plan_covariance?
 * cddp_hip_plan_montecarlo rolls S noisy closed loops per trajectory around the live plan in ONE launch (csrc/inst_mc.hip: one workgroup per
 * trajectory, one lane per sample), draws the initial-state, actuator and process noise in the lane from the counter-based generator of
 * "sampling-based plan refinement" and reduces across the samples on the device in a fixed order: moments, counts and per-sample scalars
 * leave the GPU, no [B][S][N][..] array exists unless X_out / U_out ask for one.  cddp_hip_mc_sample_noise writes the coloured noise
 * itself.  csrc/plan_mc.hpp is the normative statement (host and device compile it), restated here; the library is built with
 * -ffp-contract=off and the tests are bitwise.
 * Noise: L0, Lw, Lu are lower-triangular factors of cov(dx_0) = Sigma0, cov(w_t) = W, cov(eps_t) = Wu, one matrix each for the whole
 *  batch, row-major HOST arrays read during the call (only j <= i is read); a NULL factor means no such noise.
 * Normals: sample c of trajectory b (its index in the whole batch) uses z(e) = the normal of element e of candidate c of trajectory b of
 *  the generator above (counter (e >> 1, c, b, stream), even / odd half), with e = i (i < nx) for the initial state,
 *  e = nx + t (nu + nx) + i (i < nu) for the actuator noise of step t and e = nx + t (nu + nx) + nu + i (i < nx) for its process noise.  A
 *  NULL factor skips its draws and leaves the indices where they are.  With keep_nominal sample 0 takes z = 0 everywhere.  An MPPI call
 *  with the same (seed, stream) shares this counter space.
 * Coloured noise: v[i] = s, s = 0; for j ascending, j <= i: s += L[i][j] * z[j].
 * Rollout of sample c: x[i] = xbase[i] + v0[i] (xbase = x0[b], or row 0 of the live plan), cost = 0, viol = 0; for t = 0 .. N-1 in the
 *  order of cddp_hip_score_rollouts: uc[i] = U_t[i] + eps[i]; u[i] = uc[i] + s, s = 0; for j ascending s += K_t[i][j] * (x[j] - X_t[j]); the
 *  plant's box; cost += the running cost; v_t = 0 folded over the path rows, viol = max(viol, v_t); the step(s); with Lw
 *  x[i] = xn[i] + w[i] (cddp_hip_plant_step's line).  Then the terminal cost, and the terminal inequality rows folded from 0 as v_N.
 * Tree sum over the samples: c = 64 k + l, absent lanes contribute +0.0; for m = 1, 2, 4, 8, 16, 32: v[l] = v[l] + v[l ^ m]; lane 0 holds
 *  the chunk total; chunk totals are added with k ascending, starting from chunk 0's.
 * Moments of step t: d_c[i] = x_c,t[i] - X_t[i]; m1[i] = tree(d_c[i]), dXmean = m1[i] / S; q[i][j] = tree(d_c[i] * d_c[j]) for j <= i;
 *  SX[i][j] = (q[i][j] - (m1[i] * m1[j]) / S) / (S - 1), mirrored, 0 when S == 1.  dUmean and SU likewise from the applied control minus
 *  U_t.  nviol_step[b][t] = the number of samples with v_t > viol_tol, t = 0 .. N.  With CDDP_HIP_MC_DIAG SX and SU hold the diagonals.
 * stats[b][8] = n_finite (cost and viol finite), n_viol (viol > viol_tol), cost_mean = tree(cost) / S, cost_var = tree((cost_c -
 *  cost_mean)^2) / (S - 1) (0 when S == 1), cost_min, cost_max (by <, c ascending from sample 0), viol_mean = tree(viol) / S, viol_max
 *  (as cost_max).  Non-finite values propagate; nothing is special-cased.  (The sign of an exact zero is not specified.)
 * Pointer flags (CDDP_HIP_MC_DEVICE = device pointers for every array but the factors), checks, stream ordering, tile-group offsets and the
 * handle-owned scratch are those of cddp_hip_score_rollouts.  Any output may be NULL, not all.  The handle's solver state is not modified.
 * Refused before anything is launched, each with its own message: a NULL handle or descriptor, unknown flag bits, nsamp < 1, nsamp > 1024,
 * a NaN viol_tol, a non-finite factor entry, every output NULL, an MSIPDDP handle, a handle or plant cddp_hip_track_plan would refuse, and
 * with CDDP_HIP_MC_DEVICE a pointer cddp_hip_get_field_device would refuse.  (New entry points; ABI version unchanged.) */
typedef struct cddp_hip_mc_desc {
  uint64_t seed;
  uint32_t stream;
  int32_t nsamp;                       /* S, 1 .. 1024 */
  int32_t keep_nominal;                /* nonzero: sample 0 draws z = 0 everywhere */
  int32_t _pad;
  double viol_tol;
  const double *L0, *Lw, *Lu;          /* host; [nx][nx], [nx][nx], [nu][nu]; any may be NULL */
} cddp_hip_mc_desc;                    /* 56 bytes */
enum { CDDP_HIP_MC_DEVICE = 1, CDDP_HIP_MC_DIAG = 2 };
int cddp_hip_mc_sample_noise(cddp_hip_handle *h, int flags, const cddp_hip_mc_desc *desc, double *Z0 /* [B][S][nx] or NULL */,
                             double *E /* [B][S][N][nu] or NULL */, double *Wn /* [B][S][N][nx] or NULL */);
int cddp_hip_plan_montecarlo(cddp_hip_handle *h, cddp_hip_plant *plant /* or NULL */, int flags, const cddp_hip_mc_desc *desc,
                             const double *x0 /* [B][nx] or NULL = row 0 of the live plan */,
                             double *cost /* [B][S] */, double *viol /* [B][S] */, double *stats /* [B][8] */,
                             int32_t *nviol_step /* [B][N+1] */, double *dXmean /* [B][N+1][nx] */,
                             double *SX /* [B][N+1][nx][nx] | DIAG [B][N+1][nx] */, double *dUmean /* [B][N][nu] */,
                             double *SU /* [B][N][nu][nu] | DIAG [B][N][nu] */, double *X_out /* [B][S][N+1][nx] */,
                             double *U_out /* [B][S][N][nu] */);   /* any output may be NULL, not all */

/* ---- Monte-Carlo evaluation of a solved plan under output feedback ------------------------
 * The nonlinear check of an LQG design made with cddp_hip_plan_tvlqr and cddp_hip_plan_kalman: does it hold on the true plant with the
 * actuator box, is the filter consistent there (is the sample covariance of the estimation error Sf_t), how often is a constraint row
 * violated when the controller sees only y_t?  cddp_hip_plan_montecarlo_of is cddp_hip_plan_montecarlo with a linearised Kalman estimator
 * carried in every lane (csrc/inst_mcof.hip: the same workgroup per trajectory and lane per sample): the feedback acts on the estimate, the
 * moments of the estimation error are reduced with the state's.  cddp_hip_mc_sample_meas_noise writes the measurement noise itself.
 * csrc/plan_mcof.hpp is the normative statement of what is new (host and device compile it), restated here; everything else is the section
 * above, line for line.  -ffp-contract=off, every sum starts at the stated value and runs with the index ascending, true division.
 * Sensors: y_t = C dx_t + n_t at every step t = 0 .. N before u_t is applied, cov(n_t) = diag(v): C [ny][nx] and v [ny] are row-major HOST
 *  arrays, one each for the batch, 1 <= ny <= CDDP_HIP_KF_MAX_NY.  sd[r] = sqrt(v[r]), correctly rounded, is formed on the host.
 * Gains: L [b][t][i][r], t = 0 .. N: cddp_hip_plan_kalman's L_out, or any gains; a host array, or a device array with CDDP_HIP_MC_DEVICE (it
 *  follows the pointer flag, as x0 does).  K_t, A_t, B_t are the handle's stacks at the time of the call (see cddp_hip_plan_kalman, WHICH SWEEP).
 * Normals: the measurement normal of step t, row r is element e = nx + N (nu + nx) + t ny + r of the same (seed, stream, b, c) as above: past
 *  the end of the elements of cddp_hip_plan_montecarlo, so the initial, actuator and process noise of a sample are bit for bit those of
 *  that entry (common random numbers between state and output feedback).  keep_nominal zeroes the measurement noise of sample 0 too.
 * Rollout of sample c: as above, with xh[nx], the estimate of x - X_t, next to x; xh = 0 at the start.  At every step t = 0 .. N:
 *  1. dx[j] = x[j] - X_t[j] (the value whose moments go to dXmean and SX).
 *  2. y[r] = s + n[r], with s = 0; for j ascending s += C[r][j] * dx[j], and n[r] = sd[r] * z.
 *  3. inn[r] = y[r] - p, with p = 0; for j ascending p += C[r][j] * xh[j]: every inn from the xh held before step 4 changes any of it.
 *  4. xh[i] = xh[i] + s, with s = 0; for r ascending s += L_t[i][r] * inn[r].
 *  5. e[i] = dx[i] - xh[i]: dEmean and SE by the tree sum and the moment formulas above; row t of Xh_out is xh.
 *  6. For t < N: fb[i] = s, s = 0; for j ascending s += K_t[i][j] * xh[j]; u[i] = (U_t[i] + eps[i]) + fb[i] (the line above with xh in the
 *     place of x - X_t); the plant's box, the cost, the path rows, the step(s) and the process noise exactly as above; the prediction
 *     xp[i] = s, s = 0; for j ascending s += A_t[i][j] * xh[j], then for j ascending s += B_t[i][j] * fb[j]; xh = xp.
 *     The estimator predicts with the unclipped, noise-free fb: the model of cddp_hip_plan_kalman.
 * Outputs: every output of cddp_hip_plan_montecarlo with the same shape and meaning, then dEmean [b][t][i], SE [b][t][i][j] (with
 *  CDDP_HIP_MC_DIAG [b][t][i]) and Xh_out [b][c][t][i], t = 0 .. N.  Any may be NULL, not all.  The handle's state is not modified.
 * Stream ordering: C and sd = sqrt(v) are uploaded into the handle's staging scratch by the call itself, so, unlike cddp_hip_plan_montecarlo,
 *  a CDDP_HIP_MC_DEVICE call is not fully asynchronous on the stream of cddp_hip_set_stream: it copies the two small arrays synchronously,
 *  and when the previous user of the scratch may still be running there (such as the call before it) it first waits for the group
 *  streams on the host.  The outputs are ordered on the stream as those of cddp_hip_plan_montecarlo are.
 * Not covered: nonlinear (EKF) or saturation-aware prediction, time-varying C or v, correlated measurement noise, intermittent
 *  measurements, C or factors per trajectory, an estimator inside cddp_hip_track_plan or the MPC loop, NEES or quantiles on the device
 *  (X_out and Xh_out are returned for them).
 * Refused before anything is launched, each with its own message: everything cddp_hip_plan_montecarlo refuses; ny outside
 * 1 .. CDDP_HIP_KF_MAX_NY; a NULL L, C or v; a v entry that is not finite or not > 0; a non-finite C; a non-finite host L; a handle that was
 * never solved or swept or keeps no A / B / K stacks, and an MSIPDDP handle (A_t and B_t are read); with CDDP_HIP_MC_DEVICE an L
 * cddp_hip_get_field_device would refuse.  (New entry points; ABI version unchanged.) */
typedef struct cddp_hip_mcof_desc {
  cddp_hip_mc_desc mc;                 /* seed, stream, nsamp, keep_nominal, viol_tol, L0, Lw, Lu: exactly as cddp_hip_plan_montecarlo reads them */
  int32_t ny;                          /* 1 .. CDDP_HIP_KF_MAX_NY */
  int32_t _pad;
  const double *C;                     /* host, [ny][nx], one for the batch */
  const double *v;                     /* host, [ny] measurement variances, finite and > 0 */
} cddp_hip_mcof_desc;                  /* 80 bytes */
int cddp_hip_mc_sample_meas_noise(cddp_hip_handle *h, int flags, const cddp_hip_mcof_desc *desc, double *Yn /* [B][S][N+1][ny]; C is not read */);
int cddp_hip_plan_montecarlo_of(cddp_hip_handle *h, cddp_hip_plant *plant /* or NULL */, int flags, const cddp_hip_mcof_desc *desc,
                                const double *x0 /* [B][nx] or NULL = row 0 of the live plan */,
                                const double *L /* [B][N+1][nx][ny] */,
                                double *cost /* [B][S] */, double *viol /* [B][S] */, double *stats /* [B][8] */,
                                int32_t *nviol_step /* [B][N+1] */, double *dXmean /* [B][N+1][nx] */,
                                double *SX /* [B][N+1][nx][nx] | DIAG [B][N+1][nx] */, double *dUmean /* [B][N][nu] */,
                                double *SU /* [B][N][nu][nu] | DIAG [B][N][nu] */, double *X_out /* [B][S][N+1][nx] */,
                                double *U_out /* [B][S][N][nu] */, double *dEmean /* [B][N+1][nx] */,
                                double *SE /* [B][N+1][nx][nx] | DIAG [B][N+1][nx] */,
                                double *Xh_out /* [B][S][N+1][nx] */);   /* any output may be NULL, not all */

/* ---- extended Kalman filter on the device; the MPC loop closed through it ------------
 * A cddp_hip_ekf is a device-resident extended Kalman filter for a batch of trajectories.  Its model is a cddp_hip_plant: the filter
 * uses that object's model, parameters (shared or per trajectory), integrator, dt, box, batch and device, and the plant must outlive it.
 * Sensors: y = C x + n, cov(n) = diag(v), C ny x nx with 1 <= ny <= CDDP_HIP_KF_MAX_NY (ny may exceed nx); process noise W (nx x nx) and
 * actuator noise Wu (nu x nu), either may be NULL.  The state of the object is the estimate xh [B][nx], its covariance P [B][nx][nx]
 * (kept full and symmetric), info [B] and a step count (the number of predictions since cddp_hip_ekf_reset).
 * (New entry points; ABI version unchanged; the descriptor carries its own abi_version.)
 *
 * Arithmetic (csrc/ekf.hpp; no FMA contraction; the tests are bitwise).  Every sum starts from the stated value, its index ascending.
 *  Measurement update of trajectory b, rows r = 0 .. ny-1 ascending, c = C[r]:
 *   1. h[i] = sum_j P[i][j] * c[j], from 0.0            2. s = v[r]; s += c[j] * h[j]
 *   3. m = sum_j c[j] * xh[j], from 0.0;  e = y[r] - m   4. g[i] = h[i] / s            5. xh[i] = xh[i] + g[i] * e
 *   6. for i ascending, j <= i:  q = P[i][j]; q -= g[i] * h[j]; q -= h[i] * g[j]; q += (s * g[i]) * g[j];  P[i][j] = P[j][i] = q
 *      (cddp_hip_plan_kalman's row update)              7. nis += (e * e) / s, from 0.0 at the first row
 *   With CDDP_HIP_EKF_SKIP_NAN a row whose y[r] is NaN is skipped entirely (a sensor drop-out).  A row whose s is not > 0 leaves xh and P
 *   alone and sets info = t + 1 (t: the object's step count; the first such row wins; 0 otherwise); that trajectory's xh, P and nis are NaN
 *   from that step on, in the outputs and in the object, until the next reset.  Other trajectories are unaffected.
 *  Prediction with control u:
 *   1. u_s = the plant's clip of u (cddp_hip_plant_step's line; only with a box)       2. Fx, Fu = the model's Jacobians at (params_b, xh, u_s)
 *   3. A[i][j] = h * Fx[i][j], then += 1.0 where i == j;  Bm = h * Fu -- the solver's own linearisation, discrete plants included; h = dt
 *   4. xh <- one step of the plant from (xh, u_s)
 *   5. P <- A P A^T + W + Bm Wu Bm^T, cddp_hip_plan_covariance's steps 4 and 5 with A for Acl: Y = A P; element (i, j <= i) =
 *      sum_l A[i][l] * Y[j][l] from 0.0, then += W[i][j], then += sum_k (sum_m Bm[i][m] * Wu[m][k]) * Bm[j][k]; mirrored.  Only the lower
 *      triangles of W and Wu are read.
 * Not covered: sub-stepped estimator models (the product of sub-step Jacobians), nonlinear measurement functions, correlated measurement
 *  noise, unscented or iterated filters, smoothing, an estimator inside cddp_hip_track_plan and the Monte-Carlo entries. */
typedef struct cddp_hip_ekf_desc {
  int32_t abi_version;           /* CDDP_HIP_ABI_VERSION */
  int32_t ny;                    /* 1 .. CDDP_HIP_KF_MAX_NY */
  int32_t per_trajectory;        /* 0: one C, v, W, Wu for the batch; 1: one set per trajectory, batch-major, all of them */
  int32_t _pad;
  const double *C;               /* host, [ny][nx] */
  const double *v;               /* host, [ny] measurement variances, finite and > 0 */
  const double *W;               /* host, [nx][nx] or NULL */
  const double *Wu;              /* host, [nu][nu] or NULL */
} cddp_hip_ekf_desc;             /* 48 bytes */
typedef struct cddp_hip_ekf cddp_hip_ekf;
enum { CDDP_HIP_EKF_DEVICE = 1,     /* the array arguments are device pointers of the plant's device, complete when the call is made */
       CDDP_HIP_EKF_SKIP_NAN = 2,   /* a NaN in y is a missing measurement */
       CDDP_HIP_EKF_PER_TRAJ = 4,   /* cddp_hip_ekf_reset: P0 is [B][nx][nx] */
       CDDP_HIP_EKF_DIAG = 8 };     /* cddp_hip_ekf_run: P_out holds the diagonals, [B][T+1][nx] */
/* The descriptor is checked BEFORE the device is looked at, each refusal with its own message, in this order: a NULL desc or out; wrong
 * abi_version; ny outside 1 .. CDDP_HIP_KF_MAX_NY; a NULL C or v; a NULL model plant (the checks before it need no plant, those after it
 * read its dimensions); a v entry that is not finite and > 0; a non-finite C, W or Wu; a model plant with substeps > 1.  The arrays are
 * copied.  The filter starts at xh = 0, P = 0: call cddp_hip_ekf_reset. */
int cddp_hip_ekf_create(cddp_hip_plant *model, const cddp_hip_ekf_desc *desc, cddp_hip_ekf **out);
int cddp_hip_ekf_destroy(cddp_hip_ekf *ekf);
/* Every entry below returns after its outputs are written.  Host pointers are uploaded and downloaded through the object's own scratch;
 * with CDDP_HIP_EKF_DEVICE every array must be device memory of the plant's device whose allocation holds every byte the call touches
 * (checked as cddp_hip_plan_kalman checks its device arguments).  Host inputs must be finite (y: NaN is allowed with SKIP_NAN).
 * reset: xh <- xh0, P <- the lower triangle of P0 mirrored, info <- 0, step count <- 0. */
int cddp_hip_ekf_reset(cddp_hip_ekf *ekf, int flags, const double *xh0 /* B*nx */, const double *P0 /* nx*nx, or B*nx*nx with PER_TRAJ */);
int cddp_hip_ekf_update(cddp_hip_ekf *ekf, int flags, const double *y /* B*ny */, double *nis /* B or NULL */);
int cddp_hip_ekf_predict(cddp_hip_ekf *ekf, int flags, const double *u /* B*nu */);
int cddp_hip_ekf_get(cddp_hip_ekf *ekf, int flags, double *xh /* B*nx */, double *P /* B*nx*nx */, int32_t *info /* B */);   /* any may be NULL */
/* A whole log in ONE launch from the object's current (xh, P): update with Y[:, 0]; then for t = 0 .. T-1 predict with U[:, t] and update
 * with Y[:, t+1].  The outputs are the posterior after each update and that step's nis; any may be NULL.  The object is left at the
 * final posterior.  Bitwise the loop over cddp_hip_ekf_update / cddp_hip_ekf_predict / cddp_hip_ekf_get.  T >= 0 (U may be NULL at T = 0). */
int cddp_hip_ekf_run(cddp_hip_ekf *ekf, int flags, int T, const double *Y /* [B][T+1][ny] */, const double *U /* [B][T][nu] */,
                     double *Xh_out /* [B][T+1][nx] */, double *P_out /* [B][T+1][nx][nx] | DIAG [B][T+1][nx] */,
                     double *nis_out /* [B][T+1] */, int32_t *info /* [B] */);
/* cddp_hip_mpc_run_plant with a controller that sees only y.  The true state lives in a device buffer of its own, starting at x0_true.
 * Per step k:  y = C x_k (+ Yn[:, k]), rows formed as m above, then y = m + noise;  cddp_hip_ekf_update(y);  the equivalent of
 * cddp_hip_mpc_advance(k == 0 ? CDDP_HIP_MPC_KEEP_PLAN : mode, (k == 0 ? 0 : flags) | CDDP_HIP_MPC_X_DEVICE, xh);  cddp_hip_solve;
 * x_{k+1} = plant(x_k, u_0, W[:, k]) with u_0 = row 0 of the plan;  cddp_hip_ekf_predict(u_0) -- the commanded u_0, the estimator's own
 * plant clips it;  the saturated u_0, x_{k+1}, xh_k (the posterior the solve started from), nis_k, iterations and status into the device
 * log.  W and Yn are uploaded once; only the logs cross the bus afterwards.  X_visited[:, 0] = x0_true.  flags: those of
 * cddp_hip_mpc_advance (CDDP_HIP_MPC_SHIFT_DUALS) and CDDP_HIP_MPC_EKF_SKIP_NAN (a NaN in Yn is a drop-out).  Bitwise the loop written out
 * over cddp_hip_ekf_update, cddp_hip_ekf_get, cddp_hip_mpc_advance, cddp_hip_solve, cddp_hip_get_plan_head, cddp_hip_plant_step and
 * cddp_hip_ekf_predict.  The estimator's model may differ from `plant`.  On a solve error the steps completed so far come back, as from
 * cddp_hip_mpc_run.  The first step is an advance: the handle needs a current plan (cddp_hip_set_initial and cddp_hip_initialize or
 * cddp_hip_solve), as cddp_hip_mpc_advance does.
 * Refused, with nothing launched and nothing changed: everything cddp_hip_mpc_run_plant refuses; a NULL estimator or x0_true; an
 * estimator whose nx, nu, batch or device differ from the handle's; a non-finite x0_true or W; a Yn that is not finite (NaN allowed
 * with CDDP_HIP_MPC_EKF_SKIP_NAN). */
enum { CDDP_HIP_MPC_EKF_SKIP_NAN = 256 };
int cddp_hip_mpc_run_ekf(cddp_hip_handle *h, cddp_hip_plant *plant, cddp_hip_ekf *ekf, int steps, int mode, int flags,
                         const double *x0_true /* B*nx, host */, const double *W /* B*steps*nx or NULL, host */,
                         const double *Yn /* B*(steps+1)*ny or NULL, host; rows 0 .. steps-1 are read */,
                         double *U_applied /* B*steps*nu */, double *X_visited /* B*(steps+1)*nx */, double *Xh_visited /* B*steps*nx */,
                         double *nis /* B*steps */, int32_t *iterations /* B*steps */, int32_t *status /* B*steps */,
                         cddp_hip_stats *stats_sum);

/* ---- multi-GPU: the single collective of the path --------------------------------------
 * One process (or host thread) per GPU, each with its own handle over a contiguous block of the global batch; nothing
 * is exchanged during a solve.  After it, ONE RCCL all-gather collects every trajectory's 16-byte record.
 * The communicator is the caller's ncclComm_t (passed as void*), or one made with the helpers below (RCCL is loaded
 * lazily with dlopen: the solver core has no link-time dependency on it). */
#define CDDP_HIP_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on ONE rank, hand the 128 bytes to the others by any means (MPI, TCP store, file). */
int cddp_hip_comm_unique_id(char *id_out /* CDDP_HIP_COMM_ID_BYTES */);
/* ncclCommInitRank on `device` (collective over all ranks). */
int cddp_hip_comm_init(const char *id_in, int world, int rank, int device, void **comm_out);
int cddp_hip_comm_destroy(void *comm);
/* ncclCommCount / ncclCommUserRank of the communicator: the number of ranks RCCL itself sees, and this process's rank (round 4) */
int cddp_hip_comm_info(void *comm, int *count_out, int *rank_out);
/* All-gather the records of this rank's batch into recv_device (DEVICE buffer of world * shard_capacity records,
 * rank r's block at r * shard_capacity).  shard_capacity >= every rank's batch: with an uneven block partition the
 * ranks pad to the largest shard; padding records read status = iterations = -1.  comm == NULL is valid for
 * world == 1 (device copy).  Runs on the stream given to cddp_hip_set_stream (else the handle's own) and returns when
 * the gathered buffer is complete. */
int cddp_hip_allgather_results(cddp_hip_handle *h, void *comm /* ncclComm_t */, int world, int shard_capacity,
                               void *recv_device);

/* Total path dual dimension m and terminal-equality dimension p of the handle's problem. */
int cddp_hip_dual_dim(cddp_hip_handle *h);
int cddp_hip_batch(cddp_hip_handle *h);
/* Number of tile groups the handle's batch is cut into (whole 64-trajectory tiles per group; each group has its own
 * device buffers and stream and cddp_hip_solve keeps all of them in flight).  Results do not depend on it.
 * Environment CDDP_HIP_GROUPS=n pins it at create time (1 = one stream). */
int cddp_hip_num_groups(cddp_hip_handle *h);
/* How many of those groups cddp_hip_solve keeps in flight AT ONCE (round 5).  1: the groups (chunks of a large batch) are solved one
 * after the other.  2: the static CU partition of IPDDP / CLDDP batches of >= 32 tiles -- two groups, each with every kernel of its
 * iterations on its own symmetric half of the chip (streams made with hipExtStreamCreateWithCUMask), so one "launch" of a kernel
 * class in the timing model is the two concurrent half-batch launches.  No reference counterpart (the reference solves one problem). */
int cddp_hip_concurrency(cddp_hip_handle *h);

/* ---- stack-fed mode (host plugins) ---------------------------------------
 * Arbitrary DynamicalSystem / Objective / Constraint subclasses (e.g. the user-defined QuadraticScalarSystem of
 * tests/cddp_core/test_ipddp_solver.cpp:291-346) cannot run on the GPU.  In stack-fed mode the caller evaluates them
 * on the host and hands over the (N x batch) derivative stacks the reference precomputes per backward pass
 * (cddp_solver_base.cpp:319-394, ipddp_solver.cpp:2145-2250); the GPU runs the backward pass on them.  The forward
 * rollout needs the plugin's f(x, u) and therefore stays with the host.
 * A stack handle owns its device buffers: upload the stacks of an iterate once, sweep (one launch), read the results.
 * Layout: batch-major host arrays, fx[b][t][i][j] = A_t = I + dt*f_x, fu[b][t][i][j] = B_t = dt*f_u,
 * lx[b][t][i], lu[b][t][j], lxx[b][t][i][i'], luu[b][t][j][j'], lux[b][t][j][i]; VxN[b][i], VxxN[b][i][i'] = terminal cost
 * gradient / Hessian; path constraints stacked in std::map (name) order: y, s, g [b][t][r] (g = evaluate - upper bound),
 * Gx[b][t][r][i], Gu[b][t][r][j]. */
typedef struct cddp_hip_stack_handle cddp_hip_stack_handle;
enum cddp_hip_stacks_branch {
  CDDP_HIP_STACKS_CLDDP = 0,      /* clddp_solver.cpp:79-204 without control bounds                    */
  CDDP_HIP_STACKS_IPDDP = 1,      /* ipddp_solver.cpp:1048-1118 (no constraints)                       */
  CDDP_HIP_STACKS_IPDDP_PATH = 2, /* ipddp_solver.cpp:1355-1568 (path constraints; handle with m > 0)  */
  CDDP_HIP_STACKS_MSIPDDP = 4,    /* msipddp_solver.cpp:1112-1208 (no constraints): IPDDP recursion + defect stack (cddp_hip_set_defect_stack) */
  CDDP_HIP_STACKS_MSIPDDP_PATH = 5, /* msipddp_solver.cpp:1222-1420 (path constraints; handle with m > 0, defect stack): the condensation with
                                     plain y / s ratios (no slack floor, no clipping), Q_ux updated as :1398 writes it -- nu = 1 or nx = nu
                                     only --, no linear-policy rollout / step caps */
  CDDP_HIP_STACKS_IPDDP_TERM_EQ = 6, /* ipddp_solver.cpp:1120-1353, 413-639: the reduced LQR with terminal-equality rows.  The stacks carry the LQ
                                   * model the reference builds at :1143-1245 (fx = A, fu = B, lx = q, lu = r, lxx = Q, luu = R WITHOUT the
                                   * regularisation, lux = M as nx x nu, VxN = q_N, VxxN = Q_N; path constraints condensed by the caller) and
                                   * cddp_hip_set_terminal_equality the dense H_T, b_T = -h_T, previous multipliers (handle with m = 0) */
  CDDP_HIP_STACKS_LOGDDP = 3      /* logddp_solver.cpp:470-575: the caller folds the relaxed log barrier's gradients / Hessians (barrier.hpp:95-262)
                                     into lx, lu, lxx, luu, lux; handle with m = 0                     */
};
/* ABI 5: cddp_hip_stacks_backward copies a cddp_hip_options from a caller pointer, so the handle is created against a stated ABI
 * version and options size; C / C++ callers use the macro below, which passes the values of the header they compile against;
 * other bindings pass their own.  A mismatch is refused. */
int cddp_hip_stacks_create_abi(int abi_version, int options_bytes, int device, int batch, int nx, int nu,
                               int m /* total path dual dim, 0 = none */, int horizon, cddp_hip_stack_handle **out);
#define cddp_hip_stacks_create(device, batch, nx, nu, m, horizon, out) \
  cddp_hip_stacks_create_abi(CDDP_HIP_ABI_VERSION, (int)sizeof(cddp_hip_options), (device), (batch), (nx), (nu), (m), (horizon), (out))
int cddp_hip_stacks_destroy(cddp_hip_stack_handle *h);
/* Upload the dynamics / cost stacks of the current iterate.  The first call must supply all of them; later calls may
 * pass NULL for stacks that did not change (e.g. constant cost Hessians). */
int cddp_hip_set_stacks(cddp_hip_stack_handle *h, const double *fx, const double *fu, const double *lx, const double *lu,
                        const double *lxx, const double *luu, const double *lux, const double *VxN, const double *VxxN);
/* Multiple-shooting defects d[b][t] = f(x_t, u_t) - x_{t+1} (nx each) for CDDP_HIP_STACKS_MSIPDDP: Q_x and Q_u are formed with
 * V_x + V_xx d_t (msipddp_solver.cpp:1144-1145).  The caller derives k_lambda[t] = -lambda_t + V_x(t+1) + V_xx(t+1) d_t and
 * K_lambda[t] = V_xx(t+1) (:1192-1194) from the returned value stacks.  NULL drops the stack. */
int cddp_hip_set_defect_stack(cddp_hip_stack_handle *h, const double *defects);
/* Control limits of the CLDDP branch (the constraint named "ControlConstraint", clddp_solver.cpp:85-86, 147-178): every step
 * solves the BoxQP  min 0.5 k^T Q_uu_reg k + Q_u^T k,  lower - u_t <= k <= upper - u_t  (boxqp.cpp:25-250, parameters from
 * options.boxqp_*), warm-started with the k_t of the handle's previous sweep, and the feedback gain lives on the free
 * directions.  lower / upper: nu each; U: the current controls, batch-major [b][t][nu].  The first call supplies all three;
 * later calls may pass NULL bounds to keep them (U changes every iteration); three NULLs remove the box. */
int cddp_hip_set_control_box(cddp_hip_stack_handle *h, const double *lower, const double *upper, const double *U);
/* Full DDP (options.use_ilqr = false) for host plug-ins: the dynamics Hessian tensors of the current iterate, as the reference
 * keeps them in F_xx_ / F_uu_ / F_ux_ (cddp_solver_base.cpp:346-356) but ALREADY multiplied by dt -- Fxx[b][t][i] (nx x nx),
 * Fuu[b][t][i] (nu x nu), Fux[b][t][i] (nu x nx), i = output row of f.  The IPDDP and LogDDP branches then add V_x(i) times
 * them to Q_xx, Q_uu, Q_ux (ipddp_solver.cpp:1070-1082, 1396-1408; logddp_solver.cpp:505-515); the reference's CLDDP backward pass
 * has no such terms and cddp_hip_stacks_backward refuses that combination.  Three NULLs return to Gauss-Newton. */
int cddp_hip_set_hessian_stacks(cddp_hip_stack_handle *h, const double *Fxx, const double *Fuu, const double *Fux);
/* MSIPDDP's per-step factor cache (msipddp_solver.cpp:1169-1185, unconstrained branch): the reference keeps one LDLT of
 * sym(Q_uu) + reg I per step and refactors a step only while its cached factor is invalid, so from the second sweep of a solve on
 * every step is solved with the matrix of its FIRST sweep.  enable != 0 allocates (first call) and CLEARS the cache: call it at
 * the start of each solve; the CDDP_HIP_STACKS_MSIPDDP branch then factors the cached matrix of a step where there is one and
 * caches the one it factored where there was none.  enable == 0 (the default of a new handle): every sweep factors its own. */
int cddp_hip_stacks_factor_cache(cddp_hip_stack_handle *h, int enable);
/* Upload the condensation inputs of the path-constrained branch (same NULL rule). */
int cddp_hip_set_constraint_stacks(cddp_hip_stack_handle *h, const double *y, const double *s, const double *g,
                                   const double *Gx, const double *Gu);
/* One backwardPass on the uploaded stacks.  reg[b] = context.regularization_ per trajectory; mu[b] = barrier parameter
 * (path branch; NULL otherwise); retry != 0 adds the "increase regularisation and retry" loop of
 * cddp_solver_base.cpp:93-111 (options->reg_update_factor / reg_max_value).  ok[b] (optional) = 1 where the sweep succeeded. */
int cddp_hip_stacks_backward(cddp_hip_stack_handle *h, int branch, const cddp_hip_options *options, const double *reg,
                             const double *mu, int retry, int32_t *ok);
/* hipEvent time of the last sweep launch [ms]. */
double cddp_hip_stacks_last_kernel_ms(cddp_hip_stack_handle *h);
/* Form of the last sweep launch: 0 = one lane per trajectory, 1 = lane-cooperative (sixteen lanes per trajectory, step state in
 * LDS: the default for nx > 8; CDDP_HIP_STACKS_SWEEP=lane|coop overrides where both forms are instantiated).  Bitwise the same
 * results either way. */
int cddp_hip_stacks_last_sweep_form(cddp_hip_stack_handle *h);
/* K (B*N*nu*nx), k (B*N*nu), Vx (B*(N+1)*nx), Vxx (B*(N+1)*nx*nx), dV (B*2); any may be NULL. */
int cddp_hip_stacks_get_gains(cddp_hip_stack_handle *h, double *K, double *k, double *Vx, double *Vxx, double *dV);
/* Path branch: k_y, k_s (B*N*m), K_y, K_s (B*N*m*nx) and the linear-policy rollout dX (B*(N+1)*nx), ipddp_solver.cpp:1458-1520. */
int cddp_hip_stacks_get_constraint_gains(cddp_hip_stack_handle *h, double *k_y, double *K_y, double *k_s, double *K_s, double *dX);
/* Per-trajectory scalars of the sweep (B each, any may be NULL): regularisation used, inf_du, inf_pr, inf_comp, step_norm
 * and computeMaxStepSizes' (alpha_pr_max, alpha_du_max) (ipddp_solver.cpp:2939-2988; 1 without path constraints). */
int cddp_hip_stacks_get_scalars(cddp_hip_stack_handle *h, double *reg, double *inf_du, double *inf_pr, double *inf_comp,
                                double *step_norm, double *alpha_pr_max, double *alpha_du_max);
/* Terminal-equality branch (CDDP_HIP_STACKS_IPDDP_TERM_EQ; ipddp_solver.cpp:478-639): H_T [B][pT][nx] = the stacked terminal-equality
 * Jacobian (dense rows), b_T [B][pT] = -h_T(x_N), lambda_prev [B][pT] = Lambda_T_eq_ of the iterate, reg_floor [B] = max(1e-10,
 * options.ipddp.jacobian_regularization_value * pow(max(mu, 0), jacobian_regularization_exponent)) evaluated by the caller (:577-578: the
 * plug-in route keeps the host's elementary functions).  1 <= pT <= 8; handle created with m = 0. */
int cddp_hip_set_terminal_equality(cddp_hip_stack_handle *h, int pT, const double *H_T, const double *b_T, const double *lambda_prev,
                                   const double *reg_floor);
/* Results of the terminal-equality sweep: lambda_delta = dLambda_T_eq_ (B*pT) and the linear-policy rollout dX (B*(N+1)*nx) of the
 * recombined gains (:1252-1268); K, k, Vx (= k_lambda), Vxx (= K_lambda) come through cddp_hip_stacks_get_gains, the regularisation used,
 * inf_du and step_norm through cddp_hip_stacks_get_scalars.  Either may be NULL. */
int cddp_hip_stacks_get_terminal(cddp_hip_stack_handle *h, double *lambda_delta, double *dX);
/* One-shot unconstrained form (create + upload + one launch + download + destroy): Gauss-Newton sweep of
 * ipddp_solver.cpp:1048-1118 when reg_in_value != 0, clddp_solver.cpp:79-204 without bounds otherwise, scalar `reg`. */
int cddp_hip_backward_stacks(int device, int batch, int nx, int nu, int horizon,
                             const double *fx, const double *fu, const double *lx,
                             const double *lu, const double *lxx, const double *luu,
                             const double *lux, const double *VxN, const double *VxxN,
                             double reg, int reg_in_value, double *K, double *k, double *Vx,
                             double *Vxx, double *dV, int32_t *ok, double *kernel_ms);

/* ---- host plug-in solve (north_star: "keeps cddp-cpp's DynamicsModel / Constraint / Objective plugin surface") ----------------
 * CDDP::solve() for problems whose DynamicalSystem / Objective / Constraint objects are arbitrary HOST subclasses (the reference's
 * QuadraticScalarSystem of tests/cddp_core/test_ipddp_solver.cpp:291-346, Python plug-ins of python/tests/test_custom_dynamics.py,
 * NonlinearObjective subclasses ...).  The callbacks are the reference's virtual functions, flattened to plain pointers:
 *   discrete_dynamics            DynamicalSystem::getDiscreteDynamics(x, u, t)                       (dynamical_system.hpp)
 *   jacobians                    getStateJacobian / getControlJacobian: CONTINUOUS-time f_x (nx x nx), f_u (nx x nu), row-major;
 *                                the library forms A = I + dt f_x, B = dt f_u (cddp_solver_base.cpp:340-344)
 *   hessians                     getStateHessian / getControlHessian / getCrossHessian (needed iff options.use_ilqr == 0):
 *                                fxx[i] (nx x nx), fuu[i] (nu x nu), fux[i] (nu x nx), i = output row of f; or NULL
 *   running_cost, terminal_cost  Objective::running_cost(x, u, index), terminal_cost(x_N)           (objective.hpp)
 *   running_cost_derivatives     l_x (nx), l_u (nu), l_xx (nx x nx), l_uu (nu x nu), l_ux (nu x nx)
 *   terminal_cost_derivatives    getFinalCostGradient (nx), getFinalCostHessian (nx x nx)
 *   constraints                  the path-constraint set, stacked in std::map (name) order: g = evaluate(x, u) - getUpperBound()
 *                                (m rows), getStateJacobian (m x nx), getControlJacobian (m x nu); gx / gu may be NULL when only g
 *                                is wanted.  n_constraints objects of constraint_dims[] rows each (the reference sums the
 *                                barrier / violation terms constraint by constraint, ipddp_solver.cpp:2778-2937).
 *   control_lower / control_upper  CLDDP only: the bounds of the constraint literally named "ControlConstraint"
 *                                (clddp_solver.cpp:85-86, 147-178, 227-228) or NULL; CLDDP ignores every other constraint.
 * The GPU runs the backward pass of the whole batch (stack-fed sweeps above); the forward pass needs the plug-in's f(x, u) and runs
 * on the host (csrc/plugin_solve.hip).  All trajectories of the batch share the plug-in; they differ in x0 / U0 / X0.  Callbacks are
 * called from the calling thread only unless cddp_hip_plugin_set_host_threads says otherwise.  Terminal constraints: cddp_hip_plugin_solve_terminal
 * below.  Warm starts: a stateless call can only take the "provided trajectory" branch; the terminal entry point implements it.
 * solver = CDDP_HIP_SOLVER_LOGDDP runs the reference's LogDDP (logddp_solver.cpp:43-707: single shooting, relaxed log barrier of every
 * path constraint folded into the cost derivatives on the host, Riccati sweep of the batch on the GPU, filter line search on the
 * host); it takes the same callbacks, plus constraint_hessians when a constraint has curvature. */
/* Host evaluation of a BUILT-IN plant (the kernels' own model source compiled for the host, csrc/host_models.cpp): the reference's
 * DynamicalSystem::getDiscreteDynamics (x_next), getStateJacobian / getControlJacobian (continuous-time f_x nx*nx, f_u nx*nu,
 * row-major) and getStateHessian / getControlHessian / getCrossHessian (fxx[i] nx*nx, fuu[i] nu*nu, fux[i] nu*nx per state row i;
 * the three come together) for one (x, u).  Any output may be NULL.  This is what lets a built-in plant be paired with a user
 * Objective / Constraint in the plug-in solve below (the reference's car-parking test has exactly that shape).  model_params:
 * CDDP_HIP_MAX_MODEL_PARAMS doubles as in cddp_hip_problem.  LTI plants are not served here (x+ = A x + B u is the caller's). */
int cddp_hip_model_eval(int model /* cddp_hip_model */, int integrator /* cddp_hip_integrator */, double dt, const double *model_params,
                        int nx, int nu, const double *x, const double *u, double *x_next, double *fx, double *fu,
                        double *fxx, double *fuu, double *fux);

#define CDDP_HIP_PLUGIN_MAX_CONSTRAINTS 8
typedef struct cddp_hip_plugin {
  /* ABI 5: the entry point copies a cddp_hip_options from a caller pointer, so the caller states which layout it was built against
   * (cddp_hip_create has checked cddp_hip_problem::abi_version since round 2; this struct and the stack handles did not).  Set
   * abi_version = CDDP_HIP_ABI_VERSION and options_bytes = sizeof(cddp_hip_options); a mismatch is refused. */
  int32_t abi_version, options_bytes;
  /* Optional (may be NULL): a word the caller sets non-zero to stop the solve -- e.g. a binding whose callback raised an exception.
   * Checked once per outer iteration and after every batch of callbacks; cddp_hip_plugin_solve then returns -50. */
  const volatile int32_t *abort_flag;
  void *user;
  int32_t nx, nu;
  int32_t n_constraints;
  int32_t constraint_dims[CDDP_HIP_PLUGIN_MAX_CONSTRAINTS];
  void (*discrete_dynamics)(void *user, const double *x, const double *u, double time, double *x_next);
  void (*jacobians)(void *user, const double *x, const double *u, double time, double *fx, double *fu);
  void (*hessians)(void *user, const double *x, const double *u, double time, double *fxx, double *fuu, double *fux);
  double (*running_cost)(void *user, const double *x, const double *u, int index);
  double (*terminal_cost)(void *user, const double *x);
  void (*running_cost_derivatives)(void *user, const double *x, const double *u, int index, double *lx, double *lu, double *lxx, double *luu, double *lux);
  void (*terminal_cost_derivatives)(void *user, const double *x, double *lx, double *lxx);
  void (*constraints)(void *user, const double *x, const double *u, int index, double *g, double *gx, double *gu);
  const double *control_lower, *control_upper;
  /* LogDDP only (may be NULL): second derivatives of the m stacked constraint rows, gxx[r] (nx x nx), guu[r] (nu x nu), gux[r] (nu x nx),
   * Constraint::getHessians; rows of constraints that provide none (or throw std::logic_error in the reference) stay zero.  They
   * enter the relaxed log barrier's Hessian (barrier.hpp:137-213). */
  void (*constraint_hessians)(void *user, const double *x, const double *u, int index, double *gxx, double *guu, double *gux);
} cddp_hip_plugin;
/* ISolverAlgorithm::initialize + solve for `batch` trajectories of a host plug-in problem.  x0: batch*nx; U0: batch*N*nu or NULL
 * (zeros); X0: batch*(N+1)*nx or NULL (x0 replicated).  results: batch records; X (batch*(N+1)*nx), U (batch*N*nu), K
 * (batch*N*nu*nx, feedback gains of the last sweep) may be NULL. */
/* Terminal constraints of a plug-in problem (round 6; CDDP::addTerminalConstraint, cddp_core.cpp:173-179).  Only IPDDP reads them
 * (ipddp_solver.cpp:84-215): objects in std::map (name) order, each either a terminal EQUALITY (TerminalEqualityConstraint: residual
 * h(x_N), rows stacked into H_T / Lambda_T_eq) or a terminal INEQUALITY (TerminalInequalityConstraint: residual g_T(x_N) <= 0 with slack /
 * dual S_T, Y_T).  evaluate returns the residual rows of ALL objects stacked in that order (sum of dims) and, when rx != NULL, their state
 * Jacobian rows (sum of dims x nx, row-major).  At most 8 equality rows in total. */
typedef struct cddp_hip_plugin_terminal {
  int32_t n_terminal;
  int32_t dims[CDDP_HIP_PLUGIN_MAX_CONSTRAINTS];
  int32_t equality[CDDP_HIP_PLUGIN_MAX_CONSTRAINTS];   /* 1 = equality, 0 = inequality */
  void (*evaluate)(void *user, const double *x_terminal, double *r, double *rx);   /* user = cddp_hip_plugin::user */
} cddp_hip_plugin_terminal;
/* cddp_hip_plugin_solve with a terminal set.  The Riccati work stays on the GPU: with terminal-equality rows the reduced LQR of
 * ipddp_solver.cpp:478-639, 1120-1353 (CDDP_HIP_STACKS_IPDDP_TERM_EQ; the host condenses the path constraints into its LQ stacks as :1143-1245
 * does), otherwise the ordinary stack-fed sweeps on the terminal value with the terminal-inequality barrier terms (:1000-1031).
 * options.warm_start: the "warm start with provided trajectory" initialisation (:733-816) from (x0, U0).  terminal_out (optional):
 * per trajectory [S_T (inequality rows) | Y_T | Lambda_T_eq (equality rows)].  terminal == NULL or n_terminal == 0: cddp_hip_plugin_solve. */
int cddp_hip_plugin_solve_terminal(const cddp_hip_plugin *plugin, const cddp_hip_plugin_terminal *terminal, int solver /* cddp_hip_solver */,
                                   int horizon, double dt, const cddp_hip_options *options, int device, int batch, const double *x0,
                                   const double *U0, const double *X0, cddp_hip_result *results, double *X, double *U, double *K,
                                   double *terminal_out);
/* Host threads that run the per-trajectory host work of cddp_hip_plugin_solve's IPDDP / CLDDP loop (derivative fill, forward passes, updates;
 * the reference fans its own line search out with std::async, cddp_solver_base.cpp:264-314).  Default 1: callbacks on the calling thread
 * only.  n > 1 (0 = one per hardware thread): the plug-in's callbacks are called CONCURRENTLY for different trajectories -- for thread-safe
 * plug-ins.  Process-wide; CDDP_HIP_PLUGIN_THREADS is the default when this was never called.  Results do not depend on the count. */
int cddp_hip_plugin_set_host_threads(int n);
/* Time split of this process's LAST plug-in solve, any solver, with or without terminal constraints (any output may be NULL): wall ms of
 * its outer loop, of its GPU sections (stack upload + sweep launch + gain download), the sweeps' kernel ms (hipEvents), batch sweeps
 * launched, host threads used. */
int cddp_hip_plugin_last_stats(double *total_ms, double *gpu_section_ms, double *kernel_ms, int *sweeps, int *threads);
int cddp_hip_plugin_solve(const cddp_hip_plugin *plugin, int solver /* cddp_hip_solver */, int horizon, double dt,
                          const cddp_hip_options *options, int device, int batch, const double *x0, const double *U0, const double *X0,
                          cddp_hip_result *results, double *X, double *U, double *K);

#ifdef __cplusplus
}
#endif
#endif /* CDDP_HIP_H */
