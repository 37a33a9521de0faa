// Host evaluation of the built-in plants: dev_models.hpp (the source the kernels compile for gfx950) compiled for the host.
//
// Why: the plug-in solve (plugin_solve.hip) runs its forward passes on the host through the DynamicalSystem callbacks.  A problem
// that pairs a BUILT-IN plant with a user Objective / Constraint subclass -- the shape of the reference's own car-parking and
// NonlinearObjective tests (tests/cddp_core/test_ipddp_solver.cpp:628-885, python/tests/test_nonlinear_objective.py) -- needs
// DynamicalSystem::getDiscreteDynamics / getStateJacobian / ... of that plant on the host.  One source, two targets: no second
// restatement to drift.  (The CPU checker under the repo's test tree has its own, independently written plants; the tests compare.)
//
// Built with g++ -ffp-contract=off (Makefile); sin / cos are the host libm's by default, the shared straight-line routines under
// CDDP_TRIG_SHARED -- the same switch as the device objects of the same library.
#define CDDP_HOST_MODELS 1
#define CDDP_TRIG_HOST 1
#define DEV inline
#include "dev_models.hpp"

#include <cmath>
#include <string>

namespace {
using namespace cddp_dev;

template <class Model, bool H = Model::kHasHess> struct HessOf {
  static bool run(const double *p, const double *x, const double *u, double *fxx, double *fuu, double *fux) { Model::hess(p, x, u, fxx, fuu, fux); return true; }
};
template <class Model> struct HessOf<Model, false> {
  static bool run(const double *, const double *, const double *, double *, double *, double *) { return false; }
};

template <class Model>
int eval(int integrator, double dt, const double *params, int nx, int nu, const double *x, const double *u, double *x_next, double *fx, double *fu,
         double *fxx, double *fuu, double *fux, std::string &err) {
  if (nx != Model::NX || nu != Model::NU) { err = "model dimensions do not match the plant"; return -2; }
  double p[32];
  for (int i = 0; i < 32; ++i) p[i] = i < CDDP_HIP_MAX_MODEL_PARAMS ? params[i] : 0.0;
  if (x_next) Stepper<Model>::step(integrator, dt, p, x, u, x_next);
  if (fx || fu) {
    double Fx[Model::NX * Model::NX], Fu[Model::NX * Model::NU];
    Model::jac(p, x, u, Fx, Fu);
    if (fx) for (int i = 0; i < Model::NX * Model::NX; ++i) fx[i] = Fx[i];
    if (fu) for (int i = 0; i < Model::NX * Model::NU; ++i) fu[i] = Fu[i];
  }
  if (fxx || fuu || fux) {
    if (!fxx || !fuu || !fux) { err = "Hessian outputs come as a triple"; return -2; }
    if (!HessOf<Model>::run(p, x, u, fxx, fuu, fux)) { err = "this plant has no Hessian tensors (options.use_ilqr = 0 is not available for it)"; return -3; }
  }
  return 0;
}
}  // namespace

// C++ linkage, called by capi.hip from both flatten() (device descriptor) and cddp_hip_model_eval: the parameter block the plants read.
// Checks the dimensions of the spacecraft plants and, for the attitude plants, appends I^-1 to the inertia matrix (p[9..17]) as Eigen's
// fixed-size 3 x 3 inverse() computes it in their constructors: cofactors times 1 / det.  Usv3Dof: the whole block (M^-1 by the same
// inverse, D_L, the three effective masses) from the reference's fixed vessel (usv_3dof.cpp:17-48).  Forklift: no timestep here (the
// callers that know dt write p[3], as for the car's p[1]).
namespace {
// Eigen's fixed-size 3 x 3 inverse: cofactors times 1 / det; false when the matrix has none
bool inverse3_cofactor(const double *M, double *out, double *det_out) {
  double C[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      C[3 * i + j] = M[3 * i1 + j1] * M[3 * i2 + j2] - M[3 * i1 + j2] * M[3 * i2 + j1];
    }
  const double det = (M[0] * C[0] + M[1] * C[1]) + M[2] * C[2];
  const double invdet = 1.0 / det;
  *det_out = det;
  if (det == 0.0 || !std::isfinite(invdet)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = C[3 * j + i] * invdet;
  return true;
}
}  // namespace

int cddp_host_model_params(int model, int nx, int nu, const double *in, double *out, std::string &err) {
  for (int i = 0; i < CDDP_HIP_MAX_MODEL_PARAMS; ++i) out[i] = in[i];
  static const struct { int model, nx, nu; const char *name; } dims[] = {
      {CDDP_HIP_MODEL_EULER_ATTITUDE, 6, 3, "EulerAttitude"}, {CDDP_HIP_MODEL_QUATERNION_ATTITUDE, 7, 3, "QuaternionAttitude"},
      {CDDP_HIP_MODEL_MRP_ATTITUDE, 6, 3, "MrpAttitude"}, {CDDP_HIP_MODEL_SPACECRAFT_TWOBODY, 6, 3, "SpacecraftTwobody"},
      {CDDP_HIP_MODEL_SPACECRAFT_LANDING2D, 6, 2, "SpacecraftLanding2D"}, {CDDP_HIP_MODEL_DUBINS_CAR, 3, 1, "DubinsCar"},
      {CDDP_HIP_MODEL_DREYFUS_ROCKET, 2, 1, "DreyfusRocket"}, {CDDP_HIP_MODEL_ACROBOT, 4, 1, "Acrobot"}, {CDDP_HIP_MODEL_USV_3DOF, 6, 3, "Usv3Dof"},
      {CDDP_HIP_MODEL_FORKLIFT, 5, 2, "Forklift"}, {CDDP_HIP_MODEL_SPACECRAFT_LINEAR_FUEL, 8, 3, "SpacecraftLinearFuel"},
      {CDDP_HIP_MODEL_QUADROTOR_RATE, 10, 4, "QuadrotorRate"}, {CDDP_HIP_MODEL_SPACECRAFT_NONLINEAR, 10, 3, "SpacecraftNonlinear"}};
  for (const auto &d : dims) {
    if (d.model != model) continue;
    if (nx != d.nx || nu != d.nu) {
      err = std::string(d.name) + " has nx = " + std::to_string(d.nx) + ", nu = " + std::to_string(d.nu) + " (got nx = " + std::to_string(nx) +
            ", nu = " + std::to_string(nu) + ")";
      return -2;
    }
  }
  if (model == CDDP_HIP_MODEL_EULER_ATTITUDE || model == CDDP_HIP_MODEL_QUATERNION_ATTITUDE || model == CDDP_HIP_MODEL_MRP_ATTITUDE) {
    double det;
    if (!inverse3_cofactor(in, out + 9, &det)) { err = "the inertia matrix is singular (det = " + std::to_string(det) + "): it has no inverse"; return -2; }
  }
  if (model == CDDP_HIP_MODEL_QUADROTOR_RATE) {   // the constructor's checks and messages (quadrotor_rate.cpp:28-36)
    if (!(in[0] > 0.0)) { err = "Mass must be positive"; return -2; }
    if (!(in[1] > 0.0)) { err = "Maximum thrust must be positive"; return -2; }
    if (!(in[2] > 0.0)) { err = "Maximum angular rate must be positive"; return -2; }
  }
  if (model == CDDP_HIP_MODEL_USV_3DOF) {
    const double m = 100.0, Iz = 10.0, X_udot = -10.0, Y_vdot = -50.0, Y_rdot = -5.0, N_vdot = -5.0, N_rdot = -5.0;
    const double X_u = -20.0, Y_v = -100.0, Y_r = 0.0, N_v = 0.0, N_r = -20.0;
    const double M[9] = {m + -X_udot, 0.0, 0.0, 0.0, m + -Y_vdot, 0.0 + -Y_rdot, 0.0, 0.0 + -N_vdot, Iz + -N_rdot};
    const double D[9] = {-X_u, 0.0, 0.0, 0.0, -Y_v, -Y_r, 0.0, -N_v, -N_r};
    double det;
    for (int i = 0; i < CDDP_HIP_MAX_MODEL_PARAMS; ++i) out[i] = 0.0;
    if (!inverse3_cofactor(M, out, &det)) { err = "Usv3Dof: singular mass matrix"; return -2; }
    for (int i = 0; i < 9; ++i) out[9 + i] = D[i];
    out[18] = m - X_udot; out[19] = m - Y_vdot; out[20] = -Y_rdot;
  }
  return 0;
}

// C++ linkage: called from capi.hip (cddp_hip_model_eval), which owns the error string
int cddp_host_model_eval(int model, int integrator, double dt, const double *params, int nx, int nu, const double *x, const double *u, double *x_next,
                         double *fx, double *fu, double *fxx, double *fuu, double *fux, std::string &err) {
  if (integrator < CDDP_HIP_EULER || integrator > CDDP_HIP_RK4) { err = "Integration type not supported!"; return -2; }
  switch (model) {
    case CDDP_HIP_MODEL_PENDULUM: return eval<PendulumModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_CARTPOLE: return eval<CartPoleModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_UNICYCLE: return eval<UnicycleModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_QUADROTOR: return eval<QuadrotorModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_QUADROTOR_EULER12: return eval<Quad12Model>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_MANIPULATOR: return eval<ManipulatorModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_MANIPULATOR7: return eval<Manip7Model>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_BICYCLE: return eval<BicycleModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_HCW: return eval<HCWModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_EULER_ATTITUDE: return eval<EulerAttitudeModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_QUATERNION_ATTITUDE: return eval<QuaternionAttitudeModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_MRP_ATTITUDE: return eval<MrpAttitudeModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_SPACECRAFT_TWOBODY:
      if (fxx || fuu || fux) { err = SpacecraftTwobodyModel::kNoHessMsg; return -3; }
      return eval<SpacecraftTwobodyModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_SPACECRAFT_LANDING2D: return eval<SpacecraftLanding2DModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_DUBINS_CAR: return eval<DubinsCarModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_DREYFUS_ROCKET: return eval<DreyfusRocketModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_ACROBOT: return eval<AcrobotModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_USV_3DOF: return eval<Usv3DofModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_SPACECRAFT_LINEAR_FUEL: return eval<SpacecraftLinearFuelModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_QUADROTOR_RATE: return eval<QuadrotorRateModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_SPACECRAFT_NONLINEAR:
      if (fxx || fuu || fux) { err = SpacecraftNonlinearModel::kNoHessMsg; return -3; }
      return eval<SpacecraftNonlinearModel>(integrator, dt, params, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    case CDDP_HIP_MODEL_FORKLIFT: {   // discrete, as the car: the timestep travels as params[3]
      double pc[CDDP_HIP_MAX_MODEL_PARAMS];
      for (int i = 0; i < CDDP_HIP_MAX_MODEL_PARAMS; ++i) pc[i] = params[i];
      pc[3] = dt;
      return eval<ForkliftModel>(integrator, dt, pc, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    }
    case CDDP_HIP_MODEL_CAR: {   // a discrete plant: its step needs the timestep, which travels as params[1] (as in the device descriptor)
      double pc[CDDP_HIP_MAX_MODEL_PARAMS];
      for (int i = 0; i < CDDP_HIP_MAX_MODEL_PARAMS; ++i) pc[i] = params[i];
      pc[1] = dt;
      return eval<CarModel>(integrator, dt, pc, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
    }
    default: err = "no host evaluation for this model id (LTI plants are evaluated by the caller: x+ = A x + B u)"; return -2;
  }
}

