// Per-item bodies of the plant probe (test infrastructure, never part of the product): the conventions of dev_probe_cases.hpp
// -- the Io record, batch-minor doubles, one item per lane -- for the plants, integrators and derivative routines of
// cddp-cpp_amd/csrc/dev_models.hpp.  Every case calls product routines on one item and writes everything they return; nothing of
// the routines' text is repeated here.  Compiled twice: by hipcc for gfx950 (plant_probe.hip -> libcddp_hip_probe.so) and by g++
// for the host (plant_probe_host.cpp, built by tests/plant_probe.py at test time with -ffp-contract=off -DCDDP_TRIG_SHARED=1).
//
// Common input prefix of the plant cases: p[32] (the parameter block as the kernels read it from ProblemDev::mp), x[NX], u[NU].
#pragma once
#include "dev_probe_cases.hpp"   // Io, and the DEV / CDDP_HOST_MODELS / CDDP_TRIG_HOST switches of the host build
#include "../../cddp-cpp_amd/csrc/dev_models.hpp"

namespace probe {

template <class M>
struct PlantIn {
  static constexpr int NX = M::NX, NU = M::NU, N = 32 + NX + NU;
  double p[32], x[NX], u[NU];
  DEV void load(const Io &io, int at) {
    for (int e = 0; e < 32; ++e) p[e] = io.get(at + e);
    for (int e = 0; e < NX; ++e) x[e] = io.get(at + 32 + e);
    for (int e = 0; e < NU; ++e) u[e] = io.get(at + 32 + NX + e);
  }
};

// ---- f: in = p, x, u; out = Model::f (Model::step for the discrete plants) ---------------------------------------------------------
template <class M>
struct CaseF {
  static constexpr int NX = M::NX, NIN = PlantIn<M>::N, NOUT = NX;
  static DEV void run(const Io &io) {
    PlantIn<M> in; in.load(io, 0);
    double xd[NX];
    for (int e = 0; e < NX; ++e) xd[e] = 0.0;
    if constexpr (M::kDiscrete) M::step(in.p, in.x, in.u, xd);
    else M::f(in.p, in.x, in.u, xd);
    for (int e = 0; e < NX; ++e) io.put(e, xd[e]);
  }
};

// ---- step: in = integrator, dt, p, x, u; out = x_next of Stepper::step(int, dt, ...), of Stepper::step(DynCtx, ...) and of
//      roll_step<M, INTEG> (default FLAGGED), then the redo flag ------------------------------------------------------------------------
template <class M>
struct CaseStep {
  static constexpr int NX = M::NX, NIN = 2 + PlantIn<M>::N, NOUT = 3 * NX + 1;
  static DEV void run(const Io &io) {
    const int integ = (int)io.get(0);
    const double dt = io.get(1);
    PlantIn<M> in; in.load(io, 2);
    double a[NX], b[NX], c[NX];
    for (int e = 0; e < NX; ++e) a[e] = b[e] = c[e] = 0.0;
    Stepper<M>::step(integ, dt, in.p, in.x, in.u, a);
    DynCtx ctx; ctx.load(integ, dt, in.p);
    Stepper<M>::step(ctx, in.x, in.u, b);
    bool redo = false;
    switch (integ) {
      case CDDP_HIP_EULER: roll_step<M, CDDP_HIP_EULER>(ctx, in.x, in.u, c, &redo); break;
      case CDDP_HIP_HEUN: roll_step<M, CDDP_HIP_HEUN>(ctx, in.x, in.u, c, &redo); break;
      case CDDP_HIP_RK3: roll_step<M, CDDP_HIP_RK3>(ctx, in.x, in.u, c, &redo); break;
      default: roll_step<M, CDDP_HIP_RK4>(ctx, in.x, in.u, c, &redo); break;
    }
    for (int e = 0; e < NX; ++e) { io.put(e, a[e]); io.put(NX + e, b[e]); io.put(2 * NX + e, c[e]); }
    io.put(3 * NX, redo ? 1.0 : 0.0);
  }
};

// ---- jac: out = F_x[NX * NX], F_u[NX * NU] of Model::jac ---------------------------------------------------------------------------
template <class M>
struct CaseJac {
  static constexpr int NX = M::NX, NU = M::NU, NIN = PlantIn<M>::N, NOUT = NX * NX + NX * NU;
  static DEV void run(const Io &io) {
    PlantIn<M> in; in.load(io, 0);
    double Fx[NX * NX], Fu[NX * NU];
    for (int e = 0; e < NX * NX; ++e) Fx[e] = 0.0;
    for (int e = 0; e < NX * NU; ++e) Fu[e] = 0.0;
    M::jac(in.p, in.x, in.u, Fx, Fu);
    for (int e = 0; e < NX * NX; ++e) io.put(e, Fx[e]);
    for (int e = 0; e < NX * NU; ++e) io.put(NX * NX + e, Fu[e]);
  }
};

// ---- hess (models whose build has kHasHess): out = F_xx[NX][NX][NX], F_uu[NX][NU][NU], F_ux[NX][NU][NX] ----------------------------
template <class M>
struct CaseHess {
  static_assert(M::kHasHess, "this build of the plant has no hess()");
  static constexpr int NX = M::NX, NU = M::NU, NXX = NX * NX * NX, NUU = NX * NU * NU, NUX = NX * NU * NX;
  static constexpr int NIN = PlantIn<M>::N, NOUT = NXX + NUU + NUX;
  static DEV void run(const Io &io) {
    PlantIn<M> in; in.load(io, 0);
    double H[NOUT];   // (largest: 776 doubles on the device -- the fuel-state HCW plant --, 4802 in the host build of the 7-joint arm)
    for (int e = 0; e < NOUT; ++e) H[e] = 0.0;
    M::hess(in.p, in.x, in.u, H, H + NXX, H + NXX + NUU);
    for (int e = 0; e < NOUT; ++e) io.put(e, H[e]);
  }
};

// ---- tensor terms of the blocked plants: in = p, dt, x, u, w[NX], Q_xx[NX * NX], Q_ux[NU * NX], Q_uu[NU * NU];
//      out = the three blocks after ad_tensor_terms_blocked<Dyn, NX, NU, 4> (div = 1, every plant's kHessDiv) -----------------------------
template <class M, class Dyn>
struct CaseTensor {
  static constexpr int NX = M::NX, NU = M::NU, NQ = NX * NX + NU * NX + NU * NU;
  static constexpr int NIN = 32 + 1 + NX + NU + NX + NQ, NOUT = NQ;
  static DEV void run(const Io &io) {
    double p[32], x[NX], u[NU], w[NX], Q[NQ];
    for (int e = 0; e < 32; ++e) p[e] = io.get(e);
    const double dt = io.get(32);
    for (int e = 0; e < NX; ++e) x[e] = io.get(33 + e);
    for (int e = 0; e < NU; ++e) u[e] = io.get(33 + NX + e);
    for (int e = 0; e < NX; ++e) w[e] = io.get(33 + NX + NU + e);
    for (int e = 0; e < NQ; ++e) Q[e] = io.get(33 + NX + NU + NX + e);
    ad_tensor_terms_blocked<Dyn, NX, NU, 4>(p, x, u, w, dt, 1.0, Q, Q + NX * NX, Q + NX * NX + NU * NX);
    for (int e = 0; e < NQ; ++e) io.put(e, Q[e]);
  }
};

// ---- blocked Jacobian: out = F_x, F_u of ad_jacobian_blocked<Dyn, NX, NU, BS>, then F_x, F_u of ad_jacobian<Dyn, NX, NU> -----------------
template <class M, class Dyn, int BS>
struct CaseJacBlocked {
  static constexpr int NX = M::NX, NU = M::NU, NJ = NX * NX + NX * NU, NIN = PlantIn<M>::N, NOUT = 2 * NJ;
  static DEV void run(const Io &io) {
    PlantIn<M> in; in.load(io, 0);
    double A[NJ], B[NJ];
    for (int e = 0; e < NJ; ++e) A[e] = B[e] = 0.0;
    ad_jacobian_blocked<Dyn, NX, NU, BS>(in.p, in.x, in.u, A, A + NX * NX);
    ad_jacobian<Dyn, NX, NU>(in.p, in.x, in.u, B, B + NX * NX);
    for (int e = 0; e < NJ; ++e) { io.put(e, A[e]); io.put(NJ + e, B[e]); }
  }
};

typedef LTIModel<2, 1> Lti21;   // one of the instantiations inst_lti.hip builds

}  // namespace probe

// ---- the lists both builds expand: X(name, case type) ------------------------------------------------------------------------------
// every model struct of dev_models.hpp: Y(tag, Model)
#define PLANT_MODELS(Y) \
  Y(pendulum, cddp_dev::PendulumModel) Y(cartpole, cddp_dev::CartPoleModel) Y(unicycle, cddp_dev::UnicycleModel) Y(lti21, probe::Lti21) \
  Y(quadrotor, cddp_dev::QuadrotorModel) Y(manipulator, cddp_dev::ManipulatorModel) Y(quad12, cddp_dev::Quad12Model) \
  Y(manip7, cddp_dev::Manip7Model) Y(bicycle, cddp_dev::BicycleModel) Y(car, cddp_dev::CarModel) Y(hcw, cddp_dev::HCWModel) \
  Y(euler, cddp_dev::EulerAttitudeModel) Y(quaternion, cddp_dev::QuaternionAttitudeModel) Y(mrp, cddp_dev::MrpAttitudeModel) \
  Y(twobody, cddp_dev::SpacecraftTwobodyModel) Y(landing2d, cddp_dev::SpacecraftLanding2DModel) Y(dubins, cddp_dev::DubinsCarModel) \
  Y(dreyfus, cddp_dev::DreyfusRocketModel) Y(acrobot, cddp_dev::AcrobotModel) Y(usv, cddp_dev::Usv3DofModel) \
  Y(forklift, cddp_dev::ForkliftModel) Y(quadrotorrate, cddp_dev::QuadrotorRateModel) \
  Y(linearfuel, cddp_dev::SpacecraftLinearFuelModel) Y(nonlinear, cddp_dev::SpacecraftNonlinearModel)
// the plants whose hess() exists in BOTH builds: Y(tag, Model)
#define PLANT_HESS_BOTH(Y) \
  Y(pendulum, cddp_dev::PendulumModel) Y(cartpole, cddp_dev::CartPoleModel) Y(unicycle, cddp_dev::UnicycleModel) Y(lti21, probe::Lti21) \
  Y(manipulator, cddp_dev::ManipulatorModel) Y(bicycle, cddp_dev::BicycleModel) Y(car, cddp_dev::CarModel) Y(hcw, cddp_dev::HCWModel) \
  Y(landing2d, cddp_dev::SpacecraftLanding2DModel) Y(dubins, cddp_dev::DubinsCarModel) Y(dreyfus, cddp_dev::DreyfusRocketModel) \
  Y(acrobot, cddp_dev::AcrobotModel) Y(forklift, cddp_dev::ForkliftModel) Y(linearfuel, cddp_dev::SpacecraftLinearFuelModel)
// the eight plants whose device build contracts the tensors block by block (HessDyn); their hess() is host-only: Y(tag, Model, Dyn)
#define PLANT_BLOCKED(Y) \
  Y(quadrotor, cddp_dev::QuadrotorModel, cddp_dev::QuadrotorDyn) Y(quad12, cddp_dev::Quad12Model, cddp_dev::Quad12Dyn) \
  Y(manip7, cddp_dev::Manip7Model, cddp_dev::Manip7Dyn) Y(euler, cddp_dev::EulerAttitudeModel, cddp_dev::EulerAttitudeDyn) \
  Y(quaternion, cddp_dev::QuaternionAttitudeModel, cddp_dev::QuaternionAttitudeDyn) Y(mrp, cddp_dev::MrpAttitudeModel, cddp_dev::MrpAttitudeDyn) \
  Y(usv, cddp_dev::Usv3DofModel, cddp_dev::Usv3DofDyn) Y(quadrotorrate, cddp_dev::QuadrotorRateModel, cddp_dev::QuadrotorRateDyn)
// the plants whose jac() is ad_jacobian_blocked, with the block size each uses: Y(tag, Model, Dyn, BS)
#define PLANT_JAC_BLOCKED(Y) \
  Y(euler, cddp_dev::EulerAttitudeModel, cddp_dev::EulerAttitudeDyn, 3) Y(quaternion, cddp_dev::QuaternionAttitudeModel, cddp_dev::QuaternionAttitudeDyn, 4) \
  Y(mrp, cddp_dev::MrpAttitudeModel, cddp_dev::MrpAttitudeDyn, 3) Y(forklift, cddp_dev::ForkliftModel, cddp_dev::ForkliftDyn, 4) \
  Y(quadrotorrate, cddp_dev::QuadrotorRateModel, cddp_dev::QuadrotorRateDyn, 4)
