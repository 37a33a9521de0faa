// Device-side plants: continuous dynamics f(x,u) and continuous-time Jacobians f_x, f_u
// (the DynamicalSystem plugin surface, reference include/cddp-cpp/cddp_core/dynamical_system.hpp
// and src/dynamics_model/*.cpp), enumerated by cddp_hip_model id.
//
// Derivative source per model:
//   Pendulum / Unicycle : the reference's analytic Jacobians (pendulum.cpp:44-66, unicycle.cpp:44-66)
//   CartPole            : hand-derived exact derivatives of the autodiff expression
//                         (cartpole.cpp:69-103, which includes the damping term)
//   Quadrotor           : forward-mode duals through the quaternion normalisation, i.e. what
//                         autodiff::jacobian does on quadrotor.cpp:166-219
//   Manipulator         : central finite differences, h = 2e-5 (manipulator.cpp:53-70, helper.hpp:95-118)
//   LTI                 : (A - I)/dt, B/dt (lti_system.cpp:78-92)
#pragma once
#include <type_traits>
#include "dev_linalg.hpp"
#include "dev_trig.hpp"
#include "../../include/cddp_hip.h"

namespace cddp_dev {

// ---- trig policy of a plant's f (a template parameter of Model::f of the plants that carry `kTrigPolicy`) --------------------
// TrigChecked: what every caller gets by default -- plant_sincos, i.e. (shared-arithmetic build) the fast routine with its own range
// test, ballot and libm fallback per call.  TrigFlagged: the fast result only, the range verdict ORed into the caller's flag
// (dev_trig.hpp::sincos_fast_flag); the caller tests the flag once per integrator step and redoes the step with the checked path
// (RollStep below).  Only meaningful where plant_sincos IS the fast routine: kTrigFlaggable.
struct TrigChecked {
  DEV void sincos(double a, double *s, double *c) const { plant_sincos(a, s, c); }
};
struct TrigFlagged {
  bool *out_of_range;
  DEV void sincos(double a, double *s, double *c) const { const SinCosPair r = sincos_fast_flag(a, *out_of_range); *s = r.s; *c = r.c; }
};
#ifdef CDDP_TRIG_SHARED
constexpr bool kTrigFlaggable = true;
#else
constexpr bool kTrigFlaggable = false;
#endif
template <class Model, class = void> struct HasTrigPolicy { static constexpr bool value = false; };
template <class Model> struct HasTrigPolicy<Model, typename std::enable_if<Model::kTrigPolicy>::type> { static constexpr bool value = kTrigFlaggable; };

// ---- forward-mode dual number with NP compile-time seeds (register resident) ------------
template <int NP>
struct DualN {
  double v;
  double d[NP];
  DEV DualN() {}
  DEV DualN(double x) : v(x) {
#pragma unroll
    for (int i = 0; i < NP; ++i) d[i] = 0.0;
  }
};
template <int NP> DEV DualN<NP> operator+(const DualN<NP> &a, const DualN<NP> &b) { DualN<NP> r; r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
template <int NP> DEV DualN<NP> operator-(const DualN<NP> &a, const DualN<NP> &b) { DualN<NP> r; r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
template <int NP> DEV DualN<NP> operator-(const DualN<NP> &a) { DualN<NP> r; r.v = -a.v;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = -a.d[i]; return r; }
template <int NP> DEV DualN<NP> operator*(const DualN<NP> &a, const DualN<NP> &b) { DualN<NP> r; r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
template <int NP> DEV DualN<NP> operator/(const DualN<NP> &a, const DualN<NP> &b) { DualN<NP> r; r.v = a.v / b.v;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v; return r; }
template <int NP> DEV DualN<NP> dsin(const DualN<NP> &a) { DualN<NP> r; double s, c; plant_sincos(a.v, &s, &c); r.v = s;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = c * a.d[i]; return r; }
template <int NP> DEV DualN<NP> dcos(const DualN<NP> &a) { DualN<NP> r; double s, c; plant_sincos(a.v, &s, &c); r.v = c; double ms = -s;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = ms * a.d[i]; return r; }
template <int NP> DEV DualN<NP> dsqrt(const DualN<NP> &a) { DualN<NP> r; r.v = sqrt(a.v); double g = 0.5 / r.v;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = g * a.d[i]; return r; }
template <int NP> DEV DualN<NP> dasin(const DualN<NP> &a) { DualN<NP> r; r.v = plant_asin(a.v); double g = 1.0 / sqrt(1.0 - a.v * a.v);
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = g * a.d[i]; return r; }
template <int NP> DEV DualN<NP> dtan(const DualN<NP> &a) { DualN<NP> r; r.v = plant_tan(a.v); double g = 1.0 + r.v * r.v;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = g * a.d[i]; return r; }
DEV double dasin(double a) { return plant_asin(a); }
DEV double dtan(double a) { return plant_tan(a); }
DEV double dsin(double a) { return plant_sin(a); }
DEV double dcos(double a) { return plant_cos(a); }
DEV double dsqrt(double a) { return sqrt(a); }
DEV double dval(double a) { return a; }
template <int NP> DEV double dval(const DualN<NP> &a) { return a.v; }
// sin / cos of N scalars of type S (double or a dual) from ONE batched evaluation of the values (dev_trig.hpp: the
// independent angles of a plant share a basic block, so their chains interleave).  Used by the two large synthetic plants
// (12 / 52 evaluations per RK4 step); the reference's own plants keep the device libm -- there the rollout is not bound
// by it (no change measured at C2 / C3) and the libm's results left every strict parity case bit-stable.
DEV double lift_sin(double, double s, double) { return s; }
DEV double lift_cos(double, double, double c) { return c; }
template <int NP> DEV DualN<NP> lift_sin(const DualN<NP> &a, double s, double c) { DualN<NP> r; r.v = s;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = c * a.d[i]; return r; }
template <int NP> DEV DualN<NP> lift_cos(const DualN<NP> &a, double s, double c) { DualN<NP> r; r.v = c; const double ms = -s;
#pragma unroll
  for (int i = 0; i < NP; ++i) r.d[i] = ms * a.d[i]; return r; }
template <int N, class S> DEV void trig_n(const S *a, S *sn, S *cs) {
  double av[N], sv[N], cv[N];
#pragma unroll
  for (int i = 0; i < N; ++i) av[i] = dval(a[i]);
  sincos_n<N>(av, sv, cv);
#pragma unroll
  for (int i = 0; i < N; ++i) { sn[i] = lift_sin(a[i], sv[i], cv[i]); cs[i] = lift_cos(a[i], sv[i], cv[i]); }
}

// Second-order forward mode (the reference's autodiff::dual2nd, dynamical_system.cpp:137-217): value, gradient and Hessian
// w.r.t. NP seeded variables z = [x, u].  Only for the plants whose Hessians the reference takes from autodiff (CartPole)
// and only evaluated when options.use_ilqr == 0.
template <int NP>
struct Dual2N {
  double v, d[NP], h[NP * NP];
  DEV Dual2N() {}
  DEV Dual2N(double x) : v(x) {
    for (int i = 0; i < NP; ++i) d[i] = 0.0;
    for (int i = 0; i < NP * NP; ++i) h[i] = 0.0;
  }
};
template <int NP> DEV Dual2N<NP> d2_unary(const Dual2N<NP> &a, double val, double p1, double p2) {
  Dual2N<NP> r; r.v = val;
  for (int i = 0; i < NP; ++i) { r.d[i] = p1 * a.d[i]; for (int j = 0; j < NP; ++j) r.h[i * NP + j] = p2 * a.d[i] * a.d[j] + p1 * a.h[i * NP + j]; }
  return r;
}
template <int NP> DEV Dual2N<NP> operator+(const Dual2N<NP> &a, const Dual2N<NP> &b) { Dual2N<NP> r; r.v = a.v + b.v;
  for (int i = 0; i < NP; ++i) r.d[i] = a.d[i] + b.d[i];
  for (int i = 0; i < NP * NP; ++i) r.h[i] = a.h[i] + b.h[i]; return r; }
template <int NP> DEV Dual2N<NP> operator-(const Dual2N<NP> &a, const Dual2N<NP> &b) { Dual2N<NP> r; r.v = a.v - b.v;
  for (int i = 0; i < NP; ++i) r.d[i] = a.d[i] - b.d[i];
  for (int i = 0; i < NP * NP; ++i) r.h[i] = a.h[i] - b.h[i]; return r; }
template <int NP> DEV Dual2N<NP> operator-(const Dual2N<NP> &a) { Dual2N<NP> r; r.v = -a.v;
  for (int i = 0; i < NP; ++i) r.d[i] = -a.d[i];
  for (int i = 0; i < NP * NP; ++i) r.h[i] = -a.h[i]; return r; }
template <int NP> DEV Dual2N<NP> operator*(const Dual2N<NP> &a, const Dual2N<NP> &b) { Dual2N<NP> r; r.v = a.v * b.v;
  for (int i = 0; i < NP; ++i) {
    r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    for (int j = 0; j < NP; ++j) r.h[i * NP + j] = a.h[i * NP + j] * b.v + a.d[i] * b.d[j] + a.d[j] * b.d[i] + a.v * b.h[i * NP + j];
  }
  return r; }
template <int NP> DEV Dual2N<NP> operator/(const Dual2N<NP> &a, const Dual2N<NP> &b) {
  const double inv = 1.0 / b.v;
  return a * d2_unary<NP>(b, inv, -inv * inv, 2.0 * inv * inv * inv); }
template <int NP> DEV Dual2N<NP> dsin(const Dual2N<NP> &a) { double s, c; plant_sincos(a.v, &s, &c); return d2_unary<NP>(a, s, c, -s); }
template <int NP> DEV Dual2N<NP> dcos(const Dual2N<NP> &a) { double s, c; plant_sincos(a.v, &s, &c); return d2_unary<NP>(a, c, -s, -c); }
template <int NP> DEV Dual2N<NP> dsqrt(const Dual2N<NP> &a) { const double r = sqrt(a.v); return d2_unary<NP>(a, r, 0.5 / r, -0.25 / (a.v * r)); }
template <int NP> DEV Dual2N<NP> dasin(const Dual2N<NP> &a) { const double w = 1.0 - a.v * a.v, r = sqrt(w); return d2_unary<NP>(a, plant_asin(a.v), 1.0 / r, a.v / (w * r)); }
template <int NP> DEV Dual2N<NP> dtan(const Dual2N<NP> &a) { const double t = plant_tan(a.v), g = 1.0 + t * t; return d2_unary<NP>(a, t, g, 2.0 * t * g); }
template <int NP> DEV double dval(const Dual2N<NP> &a) { return a.v; }
template <int NP> DEV Dual2N<NP> lift_sin(const Dual2N<NP> &a, double s, double c) { return d2_unary<NP>(a, s, c, -s); }   // trig_n on second-order duals
template <int NP> DEV Dual2N<NP> lift_cos(const Dual2N<NP> &a, double s, double c) { return d2_unary<NP>(a, c, -s, -c); }

// Hessian tensors by second-order duals of a templated functor F::template eval<S>(p, x, u, out): out_i's Hessian w.r.t. z = [x, u],
// split into the solver's three blocks (f_xx[i] nx x nx, f_uu[i] nu x nu, f_ux[i] nu x nx), each entry divided by `div`
template <class F, int NX, int NU>
DEV void ad_hessian(const double *p, const double *x, const double *u, double div, double *Fxx, double *Fuu, double *Fux) {
  typedef Dual2N<NX + NU> D;
  D xs[NX], us[NU], xd[NX];
  for (int i = 0; i < NX; ++i) { xs[i] = D(x[i]); xs[i].d[i] = 1.0; }
  for (int j = 0; j < NU; ++j) { us[j] = D(u[j]); us[j].d[NX + j] = 1.0; }
  F::template eval<D>(p, xs, us, xd);
  constexpr int NP = NX + NU;
  for (int i = 0; i < NX; ++i) {
    for (int a = 0; a < NX; ++a) for (int b = 0; b < NX; ++b) Fxx[(i * NX + a) * NX + b] = xd[i].h[a * NP + b] / div;
    for (int a = 0; a < NU; ++a) for (int b = 0; b < NU; ++b) Fuu[(i * NU + a) * NU + b] = xd[i].h[(NX + a) * NP + NX + b] / div;
    for (int a = 0; a < NU; ++a) for (int b = 0; b < NX; ++b) Fux[(i * NU + a) * NX + b] = xd[i].h[(NX + a) * NP + b] / div;
  }
}

// The same second-order terms WITHOUT materialising the tensors, for plants whose full dual2nd frame does not fit a GPU lane
// (quadrotor: 17 seeds = 307 doubles per dual number, a 180-KB private frame; 7-joint arm: 21 seeds).  The Hessian of every output
// is assembled from evaluations with 2 * BS seeds at a time: the seeded variables z = [x, u] are cut into blocks of BS, and for every
// unordered pair of blocks (I, J) the functor is evaluated once with the variables of I in seed slots 0 .. BS-1 and those of J in
// slots BS .. 2 BS - 1 (73 doubles per dual number at BS = 4).  Second-order forward mode is component-wise in the seed pair --
// entry (a, b) of a product or a unary lift reads only the operands' value, d[a], d[b] and h[a][b] (operator* / d2_unary above) --
// so every entry equals, bit for bit, the entry the full Dual2N<NX + NU> evaluation (ad_hessian, the host build) produces.
// Accumulated directly into the solver's sums in its own order (for i: Q[e] += w[i] * (dt * F[i][e]), i ascending per entry):
//   Qxx[a * NX + b] += w[i] (dt f_i,xx[a][b] / div),  Qux[a * NX + b] += w[i] (dt f_i,ux[a][b] / div),  Quu likewise.
template <class F, int NX, int NU, int BS>
DEV_NOINLINE void ad_tensor_terms_blocked(const double *p, const double *x, const double *u, const double *w, double dt, double div,
                                          double *Qxx, double *Qux, double *Quu) {
  constexpr int NP = NX + NU, NBK = (NP + BS - 1) / BS, NS = 2 * BS;
  typedef Dual2N<NS> D;
  for (int I = 0; I < NBK; ++I) {
    for (int J = I; J < NBK; ++J) {
      D xs[NX], us[NU], xd[NX];
      for (int v = 0; v < NP; ++v) {
        D z(v < NX ? x[v] : u[v - NX]);
        const int blk = v / BS, off = v - blk * BS;
        if (blk == I) z.d[off] = 1.0;
        else if (blk == J) z.d[BS + off] = 1.0;
        if (v < NX) xs[v] = z; else us[v - NX] = z;
      }
      F::template eval<D>(p, xs, us, xd);
      // entries (row variable va, column variable vb) this pair owns: va in I, vb in J, and (I != J) va in J, vb in I
      for (int pass = 0; pass < (I == J ? 1 : 2); ++pass) {
        const int RB = pass == 0 ? I : J, CB = pass == 0 ? J : I;
        for (int ra = 0; ra < BS; ++ra) {
          const int va = RB * BS + ra;
          if (va >= NP) break;
          const int sa = (RB == I) ? ra : BS + ra;
          for (int cb = 0; cb < BS; ++cb) {
            const int vb = CB * BS + cb;
            if (vb >= NP) break;
            const int sb = (CB == I) ? cb : BS + cb;
            double *dst;
            if (va < NX && vb < NX) dst = Qxx + va * NX + vb;
            else if (va >= NX && vb >= NX) dst = Quu + (va - NX) * NU + (vb - NX);
            else if (va >= NX && vb < NX) dst = Qux + (va - NX) * NX + vb;
            else continue;   // d2 f / dx du: the solver reads the (u, x) block only
            double acc = *dst;
            for (int i = 0; i < NX; ++i) acc = acc + w[i] * (dt * (xd[i].h[sa * NS + sb] / div));
            *dst = acc;
          }
        }
      }
    }
  }
}

// does the plant take its second-order terms from the blocked evaluation (a `HessDyn` functor typedef, device build only)?
template <class M, class = void> struct HessBlocked { static constexpr bool value = false; };
template <class M> struct HessBlocked<M, decltype((void)sizeof(typename M::HessDyn))> { static constexpr bool value = true; };

// Jacobian by forward-mode duals of a templated dynamics functor F::template eval<S>(p, x, u, xd)
template <class F, int NX, int NU>
DEV void ad_jacobian(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
  typedef DualN<NX + NU> D;
  D xs[NX], us[NU], xd[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) { xs[i] = D(x[i]); xs[i].d[i] = 1.0; }
#pragma unroll
  for (int j = 0; j < NU; ++j) { us[j] = D(u[j]); us[j].d[NX + j] = 1.0; }
  F::template eval<D>(p, xs, us, xd);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
#pragma unroll
    for (int j = 0; j < NX; ++j) Fx[i * NX + j] = xd[i].d[j];
#pragma unroll
    for (int j = 0; j < NU; ++j) Fu[i * NU + j] = xd[i].d[NX + j];
  }
}

// ================================================================================ Pendulum
struct PendulumModel {   // pendulum.cpp:29-66; params: length, mass, damping, gravity
  static constexpr int ID = CDDP_HIP_MODEL_PENDULUM, NX = 2, NU = 1;
  static constexpr bool kDiscrete = false;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    const double length = p[0], mass = p[1], damping = p[2], gravity = p[3];
    const double inertia = mass * length * length;
    xd[0] = x[1];
    xd[1] = (u[0] - damping * x[1] + mass * gravity * length * dsin(x[0])) / inertia;
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    const double length = p[0], mass = p[1], damping = p[2], gravity = p[3];
    Fx[0] = 0.0; Fx[1] = 1.0;
    Fx[2] = (gravity / length) * dcos(x[0]);
    Fx[3] = -damping / (mass * length * length);
    Fu[0] = 0.0; Fu[1] = 1.0 / (mass * length * length);
  }
  // Hessian tensors f_xx[i] (NX x NX), f_uu[i] (NU x NU), f_ux[i] (NU x NX), i = output row: state Hessian analytic
  // (pendulum.cpp:68-78), control Hessian zero (:80-85), cross Hessian = autodiff of the -sin twin (:87-100) = zero
  static constexpr bool kHasHess = true;
  DEV static void hess(const double *p, const double *x, const double *, double *Fxx, double *Fuu, double *Fux) {
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
    Fxx[1 * NX * NX + 0] = -(p[3] / p[0]) * dsin(x[0]);
  }
};

// ================================================================================ CartPole
struct CartPoleModel {   // cartpole.cpp:38-103; params: cart_mass, pole_mass, pole_length, gravity, damping
  static constexpr int ID = CDDP_HIP_MODEL_CARTPOLE, NX = 4, NU = 1;
  static constexpr bool kDiscrete = false;
  static constexpr bool kTrigPolicy = true;
  template <class Trig = TrigChecked>
  DEV static void f(const double *p, const double *x, const double *u, double *xd, const Trig tg = Trig()) {
    // double path (cartpole.cpp:38-67): NO damping term
    const double mc = p[0], mp = p[1], l = p[2], g = p[3];
    const double theta_dot = x[3], force = u[0];
    double s, c; tg.sincos(x[1], &s, &c);
    const double total_mass = mc + mp;
    const double den = mc + mp * s * s;
    xd[0] = x[2];
    xd[1] = theta_dot;
    xd[2] = (force + mp * s * (l * theta_dot * theta_dot + g * c)) / den;
    xd[3] = (-force * c - mp * l * theta_dot * theta_dot * c * s - total_mass * g * s) / (l * den);
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
#ifdef CDDP_TRIG_SHARED
    // parity build: forward-mode duals through the autodiff expression, operation for operation what autodiff::jacobian does
    // (and what the CPU checker restates) -- the hand-derived form below is the same derivative from a different expression
    // tree, i.e. equal up to the last bits only, and a non-converging solve amplifies last bits
    {
      typedef DualN<5> D;
      D xs[4], us[1], xd[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { xs[i] = D(x[i]); xs[i].d[i] = 1.0; }
      us[0] = D(u[0]); us[0].d[4] = 1.0;
      f_ad<D>(p, xs, us, xd);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Fx[i * 4 + j] = xd[i].d[j];
        Fu[i] = xd[i].d[4];
      }
      return;
    }
#endif
    // exact derivatives of the autodiff expression (cartpole.cpp:69-103, WITH -damping*theta_dot)
    const double mc = p[0], mp = p[1], l = p[2], g = p[3], b = p[4];
    const double w = x[3], F = u[0];
    double s, c; plant_sincos(x[1], &s, &c);
    const double M = mc + mp;
    const double den = mc + mp * s * s;
    const double dden = 2.0 * mp * s * c;
    const double inner = l * w * w + g * c;
    const double num3 = F + mp * s * inner;
    const double dnum3 = mp * c * inner - mp * s * g * s;
    const double num4 = -F * c - mp * l * w * w * c * s - M * g * s - b * w;
    const double dnum4 = F * s - mp * l * w * w * (c * c - s * s) - M * g * c;
    const double den2 = den * den;
#pragma unroll
    for (int i = 0; i < 16; ++i) Fx[i] = 0.0;
    Fx[0 * 4 + 2] = 1.0;
    Fx[1 * 4 + 3] = 1.0;
    Fx[2 * 4 + 1] = (dnum3 * den - num3 * dden) / den2;
    Fx[2 * 4 + 3] = (mp * s * (2.0 * l * w)) / den;
    Fx[3 * 4 + 1] = (dnum4 * den - num4 * dden) / (l * den2);
    Fx[3 * 4 + 3] = (-2.0 * mp * l * w * c * s - b) / (l * den);
    Fu[0] = 0.0; Fu[1] = 0.0;
    Fu[2] = 1.0 / den;
    Fu[3] = -c / (l * den);
  }
  // the autodiff expression (cartpole.cpp:69-103, with the damping term) on any scalar type
  template <class S>
  DEV static void f_ad(const double *p, const S *x, const S *u, S *xd) {
    const double mc = p[0], mp = p[1], l = p[2], g = p[3], b = p[4];
    const S theta = x[1], x_dot = x[2], theta_dot = x[3], force = u[0];
    const S sin_theta = dsin(theta), cos_theta = dcos(theta);
    const double total_mass = mc + mp;
    const S den = S(mc) + S(mp) * sin_theta * sin_theta;
    xd[0] = x_dot;
    xd[1] = theta_dot;
    xd[2] = (force + S(mp) * sin_theta * (S(l) * theta_dot * theta_dot + S(g) * cos_theta)) / den;
    xd[3] = (-force * cos_theta - S(mp) * S(l) * theta_dot * theta_dot * cos_theta * sin_theta - S(total_mass) * S(g) * sin_theta - S(b) * theta_dot) / (S(l) * den);
  }
  // Hessians: the DynamicalSystem defaults (dual2nd through the autodiff path, cartpole.cpp:191-199)
  static constexpr bool kHasHess = true;
  DEV static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    typedef Dual2N<5> D;
    D xs[4], us[1], xd[4];
    for (int i = 0; i < 4; ++i) { xs[i] = D(x[i]); xs[i].d[i] = 1.0; }
    us[0] = D(u[0]); us[0].d[4] = 1.0;
    f_ad<D>(p, xs, us, xd);
    for (int i = 0; i < 4; ++i) {
      for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) Fxx[i * 16 + a * 4 + b] = xd[i].h[a * 5 + b];
      Fuu[i] = xd[i].h[4 * 5 + 4];
      for (int b = 0; b < 4; ++b) Fux[i * 4 + b] = xd[i].h[4 * 5 + b];
    }
  }
};

// ================================================================================ Unicycle
struct UnicycleModel {   // unicycle.cpp:28-66
  static constexpr int ID = CDDP_HIP_MODEL_UNICYCLE, NX = 3, NU = 2;
  static constexpr bool kDiscrete = false;
  static constexpr bool kTrigPolicy = true;
  template <class Trig = TrigChecked>
  DEV static void f(const double *, const double *x, const double *u, double *xd, const Trig tg = Trig()) {
    double s, c; tg.sincos(x[2], &s, &c);
    xd[0] = u[0] * c; xd[1] = u[0] * s; xd[2] = u[1];
  }
  DEV static void jac(const double *, const double *x, const double *u, double *Fx, double *Fu) {
    double s, c; plant_sincos(x[2], &s, &c);
#pragma unroll
    for (int i = 0; i < 9; ++i) Fx[i] = 0.0;
    Fx[0 * 3 + 2] = -u[0] * s;
    Fx[1 * 3 + 2] = u[0] * c;
    Fu[0] = c; Fu[1] = 0.0; Fu[2] = s; Fu[3] = 0.0; Fu[4] = 0.0; Fu[5] = 1.0;
  }
  // state Hessian analytic (unicycle.cpp:68-80), control Hessian zero (:82-89), cross Hessian = the autodiff default on
  // getContinuousDynamicsAutodiff (:91-107): d2(v cos th)/dv dth = -sin th, d2(v sin th)/dv dth = cos th
  static constexpr bool kHasHess = true;
  DEV static void hess(const double *, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    double s, c; plant_sincos(x[2], &s, &c);
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
    Fxx[0 * 9 + 2 * 3 + 2] = -u[0] * c;
    Fxx[1 * 9 + 2 * 3 + 2] = -u[0] * s;
    Fux[0 * 6 + 0 * 3 + 2] = -s;
    Fux[1 * 6 + 0 * 3 + 2] = c;
  }
};

// ================================================================================ LTI
// Discrete x+ = A x + B u (lti_system.cpp:71-76); A at p[0 .. NX*NX), B after it.
template <int NX_, int NU_>
struct LTIModel {
  static constexpr int ID = CDDP_HIP_MODEL_LTI, NX = NX_, NU = NU_;
  static constexpr bool kDiscrete = true;
  static constexpr bool kHasHess = true;   // lti_system.cpp:94-115: zero
  DEV static void hess(const double *, const double *, const double *, double *Fxx, double *Fuu, double *Fux) {
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
  }
  DEV static void step(const double *p, const double *x, const double *u, double *xn) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      double s = 0.0, t = 0.0;
#pragma unroll
      for (int j = 0; j < NX; ++j) s += p[i * NX + j] * x[j];
#pragma unroll
      for (int j = 0; j < NU; ++j) t += p[NX * NX + i * NU + j] * u[j];
      xn[i] = s + t;
    }
  }
  DEV static void f(const double *, const double *, const double *, double *) {}
  // continuous-equivalent Jacobians; dt arrives in p[NX*NX + NX*NU]
  DEV static void jac(const double *p, const double *, const double *, double *Fx, double *Fu) {
    const double dt = p[NX * NX + NX * NU];
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j < NX; ++j) Fx[i * NX + j] = (p[i * NX + j] - (i == j ? 1.0 : 0.0)) / dt;
#pragma unroll
    for (int i = 0; i < NX * NU; ++i) Fu[i] = p[NX * NX + i] / dt;
  }
};

// ================================================================================ Bicycle (bicycle.cpp)
// Kinematic bicycle, state [x, y, theta, v], control [a, delta]; params: wheelbase.  Analytic Jacobians (:68-111) and state /
// control Hessians (:113-156); the cross Hessian is the base class's autodiff default (dynamical_system.cpp:190-217).
struct BicycleDyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {
    const S theta = x[2], v = x[3];
    xd[0] = v * dcos(theta);
    xd[1] = v * dsin(theta);
    xd[2] = (v / S(p[0])) * dtan(u[1]);
    xd[3] = u[0];
  }
};
struct BicycleModel {
  static constexpr int ID = CDDP_HIP_MODEL_BICYCLE, NX = 4, NU = 2;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = true;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { BicycleDyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    double s, c; plant_sincos(x[2], &s, &c);
    const double v = x[3], L = p[0], cd = plant_cos(u[1]);
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) Fx[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NX * NU; ++i) Fu[i] = 0.0;
    Fx[0 * NX + 2] = -v * s; Fx[0 * NX + 3] = c;
    Fx[1 * NX + 2] = v * c;  Fx[1 * NX + 3] = s;
    Fx[2 * NX + 3] = plant_tan(u[1]) / L;
    Fu[3 * NU + 0] = 1.0;
    Fu[2 * NU + 1] = v / (L * (cd * cd));
  }
  DEV static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    double sxx[NX * NX * NX], suu[NX * NU * NU];   // the autodiff blocks the analytic overrides replace
    ad_hessian<BicycleDyn, NX, NU>(p, x, u, 1.0, sxx, suu, Fux);
    double s, c; plant_sincos(x[2], &s, &c);
    const double v = x[3], L = p[0], cd = plant_cos(u[1]);
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    Fxx[(0 * NX + 2) * NX + 2] = -v * c; Fxx[(0 * NX + 2) * NX + 3] = -s; Fxx[(0 * NX + 3) * NX + 2] = -s;
    Fxx[(1 * NX + 2) * NX + 2] = -v * s; Fxx[(1 * NX + 2) * NX + 3] = c;  Fxx[(1 * NX + 3) * NX + 2] = c;
    Fuu[(2 * NU + 1) * NU + 1] = 2.0 * v * plant_sin(u[1]) / (L * (cd * cd * cd));
  }
};

// ================================================================================ HCW (spacecraft_linear.cpp)
// Hill-Clohessy-Wiltshire equations of relative orbital motion: state [x, y, z, vx, vy, vz] (radial, along-track, cross-track), control
// [Fx, Fy, Fz]; params: mean motion n, mass.  Linear and time-invariant in continuous time: constant Jacobians (:56-83), zero Hessians
// (:85-120).
struct HCWModel {
  static constexpr int ID = CDDP_HIP_MODEL_HCW, NX = 6, NU = 3;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = true;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    const double n = p[0], n2 = n * n, mass = p[1];
    xd[0] = x[3]; xd[1] = x[4]; xd[2] = x[5];
    xd[3] = 2.0 * n * x[4] + 3.0 * n2 * x[0] + u[0] / mass;
    xd[4] = -2.0 * n * x[3] + u[1] / mass;
    xd[5] = -n2 * x[2] + u[2] / mass;
  }
  DEV static void jac(const double *p, const double *, const double *, double *Fx, double *Fu) {
    const double n = p[0], n2 = n * n, mass = p[1];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) Fx[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NX * NU; ++i) Fu[i] = 0.0;
    Fx[0 * NX + 3] = 1.0; Fx[1 * NX + 4] = 1.0; Fx[2 * NX + 5] = 1.0;
    Fx[3 * NX + 0] = 3.0 * n2; Fx[3 * NX + 4] = 2.0 * n;
    Fx[4 * NX + 3] = -2.0 * n;
    Fx[5 * NX + 2] = -n2;
    Fu[3 * NU + 0] = 1.0 / mass; Fu[4 * NU + 1] = 1.0 / mass; Fu[5 * NU + 2] = 1.0 / mass;
  }
  DEV static void hess(const double *, const double *, const double *, double *Fxx, double *Fuu, double *Fux) {
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
  }
};

// ================================================================================ Car (car.cpp)
// A DISCRETE plant: getDiscreteDynamics is overridden (:24-60) and everything else differentiates it -- Jacobians are the autodiff
// gradient of the discrete map with J.diagonal() -= 1 and J /= timestep (:62-111), Hessians its autodiff Hessian / timestep
// (:113-161; the cross Hessian through the base default on (x+ - x) / timestep is the same block).  State [x, y, theta, v],
// control [steering delta, acceleration a]; params: wheelbase, p[1] = timestep (filled in by the library).
struct CarDyn {
  template <class S, bool kClamps>
  DEV static void next(const double *p, const S *x, const S *u, S *xn) {
    const double d = p[0], h = p[1];
    const S theta = x[2], v = x[3], delta = u[0], a = u[1];
    const S cos_theta = dcos(theta), sin_theta = dsin(theta);
    const S f = S(h) * v;
    const S sin_delta = dsin(delta);
    const S f_sin_delta = f * sin_delta;
    S inside = S(d * d) - f_sin_delta * f_sin_delta;
    if (kClamps && dval(inside) < 0.0) inside = S(0.0);            // autodiff path only (:183-186)
    const S b = S(d) + f * dcos(delta) - dsqrt(inside);
    S asin_arg = sin_delta * f / S(d);
    if (kClamps && fabs(dval(asin_arg)) > 1.0) asin_arg = S(dval(asin_arg) > 0.0 ? 1.0 : -1.0);   // :196-199
    const S dtheta = dasin(asin_arg);
    xn[0] = x[0] + b * cos_theta;
    xn[1] = x[1] + b * sin_theta;
    xn[2] = x[2] + dtheta;
    xn[3] = x[3] + S(h) * a;
  }
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xn) { next<S, true>(p, x, u, xn); }
};
struct CarModel {
  static constexpr int ID = CDDP_HIP_MODEL_CAR, NX = 4, NU = 2;
  static constexpr bool kDiscrete = true;
  static constexpr bool kHasHess = true;
  DEV static void step(const double *p, const double *x, const double *u, double *xn) { CarDyn::next<double, false>(p, x, u, xn); }
  DEV static void f(const double *, const double *, const double *, double *) {}
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian<CarDyn, NX, NU>(p, x, u, Fx, Fu);
    const double h = p[1];
#pragma unroll
    for (int i = 0; i < NX; ++i) Fx[i * NX + i] -= 1.0;
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) Fx[i] = Fx[i] / h;
#pragma unroll
    for (int i = 0; i < NX * NU; ++i) Fu[i] = Fu[i] / h;
  }
  DEV static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    ad_hessian<CarDyn, NX, NU>(p, x, u, p[1], Fxx, Fuu, Fux);
  }
};

// ================================================================================ Quadrotor (nx=13)
struct QuadrotorDyn {   // quadrotor.cpp:33-104 == :166-219; params: mass, arm, Ixx, Iyy, Izz, gravity
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {
    const double mass = p[0], arm = p[1], Ixx = p[2], Iyy = p[3], Izz = p[4], grav = p[5];
    xd[0] = x[7]; xd[1] = x[8]; xd[2] = x[9];
    S qw = x[3], qx = x[4], qy = x[5], qz = x[6];
    S norm = dsqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    if (dval(norm) > 1e-6) { qw = qw / norm; qx = qx / norm; qy = qy / norm; qz = qz / norm; }
    else { qw = S(1.0); qx = S(0.0); qy = S(0.0); qz = S(0.0); }
    const S ox = x[10], oy = x[11], oz = x[12];
    xd[3] = S(-0.5) * (qx * ox + qy * oy + qz * oz);
    xd[4] = S(0.5) * (qw * ox + qy * oz - qz * oy);
    xd[5] = S(0.5) * (qw * oy - qx * oz + qz * ox);
    xd[6] = S(0.5) * (qw * oz + qx * oy - qy * ox);
    const S f1 = u[0], f2 = u[1], f3 = u[2], f4 = u[3];
    const S thrust = f1 + f2 + f3 + f4;
    const S tau_x = S(arm) * (f1 - f3);
    const S tau_y = S(arm) * (f2 - f4);
    const S tau_z = S(0.1) * (f1 - f2 + f3 - f4);
    const S R02 = S(2.0) * (qx * qz + qy * qw);
    const S R12 = S(2.0) * (qy * qz - qx * qw);
    const S R22 = S(1.0) - S(2.0) * (qx * qx + qy * qy);
    const double invm = 1.0 / mass;
    xd[7] = S(invm) * (R02 * thrust);
    xd[8] = S(invm) * (R12 * thrust);
    xd[9] = S(invm) * (R22 * thrust) - S(grav);
    const double c00 = Iyy * Izz, c11 = Ixx * Izz, c22 = Ixx * Iyy;
    const double det = c00 * Ixx;
    const double invdet = 1.0 / det;
    const double i00 = c00 * invdet, i11 = c11 * invdet, i22 = c22 * invdet;
    const S Iox = S(Ixx) * ox, Ioy = S(Iyy) * oy, Ioz = S(Izz) * oz;
    const S cx = oy * Ioz - oz * Ioy;
    const S cy = oz * Iox - ox * Ioz;
    const S cz = ox * Ioy - oy * Iox;
    xd[10] = S(i00) * (tau_x - cx);
    xd[11] = S(i11) * (tau_y - cy);
    xd[12] = S(i22) * (tau_z - cz);
  }
};
struct QuadrotorModel {
  static constexpr int ID = CDDP_HIP_MODEL_QUADROTOR, NX = 13, NU = 4;
  static constexpr bool kDiscrete = false;
  // quadrotor.cpp:224-278: dual2nd through the normalised-quaternion dynamics (17 seeds: 307 doubles per dual number).  On the
  // device that is a 180-KB private frame per lane -- beyond the 128-KB limit -- so the tensors exist in the HOST build of this file
  // only (host_models.cpp -> cddp_hip_model_eval -> the plug-in solve), and the device-resident solve refuses use_ilqr = 0 for this
  // plant.  Little is lost: the reference's own getCrossHessian returns nx x nu matrices where its solvers add nu x nx blocks (an
  // Eigen size mismatch), i.e. full DDP on the quadrotor is not defined behaviour there; here the cross block has the shape the
  // solver's formula needs.
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    ad_hessian<QuadrotorDyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux);
  }
  static constexpr bool kHessBlocked = false;
#else
  static constexpr bool kHasHess = false;
  // device (round 4): the tensors are never materialised -- their contraction with the value gradient is assembled from 8-seed
  // evaluations (ad_tensor_terms_blocked, bitwise the full 17-seed evaluation of the host build)
  static constexpr bool kHessBlocked = true;
  typedef QuadrotorDyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { QuadrotorDyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian<QuadrotorDyn, NX, NU>(p, x, u, Fx, Fu);
  }
};

// ================================================================================ SYNTHETIC quadrotor, Euler-ZYX, nx=12
struct Quad12Dyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {
    const double mass = p[0], arm = p[1], Ixx = p[2], Iyy = p[3], Izz = p[4], grav = p[5];
    const S phi = x[6], th = x[7], psi = x[8];
    const S ox = x[9], oy = x[10], oz = x[11];
    const S ang[3] = {phi, th, psi}; S sn[3], cs[3];
    trig_n<3, S>(ang, sn, cs);
    const S sph = sn[0], cph = cs[0], sth = sn[1], cth = cs[1], sps = sn[2], cps = cs[2];
    const S thrust = u[0] + u[1] + u[2] + u[3];
    xd[0] = x[3]; xd[1] = x[4]; xd[2] = x[5];
    const double invm = 1.0 / mass;
    xd[3] = S(invm) * ((cph * sth * cps + sph * sps) * thrust);
    xd[4] = S(invm) * ((cph * sth * sps - sph * cps) * thrust);
    xd[5] = S(invm) * ((cph * cth) * thrust) - S(grav);
    const S tth = sth / cth;
    xd[6] = ox + sph * tth * oy + cph * tth * oz;
    xd[7] = cph * oy - sph * oz;
    xd[8] = (sph * oy + cph * oz) / cth;
    const S tau_x = S(arm) * (u[0] - u[2]);
    const S tau_y = S(arm) * (u[1] - u[3]);
    const S tau_z = S(0.1) * (u[0] - u[1] + u[2] - u[3]);
    xd[9] = (tau_x - (S(Izz) - S(Iyy)) * oy * oz) / S(Ixx);
    xd[10] = (tau_y - (S(Ixx) - S(Izz)) * oz * ox) / S(Iyy);
    xd[11] = (tau_z - (S(Iyy) - S(Ixx)) * ox * oy) / S(Izz);
  }
};
struct Quad12Model {
  static constexpr int ID = CDDP_HIP_MODEL_QUADROTOR_EULER12, NX = 12, NU = 4;
  static constexpr bool kDiscrete = false;
  // full DDP (round 4): second-order duals through the plant's own expression, as the reference's base class does for a plant
  // without overrides (dynamical_system.cpp:137-217); host build: the whole tensors, device: blocked contraction
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) { ad_hessian<Quad12Dyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux); }
#else
  static constexpr bool kHasHess = false;
  static constexpr bool kHessBlocked = true;
  typedef Quad12Dyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { Quad12Dyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian<Quad12Dyn, NX, NU>(p, x, u, Fx, Fu);
  }
};

// ================================================================================ Manipulator (3-DOF)
struct ManipulatorModel {   // manipulator.cpp:29-70,174-208
  static constexpr int ID = CDDP_HIP_MODEL_MANIPULATOR, NX = 6, NU = 3;
  static constexpr bool kDiscrete = false;
  // manipulator.cpp:72-86: the state and control Hessians are ZERO overrides; the cross Hessian is the base class's autodiff default
  // on ddq = M(q)^-1 (tau - G(q)) (dynamical_system.cpp:190-217), i.e. d2 ddq_i / dtau_j dq_k = d(M^-1)_ij / dq_k, evaluated here in
  // closed form: -(M^-1 (dM/dq_k) M^-1)_ij, k = 1, 2 (M does not depend on q_0).
  static constexpr bool kHasHess = true;
  DEV static void hess(const double *, const double *x, const double *, double *Fxx, double *Fuu, double *Fux) {
    const double la = 1.0, lb = 0.2, lc = 1.0, m1 = 1.0, m2 = 1.0, m3 = 0.5;
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
    double s1, c1, s2, c2, s12, c12;
    plant_sincos(x[1], &s1, &c1); plant_sincos(x[2], &s2, &c2); plant_sincos(x[1] + x[2], &s12, &c12);
    double M[9], Minv[9];
    M[0] = (m1 + m2 + m3) * (la * la); M[4] = (m2 + m3) * (lb * lb); M[8] = m3 * (lc * lc);
    M[1] = M[3] = (m2 + m3) * la * lb * c1; M[5] = M[7] = m3 * lb * lc * c2; M[2] = M[6] = m3 * la * lc * c12;
    inverse_pplu<3>(M, Minv);
    for (int k = 1; k <= 2; ++k) {
      double dM[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      dM[2] = dM[6] = -(m3 * la * lc) * s12;
      if (k == 1) dM[1] = dM[3] = -((m2 + m3) * la * lb) * s1;
      else dM[5] = dM[7] = -(m3 * lb * lc) * s2;
      double T[9], R[9];
      mm_nn<3, 3, 3>(Minv, dM, T);
      mm_nn<3, 3, 3>(T, Minv, R);
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Fux[((3 + i) * NU + j) * NX + k] = -R[i * 3 + j];
    }
  }
  DEV static void f(const double *, const double *x, const double *u, double *xd) {
    const double la = 1.0, lb = 0.2, lc = 1.0, grav = 9.81;
    const double m1 = 1.0, m2 = 1.0, m3 = 0.5;
    double M[9];
    const double c1 = plant_cos(x[1]), c2 = plant_cos(x[2]), c12 = plant_cos(x[1] + x[2]);
    M[0] = (m1 + m2 + m3) * (la * la);
    M[4] = (m2 + m3) * (lb * lb);
    M[8] = m3 * (lc * lc);
    M[1] = M[3] = (m2 + m3) * la * lb * c1;
    M[5] = M[7] = m3 * lb * lc * c2;
    M[2] = M[6] = m3 * la * lc * c12;
    double G[3];
    G[0] = 0;
    G[1] = -(m2 + m3) * grav * lb * c1 - m3 * grav * lc * c12;
    G[2] = -m3 * grav * lc * c12;
    double Minv[9];
    inverse_pplu<3>(M, Minv);
    double rhs[3] = {u[0] - G[0], u[1] - G[1], u[2] - G[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      xd[i] = x[3 + i];
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += Minv[i * 3 + k] * rhs[k];
      xd[3 + i] = s;
    }
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    const double h = 2e-5;
    double xp[NX], up[NU], fp[NX], fm[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xp[i] = x[i];
#pragma unroll
    for (int i = 0; i < NU; ++i) up[i] = u[i];
    for (int i = 0; i < NX; ++i) {
      xp[i] = x[i] + h; f(p, xp, u, fp);
      xp[i] = x[i] - h; f(p, xp, u, fm);
      for (int r = 0; r < NX; ++r) Fx[r * NX + i] = (fp[r] - fm[r]) / (2.0 * h);
      xp[i] = x[i];
    }
    for (int i = 0; i < NU; ++i) {
      up[i] = u[i] + h; f(p, x, up, fp);
      up[i] = u[i] - h; f(p, x, up, fm);
      for (int r = 0; r < NX; ++r) Fu[r * NU + i] = (fp[r] - fm[r]) / (2.0 * h);
      up[i] = u[i];
    }
  }
};

// ================================================================================ SYNTHETIC 7-joint manipulator, nx=14
struct Manip7Dyn {
  template <class S>
  DEV static void eval(const double *, const S *x, const S *u, S *xd) {
    const double mi[7] = {2.5, 2.0, 1.6, 1.2, 0.9, 0.6, 0.4};
    const double li[7] = {1.0, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3};
    const double wi[7] = {0.0, 1.4, 1.1, 0.8, 0.5, 0.3, 0.15};
    const double ci[7] = {0.0, 0.30, 0.25, 0.20, 0.15, 0.10, 0.05};
    const double grav = 9.81;
    // the 13 angles (7 cumulative, 6 neighbour differences) first, one batched cosine evaluation, then the joint rows
    S ang[13], sn[13], cs[13];
    S cum = S(0.0);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      cum = cum + x[i];
      ang[i] = cum;
      if (i > 0) ang[6 + i] = x[i] - x[i - 1];
    }
    trig_n<13, S>(ang, sn, cs);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      xd[i] = x[7 + i];
      S Mii = S(mi[i] * li[i] * li[i]);
      if (i > 0) { S cd = cs[6 + i]; Mii = Mii + S(ci[i]) * cd * cd; }
      S Gi = S(-grav * wi[i]) * cs[i];
      xd[7 + i] = (u[i] - Gi) / Mii;
    }
  }
};
struct Manip7Model {
  static constexpr int ID = CDDP_HIP_MODEL_MANIPULATOR7, NX = 14, NU = 7;
  static constexpr bool kDiscrete = false;
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) { ad_hessian<Manip7Dyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux); }
#else
  static constexpr bool kHasHess = false;
  static constexpr bool kHessBlocked = true;   // see Quad12Model
  typedef Manip7Dyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { Manip7Dyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian<Manip7Dyn, NX, NU>(p, x, u, Fx, Fu);
  }
};

// ================================================================================ spacecraft plants (nx <= 8)
// Jacobian by forward-mode duals seeded in column blocks of BS variables: one evaluation of F per block of z = [x, u].  Forward mode
// is component-wise in the seeds, so every column equals, bit for bit, the column of the full DualN<NX + NU> evaluation (ad_jacobian);
// the point is the register file: 4 doubles per dual number instead of NX + NU + 1 keeps the attitude plants' derivative fill and
// sweep kernels free of scratch.
template <class F, int NX, int NU, int BS>
DEV void ad_jacobian_blocked(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
  constexpr int NP = NX + NU, NBK = (NP + BS - 1) / BS;
  typedef DualN<BS> D;
#pragma unroll
  for (int I = 0; I < NBK; ++I) {
    D xs[NX], us[NU], xd[NX];
#pragma unroll
    for (int v = 0; v < NP; ++v) {
      D z(v < NX ? x[v] : u[v - NX]);
      if (v / BS == I) z.d[v - I * BS] = 1.0;
      if (v < NX) xs[v] = z; else us[v - NX] = z;
    }
    F::template eval<D>(p, xs, us, xd);
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int c = 0; c < BS; ++c) {
        const int v = I * BS + c;
        if (v < NX) Fx[i * NX + v] = xd[i].d[c];
        else if (v < NP) Fu[i * NU + (v - NX)] = xd[i].d[c];
      }
  }
}

// Rigid-body rotational dynamics shared by the three attitude plants (euler_attitude.cpp:47-49 and its twins):
//   d(omega)/dt = I^-1 (-skew(omega) (I omega) + tau),   I = p[0..8], I^-1 = p[9..17] (row-major; host_models.cpp fills I^-1 as Eigen's
// fixed-size inverse does).  The zero entries of -skew(omega) are left out of the products (x + 0 * y == x for finite operands).
template <class S>
DEV void rigid_body_rates(const double *p, const S *w, const S *tau, S *wd) {
  S h[3], v[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) h[i] = (S(p[3 * i]) * w[0] + S(p[3 * i + 1]) * w[1]) + S(p[3 * i + 2]) * w[2];
  v[0] = (w[2] * h[1] - w[1] * h[2]) + tau[0];
  v[1] = (w[0] * h[2] - w[2] * h[0]) + tau[1];
  v[2] = (w[1] * h[0] - w[0] * h[1]) + tau[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) wd[i] = (S(p[9 + 3 * i]) * v[0] + S(p[9 + 3 * i + 1]) * v[1]) + S(p[9 + 3 * i + 2]) * v[2];
}

// ---------------------------------------------------------------------------- EulerAttitude (euler_attitude.cpp:33-52, .hpp:159-180)
// State [psi, theta, phi, wx, wy, wz] (ZYX angles), control [tau_x, tau_y, tau_z].  Jacobians and Hessians: autodiff of the autodiff
// expression (:54-76, :78-147), which is the value expression on duals.  The |cos theta| < 1e-9 guard replaces cos theta by a CONSTANT
// +-1e-9 (zero derivative), as T(1e-9 * sign) does there; tan theta is not guarded.
struct EulerAttitudeDyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {
    const S theta = x[1], phi = x[2];
    const S s_phi = dsin(phi), c_phi = dcos(phi);
    const S c_theta = dcos(theta), tan_theta = dtan(theta);
    S cos_theta_safe = c_theta;
    if (fabs(dval(c_theta)) < 1e-9) cos_theta_safe = S(dval(c_theta) >= 0 ? 1e-9 : -1e-9);
    xd[0] = (s_phi / cos_theta_safe) * x[4] + (c_phi / cos_theta_safe) * x[5];
    xd[1] = c_phi * x[4] + (-s_phi) * x[5];
    xd[2] = (x[3] + (s_phi * tan_theta) * x[4]) + (c_phi * tan_theta) * x[5];
    rigid_body_rates<S>(p, x + 3, u, xd + 3);
  }
};
struct EulerAttitudeModel {
  static constexpr int ID = CDDP_HIP_MODEL_EULER_ATTITUDE, NX = 6, NU = 3;
  static constexpr bool kDiscrete = false;
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) { ad_hessian<EulerAttitudeDyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux); }
#else
  static constexpr bool kHasHess = false;   // device: the blocked contraction (Dual2N<9> per lane would be a 700-double frame)
  static constexpr bool kHessBlocked = true;
  typedef EulerAttitudeDyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { EulerAttitudeDyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian_blocked<EulerAttitudeDyn, NX, NU, 3>(p, x, u, Fx, Fu);
  }
};

// ---------------------------------------------------------------------------- QuaternionAttitude (quaternion_attitude.cpp:33-62, 159-183)
// State [qw, qx, qy, qz, wx, wy, wz], control [tau_x, tau_y, tau_z].  The VALUE normalises q (|q| > 1e-9, else the identity); the
// autodiff expression behind the Jacobians and Hessians does NOT -- so f_x is the derivative of the un-normalised kinematics.
struct QuaternionAttitudeDyn {
  template <class S>
  DEV static void kin(const S *q, const S *w, S *qd) {   // (0.5 * Omega(omega)) q, zero entries left out
    const S a0 = S(0.5) * w[0], a1 = S(0.5) * w[1], a2 = S(0.5) * w[2];
    qd[0] = ((-a0) * q[1] + (-a1) * q[2]) + (-a2) * q[3];
    qd[1] = (a0 * q[0] + a2 * q[2]) + (-a1) * q[3];
    qd[2] = (a1 * q[0] + (-a2) * q[1]) + a0 * q[3];
    qd[3] = (a2 * q[0] + a1 * q[1]) + (-a0) * q[2];
  }
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {   // the autodiff expression (:159-183)
    kin<S>(x, x + 4, xd);
    rigid_body_rates<S>(p, x + 4, u, xd + 4);
  }
};
struct QuaternionAttitudeModel {
  static constexpr int ID = CDDP_HIP_MODEL_QUATERNION_ATTITUDE, NX = 7, NU = 3;
  static constexpr bool kDiscrete = false;
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) { ad_hessian<QuaternionAttitudeDyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux); }
#else
  static constexpr bool kHasHess = false;
  static constexpr bool kHessBlocked = true;
  typedef QuaternionAttitudeDyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {   // :33-62
    double q[4] = {x[0], x[1], x[2], x[3]};
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (nrm > 1e-9) {
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = q[i] / nrm;
    } else {
      q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
    }
    QuaternionAttitudeDyn::kin<double>(q, x + 4, xd);
    rigid_body_rates<double>(p, x + 4, u, xd + 4);
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian_blocked<QuaternionAttitudeDyn, NX, NU, 4>(p, x, u, Fx, Fu);
  }
};

// ---------------------------------------------------------------------------- MrpAttitude (mrp_attitude.cpp:31-98, .hpp:154+)
// State [s1, s2, s3, wx, wy, wz] (modified Rodrigues parameters), control [tau_x, tau_y, tau_z];
// d(sigma)/dt = (0.25 B(sigma)) omega, B = (1 - |sigma|^2) I + 2 skew(sigma) + 2 sigma sigma^T.  Every derivative is the base class's
// autodiff of the autodiff expression (dynamical_system.cpp:100-217).
struct MrpAttitudeDyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {
    const S *s = x;
    const S a = S(1.0) - ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    S B[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) B[3 * i + j] = (S(2.0) * s[i]) * s[j];
    B[0] = a + B[0]; B[4] = a + B[4]; B[8] = a + B[8];
    B[1] = S(2.0) * (-s[2]) + B[1]; B[2] = S(2.0) * s[1] + B[2];
    B[3] = S(2.0) * s[2] + B[3];    B[5] = S(2.0) * (-s[0]) + B[5];
    B[6] = S(2.0) * (-s[1]) + B[6]; B[7] = S(2.0) * s[0] + B[7];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      xd[i] = ((S(0.25) * B[3 * i]) * x[3] + (S(0.25) * B[3 * i + 1]) * x[4]) + (S(0.25) * B[3 * i + 2]) * x[5];
    rigid_body_rates<S>(p, x + 3, u, xd + 3);
  }
};
struct MrpAttitudeModel {
  static constexpr int ID = CDDP_HIP_MODEL_MRP_ATTITUDE, NX = 6, NU = 3;
  static constexpr bool kDiscrete = false;
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) { ad_hessian<MrpAttitudeDyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux); }
#else
  static constexpr bool kHasHess = false;
  static constexpr bool kHessBlocked = true;
  typedef MrpAttitudeDyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { MrpAttitudeDyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian_blocked<MrpAttitudeDyn, NX, NU, 3>(p, x, u, Fx, Fu);
  }
};

// central finite differences of the continuous dynamics, h = 2e-5 (helper.hpp:95-119, as the manipulator's Jacobians)
template <class Model>
DEV void fd_jacobian(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
  constexpr int NX = Model::NX, NU = Model::NU;
  const double h = 2e-5;
  double xp[NX], up[NU], fp[NX], fm[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) xp[i] = x[i];
#pragma unroll
  for (int i = 0; i < NU; ++i) up[i] = u[i];
  for (int i = 0; i < NX; ++i) {
    xp[i] = x[i] + h; Model::f(p, xp, u, fp);
    xp[i] = x[i] - h; Model::f(p, xp, u, fm);
    for (int r = 0; r < NX; ++r) Fx[r * NX + i] = (fp[r] - fm[r]) / (2.0 * h);
    xp[i] = x[i];
  }
  for (int i = 0; i < NU; ++i) {
    up[i] = u[i] + h; Model::f(p, x, up, fp);
    up[i] = u[i] - h; Model::f(p, x, up, fm);
    for (int r = 0; r < NX; ++r) Fu[r * NU + i] = (fp[r] - fm[r]) / (2.0 * h);
    up[i] = u[i];
  }
}

// ---------------------------------------------------------------------------- SpacecraftTwobody (spacecraft_twobody.cpp:15-74)
// State [x, y, z, vx, vy, vz], control [ux, uy, uz]; params: mu, mass.  Jacobians: central FD.  State / control Hessians are zero
// overrides, but the plant has no autodiff expression, so the base class's cross Hessian throws: full DDP is refused for it.
struct SpacecraftTwobodyModel {
  static constexpr int ID = CDDP_HIP_MODEL_SPACECRAFT_TWOBODY, NX = 6, NU = 3;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = false;
  static constexpr bool kHessBlocked = false;
  // what the reference raises on use_ilqr = false (dynamical_system.hpp:54-60, reached through getCrossHessian)
  static constexpr const char *kNoHessMsg = "getContinuousDynamicsAutodiff must be overridden in the derived class to use Autodiff-based derivatives.";
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    const double mu = p[0], mass = p[1];
    const double r = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const double r3 = (r * r) * r;
    xd[0] = x[3]; xd[1] = x[4]; xd[2] = x[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) xd[3 + i] = ((-mu) * x[i]) / r3 + u[i] / mass;
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) { fd_jacobian<SpacecraftTwobodyModel>(p, x, u, Fx, Fu); }
};

// ---------------------------------------------------------------------------- SpacecraftLanding2D (spacecraft_landing2d.cpp:20-112)
// State in the header's order (spacecraft_landing2d.hpp:159-165): [x, x_dot, y, y_dot, theta, theta_dot]; control [thrust fraction,
// gimbal angle]; params: mass, length, width, min_thrust, max_thrust, max_gimble; gravity 9.81, inertia (1/12) m L^2.  Jacobians:
// central FD (:81-98).  State / control Hessians: zero overrides (:100-110).  Cross Hessian: the base-class autodiff default on the
// autodiff expression (:112+), which differs from the value -- thrust = u0 (no max_thrust factor) -- in closed form:
//   d2(u0 sin(u1 + th) / m) / du0 dth = cos(u1 + th) / m,   / du1 dth = -u0 sin(u1 + th) / m
//   d2(u0 cos(u1 + th) / m) / du0 dth = -sin(u1 + th) / m,  / du1 dth = -u0 cos(u1 + th) / m     (theta_dot row: no theta)
struct SpacecraftLanding2DModel {
  static constexpr int ID = CDDP_HIP_MODEL_SPACECRAFT_LANDING2D, NX = 6, NU = 2;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    const double mass = p[0], length = p[1], max_thrust = p[4];
    const double inertia = (1.0 / 12.0) * mass * length * length;
    const double total_angle = u[1] + x[4];
    const double thrust = max_thrust * u[0];
    double s, c; plant_sincos(total_angle, &s, &c);
    const double T = -length / 2.0 * thrust * plant_sin(u[1]);
    xd[0] = x[1]; xd[2] = x[3]; xd[4] = x[5];
    xd[1] = (thrust * s) / mass;
    xd[3] = (thrust * c) / mass - 9.81;
    xd[5] = T / inertia;
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) { fd_jacobian<SpacecraftLanding2DModel>(p, x, u, Fx, Fu); }
  DEV static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
    const double mass = p[0];
    double s, c; plant_sincos(u[1] + x[4], &s, &c);
    Fux[(1 * NU + 0) * NX + 4] = c / mass;
    Fux[(1 * NU + 1) * NX + 4] = -(u[0] * s) / mass;
    Fux[(3 * NU + 0) * NX + 4] = -s / mass;
    Fux[(3 * NU + 1) * NX + 4] = -(u[0] * c) / mass;
  }
};

// ================================================================================ the remaining small plants (nx <= 8)
// ---------------------------------------------------------------------------- DubinsCar (dubins_car.cpp)
// State [x, y, theta], control [omega]; params: speed.  Analytic Jacobians (:72-102) and state Hessian (:104-126), zero control Hessian
// (:128-141); the cross Hessian is the base class's autodiff default on speed cos / sin(theta), omega: no (u, x) term, i.e. zero.
struct DubinsCarModel {
  static constexpr int ID = CDDP_HIP_MODEL_DUBINS_CAR, NX = 3, NU = 1;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = true;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    double s, c; plant_sincos(x[2], &s, &c);
    xd[0] = p[0] * c; xd[1] = p[0] * s; xd[2] = u[0];
  }
  DEV static void jac(const double *p, const double *x, const double *, double *Fx, double *Fu) {
    double s, c; plant_sincos(x[2], &s, &c);
#pragma unroll
    for (int i = 0; i < 9; ++i) Fx[i] = 0.0;
    Fx[0 * 3 + 2] = -p[0] * s;
    Fx[1 * 3 + 2] = p[0] * c;
    Fu[0] = 0.0; Fu[1] = 0.0; Fu[2] = 1.0;
  }
  DEV static void hess(const double *p, const double *x, const double *, double *Fxx, double *Fuu, double *Fux) {
    double s, c; plant_sincos(x[2], &s, &c);
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
    Fxx[0 * 9 + 2 * 3 + 2] = -p[0] * c;
    Fxx[1 * 9 + 2 * 3 + 2] = -p[0] * s;
  }
};

// ---------------------------------------------------------------------------- DreyfusRocket (dreyfus_rocket.cpp)
// State [x, x_dot], control [theta]; params: thrust_acceleration, gravity_acceleration.  Analytic Jacobians (:46-64), zero state Hessian,
// analytic control Hessian (:72-82); cross Hessian: the autodiff default on an expression without a (u, x) term, i.e. zero.
struct DreyfusRocketModel {
  static constexpr int ID = CDDP_HIP_MODEL_DREYFUS_ROCKET, NX = 2, NU = 1;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = true;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    xd[0] = x[1];
    xd[1] = p[0] * dcos(u[0]) - p[1];
  }
  DEV static void jac(const double *p, const double *, const double *u, double *Fx, double *Fu) {
    Fx[0] = 0.0; Fx[1] = 1.0; Fx[2] = 0.0; Fx[3] = 0.0;
    Fu[0] = 0.0; Fu[1] = -p[0] * dsin(u[0]);
  }
  DEV static void hess(const double *p, const double *, const double *u, double *Fxx, double *Fuu, double *Fux) {
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
    Fuu[0] = 0.0;
    Fuu[1] = -p[0] * dcos(u[0]);
  }
};

// ---------------------------------------------------------------------------- Acrobot (acrobot.cpp)
// State [theta1, theta2, theta1_dot, theta2_dot], control [torque on the second joint]; params: l1, l2, m1, m2, J1, J2; gravity 9.81 and
// friction 1.0 are fixed (acrobot.hpp:138-139).  No derivative override: every Jacobian and Hessian is the base class's autodiff of the
// autodiff expression (:98-163), which is the value expression on duals.  The 2 x 2 mass-matrix inverse is Eigen's fixed-size one on the
// scalar type at hand: cofactors times 1 / det, then the matrix-vector product.
struct AcrobotDyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {
    const double l1 = p[0], l2 = p[1], m1 = p[2], m2 = p[3], J1 = p[4], J2 = p[5], gravity = 9.81, friction = 1.0;
    const S theta1 = x[0], theta2 = x[1], w1 = x[2], w2 = x[3];
    const S c1 = dcos(theta1), s2 = dsin(theta2), c2 = dcos(theta2), c12 = dcos(theta1 + theta2);
    const S m11 = (S(m1 * l1 * l1 + J1) + S(m2) * (S(l1 * l1 + l2 * l2) + S(2 * l1 * l2) * c2)) + S(J2);
    const S m12 = S(m2) * (S(l2 * l2) + S(l1 * l2) * c2) + S(J2);
    const S m22 = S(l2 * l2 * m2 + J2);
    const S tmp = S(l1 * l2 * m2) * s2;
    const S b1 = -((S(2.0) * w1) * w2 + w2 * w2) * tmp;
    const S b2 = (tmp * w1) * w1;
    const S g1 = (S((m1 + m2) * l1) * c1 + S(m2 * l2) * c12) * S(gravity);
    const S g2 = (S(m2 * l2) * c12) * S(gravity);
    const S r1 = ((S(0.0) - b1) - g1) - S(friction) * w1;
    const S r2 = ((u[0] - b2) - g2) - S(friction) * w2;
    const S invdet = S(1.0) / (m11 * m22 - m12 * m12);
    xd[0] = w1;
    xd[1] = w2;
    xd[2] = (m22 * invdet) * r1 + ((-m12) * invdet) * r2;
    xd[3] = ((-m12) * invdet) * r1 + (m11 * invdet) * r2;
  }
};
struct AcrobotModel {
  static constexpr int ID = CDDP_HIP_MODEL_ACROBOT, NX = 4, NU = 1;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = true;   // Dual2N<5>, the cart-pole's frame
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { AcrobotDyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) { ad_jacobian<AcrobotDyn, NX, NU>(p, x, u, Fx, Fu); }
  DEV static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    ad_hessian<AcrobotDyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux);
  }
};

// ---------------------------------------------------------------------------- Usv3Dof (usv_3dof.cpp)
// Surface vessel, state [x, y, psi, u, v, r], control [tau_u, tau_v, tau_r].  The caller passes no parameters: the library fills
// p[0..8] = M^-1 (Eigen's fixed 3 x 3 inverse of M_rb + M_a), p[9..17] = D_L, p[18..20] = m_x, m_y, m_yr from the reference's fixed vessel
// (:17-48; host_models.cpp).  Jacobians: the analytic ones as written at :152-227 (not autodiff: equal to rounding, another operation
// order).  State and cross Hessians: the base class's autodiff of :104-150; control Hessian: a zero override (:237-246) -- and the
// autodiff expression is linear in tau, so the blocked contraction of the device build adds exact zeros there.
struct Usv3DofDyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *tau, S *xd) {
    const S psi = x[2], u = x[3], v = x[4], r = x[5];
    const S c_psi = dcos(psi), s_psi = dsin(psi);
    const double m_x = p[18], m_y = p[19], m_yr = p[20];
    xd[0] = c_psi * u - s_psi * v;
    xd[1] = s_psi * u + c_psi * v;
    xd[2] = r;
    const S nu[3] = {u, v, r};
    // C(nu) nu with C's structural zeros left out (x + 0 * y == x for finite operands)
    const S C02 = S(-m_y) * v - S(m_yr) * r, C12 = S(m_x) * u, C20 = S(m_y) * v + S(m_yr) * r, C21 = S(-m_x) * u;
    const S Cnu[3] = {C02 * r, C12 * r, C20 * u + C21 * v};
    S w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const S Dnu = (S(p[9 + 3 * i]) * nu[0] + S(p[9 + 3 * i + 1]) * nu[1]) + S(p[9 + 3 * i + 2]) * nu[2];
      w[i] = (tau[i] - Cnu[i]) - Dnu;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) xd[3 + i] = (S(p[3 * i]) * w[0] + S(p[3 * i + 1]) * w[1]) + S(p[3 * i + 2]) * w[2];
  }
};
struct Usv3DofModel {
  static constexpr int ID = CDDP_HIP_MODEL_USV_3DOF, NX = 6, NU = 3;
  static constexpr bool kDiscrete = false;
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    ad_hessian<Usv3DofDyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux);
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
  }
#else
  static constexpr bool kHasHess = false;   // device: the blocked contraction, as the attitude plants of the same size
  static constexpr bool kHessBlocked = true;
  typedef Usv3DofDyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { Usv3DofDyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *, double *Fx, double *Fu) {
    const double u = x[3], v = x[4], r = x[5];
    double s_psi, c_psi; plant_sincos(x[2], &s_psi, &c_psi);
    const double m_x = p[18], m_y = p[19], m_yr = p[20];
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) Fx[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NX * NU; ++i) Fu[i] = 0.0;
    Fx[0 * NX + 2] = -s_psi * u - c_psi * v;
    Fx[1 * NX + 2] = c_psi * u - s_psi * v;
    Fx[0 * NX + 3] = c_psi; Fx[0 * NX + 4] = -s_psi;
    Fx[1 * NX + 3] = s_psi; Fx[1 * NX + 4] = c_psi;
    Fx[2 * NX + 5] = 1.0;
    double G[9];   // -dCnu_dnu - D_L
    G[0] = 0.0; G[1] = -m_y * r; G[2] = -m_y * v - 2 * m_yr * r;
    G[3] = m_x * r; G[4] = 0.0; G[5] = m_x * u;
    G[6] = (m_y - m_x) * v + m_yr * r; G[7] = (m_y - m_x) * u; G[8] = m_yr * u;
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = -G[i] - p[9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Fx[(3 + i) * NX + 3 + j] = (p[3 * i] * G[j] + p[3 * i + 1] * G[3 + j]) + p[3 * i + 2] * G[6 + j];
        Fu[(3 + i) * NU + j] = p[3 * i + j];
      }
  }
};

// ---------------------------------------------------------------------------- Forklift (forklift.cpp)
// A DISCRETE plant like the car: getDiscreteDynamics is overridden (:17-48, the integrator argument is ignored) and everything else
// differentiates it -- Jacobians are the autodiff gradient of the discrete map with J.diagonal() -= 1 and J /= timestep (:50-87),
// Hessians its autodiff Hessian / timestep (:89-125; the cross Hessian through the base default on (x+ - x) / timestep is the same
// block).  State [x, y, theta, v, steering angle], control [acceleration, steering rate]; params: wheelbase, rear_steer (0 / 1),
// max_steering_angle (carried, unused by the dynamics), p[3] = timestep (filled in by the library).
struct ForkliftDyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xn) {
    const double L = p[0], h = p[3];
    const double steer_sign = p[1] != 0.0 ? -1.0 : 1.0;
    const S theta = x[2], v = x[3];
    const S effective_delta = S(steer_sign) * x[4];
    const S cos_theta = dcos(theta), sin_theta = dsin(theta), tan_delta = dtan(effective_delta);
    const S hv = S(h) * v;
    xn[0] = x[0] + hv * cos_theta;
    xn[1] = x[1] + hv * sin_theta;
    xn[2] = x[2] + (hv * tan_delta) / S(L);
    xn[3] = x[3] + S(h) * u[0];
    xn[4] = x[4] + S(h) * u[1];
  }
};
struct ForkliftModel {
  static constexpr int ID = CDDP_HIP_MODEL_FORKLIFT, NX = 5, NU = 2;
  static constexpr bool kDiscrete = true;
  static constexpr bool kHasHess = true;
  DEV static void step(const double *p, const double *x, const double *u, double *xn) { ForkliftDyn::eval<double>(p, x, u, xn); }
  DEV static void f(const double *, const double *, const double *, double *) {}
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian_blocked<ForkliftDyn, NX, NU, 4>(p, x, u, Fx, Fu);
    const double h = p[3];
#pragma unroll
    for (int i = 0; i < NX; ++i) Fx[i * NX + i] -= 1.0;
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) Fx[i] = Fx[i] / h;
#pragma unroll
    for (int i = 0; i < NX * NU; ++i) Fu[i] = Fu[i] / h;
  }
  DEV static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) {
    ad_hessian<ForkliftDyn, NX, NU>(p, x, u, p[3], Fxx, Fuu, Fux);
  }
};

// ---------------------------------------------------------------------------- SpacecraftLinearFuel (spacecraft_linear_fuel.cpp)
// HCW relative motion with a mass state: [x, y, z, vx, vy, vz, mass, accumulated control effort], control [Fx, Fy, Fz]; params:
// mean_motion, isp, g0; epsilon = 1e-8 under the thrust norm is fixed (:27).  Jacobians: central FD (:124-139).  All three Hessians are
// zero overrides (:141-158): full DDP is allowed and adds nothing.
struct SpacecraftLinearFuelModel {
  static constexpr int ID = CDDP_HIP_MODEL_SPACECRAFT_LINEAR_FUEL, NX = 8, NU = 3;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    const double n = p[0], n2 = n * n, isp = p[1], g0 = p[2], mass = x[6];
    xd[0] = x[3]; xd[1] = x[4]; xd[2] = x[5];
    xd[3] = (2.0 * n * x[4] + 3.0 * n2 * x[0]) + u[0] / mass;
    xd[4] = -2.0 * n * x[3] + u[1] / mass;
    xd[5] = -n2 * x[2] + u[2] / mass;
    const double thrust_squared = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    xd[6] = -sqrt(thrust_squared + 1e-8) / (isp * g0);
    xd[7] = 0.5 * thrust_squared;
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) { fd_jacobian<SpacecraftLinearFuelModel>(p, x, u, Fx, Fu); }
  DEV static void hess(const double *, const double *, const double *, double *Fxx, double *Fuu, double *Fux) {
    for (int i = 0; i < NX * NX * NX; ++i) Fxx[i] = 0.0;
    for (int i = 0; i < NX * NU * NU; ++i) Fuu[i] = 0.0;
    for (int i = 0; i < NX * NU * NX; ++i) Fux[i] = 0.0;
  }
};

// ================================================================================ the two nx = 10 plants
// ---------------------------------------------------------------------------- QuadrotorRate (quadrotor_rate.cpp)
// Rate-controlled quadrotor: state [px, py, pz, vx, vy, vz, qw, qx, qy, qz], control [thrust, wx, wy, wz]; params: mass, max_thrust,
// max_rate (the last two are carried, the dynamics do not read them; all three must be positive, host_models.cpp); gravity 9.81.
// The value (:35-97) normalises q without a guard and goes through R (0, 0, thrust)^T and 0.5 Omega q; with the structural zeros left
// out and the exact factor 0.5 taken out of the sums, those products are, operation for operation, the sums of the autodiff expression
// (:142-202), so one templated body serves both.  Every derivative is the base class's autodiff THROUGH the normalisation.
struct QuadrotorRateDyn {
  template <class S>
  DEV static void eval(const double *p, const S *x, const S *u, S *xd) {
    const double mass = p[0], grav = 9.81;
    const S qw = x[6], qx = x[7], qy = x[8], qz = x[9];
    const S q_norm = dsqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    const S qw_n = qw / q_norm, qx_n = qx / q_norm, qy_n = qy / q_norm, qz_n = qz / q_norm;
    const S thrust = u[0], wx = u[1], wy = u[2], wz = u[3];
    xd[0] = x[3]; xd[1] = x[4]; xd[2] = x[5];
    const S R02 = S(2.0) * (qx_n * qz_n + qy_n * qw_n);
    const S R12 = S(2.0) * (qy_n * qz_n - qx_n * qw_n);
    const S R22 = S(1.0) - S(2.0) * (qx_n * qx_n + qy_n * qy_n);
    xd[3] = (R02 * thrust) / S(mass);
    xd[4] = (R12 * thrust) / S(mass);
    xd[5] = (R22 * thrust) / S(mass) - S(grav);
    xd[6] = S(0.5) * (((-qx_n) * wx - qy_n * wy) - qz_n * wz);
    xd[7] = S(0.5) * ((qw_n * wx + qy_n * wz) - qz_n * wy);
    xd[8] = S(0.5) * ((qw_n * wy - qx_n * wz) + qz_n * wx);
    xd[9] = S(0.5) * ((qw_n * wz + qx_n * wy) - qy_n * wx);
  }
};
struct QuadrotorRateModel {
  static constexpr int ID = CDDP_HIP_MODEL_QUADROTOR_RATE, NX = 10, NU = 4;
  static constexpr bool kDiscrete = false;
#ifdef CDDP_HOST_MODELS
  static constexpr bool kHasHess = true;
  static constexpr bool kHessBlocked = false;
  static void hess(const double *p, const double *x, const double *u, double *Fxx, double *Fuu, double *Fux) { ad_hessian<QuadrotorRateDyn, NX, NU>(p, x, u, 1.0, Fxx, Fuu, Fux); }
#else
  static constexpr bool kHasHess = false;   // device: the blocked contraction, as the 13-state quadrotor
  static constexpr bool kHessBlocked = true;
  typedef QuadrotorRateDyn HessDyn;
  static constexpr double kHessDiv = 1.0;
#endif
  DEV static void f(const double *p, const double *x, const double *u, double *xd) { QuadrotorRateDyn::eval<double>(p, x, u, xd); }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) {
    ad_jacobian_blocked<QuadrotorRateDyn, NX, NU, 4>(p, x, u, Fx, Fu);
  }
};

// ---------------------------------------------------------------------------- SpacecraftNonlinear (spacecraft_nonlinear.cpp)
// Nonlinear relative motion about an orbit that is itself integrated: state [px, py, pz, vx, vy, vz, r0, theta, dr0, dtheta], control
// [ux, uy, uz]; params: mass, r_scale, v_scale (carried, unused by the dynamics), mu.  pow(s, 1.5) of the reference (:51) is taken as
// s * sqrt(s): one correctly rounded square root and one product, within an ulp or two of the libm's pow and far inside the plant
// tests' 1e-13.  Jacobians: central FD (:75-91).  State / control Hessians are zero overrides, but there is no autodiff expression, so
// the base class's cross Hessian throws: full DDP is refused for this plant, as for SpacecraftTwobody.
struct SpacecraftNonlinearModel {
  static constexpr int ID = CDDP_HIP_MODEL_SPACECRAFT_NONLINEAR, NX = 10, NU = 3;
  static constexpr bool kDiscrete = false;
  static constexpr bool kHasHess = false;
  static constexpr bool kHessBlocked = false;
  static constexpr const char *kNoHessMsg = SpacecraftTwobodyModel::kNoHessMsg;
  DEV static void f(const double *p, const double *x, const double *u, double *xd) {
    const double mass = p[0], mu = p[3];
    const double px = x[0], py = x[1], pz = x[2], vx = x[3], vy = x[4], r0 = x[6], dr0 = x[8], dtheta = x[9];
    const double s = ((r0 + px) * (r0 + px) + py * py) + pz * pz;
    const double den = s * sqrt(s);
    const double r0_sq = r0 * r0;
    const double ddr0 = -mu / r0_sq + r0 * dtheta * dtheta;
    const double ddtheta = -2.0 * dr0 * dtheta / r0;
    xd[0] = vx; xd[1] = vy; xd[2] = x[5];
    xd[3] = ((((2.0 * dtheta * vy + ddtheta * py) + dtheta * dtheta * px) - mu * (px + r0) / den) + mu / r0_sq) + u[0] / mass;
    xd[4] = ((((-2.0 * dtheta * vx - ddtheta * px) + dtheta * dtheta * py) - mu * py / den)) + u[1] / mass;
    xd[5] = -mu * pz / den + u[2] / mass;
    xd[6] = dr0; xd[7] = dtheta; xd[8] = ddr0; xd[9] = ddtheta;
  }
  DEV static void jac(const double *p, const double *x, const double *u, double *Fx, double *Fu) { fd_jacobian<SpacecraftNonlinearModel>(p, x, u, Fx, Fu); }
};

// ---- explicit integrators (dynamical_system.cpp:28-83) --------------------------------------
// Loop-invariant integrator constants held in registers (SGPRs) by the serial kernels: the step size products
// and the plant parameters would otherwise be re-fetched through dependent scalar loads -- and dt/6 re-divided --
// on every step of the chain.  Same values, same arithmetic as Stepper::step(integrator, dt, p, ...).
struct DynCtx {
  int integrator;
  double dt, hdt, dt6, dt2;
  double mp[32];
  DEV void load(int integrator_, double dt_, const double *mp_) {
    integrator = integrator_; dt = dt_; hdt = 0.5 * dt; dt6 = dt / 6; dt2 = 2 * dt;
#pragma unroll
    for (int i = 0; i < 32; ++i) mp[i] = mp_[i];   // unused entries are dead code after unrolling
  }
};

template <class Model, bool D = Model::kDiscrete> struct Stepper;
template <class Model> struct Stepper<Model, true> {
  DEV static void step(int, double, const double *p, const double *x, const double *u, double *xn) { Model::step(p, x, u, xn); }
  DEV static void step(const DynCtx &c, const double *x, const double *u, double *xn) { Model::step(c.mp, x, u, xn); }
};
template <class Model> struct Stepper<Model, false> {
  DEV static void step(int integrator, double dt, const double *p, const double *x, const double *u, double *xn) {
    constexpr int NX = Model::NX;
    double k1[NX];
    Model::f(p, x, u, k1);
    if (integrator == CDDP_HIP_EULER) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + dt * k1[i];
      return;
    }
    double xt[NX], k2[NX];
    if (integrator == CDDP_HIP_HEUN) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + dt * k1[i];
      Model::f(p, xt, u, k2);
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + (0.5 * dt) * (k1[i] + k2[i]);
      return;
    }
    double k3[NX];
    if (integrator == CDDP_HIP_RK3) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + (0.5 * dt) * k1[i];
      Model::f(p, xt, u, k2);
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = (x[i] - dt * k1[i]) + (2 * dt) * k2[i];
      Model::f(p, xt, u, k3);
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + (dt / 6) * ((k1[i] + 4.0 * k2[i]) + k3[i]);
      return;
    }
    double k4[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xt[i] = x[i] + (0.5 * dt) * k1[i];
    Model::f(p, xt, u, k2);
#pragma unroll
    for (int i = 0; i < NX; ++i) xt[i] = x[i] + (0.5 * dt) * k2[i];
    Model::f(p, xt, u, k3);
#pragma unroll
    for (int i = 0; i < NX; ++i) xt[i] = x[i] + dt * k3[i];
    Model::f(p, xt, u, k4);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = x[i] + (dt / 6) * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
  }
  // the same integrators on hoisted constants
  DEV static void step(const DynCtx &c, const double *x, const double *u, double *xn) {
    constexpr int NX = Model::NX;
    const double *p = c.mp;
    double k1[NX];
    Model::f(p, x, u, k1);
    if (c.integrator == CDDP_HIP_EULER) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.dt * k1[i];
      return;
    }
    double xt[NX], k2[NX];
    if (c.integrator == CDDP_HIP_HEUN) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.dt * k1[i];
      Model::f(p, xt, u, k2);
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.hdt * (k1[i] + k2[i]);
      return;
    }
    double k3[NX];
    if (c.integrator == CDDP_HIP_RK3) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.hdt * k1[i];
      Model::f(p, xt, u, k2);
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = (x[i] - c.dt * k1[i]) + c.dt2 * k2[i];
      Model::f(p, xt, u, k3);
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.dt6 * ((k1[i] + 4.0 * k2[i]) + k3[i]);
      return;
    }
    double k4[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.hdt * k1[i];
    Model::f(p, xt, u, k2);
#pragma unroll
    for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.hdt * k2[i];
    Model::f(p, xt, u, k3);
#pragma unroll
    for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.dt * k3[i];
    Model::f(p, xt, u, k4);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.dt6 * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
  }
};

// ---- one step of the two-role rollout's producer (kernels_lean.hpp::k_forward_ipddp_pc) ----------------------------------------
// The integrator is a TEMPLATE parameter: the producer switches on ProblemDev::integrator once, in front of its step loop, so the
// loop holds one integrator's code and no test of it.  Each integrator is the expressions of Stepper::step(const DynCtx &, ...)
// above, in the same order.  A plant with a trig policy takes its sines and cosines through TrigFlagged: the step is then ONE
// basic block, and `*redo` tells the caller that some angle of the step was outside the fast routine's range (or not finite), in
// which case the caller evaluates the step again with Stepper::step, whose plant_sincos serves such angles from the libm -- lanes
// in range get the values they had, lanes out of range the values the checked path always gave them.  A plant without the policy
// (or a caller that passes FLAGGED = false) keeps the per-call checks and never sets the flag.
template <class Model, bool FLAGGED, class Trig>
DEV void roll_f(const double *p, const double *x, const double *u, double *xd, const Trig tg) {
  if constexpr (FLAGGED) Model::f(p, x, u, xd, tg);
  else Model::f(p, x, u, xd);
}
template <class Model, int INTEG, bool FLAGGED = HasTrigPolicy<Model>::value>
DEV void roll_step(const DynCtx &c, const double *x, const double *u, double *xn, bool *redo) {
  if constexpr (Model::kDiscrete) {
    Stepper<Model>::step(c, x, u, xn);
  } else {
    constexpr int NX = Model::NX;
    const double *p = c.mp;
    const TrigFlagged tg{redo};
    double k1[NX];
    roll_f<Model, FLAGGED>(p, x, u, k1, tg);
    if constexpr (INTEG == CDDP_HIP_EULER) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.dt * k1[i];
    } else if constexpr (INTEG == CDDP_HIP_HEUN) {
      double xt[NX], k2[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.dt * k1[i];
      roll_f<Model, FLAGGED>(p, xt, u, k2, tg);
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.hdt * (k1[i] + k2[i]);
    } else if constexpr (INTEG == CDDP_HIP_RK3) {
      double xt[NX], k2[NX], k3[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.hdt * k1[i];
      roll_f<Model, FLAGGED>(p, xt, u, k2, tg);
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = (x[i] - c.dt * k1[i]) + c.dt2 * k2[i];
      roll_f<Model, FLAGGED>(p, xt, u, k3, tg);
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.dt6 * ((k1[i] + 4.0 * k2[i]) + k3[i]);
    } else {
      double xt[NX], k2[NX], k3[NX], k4[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.hdt * k1[i];
      roll_f<Model, FLAGGED>(p, xt, u, k2, tg);
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.hdt * k2[i];
      roll_f<Model, FLAGGED>(p, xt, u, k3, tg);
#pragma unroll
      for (int i = 0; i < NX; ++i) xt[i] = x[i] + c.dt * k3[i];
      roll_f<Model, FLAGGED>(p, xt, u, k4, tg);
#pragma unroll
      for (int i = 0; i < NX; ++i) xn[i] = x[i] + c.dt6 * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
    }
  }
}

}  // namespace cddp_dev
