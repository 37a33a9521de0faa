// Extended Kalman filter for a batch of trajectories with one of the built-in plants as its model (include/cddp_hip.h "extended Kalman
// filter on the device"): the ONE statement of the step bodies that the filter kernels (inst_ekf.hip) run.  Plain templates, host and
// device: tests/cpp/test_ekf.cpp compiles this file with g++ -ffp-contract=off and tests/plan_ekf_ref.py restates it in numpy; both
// comparisons are bitwise.
//
// The covariance algebra is plan_kf.hpp's row-at-a-time Joseph update and plan_cov.hpp's  A S A^T + W + B Wu B^T  with other operands;
// what is new here is the state estimate next to the covariance (the innovation of a row, e = y_r - c_r . xh) and the relinearisation:
// A = I + h Fx, B = h Fu at the estimate and the clipped control, the solver's own convention (kernels.hpp, k_derivs).
//
// One trajectory is one sequential walk (a lane of the kernel, a loop iteration of the CPU test).  Its matrices are reached through
// Mat<TL>: element (i, j) at p[(i * cols + j) * TL] -- TL lanes side by side in LDS, TL = 1 for an array.  Every sum is the one
// include/cddp_hip.h fixes: a stated start value, the index ascending.  True division throughout.
#pragma once

#if !defined(__HIPCC__)
#include <cmath>
#endif

#include "plan_kf.hpp"

#define CDDP_EKF_HD CDDP_COV_HD

namespace cddp_ekf {

template <int TL>
struct Mat {
  double *p; int cols;
  CDDP_EKF_HD double operator()(int i, int j) const { return p[(i * cols + j) * TL]; }
  CDDP_EKF_HD void set(int i, int j, double v) const { p[(i * cols + j) * TL] = v; }
};

template <int NN>
struct Vec {
  const double (&r)[NN];
  CDDP_EKF_HD double operator()(int j) const { return r[j]; }
};

enum { kRowOk = 0, kRowSkipped = 1, kRowFailed = 2 };

// One measurement row (steps 1 - 7 of the header) on the estimate xh and the symmetric P, in place:
//   h[i] = sum_j P[i][j] c[j] from 0;   s = v + sum_j c[j] h[j];   m = sum_j c[j] xh[j] from 0;   e = y - m;   g = h / s;
//   xh[i] = xh[i] + g[i] * e;   P <- plan_kf.hpp's joseph_row for i ascending (elements j <= i, mirrored);   nis += (e * e) / s
// skip_nan: a NaN y leaves everything alone.  A row whose s is not > 0 (NaN included) changes nothing and reports kRowFailed.
// In place is safe: row i reads the elements (i, j <= i), and the rows before it have written (i' < i, j <= i') and the mirrors (j, i'),
// which lie on or above the diagonal of rows j <= i' < i.
template <int NX, int TL, class VC>
CDDP_EKF_HD int update_row(const VC &c, double v, double y, bool skip_nan, double (&xh)[NX], const Mat<TL> &P, double &nis) {
  if (skip_nan && y != y) return kRowSkipped;
  double h[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) h[i] = cddp_kf::h_elem<NX>(i, P, c);
  const Vec<NX> hv{h};
  const double s = cddp_kf::innovation<NX>(v, c, hv);
  if (!(s > 0.0)) return kRowFailed;
  double m = 0.0;
#pragma unroll
  for (int j = 0; j < NX; ++j) m += c(j) * xh[j];
  const double e = y - m;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const double g = h[i] / s;
    xh[i] = xh[i] + g * e;
  }
  double gsum[NX];   // (plan_kf.hpp's G, which this filter has no use for)
#pragma unroll
  for (int i = 0; i < NX; ++i) {
#pragma unroll
    for (int j = 0; j < NX; ++j) gsum[j] = 0.0;
    cddp_kf::joseph_row<NX>(i, s, hv, P, [&](int j, double q) { P.set(i, j, q); P.set(j, i, q); }, gsum);
  }
  nis += (e * e) / s;
  return kRowOk;
}

// The plant's clip of a control (plant_advance's line): only with a box
template <int NU>
CDDP_EKF_HD void clip(const double *lower, const double *upper, double (&u)[NU]) {
  if (lower) {
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] = fmin(fmax(u[i], lower[i]), upper[i]);
  }
}

// The relinearisation at (xh, u_s) into A and Bm, k_derivs' expressions:  a = h * Fx[i][j];  if (i == j) a += 1.0;   b = h * Fu[i][k]
template <class M, int TL>
CDDP_EKF_HD void linearise(double h, const double *p, const double *xh, const double *u, const Mat<TL> &A, const Mat<TL> &Bm) {
  constexpr int NX = M::NX, NU = M::NU;
  double Fx[NX * NX], Fu[NX * NU];
  M::jac(p, xh, u, Fx, Fu);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      double a = h * Fx[i * NX + j];
      if (i == j) a += 1.0;
      A.set(i, j, a);
    }
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) {
#pragma unroll
    for (int k = 0; k < NU; ++k) Bm.set(i, k, h * Fu[i * NU + k]);
  }
}

// P <- A P A^T + W + B Wu B^T, cddp_hip_plan_covariance's steps 4 and 5 with A for Acl: Y = A P row by row into Y, then the elements
// j <= i of row i of the result into P (which Y has replaced), mirrored.  Only the lower triangles of W and Wu are read.
template <int NX, int NU, int TL>
CDDP_EKF_HD void propagate(const Mat<TL> &A, const Mat<TL> &Bm, const Mat<TL> &P, const Mat<TL> &Y, const cddp_cov::SymLower &W, const cddp_cov::SymLower &Wu) {
  for (int i = 0; i < NX; ++i) {
    double a[1][NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) a[0][j] = A(i, j);
    cddp_cov::y_rows_to<NX, 1>(a, P, [&](int, int j, double v) { Y.set(i, j, v); });
  }
  for (int i = 0; i < NX; ++i) {
    double a[1][NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) a[0][j] = A(i, j);
    const int row[1] = {i};
    const auto put = [&](int, int j, double v) { P.set(i, j, v); P.set(j, i, v); };
    if (Wu.m) cddp_cov::next_rows_to<NX, NU, 1, true>(row, a, Y, W, Wu, Bm, put);
    else cddp_cov::next_rows_to<NX, NU, 1, false>(row, a, Y, W, Wu, Bm, put);
  }
}

// The prediction with control u (clipped in place): linearise at (xh, u_s), advance xh by one step of the plant, propagate P.
// STEP is Stepper<M> of dev_models.hpp (a template argument so that this header needs no more of it than M::jac).
template <class M, class STEP, int TL>
CDDP_EKF_HD void predict(int integrator, double h, const double *p, const double *lower, const double *upper, double (&xh)[M::NX], double (&u)[M::NU],
                         const Mat<TL> &P, const Mat<TL> &A, const Mat<TL> &Bm, const Mat<TL> &Y, const cddp_cov::SymLower &W, const cddp_cov::SymLower &Wu) {
  constexpr int NX = M::NX, NU = M::NU;
  clip<NU>(lower, upper, u);
  linearise<M, TL>(h, p, xh, u, A, Bm);
  double xn[NX];
  STEP::step(integrator, h, p, xh, u, xn);
#pragma unroll
  for (int i = 0; i < NX; ++i) xh[i] = xn[i];
  propagate<NX, NU, TL>(A, Bm, P, Y, W, Wu);
}

}  // namespace cddp_ekf
