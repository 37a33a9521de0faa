// Kalman filter along a plan's linearisation and the covariance of the plan under output feedback: the ONE statement of the step bodies
// that the filter kernel (inst_kf.hip) runs.  Plain templates, host and device: tests/cpp/test_plan_kf.cpp compiles this file with
// g++ -ffp-contract=off and checks every body bitwise against the sums written out.
//
// The measurement update takes the rows of C one at a time (diagonal measurement noise): for row r, with c = C[r] and S the covariance so far,
//   h = S c;   s = v_r + c . h;   g = h / s;   S' = S - g h^T - h g^T + s g g^T;   G += h g^T
// (the symmetric three-term Joseph form; G, a sum of rank-one terms, is what the update has taken off S and so what the estimate has gained).
// The time update and the control covariance are plan_cov.hpp's bodies with other operands:
//   Sm' = A Sf A^T + W + B Wu B^T  (steps 4, 5 with A for Acl),   Xm' = Acl Xh Acl^T  (steps 1, 4, 5),   SU = K Xh K^T + Wu  (steps 2, 3).
//
// The bodies are written per OWNER i (a group of lanes of the kernel owns row i of S, of G and of the gain), on accessors M(i, j) = M[i][j]
// and vectors V(j): a kernel passes its LDS buffers, the CPU test passes arrays.  Every sum is the one include/cddp_hip.h fixes: a stated
// start value, the index ascending.  Symmetric results are computed for j <= i and mirrored by the caller.  True division throughout.
#pragma once

#include "plan_cov.hpp"

#define CDDP_KF_HD CDDP_COV_HD

namespace cddp_kf {

// A vector in an array: a row of C for the CPU test and for the kernel (the same address for every lane when C is shared)
struct Row {
  const double *p;
  CDDP_KF_HD double operator()(int j) const { return p[j]; }
};

// Step U1, element i of h = S c:  s = 0;  for j ascending  s += S[i][j] * c[j].
// The gain element L[i][r] is the same sum over the posterior, divided by v_r (step L).
template <int NX, class MS, class VC>
CDDP_KF_HD double h_elem(int i, const MS &S, const VC &c) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < NX; ++j) s += S(i, j) * c(j);
  return s;
}

// Step U2, the innovation variance of the row:  s = v;  for j ascending  s += c[j] * h[j].   The row FAILS unless s > 0.
template <int NX, class VC, class VH>
CDDP_KF_HD double innovation(double v, const VC &c, const VH &h) {
  double s = v;
#pragma unroll
  for (int j = 0; j < NX; ++j) s += c(j) * h(j);
  return s;
}

// Steps U3 - U5, the elements j <= i of row i of S' and of G:  g[i] = h[i] / s,  g[j] = h[j] / s;
//   e = S[i][j];  e -= g[i] * h[j];  e -= h[i] * g[j];  q = s * g[i];  e += q * g[j];   Sout(j, e)
//   G[i][j] += h[i] * g[j]                                                             (grow[j], j <= i; the rest is left alone)
template <int NX, class VH, class MS, class SW>
CDDP_KF_HD void joseph_row(int i, double s, const VH &h, const MS &S, const SW &Sout, double (&grow)[NX]) {
  const double hi = h(i), gi = hi / s, q = s * gi;
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    if (j <= i) {
      const double hj = h(j), gj = hj / s;
      double e = S(i, j);
      e -= gi * hj;
      e -= hi * gj;
      e += q * gj;
      Sout(j, e);
      grow[j] += hi * gj;
    }
  }
}

}  // namespace cddp_kf
