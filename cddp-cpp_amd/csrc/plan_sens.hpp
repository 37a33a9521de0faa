// Linear response of a closed-loop plan to its initial state: the ONE statement of the two step bodies that the sensitivity kernels
// (inst_sens.hip) run, on register arrays, for RV vectors at once.  Plain templates, host and device, no other header needed:
// tests/cpp/test_plan_sens.cpp compiles this file with g++ -ffp-contract=off and checks both bodies bitwise against the sums written out.
//
//   forward (JVP):  du = K dx;  dx' = A dx + B du                 adjoint (VJP):  mu = gU + B^T lam;  lam' = gX + A^T lam + K^T mu
//
// The matrices come through accessors, A(i, j) = A_t[i][j] (row-major, as cddp_hip_get_linearization / cddp_hip_get_gains return them):
// a kernel passes registers it filled ahead of the step, or loads from the stack; either way every element is fetched once per step
// and used for all RV vectors.  Per vector the order of every sum is the one include/cddp_hip.h fixes: a zero accumulator, terms
// ascending, the B / K terms on the accumulator of the A terms.
#pragma once

#if defined(__HIPCC__)
#define CDDP_SENS_HD __host__ __device__ __forceinline__
#else
#define CDDP_SENS_HD inline
#endif

namespace cddp_sens {

// A row-major matrix held in an array (registers in a kernel): the accessor of the prefetching kernels and of the CPU test
struct Dense {
  const double *m; int cols;
  CDDP_SENS_HD double operator()(int i, int j) const { return m[i * cols + j]; }
};

// du[r] = K dx[r];  dxn[r] = A dx[r] + B du[r]
template <int NX, int NU, int RV, class MA, class MB, class MK>
CDDP_SENS_HD void jvp_step(const MA &A, const MB &Bm, const MK &K, const double (&dx)[RV][NX], double (&du)[RV][NU], double (&dxn)[RV][NX]) {
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    double s[RV];
#pragma unroll
    for (int r = 0; r < RV; ++r) s[r] = 0.0;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const double k = K(i, j);
#pragma unroll
      for (int r = 0; r < RV; ++r) s[r] += k * dx[r][j];
    }
#pragma unroll
    for (int r = 0; r < RV; ++r) du[r][i] = s[r];
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    double s[RV];
#pragma unroll
    for (int r = 0; r < RV; ++r) s[r] = 0.0;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const double a = A(i, j);
#pragma unroll
      for (int r = 0; r < RV; ++r) s[r] += a * dx[r][j];
    }
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const double b = Bm(i, k);
#pragma unroll
      for (int r = 0; r < RV; ++r) s[r] += b * du[r][k];
    }
#pragma unroll
    for (int r = 0; r < RV; ++r) dxn[r][i] = s[r];
  }
}

// mu[r] = gu[r] + B^T lam[r];  lamn[r] = gx[r] + A^T lam[r] + K^T mu[r].  HAVE_GU / HAVE_GX false: the cotangent is absent (zeros) and the
// sum is stored as it is -- gu / gx are not read.
template <int NX, int NU, int RV, bool HAVE_GX, bool HAVE_GU, class MA, class MB, class MK>
CDDP_SENS_HD void vjp_step(const MA &A, const MB &Bm, const MK &K, const double (&lam)[RV][NX], const double (&gx)[RV][NX], const double (&gu)[RV][NU],
                           double (&mu)[RV][NU], double (&lamn)[RV][NX]) {
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    double s[RV];
#pragma unroll
    for (int r = 0; r < RV; ++r) s[r] = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double b = Bm(i, k);
#pragma unroll
      for (int r = 0; r < RV; ++r) s[r] += b * lam[r][i];
    }
#pragma unroll
    for (int r = 0; r < RV; ++r) mu[r][k] = HAVE_GU ? gu[r][k] + s[r] : s[r];
  }
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    double s[RV];
#pragma unroll
    for (int r = 0; r < RV; ++r) s[r] = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double a = A(i, j);
#pragma unroll
      for (int r = 0; r < RV; ++r) s[r] += a * lam[r][i];
    }
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const double kk = K(k, j);
#pragma unroll
      for (int r = 0; r < RV; ++r) s[r] += kk * mu[r][k];
    }
#pragma unroll
    for (int r = 0; r < RV; ++r) lamn[r][j] = HAVE_GX ? gx[r][j] + s[r] : s[r];
  }
}

}  // namespace cddp_sens
