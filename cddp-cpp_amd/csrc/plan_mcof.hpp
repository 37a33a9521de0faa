// Monte-Carlo evaluation of a solved plan with the estimator in the loop: the ONE statement of what cddp_hip_mc_sample_meas_noise /
// cddp_hip_plan_montecarlo_of add to plan_mc.hpp (include/cddp_hip.h "Monte-Carlo evaluation of a solved plan under output feedback").
// Plain functions, host and device: the kernels of inst_mcof.hip call them, tests/cpp/test_plan_mcof.cpp compiles this file with
// g++ -ffp-contract=off, checks it on written-out sums and writes the files the GPU tests compare with bit for bit.
// Needs plan_mc.hpp (and through it mppi.hpp) only.  A matrix argument is a pointer of any address space with a stride: element (i, j) of
// a matrix of `cols` columns is M[(i * cols + j) * st] -- 1 for a host or batch-major array, 64 or 4 for a stack read in place.
//
//   normals     the measurement normal of step t, row r of sample c of trajectory b is element e = nx + N (nu + nx) + t ny + r of
//               plan_mc.hpp's generator at the same (seed, stream, b, c): past the end of plan_mc.hpp's elements, so the initial, actuator
//               and process noise of a sample are those of cddp_hip_plan_montecarlo.  keep_nominal zeroes them for sample 0 as well.  The
//               walk over t, r is ascending in e: a Draw of its own draws each pair once.
//   rollout     plan_mc.hpp's, with xh[nx] = the estimate of x - X_t next to x, xh = 0 at the start.  At every step t = 0 .. N:
//     1. dx[j] = x[j] - X_t[j]
//     2. y[r] = s + n[r], s = 0; s += C[r][j] * dx[j] (j ascending); n[r] = sd[r] * z, sd[r] = sqrt(v[r]) rounded correctly on the host
//     3. inn[r] = y[r] - p, p = 0; p += C[r][j] * xh[j]: every inn from the xh held before step 4
//     4. xh[i] = xh[i] + s, s = 0; s += L_t[i][r] * inn[r] (r ascending)
//     5. e[i] = dx[i] - xh[i]: its moments by plan_mc.hpp's tree sum, moment_mean and moment_cov
//     6. t < N: fb[i] = s, s = 0; s += K_t[i][j] * xh[j]; u[i] = (U_t[i] + eps[i]) + fb[i]; box, cost, rows, step(s), process noise as in
//        plan_mc.hpp; xp[i] = s, s = 0; s += A_t[i][j] * xh[j] (j ascending), then s += B_t[i][j] * fb[j] (j ascending); xh = xp.
//        The prediction takes the unclipped, noise-free fb: cddp_hip_plan_kalman's model.
#pragma once
#include <cstdint>

#include "plan_mc.hpp"

namespace cddp_mcof {

DEV uint32_t elem_y(int nx, int nu, int N, int ny, int t, int r) {
  return (uint32_t)nx + (uint32_t)N * (uint32_t)(nu + nx) + (uint32_t)t * (uint32_t)ny + (uint32_t)r;
}

// steps 2 and 3 for one row c = C[r] (contiguous): the innovation of the row from dx, its noise n = sd[r] * z and the estimate before the update
template <class P>
DEV double innovation(int nx, P c, double n, const double *dx, const double *xh) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < nx; ++j) s += c[j] * dx[j];
  const double y = s + n;
  double p = 0.0;
#pragma unroll
  for (int j = 0; j < nx; ++j) p += c[j] * xh[j];
  return y - p;
}

// step 4, one term of every row's sum: acc[i] += L_t[i][r] * inn.  acc starts at 0 and the rows r come ascending, so acc[i] ends as the
// stated s; the innovations are all formed before update_end touches xh
template <class P>
DEV void update_add(int nx, int ny, int r, P Lt, double inn, double *acc) {
#pragma unroll
  for (int i = 0; i < nx; ++i) acc[i] += Lt[i * ny + r] * inn;
}
DEV void update_end(int nx, const double *acc, double *xh) {
#pragma unroll
  for (int i = 0; i < nx; ++i) xh[i] = xh[i] + acc[i];
}

// step 6's feedback: fb = K_t xh
template <class P>
DEV void feedback(int nx, int nu, P Kt, int st, const double *xh, double *fb) {
#pragma unroll
  for (int i = 0; i < nu; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < nx; ++j) s += Kt[(i * nx + j) * st] * xh[j];
    fb[i] = s;
  }
}

// step 6's prediction: xp = A_t xh + B_t fb in one sum per row (xp must not alias xh)
template <class P>
DEV void predict(int nx, int nu, P At, P Bt, int st, const double *xh, const double *fb, double *xp) {
#pragma unroll
  for (int i = 0; i < nx; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < nx; ++j) s += At[(i * nx + j) * st] * xh[j];
#pragma unroll
    for (int j = 0; j < nu; ++j) s += Bt[(i * nu + j) * st] * fb[j];
    xp[i] = s;
  }
}

}  // namespace cddp_mcof
