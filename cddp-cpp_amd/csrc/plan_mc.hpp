// Monte-Carlo closed-loop evaluation of a solved plan under noise: the ONE statement of the arithmetic of cddp_hip_mc_sample_noise /
// cddp_hip_plan_montecarlo (include/cddp_hip.h "Monte-Carlo evaluation of a solved plan").  Plain functions, host and device: the kernels
// of inst_mc.hip call them or restate them with cross-lane operations, tests/cpp/test_plan_mc.cpp compiles this file with
// g++ -ffp-contract=off, checks it on written-out sums and writes the noise files the GPU tests compare with bit for bit.
// Needs mppi.hpp (the generator) only.
//
//   normals     sample c of (global) trajectory b draws cddp_mppi::normal(seed, stream, b, c, e) with the elements
//                 e = i                          i < nx   initial state
//                 e = nx + t (nu + nx) + i       i < nu   actuator noise of step t
//                 e = nx + t (nu + nx) + nu + i  i < nx   process noise of step t
//               A source without a factor draws nothing and the indices stay where they are: switching one source off does not change
//               the others.  Elements 2j and 2j + 1 are the two halves of one pair (a pair may straddle a step when nx + nu is odd); Draw
//               keeps the last pair, so a walk in ascending e draws every pair once.  keep_nominal: sample 0 takes z = 0 everywhere.
//               An MPPI call with the same (seed, stream) shares this counter space (mppi.hpp: e = t nu + i of candidate c): give the two
//               different streams when their draws must be independent.
//   colour      v[i] = s, s = 0; s += L[i][j] * z[j], j ascending, j <= i (L row-major [n][n], only the lower triangle is read)
//   rollout     x[i] = xbase[i] + v0[i]; per step: uc = U_t + eps; u = uc + K_t (x - X_t) (s = 0; j ascending: cddp_hip_score_rollouts'
//               FEEDBACK line); the plant's box; cost += running cost; v_t = the path rows folded from 0, viol = dmax(viol, v_t); the
//               step(s); x[i] = xn[i] + w[i] with Lw.  Then the terminal cost and the terminal inequality rows as v_N.
//   tree sum    c = 64 k + l, absent lanes +0.0; for m = 1, 2, 4, 8, 16, 32: v[l] = v[l] + v[l ^ m]; lane 0 holds the chunk total; chunk
//               totals are added with k ascending from chunk 0's.
//   moments     d_c = x_c,t - X_t: m1[i] = tree(d_c[i]), mean = m1[i] / S, q[i][j] = tree(d_c[i] * d_c[j]) (j <= i),
//               cov = (q[i][j] - (m1[i] * m1[j]) / S) / (S - 1), 0 at S == 1, mirrored; the controls likewise from the applied u - U_t.
//   stats       [8] = n_finite (cost and viol finite), n_viol (viol > viol_tol), cost_mean = tree(cost) / S, cost_var =
//               tree((cost_c - cost_mean)^2) / (S - 1) (0 at S == 1), cost_min, cost_max (by <, c ascending from sample 0), viol_mean =
//               tree(viol) / S, viol_max (as cost_max).  Non-finite values propagate, nothing is special-cased.
#pragma once
#include <cstdint>

#include "mppi.hpp"

namespace cddp_mc {

constexpr int kMaxSamples = 1024;   // one workgroup holds the samples of a trajectory

DEV uint32_t elem_x0(int i) { return (uint32_t)i; }
DEV uint32_t elem_u(int nx, int nu, int t, int i) { return (uint32_t)nx + (uint32_t)t * (uint32_t)(nu + nx) + (uint32_t)i; }
DEV uint32_t elem_w(int nx, int nu, int t, int i) { return (uint32_t)nx + (uint32_t)t * (uint32_t)(nu + nx) + (uint32_t)nu + (uint32_t)i; }

// the normals of one sample, walked in ascending e: a pair is drawn once and both halves are used
struct Draw {
  uint64_t seed; uint32_t stream, b, c, have; bool zero; cddp_mppi::Pair p;
  DEV void begin(uint64_t seed_, uint32_t stream_, uint32_t b_, uint32_t c_, bool zero_) {
    seed = seed_; stream = stream_; b = b_; c = c_; zero = zero_; have = 0xffffffffu; p.even = 0.0; p.odd = 0.0;
  }
  DEV double get(uint32_t e) {
    const uint32_t j = e >> 1;
    if (j != have) { p = cddp_mppi::normal_pair(seed, stream, b, c, j); have = j; }
    const double z = (e & 1u) ? p.odd : p.even;
    return zero ? 0.0 : z;
  }
};

// v = L z over the lower triangle, L row-major [n][n] (entries above the diagonal are not read)
DEV void colour(int n, const double *L, const double *z, double *v) {
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    for (int j = 0; j <= i; ++j) s += L[i * n + j] * z[j];
    v[i] = s;
  }
}

DEV double moment_mean(double m1, int S) { return m1 / (double)S; }
DEV double moment_cov(double q, double m1i, double m1j, int S) { return S == 1 ? 0.0 : (q - (m1i * m1j) / (double)S) / (double)(S - 1); }

DEV bool below(double a, double b) { return a < b; }   // the one comparison of min and max

#ifdef CDDP_TRIG_HOST   // the sums over the samples written out for the host; the kernel restates them with cross-lane moves (inst_mc.hip)
// the tree sum of v[0 .. S), as the kernel's lanes hold it
inline double tree_sum(int S, const double *v) {
  double total = 0.0;
  for (int k = 0; 64 * k < S; ++k) {
    double w[64], n[64];
    for (int l = 0; l < 64; ++l) w[l] = 64 * k + l < S ? v[64 * k + l] : 0.0;
    for (int m = 1; m < 64; m <<= 1) {
      for (int l = 0; l < 64; ++l) n[l] = w[l] + w[l ^ m];
      for (int l = 0; l < 64; ++l) w[l] = n[l];
    }
    total = k == 0 ? w[0] : total + w[0];
  }
  return total;
}

// stats[8] of one trajectory from its S records
inline void stats(int S, const double *cost, const double *viol, double viol_tol, double *out) {
  int n_finite = 0, n_viol = 0;
  for (int c = 0; c < S; ++c) {
    if (cddp_mppi::is_finite(cost[c]) && cddp_mppi::is_finite(viol[c])) ++n_finite;
    if (viol[c] > viol_tol) ++n_viol;
  }
  const double mean = tree_sum(S, cost) / (double)S;
  double var = 0.0;
  if (S > 1) {
    double dev[kMaxSamples];
    for (int c = 0; c < S; ++c) { const double e = cost[c] - mean; dev[c] = e * e; }
    var = tree_sum(S, dev) / (double)(S - 1);
  }
  double cmin = cost[0], cmax = cost[0], vmax = viol[0];
  for (int c = 1; c < S; ++c) {
    if (below(cost[c], cmin)) cmin = cost[c];
    if (below(cmax, cost[c])) cmax = cost[c];
    if (below(vmax, viol[c])) vmax = viol[c];
  }
  out[0] = (double)n_finite; out[1] = (double)n_viol; out[2] = mean; out[3] = var; out[4] = cmin; out[5] = cmax;
  out[6] = tree_sum(S, viol) / (double)S; out[7] = vmax;
}
#endif

}  // namespace cddp_mc
