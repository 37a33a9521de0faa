// Sampling-based plan refinement (MPPI): the ONE statement of the arithmetic of cddp_hip_sample_controls / cddp_hip_mppi_blend /
// cddp_hip_mppi_refine (include/cddp_hip.h "sampling-based plan refinement").  Plain functions, host and device: the kernels of
// inst_mppi.hip call them, tests/cpp/test_mppi.cpp compiles this file with g++ -ffp-contract=off and checks it on known answers, hand-built
// records and moments, and writes the files the GPU tests compare with bit for bit.  Needs dev_trig.hpp only.
//
//   generator   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53 / 0xCD9E8D57,
//               key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.  Counter-based: nothing is stored, a number is a function of its index.
//   normal pair element e = t * nu + i of candidate c of trajectory b belongs to pair j = e >> 1; counter = (j, c, b_global, stream),
//               key = (seed low, seed high); the four words r0..r3 give m1 = (r1:r0) >> 11, m2 = (r3:r2) >> 11, u1 = (m1 + 1) 2^-53 in
//               (0, 1], u2 = m2 2^-53 in [0, 1), rad = sqrt(-2 log_fast(u1)), (s, co) = sincos_fast(2 pi u2) (Box-Muller); the even
//               element takes rad * co, the odd one rad * s.  Both arguments lie inside the fast ranges of dev_trig.hpp by construction.
//   candidate   u_c = mean + sigma[i] * z, then fmin(fmax(u, lower[i]), upper[i]) with a box; keep_mean: candidate 0 takes z = 0
//   weights     admissible = cost and viol finite and viol <= viol_tol (score_select.hpp's predicate); rho = the lowest admissible cost;
//               q = (cost_c - rho) / lambda; a_c = q <= 700 ? exp_fast(-q) : 0 (0 for an inadmissible c); eta = sum a_c (c ascending,
//               at least 1); w_c = a_c / eta; ess = 1 / sum w_c^2.  None admissible: every w_c = 0, n_adm = rho = ess = 0.
//   blend       s = 0; for c ascending s += w_c * (u_c - mean); mean' = mean + s, clipped to the box when there is one; a trajectory
//               without an admissible candidate keeps its mean as it is.
#pragma once
#include <cstdint>

#include "dev_trig.hpp"

namespace cddp_mppi {

struct Words { uint32_t w[4]; };

DEV Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  Words o; o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// the two uniforms of a draw: u1 in (0, 1], u2 in [0, 1), both multiples of 2^-53
DEV double uniform_open0(uint32_t lo, uint32_t hi) { return ((double)((((uint64_t)hi << 32) | lo) >> 11) + 1.0) * 0x1p-53; }
DEV double uniform_open1(uint32_t lo, uint32_t hi) { return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53; }

struct Pair { double even, odd; };   // the normals of elements 2j and 2j + 1

DEV Pair box_muller(const Words &r) {
  const double u1 = uniform_open0(r.w[0], r.w[1]), u2 = uniform_open1(r.w[2], r.w[3]);
  const double rad = __builtin_sqrt(-2.0 * cddp_dev::log_fast(u1));
  const cddp_dev::SinCosPair sc = cddp_dev::sincos_fast(0x1.921fb54442d18p+2 * u2);
  Pair o; o.even = rad * sc.c; o.odd = rad * sc.s;
  return o;
}

// pair j of candidate c of (global) trajectory b in noise stream `stream`
DEV Pair normal_pair(uint64_t seed, uint32_t stream, uint32_t b, uint32_t c, uint32_t j) {
  return box_muller(philox4x32_10(j, c, b, stream, (uint32_t)seed, (uint32_t)(seed >> 32)));
}

// the normal of element e alone (the kernels draw a pair once and use both halves)
DEV double normal(uint64_t seed, uint32_t stream, uint32_t b, uint32_t c, uint32_t e) {
  const Pair p = normal_pair(seed, stream, b, c, e >> 1);
  return (e & 1u) ? p.odd : p.even;
}

// candidate control from the mean and a normal; box false: lower and upper are not read
DEV double candidate(double mean, double sigma, double z, bool box, double lower, double upper) {
  const double u = mean + sigma * z;
  return box ? __builtin_fmin(__builtin_fmax(u, lower), upper) : u;
}

DEV bool is_finite(double v) { return v - v == 0.0; }
DEV bool admissible(double cost, double viol, double viol_tol) { return is_finite(cost) && is_finite(viol) && viol <= viol_tol; }

// w[c] for c < ncand (w may alias nothing of cost / viol); viol == nullptr: every violation is 0.  stats: n_adm, rho, ess
DEV void weights(int ncand, const double *cost, const double *viol, double viol_tol, double lambda, double *w, double *stats) {
  int n_adm = 0;
  double rho = 0.0;
  for (int c = 0; c < ncand; ++c) {
    if (!admissible(cost[c], viol ? viol[c] : 0.0, viol_tol)) continue;
    if (n_adm == 0 || cost[c] < rho) rho = cost[c];
    ++n_adm;
  }
  if (n_adm == 0) {
    for (int c = 0; c < ncand; ++c) w[c] = 0.0;
    stats[0] = 0.0; stats[1] = 0.0; stats[2] = 0.0;
    return;
  }
  double eta = 0.0;
  for (int c = 0; c < ncand; ++c) {
    double a = 0.0;
    if (admissible(cost[c], viol ? viol[c] : 0.0, viol_tol)) {
      const double q = (cost[c] - rho) / lambda;
      a = q <= 700.0 ? cddp_dev::exp_fast(-q) : 0.0;
    }
    w[c] = a;
    eta += a;
  }
  double sq = 0.0;
  for (int c = 0; c < ncand; ++c) {
    const double wc = w[c] / eta;
    w[c] = wc;
    sq += wc * wc;
  }
  stats[0] = (double)n_adm; stats[1] = rho; stats[2] = 1.0 / sq;
}

// one term of the blend's sum, and its end
DEV void blend_add(double &s, double w, double u_c, double mean) { s += w * (u_c - mean); }
DEV double blend_end(double mean, double s, bool box, double lower, double upper) {
  const double u = mean + s;
  return box ? __builtin_fmin(__builtin_fmax(u, lower), upper) : u;
}

}  // namespace cddp_mppi
