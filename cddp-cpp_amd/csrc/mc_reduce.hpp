// The sums over the samples of the Monte-Carlo kernels (inst_mc.hip, inst_mcof.hip), restated with cross-lane moves: plan_mc.hpp's tree sum
// inside a wavefront, for one value and for the values of a step at once, the scans of stats, and the decoding of a triangle's entry
// number.  Every translation unit that includes this file gets its own copies (anonymous namespace).
#pragma once
#include "dev_linalg.hpp"
#include "plan_mc.hpp"

namespace cddp_dev {
namespace {

// the chunk total of plan_mc.hpp's tree sum, in every lane
DEV double wave_tree(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}
DEV double wave_min(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const double o = __shfl_xor(v, m, 64); v = cddp_mc::below(o, v) ? o : v; }
  return v;
}
DEV double wave_max(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const double o = __shfl_xor(v, m, 64); v = cddp_mc::below(v, o) ? o : v; }
  return v;
}

// The tree sums of N values at once.  At stage m a lane keeps one value of a pair and hands the other to lane l ^ m, which keeps that one: the
// lane that ends up with a value's total has added exactly the operands of the butterfly above, v[l] + v[l ^ m] at every stage (the same
// bits: an addition commutes), but a stage moves half as many words as the one before -- N + 6 moves instead of 6 N.  The total of value k
// ends in every lane whose low bits are k; a lone value takes the plain butterfly.
template <int N, int ST>
DEV void tree_stage(double *a, int lane) {
  if constexpr (ST < 6) {
    constexpr int m = 1 << ST, half = N / 2;
    if constexpr (N > 1) {
      const bool bit = ((lane >> ST) & 1) != 0;
#pragma unroll
      for (int k = 0; k < half; ++k) {
        const double send = bit ? a[2 * k] : a[2 * k + 1], keep = bit ? a[2 * k + 1] : a[2 * k];
        a[k] = keep + __shfl_xor(send, m, 64);
      }
    }
    if constexpr (N & 1) a[half] = a[N - 1] + __shfl_xor(a[N - 1], m, 64);
    tree_stage<(N + 1) / 2, ST + 1>(a, lane);
  }
}
constexpr int kTreeChunk = 32;   // values summed together: 32 doubles of registers while they are
// dst[k] = the chunk total of v[k] over the wavefront's live lanes, k < N (dst: the wavefront's row of partial sums in LDS)
template <int N, int C0 = 0>
DEV void tree_store(const double *v, int lane, bool live, double *dst) {
  constexpr int n = N - C0 < kTreeChunk ? N - C0 : kTreeChunk;
  double a[n];
#pragma unroll
  for (int i = 0; i < n; ++i) a[i] = live ? v[C0 + i] : 0.0;
  tree_stage<n, 0>(a, lane);
  if (lane < n) dst[C0 + lane] = a[0];
  if constexpr (C0 + n < N) tree_store<N, C0 + n>(v, lane, live, dst);
}
// the sums of one step over d (N deviations): m1 at dst[0 .. N), then q -- the lower triangle row by row, or with diag the N squares
template <int N>
DEV void put_group(const double *d, bool cov, bool diag, int lane, bool live, double *dst) {
  constexpr int T = N * (N + 1) / 2;
  if (cov && !diag) {
    double v[N + T];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      v[i] = d[i];
#pragma unroll
      for (int j = 0; j <= i; ++j) v[N + i * (i + 1) / 2 + j] = d[i] * d[j];
    }
    tree_store<N + T>(v, lane, live, dst);
  } else if (cov) {
    double v[2 * N];
#pragma unroll
    for (int i = 0; i < N; ++i) { v[i] = d[i]; v[N + i] = d[i] * d[i]; }
    tree_store<2 * N>(v, lane, live, dst);
  } else tree_store<N>(d, lane, live, dst);
}

// row i, column j <= i of the triangle whose entries are numbered row by row
DEV void tri_decode(int p, int &i, int &j) {
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= p) ++i;
  j = p - i * (i + 1) / 2;
}

}  // namespace
}  // namespace cddp_dev
