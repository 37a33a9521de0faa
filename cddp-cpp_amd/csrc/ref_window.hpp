// The reference window of a path-following MPC step (cddp_hip_mpc_set_reference_path): the ONE statement of which path rows a window
// row reads and how it blends them.  Plain function, host and device: the window kernel (inst_ref.hip) runs it
// per element, and tests/cpp/test_ref_window.cpp compiles this file with g++ -ffp-contract=off and prints its windows.
//
//   window row t of cursor k (t = 0 .. N), path of L rows p_0 .. p_{L-1}:
//     pos = (double)(k + t) * rows_per_step;   i = floor(pos);   a = pos - i
//     i >= L - 1:  p_{L-1}[e]                                   (past the end the window holds the last row)
//     otherwise:   p_i[e] + a * (p_{i+1}[e] - p_i[e])            (product rounded, then the sum: no FMA; a == 0 gives p_i[e])
//
// The goal of the window is its row N.  Angles are blended like any other element: wrapping them is the caller's business.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define CDDP_REF_HD __host__ __device__ __forceinline__
#else
#define CDDP_REF_HD inline
#endif

namespace cddp_ref {

// element e of window row t.  L >= 1, k >= 0, t >= 0, rows_per_step > 0 and finite (checked when the path is bound); 0 <= e < nx.
// Every index formed is in [0, L - 1]: pos < L - 1 is tested in double BEFORE the conversion to an integer (a product that overflowed
// to +inf, or is beyond the integer range, takes the last row), and then floor(pos) + 1 <= L - 1.
CDDP_REF_HD double window_elem(const double *path, long long L, int nx, long long k, double rows_per_step, int t, int e) {
  const double pos = (double)(k + (long long)t) * rows_per_step;
  if (!(pos < (double)(L - 1))) return path[(size_t)(L - 1) * (size_t)nx + (size_t)e];
  const long long i = (long long)pos;            // pos >= 0: truncation is floor
  if (i >= L - 1) return path[(size_t)(L - 1) * (size_t)nx + (size_t)e];   // ((double)(L - 1) rounded up, L > 2^53)
  const double a = pos - (double)i;
  const double p0 = path[(size_t)i * (size_t)nx + (size_t)e], p1 = path[(size_t)(i + 1) * (size_t)nx + (size_t)e];
  return p0 + a * (p1 - p0);
}

}  // namespace cddp_ref
