// Gain-design kernel of the resident handle: the finite-horizon LQR of the plan's linearisation for the caller's weights, the backward
// Riccati recursion in Joseph form  P_t = Qd + K_t^T Rd K_t + Acl_t^T P_{t+1} Acl_t,  K_t = -(Rd + B_t^T P_{t+1} B_t)^-1 B_t^T P_{t+1} A_t,
// Acl_t = A_t + B_t K_t, run backward from P_N = Qf.  The dual of inst_cov.hip's forward recursion, with a small Cholesky factorisation
// per step.  The arithmetic is plan_lqr.hpp's, fixed by include/cddp_hip.h.
//
// ONE WORKGROUP walks the horizon backward for a tile of TL trajectories (blockDim = (TL, NX)): lane x = trajectory, and the NX "owners"
// y each hold one index: row y of M and of P_t, row y of Quu (y < NU), column y of Qux / K_t / Acl_t / Y / T.  P lives in LDS as
// [NX][NX][TL] doubles, lane-consecutive.  Of the stacks an owner loads its column of A_t and all of B_t, where they lie (StackRef /
// Strided, as inst_cov.hip: wave-tiled rows or sub-tile-minor quads).  A step, six barriers:
//   1  read P:   row y of M = P B                                  -> the M buffer
//   2  read M:   row y < NU of Quu = B^T M + Rd (lower triangle)   -> the Quu buffer
//   3  read Quu, M, P:  EVERY owner factors Quu for itself (fully unrolled, L in registers: 28 doubles at nu = 7) -- the factor is needed
//      by all the columns, and nu^3 / 6 products per owner cost less than a barrier and a trip through LDS;  column y of Qux, the two
//      triangular solves, column y of K_t out (to K_out and / or the tiled gain stack);  column y of Acl, of Y = P Acl and of T = Rd K
//      into registers
//   4  column y of Y over the P buffer, column y of T over the M buffer (T [NU][NX] overlays M [NX][NU])
//   5  read Y, T:  the elements j <= y of row y of P_t into registers (Acl and K columns are still held)
//   6  P_t back, mirrored, and out
// TL = 64 up to nx = 8: an owner is a wavefront (its index is a scalar), at most 8 waves, two to a SIMD, 256 registers.  From nx = 10 on
// TL = 32 and two owners share a wavefront (the owner index is then a per-lane value that enters addresses and guards only, never a
// register index): 5 .. 7 waves on 256 registers each instead of 10 .. 14 on 128, and (14, 7) fits LDS -- with 64 trajectories its
// P + M/T + Quu would be 343 * 512 bytes = 171.5 KB of the 160 KB.  LDS: (NX NX + NX NU + NU NU) * 8 * TL bytes: 87.8 KB at (14, 7),
// 60.7 KB at (13, 4) (two groups per CU), 49.7 KB at (8, 3).  Registers and scratch per pair: profiles/r20_plan_tvlqr.md.
// A failed pivot (not > 0, NaN included) at step t marks the lane dead from then on: K_s = 0 and P_s = NaN are stored for s <= t,
// info = t + 1 of the first failure met (the largest such t); the lane keeps walking for the barriers, on whatever its buffers hold.
//
// Bounds: lanes beyond the batch (the last workgroup) walk along for the barriers on the rows of trajectory B - 1 and store nothing:
// every access is that of a trajectory b < B, and B - 1 lies in the workgroup's own 64-tile.  A stack access is (t < N, e < E, b), inside
// the N * E * NB * 64 doubles every stack is allocated with; the gain stack is written at (t < N, e < NU NX, b < B) of the same
// extent.  A batch-major access is row t <= N (P_out) or t < N (K_out) of trajectory b, inside the extents capi.hip has checked; Q / R /
// Qf are read at element (i, j <= i) of trajectory b (or of the one shared matrix); info at b.  LDS indices are (r < NX or NU,
// c < NX or NU, lane < TL) of buffers of exactly those extents.
#include "lqr_kernels.hpp"

#include "plan_lqr.hpp"

namespace cddp_dev {

namespace {

// A tile's view of a stack with E elements per step (inst_cov.hip's): element e of step t of lane l of the tile is at base[t * st + e * se + lo(l)]
template <int LAYOUT, int E>
struct StackRef {
  const double *p; size_t st; unsigned lo;
  static constexpr int se = LAYOUT == cddp_io::kT4 ? 4 : 64;
  __device__ StackRef(const double *base, int NB, int tile, int l) {
    p = base + cddp_io::internal(LAYOUT, 0, 0, 0, NB, E, 0, tile * 64);
    st = cddp_io::internal(LAYOUT, 0, 0, 1, NB, E, 0, 0);
    lo = (unsigned)cddp_io::internal(LAYOUT, 0, 0, 0, 1, E, 0, l);
  }
};

// accessor of plan_lqr.hpp that loads from the stack: p = the tile's first element of the step
template <int SE>
struct Strided {
  const double *p; unsigned lo; int cols;
  __device__ __forceinline__ double operator()(int i, int j) const { return p[(i * cols + j) * SE + lo]; }
};

// accessor of an LDS buffer [rows][cols][TL] through the lane's own column
template <int TL>
struct Lds {
  const double *p; int cols;
  __device__ __forceinline__ double operator()(int i, int j) const { return p[(i * cols + j) * TL]; }
};

// trajectories per workgroup: from nx = 10 on two owners share a wavefront (the head comment)
template <int NX>
struct Tile {
  static constexpr int kLanes = NX >= 10 ? 32 : 64;
  static constexpr int kThreads = kLanes * NX;
};

template <int NX, int NU, int LAYOUT>
__global__ __launch_bounds__(Tile<NX>::kThreads) void k_plan_lqr(SensStacks s, LqrArgs a) {
  static_assert(NU <= NX, "the owners y < NU own the rows of Quu");
  static_assert(Tile<NX>::kThreads <= 1024 && 64 % Tile<NX>::kLanes == 0, "a workgroup lies inside one 64-tile of the stacks");
  constexpr int TL = Tile<NX>::kLanes;
  __shared__ double sP[NX * NX * TL], sM[NX * NU * TL], sQ[NU * NU * TL];
  const int lane = (int)threadIdx.x;
  const int o0 = TL == 64 ? __builtin_amdgcn_readfirstlane((int)threadIdx.y) : (int)threadIdx.y;   // the owner index
  const int b0 = (int)blockIdx.x * TL + lane, N = s.N;
  const bool live = b0 < s.B;
  const int b = live ? b0 : s.B - 1;
  const int tile = ((int)blockIdx.x * TL) >> 6, bl = b & 63;     // (B - 1 lies in the last workgroup's tile, as its live lanes do)
  const StackRef<LAYOUT, NX * NX> SA(s.A, s.NB, tile, bl);
  const StackRef<LAYOUT, NX * NU> SB(s.Bm, s.NB, tile, bl);
  const cddp_lqr::Weight Qd{a.Q + (a.q_per ? (size_t)b * (NX * NX) : 0), NX, a.q_scale}, Rd{a.R + (a.r_per ? (size_t)b * (NU * NU) : 0), NU, a.r_scale};
  const cddp_lqr::Weight Qf{a.Qf + (a.qf_per ? (size_t)b * (NX * NX) : 0), NX, 1.0};
  double *const kout = a.K_out ? a.K_out + (size_t)b * (size_t)N * (NU * NX) : nullptr;
  double *const pout = a.P_out ? a.P_out + (size_t)b * (size_t)(N + 1) * (NX * NX) : nullptr;
  double *const kst = a.K_stack ? a.K_stack + cddp_io::tiled(0, s.NB, NU * NX, 0, b) : nullptr;
  const size_t kstep = cddp_io::tiled(1, s.NB, NU * NX, 0, 0);
  const double nan = __builtin_nan("");

  // Every LDS and stack address of a step is lane + owner offset + constant, invariant over the horizon loop: the compiler would compute
  // the few hundred of them ahead of it and keep them in registers.  set_step passes the lane and the owner through an empty asm at the
  // top of every step: the addresses then belong to the step (inst_cov.hip's device).
  double *P = sP + lane, *M = sM + lane, *Q = sQ + lane;
  int o = o0;
  auto set_step = [&](unsigned l, int w) {
    if constexpr (TL == 64) asm volatile("" : "+v"(l), "+s"(w));
    else asm volatile("" : "+v"(l), "+v"(w));
    P = sP + l; M = sM + l; Q = sQ + l;
    o = w;
  };

  // P_N = the lower triangle of Qf, mirrored
  set_step((unsigned)lane, o0);
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    if (j <= o) {
      const double v = Qf(o, j);
      P[(o * NX + j) * TL] = v; P[(j * NX + o) * TL] = v;
      if (pout && live) { pout[((size_t)N * NX + o) * NX + j] = v; pout[((size_t)N * NX + j) * NX + o] = v; }
    }
  }
  __syncthreads();
  int fail = 0;
  for (int t = N - 1; t >= 0; --t) {
    set_step((unsigned)lane, o0);
    const Strided<SA.se> A{SA.p + (size_t)t * SA.st, SA.lo, NX}, Bm{SB.p + (size_t)t * SB.st, SB.lo, NU};
    const Lds<TL> Pg{P, NX}, Mg{M, NU}, Qg{Q, NU}, Tg{M, NX};
    // 1: read P
    cddp_lqr::m_row<NX, NU>(o, Pg, Bm, [&](int k, double v) { M[(o * NU + k) * TL] = v; });
    __syncthreads();
    // 2: read M
    if (o < NU) cddp_lqr::quu_row<NX, NU>(o, Bm, Mg, Rd, [&](int c, double v) { Q[(o * NU + c) * TL] = v; });
    __syncthreads();
    // 3: read Quu, M, P
    double kc[NU], acl[NX], y[NX], tc[NU];
    {
      double L[NU][NU];
      const bool ok = cddp_lqr::chol<NU>(Qg, L);
      if (!ok && fail == 0) fail = t + 1;
      cddp_lqr::qux_col<NX, NU>(o, Mg, A, kc);
      cddp_lqr::solve_col<NU>(L, kc);
    }
    const bool dead = fail != 0;
    if (live) {
#pragma unroll
      for (int k = 0; k < NU; ++k) {
        const double v = dead ? 0.0 : kc[k];
        if (kout) kout[((size_t)t * NU + k) * NX + o] = v;
        if (kst) kst[(size_t)t * kstep + (size_t)((k * NX + o) * 64)] = v;
      }
    }
    cddp_lqr::acl_col<NX, NU>(o, A, Bm, kc, acl);
    cddp_lqr::y_col<NX>(Pg, acl, y);
    cddp_lqr::t_col<NU>(Rd, kc, tc);
    __syncthreads();
    // 4: Y over P, T over M
#pragma unroll
    for (int l = 0; l < NX; ++l) P[(l * NX + o) * TL] = y[l];
#pragma unroll
    for (int k = 0; k < NU; ++k) M[(k * NX + o) * TL] = tc[k];
    __syncthreads();
    // 5: read Y, T
    double n[NX];
    cddp_lqr::p_row<NX, NU>(o, acl, kc, Pg, Tg, Qd, [&](int j, double v) { n[j] = v; });
    __syncthreads();
    // 6: P_t back, mirrored, and out
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      if (j <= o) {
        P[(o * NX + j) * TL] = n[j]; P[(j * NX + o) * TL] = n[j];
        if (pout && live) {
          const double v = dead ? nan : n[j];
          pout[((size_t)t * NX + o) * NX + j] = v; pout[((size_t)t * NX + j) * NX + o] = v;
        }
      }
    }
    __syncthreads();
  }
  if (a.info && live && o0 == 0) a.info[b] = fail;
}

// the pairs of inst_sens.hip's SENS_PAIR_LIST (tests/test_plan_lqr_abi.py holds the two lists to each other): Y(NX, NU)
#ifndef LQR_PAIR_LIST   // (a one-pair build, -D'LQR_PAIR_LIST(Y)=Y(14, 7)', shows one kernel's registers in seconds)
#define LQR_PAIR_LIST(Y) \
  Y(1, 1) Y(2, 1) Y(3, 1) Y(3, 2) Y(4, 1) Y(4, 2) Y(5, 2) Y(6, 2) Y(6, 3) Y(7, 3) Y(8, 3) Y(10, 3) Y(10, 4) Y(12, 4) Y(13, 4) Y(14, 7)
#endif

template <int NX, int NU>
void launch_pair(const SensStacks &s, const LqrArgs &a, hipStream_t st) {
  constexpr int TL = Tile<NX>::kLanes;
  const dim3 grid((s.B + TL - 1) / TL), block(TL, NX);
  if (s.layout == cddp_io::kT4) hipLaunchKernelGGL((k_plan_lqr<NX, NU, cddp_io::kT4>), grid, block, 0, st, s, a);
  else hipLaunchKernelGGL((k_plan_lqr<NX, NU, cddp_io::kTiled>), grid, block, 0, st, s, a);
}

}  // namespace

hipError_t plan_lqr(const SensStacks &s, const LqrArgs &a, hipStream_t stream) {
  if (s.B <= 0 || s.N <= 0 || !a.Q || !a.R || !a.Qf || (!a.K_out && !a.P_out && !a.K_stack)) return hipErrorInvalidValue;
#define Y(NX, NU) if (s.nx == NX && s.nu == NU) { launch_pair<NX, NU>(s, a, stream); return hipGetLastError(); }
  LQR_PAIR_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

}  // namespace cddp_dev
