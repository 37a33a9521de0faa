// Filter kernel of the resident handle: the Kalman filter of the plan's linearisation for the caller's sensors (y_t = C dx_t + n_t,
// cov(n_t) = diag v, a measurement at every step before u_t is applied) and the covariance of states and controls when the plan's feedback
// acts on the filtered estimate, du_t = K_t xhat_t|t.  Run forward from Sm_0 = Sigma0, Xm_0 = 0:
//   update, one row of C at a time:  h = S c,  s = v_r + c . h,  g = h / s,  S <- S - g h^T - h g^T + s g g^T,  G += h g^T     (Sf_t = S)
//   L_t = Sf_t C^T diag(v)^-1,   Xh_t = Xm_t + G,   SX_t = Xh_t + Sf_t,   SU_t = K_t Xh_t K_t^T + Wu
//   Sm_{t+1} = A_t Sf_t A_t^T + W + B_t Wu B_t^T,   Xm_{t+1} = Acl_t Xh_t Acl_t^T,   Acl_t = A_t + B_t K_t
// The forward dual of inst_lqr.hip's recursion, with no factorisation: the rows of a step are scalar updates, so ny is a run-time loop
// bound.  The arithmetic is plan_kf.hpp's and plan_cov.hpp's, fixed by include/cddp_hip.h.
//
// ONE WORKGROUP walks the horizon for a tile of TL trajectories (blockDim = (TL, NX), inst_lqr.hip's split): lane x = trajectory, and
// the NX "owners" y each hold one row: row y of S (the error covariance, Sm_t then Sf_t), of G (registers), of Xh / Xm, of L_t, of SX, of
// SU (y < NU), of A_t and Acl_t (registers).  S and X (the estimate covariance) live in LDS as [NX][NX][TL] doubles, lane-consecutive;
// T is the product buffer: Z = K Xh and the trace rows first, then Y = A Sf, then Y' = Acl Xh -- three tenants in a step, one buffer;
// H holds h.  A step:
//   row r of the update, two barriers each:  h[y] -> H  |  every owner forms s for itself (nx products: cheaper than a third barrier),
//        the elements j <= y of row y of S back, mirrored, and of G on
//   L_t row y out (the same sum as h over the posterior);  Xh row y back, mirrored  |  SX row y out, its trace row;  Z column y -> T  |
//   SU row y < NU out, its trace row  |  owner 0 sums the trace rows;  row y of Y -> registers  |  Y -> T  |  Sm_{t+1} row y ->
//   registers  |  S back, mirrored;  row y of Acl and of Y';  Y' -> T  |  Xm_{t+1} row y back, mirrored.
// 2 ny + 7 barriers a step (2 ny + 5 when neither SU nor dcost is wanted).
// TL = 64 up to nx = 8: an owner is a wavefront (its index is a scalar).  From nx = 10 on TL = 32 and two owners share a wavefront (the
// owner index is a per-lane value that enters addresses and guards only, never a register index), as in inst_lqr.hip: 5 .. 7 waves on
// 256 registers each, and (14, 7) fits LDS.  LDS: (2 NX NX + max(NX NX, NU NX + NX + NU) + NX) * 8 * TL bytes: 150.5 KB of the 160 KB at
// (14, 7), 133 KB at (13, 4), 100 KB at (8, 3): one group per CU from nx = 8 on.  Registers and scratch per pair:
// profiles/r21_plan_kalman.md.
// C and v shared by the batch (PER = false) are read at addresses that are the same for every lane; per trajectory they are vector loads.
// A failed row (s not > 0, NaN included) at step t marks the lane dead from then on: every owner of the lane forms the same s and so the
// same verdict.  NaN is stored in every output row s >= t (row t of SP, written before the update, is overwritten), info = t + 1 of the
// first failure, dcost = NaN; the lane keeps walking for the barriers, on whatever its buffers hold.
//
// Bounds: lanes beyond the batch (the last workgroup) walk along for the barriers on the rows of trajectory B - 1 and store nothing:
// every access is that of a trajectory b < B, and B - 1 lies in the workgroup's own 64-tile.  A stack access is (t < N, e < E, b), inside
// the N * E * NB * 64 doubles every stack is allocated with.  A batch-major access is row t <= N (L, SP, SF, SX) or t < N (SU) of
// trajectory b, inside the extents capi.hip has checked; C at (r < ny, j < NX) and v at r < ny of trajectory b or of the shared array;
// Sigma0 / W / Wu at element (i, j <= i); dcost and info at b.  LDS indices are (r < NX or NU, c < NX, lane < TL) of S, X and Z, r < NX + NU
// of the trace rows behind Z (kT counts both), r < NX of H.
#include "kf_kernels.hpp"

#include "plan_kf.hpp"

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

// accessor of the step bodies that loads from the stack: p = the tile's first element of the step
template <int SE>
struct Strided {
  const double *p; unsigned lo; int cols;
  __device__ __forceinline__ double operator()(int i, int j) const { return p[(i * cols + j) * SE + lo]; }
};

// accessors of an LDS buffer [rows][cols][TL] and of an LDS vector [n][TL] through the lane's own column
template <int TL>
struct Lds {
  const double *p; int cols;
  __device__ __forceinline__ double operator()(int i, int j) const { return p[(i * cols + j) * TL]; }
};
template <int TL>
struct LdsVec {
  const double *p;
  __device__ __forceinline__ double operator()(int j) const { return p[j * TL]; }
};

// a row held in registers, as the matrix whose every row it is
template <int NN>
struct RowReg {
  const double (&r)[NN];
  __device__ __forceinline__ double operator()(int, int j) const { return r[j]; }
};

// trajectories per workgroup (inst_lqr.hip's): from nx = 10 on two owners share a wavefront
template <int NX, int NU>
struct Tile {
  static constexpr int kLanes = NX >= 10 ? 32 : 64;
  static constexpr int kThreads = kLanes * NX;
  static constexpr int kT = NX * NX > NU * NX + NX + NU ? NX * NX : NU * NX + NX + NU;   // doubles per lane of the product buffer
};

template <int NX, int NU, int LAYOUT, bool PER>
__device__ __forceinline__ void kf_walk(const SensStacks &s, const KfArgs &a, double *sS, double *sX, double *sT, double *sH) {
  constexpr int TL = Tile<NX, NU>::kLanes;
  const int lane = (int)threadIdx.x;
  const int o0 = TL == 64 ? __builtin_amdgcn_readfirstlane((int)threadIdx.y) : (int)threadIdx.y;   // the owner index
  const int b0 = (int)blockIdx.x * TL + lane, N = s.N, ny = a.ny;
  const bool live = b0 < s.B;
  const int b = live ? b0 : s.B - 1;
  const int tile = ((int)blockIdx.x * TL) >> 6, bl = b & 63;     // (B - 1 lies in the last workgroup's tile, as its live lanes do)
  const StackRef<LAYOUT, NX * NX> SA(s.A, s.NB, tile, bl);
  const StackRef<LAYOUT, NX * NU> SB(s.Bm, s.NB, tile, bl);
  const StackRef<cddp_io::kTiled, NU * NX> SK(s.K, s.NB, tile, bl);
  const size_t per = PER ? (size_t)b : 0;
  const double *const Cp = a.C + per * (size_t)(ny * NX), *const vp = a.v + per * (size_t)ny;
  const cddp_cov::SymLower Sig0{a.Sigma0 + per * (NX * NX), NX}, W{a.W ? a.W + per * (NX * NX) : nullptr, NX}, Wu{a.Wu ? a.Wu + per * (NU * NU) : nullptr, NU};
  const cddp_cov::SymLower none{nullptr, NX};
  const cddp_cov::Dense Qdt{a.Qdt, NX}, Rdt{a.Rdt, NU}, Qf{a.Qf, NX};
  const bool diag = a.diag != 0, want_c = a.dcost != nullptr, want_u = a.SU != nullptr || want_c, have_wu = a.Wu != nullptr;
  const int EX = diag ? NX : NX * NX, EU = diag ? NU : NU * NU;
  double *const lout = a.L ? a.L + (size_t)b * (size_t)(N + 1) * (size_t)(NX * ny) : nullptr;
  double *const sp = a.SP ? a.SP + (size_t)b * (size_t)(N + 1) * EX : nullptr;
  double *const sf = a.SF ? a.SF + (size_t)b * (size_t)(N + 1) * EX : nullptr;
  double *const sx = a.SX ? a.SX + (size_t)b * (size_t)(N + 1) * EX : nullptr;
  double *const su = a.SU ? a.SU + (size_t)b * (size_t)N * EU : nullptr;
  const double nan = __builtin_nan("");

  // Every LDS and stack address of a step is lane + owner offset + constant, invariant over the horizon loop: set_step passes the lane and
  // the owner through an empty asm at the top of every step, so the addresses belong to the step (inst_cov.hip's device).
  double *S = sS + lane, *X = sX + lane, *T = sT + lane, *H = sH + lane;
  int o = o0;
  auto set_step = [&](unsigned l, int w) {
    if constexpr (TL == 64) asm volatile("" : "+v"(l), "+s"(w));
    else asm volatile("" : "+v"(l), "+v"(w));
    S = sS + l; X = sX + l; T = sT + l; H = sH + l;
    o = w;
  };
  // row o of a covariance in LDS to row t of an output (diag: its diagonal element), NaN for a dead lane
  auto row_out = [&](double *out, int t, const Lds<TL> &M, bool dead) {
    if (diag) out[(size_t)t * NX + o] = dead ? nan : M(o, o);
    else {
#pragma unroll
      for (int j = 0; j < NX; ++j) out[((size_t)t * NX + o) * NX + j] = dead ? nan : M(o, j);
    }
  };

  // Sm_0 = the lower triangle of Sigma0, mirrored;  Xm_0 = 0
  set_step((unsigned)lane, o0);
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    if (j <= o) {
      const double v = Sig0(o, j);
      S[(o * NX + j) * TL] = v; S[(j * NX + o) * TL] = v;
      X[(o * NX + j) * TL] = 0.0; X[(j * NX + o) * TL] = 0.0;
    }
  }
  __syncthreads();
  int fail = 0;
  double dc = 0.0;
  for (int t = 0; t <= N; ++t) {
    set_step((unsigned)lane, o0);
    const Lds<TL> Sg{S, NX}, Xg{X, NX}, Zg{T, NX}, Yg{T, NX};
    const LdsVec<TL> Hg{H};
    double *const R = T + NU * NX * TL;       // the trace rows, behind Z
    const int row[1] = {o};
    if (sp && live) row_out(sp, t, Sg, fail != 0);
    // the measurement update, row by row
    double gr[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) gr[j] = 0.0;
    for (int r = 0; r < ny; ++r) {
      const cddp_kf::Row c{Cp + r * NX};
      H[o * TL] = cddp_kf::h_elem<NX>(o, Sg, c);
      __syncthreads();
      const double sr = cddp_kf::innovation<NX>(vp[r], c, Hg);
      if (!(sr > 0.0) && fail == 0) fail = t + 1;
      cddp_kf::joseph_row<NX>(o, sr, Hg, Sg, [&](int j, double e) { S[(o * NX + j) * TL] = e; S[(j * NX + o) * TL] = e; }, gr);
      __syncthreads();
    }
    const bool dead = fail != 0;
    if (live) {
      if (sp && fail == t + 1) {
        if (diag) sp[(size_t)t * NX + o] = nan;
        else {
#pragma unroll
          for (int j = 0; j < NX; ++j) sp[((size_t)t * NX + o) * NX + j] = nan;
        }
      }
      if (sf) row_out(sf, t, Sg, dead);
      if (lout) {
        for (int r = 0; r < ny; ++r) {
          const double l = cddp_kf::h_elem<NX>(o, Sg, cddp_kf::Row{Cp + r * NX}) / vp[r];
          lout[((size_t)t * NX + o) * ny + r] = dead ? nan : l;
        }
      }
    }
    // Xh = Xm + G: the owner's elements j <= o, which it wrote itself
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      if (j <= o) {
        const double v = X[(o * NX + j) * TL] + gr[j];
        X[(o * NX + j) * TL] = v; X[(j * NX + o) * TL] = v;
      }
    }
    __syncthreads();
    // SX = Xh + Sf, row o, and its trace row
    if (sx || want_c) {
      double xr[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) xr[j] = Xg(o, j) + Sg(o, j);
      if (sx && live) {
        if (diag) sx[(size_t)t * NX + o] = dead ? nan : Xg(o, o) + Sg(o, o);
        else {
#pragma unroll
          for (int j = 0; j < NX; ++j) sx[((size_t)t * NX + o) * NX + j] = dead ? nan : xr[j];
        }
      }
      if (want_c) R[o * TL] = t < N ? cddp_cov::trace_row<NX>(o, Qdt, RowReg<NX>{xr}) : cddp_cov::trace_row<NX>(o, Qf, RowReg<NX>{xr});
    }
    if (t == N) break;
    const Strided<SA.se> A{SA.p + (size_t)t * SA.st, SA.lo, NX}, Bm{SB.p + (size_t)t * SB.st, SB.lo, NU};
    const Strided<SK.se> K{SK.p + (size_t)t * SK.st, SK.lo, NX};
    if (want_u) {
      cddp_cov::z_cols<NX, NU, 1>(row, K, Xg, [&](int, int k, double v) { T[(k * NX + o) * TL] = v; });
      __syncthreads();
      if (o < NU) {
        double u[1][NU];
        cddp_cov::su_rows<NX, NU, 1>(row, Zg, K, Wu, false, u);
        if (su && live) {
#pragma unroll
          for (int j = 0; j < NU; ++j) {
            if (!diag) su[((size_t)t * NU + o) * NU + j] = dead ? nan : u[0][j];
            else if (j == o) su[(size_t)t * NU + o] = dead ? nan : u[0][j];
          }
        }
        if (want_c) R[(NX + o) * TL] = cddp_cov::trace_row<NU>(o, Rdt, RowReg<NU>{u[0]});
      }
      __syncthreads();
      if (want_c && o == 0) {
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < NX + NU; ++r) c += R[r * TL];
        dc += c;
      }
    }
    // row o of A and of Y = A Sf;  then, once Sm_{t+1} is in registers, row o of Acl and of Y' = Acl Xh (X is not written before the
    // end of the step): one pair of rows is held at a time
    double a0[1][NX], y[1][NX], n[1][NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) a0[0][j] = A(o, j);
    cddp_cov::y_rows<NX, 1>(a0, Sg, y);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NX; ++j) T[(o * NX + j) * TL] = y[0][j];
    __syncthreads();
    if (have_wu) cddp_cov::next_rows<NX, NU, 1, true>(row, a0, Yg, W, Wu, Bm, n);
    else cddp_cov::next_rows<NX, NU, 1, false>(row, a0, Yg, W, Wu, Bm, n);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      if (j <= o) { S[(o * NX + j) * TL] = n[0][j]; S[(j * NX + o) * TL] = n[0][j]; }
    }
    double acl[1][NX];
    cddp_cov::acl_z<NX, NU, 1, false>(row, A, Bm, K, Xg, acl, [](int, int, double) {});
    cddp_cov::y_rows<NX, 1>(acl, Xg, y);
#pragma unroll
    for (int j = 0; j < NX; ++j) T[(o * NX + j) * TL] = y[0][j];
    __syncthreads();
    cddp_cov::next_rows<NX, NU, 1, false>(row, acl, Yg, none, none, Bm, n);
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      if (j <= o) { X[(o * NX + j) * TL] = n[0][j]; X[(j * NX + o) * TL] = n[0][j]; }
    }
  }
  if (want_c) {
    __syncthreads();
    if (o0 == 0) {
      const double *const R = T + NU * NX * TL;
      double c = 0.0;
#pragma unroll
      for (int r = 0; r < NX; ++r) c += R[r * TL];
      dc += c;
      if (live) a.dcost[b] = fail != 0 ? nan : dc;
    }
  }
  if (a.info && live && o0 == 0) a.info[b] = fail;
}

template <int NX, int NU, int LAYOUT>
__global__ __launch_bounds__((Tile<NX, NU>::kThreads)) void k_plan_kf(SensStacks s, KfArgs a) {
  static_assert(NU <= NX, "the owners y < NU own the rows of SU");
  static_assert(Tile<NX, NU>::kThreads <= 1024 && 64 % Tile<NX, NU>::kLanes == 0, "a workgroup lies inside one 64-tile of the stacks");
  constexpr int TL = Tile<NX, NU>::kLanes;
  __shared__ double sS[NX * NX * TL], sX[NX * NX * TL], sT[Tile<NX, NU>::kT * TL], sH[NX * TL];
  if (a.per_traj) kf_walk<NX, NU, LAYOUT, true>(s, a, sS, sX, sT, sH);
  else kf_walk<NX, NU, LAYOUT, false>(s, a, sS, sX, sT, sH);
}

// the pairs of inst_sens.hip's SENS_PAIR_LIST (tests/test_plan_kf_abi.py holds the two lists to each other): Y(NX, NU)
#ifndef KF_PAIR_LIST   // (a one-pair build, -D'KF_PAIR_LIST(Y)=Y(14, 7)', shows one kernel's registers in seconds)
#define KF_PAIR_LIST(Y) \
  Y(1, 1) Y(2, 1) Y(3, 1) Y(3, 2) Y(4, 1) Y(4, 2) Y(5, 2) Y(6, 2) Y(6, 3) Y(7, 3) Y(8, 3) Y(10, 3) Y(10, 4) Y(12, 4) Y(13, 4) Y(14, 7)
#endif

template <int NX, int NU>
void launch_pair(const SensStacks &s, const KfArgs &a, hipStream_t st) {
  constexpr int TL = Tile<NX, NU>::kLanes;
  const dim3 grid((s.B + TL - 1) / TL), block(TL, NX);
  if (s.layout == cddp_io::kT4) hipLaunchKernelGGL((k_plan_kf<NX, NU, cddp_io::kT4>), grid, block, 0, st, s, a);
  else hipLaunchKernelGGL((k_plan_kf<NX, NU, cddp_io::kTiled>), grid, block, 0, st, s, a);
}

}  // namespace

hipError_t plan_kf(const SensStacks &s, const KfArgs &a, hipStream_t stream) {
  if (s.B <= 0 || s.N <= 0 || a.ny < 1 || a.ny > 16 || !a.C || !a.v || !a.Sigma0) return hipErrorInvalidValue;
  if (!a.L && !a.SP && !a.SF && !a.SX && !a.SU && !a.dcost && !a.info) return hipErrorInvalidValue;
#define Y(NX, NU) if (s.nx == NX && s.nu == NU) { launch_pair<NX, NU>(s, a, stream); return hipGetLastError(); }
  KF_PAIR_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

}  // namespace cddp_dev
