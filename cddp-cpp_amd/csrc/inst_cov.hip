// Plan-covariance kernel of the resident handle: Sigma_{t+1} = Acl_t Sigma_t Acl_t^T + W + B_t Wu B_t^T with Acl_t = A_t + B_t K_t, run
// forward from Sigma_0, with cov(du_t) = K_t Sigma_t K_t^T + Wu and the expected increase of the quadratic objective along the way.  The
// arithmetic is plan_cov.hpp's, fixed by include/cddp_hip.h.
//
// A matrix recursion, 2 nx^3 products per step: one lane per trajectory cannot hold it in registers from nx = 10 on.  So ONE WORKGROUP walks
// the horizon for a 64-trajectory tile (blockDim = (64, waves)): lane = trajectory, a wavefront owns one row of Sigma, and from nx = 10 on
// two: wave w owns rows w and NX - 1 - w, which is NX + 1 elements of the lower triangle for every wave (Rows).  Sigma_t lives in LDS as
// [NX][NX][64] doubles (lane-consecutive: every 64-bit LDS access is conflict-free), the wave's rows of Acl_t in registers.  Of the stacks
// a wave loads its rows of A_t and of B_t and all of K_t, where they lie: an element is a lane-consecutive 512-byte row (wave-tiled) or a
// 32-byte quad per four lanes (sub-tile-minor); the waves of a group re-read K_t out of the cache.  A step, four barriers:
//   A  read Sigma_t:  the rows of SX out and the Qdt trace rows;  Acl rows and Z columns in one pass over K_t (Z to its LDS buffer);  Y rows -> registers
//   B  the Y rows over the Sigma buffer;  the waves of rows i < NU: row i of SU from Z and K_t, out, and the Rdt trace row
//   C  read Y:  a wave computes Sigma_{t+1}[i][j] for j <= i of its rows into registers (B_t's other rows come from the stack);  wave 0 sums the trace rows
//   D  Sigma_{t+1} back, mirrored
// With one row per wave (nx <= 8) row i has i + 1 elements in phase C and the last wave does the most; the waves sit on the SIMDs
// round-robin, which evens part of it out.
// NX = 14 (Rows::kConst, kStage) differs in three ways, which together bring (14, 7) from 168 bytes of scratch per lane to none:
//   - every phase is compiled once per wave with the wave's rows as constants (for_wave): no run-time row enters an address or a guard;
//   - Z and SU get two phases of their own at the head of the step (Z: read Sigma_t, Z columns out;  U: SU rows from Z and K_t), before Acl
//     and Y are held -- six barriers instead of four when SU or dcost is wanted -- and from then on the Z buffer is free: the second
//     row of a wave's Y (phase A -> B) and of its Sigma_{t+1} (C -> D) waits in the wave's own NX slots of it instead of in registers;
//   - the stack accessor passes every element's address through an empty asm (Strided<.., ORDERED>), which keeps the loads of an output
//     column behind the fence before it: without it the compiler issues the loads of all of K_t (98 values, 196 registers) ahead of the sums.
// LDS: (NX NX + NU NX + NX + NU) * 512 bytes, 157.5 KB of the 160 KB at (14, 7): one group per CU there.  DIAG is a run-time branch on
// the stores.  Registers and scratch per pair: profiles/r17_plan_covariance.md (scratch is 0 for every pair).
//
// Bounds: lanes beyond the batch (the last tile) walk along for the barriers on the rows of trajectory B - 1 and store nothing: every
// access is that of a trajectory b < B.  A stack access is (t < N, e < E, b), inside the N * E * NB * 64 doubles every stack is allocated
// with; a batch-major access is row t <= N (SX) or t < N (SU) of trajectory b, inside the extents capi.hip has checked; Sigma0 / W / Wu
// are read at element (i, j <= i) of trajectory b (or of the one shared matrix).  LDS indices are (r < NX or NU, c < NX, lane < 64).
#include "cov_kernels.hpp"

#include <type_traits>

#include "plan_cov.hpp"

namespace cddp_dev {

namespace {

// A tile's view of a stack with E elements per step.  Every index map of io_layout.hpp splits into a part that is the same for the 64
// lanes of a tile (step, tile, element) and a part that depends on the lane alone: element e of step t of lane l is at
// base[t * st + e * se + lo(l)].  The first part is scalar arithmetic and the second one 32-bit register for the whole walk, so a load
// needs no 64-bit address register of its own.
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

// accessor of plan_cov.hpp that loads from the stack: p = the tile's first element of the step
template <int SE, bool ORDERED = false>
struct Strided {
  const double *p; unsigned lo; int cols;
  __device__ __forceinline__ double operator()(int i, int j) const {
    const double *q = p + (i * cols + j) * SE;
    if (ORDERED) asm volatile("" : "+s"(q));     // the element's address exists from here on: the load stays behind the fence before it
    return q[lo];
  }
};

// accessor of an LDS buffer [rows][cols][64] through the lane's own column
struct Lds {
  const double *p; int cols;
  __device__ __forceinline__ double operator()(int i, int j) const { return p[(i * cols + j) * 64]; }
};

// a row held in registers, as the matrix whose every row it is
template <int NN>
struct RowReg {
  const double (&r)[NN];
  __device__ __forceinline__ double operator()(int, int j) const { return r[j]; }
};

// rows of Sigma a wavefront owns.  One row per wave is the natural split, but NX >= 10 would then run 10 .. 14 waves, three or four to a
// SIMD, on 168 or 128 registers each, and the step spills; two rows per wave run at most seven waves, two to a SIMD, on 256 registers,
// fetch every element of K_t once for both rows, and pair a short row of the triangle with a long one.
template <int NX>
struct Rows {
  static constexpr int kPerWave = NX >= 10 ? 2 : 1, kWaves = (NX + kPerWave - 1) / kPerWave;
  static constexpr bool kConst = NX >= 14;    // the phases are compiled once per wave, with the wave's rows as constants
  // kStage: the second row of a wave's Y and of its Sigma_{t+1} waits in the wave's own NX slots of the Z buffer instead of registers; Z and
  // SU are then computed in two phases of their own at the head of the step (two more barriers), before Acl and Y are held
  static constexpr bool kStage = NX >= 14;
};

// f(integral_constant<int, w>) for the w < NWAVES a wavefront is (the same for its 64 lanes)
template <int I, int NWAVES, class F>
__device__ __forceinline__ void for_wave(int w, const F &f) {
  if constexpr (I < NWAVES) {
    if (w == I) f(std::integral_constant<int, I>{});
    else for_wave<I + 1, NWAVES>(w, f);
  }
}

// The walk of one tile.  WANT_U (SU or dcost is wanted: Z and SU are computed) and HAVE_WU (actuator noise is given) are fixed for a call,
// so the kernel branches on them once, outside the horizon loop, and the sums run without a branch inside; DIAG and W stay run-time
// branches, one per stored or computed element.
template <int NX, int NU, int LAYOUT, bool WANT_U, bool HAVE_WU>
__device__ __forceinline__ void cov_walk(const SensStacks &s, const CovArgs &a, double *sS, double *sZ, double *sR) {
  constexpr int RW = Rows<NX>::kPerWave;
  const int lane = (int)threadIdx.x, i0 = __builtin_amdgcn_readfirstlane((int)threadIdx.y);   // the wave
  const int b0 = (int)blockIdx.x * 64 + lane, N = s.N;
  const bool live = b0 < s.B;
  const int b = live ? b0 : s.B - 1;
  const int tile = (int)blockIdx.x, bl = b & 63;     // (B - 1 lies in the last tile, as its live lanes do)
  const StackRef<LAYOUT, NX * NX> SA(s.A, s.NB, tile, bl);
  const StackRef<LAYOUT, NX * NU> SB(s.Bm, s.NB, tile, bl);
  const StackRef<cddp_io::kTiled, NU * NX> SK(s.K, s.NB, tile, bl);
  const size_t per = a.per_traj ? (size_t)b : 0;
  const cddp_cov::SymLower Sig0{a.Sigma0 + per * (NX * NX), NX}, W{a.W ? a.W + per * (NX * NX) : nullptr, NX}, Wu{HAVE_WU ? a.Wu + per * (NU * NU) : nullptr, NU};
  const cddp_cov::Dense Qdt{a.Qdt, NX}, Rdt{a.Rdt, NU}, Qf{a.Qf, NX};
  const bool diag = a.diag != 0, want_c = a.dcost != nullptr;
  const int EX = diag ? NX : NX * NX, EU = diag ? NU : NU * NU;
  double *const sx = a.SX ? a.SX + (size_t)b * (size_t)(N + 1) * EX : nullptr;
  double *const su = a.SU ? a.SU + (size_t)b * (size_t)N * EU : nullptr;
  double *S = sS + lane, *Z = sZ + lane, *R = sR + lane;
  Lds Sg{S, NX}, Zg{Z, NX};

  // row i of row t of SX out of LDS, and the trace row of Sigma_t with Q
  auto row_out = [&](int t, int i, const cddp_cov::Dense &Q) {
    if (sx && live) {
      if (diag) sx[(size_t)t * NX + i] = Sg(i, i);
      else {
#pragma unroll
        for (int j = 0; j < NX; ++j) sx[((size_t)t * NX + i) * NX + j] = Sg(i, j);
      }
    }
    if (want_c) R[i * 64] = cddp_cov::trace_row<NX>(i, Q, Sg);
  };

  // Every LDS and stack address of a step is lane + row offset + constant.  All of them are invariant over the horizon loop, so the
  // compiler would compute the few hundred of them ahead of it and keep them in registers (spilled, at nx >= 10).  set_step is called
  // at the top of every step with the lane and the wave passed through an empty asm: the addresses then belong to the step.
  int wv = i0;
  auto set_step = [&](unsigned l, int w) {
    asm volatile("" : "+v"(l), "+s"(w));
    S = sS + l; Z = sZ + l; R = sR + l;
    Sg = Lds{S, NX}; Zg = Lds{Z, NX};
    wv = w;
  };
  // wave w owns row w, and with two rows per wave also row NX - 1 - w: NX + 1 elements of the lower triangle for every wave (NX odd: the
  // middle wave has its one row twice, the same values to the same places).  Wc >= 0: the wave is a constant of this copy of the phase.
  auto rows_of = [&](auto Wc, int (&row)[RW]) {
    constexpr int wc = decltype(Wc)::value;
    const int w = wc >= 0 ? wc : wv;
    row[0] = w;
    if (RW == 2) row[RW - 1] = NX - 1 - w;
  };
  auto run = [&](const auto &phase) {
    if constexpr (Rows<NX>::kConst) for_wave<0, Rows<NX>::kWaves>(wv, phase);
    else phase(std::integral_constant<int, -1>{});
  };
  set_step((unsigned)lane, i0);
  run([&](auto Wc) {
    int row[RW]; rows_of(Wc, row);
#pragma unroll
    for (int q = 0; q < RW; ++q) {
      const int i = row[q];
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        if (j <= i) { const double v = Sig0(i, j); S[(i * NX + j) * 64] = v; S[(j * NX + i) * 64] = v; }
      }
    }
  });
  __syncthreads();
  double dc = 0.0;
  for (int t = 0; t < N; ++t) {
    set_step((unsigned)lane, i0);
    const Strided<SA.se, Rows<NX>::kStage> A{SA.p + (size_t)t * SA.st, SA.lo, NX}, Bm{SB.p + (size_t)t * SB.st, SB.lo, NU};
    const Strided<SK.se, Rows<NX>::kStage> K{SK.p + (size_t)t * SK.st, SK.lo, NX};
    if constexpr (Rows<NX>::kStage) {
      static_assert(RW == 2 && Rows<NX>::kWaves * NX <= NU * NX, "a wave's NX slots of the Z buffer");
      run([&](auto Wc) {   // Z: read Sigma_t
        int row[RW]; rows_of(Wc, row);
#pragma unroll
        for (int q = 0; q < RW; ++q) row_out(t, row[q], Qdt);
        CDDP_COV_FENCE();
        if (WANT_U) cddp_cov::z_cols<NX, NU, RW>(row, K, Sg, [&](int q, int k, double v) { Z[(k * NX + row[q]) * 64] = v; });
      });
      if (WANT_U) {
        __syncthreads();
        run([&](auto Wc) {   // U: read Z
          int row[RW]; rows_of(Wc, row);
          if (row[0] < NU) {
            double u[RW][NU];
            cddp_cov::su_rows<NX, NU, RW>(row, Zg, K, Wu, diag && !want_c, u);
#pragma unroll
            for (int q = 0; q < RW; ++q) {
              const int i = row[q];
              if (i < NU) {
                if (su && live) {
#pragma unroll
                  for (int j = 0; j < NU; ++j) {
                    if (!diag) su[((size_t)t * NU + i) * NU + j] = u[q][j];
                    else if (j == i) su[(size_t)t * NU + i] = u[q][j];
                  }
                }
                if (want_c) R[(NX + i) * 64] = cddp_cov::trace_row<NU>(i, Rdt, RowReg<NU>{u[q]});
              }
            }
          }
        });
        __syncthreads();
      }
      double acl[RW][NX], y0[NX], n0[NX];
      run([&](auto Wc) {   // A: read Sigma_t; the second row of Y to the wave's slots of Z
        int row[RW]; rows_of(Wc, row);
        double *const mine = Z + row[0] * NX * 64;
        cddp_cov::acl_z<NX, NU, RW, false>(row, A, Bm, K, Sg, acl, [](int, int, double) {});
        cddp_cov::y_rows_to<NX, RW>(acl, Sg, [&](int q, int j, double v) {
          if (q == 0) { y0[j] = v; CDDP_COV_PIN(y0[j]); } else mine[j * 64] = v;
        });
      });
      __syncthreads();
      run([&](auto Wc) {   // B: the Y rows over the Sigma buffer
        int row[RW]; rows_of(Wc, row);
        const double *const mine = Z + row[0] * NX * 64;
#pragma unroll
        for (int j = 0; j < NX; ++j) { S[(row[0] * NX + j) * 64] = y0[j]; S[(row[1] * NX + j) * 64] = mine[j * 64]; }
      });
      __syncthreads();
      if (want_c && i0 == 0) {   // C: read Y
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < NX + NU; ++r) c += R[r * 64];
        dc += c;
      }
      run([&](auto Wc) {
        int row[RW]; rows_of(Wc, row);
        double *const mine = Z + row[0] * NX * 64;
        cddp_cov::next_rows_to<NX, NU, RW, HAVE_WU>(row, acl, Sg, W, Wu, Bm, [&](int q, int j, double v) {
          if (q == 0) { n0[j] = v; CDDP_COV_PIN(n0[j]); } else mine[j * 64] = v;
        });
      });
      __syncthreads();
      run([&](auto Wc) {   // D: Sigma_{t+1} back, mirrored
        int row[RW]; rows_of(Wc, row);
        const double *const mine = Z + row[0] * NX * 64;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          if (j <= row[0]) { S[(row[0] * NX + j) * 64] = n0[j]; S[(j * NX + row[0]) * 64] = n0[j]; }
          if (row[1] != row[0] && j <= row[1]) { const double v = mine[j * 64]; S[(row[1] * NX + j) * 64] = v; S[(j * NX + row[1]) * 64] = v; }
        }
      });
      __syncthreads();
    } else {
      double acl[RW][NX], y[RW][NX];
      run([&](auto Wc) {   // A
        int row[RW]; rows_of(Wc, row);
#pragma unroll
        for (int q = 0; q < RW; ++q) row_out(t, row[q], Qdt);
        CDDP_COV_FENCE();
        cddp_cov::acl_z<NX, NU, RW, WANT_U>(row, A, Bm, K, Sg, acl, [&](int q, int k, double v) { Z[(k * NX + row[q]) * 64] = v; });
        cddp_cov::y_rows<NX, RW>(acl, Sg, y);
      });
      __syncthreads();
      run([&](auto Wc) {   // B
        int row[RW]; rows_of(Wc, row);
#pragma unroll
        for (int q = 0; q < RW; ++q) {
#pragma unroll
          for (int j = 0; j < NX; ++j) S[(row[q] * NX + j) * 64] = y[q][j];
        }
        if (WANT_U && row[0] < NU) {
          double u[RW][NU];
          cddp_cov::su_rows<NX, NU, RW>(row, Zg, K, Wu, diag && !want_c, u);
#pragma unroll
          for (int q = 0; q < RW; ++q) {
            const int i = row[q];
            if (i < NU) {
              if (su && live) {
#pragma unroll
                for (int j = 0; j < NU; ++j) {
                  if (!diag) su[((size_t)t * NU + i) * NU + j] = u[q][j];
                  else if (j == i) su[(size_t)t * NU + i] = u[q][j];
                }
              }
              if (want_c) R[(NX + i) * 64] = cddp_cov::trace_row<NU>(i, Rdt, RowReg<NU>{u[q]});
            }
          }
        }
      });
      __syncthreads();
      if (want_c && i0 == 0) {   // C
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < NX + NU; ++r) c += R[r * 64];
        dc += c;
      }
      run([&](auto Wc) {
        int row[RW]; rows_of(Wc, row);
        cddp_cov::next_rows<NX, NU, RW, HAVE_WU>(row, acl, Sg, W, Wu, Bm, y);
      });
      __syncthreads();
      run([&](auto Wc) {   // D
        int row[RW]; rows_of(Wc, row);
#pragma unroll
        for (int q = 0; q < RW; ++q) {
          const int i = row[q];
#pragma unroll
          for (int j = 0; j < NX; ++j) {
            if (j <= i) { S[(i * NX + j) * 64] = y[q][j]; S[(j * NX + i) * 64] = y[q][j]; }
          }
        }
      });
      __syncthreads();
    }
  }
  set_step((unsigned)lane, i0);
  run([&](auto Wc) {
    int row[RW]; rows_of(Wc, row);
#pragma unroll
    for (int q = 0; q < RW; ++q) row_out(N, row[q], Qf);
  });
  if (want_c) {
    __syncthreads();
    if (i0 == 0) {
      double c = 0.0;
#pragma unroll
      for (int r = 0; r < NX; ++r) c += R[r * 64];
      dc += c;
      if (live) a.dcost[b] = dc;
    }
  }
}

template <int NX, int NU, int LAYOUT>
__global__ __launch_bounds__(64 * Rows<NX>::kWaves) void k_plan_cov(SensStacks s, CovArgs a) {
  static_assert(NU <= NX, "the waves of rows i < NU own the rows of SU");
  // two rows per wave: row w < NU of SU is wave w's FIRST row, and no wave's second row NX - 1 - w is a row of SU -- every row of SU
  // is computed exactly once, by the waves the `row[0] < NU` tests pick
  static_assert(Rows<NX>::kPerWave == 1 || (NU <= Rows<NX>::kWaves && NX - Rows<NX>::kWaves >= NU), "ownership of the SU rows");
  __shared__ double sS[NX * NX * 64], sZ[NU * NX * 64], sR[(NX + NU) * 64];
  const bool want_u = a.SU != nullptr || a.dcost != nullptr;
  if (want_u) {
    if (a.Wu) cov_walk<NX, NU, LAYOUT, true, true>(s, a, sS, sZ, sR);
    else cov_walk<NX, NU, LAYOUT, true, false>(s, a, sS, sZ, sR);
  } else {
    if (a.Wu) cov_walk<NX, NU, LAYOUT, false, true>(s, a, sS, sZ, sR);
    else cov_walk<NX, NU, LAYOUT, false, false>(s, a, sS, sZ, sR);
  }
}

// the pairs of inst_sens.hip's SENS_PAIR_LIST (tests/test_plan_cov_abi.py holds the two lists to each other): Y(NX, NU)
#ifndef COV_PAIR_LIST   // (a one-pair build, -D'COV_PAIR_LIST(Y)=Y(14, 7)', shows one kernel's registers in seconds)
#define COV_PAIR_LIST(Y) \
  Y(1, 1) Y(2, 1) Y(3, 1) Y(3, 2) Y(4, 1) Y(4, 2) Y(5, 2) Y(6, 2) Y(6, 3) Y(7, 3) Y(8, 3) Y(10, 3) Y(10, 4) Y(12, 4) Y(13, 4) Y(14, 7)
#endif

template <int NX, int NU>
void launch_pair(const SensStacks &s, const CovArgs &a, hipStream_t st) {
  const dim3 grid((s.B + 63) / 64), block(64, Rows<NX>::kWaves);
  if (s.layout == cddp_io::kT4) hipLaunchKernelGGL((k_plan_cov<NX, NU, cddp_io::kT4>), grid, block, 0, st, s, a);
  else hipLaunchKernelGGL((k_plan_cov<NX, NU, cddp_io::kTiled>), grid, block, 0, st, s, a);
}

}  // namespace

hipError_t plan_cov(const SensStacks &s, const CovArgs &a, hipStream_t stream) {
  if (s.B <= 0 || s.N <= 0 || !a.Sigma0 || (!a.SX && !a.SU && !a.dcost)) return hipErrorInvalidValue;
#define Y(NX, NU) if (s.nx == NX && s.nu == NU) { launch_pair<NX, NU>(s, a, stream); return hipGetLastError(); }
  COV_PAIR_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

}  // namespace cddp_dev
