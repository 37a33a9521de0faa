// Plan-sensitivity kernels of the resident handle: dx_{t+1} = A_t dx_t + B_t du_t, du_t = K_t dx_t run forward from dx_0 (JVP), and its
// adjoint run backward from the cotangents of (X, U) (VJP).  The arithmetic is plan_sens.hpp's, fixed by include/cddp_hip.h.
//
// One lane per trajectory walks the horizon, as k_track_plan does; a lane carries RV vectors, so each element of A_t, B_t, K_t is loaded
// once per step and used RV times; blockIdx.y numbers the chunks of RV vectors (the last one may be partial: its idle vectors compute on
// zeros and neither read nor write memory).  The stacks are read where they lie: an element is a lane-consecutive 512-byte row (wave-tiled)
// or a 32-byte quad per four lanes (sub-tile-minor); the per-lane base and the element / step strides come from io_layout.hpp's maps.
// PF kernels (small plants, the matrices of two steps fit the register file): step t + 1's elements are loaded into a second register set
// before step t's arithmetic, so a wave always has one step of loads in flight.  Larger plants read through the accessor and leave the
// interleaving to the unrolled step body.
//
// Bounds: every access is guarded by b < B; a stack access is (t < N, e < E, b), inside the N * E * NB * 64 doubles every stack is allocated
// with; a batch-major access is vector r < nvec of trajectory b, row t <= N (X) or t < N (U), inside the extents capi.hip has checked.
#include "sens_kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "plan_sens.hpp"

namespace cddp_dev {

namespace {

// one trajectory's view of a stack with E elements per step: element e of step t at p[t * st + e * se]
template <int LAYOUT, int E>
struct StackRef {
  const double *p; size_t st, se;
  __device__ StackRef(const double *base, int NB, int b) {
    const size_t o = cddp_io::internal(LAYOUT, 0, 0, 0, NB, E, 0, b);
    p = base + o;
    se = cddp_io::internal(LAYOUT, 0, 0, 0, 1, E, 1, 0) - cddp_io::internal(LAYOUT, 0, 0, 0, 1, E, 0, 0);   // the same for every trajectory: folds to a constant
    st = cddp_io::internal(LAYOUT, 0, 0, 1, NB, E, 0, b) - o;
  }
};

// accessor of plan_sens.hpp that loads from the stack
struct Strided {
  const double *p; size_t se; int cols;
  __device__ __forceinline__ double operator()(int i, int j) const { return p[(size_t)(i * cols + j) * se]; }
};

template <int NX, int NU>
struct Dims {
  static constexpr int EA = NX * NX, EB = NX * NU, EK = NU * NX, EM = EA + EB + EK;
  static constexpr bool kPrefetch = EM <= 64;   // two register sets of the matrices: at most 256 VGPRs
  // STAGED kernels (the experiment of profiles/r14_plan_sensitivity.md, small plants only): kStage steps of a lane's rows wait in LDS and
  // the wave moves them between LDS and the batch-major arrays as runs, kStage * nx (nu) doubles per trajectory and vector.  Row pitches
  // are odd (inst_io.hip: the 64-bit LDS instructions are conflict-free across lanes exactly then); 4 steps, 2 where 4 would not fit 64 KB
  static constexpr int stage(int rv) { return rv * (NX + NU) > 24 ? 2 : 4; }
  static constexpr int kWide = NX > 10 ? 1 : 4;  // vectors per lane of the wide kernels.  nx >= 12: 4 (and 2) spill, up to 1800 bytes of scratch per lane at nx = 14
};

template <int NX, int NU, int LAYOUT>
struct Stacks {
  using D = Dims<NX, NU>;
  StackRef<LAYOUT, D::EA> A; StackRef<LAYOUT, D::EB> Bm; StackRef<cddp_io::kTiled, D::EK> K;
  __device__ Stacks(const SensStacks &s, int b) : A(s.A, s.NB, b), Bm(s.Bm, s.NB, b), K(s.K, s.NB, b) {}
  __device__ __forceinline__ void load(int t, double (&m)[D::EM]) const {
    const double *a = A.p + (size_t)t * A.st, *bm = Bm.p + (size_t)t * Bm.st, *k = K.p + (size_t)t * K.st;
#pragma unroll
    for (int e = 0; e < D::EA; ++e) m[e] = a[(size_t)e * A.se];
#pragma unroll
    for (int e = 0; e < D::EB; ++e) m[D::EA + e] = bm[(size_t)e * Bm.se];
#pragma unroll
    for (int e = 0; e < D::EK; ++e) m[D::EA + D::EB + e] = k[(size_t)e * K.se];
  }
};

template <int NX, int NU, int LAYOUT, int RV, bool STAGED>
__global__ __launch_bounds__(64) void k_plan_jvp(SensStacks s, int nvec, const double *__restrict__ dx0, double *__restrict__ dX, double *__restrict__ dU) {
  using D = Dims<NX, NU>;
  constexpr int SS = D::stage(RV), PX = (RV * SS * NX) | 1, PU = (RV * SS * NU) | 1;
  __shared__ double sx[STAGED ? 64 * PX : 1], su[STAGED ? 64 * PU : 1];
  const int lane = (int)threadIdx.x, b = (int)blockIdx.x * 64 + lane;
  const bool live = b < s.B;     // STAGED: a dead lane of the last tile walks along (its stack rows are the tile's padding) and helps to store
  if (!STAGED && !live) return;
  const int r0 = (int)blockIdx.y * RV, nr = min(RV, nvec - r0), N = s.N;
  const Stacks<NX, NU, LAYOUT> S(s, b);
  const size_t v0 = (size_t)b * (size_t)nvec + (size_t)r0, vX = (size_t)(N + 1) * NX, vU = (size_t)N * NU;
  double dx[RV][NX], du[RV][NU], dxn[RV][NX];
#pragma unroll
  for (int r = 0; r < RV; ++r) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      dx[r][i] = (live && r < nr) ? dx0[(v0 + r) * NX + i] : 0.0;
      if (live && dX && r < nr) dX[(v0 + r) * vX + i] = dx[r][i];
    }
  }
  // STAGED: the runs of `cnt` steps from step t0 on, out of LDS: element c of the run of (lane l, vector r)
  auto flush = [&](int t0, int cnt) {
    __syncthreads();
    const size_t tile0 = (size_t)blockIdx.x * 64;
    if (dX) {
      const int run = cnt * NX, n = 64 * nr * run;
      for (int idx = lane; idx < n; idx += 64) {
        const int c = idx % run, lr = idx / run, r = lr % nr, l = lr / nr;
        if (tile0 + l < (size_t)s.B) dX[((tile0 + l) * (size_t)nvec + (size_t)(r0 + r)) * vX + (size_t)(t0 + 1) * NX + c] = sx[l * PX + r * (SS * NX) + c];
      }
    }
    if (dU) {
      const int run = cnt * NU, n = 64 * nr * run;
      for (int idx = lane; idx < n; idx += 64) {
        const int c = idx % run, lr = idx / run, r = lr % nr, l = lr / nr;
        if (tile0 + l < (size_t)s.B) dU[((tile0 + l) * (size_t)nvec + (size_t)(r0 + r)) * vU + (size_t)t0 * NU + c] = su[l * PU + r * (SS * NU) + c];
      }
    }
    __syncthreads();
  };
  auto finish = [&](int t) {   // rows du_t and dx_{t+1} out, dx <- dx_{t+1}
    if constexpr (STAGED) {
      const int k = t % SS;
#pragma unroll
      for (int r = 0; r < RV; ++r) {
#pragma unroll
        for (int i = 0; i < NU; ++i) su[lane * PU + r * (SS * NU) + k * NU + i] = du[r][i];
#pragma unroll
        for (int i = 0; i < NX; ++i) { sx[lane * PX + r * (SS * NX) + k * NX + i] = dxn[r][i]; dx[r][i] = dxn[r][i]; }
      }
      if (k == SS - 1) flush(t - (SS - 1), SS);
      else if (t == N - 1) flush(t - k, k + 1);
      return;
    }
#pragma unroll
    for (int r = 0; r < RV; ++r) {
      if (r < nr) {
        if (dU) {
#pragma unroll
          for (int i = 0; i < NU; ++i) dU[(v0 + r) * vU + (size_t)t * NU + i] = du[r][i];
        }
        if (dX) {
#pragma unroll
          for (int i = 0; i < NX; ++i) dX[(v0 + r) * vX + (size_t)(t + 1) * NX + i] = dxn[r][i];
        }
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) dx[r][i] = dxn[r][i];
    }
  };
  if constexpr (D::kPrefetch) {
    double m0[D::EM], m1[D::EM];
    auto step = [&](const double (&m)[D::EM], int t) {
      cddp_sens::jvp_step<NX, NU, RV>(cddp_sens::Dense{m, NX}, cddp_sens::Dense{m + D::EA, NU}, cddp_sens::Dense{m + D::EA + D::EB, NX}, dx, du, dxn);
      finish(t);
    };
    S.load(0, m0);
    for (int t = 0; t < N; t += 2) {
      if (t + 1 < N) S.load(t + 1, m1);
      step(m0, t);
      if (t + 1 >= N) break;
      if (t + 2 < N) S.load(t + 2, m0);
      step(m1, t + 1);
    }
  } else {
    for (int t = 0; t < N; ++t) {
      cddp_sens::jvp_step<NX, NU, RV>(Strided{S.A.p + (size_t)t * S.A.st, S.A.se, NX}, Strided{S.Bm.p + (size_t)t * S.Bm.st, S.Bm.se, NU},
                                      Strided{S.K.p + (size_t)t * S.K.st, S.K.se, NX}, dx, du, dxn);
      finish(t);
    }
  }
}

template <int NX, int NU, int LAYOUT, int RV, bool HAVE_GX, bool HAVE_GU, bool STAGED>
__global__ __launch_bounds__(64) void k_plan_vjp(SensStacks s, int nvec, const double *__restrict__ gX, const double *__restrict__ gU, double *__restrict__ gx0) {
  using D = Dims<NX, NU>;
  constexpr int SS = D::stage(RV), PX = (RV * SS * NX) | 1, PU = (RV * SS * NU) | 1;
  __shared__ double sx[STAGED && HAVE_GX ? 64 * PX : 1], su[STAGED && HAVE_GU ? 64 * PU : 1];
  const int lane = (int)threadIdx.x, b = (int)blockIdx.x * 64 + lane;
  const bool live = b < s.B;     // STAGED: as k_plan_jvp
  if (!STAGED && !live) return;
  const int r0 = (int)blockIdx.y * RV, nr = min(RV, nvec - r0), N = s.N;
  const Stacks<NX, NU, LAYOUT> S(s, b);
  const size_t v0 = (size_t)b * (size_t)nvec + (size_t)r0, vX = (size_t)(N + 1) * NX, vU = (size_t)N * NU;
  double lam[RV][NX], lamn[RV][NX], mu[RV][NU], gx[RV][NX], gu[RV][NU];
#pragma unroll
  for (int r = 0; r < RV; ++r) {
#pragma unroll
    for (int i = 0; i < NX; ++i) { lam[r][i] = (HAVE_GX && live && r < nr) ? gX[(v0 + r) * vX + (size_t)N * NX + i] : 0.0; gx[r][i] = 0.0; }
#pragma unroll
    for (int i = 0; i < NU; ++i) gu[r][i] = 0.0;
  }
  int t_lo = N;                    // STAGED: rows t_lo .. t_lo + SS - 1 wait in LDS
  auto cotangents = [&](int t) {   // rows gX_t and gU_t in
    if constexpr (STAGED && (HAVE_GX || HAVE_GU)) {
      if (t < t_lo) {              // (the same t in every lane) the runs of the next SS steps down, into LDS
        const int cnt = min(SS, t + 1);
        t_lo = t - cnt + 1;
        const size_t tile0 = (size_t)blockIdx.x * 64;
        __syncthreads();
        if constexpr (HAVE_GX) {
          const int run = cnt * NX, n = 64 * nr * run;
          for (int idx = lane; idx < n; idx += 64) {
            const int c = idx % run, lr = idx / run, r = lr % nr, l = lr / nr;
            if (tile0 + l < (size_t)s.B) sx[l * PX + r * (SS * NX) + c] = gX[((tile0 + l) * (size_t)nvec + (size_t)(r0 + r)) * vX + (size_t)t_lo * NX + c];
          }
        }
        if constexpr (HAVE_GU) {
          const int run = cnt * NU, n = 64 * nr * run;
          for (int idx = lane; idx < n; idx += 64) {
            const int c = idx % run, lr = idx / run, r = lr % nr, l = lr / nr;
            if (tile0 + l < (size_t)s.B) su[l * PU + r * (SS * NU) + c] = gU[((tile0 + l) * (size_t)nvec + (size_t)(r0 + r)) * vU + (size_t)t_lo * NU + c];
          }
        }
        __syncthreads();
      }
      const int k = t - t_lo;
#pragma unroll
      for (int r = 0; r < RV; ++r) {
        if (live && r < nr) {
          if constexpr (HAVE_GX) {
#pragma unroll
            for (int i = 0; i < NX; ++i) gx[r][i] = sx[lane * PX + r * (SS * NX) + k * NX + i];
          }
          if constexpr (HAVE_GU) {
#pragma unroll
            for (int i = 0; i < NU; ++i) gu[r][i] = su[lane * PU + r * (SS * NU) + k * NU + i];
          }
        }
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < RV; ++r) {
      if (r < nr) {
        if constexpr (HAVE_GX) {
#pragma unroll
          for (int i = 0; i < NX; ++i) gx[r][i] = gX[(v0 + r) * vX + (size_t)t * NX + i];
        }
        if constexpr (HAVE_GU) {
#pragma unroll
          for (int i = 0; i < NU; ++i) gu[r][i] = gU[(v0 + r) * vU + (size_t)t * NU + i];
        }
      }
    }
  };
  auto finish = [&]() {
#pragma unroll
    for (int r = 0; r < RV; ++r) {
#pragma unroll
      for (int i = 0; i < NX; ++i) lam[r][i] = lamn[r][i];
    }
  };
  if constexpr (D::kPrefetch) {
    double m0[D::EM], m1[D::EM];
    auto step = [&](const double (&m)[D::EM], int t) {
      cotangents(t);
      cddp_sens::vjp_step<NX, NU, RV, HAVE_GX, HAVE_GU>(cddp_sens::Dense{m, NX}, cddp_sens::Dense{m + D::EA, NU}, cddp_sens::Dense{m + D::EA + D::EB, NX}, lam, gx, gu,
                                                        mu, lamn);
      finish();
    };
    S.load(N - 1, m0);
    for (int t = N - 1; t >= 0; t -= 2) {
      if (t - 1 >= 0) S.load(t - 1, m1);
      step(m0, t);
      if (t - 1 < 0) break;
      if (t - 2 >= 0) S.load(t - 2, m0);
      step(m1, t - 1);
    }
  } else {
    for (int t = N - 1; t >= 0; --t) {
      cotangents(t);
      cddp_sens::vjp_step<NX, NU, RV, HAVE_GX, HAVE_GU>(Strided{S.A.p + (size_t)t * S.A.st, S.A.se, NX}, Strided{S.Bm.p + (size_t)t * S.Bm.st, S.Bm.se, NU},
                                                        Strided{S.K.p + (size_t)t * S.K.st, S.K.se, NX}, lam, gx, gu, mu, lamn);
      finish();
    }
  }
#pragma unroll
  for (int r = 0; r < RV; ++r) {
    if (live && r < nr) {
#pragma unroll
      for (int i = 0; i < NX; ++i) gx0[(v0 + r) * NX + i] = lam[r][i];
    }
  }
}

// the distinct (nx, nu) of the model list (dev_models.hpp; LTI: the shapes inst_lti.hip builds): Y(NX, NU)
#ifndef SENS_PAIR_LIST   // (a one-pair build, -D'SENS_PAIR_LIST(Y)=Y(14, 7)', shows one kernel's registers in seconds)
#define SENS_PAIR_LIST(Y) \
  Y(1, 1) Y(2, 1) Y(3, 1) Y(3, 2) Y(4, 1) Y(4, 2) Y(5, 2) Y(6, 2) Y(6, 3) Y(7, 3) Y(8, 3) Y(10, 3) Y(10, 4) Y(12, 4) Y(13, 4) Y(14, 7)
#endif

constexpr int kSensMaxGridY = 65535;

struct JvpArgs { int nvec; const double *dx0; double *dX, *dU; };
struct VjpArgs { int nvec; const double *gX, *gU; double *gx0; };

template <int NX, int NU, int LAYOUT, int RV, bool STAGED>
void launch(const SensStacks &s, const JvpArgs &a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((k_plan_jvp<NX, NU, LAYOUT, RV, STAGED>), grid, dim3(64), 0, st, s, a.nvec, a.dx0, a.dX, a.dU);
}
template <int NX, int NU, int LAYOUT, int RV, bool STAGED>
void launch(const SensStacks &s, const VjpArgs &a, dim3 grid, hipStream_t st) {
  if (a.gX && a.gU) hipLaunchKernelGGL((k_plan_vjp<NX, NU, LAYOUT, RV, true, true, STAGED>), grid, dim3(64), 0, st, s, a.nvec, a.gX, a.gU, a.gx0);
  else if (a.gX) hipLaunchKernelGGL((k_plan_vjp<NX, NU, LAYOUT, RV, true, false, STAGED>), grid, dim3(64), 0, st, s, a.nvec, a.gX, a.gU, a.gx0);
  else if (a.gU) hipLaunchKernelGGL((k_plan_vjp<NX, NU, LAYOUT, RV, false, true, STAGED>), grid, dim3(64), 0, st, s, a.nvec, a.gX, a.gU, a.gx0);
  else hipLaunchKernelGGL((k_plan_vjp<NX, NU, LAYOUT, RV, false, false, false>), grid, dim3(64), 0, st, s, a.nvec, a.gX, a.gU, a.gx0);
}
// the staged kernels exist for the small (prefetching) plants only
template <int NX, int NU, int LAYOUT, int RV, class Args>
void launch_store(const SensStacks &s, const Args &a, bool staged, dim3 grid, hipStream_t st) {
  if constexpr (Dims<NX, NU>::kPrefetch) { if (staged) { launch<NX, NU, LAYOUT, RV, true>(s, a, grid, st); return; } }
  launch<NX, NU, LAYOUT, RV, false>(s, a, grid, st);
}

template <int NX, int NU, class Args>
void launch_pair(const SensStacks &s, const Args &a, int rv, dim3 grid, hipStream_t st) {
  const bool t4 = s.layout == cddp_io::kT4;
  constexpr int W = Dims<NX, NU>::kWide;
  const bool staged = sens_staged();
  if (W > 1 && rv == W) { if (t4) launch_store<NX, NU, cddp_io::kT4, W>(s, a, staged, grid, st); else launch_store<NX, NU, cddp_io::kTiled, W>(s, a, staged, grid, st); }
  else { if (t4) launch_store<NX, NU, cddp_io::kT4, 1>(s, a, staged, grid, st); else launch_store<NX, NU, cddp_io::kTiled, 1>(s, a, staged, grid, st); }
}

template <class Args>
hipError_t dispatch(const SensStacks &s, const Args &a, hipStream_t st) {
  if (s.B <= 0 || s.N <= 0 || a.nvec <= 0) return hipErrorInvalidValue;
  const int rv = sens_chunk(a.nvec, s.nx, (s.B + 63) / 64), passes = (a.nvec + rv - 1) / rv;
  if (passes > kSensMaxGridY) return hipErrorInvalidValue;
  const dim3 grid((s.B + 63) / 64, passes);
#define Y(NX, NU) if (s.nx == NX && s.nu == NU) { launch_pair<NX, NU>(s, a, rv, grid, st); return hipGetLastError(); }
  SENS_PAIR_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

}  // namespace

bool sens_staged() { const char *e = std::getenv("CDDP_HIP_SENS_IO"); return e && !std::strcmp(e, "staged"); }

// Vectors per lane and pass.  The walk is bound by latency, not by traffic, until the grid holds several waves per compute unit: at 64 tiles
// (cart-pole, B = 4096, nvec = 4) four passes of one vector take 0.176 ms and one pass of four 0.211 ms, the time of nvec = 1 being 0.174 ms
// (profiles/r14_plan_sensitivity.md) -- the passes of a tile run side by side and find the matrices in the cache.  So chunks of Dims::kWide
// are used only where the chunked grid alone has kSensWideWaves waves; that crossover is reasoned (4 waves on each of 256 CUs), not measured.
constexpr int kSensWideWaves = 1024;

int sens_chunk(int nvec, int nx, int tiles) {
  const int wide = nx > 10 ? 1 : 4;   // Dims::kWide
  if (nvec < wide) return 1;
  if (const char *e = std::getenv("CDDP_HIP_SENS_RV")) {
    if (e[0] == '1' && !e[1]) return 1;
    if (e[0] == '4' && !e[1]) return wide;
  }
  return (long long)tiles * ((nvec + wide - 1) / wide) >= kSensWideWaves ? wide : 1;
}

hipError_t sens_jvp(const SensStacks &s, int nvec, const double *dx0, double *dX, double *dU, hipStream_t stream) {
  return dispatch(s, JvpArgs{nvec, dx0, dX, dU}, stream);
}

hipError_t sens_vjp(const SensStacks &s, int nvec, const double *gX, const double *gU, double *gx0, hipStream_t stream) {
  return dispatch(s, VjpArgs{nvec, gX, gU, gx0}, stream);
}

}  // namespace cddp_dev
