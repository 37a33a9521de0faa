// Kernels of the device-resident extended Kalman filter (ekf_kernels.hpp; include/cddp_hip.h "extended Kalman filter on the device"),
// instantiated for every model struct of dev_models.hpp and dispatched on the model id, as inst_plant.hip's: no KernelSet, no solver kernel.
//
// ONE LANE WALKS ONE TRAJECTORY, and a workgroup is a single (possibly partial) wavefront of TL lanes: f and jac are per-lane code, and
// the whole step of a trajectory -- the rows of the update, the relinearisation, the plant step, A P A^T -- is the sequential walk of
// ekf.hpp.  No barrier, no atomics: a lane touches only its own column of LDS.  The estimate xh, the control and the parameter block live
// in registers; P, A = I + h Fx, Bm = h Fu and the product buffer Y = A P live in LDS as [element][TL] doubles, lane-consecutive (an
// 8-byte access of 64 consecutive lanes is two conflict-free passes over the banks), because A and P together do not fit a lane's
// registers from nx = 10 on.  LDS per lane: (3 nx nx + nx nu) * 8 bytes.  TL = 64 up to nx = 8 and 32 from nx = 10 on, the widths the
// sibling kernels settled on, halved while the 160 KB of a CU demand it: (14, 7) runs 16 lanes wide (686 doubles a lane: 85.8 KB).
// Registers, LDS and scratch per model: profiles/r23_ekf.md.
//
// k_ekf_walk serves the three entries (ekf_kernels.hpp, EkfWalk): xh and P are loaded once, kept for all T steps, stored once.  C, v, W
// and Wu are read where they lie at every step: shared by the batch they are wave-uniform addresses (scalar loads, cached), per
// trajectory they are vector loads -- 16 x 14 doubles of C per lane have no other home.  The measurement rows are a run-time loop.
// A row whose s is not > 0 at step t marks the lane dead (info = t + 1 of the first failure): from then on NaN is stored in every
// output row and in the object's state; the lane walks on, on whatever its buffers hold.
//
// Bounds: a lane beyond its launch's trajectories returns at once (there is no barrier to keep it for).  Trajectory b < batch reads
// row b of xh, P, info, of the per-trajectory C / v / W / Wu and parameter blocks, rows (b, t <= T) of Y and of the outputs and
// (b, t < T) of U, inside the extents capi.hip has allocated or checked; C at (r < ny, j < NX); W / Wu at (i, j <= i).  LDS indices are
// (i < NX, j < NX or NU, lane < TL) of the four buffers.
#include "ekf_kernels.hpp"

#include "dev_models.hpp"
#include "plant_models.hpp"
#include "ekf.hpp"

namespace cddp_dev {
namespace {

template <int NX, int NU>
struct EkfTile {
  static constexpr int kDoubles = 3 * NX * NX + NX * NU;                  // per lane
  static constexpr int kWide = NX >= 10 ? 32 : 64;
  static constexpr int kRoom = 160 * 1024 / (kDoubles * 8);               // lanes the LDS of a CU holds
  static constexpr int kLanes = kRoom >= kWide ? kWide : kRoom >= kWide / 2 ? kWide / 2 : kWide / 4;
  static_assert(kLanes * kDoubles * 8 <= 160 * 1024, "the tile fits the LDS of a CU");
};

template <class M, bool PER>
__global__ __launch_bounds__((EkfTile<M::NX, M::NU>::kLanes)) void k_ekf_walk(PlantDev pd, EkfDev e, EkfWalk w) {
  constexpr int NX = M::NX, NU = M::NU, TL = EkfTile<NX, NU>::kLanes;
  __shared__ double sP[NX * NX * TL], sA[NX * NX * TL], sY[NX * NX * TL], sB[NX * NU * TL];
  const int lane = (int)threadIdx.x, bl = (int)blockIdx.x * TL + lane;
  if (bl >= w.B) return;
  const size_t b = (size_t)(w.b0 + bl);
  const cddp_ekf::Mat<TL> P{sP + lane, NX}, A{sA + lane, NX}, Y{sY + lane, NX}, Bm{sB + lane, NU};
  const int ny = e.ny, T = w.T;
  const size_t per = e.per_traj ? b : 0;
  const double *const Cp = e.C + per * (size_t)(ny * NX), *const vp = e.v + per * (size_t)ny;
  const cddp_cov::SymLower W{e.W ? e.W + per * (NX * NX) : nullptr, NX}, Wu{e.Wu ? e.Wu + per * (NU * NU) : nullptr, NU};
  const double nan = __builtin_nan("");
  double p[32], xh[NX];
#pragma unroll
  for (int i = 0; i < 32; ++i) p[i] = PER ? pd.params[(size_t)i * (size_t)pd.Bp + b] : pd.params[i];
#pragma unroll
  for (int i = 0; i < NX; ++i) xh[i] = e.xh[b * NX + i];
  double *const Pb = e.P + b * (NX * NX);
  for (int i = 0; i < NX * NX; ++i) sP[i * TL + lane] = Pb[i];
  int info = e.info[b];

  for (int t = 0; t <= T; ++t) {
    if (t > 0) {
      double u[NU];
#pragma unroll
      for (int i = 0; i < NU; ++i) u[i] = w.U[(b * (size_t)T + (size_t)(t - 1)) * NU + i];
      cddp_ekf::predict<M, Stepper<M>, TL>(pd.integrator, pd.h, p, pd.lower, pd.upper, xh, u, P, A, Bm, Y, W, Wu);
    }
    if (!(t > 0 ? w.upd_after : w.upd0)) continue;
    const size_t row = b * (size_t)(T + 1) + (size_t)t;
    double nis = 0.0;
    for (int r = 0; r < ny; ++r) {
      const int rc = cddp_ekf::update_row<NX, TL>(cddp_kf::Row{Cp + r * NX}, vp[r], w.Y[row * (size_t)ny + r], w.skip_nan != 0, xh, P, nis);
      if (rc == cddp_ekf::kRowFailed && info == 0) info = w.t0 + t + 1;
    }
    const bool dead = info != 0;
    if (w.Xh_out) {
#pragma unroll
      for (int i = 0; i < NX; ++i) w.Xh_out[row * NX + i] = dead ? nan : xh[i];
    }
    if (w.P_out) {
      if (w.diag) {
        for (int i = 0; i < NX; ++i) w.P_out[row * NX + i] = dead ? nan : P(i, i);
      } else {
        for (int i = 0; i < NX * NX; ++i) w.P_out[row * (NX * NX) + i] = dead ? nan : sP[i * TL + lane];
      }
    }
    if (w.nis_out) w.nis_out[row] = dead ? nan : nis;
  }

  const bool dead = info != 0;
#pragma unroll
  for (int i = 0; i < NX; ++i) e.xh[b * NX + i] = dead ? nan : xh[i];
  for (int i = 0; i < NX * NX; ++i) Pb[i] = dead ? nan : sP[i * TL + lane];
  e.info[b] = info;
  if (w.info_out) w.info_out[b] = info;
}

__global__ void k_ekf_reset(EkfDev e, int nx, int B, const double *xh0, const double *P0, int per_traj) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double *src = P0 + (per_traj ? (size_t)b * nx * nx : 0);
  double *dst = e.P + (size_t)b * nx * nx;
  for (int i = 0; i < nx; ++i) {
    e.xh[(size_t)b * nx + i] = xh0[(size_t)b * nx + i];
    for (int j = 0; j <= i; ++j) { const double v = src[i * nx + j]; dst[i * nx + j] = v; dst[j * nx + i] = v; }
  }
  e.info[b] = 0;
}

__global__ void k_ekf_measure(EkfDev e, int nx, int b0, int B, const double *x, const double *yn, double *y) {
  const int bl = blockIdx.x * blockDim.x + threadIdx.x;
  if (bl >= B) return;
  const size_t b = (size_t)(b0 + bl);
  const int ny = e.ny;
  const double *C = e.C + (e.per_traj ? b * (size_t)(ny * nx) : 0);
  for (int r = 0; r < ny; ++r) {
    double m = 0.0;
    for (int j = 0; j < nx; ++j) m += C[r * nx + j] * x[b * nx + j];
    y[b * ny + r] = yn ? m + yn[b * ny + r] : m;
  }
}

__global__ void k_ekf_head(DevBuf d, int nu, int b0, double *u0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  const double *Uc = d.U + (size_t)d.cur[b] * d.planeU;
  for (int i = 0; i < nu; ++i) u0[(size_t)(b0 + b) * nu + i] = Uc[((size_t)(b >> 6) * nu + i) * 64 + (size_t)(b & 63)];
}

__global__ void k_ekf_log(EkfLog l) {
  const int bl = blockIdx.x * blockDim.x + threadIdx.x;
  if (bl >= l.B) return;
  const size_t b = (size_t)(l.b0 + bl), steps = (size_t)l.steps;
  const int nx = l.nx, nu = l.nu, k = l.k;
  if (k >= 0 && l.xh) for (int i = 0; i < nx; ++i) l.Xh_log[(b * steps + k) * nx + i] = l.xh[b * nx + i];
  if (k >= 0 && l.nis) l.nis_log[b * steps + k] = l.nis[b];
  if (k >= 0 && l.u0) {
    for (int i = 0; i < nu; ++i) {
      const double u = l.u0[b * nu + i];
      l.Ulog[((size_t)bl * steps + k) * nu + i] = l.lower ? fmin(fmax(u, l.lower[i]), l.upper[i]) : u;
    }
  }
  if (l.x) for (int i = 0; i < nx; ++i) l.Xlog[((size_t)bl * (steps + 1) + (size_t)(k + 1)) * nx + i] = l.x[b * nx + i];
}

template <class M> bool is_model(int model, int nx, int nu) { return model == M::ID && nx == M::NX && nu == M::NU; }

template <class M, bool PER> void launch(const PlantDev &pd, const EkfDev &e, const EkfWalk &w, hipStream_t s) {
  constexpr int TL = EkfTile<M::NX, M::NU>::kLanes;
  hipLaunchKernelGGL((k_ekf_walk<M, PER>), dim3((w.B + TL - 1) / TL), dim3(TL), 0, s, pd, e, w);
}

}  // namespace

hipError_t ekf_launch_walk(const PlantDev &pd, const EkfDev &e, const EkfWalk &w, hipStream_t s) {
  if (w.B <= 0 || w.T < 0 || e.ny < 1 || e.ny > 16 || !e.C || !e.v || !e.xh || !e.P || !e.info) return hipErrorInvalidValue;
  if ((w.upd0 || (w.T > 0 && w.upd_after)) && !w.Y) return hipErrorInvalidValue;
  if (w.T > 0 && !w.U) return hipErrorInvalidValue;
#define Y(M) if (is_model<M>(pd.model, pd.nx, pd.nu)) { if (pd.per_traj) launch<M, true>(pd, e, w, s); else launch<M, false>(pd, e, w, s); return hipGetLastError(); }
  PLANT_MODEL_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

hipError_t ekf_launch_reset(const EkfDev &e, int nx, int B, const double *xh0, const double *P0, int per_traj, hipStream_t s) {
  hipLaunchKernelGGL(k_ekf_reset, dim3((B + 63) / 64), dim3(64), 0, s, e, nx, B, xh0, P0, per_traj);
  return hipGetLastError();
}

hipError_t ekf_launch_measure(const EkfDev &e, int nx, int b0, int B, const double *x, const double *yn, double *y, hipStream_t s) {
  hipLaunchKernelGGL(k_ekf_measure, dim3((B + 63) / 64), dim3(64), 0, s, e, nx, b0, B, x, yn, y);
  return hipGetLastError();
}

hipError_t ekf_launch_head(const DevBuf &d, int nu, int b0, double *u0, hipStream_t s) {
  hipLaunchKernelGGL(k_ekf_head, dim3((d.B + 63) / 64), dim3(64), 0, s, d, nu, b0, u0);
  return hipGetLastError();
}

hipError_t ekf_launch_log(const EkfLog &l, hipStream_t s) {
  hipLaunchKernelGGL(k_ekf_log, dim3((l.B + 63) / 64), dim3(64), 0, s, l);
  return hipGetLastError();
}

}  // namespace cddp_dev
