// Kernels of the device-resident plant (plant.hpp; include/cddp_hip.h "closed loop against a separate plant"), instantiated for every
// model struct of dev_models.hpp and dispatched on the model id: no KernelSet, no solver kernel.
//
// One lane per trajectory.  The state, the control and the parameter block stay in registers for all substeps of a step (k_plant_step,
// k_plant_head) and for the whole horizon (k_track_plan).  Arithmetic, fixed by the header because the tests are bitwise:
//   u_s[i] = fmin(fmax(u[i], lower[i]), upper[i])                      (only with a box)
//   x <- Stepper<Model>::step(integrator, h, params_b, x, u_s)         substeps times, h = dt / substeps from the host
//   x_next[i] = x[i] + w[i]                                            (only with w)
// Parameters: PER = true reads the trajectory's own block from the parameter-major array (lane-consecutive addresses: one 512-B line per
// entry and wavefront), PER = false reads the shared block at a wave-uniform address (scalar loads: at most 32 doubles, of which a
// plant keeps the few it names -- the unrolled copy of the others is dead code).
#include "plant.hpp"
#include "dev_models.hpp"
#include "plant_models.hpp"

namespace cddp_dev {
namespace {

template <bool PER>
DEV void plant_params(const PlantDev &pd, int bg, double *p) {
#pragma unroll
  for (int i = 0; i < 32; ++i) p[i] = PER ? pd.params[(size_t)i * (size_t)pd.Bp + (size_t)bg] : pd.params[i];
}

// u: the commanded control in, the saturated control out; x: advanced in place by one control interval
template <class M>
DEV void plant_advance(const PlantDev &pd, const double *p, double *x, double *u) {
  constexpr int NX = M::NX, NU = M::NU;
  if (pd.lower) {
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] = fmin(fmax(u[i], pd.lower[i]), pd.upper[i]);
  }
  for (int s = 0; s < pd.substeps; ++s) {
    double xn[NX];
    Stepper<M>::step(pd.integrator, pd.h, p, x, u, xn);
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = xn[i];
  }
}

template <class M, bool PER>
__global__ __launch_bounds__(64) void k_plant_step(PlantDev pd, int B, int b0, const double *xin, const double *uin, const double *w, double *xout) {
  constexpr int NX = M::NX, NU = M::NU;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double p[32], x[NX], u[NU];
  plant_params<PER>(pd, b0 + b, p);
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = xin[(size_t)b * NX + i];
#pragma unroll
  for (int i = 0; i < NU; ++i) u[i] = uin[(size_t)b * NU + i];
  plant_advance<M>(pd, p, x, u);
  if (w) {
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = x[i] + w[(size_t)b * NX + i];
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) xout[(size_t)b * NX + i] = x[i];
}

// the same body on the handle's wave-tiled live slot: row 0 of X and of U at cur[b]
template <class M, bool PER>
__global__ __launch_bounds__(64) void k_plant_head(PlantDev pd, DevBuf d, int b0, const double *W, int steps, int k, double *stage, double *Ulog, double *Xlog) {
  constexpr int NX = M::NX, NU = M::NU;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= d.B) return;
  const size_t tile = (size_t)(b >> 6), lane = (size_t)(b & 63);
  const int cur = d.cur[b];
  const double *Xc = d.X + (size_t)cur * d.planeX, *Uc = d.U + (size_t)cur * d.planeU;
  double p[32], x[NX], u[NU];
  plant_params<PER>(pd, b0 + b, p);
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = Xc[(tile * NX + i) * 64 + lane];
#pragma unroll
  for (int i = 0; i < NU; ++i) u[i] = Uc[(tile * NU + i) * 64 + lane];
  plant_advance<M>(pd, p, x, u);
  if (W) {
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = x[i] + W[((size_t)b * steps + k) * NX + i];
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    stage[(size_t)b * NX + i] = x[i];
    Xlog[((size_t)b * (steps + 1) + k + 1) * NX + i] = x[i];
  }
#pragma unroll
  for (int i = 0; i < NU; ++i) Ulog[((size_t)b * steps + k) * NU + i] = u[i];
}

// u_t = U_t + K_t (x_t - X_t), the sum over j ascending from a zero accumulator; X_t, U_t, K_t are 64-lane rows of the wave-tiled stacks
template <class M, bool PER>
__global__ __launch_bounds__(64) void k_track_plan(PlantDev pd, DevBuf d, int b0, const double *x0, const double *W, double *Xlog, double *Ulog, int NBlog) {
  constexpr int NX = M::NX, NU = M::NU;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= d.B) return;
  const size_t tile = (size_t)(b >> 6), lane = (size_t)(b & 63), NB = (size_t)d.NB;
  const size_t ltile = (size_t)((b0 + b) >> 6), LNB = (size_t)NBlog;
  const int N = d.N;
  const int cur = d.cur[b];
  const double *Xc = d.X + (size_t)cur * d.planeX, *Uc = d.U + (size_t)cur * d.planeU;
  double p[32], x[NX], u[NU], dx[NX];
  plant_params<PER>(pd, b0 + b, p);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    x[i] = x0 ? x0[(size_t)b * NX + i] : Xc[(tile * NX + i) * 64 + lane];
    Xlog[(ltile * NX + i) * 64 + lane] = x[i];
  }
  for (int t = 0; t < N; ++t) {
    const size_t rec = (size_t)t * NB + tile;
#pragma unroll
    for (int j = 0; j < NX; ++j) dx[j] = x[j] - Xc[(rec * NX + j) * 64 + lane];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NX; ++j) s += d.K[(rec * (NU * NX) + i * NX + j) * 64 + lane] * dx[j];
      u[i] = Uc[(rec * NU + i) * 64 + lane] + s;
    }
    plant_advance<M>(pd, p, x, u);
    if (W) {
#pragma unroll
      for (int i = 0; i < NX; ++i) x[i] = x[i] + W[((size_t)b * N + t) * NX + i];
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) Ulog[(((size_t)t * LNB + ltile) * NU + i) * 64 + lane] = u[i];
#pragma unroll
    for (int i = 0; i < NX; ++i) Xlog[(((size_t)(t + 1) * LNB + ltile) * NX + i) * 64 + lane] = x[i];
  }
}

template <class M> bool is_model(int model, int nx, int nu) { return model == M::ID && nx == M::NX && nu == M::NU; }

struct StepArgs { int B, b0; const double *x, *u, *w; double *xn; };
struct HeadArgs { const DevBuf *d; int b0; const double *W; int steps, k; double *stage, *Ulog, *Xlog; };
struct TrackArgs { const DevBuf *d; int b0; const double *x0, *W; double *Xlog, *Ulog; int NBlog; };

template <class M, bool PER> void launch(const PlantDev &pd, const StepArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((k_plant_step<M, PER>), dim3((a.B + 63) / 64), dim3(64), 0, s, pd, a.B, a.b0, a.x, a.u, a.w, a.xn);
}
template <class M, bool PER> void launch(const PlantDev &pd, const HeadArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((k_plant_head<M, PER>), dim3((a.d->B + 63) / 64), dim3(64), 0, s, pd, *a.d, a.b0, a.W, a.steps, a.k, a.stage, a.Ulog, a.Xlog);
}
template <class M, bool PER> void launch(const PlantDev &pd, const TrackArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((k_track_plan<M, PER>), dim3((a.d->B + 63) / 64), dim3(64), 0, s, pd, *a.d, a.b0, a.x0, a.W, a.Xlog, a.Ulog, a.NBlog);
}

template <class Args>
hipError_t dispatch(const PlantDev &pd, const Args &a, hipStream_t s) {
#define Y(M) if (is_model<M>(pd.model, pd.nx, pd.nu)) { if (pd.per_traj) launch<M, true>(pd, a, s); else launch<M, false>(pd, a, s); return hipGetLastError(); }
  PLANT_MODEL_LIST(Y)
#undef Y
  return hipErrorInvalidValue;   // (cddp_hip_plant_create has refused every descriptor that gets here)
}

}  // namespace

bool plant_lti_has(int nx, int nu) { return is_model<Lti11>(CDDP_HIP_MODEL_LTI, nx, nu) || is_model<Lti21>(CDDP_HIP_MODEL_LTI, nx, nu); }

int plant_model_dims(int model, int *nx, int *nu, int *discrete) {
  if (model == CDDP_HIP_MODEL_LTI) { *discrete = 1; return 0; }   // (dimensions: plant_lti_has)
#define Y(M) if (model == M::ID) { *nx = M::NX; *nu = M::NU; *discrete = M::kDiscrete ? 1 : 0; return 0; }
  PLANT_MODEL_LIST(Y)
#undef Y
  return -1;
}

hipError_t plant_launch_step(const PlantDev &pd, int B, int b0, const double *x, const double *u, const double *w, double *x_next, hipStream_t s) {
  return dispatch(pd, StepArgs{B, b0, x, u, w, x_next}, s);
}
hipError_t plant_launch_head(const PlantDev &pd, const DevBuf &d, int b0, const double *W, int steps, int k, double *stage, double *Ulog, double *Xlog, hipStream_t s) {
  return dispatch(pd, HeadArgs{&d, b0, W, steps, k, stage, Ulog, Xlog}, s);
}
hipError_t plant_launch_track(const PlantDev &pd, const DevBuf &d, int b0, const double *x0, const double *W, double *Xlog, double *Ulog, int NBlog, hipStream_t s) {
  return dispatch(pd, TrackArgs{&d, b0, x0, W, Xlog, Ulog, NBlog}, s);
}

}  // namespace cddp_dev
