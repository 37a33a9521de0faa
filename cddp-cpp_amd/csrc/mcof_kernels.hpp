// Launchers of the output-feedback Monte-Carlo kernels (inst_mcof.hip) for cddp_hip_mc_sample_meas_noise / cddp_hip_plan_montecarlo_of
// (capi.hip): mc_kernels.hpp's rollouts with a linearised Kalman estimator carried in every lane (plan_mcof.hpp) -- the feedback acts on
// the estimate, the error's moments are reduced with the state's.
// Every launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.
#pragma once
#include "mc_kernels.hpp"

namespace cddp_dev {

constexpr int kMcofMaxNy = 16;   // CDDP_HIP_KF_MAX_NY

// What one tile group's share of a call adds to McArgs.  Arrays are batch-major and start at the group's first trajectory.
struct McofArgs {
  int ny;                       // measurement rows, 1 .. kMcofMaxNy
  int t4;                       // the A / Bm stacks are sub-tile-minor (cddp_io::kT4) instead of wave-tiled
  const double *C, *sd;         // [ny][nx], [ny] = sqrt(v): one for the batch, read wave-uniformly
  const double *L;              // [B][N+1][nx][ny] the filter gains
  double *dEmean, *SE, *Xh_out; // [B][N+1][nx], [B][N+1][nx][nx] | diag [B][N+1][nx], [B][S][N+1][nx]; or NULL
};

// pd: the plant, or the handle's own model dressed as one.  d.A, d.Bm and d.K must be there.  hipErrorInvalidValue: no kernel for this model.
hipError_t mcof_launch(const PlantDev &pd, const DevBuf &d, const McArgs &a, const McFactors &f, const McofArgs &o, hipStream_t stream);

// The measurement noise itself: Yn [B][S][N+1][ny], row t = sd[r] * z of step t.  Of a: seed, stream, S, b0 and keep_nominal are read.
hipError_t mcof_noise_launch(const McArgs &a, int B, int N, int nx, int nu, int ny, const double *sd, double *Yn, hipStream_t stream);

}  // namespace cddp_dev
