// Launchers of the Monte-Carlo kernels (inst_mc.hip) for cddp_hip_mc_sample_noise / cddp_hip_plan_montecarlo (capi.hip): S noisy closed-loop
// rollouts per trajectory around the live plan, with the noise drawn in the lane (plan_mc.hpp) and the sums over the samples taken on the
// device in a fixed order, so that only moments, counts and per-sample scalars leave it.
// Every launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "plant.hpp"

namespace cddp_dev {

constexpr int kMcMaxNx = 14, kMcMaxNu = 8;   // the widest state and control of PLANT_MODEL_LIST (static_assert in inst_mc.hip)
constexpr int kMcMaxSamples = 1024;          // cddp_mc::kMaxSamples: one workgroup holds the samples of a trajectory

// The lower triangles of the three factors, row i at i (i + 1) / 2: passed by value, so an entry is a scalar load wherever its index is known
// at compile time.
struct McFactors {
  double l0[kMcMaxNx * (kMcMaxNx + 1) / 2], lw[kMcMaxNx * (kMcMaxNx + 1) / 2], lu[kMcMaxNu * (kMcMaxNu + 1) / 2];
};

// One tile group's share of a call.  Arrays are batch-major and start at the group's first trajectory.
struct McArgs {
  uint64_t seed;
  uint32_t stream;
  int S;               // samples per trajectory, 1 .. cddp_mc::kMaxSamples
  int b0;              // the group's first trajectory in the whole batch: the counter carries b0 + b, and so do per-trajectory plant parameters
  int keep_nominal;    // sample 0 takes z = 0
  int have0, havew, haveu;   // which factors there are
  int diag;            // SX / SU hold the diagonals only
  double viol_tol;
  const double *x0;    // [B][nx] or NULL: row 0 of the live slot
  double *cost, *viol, *stats;           // [B][S], [B][S], [B][8]; each may be NULL
  int32_t *nviol_step;                   // [B][N + 1] or NULL
  double *dXmean, *SX, *dUmean, *SU;     // [B][N+1][nx], [B][N+1][nx][nx] | diag [B][N+1][nx], [B][N][nu], [B][N][nu][nu] | diag [B][N][nu]; or NULL
  double *X_out, *U_out;                 // [B][S][N+1][nx], [B][S][N][nu]; or NULL
};

// pd: the plant, or the handle's own model dressed as one (as score_launch takes it).  hipErrorInvalidValue: no kernel for this model.
hipError_t mc_launch(const PlantDev &pd, const DevBuf &d, const McArgs &a, const McFactors &f, hipStream_t stream);

// The coloured noise itself: Z0 [B][S][nx], E [B][S][N][nu], Wn [B][S][N][nx] (each may be NULL; a source without a factor is written as 0).
hipError_t mc_noise_launch(const McArgs &a, const McFactors &f, int B, int N, int nx, int nu, double *Z0, double *E, double *Wn, hipStream_t stream);

}  // namespace cddp_dev
