// Launchers of the sampling kernels (inst_mppi.hip) for cddp_hip_sample_controls / cddp_hip_mppi_blend / cddp_hip_mppi_refine (capi.hip):
// candidate controls are drawn around a mean plan from a counter-based generator (mppi.hpp), so the lane that scores a candidate and the
// lane that blends it draw the same numbers and no [B][S][N][nu] array lies between them.
// Every launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "plant.hpp"

namespace cddp_dev {

constexpr int kMppiMaxNu = 8;   // the widest control of PLANT_MODEL_LIST is 7 (static_assert in inst_mppi.hip)

// The draw of one tile group: passed by value, so sigma and the box are scalar loads wherever the element index is known at compile time.
struct MppiDraw {
  uint64_t seed;
  uint32_t stream;
  int S;               // candidates per trajectory
  int b0;              // the group's first trajectory in the whole batch: the counter carries b0 + b, and so do per-trajectory plant parameters
  int keep_mean;       // candidate 0 takes z = 0
  int box;             // lower / upper hold a box
  int _pad;
  double sigma[kMppiMaxNu], lower[kMppiMaxNu], upper[kMppiMaxNu];
};

// cost[g], viol[g] of candidate g = b * S + c drawn around mean [B][N][nu]: k_score's rollout (no feedback) with the control drawn in the lane.
// x0: [B][nx], or NULL: row 0 of the live slot.  hipErrorInvalidValue: no kernel for this model, or more lanes than a grid holds.
hipError_t mppi_score_launch(const PlantDev &pd, const DevBuf &d, const MppiDraw &a, const double *x0, const double *mean, double *cost, double *viol,
                             hipStream_t stream);

// w [B][S] and stats [B][3] = n_adm, rho, ess from cost and viol [B][S] (viol may be NULL): cddp_mppi::weights, one lane per trajectory
void mppi_weights_launch(int B, int S, const double *cost, const double *viol, double viol_tol, double lambda, double *w, double *stats, hipStream_t stream);

// mean_out [B][N][nu] = the blend of mean_in with weights w; the candidates are read from U_cand [B][S][N][nu], or redrawn when it is NULL.
// stats: the n_adm of mppi_weights_launch (a trajectory without an admissible candidate keeps its mean).  One lane per trajectory and pair.
hipError_t mppi_blend_launch(const MppiDraw &a, int B, int N, int nu, const double *mean_in, const double *U_cand, const double *w, const double *stats,
                             double *mean_out, hipStream_t stream);

// U_out [B][S][N][nu] = the candidates themselves.  One lane per trajectory, candidate and pair.
hipError_t mppi_sample_launch(const MppiDraw &a, int B, int N, int nu, const double *mean, double *U_out, hipStream_t stream);

}  // namespace cddp_dev
