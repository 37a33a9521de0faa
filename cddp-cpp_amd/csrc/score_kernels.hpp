// Launchers of the scoring kernels (inst_score.hip) for cddp_hip_score_rollouts / cddp_hip_seed_best (capi.hip): roll S candidate control
// sequences per trajectory out on the handle's model or on a plant, with the objective and the constraint rows evaluated along the way.
// Every launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "plant.hpp"

namespace cddp_dev {

// One tile group's share of a call.  Arrays are batch-major and start at the group's first trajectory; g = b * S + c numbers the lanes.
struct ScoreArgs {
  int S;               // candidates per trajectory
  int b0;              // the group's first trajectory in the whole batch (per-trajectory plant parameters)
  int feedback;        // u = U + K_t (x - X_t) around the live slot
  int x0_per_cand;     // x0 is [B][S][nx] instead of [B][nx]
  const double *x0;    // or NULL: row 0 of the live slot
  const double *U;     // [B][S][N][nu], or NULL (feedback only): the live slot's own U
  double *cost, *viol, *X_out, *U_out;   // [B][S], [B][S] | NULL, [B][S][N+1][nx] | NULL, [B][S][N][nu] | NULL
};

// pd: the plant, or the handle's own model dressed as one (substeps 1, h = dt, no box, params = ProblemDev::mp on the device).
// hipErrorInvalidValue: no kernel for this model, or more lanes than a grid holds; nothing launched
hipError_t score_launch(const PlantDev &pd, const DevBuf &d, const ScoreArgs &a, hipStream_t stream);

// winner[b] = cddp_score::select over the S records of trajectory b (score_select.hpp); viol may be NULL
void score_select_launch(int B, int S, const double *cost, const double *viol, double viol_tol, int32_t *winner, hipStream_t stream);

}  // namespace cddp_dev
