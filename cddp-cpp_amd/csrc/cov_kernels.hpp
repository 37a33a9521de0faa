// Launcher of the plan-covariance kernel (inst_cov.hip): state and control covariance of a solved plan under its own feedback gains, and
// the expected increase of the quadratic objective, from the A / Bm / K stacks where the last backward sweep left them, for
// cddp_hip_plan_covariance (capi.hip).  The arithmetic is the step bodies of plan_cov.hpp; the kernel is templated on (nx, nu) and the
// stack layout only, not on the model.  The launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.
#pragma once
#include <hip/hip_runtime.h>

#include "sens_kernels.hpp"

namespace cddp_dev {

// Sigma0 / W / Wu: nx*nx | nx*nx | nu*nu doubles shared by the batch, or (per_traj) batch-major per trajectory; W and Wu may be null.
// SX [B][N+1][nx][nx], SU [B][N][nu][nu] (diag: [B][N+1][nx], [B][N][nu]), dcost [B]: any may be null, not all.
// Qdt / Rdt / Qf: the handle's cost matrices on the device (ProblemDev::pool), read only when dcost is wanted.
struct CovArgs {
  const double *Sigma0, *W, *Wu;
  double *SX, *SU, *dcost;
  const double *Qdt, *Rdt, *Qf;
  int per_traj, diag;
};

// hipErrorInvalidValue: no kernel for this (nx, nu); nothing launched
hipError_t plan_cov(const SensStacks &s, const CovArgs &a, hipStream_t stream);

}  // namespace cddp_dev
