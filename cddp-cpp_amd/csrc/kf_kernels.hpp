// Launcher of the filter kernel (inst_kf.hip): the Kalman filter gains of a solved plan's linearisation for the caller's sensors and the
// covariance of states and controls when the plan's feedback acts on the filtered estimate, from the A / Bm / K stacks where the last
// backward sweep left them, for cddp_hip_plan_kalman (capi.hip).  The arithmetic is the step bodies of plan_kf.hpp and plan_cov.hpp; the
// kernel is templated on (nx, nu) and the stack layout only, not on the model or on ny.  The launcher enqueues on `stream` and returns;
// the pointers are device pointers the caller has checked.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sens_kernels.hpp"

namespace cddp_dev {

// C [ny][nx], v [ny], Sigma0 / W [nx][nx], Wu [nu][nu]: shared by the batch, or (per_traj) batch-major per trajectory, all of them; W and
// Wu may be null.  L [B][N+1][nx][ny], SP / SF / SX [B][N+1][nx][nx], SU [B][N][nu][nu] (diag: SP / SF / SX [B][N+1][nx], SU [B][N][nu]),
// dcost [B], info [B]: any may be null, not all.  Qdt / Rdt / Qf: the handle's cost matrices on the device (ProblemDev::pool), read only
// when dcost is wanted.  1 <= ny <= 16 is the caller's to check.
struct KfArgs {
  int ny;
  const double *C, *v, *Sigma0, *W, *Wu;
  double *L, *SP, *SF, *SX, *SU, *dcost;
  int32_t *info;
  const double *Qdt, *Rdt, *Qf;
  int per_traj, diag;
};

// hipErrorInvalidValue: no kernel for this (nx, nu); nothing launched
hipError_t plan_kf(const SensStacks &s, const KfArgs &a, hipStream_t stream);

}  // namespace cddp_dev
