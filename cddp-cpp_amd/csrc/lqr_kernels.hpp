// Launcher of the gain-design kernel (inst_lqr.hip): the time-varying LQR gains K_t and cost-to-go matrices P_t of a solved plan's
// linearisation for the caller's tracking weights, from the A / Bm stacks where the last backward sweep left them, for
// cddp_hip_plan_tvlqr (capi.hip).  The arithmetic is the step bodies of plan_lqr.hpp; the kernel is templated on (nx, nu) and the stack
// layout only, not on the model.  The launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sens_kernels.hpp"

namespace cddp_dev {

// Q / Qf: nx*nx doubles, R: nu*nu, each ONE matrix for the batch or (q_per / r_per / qf_per) batch-major per trajectory; only lower
// triangles are read.  q_scale / r_scale: what every element of Q / R is multiplied by where it is read (dt for a caller's weight, 1 for
// the handle's own Q dt / R dt in ProblemDev::pool).  K_out [B][N][nu][nx], P_out [B][N+1][nx][nx], info [B]: any may be null.
// K_stack: the group's wave-tiled gain stack (DevBuf::K) to write K_t into as well, or null.  Not all of K_out, P_out, K_stack null.
struct LqrArgs {
  const double *Q, *R, *Qf;
  int q_per, r_per, qf_per;
  double q_scale, r_scale;
  double *K_out, *P_out, *K_stack;
  int32_t *info;
};

// hipErrorInvalidValue: no kernel for this (nx, nu); nothing launched.  s.K is not read.
hipError_t plan_lqr(const SensStacks &s, const LqrArgs &a, hipStream_t stream);

}  // namespace cddp_dev
