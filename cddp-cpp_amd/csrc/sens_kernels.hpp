// Launchers of the plan-sensitivity kernels (inst_sens.hip): the linear response of a solved plan to its initial state, forward (JVP) and
// adjoint (VJP), from the A / Bm / K stacks where the last backward sweep left them, for cddp_hip_plan_jvp / cddp_hip_plan_vjp (capi.hip).
// The arithmetic is the step bodies of plan_sens.hpp; the kernels are templated on (nx, nu) and the stack layout only, not on the model.
// Every launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.  All arrays batch-major
// [b][r][t][e] for b < B, r < nvec (include/cddp_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include "io_layout.hpp"

namespace cddp_dev {

// the stacks of one tile group: layout = cddp_io::kT4 or kTiled for A / Bm; K is always wave-tiled
struct SensStacks { const double *A, *Bm, *K; int layout, B, NB, N, nx, nu; };

// Vectors a lane carries per pass: 1, or chunks of 4 (never for nx > 10: wider chunks spill there) once the chunked grid alone fills the
// machine (inst_sens.hip::sens_chunk).  CDDP_HIP_SENS_RV=1 / =4 (read at every call: a switch of profiles/scripts/plan_sensitivity.py and
// of the tests) forces one or the other; the results are the same bits.
int sens_chunk(int nvec, int nx, int tiles);
// CDDP_HIP_SENS_IO=staged (read at every call, the same script's switch) moves the batch-major rows of the small plants (the kernels that
// prefetch) through LDS in runs of a few steps instead of one 8-byte access per lane and element; the results are the same bits.
bool sens_staged();

// hipErrorInvalidValue: no kernel for this (nx, nu) or more passes than a grid holds; nothing launched
hipError_t sens_jvp(const SensStacks &s, int nvec, const double *dx0, double *dX, double *dU, hipStream_t stream);
hipError_t sens_vjp(const SensStacks &s, int nvec, const double *gX, const double *gU, double *gx0, hipStream_t stream);

}  // namespace cddp_dev
