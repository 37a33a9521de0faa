// Launcher of the reference-window kernel (inst_ref.hip) for cddp_hip_mpc_set_reference_path / cddp_hip_mpc_advance (capi.hip): the window of
// cursor k of a device-resident path (ref_window.hpp) into a tile group's per-step reference buffer and the goal slot of its ProblemDev.
// It enqueues on `stream` and returns; the pointers are the handle's own buffers.
#pragma once
#include <hip/hip_runtime.h>

namespace cddp_dev {

// traj[(N + 1) * nx] <- window rows 0 .. N of cursor k;  goal[nx] <- row N.  path: [L][nx] on the device.
hipError_t ref_window_launch(const double *path, long long L, int nx, int N, long long k, double rows_per_step, double *traj, double *goal, hipStream_t stream);

}  // namespace cddp_dev
