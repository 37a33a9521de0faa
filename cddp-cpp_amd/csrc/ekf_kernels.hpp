// Launchers of the extended Kalman filter kernels (inst_ekf.hip) for the cddp_hip_ekf entries of capi.hip.  The arithmetic is the step
// bodies of ekf.hpp; the walk kernel is templated on the model struct (PLANT_MODEL_LIST) and on shared / per-trajectory plant parameters
// and dispatched on the model id, ny is a run-time loop bound.  Every launcher enqueues on `stream` and returns; the pointers are device
// pointers the caller has checked.  All arrays are those of the WHOLE batch, batch-major: a launch covers trajectories [b0, b0 + B).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "plant.hpp"

namespace cddp_dev {

// The estimator: C [ny][nx], v [ny], W [nx][nx], Wu [nu][nu] shared by the batch or (per_traj) one set per trajectory; W, Wu may be null.
// xh [B][nx], P [B][nx][nx] (full, symmetric), info [B]: the object's state.
struct EkfDev {
  int ny, per_traj;
  const double *C, *v, *W, *Wu;
  double *xh, *P;
  int32_t *info;
};

// One walk from the object's state: for t = 0 .. T { t > 0: predict with U[b][t - 1];  (t > 0 ? upd_after : upd0): update with
// Y[b][t], then row t of the outputs }.  cddp_hip_ekf_update is (upd0 = 1, T = 0), cddp_hip_ekf_predict (upd0 = 0, T = 1, upd_after = 0),
// cddp_hip_ekf_run (1, T, 1).  Y [B][T+1][ny], U [B][T][nu], Xh_out [B][T+1][nx], P_out [B][T+1][nx][nx] (diag: [B][T+1][nx]),
// nis_out [B][T+1], info_out [B]: any output may be null.  t0: the object's step count at entry (a failing row at step t: info = t0 + t + 1).
struct EkfWalk {
  int b0, B, t0, T, upd0, upd_after, skip_nan, diag;
  const double *Y, *U;
  double *Xh_out, *P_out, *nis_out;
  int32_t *info_out;
};

// hipErrorInvalidValue: no kernel for this model id; nothing launched
hipError_t ekf_launch_walk(const PlantDev &pd, const EkfDev &e, const EkfWalk &w, hipStream_t stream);
// xh <- xh0 [B][nx];  P <- the lower triangle of P0 ([nx][nx], or per_traj [B][nx][nx]) mirrored;  info <- 0
hipError_t ekf_launch_reset(const EkfDev &e, int nx, int B, const double *xh0, const double *P0, int per_traj, hipStream_t stream);
// y[b][r] = m (+ yn[b][r]),  m = sum_j C[r][j] * x[b][j] from 0.0, j ascending
hipError_t ekf_launch_measure(const EkfDev &e, int nx, int b0, int B, const double *x, const double *yn, double *y, hipStream_t stream);
// row 0 of U of every trajectory's live slot of one tile group (k_gather_plan_head's addressing) -> u0[b0 + b][nu]
hipError_t ekf_launch_head(const DevBuf &d, int nu, int b0, double *u0, hipStream_t stream);
// The closed-loop log of cddp_hip_mpc_run_ekf for MPC step k of one tile group.  Xh_log [B][steps][nx] and nis_log [B][steps] (whole
// batch) take the estimate and nis (k >= 0, xh / nis given);  Ulog [Bg][steps][nu] and Xlog [Bg][steps+1][nx] (the group's) take the
// plant's clip of u0 and the true state x (k >= 0, u0 given: row k + 1 of Xlog;  k < 0: row 0 of Xlog).
struct EkfLog {
  int nx, nu, b0, B, steps, k;
  const double *xh, *nis, *u0, *x, *lower, *upper;
  double *Xh_log, *nis_log, *Ulog, *Xlog;
};
hipError_t ekf_launch_log(const EkfLog &l, hipStream_t stream);

}  // namespace cddp_dev
