// Device-resident plant (cddp_hip_plant, include/cddp_hip.h "closed loop against a separate plant"): what capi.hip (host side: descriptor
// checks, buffers, sequencing) and inst_plant.hip (the kernels, dispatched on the model id over the model structs of dev_models.hpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.hpp"

namespace cddp_dev {

// What a plant kernel is given by value.  params: the DERIVED parameter blocks (32 doubles, cddp_host_model_params applied to the caller's
// 24 entries) -- per_traj = 0: one block, read at a wave-uniform address; per_traj = 1: parameter-major [32][Bp], entry i of trajectory b at
// params[i * Bp + b], so the 64 lanes of a wavefront load one 512-B line per entry.  lower / upper: nu doubles each or both NULL.
struct PlantDev {
  int model, integrator, substeps, nx, nu, per_traj, Bp, _pad;
  double h;                       // dt / substeps, divided once on the host
  const double *params, *lower, *upper;
};

// model id -> dimensions of the plant (LTI: nx, nu pick the instantiation); 0, or -1 when the library has no such plant
int plant_model_dims(int model, int *nx, int *nu, int *discrete);
bool plant_lti_has(int nx, int nu);

// One plant step of trajectories [0, B) (parameters of trajectory b0 + b): batch-major x (B * nx), u (B * nu), w (B * nx or NULL) -> x_next.
hipError_t plant_launch_step(const PlantDev &pd, int B, int b0, const double *x, const double *u, const double *w, double *x_next, hipStream_t s);
// The MPC step of one tile group: row 0 of X and of U of every trajectory's live slot (k_gather_plan_head's addressing) -> the plant ->
// stage (batch-major B * nx, what k_mpc_state consumes) and rows k of the group's logs (saturated u_0 into Ulog, x_next into Xlog row k + 1).
// W: this group's disturbances (B * steps * nx, batch-major) on the device, or NULL.
hipError_t plant_launch_head(const PlantDev &pd, const DevBuf &d, int b0, const double *W, int steps, int k, double *stage, double *Ulog, double *Xlog, hipStream_t s);
// Gain-tracking rollout of one tile group over the horizon: u_t = U_t + K_t (x_t - X_t) on the live slot and the gain stack, then the plant.
// x0 (B * nx, batch-major) or NULL = row 0 of the plan; W (B * N * nx) or NULL.  Xlog / Ulog: wave-tiled logs of the WHOLE batch
// ([N + 1][NBlog][nx][64], [N][NBlog][nu][64]); the group writes the tiles b0 / 64 ...
hipError_t plant_launch_track(const PlantDev &pd, const DevBuf &d, int b0, const double *x0, const double *W, double *Xlog, double *Ulog, int NBlog, hipStream_t s);

}  // namespace cddp_dev
