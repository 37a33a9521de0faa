// The reference window of a path-following MPC step (cddp_hip_mpc_set_reference_path): one small launch per tile group and step that
// writes the (N + 1) * nx doubles of the per-step reference and the nx doubles of the goal from the device-resident path.  The destinations
// are the handle's fixed buffers (the buffer DevBuf::xref_traj points to, ProblemDev::pool + off_xref), which every solver, scoring and
// sampling kernel reads on every launch: no pointer in a DevBuf moves, captured windows stay valid, nothing crosses the bus.
//
// One lane per window element c = t * nx + e; the arithmetic is ref_window.hpp's.  Workgroup 0 also writes the goal (row N).  Stores are
// consecutive doubles along c: whole 512-byte runs per wavefront.  The loads of a row are nx consecutive doubles of one or two path rows.
// Bounds: c < (N + 1) * nx guards the window; a goal lane has e < nx; path indices lie in [0, L - 1] (ref_window.hpp).
#include "ref_kernels.hpp"
#include "ref_window.hpp"

namespace cddp_dev {

namespace {

constexpr int kRefThreads = 256;

__global__ __launch_bounds__(kRefThreads) void k_ref_window(const double *__restrict__ path, long long L, int nx, int N, long long k, double rows_per_step,
                                                            double *__restrict__ traj, double *__restrict__ goal) {
  const int n = (N + 1) * nx, c = (int)blockIdx.x * kRefThreads + (int)threadIdx.x;
  if (c < n) {
    const int t = c / nx, e = c - t * nx;
    traj[c] = cddp_ref::window_elem(path, L, nx, k, rows_per_step, t, e);
  }
  if (blockIdx.x == 0)
    for (int e = (int)threadIdx.x; e < nx; e += kRefThreads) goal[e] = cddp_ref::window_elem(path, L, nx, k, rows_per_step, N, e);
}

}  // namespace

hipError_t ref_window_launch(const double *path, long long L, int nx, int N, long long k, double rows_per_step, double *traj, double *goal, hipStream_t stream) {
  if (!path || !traj || !goal || L < 1 || nx <= 0 || N < 0) return hipErrorInvalidValue;
  const int n = (N + 1) * nx;
  hipLaunchKernelGGL(k_ref_window, dim3((n + kRefThreads - 1) / kRefThreads), dim3(kRefThreads), 0, stream, path, L, nx, N, k, rows_per_step, traj, goal);
  return hipGetLastError();
}

}  // namespace cddp_dev
