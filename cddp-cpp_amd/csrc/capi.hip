// C-ABI of the MI355X-native batched CLDDP / IPDDP solver core (include/cddp_hip.h).
// Host side only: descriptor flattening, device-buffer ownership, kernel sequencing
// (the device-resident per-trajectory state machine lives in kernels.hpp).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <map>

#include "launch.hpp"
#include "plant.hpp"
#include "io_kernels.hpp"
#include "sens_kernels.hpp"
#include "cov_kernels.hpp"
#include "lqr_kernels.hpp"
#include "kf_kernels.hpp"
#include "score_kernels.hpp"
#include "mppi_kernels.hpp"
#include "mc_kernels.hpp"
#include "mcof_kernels.hpp"
#include "ref_kernels.hpp"
#include "ekf_kernels.hpp"

// 1 when a[0] > a[1] > ... > a[n - 1] (NaN-free): the ladders cddp_hip_build_alphas makes; DevBuf::ladder_sorted
static int ladder_strictly_decreasing(const double *a, int n) {
  for (int i = 1; i < n; ++i) if (!(a[i] < a[i - 1])) return 0;
  return n > 0 ? 1 : 0;
}

using namespace cddp_dev;

namespace cddp_dev {
// gather records for the RCCL all-gather
static __global__ void k_gather_records(DevBuf d, cddp_hip_gather_record *out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  cddp_hip_gather_record r;
  r.final_objective = d.cost[b]; r.iterations = d.iter[b]; r.status = d.status[b];
  out[b] = r;
}

// head of the plan: u_0 and x_1 of every trajectory's CURRENT iterate (batch-major), what a receding-horizon caller reads back
static __global__ void k_gather_plan_head(DevBuf d, int nx, int nu, double *out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  const int cur = d.cur[b];
  const double *Xc = d.X + (size_t)cur * d.planeX, *Uc = d.U + (size_t)cur * d.planeU;
  double *o = out + (size_t)b * (nu + nx);
  for (int i = 0; i < nu; ++i) o[i] = Uc[((((size_t)0 * d.NB + (size_t)(b >> 6)) * nu + i) * 64) + (size_t)(b & 63)];
  for (int i = 0; i < nx; ++i) o[nu + i] = Xc[((((size_t)1 * d.NB + (size_t)(b >> 6)) * nx + i) * 64) + (size_t)(b & 63)];
}

// ---- device-resident MPC step (cddp_hip_mpc_advance / cddp_hip_mpc_run) ----------------------------------------
// The shifted seed of the next solve is a row permutation of every trajectory's CURRENT iterate (slot cur[b]): it never leaves the device.
//
// k_mpc_shift: one lane per (trajectory b, element e); blockIdx.x = 64-trajectory tile, blockIdx.y = element over [X | U | S | Y].  The lane
// walks t UPWARDS for its own (b, e): it reads row t + 1 of the live slot and writes row t of the seed copy (Xinit / Uinit, what restore_initial
// reads) AND row t of the live slot itself, so cur[b] and everything else a warm re-initialisation stages from the live slot (slack / dual /
// costate rows, k_stage) stay where they are and the getters, which read slot cur[b], return the shifted plan.  Race-free: the addresses of
// (b, e, any t) in the live slot and in the seed are touched by this one lane only, and within the lane row t + 1 is read before the same
// iteration of the walk writes row t and before the NEXT iteration overwrites row t + 1 (program order of one thread) -- no second launch, no
// grid-wide ordering.  A grid that spread t over blocks would read row t + 1 while another block writes it.
// Coalescing: the 64 lanes of a wavefront are the 64 trajectories of one tile, so a row access is one 512-B line per slot value present among them.
// The last row repeats (X_shifted[N] = X[N], U_shifted[N - 1] = U[N - 1]).  Padding lanes (b >= B) of X / U are left alone: the seed keeps what
// cddp_hip_set_initial put there.  S / Y (shift_duals): row t of EVERY slot receives the shifted row and padding lanes zeros, as cddp_hip_set_duals writes them.
static __global__ __launch_bounds__(64) void k_mpc_shift(DevBuf d, int nx, int nu, int m, int shift_duals, double *Xinit, double *Uinit) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  int e = blockIdx.y;
  const size_t tile = (size_t)(b >> 6), lane = (size_t)(b & 63), NB = (size_t)d.NB;
  const int N = d.N;
  const int cur = b < d.B ? d.cur[b] : 0;
  if (e < nx) {
    if (b >= d.B) return;
    double *Xc = d.X + (size_t)cur * d.planeX;
    for (int t = 0; t <= N; ++t) {
      const size_t dst = (((size_t)t * NB + tile) * nx + e) * 64 + lane, src = (((size_t)(t < N ? t + 1 : N) * NB + tile) * nx + e) * 64 + lane;
      const double v = Xc[src];
      Xc[dst] = v; Xinit[dst] = v;
    }
    return;
  }
  e -= nx;
  if (e < nu) {
    if (b >= d.B) return;
    double *Uc = d.U + (size_t)cur * d.planeU;
    for (int t = 0; t < N; ++t) {
      const size_t dst = (((size_t)t * NB + tile) * nu + e) * 64 + lane, src = (((size_t)(t < N - 1 ? t + 1 : N - 1) * NB + tile) * nu + e) * 64 + lane;
      const double v = Uc[src];
      Uc[dst] = v; Uinit[dst] = v;
    }
    return;
  }
  e -= nu;
  if (!shift_duals || e >= 2 * m) return;
  double *base = e < m ? d.S : d.Y;
  if (e >= m) e -= m;
  const double *live = base + (size_t)cur * d.planeM;
  for (int t = 0; t < N; ++t) {
    const size_t dst = (((size_t)t * NB + tile) * m + e) * 64 + lane, src = (((size_t)(t < N - 1 ? t + 1 : N - 1) * NB + tile) * m + e) * 64 + lane;
    const double v = b < d.B ? live[src] : 0.0;   // (read before the slot loop below overwrites row t of the live slot; row t + 1 is still the old one)
    for (int sl = 0; sl < d.n_slots; ++sl) base[(size_t)sl * d.planeM + dst] = v;
  }
}

// k_mpc_state: row 0 of the seed from the measured state x_next (batch-major, on the device) or, x_next == NULL and every_slot, from row 1 of
// the live slot.  every_slot = 1 (KEEP_PLAN): row 0 of Xinit and of EVERY slot, padding lanes zero, as cddp_hip_set_initial_state writes them;
// every_slot = 0 (after k_mpc_shift): row 0 of Xinit and of the live slot, X_[0] = initial_state as cddp_hip_set_initial writes it.
static __global__ void k_mpc_state(DevBuf d, int nx, const double *x_next, int every_slot, double *Xinit) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.Bp || (b >= d.B && !every_slot)) return;
  const size_t tile = (size_t)(b >> 6), lane = (size_t)(b & 63), NB = (size_t)d.NB;
  const int cur = b < d.B ? d.cur[b] : 0;
  for (int e = 0; e < nx; ++e) {
    const size_t r0 = (((size_t)0 * NB + tile) * nx + e) * 64 + lane, r1 = (((size_t)1 * NB + tile) * nx + e) * 64 + lane;
    const double v = b >= d.B ? 0.0 : (x_next ? x_next[(size_t)b * nx + e] : d.X[(size_t)cur * d.planeX + r1]);
    Xinit[r0] = v;
    if (every_slot) for (int sl = 0; sl < d.n_slots; ++sl) d.X[(size_t)sl * d.planeX + r0] = v;
    else d.X[(size_t)cur * d.planeX + r0] = v;
  }
}

// the closed-loop log of cddp_hip_mpc_run, in the layout of its outputs: u_0 and x_1 (k_gather_plan_head's addressing), iteration count and
// status of MPC step k of every trajectory; k < 0: the initial state of the first solve (row 0 of the seed) into X_visited[:, 0]
static __global__ void k_mpc_log(DevBuf d, int nx, int nu, int steps, int k, const double *Xinit, double *Ulog, double *Xlog, int32_t *itlog, int32_t *stlog) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  const size_t tile = (size_t)(b >> 6), lane = (size_t)(b & 63), NB = (size_t)d.NB;
  if (k < 0) {
    for (int i = 0; i < nx; ++i) Xlog[((size_t)b * (steps + 1)) * nx + i] = Xinit[(((size_t)0 * NB + tile) * nx + i) * 64 + lane];
    return;
  }
  const int cur = d.cur[b];
  const double *Xc = d.X + (size_t)cur * d.planeX, *Uc = d.U + (size_t)cur * d.planeU;
  for (int i = 0; i < nu; ++i) Ulog[((size_t)b * steps + k) * nu + i] = Uc[(((size_t)0 * NB + tile) * nu + i) * 64 + lane];
  for (int i = 0; i < nx; ++i) Xlog[((size_t)b * (steps + 1) + k + 1) * nx + i] = Xc[(((size_t)1 * NB + tile) * nx + i) * 64 + lane];
  itlog[(size_t)b * steps + k] = d.iter[b]; stlog[(size_t)b * steps + k] = d.status[b];
}

// CDDPOptions::max_cpu_time expired (cddp_solver_base.cpp:77-90): the check sits after ++iter and before the
// backward pass, so every trajectory still running reports the iteration the check fired in.
static __global__ void k_mark_cpu_time(DevBuf d) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B || d.phase[b] == PH_DONE) return;
  d.iter[b] += 1; d.status[b] = CDDP_HIP_STATUS_MAX_CPU_TIME; d.phase[b] = PH_DONE;
}

}  // namespace cddp_dev

int cddp_host_model_eval(int model, int integrator, double dt, const double *params, int nx, int nu, const double *x, const double *u, double *x_next,
                         double *fx, double *fu, double *fxx, double *fuu, double *fux, std::string &err);   // host_models.cpp
int cddp_host_model_params(int model, int nx, int nu, const double *in, double *out, std::string &err);         // host_models.cpp

namespace {

thread_local std::string g_err;
int fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace
extern "C" int cddp_hip_internal_set_error(int code, const char *msg) { g_err = msg ? msg : ""; return code; }   // comm.hip
extern "C" int cddp_hip_internal_allgather(const void *send, void *recv, size_t bytes_per_rank, void *comm, void *stream);
namespace {
#define HIPCHK(expr)                                                                          \
  do { hipError_t e_ = (expr); if (e_ != hipSuccess)                                           \
      return fail(-10, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

const std::vector<KernelSet> &registry() {
  static std::vector<KernelSet> v = [] {
    std::vector<KernelSet> r;
    register_pendulum(r); register_cartpole(r); register_unicycle(r); register_lti(r);
    register_quadrotor(r); register_quad12(r); register_manipulator(r); register_manip7(r); register_terminal(r); register_statebox(r);
    register_vehicles(r); register_spacecraft(r); register_plants_small(r); register_plants_nx10(r);
    return r;
  }();
  return v;
}

}  // namespace

// ---- CU-partitioned streams (round 5) --------------------------------------------------------------------------
// CDDP_HIP_CUMASK = "<spec>[|<spec> ...]", one spec per tile group (the last one repeats), spec = comma-separated "X=lo-hi" with
//   C = the group's main stream (derivative fill, condensation, post, costate, update), F = its rollout stream, W = its serial-sweep stream
// and [lo, hi) a range of CU-mask bits.  On gfx942 / gfx950 the KFD maps mask bit i to XCC i % 8, then shader engine, then CU
// (kfd_mqd_manager.c::mqd_symmetrically_map_cu_mask), so a contiguous bit range is a symmetric slice of every XCD.  A class without
// a range runs on the main stream (F, W) or on an unmasked stream (C).  Kernels of one group on different streams are ordered by
// events (SolveRun::enqueue_iteration, launch.hpp::sweep_hop_in / out); nothing else changes, so results are bitwise those of one
// stream (tests/test_determinism.py).
//   "X=x<digits>" instead of a range: the whole of the named XCDs (bits i with i % 8 among the digits).
struct CuSpec { int lo[3] = {-1, -1, -1}, hi[3] = {-1, -1, -1}; unsigned xcd[3] = {0, 0, 0}; };   // index 0 = C, 1 = F, 2 = W; xcd: bit k = XCD k (0 = a range)
struct CuPlan {
  hipStream_t fwd = nullptr, sweep = nullptr;   // nullptr: the main stream
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // main->fwd, fwd->main (stage 1, stage 2); main->sweep, sweep->main
  SweepHop hop{nullptr, nullptr, nullptr};
};

struct Inner {
  ProblemDev P;
  DevBuf d;
  const KernelSet *ks = nullptr;
  const Knobs *knob = nullptr;   // the handle's switches (cddp_hip_handle::knob)
  Route route;                   // the kernel route (resolve_route); route.t4 is d.t4
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  CuPlan cu;
  std::vector<void *> allocs;
  ProblemDev *dP = nullptr;
  double *d_xref_traj = nullptr;
  unsigned long long *d_launched = nullptr;
  double *d_Xinit = nullptr, *d_Uinit = nullptr;   // initial trajectory kept on the device so solve() is repeatable
  bool have_initial = false;
  bool initialized = false;
  bool has_state = false;        // gains / duals of an earlier initialize() or solve() live on the device (warm start)
  bool initial_dirty = false;    // set_initial() since the last initialize(): the caller supplied a new trajectory
  bool ms_cache_started = false; // MSIPDDP: the per-step factor cache has been cleared once (it lives as long as the handle)
  size_t bytes = 0;
  int timing_detail = CDDP_HIP_TIMING_ROLLOUT;   // which kernel classes cddp_hip_solve brackets with events
  std::vector<hipEvent_t> ev_pool;               // reused across solves (creating an event per mark costs host time)
  hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_poll = nullptr, ev_poll2 = nullptr;
  double *d_head = nullptr, *h_head = nullptr; size_t head_cap = 0;   // cddp_hip_get_plan_head staging (device, pinned host)
  int *h_poll = nullptr;                         // pinned host words of the solve loop's polls, two slots of kPollWords: [0] running count, [1..] alpha histogram
  std::map<unsigned long long, hipGraphExec_t> graphs;   // CDDP_HIP_GRAPH=1: captured iteration windows by (ladder shape, length, last flag)
  // shadow costate (K4b deferred into the next sweep launch; SolveRun::enqueue_iteration, kernels_lean.hpp "K4b, deferred")
  bool shadow_bufs = false;      // the second value stack and the accept records are allocated (layout eligible at create)
  int cs_epoch = 0;              // stamps handed out: two per enqueued outer iteration over the handle's life (SolveRun::enqueue_iteration)
  unsigned long long *h_ls = nullptr;   // pinned host copy of the rollout counter and the stage-2 tile counters (dev_types.hpp, kLsRan ...)
  long long ls_counts[3] = {0, 0, 0};   // the last solve's stage-2 tiles that ran / returned at once / gave the poll up (cddp_hip_ls_stage_counts)
  int n_redo = 0;                // speculative solves discarded and run again with K4b on the chain (cddp_hip_costate_redos)
  bool last_shadow = false;      // the last solve ran (and kept) the shadow schedule (cddp_hip_costate_mode)
  bool ever_solved = false;
  int *h_bad = nullptr;          // pinned host copy of DevBuf::cs_bad
  // device-resident MPC step (cddp_hip_mpc_advance / cddp_hip_mpc_run)
  bool has_plan = false;         // an initialize() or solve() has run: slot cur[b] holds every trajectory's current plan
  double *d_xnext = nullptr;     // staging of a host x_next (B * nx doubles, batch-major): the one upload of an MPC step
  double *d_log_u = nullptr, *d_log_x = nullptr; int32_t *d_log_it = nullptr, *d_log_st = nullptr; int log_steps = 0;   // closed-loop log of cddp_hip_mpc_run
  // movable goal / per-step reference (cddp_hip_set_reference, cddp_hip_mpc_set_reference_path)
  bool goal_on_device = false;   // the goal slot of dP was last written ON the device (device-pointer setter, window kernel): P.pool's copy is
                                 // stale and is read back (goal_to_host) before P is uploaded whole again
  double *d_path = nullptr;      // the bound reference path, [path_L][nx], this group's own copy; nullptr: no path bound
  long long path_L = 0, path_cursor = -1;
  double path_rps = 1.0;
};

namespace {

template <class T>
int dalloc(Inner *h, T **p, size_t n) {
  if (n == 0) n = 1;
  void *q = nullptr;
  HIPCHK(hipMalloc(&q, n * sizeof(T)));
  HIPCHK(hipMemsetAsync(q, 0, n * sizeof(T), h->stream));
  h->allocs.push_back(q);
  h->bytes += n * sizeof(T);
  *p = (T *)q;
  return 0;
}

int pool_put(ProblemDev &P, int &top, const double *src, int n) {
  if (top + n > kPool) return -1;
  int off = top;
  for (int i = 0; i < n; ++i) P.pool[off + i] = src[i];
  top += n;
  return off;
}

// plants with device-side Hessian tensors (dev_models.hpp: Model::kHasHess) -- full DDP (options.use_ilqr = 0) needs them
bool model_has_hessians(int model) {
  return model == CDDP_HIP_MODEL_PENDULUM || model == CDDP_HIP_MODEL_CARTPOLE || model == CDDP_HIP_MODEL_UNICYCLE || model == CDDP_HIP_MODEL_LTI ||
         model == CDDP_HIP_MODEL_BICYCLE || model == CDDP_HIP_MODEL_CAR || model == CDDP_HIP_MODEL_MANIPULATOR || model == CDDP_HIP_MODEL_HCW ||
         model == CDDP_HIP_MODEL_QUADROTOR || model == CDDP_HIP_MODEL_QUADROTOR_EULER12 || model == CDDP_HIP_MODEL_MANIPULATOR7 ||   // round 4: blocked second-order duals
         model == CDDP_HIP_MODEL_EULER_ATTITUDE || model == CDDP_HIP_MODEL_QUATERNION_ATTITUDE || model == CDDP_HIP_MODEL_MRP_ATTITUDE ||
         model == CDDP_HIP_MODEL_SPACECRAFT_LANDING2D ||   // (SpacecraftTwobody: none -- the reference's cross Hessian throws)
         model == CDDP_HIP_MODEL_DUBINS_CAR || model == CDDP_HIP_MODEL_DREYFUS_ROCKET || model == CDDP_HIP_MODEL_ACROBOT || model == CDDP_HIP_MODEL_USV_3DOF ||
         model == CDDP_HIP_MODEL_FORKLIFT || model == CDDP_HIP_MODEL_SPACECRAFT_LINEAR_FUEL || model == CDDP_HIP_MODEL_QUADROTOR_RATE;   // (SpacecraftNonlinear: none, as SpacecraftTwobody)
}

// the refusal of options.use_ilqr = 0 for a plant without Hessian tensors
int fail_no_hessians(int model) {
  if (model == CDDP_HIP_MODEL_SPACECRAFT_NONLINEAR) return fail(-3, "use_ilqr=false: %s", SpacecraftNonlinearModel::kNoHessMsg);
  if (model == CDDP_HIP_MODEL_SPACECRAFT_TWOBODY) return fail(-3, "use_ilqr=false: %s", SpacecraftTwobodyModel::kNoHessMsg);
  return fail(-3, "use_ilqr=false needs the plant's Hessian tensors, which model id %d does not have", model);
}

// The ladder a solver walks.  CLDDP, IPDDP and MSIPDDP walk the context's alphas_ = detail::buildLineSearchAlphas (cddp_core.cpp:60, 111);
// LogDDP rebuilds the ladder in its initialize as the plain geometric sequence, without the stop at ls_min_step_size
// (logddp_solver.cpp:104-109, 177-182).  alphas == NULL: the ladder's own length.
int build_ladder(int solver, const cddp_hip_options *opt, double *alphas, int cap) {
  if (solver != CDDP_HIP_SOLVER_LOGDDP) return cddp_hip_build_alphas(opt, alphas, cap);
  int n = 0;
  double cur = opt->ls_initial_step_size;
  for (int i = 0; i < opt->ls_max_iterations; ++i) { if (alphas && n < cap) alphas[n] = cur; ++n; cur *= opt->ls_step_reduction_factor; }
  return (alphas && n > cap) ? cap : n;
}

// cddp_hip_problem -> ProblemDev (constraints sorted by name as std::map iterates)
int flatten(const cddp_hip_problem *p, ProblemDev &P) {
  std::memset(&P, 0, sizeof(P));
  if (p->abi_version != CDDP_HIP_ABI_VERSION) return fail(-2, "ABI version mismatch: got %d want %d", p->abi_version, CDDP_HIP_ABI_VERSION);
  if (p->nx <= 0 || p->nu <= 0 || p->horizon <= 0 || !(p->dt > 0)) return fail(-2, "bad dimensions nx=%d nu=%d N=%d dt=%g", p->nx, p->nu, p->horizon, p->dt);
  if (!p->Q || !p->R || !p->Qf || !p->x_ref) return fail(-2, "objective matrices (Q, R, Qf, x_ref) must be set before solving");
  // (LogDDP and MSIPDDP, round 4: resident for the built-in plants -- kernels_logddp.hpp, kernels_msipddp.hpp)
  if (p->solver != CDDP_HIP_SOLVER_CLDDP && p->solver != CDDP_HIP_SOLVER_IPDDP && p->solver != CDDP_HIP_SOLVER_LOGDDP && p->solver != CDDP_HIP_SOLVER_MSIPDDP)
    return fail(-2, "UnknownSolver - No solver registered for id %d", p->solver);
  if (p->solver == CDDP_HIP_SOLVER_MSIPDDP && p->n_constraints > 0 && !(p->nu == 1 || p->nx == p->nu))
    return fail(-3, "MSIPDDP with path constraints is only defined for nu = 1 or nx = nu: the reference adds an (nx x nu) product to its (nu x nx) block Q_ux (msipddp_solver.cpp:1398)");
  if (p->solver == CDDP_HIP_SOLVER_LOGDDP && !(p->options.logddp_relaxed_delta > 0.0))
    return fail(-2, "Relaxation delta must be positive.");   // barrier.hpp:49-51
  // the device-resident retry loops (cddp_solver_base.cpp:93-111) terminate because the regularisation grows: a factor <= 1
  // is an endless loop on the reference's host and would be a wedged queue here
  if (!(p->options.reg_update_factor > 1.0) || !(p->options.reg_max_value > 0.0))
    return fail(-2, "regularization.update_factor must be > 1 and max_value > 0 (got %g, %g)", p->options.reg_update_factor, p->options.reg_max_value);
  if (!p->options.use_ilqr && !model_has_hessians(p->model)) return fail_no_hessians(p->model);
  P.solver = p->solver; P.model = p->model; P.integrator = p->integrator;
  P.nx = p->nx; P.nu = p->nu; P.N = p->horizon; P.dt = p->dt; P.opt = p->options;
  P.ls_rule = p->options.enable_parallel ? CDDP_HIP_LS_BEST_MERIT : CDDP_HIP_LS_FIRST_SUCCESS;
  {
    std::string err;
    if (cddp_host_model_params(p->model, p->nx, p->nu, p->model_params, P.mp, err)) return fail(-2, "%s", err.c_str());
  }
  if (p->model == CDDP_HIP_MODEL_CAR) P.mp[1] = p->dt;   // the car is a discrete plant: its step uses the timestep (car.cpp:24-60)
  if (p->model == CDDP_HIP_MODEL_FORKLIFT) P.mp[3] = p->dt;   // likewise (forklift.cpp:17-48)
  if (p->model == CDDP_HIP_MODEL_LTI) {
    if (!p->lti_A || !p->lti_B) return fail(-2, "LTI model needs lti_A and lti_B");
    if (p->nx * p->nx + p->nx * p->nu + 1 > 32) return fail(-3, "LTI dims too large for the device parameter block");
    for (int i = 0; i < p->nx * p->nx; ++i) P.mp[i] = p->lti_A[i];
    for (int i = 0; i < p->nx * p->nu; ++i) P.mp[p->nx * p->nx + i] = p->lti_B[i];
    P.mp[p->nx * p->nx + p->nx * p->nu] = p->dt;
  }
  int top = 0;
  {
    std::vector<double> q((size_t)p->nx * p->nx), r((size_t)p->nu * p->nu);
    for (size_t i = 0; i < q.size(); ++i) q[i] = p->Q[i] * p->dt;   // objective.cpp:38-39
    for (size_t i = 0; i < r.size(); ++i) r[i] = p->R[i] * p->dt;
    P.off_Qdt = pool_put(P, top, q.data(), (int)q.size());
    P.off_Rdt = pool_put(P, top, r.data(), (int)r.size());
    P.off_Qf = pool_put(P, top, p->Qf, p->nx * p->nx);
    P.off_xref = pool_put(P, top, p->x_ref, p->nx);
    if (P.off_Qdt < 0 || P.off_Rdt < 0 || P.off_Qf < 0 || P.off_xref < 0) return fail(-3, "constant pool overflow");
  }
  P.has_xref_traj = p->x_ref_traj ? 1 : 0;
  if (p->n_constraints > kMaxCons) return fail(-3, "too many path constraints (%d > %d)", p->n_constraints, kMaxCons);
  std::vector<int> order(p->n_constraints);
  for (int i = 0; i < p->n_constraints; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::strcmp(p->constraints[a].name, p->constraints[b].name) < 0; });
  int off = 0;
  P.clddp_box = -1;
  for (int k = 0; k < p->n_constraints; ++k) {
    const cddp_hip_constraint &c = p->constraints[order[k]];
    ConDev &cd = P.cons[k];
    cd.kind = c.kind; cd.dim = c.dim; cd.scale = c.scale; cd.radius = c.radius; cd.offset = off;
    cd.off_lower = cd.off_upper = cd.off_center = cd.off_A = cd.off_b = -1;
    switch (c.kind) {
      case CDDP_HIP_CON_CONTROL_BOX:
      case CDDP_HIP_CON_STATE_BOX:
        if (!c.lower || !c.upper) return fail(-2, "Cannot add null constraint.");
        if (c.dim != (c.kind == CDDP_HIP_CON_CONTROL_BOX ? p->nu : p->nx)) return fail(-2, "box constraint '%s' dimension mismatch", c.name);
        cd.dual_dim = 2 * c.dim;
        cd.off_lower = pool_put(P, top, c.lower, c.dim); cd.off_upper = pool_put(P, top, c.upper, c.dim);
        if (c.kind == CDDP_HIP_CON_CONTROL_BOX && std::strcmp(c.name, "ControlConstraint") == 0) P.clddp_box = k;  // clddp_solver.cpp:85-86
        break;
      case CDDP_HIP_CON_BALL:
        if (!c.center) return fail(-2, "Cannot add null constraint.");
        cd.dual_dim = 1; cd.off_center = pool_put(P, top, c.center, c.dim); break;
      case CDDP_HIP_CON_LINEAR:
        if (!c.A || !c.b) return fail(-2, "Cannot add null constraint.");
        cd.dual_dim = c.dim; cd.off_A = pool_put(P, top, c.A, c.dim * p->nx); cd.off_b = pool_put(P, top, c.b, c.dim); break;
      case CDDP_HIP_CON_SOC: {   // constraint.hpp:626-668: state dimension >= 3, the opening direction stored as a unit vector
        if (!c.center || !c.lower) return fail(-2, "Cannot add null constraint.");
        if (p->nx < 3 || c.dim != 3) return fail(-2, "SecondOrderConeConstraint: State dimension must be at least 3.");
        if (!(c.scale > 0.0)) return fail(-2, "SecondOrderConeConstraint: Regularization epsilon must be positive.");
        const double n2 = c.lower[0] * c.lower[0] + c.lower[1] * c.lower[1] + c.lower[2] * c.lower[2];
        if (n2 == 0.0) return fail(-2, "SecondOrderConeConstraint: Opening direction cannot be zero vector.");
        if (std::fabs(std::sqrt(n2) - 1.0) > 1e-6) return fail(-2, "SecondOrderConeConstraint: pass the opening direction normalised (the reference's constructor normalises it)");
        cd.dual_dim = 1; cd.off_center = pool_put(P, top, c.center, 3); cd.off_lower = pool_put(P, top, c.lower, 3); break;
      }
      case CDDP_HIP_CON_THRUST:
      case CDDP_HIP_CON_MAX_THRUST: {   // constraint.hpp:802-838, 929-953
        if (c.dim != p->nu) return fail(-2, "thrust-magnitude constraint '%s' dimension mismatch", c.name);
        if (!(c.scale > 0.0)) return fail(-2, "ThrustMagnitudeConstraint: epsilon must be positive.");
        const double mn = (c.kind == CDDP_HIP_CON_THRUST && c.lower) ? c.lower[0] : 0.0;
        if (c.kind == CDDP_HIP_CON_THRUST && !c.lower) return fail(-2, "Cannot add null constraint.");
        if (mn < 0.0) return fail(-2, "ThrustMagnitudeConstraint: min_thrust_norm must be non-negative.");
        if (c.radius < mn) return fail(-2, "ThrustMagnitudeConstraint: max_thrust_norm must be greater than or equal to min_thrust_norm.");
        cd.dual_dim = c.kind == CDDP_HIP_CON_THRUST ? 2 : 1; cd.off_lower = pool_put(P, top, &mn, 1); break;
      }
      default: return fail(-2, "unknown constraint kind %d", c.kind);
    }
    if (top > kPool || (cd.off_lower < 0 && cd.off_center < 0 && cd.off_A < 0)) return fail(-3, "constant pool overflow");
    off += cd.dual_dim;
  }
  P.n_cons = p->n_constraints; P.m = off;
  // terminal constraints, in std::map (name) order; inequality rows and equality rows are stacked separately
  if (p->n_terminal > kMaxTerms) return fail(-3, "too many terminal constraints (%d > %d)", p->n_terminal, kMaxTerms);
  if (p->n_terminal > 0 && p->solver != CDDP_HIP_SOLVER_IPDDP) { /* CLDDP ignores the terminal set, as the reference does */ }
  {
    std::vector<int> tord(p->n_terminal);
    for (int i = 0; i < p->n_terminal; ++i) tord[i] = i;
    std::stable_sort(tord.begin(), tord.end(), [&](int a, int b) { return std::strcmp(p->terminal[a].name, p->terminal[b].name) < 0; });
    int offI = 0, offE = 0;
    for (int k = 0; k < p->n_terminal && p->solver == CDDP_HIP_SOLVER_IPDDP; ++k) {
      const cddp_hip_terminal_constraint &c = p->terminal[tord[k]];
      TermDev &td = P.terms[k];
      td.kind = c.kind; td.dim = c.dim; td.off_target = td.off_A = td.off_b = -1;
      if (c.kind == CDDP_HIP_TERM_EQUALITY) {
        if (!c.target) return fail(-2, "Cannot add null constraint.");
        if (c.dim > p->nx) return fail(-2, "TerminalEqualityConstraint: final_state dimension mismatch.");
        td.offset = offE; offE += c.dim; td.off_target = pool_put(P, top, c.target, c.dim);
        if (td.off_target < 0) return fail(-3, "constant pool overflow");
      } else if (c.kind == CDDP_HIP_TERM_INEQUALITY) {
        if (!c.A || !c.b) return fail(-2, "Cannot add null constraint.");
        td.offset = offI; offI += c.dim; td.off_A = pool_put(P, top, c.A, c.dim * p->nx); td.off_b = pool_put(P, top, c.b, c.dim);
        if (td.off_A < 0 || td.off_b < 0) return fail(-3, "constant pool overflow");
      } else {
        return fail(-2, "IPDDP: terminal constraint '%s' has unsupported type. Supported terminal constraints are "
                        "TerminalEqualityConstraint and TerminalInequalityConstraint.", c.name);   // ipddp_solver.cpp:58-67
      }
      P.n_term = k + 1;
    }
    P.mT = offI; P.pT = offE;
    if (P.mT > 8 || P.pT > 16) return fail(-3, "terminal constraint dimension too large (ineq %d > 8 or eq %d > 16)", P.mT, P.pT);
  }
  P.n_alphas = build_ladder(p->solver, &p->options, P.alphas, CDDP_HIP_MAX_ALPHAS);
  if (P.n_alphas <= 0) return fail(-2, "empty line-search ladder");
  return 0;
}

int restore_initial(Inner *h) {
  if (!h->have_initial) return fail(-1, "cddp_hip_set_initial must be called before initialize/solve");
  HIPCHK(hipMemcpyAsync(h->d.X, h->d_Xinit, h->d.planeX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d.U, h->d_Uinit, h->d.planeU * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

int free_all(Inner *h) {
  for (void *q : h->allocs) hipFree(q);
  h->allocs.clear();
  return 0;
}

}  // namespace

extern "C" {

void cddp_hip_default_options(cddp_hip_options *o) {
  std::memset(o, 0, sizeof(*o));
  o->tolerance = 1e-5; o->acceptable_tolerance = 1e-6; o->max_iterations = 1; o->use_ilqr = 1;
  o->termination_scaling_max_factor = 100.0;
  o->ls_max_iterations = 11; o->ls_initial_step_size = 1.0; o->ls_min_step_size = 1e-8; o->ls_step_reduction_factor = 0.5;
  o->reg_initial_value = 1e-6; o->reg_update_factor = 10.0; o->reg_max_value = 1e7; o->reg_min_value = 1e-10;
  o->boxqp_max_iterations = 100; o->boxqp_min_gradient_norm = 1e-8; o->boxqp_min_relative_improvement = 1e-8;
  o->boxqp_step_decrease_factor = 0.6; o->boxqp_min_step_size = 1e-22; o->boxqp_armijo_constant = 0.1;
  o->filter_merit_acceptance_threshold = 1e-6; o->filter_violation_acceptance_threshold = 1e-6;
  o->filter_max_violation_threshold = 1e4; o->filter_min_violation_for_armijo_check = 1e-7; o->filter_armijo_constant = 1e-4;
  o->ipddp_dual_var_init_scale = 0.1; o->ipddp_slack_var_init_scale = 1e-2; o->ipddp_barrier_tol_mult = 0.1;
  o->ipddp_barrier_update_dual_weight = 0.01; o->ipddp_mu_kappa_epsilon = 10.0; o->ipddp_max_filter_size = 5;
  o->ipddp_theta_0_floor = 1.0; o->ipddp_warmstart_s_min = 1e-4; o->ipddp_warmstart_y_min = 1e-4;
  o->ipddp_warmstart_interior_factor = 1.1; o->ipddp_jacobian_regularization_value = 1e-8;
  o->ipddp_jacobian_regularization_exponent = 0.25;
  o->barrier_mu_initial = 1.0; o->barrier_mu_min_value = 1e-10; o->barrier_mu_update_factor = 0.5;
  o->barrier_mu_update_power = 1.2; o->barrier_min_fraction_to_boundary = 0.99; o->barrier_strategy = CDDP_HIP_BARRIER_ADAPTIVE;
  o->max_cpu_time = 0.0;
  o->logddp_mu_initial = 1.0; o->logddp_mu_min_value = 1e-10; o->logddp_mu_update_factor = 0.5; o->logddp_relaxed_delta = 1e-10;
  o->msipddp_costate_var_init_scale = 1e-6; o->msipddp_segment_length = 5; o->msipddp_rollout_type = 0; o->msipddp_use_controlled_rollout = 0; o->_pad4 = 0;
}

int cddp_hip_abi_version(void) { return CDDP_HIP_ABI_VERSION; }

int cddp_hip_model_eval(int model, int integrator, double dt, const double *model_params, int nx, int nu, const double *x, const double *u,
                        double *x_next, double *fx, double *fu, double *fxx, double *fuu, double *fux) {
  if (!model_params || !x || !u) return fail(-2, "cddp_hip_model_eval: null argument");
  std::string err;
  double mp[CDDP_HIP_MAX_MODEL_PARAMS];
  if (cddp_host_model_params(model, nx, nu, model_params, mp, err)) return fail(-2, "cddp_hip_model_eval: %s", err.c_str());
  const int rc = cddp_host_model_eval(model, integrator, dt, mp, nx, nu, x, u, x_next, fx, fu, fxx, fuu, fux, err);
  return rc == 0 ? 0 : fail(rc, "cddp_hip_model_eval: %s", err.c_str());
}
const char *cddp_hip_last_error(void) { return g_err.c_str(); }

int cddp_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *cddp_hip_status_string(int status) {
  switch (status) {
    case CDDP_HIP_STATUS_RUNNING: return "Running";
    case CDDP_HIP_STATUS_OPTIMAL: return "OptimalSolutionFound";
    case CDDP_HIP_STATUS_ACCEPTABLE: return "AcceptableSolutionFound";
    case CDDP_HIP_STATUS_MAX_ITERATIONS: return "MaxIterationsReached";
    case CDDP_HIP_STATUS_REG_LIMIT: return "RegularizationLimitReached_NotConverged";
    case CDDP_HIP_STATUS_MAX_CPU_TIME: return "MaxCpuTimeReached";
    case CDDP_HIP_STATUS_REG_LIMIT_CONVERGED: return "RegularizationLimitReached_Converged";
  }
  return "Unknown";
}

// detail::buildLineSearchAlphas (reference cddp_context_utils.cpp:37-57)
int cddp_hip_build_alphas(const cddp_hip_options *opt, double *alphas, int cap) {
  int n = 0;
  double cur = opt->ls_initial_step_size;
  for (int i = 0; i < opt->ls_max_iterations; ++i) {
    if (alphas && n < cap) alphas[n] = cur;
    ++n;
    cur *= opt->ls_step_reduction_factor;
    if (cur < opt->ls_min_step_size && i < opt->ls_max_iterations - 1) {
      if (alphas && n < cap) alphas[n] = opt->ls_min_step_size;
      ++n;
      break;
    }
  }
  if (n == 0) { if (alphas && cap > 0) alphas[0] = opt->ls_initial_step_size; n = 1; }
  if (!alphas) return n;   // the ladder's own length, whatever a buffer could hold
  return n > cap ? cap : n;
}

// What the fixed capacities of a handle cannot hold is refused, not truncated (cddp_hip_create and cddp_hip_set_options):
//  * the ladder lives in ProblemDev::alphas[CDDP_HIP_MAX_ALPHAS]; the reference runs every step size buildLineSearchAlphas makes;
//  * the IPDDP filter column holds kFilterCap points, and between an accept and the prune that follows it the reference's filter holds
//    max_filter_size + 1 (ipddp_solver.cpp: acceptFilterEntry, then pruneFilterToBestPoints above max_filter_size).  MSIPDDP sizes its
//    filter by max_iterations and never reads the option.
static int check_capacities(int solver, const cddp_hip_options *opt) {
  const int n_full = build_ladder(solver, opt, nullptr, 0);
  if (n_full > CDDP_HIP_MAX_ALPHAS)
    return fail(-3, "line_search: ls_max_iterations = %d gives a ladder of %d step sizes, more than CDDP_HIP_MAX_ALPHAS = %d", opt->ls_max_iterations,
                n_full, CDDP_HIP_MAX_ALPHAS);
  if (solver == CDDP_HIP_SOLVER_IPDDP && opt->ipddp_max_filter_size > kFilterCap - 1)
    return fail(-3, "ipddp_max_filter_size = %d: the filter holds max_filter_size + 1 points before it is pruned and has %d slots, so at most %d",
                opt->ipddp_max_filter_size, kFilterCap, kFilterCap - 1);
  return 0;
}


// one "X=lo-hi,..." spec
static bool parse_cu_spec(const std::string &t, CuSpec *o) {
  size_t i = 0;
  while (i < t.size()) {
    size_t j = t.find(',', i); if (j == std::string::npos) j = t.size();
    const std::string f = t.substr(i, j - i);
    i = j + 1;
    if (f.empty()) continue;
    int lo = 0, hi = 0; char c = 0;
    unsigned xm = 0;
    if (f.size() >= 4 && f[1] == '=' && f[2] == 'x') {
      c = f[0];
      for (size_t q = 3; q < f.size(); ++q) { if (f[q] < '0' || f[q] > '7') return false; xm |= 1u << (f[q] - '0'); }
      lo = 0; hi = 1024;
    } else if (std::sscanf(f.c_str(), " %c=%d-%d", &c, &lo, &hi) != 3 || lo < 0 || hi <= lo || hi > 1024) return false;
    const int k = (c == 'C') ? 0 : (c == 'F') ? 1 : (c == 'W') ? 2 : -1;
    if (k < 0) return false;
    o->lo[k] = lo; o->hi[k] = hi; o->xcd[k] = xm;
  }
  return true;
}
// the spec of group `gi` from CDDP_HIP_CUMASK (false: no partition requested / malformed -> plain streams)
static bool cu_spec_for_group(const Knobs &knob, int gi, CuSpec *o) {
  if (knob.cumask.empty()) return false;
  std::vector<std::string> parts;
  { const std::string &t = knob.cumask; size_t i = 0; for (;;) { size_t j = t.find('|', i); parts.push_back(t.substr(i, j == std::string::npos ? j : j - i)); if (j == std::string::npos) break; i = j + 1; } }
  const std::string &t = parts[std::min((size_t)gi, parts.size() - 1)];
  CuSpec sp;
  if (!parse_cu_spec(t, &sp)) { std::fprintf(stderr, "[cddp_hip] CDDP_HIP_CUMASK: cannot parse '%s' -- ignored\n", t.c_str()); return false; }
  *o = sp;
  return true;
}
static int device_cu_count(int device) {
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
  return ncu;
}
// A mask that selects no CU of THIS device (a spec written for 256 CUs on a 128-CU partition), or a runtime that refuses the masked
// stream, must not fail the handle: the group then runs on a plain stream (same results -- the partition is placement only).
static hipError_t make_stream(hipStream_t *s, int device, int lo, int hi, unsigned xcd = 0) {
  if (lo < 0) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  const int ncu = device_cu_count(device);
  const int words = (ncu + 31) / 32;
  std::vector<uint32_t> mask((size_t)words, 0u);
  int bits = 0;
  for (int b = lo; b < hi && b < ncu; ++b) if (!xcd || ((xcd >> (b % 8)) & 1u)) { mask[(size_t)b >> 5] |= 1u << (b & 31); ++bits; }
  if (bits == 0) {
    std::fprintf(stderr, "[cddp_hip] CU mask [%d, %d) selects none of the device's %d CUs: plain stream instead\n", lo, hi, ncu);
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  }
  const hipError_t e = hipExtStreamCreateWithCUMask(s, (uint32_t)words, mask.data());
  if (e == hipSuccess) return e;
  (void)hipGetLastError();
  std::fprintf(stderr, "[cddp_hip] hipExtStreamCreateWithCUMask([%d, %d) of %d CUs): %s -- plain stream instead\n", lo, hi, ncu, hipGetErrorString(e));
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
static int in_destroy(Inner *h);

// the kernel route of a group (launch.hpp::Route): fixed by the switches read at create, the solver, the buffers and use_ilqr
static void resolve_route(Inner *h) { h->route = h->ks->route(h->d, h->P.solver, *h->knob); h->d.t4 = h->route.t4; }

// Shadow costate: the layouts whose K4b can leave the iteration's chain -- IPDDP with path rows on the role-split cooperative sweep, no
// terminal set, Gauss-Newton, first-success rule (nothing reads Lambda during such a solve).  Not with the costate test hook (it needs
// flag 2 on the chain) and not with captured windows (the value stack's parity would have to enter the graph key).
static bool shadow_layout(const Inner *h) {
  return h->P.solver == CDDP_HIP_SOLVER_IPDDP && h->P.m > 0 && h->P.n_term == 0 && !h->d.ddp && h->route.sweep == Route::kCoop && h->route.roles_nh > 0 &&
         h->ks->shadow_extra(h->d, h->route) > 0;
}
// ... and the solves that may take it: the solve must be restartable from the device-resident initial trajectory (cold, or the "provided
// trajectory" warm start; an "existing solver state" warm solve consumes state the solve itself overwrites, so it keeps K4b on the chain).
// COSTATE unset: only where the sweep launch puts at most ONE workgroup on every CU of the group's share of the chip (conc groups in flight
// share it).  The extra blocks are workgroups of the sweep kernel and carry its static LDS (53.6 - 57.2 KB), of which a CU holds two: beside
// one sweep workgroup per CU they run under the sweep (C2: 128 sweep workgroups on 128 CUs, measured faster, profiles/r09_costate_shadow.md);
// where the sweep already fills both places (C3 at its bench batch) they could only start as sweep workgroups finish, i.e. behind the sweep
// -- that shape stays on the chain unless CDDP_HIP_COSTATE=shadow asks for it.
static bool shadow_eligible(const Inner *h, int conc) {
  if (!h->shadow_bufs || !shadow_layout(h)) return false;
  if (h->knob->costate == Knobs::kCostateAuto) {
    const int own = h->ks->shadow_extra(h->d, h->route) > 0 ? h->ks->sweep_blocks(h->d) : 0;
    if (own <= 0 || own > device_cu_count(h->device) / std::max(1, conc)) return false;
  }
  if (h->knob->costate == Knobs::kCostateSync || h->knob->fail_costate != 0 || h->knob->graph) return false;
  if (h->P.ls_rule != CDDP_HIP_LS_FIRST_SUCCESS) return false;
  if (h->P.opt.warm_start && h->has_state) return false;
  return true;
}

static int in_create(const cddp_hip_problem *problem, int batch, int device, const Knobs &knob, const CuSpec *cu, Inner **out) {
  if (!problem || !out) return fail(-1, "null argument");
  if (batch <= 0) return fail(-1, "batch must be positive");
  int ndev = cddp_hip_device_count();
  if (ndev <= 0) return fail(-20, "no HIP device available: the cddp_hip solver core has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(-1, "device %d out of range (%d devices)", device, ndev);
  Inner *h = new Inner();
  h->knob = &knob;
  int rc = flatten(problem, h->P);
  if (rc) { delete h; return rc; }
  for (const KernelSet &k : registry()) if (k.matches(h->P)) { h->ks = &k; break; }
  if (!h->ks) {
    const int m = h->P.m, nc = h->P.n_cons;
    delete h;
    return fail(-4, "no kernel instantiation for model=%d nx=%d nu=%d with this constraint layout (m=%d, %d constraints)",
                problem->model, problem->nx, problem->nu, m, nc);
  }
  if (h->P.solver == CDDP_HIP_SOLVER_LOGDDP && !h->ks->has_logddp) {
    delete h;
    return fail(-4, "LogDDP has no resident kernels for this layout (model=%d, nx=%d): use cddp_hip_plugin_solve", problem->model, problem->nx);
  }
  if (h->P.solver == CDDP_HIP_SOLVER_MSIPDDP && !h->ks->has_msipddp) {
    delete h;
    return fail(-4, "MSIPDDP has no resident kernels for this layout (model=%d, nx=%d; terminal sets and nx > 8 are served by cddp_hip_plugin_solve)", problem->model, problem->nx);
  }
  if (h->P.solver == CDDP_HIP_SOLVER_MSIPDDP && !h->P.opt.use_ilqr) {
    bool curved = false;
    for (int c = 0; c < h->P.n_cons; ++c) { const int kd = h->P.cons[c].kind; if (kd != CDDP_HIP_CON_CONTROL_BOX && kd != CDDP_HIP_CON_STATE_BOX && kd != CDDP_HIP_CON_LINEAR) curved = true; }
    if (curved || !h->ks->logddp_ddp) {
      delete h;
      return fail(-3, "MSIPDDP with use_ilqr=false is resident for plants with explicit Hessian tensors and constraint rows without curvature: use cddp_hip_plugin_solve");
    }
  }
  if (h->P.solver == CDDP_HIP_SOLVER_LOGDDP && !h->P.opt.use_ilqr && !h->ks->logddp_ddp) {
    delete h;
    return fail(-3, "LogDDP with use_ilqr=false needs the plant's explicit Hessian tensors, which model id %d keeps only in the blocked dual form: use cddp_hip_plugin_solve", problem->model);
  }
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) { delete h; return fail(-10, "hipSetDevice: %s", hipGetErrorString(e)); }
  e = make_stream(&h->stream, device, cu ? cu->lo[0] : -1, cu ? cu->hi[0] : -1, cu ? cu->xcd[0] : 0);
  if (e != hipSuccess) { delete h; return fail(-10, "hipStreamCreate: %s", hipGetErrorString(e)); }
  h->own_stream = true;
  if (cu && (cu->lo[1] >= 0 || cu->lo[2] >= 0)) {
    if (cu->lo[1] >= 0) e = make_stream(&h->cu.fwd, device, cu->lo[1], cu->hi[1], cu->xcd[1]);
    if (e == hipSuccess && cu->lo[2] >= 0) e = make_stream(&h->cu.sweep, device, cu->lo[2], cu->hi[2], cu->xcd[2]);
    for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&h->cu.ev[k], hipEventDisableTiming);
    if (e != hipSuccess) { const int rc_ = fail(-10, "CU-masked stream: %s", hipGetErrorString(e)); in_destroy(h); return rc_; }   // (streams / events created so far go with it)
    h->cu.hop = SweepHop{h->cu.sweep, h->cu.ev[4], h->cu.ev[5]};
  }

  const ProblemDev &P = h->P;
  DevBuf &d = h->d;
  std::memset(&d, 0, sizeof(d));
  const int B = batch, Bp = (batch + 63) / 64 * 64, N = P.N, nx = P.nx, nu = P.nu, m = P.m;
  d.B = B; d.Bp = Bp; d.NB = Bp / 64; d.N = N; d.n_alphas = P.n_alphas; d.n_slots = P.n_alphas + 1;
  d.ladder_sorted = ladder_strictly_decreasing(P.alphas, P.n_alphas);
  d.ddp = P.opt.use_ilqr ? 0 : 1;
  d.fail_costate_mask = knob.fail_costate;   // test hook
  d.xcd_map = knob.xcd_map ? 1 : 0;
  d.hist_batch = P.opt.return_iteration_info ? std::min(B, 64) : 0;
  d.hist_cap = std::max(P.opt.max_iterations, 0) + 1;
  d.planeX = (size_t)(N + 1) * nx * Bp; d.planeU = (size_t)N * nu * Bp; d.planeM = (size_t)N * (m > 0 ? m : 0) * Bp;
  const bool ip = (P.solver == CDDP_HIP_SOLVER_IPDDP);
  d.lg = (P.solver == CDDP_HIP_SOLVER_LOGDDP) ? 1 : 0;
  const bool ms = (P.solver == CDDP_HIP_SOLVER_MSIPDDP);
  d.ms = ms ? 1 : 0;
  d.filt_cap = ms ? std::max(P.opt.max_iterations, 0) + 2 : kFilterCap;   // (a negative max_iterations is a legal no-op solve, SolveRun::begin)
#define DA(ptr, n) do { int rc_ = dalloc(h, &(ptr), (size_t)(n)); if (rc_) { in_destroy(h); return rc_; } } while (0)
  DA(d.X, d.planeX * d.n_slots); DA(d.U, d.planeU * d.n_slots);
  if (ip) { DA(d.S, d.planeM * d.n_slots); DA(d.Y, d.planeM * d.n_slots); DA(d.G, d.planeM * d.n_slots); DA(d.Lam, d.planeX * d.n_slots); }
  if (ms) {   // kernels_msipddp.hpp: slack / dual / constraint / costate / dynamics-value planes per slot, costate gains, factor cache
    if (m > 0) { DA(d.S, d.planeM * d.n_slots); DA(d.Y, d.planeM * d.n_slots); DA(d.G, d.planeM * d.n_slots);
                 DA(d.ks, (size_t)N * m * Bp); DA(d.ky, (size_t)N * m * Bp); DA(d.Ks, (size_t)N * m * nx * Bp); DA(d.Ky, (size_t)N * m * nx * Bp); }
    DA(d.Lam, d.planeX * d.n_slots); DA(d.F, d.planeX * d.n_slots);
    DA(d.kl, (size_t)N * nx * Bp);
    if (m == 0) DA(d.fac, (size_t)N * (nu * nu + nu + 1) * Bp);
    if (m > 0) { DA(d.ms_res, (size_t)3 * Bp); DA(d.ev, (size_t)d.n_slots * N * P.n_cons * Bp); }   // parked log-barrier sums per slot (k_update_msipddp replays them)
    if (m > 0 && h->ks->ms_cst_size > 0) DA(d.cst, (size_t)N * h->ks->ms_cst_size * Bp);   // V-independent terms of the split sweep (k_ms_condense)
  }
  DA(d.A, (size_t)N * nx * nx * Bp); DA(d.Bm, (size_t)N * nx * nu * Bp);
  DA(d.K, (size_t)N * nu * nx * Bp); DA(d.k, (size_t)N * nu * Bp);
  if (ip && nx > 8) DA(d.Kt, (size_t)N * (nu * nx + nu) * Bp);   // G = 16 sweeps (launch.hpp::Launcher::route, Route::t4)
  DA(d.Vx, (size_t)(N + 1) * nx * Bp); DA(d.Vxx, (size_t)(N + 1) * nx * nx * Bp);
  if (ip && h->ks->cst_size > 0) { DA(d.cst, (size_t)N * h->ks->cst_size * Bp); DA(d.dX, (size_t)N * nx * Bp); DA(d.ys, (size_t)N * (m > 0 ? m : 1) * Bp); }
  if (ip && m > 0) { DA(d.ks, (size_t)N * m * Bp); DA(d.ky, (size_t)N * m * Bp); DA(d.Ks, (size_t)N * m * nx * Bp); DA(d.Ky, (size_t)N * m * nx * Bp); }
  double **scal[] = {&d.cost, &d.merit, &d.inf_pr, &d.inf_du, &d.inf_comp, &d.step_norm, &d.alpha_pr, &d.alpha_du, &d.reg, &d.mu,
                     &d.dV0, &d.dV1, &d.phi, &d.theta, &d.filter_theta, &d.apr_max, &d.adu_max};
  for (double **sp : scal) DA(*sp, Bp);
  DA(d.filt, (size_t)2 * d.filt_cap * Bp);
  int **iscal[] = {&d.filt_n, &d.iter, &d.status, &d.phase, &d.cur, &d.n_bwd, &d.n_fwd, &d.bwd_ok};
  for (int **sp : iscal) DA(*sp, Bp);
  double **tr[] = {&d.t_cost, &d.t_merit, &d.t_theta, &d.t_inf_pr, &d.t_inf_comp, &d.t_apr, &d.t_adu, &d.t_ysmin, &d.t_ysmax};
  for (double **sp : tr) DA(*sp, (size_t)d.n_alphas * Bp);
  DA(d.sink, kSinkDoubles);
  DA(d.t_success, (size_t)d.n_alphas * Bp);
  DA(d.t_steps, (size_t)d.n_alphas * Bp); DA(d.n_fwd_steps, Bp); DA(d.cand, Bp);
  if (ip && P.n_cons > 0) DA(d.ev, (size_t)d.n_alphas * N * 2 * P.n_cons * Bp);
  if (d.lg && P.n_cons > 0) DA(d.ev, (size_t)d.n_slots * N * P.n_cons * Bp);   // parked barrier sums per trial slot (kernels_logddp.hpp)
  DA(d.hist, (size_t)std::max(1, d.hist_batch) * d.hist_cap * kHistCols);
  DA(d.hist_n, std::max(1, d.hist_batch));
  if (ip && P.n_term > 0) {
    DA(d.ST, (size_t)8 * Bp); DA(d.YT, (size_t)8 * Bp); DA(d.GT, (size_t)8 * Bp); DA(d.dST, (size_t)8 * Bp); DA(d.dYT, (size_t)8 * Bp);
    DA(d.LamT, (size_t)16 * Bp); DA(d.dLamT, (size_t)16 * Bp);
    DA(d.STt, (size_t)d.n_alphas * 8 * Bp); DA(d.YTt, (size_t)d.n_alphas * 8 * Bp); DA(d.GTt, (size_t)d.n_alphas * 8 * Bp);
    DA(d.LamTt, (size_t)d.n_alphas * 16 * Bp);
    if (P.pT > 0) {
      // cooperative reduced-LQR sweep (kernels_te.hpp): one lane per gradient variant, variant stride 16
      const bool te_coop = h->ks->te_rec_size > 0 && P.mT == 0 && P.pT + 1 <= h->ks->te_group && P.pT <= P.nx;   // TeCfg::PMAX
      const size_t nv = te_coop ? 16 : (size_t)(P.pT + 1);
      DA(d.te_k, nv * N * nu * Bp); DA(d.te_p, nv * (N + 1) * nx * Bp);
      if (te_coop) {
        DA(d.te_cst, (size_t)N * h->ks->te_rec_size * Bp); DA(d.te_cnt, Bp);
        if (!d.dX) DA(d.dX, (size_t)N * nx * Bp);
        if (!d.ys) DA(d.ys, (size_t)N * (m > 0 ? m : 1) * Bp);
      }
    }
  }
  DA(d.n_active, 1);
  DA(d.win_hist, CDDP_HIP_MAX_ALPHAS + 1);
  DA(h->d_launched, ls_words(Bp / 64));   // + the line-search stage words (dev_types.hpp, kLsGran)
  DA(h->dP, 1);
  DA(h->d_Xinit, d.planeX); DA(h->d_Uinit, d.planeU);
  if (problem->x_ref_traj) {
    DA(h->d_xref_traj, (size_t)(N + 1) * nx);
    hipMemcpyAsync(h->d_xref_traj, problem->x_ref_traj, sizeof(double) * (N + 1) * nx, hipMemcpyHostToDevice, h->stream);
    d.xref_traj = h->d_xref_traj;
  }
#undef DA
  hipMemcpyAsync(h->dP, &h->P, sizeof(ProblemDev), hipMemcpyHostToDevice, h->stream);
  d.P = h->dP;
  d.launched = h->d_launched;
  resolve_route(h);
  if (shadow_layout(h) && knob.costate != Knobs::kCostateSync && !knob.fail_costate && !knob.graph) {
#define DA(ptr, n) do { int rc_ = dalloc(h, &(ptr), (size_t)(n)); if (rc_) { in_destroy(h); return rc_; } } while (0)
    DA(d.Vx2, (size_t)(N + 1) * nx * Bp); DA(d.Vxx2, (size_t)(N + 1) * nx * nx * Bp);
    DA(d.cs_stampv, Bp); DA(d.cs_old, Bp); DA(d.cs_new, Bp); DA(d.cs_apr, Bp); DA(d.cs_vbuf, Bp); DA(d.cs_bad, 1);
#undef DA
    if (hipHostMalloc((void **)&h->h_bad, sizeof(int)) != hipSuccess) { const int rc_ = fail(-10, "hipHostMalloc failed"); in_destroy(h); return rc_; }
    *h->h_bad = 0;
    h->shadow_bufs = true;
  }
  e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { const int rc_ = fail(-10, "device initialisation failed: %s", hipGetErrorString(e)); in_destroy(h); return rc_; }
  *out = h;
  return 0;
}

static int in_destroy(Inner *h) {
  if (h) { for (auto &kv : h->graphs) hipGraphExecDestroy(kv.second); h->graphs.clear(); }
  if (!h) return 0;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  if (h->cu.fwd) hipStreamSynchronize(h->cu.fwd);
  if (h->cu.sweep) hipStreamSynchronize(h->cu.sweep);
  free_all(h);
  for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
  if (h->ev_begin) { hipEventDestroy(h->ev_begin); hipEventDestroy(h->ev_end); }
  if (h->ev_poll) hipEventDestroy(h->ev_poll);
  if (h->ev_poll2) hipEventDestroy(h->ev_poll2);
  if (h->h_poll) hipHostFree(h->h_poll);
  if (h->h_ls) hipHostFree(h->h_ls);
  if (h->h_bad) hipHostFree(h->h_bad);
  if (h->d_head) hipFree(h->d_head);
  if (h->h_head) hipHostFree(h->h_head);
  if (h->d_xnext) hipFree(h->d_xnext);
  if (h->d_log_u) { hipFree(h->d_log_u); hipFree(h->d_log_x); hipFree(h->d_log_it); hipFree(h->d_log_st); }
  if (h->d_path) hipFree(h->d_path);
  if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
  if (h->cu.fwd) hipStreamDestroy(h->cu.fwd);
  if (h->cu.sweep) hipStreamDestroy(h->cu.sweep);
  for (hipEvent_t e : h->cu.ev) if (e) hipEventDestroy(e);
  delete h;
  return 0;
}

static int in_set_timing_detail(Inner *h, int detail) {
  if (!h) return fail(-1, "null handle");
  if (detail != CDDP_HIP_TIMING_ROLLOUT && detail != CDDP_HIP_TIMING_ALL && detail != CDDP_HIP_TIMING_SWEEP)
    return fail(-2, "unknown timing detail %d", detail);
  h->timing_detail = detail;
  return 0;
}

static int in_set_stream(Inner *h, void *hip_stream) {
  if (!h) return fail(-1, "null handle");
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
  h->stream = (hipStream_t)hip_stream;
  h->own_stream = false;
  return 0;
}

static int in_dual_dim(Inner *h) { return h ? h->P.m : -1; }
static int in_batch(Inner *h) { return h ? h->d.B : -1; }

// host batch-major [b][t][e]  <->  device batch-minor [t][e][b]
// wave-tiled stack index (dev_types.hpp): element e of step t of trajectory b
static inline size_t tix(int t, int E, int e, int b, int Bp) { return ((((size_t)t * (Bp / 64) + (size_t)(b >> 6)) * E + e) * 64) + (size_t)(b & 63); }
static void to_soa(const double *src, double *dst, int B, int Bp, int T, int E) {
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      for (int e = 0; e < E; ++e) dst[tix(t, E, e, b, Bp)] = src[((size_t)b * T + t) * E + e];
}
static void from_soa(const double *src, double *dst, int B, int Bp, int T, int E) {
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      for (int e = 0; e < E; ++e) dst[((size_t)b * T + t) * E + e] = src[tix(t, E, e, b, Bp)];
}

// the same, from the sub-tile-minor layout of the G = 16 sweeps' input stacks (kernels.hpp::GT)
static void from_t4(const double *src, double *dst, int B, int Bp, int T, int E) {
  const size_t NB16 = (size_t)(Bp / 64) * 16;
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      for (int e = 0; e < E; ++e) dst[((size_t)b * T + t) * E + e] = src[((((size_t)t * NB16 + (size_t)(b >> 2)) * (size_t)E + (size_t)e) * 4) + (size_t)(b & 3)];
}

// a new initial trajectory lies in d_Xinit / d_Uinit: the next initialize is cold and starts from it
static void mark_seeded(Inner *q) { q->have_initial = true; q->initialized = false; q->initial_dirty = true; }

static int in_set_initial(Inner *h, const double *x0, const double *U0, const double *X0) {
  if (!h || !x0) return fail(-1, "null argument");
  HIPCHK(hipSetDevice(h->device));
  const DevBuf &d = h->d;
  const int B = d.B, Bp = d.Bp, N = d.N, nx = h->P.nx, nu = h->P.nu;
  std::vector<double> hx((size_t)(N + 1) * nx * Bp, 0.0), hu((size_t)N * nu * Bp, 0.0);
  if (X0) to_soa(X0, hx.data(), B, Bp, N + 1, nx);
  else
    for (int b = 0; b < B; ++b)
      for (int t = 0; t <= N; ++t)
        for (int e = 0; e < nx; ++e) hx[tix(t, nx, e, b, Bp)] = x0[(size_t)b * nx + e];
  for (int b = 0; b < B; ++b)
    for (int e = 0; e < nx; ++e) hx[tix(0, nx, e, b, Bp)] = x0[(size_t)b * nx + e];   // X_[0] = initial_state (cddp_core.cpp:294)
  if (U0) to_soa(U0, hu.data(), B, Bp, N, nu);
  HIPCHK(hipMemcpyAsync(h->d_Xinit, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_Uinit, hu.data(), hu.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  mark_seeded(h);
  return 0;
}

// ISolverAlgorithm::initialize on this handle (the handle IS the solver object).  Cold: the initial trajectory is
// restored and everything re-initialised.  options.warm_start: "provided trajectory" on a fresh handle, "existing
// solver state" afterwards -- the live slack / dual / costate rows are staged into slot 0 (and X, U too unless the
// caller supplied a new trajectory since), see k_init.
static int run_initialize(Inner *h) {
  const bool ip = (h->P.solver == CDDP_HIP_SOLVER_IPDDP) || (h->P.solver == CDDP_HIP_SOLVER_MSIPDDP);   // slack / dual / costate rows staged for a warm re-solve
  int mode = kInitCold;
  if (h->P.opt.warm_start) mode = h->has_state ? kInitWarmExisting : kInitWarmProvided;
  if (mode == kInitWarmExisting) {
    h->ks->stage(h->d, h->initial_dirty ? 0 : 1, ip ? 1 : 0, h->stream);
    if (h->initial_dirty) { int rc = restore_initial(h); if (rc) return rc; }
  } else {
    int rc = restore_initial(h); if (rc) return rc;
  }
  if (h->d.ms) {   // the reference's factor cache belongs to the solver object, not to one solve: invalid only before the handle's first initialize
    DevBuf dd = h->d;
    dd.ms_fresh = h->ms_cache_started ? 0 : 1;
    h->ks->init(dd, mode, h->stream);
    h->ms_cache_started = true;
  } else
  h->ks->init(h->d, mode, h->stream);
  h->has_state = true;
  h->has_plan = true;
  h->initial_dirty = false;
  h->initialized = true;
  return 0;
}

static int in_initialize(Inner *h) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  { int rc = run_initialize(h); if (rc) return rc; }
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- movable goal and per-step reference (cddp_hip_set_reference, cddp_hip_mpc_set_reference_path) --------------------
// The kernels read the goal from dP->pool + off_xref and the per-step reference through DevBuf::xref_traj on every launch, so new CONTENTS
// need nothing but the write; captured windows bake in the DevBuf and are dropped only when xref_traj changes between null and non-null.
// ProblemDev::has_xref_traj (read by no kernel) follows DevBuf::xref_traj in h->P and, through push_has_traj, in dP.
static double *goal_slot(Inner *h) { return h->dP->pool + h->P.off_xref; }   // a device address, formed but not read on the host

// P.pool's goal from the device when the device holds the newer one: before the host reads it or uploads P whole (in_set_options,
// in_set_reference, in_forward -- every place that copies sizeof(ProblemDev) to dP after create)
static int goal_to_host(Inner *h) {
  if (!h->goal_on_device) return 0;
  HIPCHK(hipMemcpyAsync(h->P.pool + h->P.off_xref, goal_slot(h), sizeof(double) * h->P.nx, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->goal_on_device = false;
  return 0;
}

static void drop_graphs(Inner *h) { for (auto &kv : h->graphs) hipGraphExecDestroy(kv.second); h->graphs.clear(); }

static int push_has_traj(Inner *h) {
  HIPCHK(hipMemcpyAsync(&h->dP->has_xref_traj, &h->P.has_xref_traj, sizeof(int), hipMemcpyHostToDevice, h->stream));
  return 0;
}

// the per-step reference buffer: allocated on first use, kept for the handle's life (ref_alloc_traj); attached, it is what the kernels read
static int ref_alloc_traj(Inner *h) {
  if (h->d_xref_traj) return 0;
  return dalloc(h, &h->d_xref_traj, (size_t)(h->d.N + 1) * h->P.nx);
}
static int ref_attach_traj(Inner *h) {
  { int rc = ref_alloc_traj(h); if (rc) return rc; }
  if (!h->d.xref_traj) { h->d.xref_traj = h->d_xref_traj; h->P.has_xref_traj = 1; drop_graphs(h); return push_has_traj(h); }
  return 0;
}

// one group's cddp_hip_set_reference (checked by the caller): copies enqueued on the group's stream; host pointers: complete on return
static int in_set_reference(Inner *h, int flags, const double *x_ref, const double *x_ref_traj) {
  HIPCHK(hipSetDevice(h->device));
  const bool dev = (flags & CDDP_HIP_REF_DEVICE) != 0;
  const int nx = h->P.nx;
  if (x_ref_traj) {
    { int rc = ref_attach_traj(h); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(h->d_xref_traj, x_ref_traj, sizeof(double) * (size_t)(h->d.N + 1) * nx, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  }
  if ((flags & CDDP_HIP_REF_CLEAR_TRAJ) && h->d.xref_traj) {
    h->d.xref_traj = nullptr; h->P.has_xref_traj = 0; drop_graphs(h);
    int rc = push_has_traj(h); if (rc) return rc;
  }
  if (dev) {
    if (x_ref) { HIPCHK(hipMemcpyAsync(goal_slot(h), x_ref, sizeof(double) * nx, hipMemcpyDeviceToDevice, h->stream)); h->goal_on_device = true; }
    return 0;
  }
  if (x_ref) { for (int i = 0; i < nx; ++i) h->P.pool[h->P.off_xref + i] = x_ref[i]; h->goal_on_device = false; }
  else { int rc = goal_to_host(h); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(h->dP, &h->P, sizeof(ProblemDev), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the window of the group's cursor into its per-step reference buffer and goal slot (inst_ref.hip), on the group's stream
static int ref_install_window(Inner *h) {
  const hipError_t e = ref_window_launch(h->d_path, h->path_L, h->P.nx, h->d.N, h->path_cursor, h->path_rps, h->d_xref_traj, goal_slot(h), h->stream);
  if (e != hipSuccess) return fail(-10, "reference window launch failed: %s", hipGetErrorString(e));
  h->goal_on_device = true;
  return 0;
}

// one group's cddp_hip_mpc_set_reference_path (checked by the caller), in two parts so that a failure in any group leaves every group as it
// was.  Stage: everything that allocates -- the per-step reference buffer (kept, not attached) and this group's own copy of the rows.
static int in_stage_path(Inner *h, const cddp_hip_ref_path *c, double **out) {
  HIPCHK(hipSetDevice(h->device));
  { int rc = ref_alloc_traj(h); if (rc) return rc; }
  const bool dev = (c->flags & CDDP_HIP_REF_DEVICE) != 0;
  const size_t bytes = (size_t)c->rows * (size_t)h->P.nx * sizeof(double);
  double *p = nullptr;
  HIPCHK(hipMalloc((void **)&p, bytes));
  const hipError_t e = hipMemcpyAsync(p, c->path, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream);
  if (e != hipSuccess) { hipFree(p); return fail(-10, "cddp_hip_mpc_set_reference_path: copy of the path failed: %s", hipGetErrorString(e)); }
  *out = p;
  return 0;
}
// Commit: the staged rows become the bound path and the window of cursor `start` is installed
static int in_commit_path(Inner *h, const cddp_hip_ref_path *c, double *p) {
  HIPCHK(hipSetDevice(h->device));
  if (h->d_path) { hipStreamSynchronize(h->stream); hipFree(h->d_path); }   // (a window kernel of the old path may still be queued)
  h->d_path = p; h->path_L = c->rows; h->path_cursor = c->start; h->path_rps = c->rows_per_step;
  { int rc = ref_attach_traj(h); if (rc) return rc; }
  { int rc = ref_install_window(h); if (rc) return rc; }
  if (!(c->flags & CDDP_HIP_REF_DEVICE)) HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

static int in_unbind_path(Inner *h) {
  if (!h->d_path) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  hipFree(h->d_path);
  h->d_path = nullptr; h->path_L = 0; h->path_cursor = -1;
  return 0;
}

static int in_set_options(Inner *h, const cddp_hip_options *opt) {
  if (!h || !opt) return fail(-1, "null argument");
  if (!(opt->reg_update_factor > 1.0) || !(opt->reg_max_value > 0.0))
    return fail(-2, "regularization.update_factor must be > 1 and max_value > 0 (got %g, %g)", opt->reg_update_factor, opt->reg_max_value);
  if (!opt->use_ilqr && !model_has_hessians(h->P.model)) return fail_no_hessians(h->P.model);
  { int rc = check_capacities(h->P.solver, opt); if (rc) return rc; }
  HIPCHK(hipSetDevice(h->device));
  { int rc = goal_to_host(h); if (rc) return rc; }   // P goes up whole below: with the goal the device holds
  double al[CDDP_HIP_MAX_ALPHAS];
  const int na = build_ladder(h->P.solver, opt, al, CDDP_HIP_MAX_ALPHAS);
  if (na != h->P.n_alphas) return fail(-3, "the line-search ladder size is fixed at create time (%d alphas, new options give %d)", h->P.n_alphas, na);
  if (h->d.ms && opt->max_iterations + 2 > h->d.filt_cap)
    return fail(-3, "max_iterations cannot grow beyond %d on an MSIPDDP handle (filter capacity fixed by cddp_hip_create)", h->d.filt_cap - 2);
  if (opt->max_iterations + 1 > h->d.hist_cap && h->P.opt.return_iteration_info)
    return fail(-3, "max_iterations cannot grow beyond %d on a handle created with return_iteration_info (history capacity)", h->d.hist_cap - 1);
  if ((opt->return_iteration_info != 0) != (h->P.opt.return_iteration_info != 0))
    return fail(-3, "return_iteration_info is fixed at create time (the history buffers are sized by cddp_hip_create)");
  h->P.opt = *opt;
  h->d.ddp = opt->use_ilqr ? 0 : 1;
  resolve_route(h);   // (full DDP takes other sweeps) -- and captured windows, which bake in the route and the DevBuf, are dropped
  for (auto &kv : h->graphs) hipGraphExecDestroy(kv.second); h->graphs.clear();
  for (int i = 0; i < na; ++i) h->P.alphas[i] = al[i];
  h->d.ladder_sorted = ladder_strictly_decreasing(al, na);
  h->P.ls_rule = opt->enable_parallel ? CDDP_HIP_LS_BEST_MERIT : CDDP_HIP_LS_FIRST_SUCCESS;
  HIPCHK(hipMemcpyAsync(h->dP, &h->P, sizeof(ProblemDev), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

static int in_set_initial_state(Inner *h, const double *x0) {
  if (!h || !x0) return fail(-1, "null argument");
  if (!h->have_initial) return fail(-1, "cddp_hip_set_initial must be called once before cddp_hip_set_initial_state");
  HIPCHK(hipSetDevice(h->device));
  const DevBuf &d = h->d;
  const int B = d.B, Bp = d.Bp, nx = h->P.nx;
  // the t = 0 record of every tile is the first NB * nx * 64 doubles of an X plane
  std::vector<double> row((size_t)d.NB * nx * 64, 0.0);
  for (int b = 0; b < B; ++b)
    for (int e = 0; e < nx; ++e) row[tix(0, nx, e, b, Bp)] = x0[(size_t)b * nx + e];
  for (int sl = 0; sl < d.n_slots; ++sl)
    HIPCHK(hipMemcpyAsync(d.X + (size_t)sl * d.planeX, row.data(), row.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_Xinit, row.data(), row.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->initialized = false;
  return 0;
}

static int in_set_duals(Inner *h, const double *S, const double *Y) {
  if (!h) return fail(-1, "null handle");
  if (h->P.solver != CDDP_HIP_SOLVER_IPDDP || h->P.m <= 0) return fail(-1, "cddp_hip_set_duals: the problem has no path duals");
  if (!h->has_state) return fail(-1, "cddp_hip_set_duals needs an initialised handle (call cddp_hip_initialize or cddp_hip_solve first)");
  HIPCHK(hipSetDevice(h->device));
  const DevBuf &d = h->d;
  std::vector<double> buf(d.planeM);
  const double *src[2] = {S, Y};
  double *dst[2] = {d.S, d.Y};
  for (int k = 0; k < 2; ++k) {
    if (!src[k]) continue;
    std::fill(buf.begin(), buf.end(), 0.0);
    to_soa(src[k], buf.data(), d.B, d.Bp, d.N, h->P.m);
    for (int sl = 0; sl < d.n_slots; ++sl)   // the live slot differs per trajectory: every slot gets the rows
      HIPCHK(hipMemcpyAsync(dst[k] + (size_t)sl * d.planeM, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

static int in_set_barrier_state(Inner *h, const double *mu, const double *reg) {
  if (!h) return fail(-1, "null handle");
  if (!h->has_state) return fail(-1, "cddp_hip_set_barrier_state needs an initialised handle (call cddp_hip_initialize or cddp_hip_solve first)");
  HIPCHK(hipSetDevice(h->device));
  const DevBuf &d = h->d;
  if (mu) {
    if (h->P.solver != CDDP_HIP_SOLVER_IPDDP) return fail(-1, "cddp_hip_set_barrier_state: mu is an IPDDP quantity");
    for (int b = 0; b < d.B; ++b) if (!(mu[b] > 0.0)) return fail(-2, "barrier parameter of trajectory %d must be positive (got %g)", b, mu[b]);
    HIPCHK(hipMemcpyAsync(d.mu, mu, sizeof(double) * d.B, hipMemcpyHostToDevice, h->stream));
  }
  if (reg) {
    for (int b = 0; b < d.B; ++b) if (!(reg[b] >= 0.0)) return fail(-2, "regularisation of trajectory %d must be non-negative (got %g)", b, reg[b]);
    HIPCHK(hipMemcpyAsync(d.reg, reg, sizeof(double) * d.B, hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

static int in_set_terminal(Inner *h, const double *S_T, const double *Y_T, const double *Lambda_T) {
  if (!h) return fail(-1, "null handle");
  if (h->P.n_term <= 0) return fail(-1, "cddp_hip_set_terminal: the problem has no terminal constraints");
  if (!h->has_state) return fail(-1, "cddp_hip_set_terminal needs an initialised handle");
  HIPCHK(hipSetDevice(h->device));
  const DevBuf &d = h->d;
  struct { const double *host; double *dev; int n; } items[] = {{S_T, d.ST, h->P.mT}, {Y_T, d.YT, h->P.mT}, {Lambda_T, d.LamT, h->P.pT}};
  for (auto &it : items) {
    if (!it.host || it.n <= 0) continue;
    std::vector<double> buf((size_t)it.n * d.Bp, 0.0);
    for (int b = 0; b < d.B; ++b) for (int i = 0; i < it.n; ++i) buf[(size_t)i * d.Bp + b] = it.host[(size_t)b * it.n + i];
    HIPCHK(hipMemcpyAsync(it.dev, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

static int in_backward(Inner *h, int32_t *ok) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (!h->initialized) { int rc = in_initialize(h); if (rc) return rc; }
  h->ks->derivs(h->d, h->route, 1, h->stream);
  h->ks->backward(h->d, h->route, h->P.solver, 1, 0, h->stream);
  HIPCHK(hipGetLastError());
  if (ok) HIPCHK(hipMemcpyAsync(ok, h->d.bwd_ok, sizeof(int) * h->d.B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// Time-sliced wave priority of a two-role IPDDP rollout launch (launch.hpp::RollSlice, PcSlice; kernels_lean.hpp::k_forward_ipddp_pc_sl).  n_run: the
// step sizes whose workgroups run from the launch's start (the whole ladder, or the first stage of a split launch: a sleeping stage-2
// workgroup takes no issue slots).  late_from = the workgroups that give every SIMD of the stream's share of the chip one wave; the window
// is on only where the running waves exceed those SIMDs.  CDDP_HIP_K4_SLICE_US = 0: never; n > 0: a window of about n us on EVERY launch,
// those of cddp_hip_forward included (the tests); CDDP_HIP_K4_LATE_PRIO=1: a fixed priority 3 for the late class instead of the window
// (the comparison row).  A speed heuristic only: HIP promises no dispatch order and no result depends on either figure.
// The default window, microseconds (rounded to a power of two of 10-ns ticks: 2.56 us, about one and a half producer steps of the cart-pole).
// Headline sweep of profiles/r17_simd_sharing.md section 3: the shorter the window the better down to this one; a fixed priority is worse than none.
constexpr int kK4SliceUs = 2;
static RollSlice roll_slice_for(const Inner *h, int conc, int n_run) {
  RollSlice sl;
  const Knobs &k = *h->knob;
  if (k.k4_slice_us == 0 || h->P.solver != CDDP_HIP_SOLVER_IPDDP || h->route.rollout != Route::kPair) return sl;
  const long simds = std::max(4L, (long)device_cu_count(h->device) * 4 / std::max(1, conc)), waves_per_wg = 2;
  sl.late_from = (int)(simds / waves_per_wg);
  const bool forced = k.k4_slice_us > 0;
  if (!forced && (long)((h->d.B + 63) / 64) * n_run * waves_per_wg <= simds) return sl;
  if (k.k4_late_prio) { sl.ticks = kSliceFixedLate; return sl; }
  const long want = 100L * (forced ? k.k4_slice_us : kK4SliceUs);   // ticks of the 100 MHz clock, rounded to a power of two (3 / 4 < ratio <= 3 / 2)
  sl.ticks = 1ull;
  while ((long)sl.ticks * 4 < want * 3) sl.ticks <<= 1;
  return sl;
}

static int in_forward(Inner *h, const double *alphas, int n_alphas, cddp_hip_trial *trials) {
  if (!h || !alphas || !trials) return fail(-1, "null argument");
  if (n_alphas <= 0 || n_alphas > h->d.n_alphas) return fail(-1, "n_alphas must be in [1, %d] (the handle's ladder size)", h->d.n_alphas);
  HIPCHK(hipSetDevice(h->device));
  { int rc = goal_to_host(h); if (rc) return rc; }   // P goes up whole, twice, below: with the goal the device holds
  // temporarily install the caller's alphas in the device problem block
  ProblemDev tmp = h->P;
  for (int i = 0; i < n_alphas; ++i) tmp.alphas[i] = alphas[i];
  HIPCHK(hipMemcpyAsync(h->dP, &tmp, sizeof(ProblemDev), hipMemcpyHostToDevice, h->stream));
  DevBuf dcall = h->d;   // (the caller's ladder may be any set of step sizes)
  dcall.ladder_sorted = ladder_strictly_decreasing(tmp.alphas, h->d.n_alphas);
  h->ks->forward(dcall, h->route, h->P.solver, 0, n_alphas, PH_FWD1, 1, 0, h->stream, 0, 0, roll_slice_for(h, 1, n_alphas));
  h->ks->costate(dcall, h->route, h->P.solver, 0, n_alphas, PH_FWD1, 1, 0, h->stream);
  HIPCHK(hipGetLastError());
  const DevBuf &d = h->d;
  const size_t n = (size_t)n_alphas * d.Bp;
  std::vector<double> c(n), mf(n), th(n), ipr(n), ic(n), ap(n), ad(n);
  std::vector<int> su(n);
  HIPCHK(hipMemcpyAsync(c.data(), d.t_cost, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(mf.data(), d.t_merit, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(th.data(), d.t_theta, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ipr.data(), d.t_inf_pr, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ic.data(), d.t_inf_comp, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ap.data(), d.t_apr, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ad.data(), d.t_adu, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(su.data(), d.t_success, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(h->dP, &h->P, sizeof(ProblemDev), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int b = 0; b < d.B; ++b)
    for (int a = 0; a < n_alphas; ++a) {
      cddp_hip_trial &t = trials[(size_t)b * n_alphas + a];
      const size_t i = (size_t)a * d.Bp + b;
      t.alpha = alphas[a]; t.alpha_pr = ap[i]; t.alpha_du = ad[i]; t.cost = c[i]; t.merit_function = mf[i];
      t.theta = th[i]; t.inf_pr = ipr[i]; t.inf_comp = ic[i]; t.success = (su[i] == 1) ? 1 : 0; t._pad = 0;   // 2 = non-finite costate (k_costate)
    }
  return 0;
}

// ---- ISolverAlgorithm::solve (cddp_solver_base.cpp:29-186) for one tile group -------------------------------
// The host loop of a group is resumable: `advance` enqueues iterations up to and including the next one that needs the
// "anything still running?" poll and records an event behind the poll's device-to-host copies; `complete_poll` waits for
// that event and digests the poll.  cddp_hip_solve interleaves the groups of a handle this way, so the kernels of several
// groups are in flight at once (each on its own stream) and the phases of different groups overlap on the chip.
struct SolveRun {
  Inner *h = nullptr;
  bool want_stats = false;
  int conc = 1;                     // groups solved concurrently (the ladder heuristics count the chip's wavefronts)
  int detail = -1;
  std::vector<int> ev_slot;         // ev_slot[6 * (iteration - 1) + point] = index into the pool, or -1
  size_t ev_used = 0;
  int launches = 0, outer = 0, it = 0, max_it = 0, na = 0;
  bool two_stage_marks = false, first_rule = true, pinned = false, one_stage = true, done = false, cpu_time_hit = false, use_graph = false;
  int k1 = 1, k_cap = 1, k_cap2 = 1;
  // shadow costate: K4b of an iteration rides in the next sweep launch (Inner::shadow_bufs); force_sync: the re-run of a discarded solve
  bool shadow = false, force_sync = false, pre_has_state = false, redo_needed = false;
  // Both stages of a two-stage iteration in ONE rollout launch (kernels_lean.hpp::k_forward_ipddp_pc, split argument): first-success rule,
  // the two-role rollout, and only with the shadow costate -- with k_costate on the chain a trial can be re-flagged 2 AFTER the rollout, and
  // a lane may then need step sizes the launch skipped for it.  CDDP_HIP_LS_INKERNEL=0: two launches everywhere (the comparison side).
  bool inkernel = false;
  int poll_us = kLsPollUs;
  int stamp0 = 0;                   // the handle's stamp count when the solve began (outer iteration i carries stamp0 + 2 i and + 1)
  long waves_all = 0, per_alpha_waves = 1, two_stage_max_waves = 768;
  std::vector<int> hist_now, hist_prev;
  // Polls are double-buffered (round 5): behind a poll the host enqueues Knobs::run_ahead more iterations (default 1; none behind the two early polls that settle the ladder shape) BEFORE it waits for
  // the poll's words, so the group's queue does not drain while the host wakes up and enqueues (the poll only decides the ladder
  // shape and whether anything is still running; surplus iterations after the last trajectory finished are launches whose every
  // lane exits on its phase check).  A whole window ahead (4) lags the ladder adaptation of converging solves by a window and costs
  // C3 more than the drain (profiles/r05_cumask.md); CDDP_HIP_RUNAHEAD=0 restores the drain-at-every-poll loop of rounds 1 - 4.
  static constexpr int kPollWords = CDDP_HIP_MAX_ALPHAS + 2;
  hipEvent_t poll_evs[2] = {nullptr, nullptr};
  int win_enq = 0, win_dig = 0, win_it[2] = {0, 0};
  int outstanding() const { return win_enq - win_dig; }
  bool ran_ahead = false;
  int post_poll(hipStream_t s) {
    const int slot = win_enq & 1;
    HIPCHK(hipMemcpyAsync(h->h_poll + slot * kPollWords, h->d.n_active, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->h_poll + slot * kPollWords + 1, h->d.win_hist, sizeof(int) * (na + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(poll_evs[slot], s));
    win_it[slot] = it;
    ++win_enq;
    return 0;
  }
  std::chrono::steady_clock::time_point wall0;
  // ping-pong of two half-batch groups (cddp_hip_solve): this group's rollout launches wait for the other group's last rollout and
  // are followed by an event the other group waits for -- the two groups' rollouts never share the chip, each runs beside the other
  // group's sweep / update kernels
  hipEvent_t fwd_wait = nullptr, fwd_done = nullptr;

  void mark(int point) {
    if (detail < 0) return;
    const bool want = detail == CDDP_HIP_TIMING_ALL ||
                      (detail == CDDP_HIP_TIMING_ROLLOUT && (point == 1 || point == 2 || (two_stage_marks && (point == 3 || point == 4)))) ||
                      (detail == CDDP_HIP_TIMING_SWEEP && (point == 0 || point == 1));
    if (!want) return;
    // class-timing events: no system-scope fence at the record (hipEventDisableSystemFence) -- a default event releases to system
    // scope, i.e. a cache write-back between two kernels of the chain; only the timestamps are read, after the solve's final sync.
    // CDDP_HIP_EVENT_FENCE=1 restores the default flags (A/B: profiles/r04_graph_ab.md)
    if (ev_used == h->ev_pool.size()) {
      hipEvent_t e;
      if ((h->knob->event_fence ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableSystemFence)) != hipSuccess) return;
      h->ev_pool.push_back(e);
    }
    const size_t slot = (size_t)6 * (size_t)(outer - 1) + (size_t)point;
    if (ev_slot.size() <= slot) ev_slot.resize(slot + 1, -1);
    hipEventRecord(h->ev_pool[ev_used], h->stream);
    ev_slot[slot] = (int)ev_used++;
  }

  // Ladder shape.  one_stage: all n_alpha trials of every trajectory in ONE launch.  Otherwise stage 1 evaluates the
  // first k1 alphas for every trajectory and stage 2 the rest, only for the trajectories none of the first k1 worked
  // for (a launch whose workgroups exit at once when there is no such trajectory).  The rollout is a latency chain:
  // up to one wavefront per SIMD (1024) extra alphas in a launch cost no wall time, beyond that the chains slow
  // each other down -- and a stage-2 launch costs a full chain as soon as ONE trajectory needs it.  The best shape
  // therefore depends on how many alphas the problem at hand needs (measured on MI355X, ms per solve at B = 4096 /
  // 8192: cart-pole, 5.3 alphas per iteration on average: one launch 48.7 / 98, k1 = 4: 54.6 / 89.5; unicycle, 1.4
  // alphas: one launch 96 / 152, k1 = 4: 66.8 / 86.0, k1 = 1: - / 124), so it follows the accepted-alpha histogram
  // K5 keeps (read with the "anything still running" poll): k1 = the smallest count that satisfies all but about one
  // trajectory per four iterations, capped at one wavefront per SIMD; when nearly the whole ladder is needed, all of it
  // in one launch if that fits two wavefronts per SIMD, else as many alphas as do (B = 16384 cart-pole: 210 vs 243 ms).
  // The selected trials do not depend on the shape (tests/test_gpu_parity.py::test_two_stage_ladder_selects_the_same_trials);
  // CDDP_HIP_LS_STAGES=1|2 and CDDP_HIP_LS_FIRST=k pin it.
  void adapt_ladder(int window_iters) {
    if (pinned) return;
    long total = 0;
    std::vector<long> hd(na + 1);
    for (int a = 0; a <= na; ++a) { hd[a] = (long)hist_now[a] - (long)hist_prev[a]; total += hd[a]; }
    hist_prev = hist_now;
    if (total <= 0) return;
    const long allow = std::max(1L, (long)window_iters / 4);   // trajectory-iterations left to stage 2 per window
    int kq = na;                                               // alphas needed to satisfy all but `allow`
    long tail = hd[na];
    for (int k = na - 1; k >= 1; --k) {                        // tail(k) = # not satisfied by the first k alphas
      tail += hd[k];
      if (tail <= allow) kq = k; else break;
    }
    if (kq >= na - 1) {
      if (waves_all <= 2048) { one_stage = true; }
      else { one_stage = false; k1 = k_cap2; }
    } else {
      // Margin (CDDP_HIP_LS_MARGIN; an explicit value holds everywhere): + 1 for the two-launch shapes, because the histogram drifts
      // between polls and a miss costs a second group-wide rollout + update (+ flush); + 0 where both stages run in one rollout launch
      // (`inkernel`), where a miss costs one tile's chain inside the launch (round 17).
      const int margin = h->knob->ls_margin >= 0 ? h->knob->ls_margin : (inkernel ? 0 : 1);
      one_stage = false; k1 = std::max(1, std::min(kq + margin, k_cap));
      // A chip that the whole ladder fills at most twice (one-stage territory) gains from a short first stage only what the
      // smaller launch saves over the rollout's latency floor (C2: 291 -> ~200 us at five step sizes), and loses a full second
      // rollout + costate + update (~235 us) whenever ONE trajectory walks past k1: kept only for a first stage of at most 768
      // waves (CDDP_HIP_LS_TWO_MAX_WAVES; profiles/r03_ladder_sweep.md: 512 / 640 / 768 / 1024 -> 47.3 / 46.8 / 46.1 / 46.4 ms
      // per C2 solve on one box, differences at the box-to-box noise level).
      // (Round 13: where both stages run in one rollout launch -- `inkernel` -- a miss costs one tile's chain inside the launch, not
      //  a second group-wide rollout + update + flush.  Re-swept under that cost, profiles/r13_inkernel_stages.md section 7: 768 /
      //  1024 / 2048 -> 37.0 / 37.2 / 37.2 ms per C2 solve, inside the spread: the threshold stays.  CDDP_HIP_LS_MARGIN=0 measured
      //  -0.6 ms there; round 17 repeated it in alternated rounds and made it the default of the in-kernel form, see `margin` above and
      //  profiles/r17_simd_sharing.md.)
      if (waves_all <= 2048 && (long)k1 * per_alpha_waves > two_stage_max_waves) one_stage = true;
      // A ladder that fits the chip once (at most one wavefront per SIMD) and light per-step work (nx <= 8): a first stage of more than
      // half of the ladder saves next to nothing over the whole ladder, while ONE trajectory past k1 costs a second full chain -- and
      // the histogram of such solves drifts towards smaller steps from window to window (resident LogDDP, cart-pole: k1 = 6 ... 10 of 11
      // during iterations 4 - 15; 34.3 -> 32.7 ms per solve with the whole ladder at once, profiles/r04_ladder_small.md).  Heavier plants keep the
      // short first stage (C4 share, 704 wavefronts: 955 ms adaptive against 985 ms with the whole ladder at once).  "Half" became "a third" after a sweep (CDDP_HIP_LS_SMALL_FRAC;
      // 2 / 3 / 4 / 11 -> C2-CLDDP 30.55 / 30.33 / 30.29 / 30.3 ms, pendulum MSIPDDP 15.2 / 15.0 / 15.05 / 17.3).
      // (the two-role rollouts of LogDDP / MSIPDDP, round 5, put two wavefronts per (tile, alpha) in the launch: the same ladders, twice the count)
      const long small_cap = (h->P.solver == CDDP_HIP_SOLVER_LOGDDP || h->P.solver == CDDP_HIP_SOLVER_MSIPDDP) ? 2048 : 1024;
      if (waves_all <= small_cap && h->P.nx <= 8 && h->knob->ls_small_frac * k1 > na) one_stage = true;
    }
    if (h->knob->debug_ladder) {
      std::fprintf(stderr, "[ladder] it=%d total=%ld kq=%d -> %s k1=%d hist:", outer, total, kq, one_stage ? "one" : "two", k1);
      for (int a = 0; a <= na; ++a) std::fprintf(stderr, " %ld", hd[a]);
      std::fprintf(stderr, "\n");
    }
  }

  RollSlice roll_slice(int n_run) const { return roll_slice_for(h, conc, n_run); }

  int begin(Inner *h_, bool stats_, int conc_) {
    h = h_; want_stats = stats_; conc = std::max(1, conc_);
    const ProblemDev &P = h->P;
    const DevBuf &d = h->d;
    hipStream_t s = h->stream;
    const KernelSet *ks = h->ks;
    max_it = P.opt.max_iterations;
    first_rule = (P.ls_rule == CDDP_HIP_LS_FIRST_SUCCESS);
    na = d.n_alphas;
    // Class timing: up to six mark points per outer iteration (0 start, 1 after the sweep, 2 after rollout stage 1,
    // 3 after update 1, 4 after rollout stage 2, 5 after update 2).  Every event costs ~5 us of queue time, so only
    // the points the selected detail needs are recorded (cddp_hip_set_timing_detail): 2 per iteration by default.
    use_graph = h->knob->graph;
    if (use_graph && conc > 1) {   // captured kernel nodes do not carry a stream's CU mask: the static partition is lost in replay (experiment switch; results unchanged)
      static bool said = false;
      if (!said) { said = true; std::fprintf(stderr, "[cddp_hip] CDDP_HIP_GRAPH=1: graph replay does not keep the CU-masked streams' partition; the tile groups share the whole chip\n"); }
    }
    detail = (want_stats && !use_graph) ? h->timing_detail : -1;
    if (!h->ev_begin) { HIPCHK(hipEventCreate(&h->ev_begin)); HIPCHK(hipEventCreate(&h->ev_end)); }
    if (!h->ev_poll) { HIPCHK(hipEventCreateWithFlags(&h->ev_poll, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&h->ev_poll2, hipEventDisableTiming)); }
    poll_evs[0] = h->ev_poll; poll_evs[1] = h->ev_poll2;
    win_enq = win_dig = 0; ran_ahead = false;
    if (!h->h_poll) HIPCHK(hipHostMalloc((void **)&h->h_poll, sizeof(int) * 2 * kPollWords));
    HIPCHK(hipMemsetAsync(h->d_launched, 0, sizeof(unsigned long long) * kLsGran, s));   // the rollout counter and the stage-2 tile counters
    HIPCHK(hipEventRecord(h->ev_begin, s));
    pre_has_state = h->has_state;
    shadow = !force_sync && shadow_eligible(h, conc) && max_it > 0;
    redo_needed = false;
    inkernel = shadow && P.ls_rule == CDDP_HIP_LS_FIRST_SUCCESS && h->knob->ls_inkernel &&
               (h->route.rollout == Route::kPair || h->route.rollout == Route::kTwoConsumers);
    poll_us = h->knob->ls_poll_us >= 0 ? h->knob->ls_poll_us : kLsPollUs;
    h->ls_counts[0] = h->ls_counts[1] = h->ls_counts[2] = 0;
    if (inkernel && !h->h_ls) HIPCHK(hipHostMalloc((void **)&h->h_ls, sizeof(unsigned long long) * kLsGran));
    h->last_shadow = shadow; h->ever_solved = true;
    if (shadow) HIPCHK(hipMemsetAsync(h->d.cs_bad, 0, sizeof(int), s));
    stamp0 = h->cs_epoch;
    { int rc = run_initialize(h); if (rc) return rc; }
    launches = 1; outer = 0; it = 0; done = false;
    *h->h_poll = d.B;
    // Speculative line search: when batch x n_alphas wavefronts still underfill the chip (256 CUs x 4 SIMDs),
    // evaluating the whole ladder in ONE launch costs no extra wall time and removes one rollout latency
    // per iteration; the first-success rule is then applied to the recorded trials, so results are unchanged.
    // (the two-role rollout of the path-constrained layouts runs two wavefronts per tile and alpha; with several tile
    // groups in flight the chip is shared: the group's wavefront count is scaled by the number of groups)
    waves_all = (long)conc * (long)((d.B + 63) / 64) * na * (((P.solver == CDDP_HIP_SOLVER_IPDDP && (ks->cst_size > 0 || (d.te_cst && P.m > 0))) || P.solver == CDDP_HIP_SOLVER_MSIPDDP || P.solver == CDDP_HIP_SOLVER_LOGDDP) ? 2 : 1);   // (layouts with two consumer waves keep the count the ladder rules were tuned with: their third wave is light)
    // CDDP_HIP_LS_STAGES=2 forces the two-stage ladder (alpha_0 first, the rest only for trajectories that need it)
    // regardless of the fill heuristic -- same selected trials; used by the tests to cover both launch shapes.
    const bool force_two = h->knob->ls_stages == '2', force_one = h->knob->ls_stages == '1';
    const long per_alpha = std::max(1L, waves_all / std::max(1, na));
    per_alpha_waves = per_alpha;
    two_stage_max_waves = h->knob->ls_two_max_waves;
    k_cap = (int)std::max(1L, std::min((long)na - 1, 1024 / per_alpha));    // one wavefront per SIMD
    k_cap2 = (int)std::max(1L, std::min((long)na - 1, 2048 / per_alpha));   // two (a ladder that is needed almost whole)
    const int k_forced = h->knob->ls_first;
    pinned = !first_rule || na == 1 || force_one || force_two || (k_forced >= 1 && k_forced < na);
    one_stage = !first_rule || na == 1 || force_one || (waves_all <= 2048 && !force_two);
    k1 = force_two ? 1 : k_cap2;
    if (k_forced >= 1 && k_forced < na && !force_one && first_rule) { one_stage = false; k1 = k_forced; }
    hist_now.assign(na + 1, 0); hist_prev.assign(na + 1, 0);
    HIPCHK(hipMemsetAsync(d.win_hist, 0, sizeof(int) * (CDDP_HIP_MAX_ALPHAS + 1), s));
    wall0 = std::chrono::steady_clock::now();
    if (max_it <= 0) { ks->update(d, h->route, 2, 0, 1, 1, s); ++launches; done = true; }
    return 0;
  }

  // The kernels of ONE outer iteration (K1 .. K5 in the current ladder shape), enqueued on the group's stream.
  void enqueue_iteration(int last) {
    const ProblemDev &P = h->P;
    if (shadow) {
      // the sweep of this iteration writes the other value stack; its extra blocks read the one the previous sweep wrote
      DevBuf &hd = h->d;
      hd.Vx_prev = hd.Vx; hd.Vxx_prev = hd.Vxx;
      std::swap(hd.Vx, hd.Vx2); std::swap(hd.Vxx, hd.Vxx2);
      hd.cs_vsel ^= 1;
    }
    DevBuf dsh = h->d;   // the launches' copy: the shadow words of this iteration
    if (shadow) {
      // Two stamps per outer iteration: cs_epoch (even) for the accepts of stage 1 of a TWO-stage iteration, cs_epoch + 1 for every other
      // accept.  The first kind cannot wait for the next sweep: the stage-2 rollout's lanes of a trajectory that is no longer in its phase
      // run along on trial slots taken relative to the NEW current slot (kernels_lean.hpp, k_forward_ipddp_pc), one of which may be the
      // slot the accepted step left -- whose x rows the costate needs.  Those rows are evaluated between update 1 and rollout 2.
      // (Only the two-LAUNCH form of a two-stage iteration has a stage-1 update: with both stages in one rollout launch -- `inkernel`,
      //  the default of a shadow solve -- cur[b] changes once, behind the launch, and every accept carries cs_epoch + 1.)
      h->cs_epoch += 2;
      dsh.cs_mode = 1; dsh.cs_stamp = h->cs_epoch + 1; dsh.cs_want = dsh.cs_stamp - 2;
      dsh.cs_fail_stamp = h->knob->fail_shadow > 0 ? stamp0 + 2 * h->knob->fail_shadow + 1 : 0;
    }
    const DevBuf &d = dsh;
    hipStream_t s = h->stream;
    const KernelSet *ks = h->ks;
    const Route &r = h->route;
    // CU-partitioned streams (CuPlan): the rollout on its own stream, ordered against the main stream by two events per launch
    hipStream_t sf = h->cu.fwd ? h->cu.fwd : s;
    auto to_fwd = [&](int k) { if (sf != s) { order_check(hipEventRecord(h->cu.ev[k], s)); order_check(hipStreamWaitEvent(sf, h->cu.ev[k], 0)); } };
    auto from_fwd = [&](int k) { if (sf != s) { order_check(hipEventRecord(h->cu.ev[k], sf)); order_check(hipStreamWaitEvent(s, h->cu.ev[k], 0)); } };
    const bool split = !one_stage && inkernel;   // a two-stage iteration as ONE rollout launch: the one-stage chain with the split handed to the kernel
    two_stage_marks = !one_stage && !split;
    mark(0);
    ks->derivs(d, r, 0, s);
    tl_sweep_hop = h->cu.sweep ? &h->cu.hop : nullptr;
    if (shadow && outer > 1) { dsh.cs_extra = ks->shadow_extra(d, r); ks->backward(dsh, r, P.solver, 0, 1, s); dsh.cs_extra = 0; }   // (the first iteration has nothing pending)
    else ks->backward(d, r, P.solver, 0, 1, s);
    tl_sweep_hop = nullptr;
    mark(1);
    to_fwd(0);
    if (fwd_wait) hipStreamWaitEvent(sf, fwd_wait, 0);
    if (one_stage || split) {
      // (split: the workgroups of the step sizes >= k1 learn inside the launch which lanes of their tile still need them; cur[b] does not
      //  change between the stages, so every accept carries the deferred stamp and no flush sits between rollouts)
      ks->forward(d, r, P.solver, 0, na, PH_FWD1, 0, first_rule ? 1 : 0, sf, split ? k1 : 0, poll_us, roll_slice(split ? k1 : na));
      if (fwd_done) hipEventRecord(fwd_done, sf);
      from_fwd(1);
      mark(2);
      if (!shadow) ks->costate(d, r, P.solver, 0, na, PH_FWD1, 0, first_rule ? 1 : 2, s);   // best-merit rule: the candidate winner's costate only (k_costate)
      ks->update(d, r, 1, na, last, 1, s);
      mark(3);
      launches += shadow ? 3 : 4;
    } else {
      ks->forward(d, r, P.solver, 0, k1, PH_FWD1, 0, 1, sf, 0, 0, roll_slice(k1));
      from_fwd(1);
      mark(2);
      if (!shadow) ks->costate(d, r, P.solver, 0, k1, PH_FWD1, 0, 1, s);
      if (shadow) {   // stage-1 accepts of a two-stage iteration: their own stamp, evaluated at once from this sweep's value stack (see above)
        DevBuf d1 = dsh;
        d1.cs_stamp = h->cs_epoch;
        ks->update(d1, r, 1, k1, last, 0, s);
        d1.cs_want = d1.cs_stamp; d1.Vx_prev = d1.Vx; d1.Vxx_prev = d1.Vxx;
        ks->shadow_flush(d1, nullptr, s);
      } else
      ks->update(d, r, 1, k1, last, 0, s);
      mark(3);
      to_fwd(2);
      ks->forward(d, r, P.solver, k1, na - k1, PH_FWD2, 0, 1, sf, 0, 0, RollSlice());   // (few of its workgroups run: no slicing)
      if (fwd_done) hipEventRecord(fwd_done, sf);
      from_fwd(3);
      mark(4);
      if (!shadow) ks->costate(d, r, P.solver, k1, na - k1, PH_FWD2, 0, 1, s);
      ks->update(d, r, 2, na, last, 1, s);
      mark(5);
      launches += shadow ? 5 : 6;
    }
  }
  bool polled_iteration(int i) const { return i % h->knob->poll_every == 0 || i == max_it || (i <= 2 && !pinned); }

  // CDDP_HIP_GRAPH=1 (experiment): the iterations between two polls are captured ONCE per (ladder shape, window
  // length, last-iteration flag) into a hipGraph and replayed with one hipGraphLaunch -- every kernel argument of an iteration is
  // a function of exactly those.  Measured on MI355X (profiles/r04_graph_ab.md): the gaps between dependent kernels are device-side
  // (barrier packet + cache invalidate), not submission latency -- the host already runs four iterations ahead of the device --
  // so replaying changes nothing measurable; class timing (hipEvents inside the window) is unavailable in this mode.  Off by default.
  int advance_graph() {
    const hipStream_t s = h->stream;
    int w = 0;
    while (it + w < max_it) { ++w; if (polled_iteration(it + w)) break; }
    if (w == 0) { done = true; return 0; }
    const int last = (it + w == max_it) ? 1 : 0;
    const unsigned long long key = ((unsigned long long)(one_stage ? 0 : k1) << 16) | ((unsigned long long)w << 4) | (unsigned long long)last;
    auto f = h->graphs.find(key);
    if (f == h->graphs.end()) {
      hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
      const int launches0 = launches;
      HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      for (int j = 1; j <= w; ++j) enqueue_iteration((j == w) ? last : 0);
      HIPCHK(hipStreamEndCapture(s, &g));
      HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
      hipGraphDestroy(g);
      launches = launches0;
      f = h->graphs.emplace(key, ge).first;
    }
    { const int l0 = launches; for (int j = 0; j < w; ++j) launches += one_stage ? 4 : 6; (void)l0; }
    HIPCHK(hipGraphLaunch(f->second, s));
    it += w; outer += w;
    { int rc = post_poll(s); if (rc) return rc; }
    return 1;
  }

  // enqueue iterations up to (and including) the next polled one
  int advance(int max_new = 1 << 30) {   // returns 1: a poll is pending, 2: stopped at the cap (no poll), 0: nothing more to enqueue
    if (done) return 0;
    int enq = 0;
    const ProblemDev &P = h->P;
    const DevBuf &d = h->d;
    hipStream_t s = h->stream;
    if (use_graph && !(P.opt.max_cpu_time > 0.0)) return advance_graph();
    while (it < max_it) {
      ++it;
      if (P.opt.max_cpu_time > 0.0) {   // cddp_solver_base.cpp:77-90 (host clock, like the reference; the queue is drained first)
        HIPCHK(hipStreamSynchronize(s));
        // whole elapsed milliseconds against max_cpu_time * 1000, as the reference's duration_cast<milliseconds> compares them
        const double el_ms = (double)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - wall0).count();
        if (el_ms > P.opt.max_cpu_time * 1000.0) {
          hipLaunchKernelGGL(k_mark_cpu_time, dim3((d.B + 255) / 256), dim3(256), 0, s, d);
          ++launches; done = true; cpu_time_hit = true;
          return 0;
        }
      }
      ++outer;
      const int last = (it == max_it) ? 1 : 0;
      enqueue_iteration(last);
      // The "anything still running?" poll drains the group's queue (host round trip + an empty pipeline for the next
      // launches), so it is made every Knobs::poll_every (4) iterations; the up-to-3 surplus iterations after the last
      // trajectory finished are launches whose every lane exits on its phase check.
      if (polled_iteration(it)) {   // every poll_every iterations, the last one, and two early polls: the ladder statistics settle the shape
        { int rc = post_poll(s); if (rc) return rc; }
        return 1;   // a poll is pending
      }
      if (++enq >= max_new) return 2;
    }
    done = true;
    return 0;
  }

  int complete_poll() {   // digests the OLDEST outstanding poll
    const int kPollEvery = h->knob->poll_every;
    if (outstanding() <= 0) return 0;
    const int slot = win_dig & 1;
    HIPCHK(hipEventSynchronize(poll_evs[slot]));
    ++win_dig;
    const int *w = h->h_poll + slot * kPollWords;
    const int pit = win_it[slot];
    if (w[0] == 0 || pit >= max_it) { done = true; win_dig = win_enq; return 0; }   // (later polls, if any, are dropped: finish() drains the stream)
    for (int a = 0; a <= na; ++a) hist_now[a] = w[1 + a];
    adapt_ladder(pit <= 2 ? 1 : (pit == kPollEvery ? 2 : kPollEvery));
    return 0;
  }

  // shadow costate, end of the solve (every exit: converged, max_iterations, max_cpu_time)
  int flush() {
    const DevBuf &d = h->d;
    hipStream_t s = h->stream;
    if (shadow) {
      // the rows of the last enqueued iteration's accepts, then the value rows of trajectories whose last sweep wrote the other stack;
      // the "not finite" word rides behind them and is read after the solve's one synchronisation
      DevBuf df = h->d, dm = h->d;
      df.cs_mode = 1; df.cs_want = h->cs_epoch > stamp0 ? h->cs_epoch + 1 : 0; df.Vx_prev = df.Vx; df.Vxx_prev = df.Vxx;
      df.cs_fail_stamp = h->knob->fail_shadow > 0 ? stamp0 + 2 * h->knob->fail_shadow + 1 : 0;
      h->ks->shadow_flush(df, &dm, s);
      launches += df.cs_want > 0 ? 2 : 1;
      HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d.cs_vbuf, d.cs_vsel, (size_t)d.Bp, s));   // every trajectory's rows are in the current stack now
      HIPCHK(hipMemcpyAsync(h->h_bad, d.cs_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    return 0;
  }

  int finish(cddp_hip_stats *stats) {
    const DevBuf &d = h->d;
    hipStream_t s = h->stream;
    HIPCHK(hipEventRecord(h->ev_end, s));
    if (inkernel) HIPCHK(hipMemcpyAsync(h->h_ls, h->d_launched, sizeof(unsigned long long) * kLsGran, hipMemcpyDeviceToHost, s));   // read with the solve's one synchronisation
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (inkernel) { h->ls_counts[0] = (long long)h->h_ls[kLsRan]; h->ls_counts[1] = (long long)h->h_ls[kLsRet]; h->ls_counts[2] = (long long)h->h_ls[kLsGiveUp]; }
    if (shadow && *h->h_bad != 0) { redo_needed = true; return 0; }   // discarded: cddp_hip_solve runs this group again with K4b on the chain
    if (tl_order_error != hipSuccess) {   // a cross-stream ordering call of this solve failed (launch.hpp::order_check): the results may come from racing kernels
      const hipError_t oe = tl_order_error; tl_order_error = hipSuccess;
      return fail(-10, "stream ordering (event record / wait) failed during the solve: %s", hipGetErrorString(oe));
    }
    if (!stats) return 0;
    std::memset(stats, 0, sizeof(*stats));
    float ms = 0;
    hipEventElapsedTime(&ms, h->ev_begin, h->ev_end);
    stats->solve_ms = ms;
    auto span = [&](size_t it0, int pa, int pb) -> double {   // elapsed between two mark points of one iteration
      const size_t ia = it0 * 6 + (size_t)pa, ib = it0 * 6 + (size_t)pb;
      if (ib >= ev_slot.size() || ev_slot[ia] < 0 || ev_slot[ib] < 0) return 0.0;
      float v = 0;
      hipEventElapsedTime(&v, h->ev_pool[ev_slot[ia]], h->ev_pool[ev_slot[ib]]);
      return v;
    };
    for (size_t it0 = 0; it0 * 6 < ev_slot.size(); ++it0) {
      stats->backward_ms += span(it0, 0, 1);                     // derivs + sweep
      stats->forward_ms += span(it0, 1, 2) + span(it0, 3, 4);    // rollout stage 1 (+ stage 2)
      stats->update_ms += span(it0, 2, 3) + span(it0, 4, 5);     // costate + update
    }
    // (two-stage iterations record the point between update 1 and rollout 2 in every mode; only the classes the
    //  detail names are reported)
    if (detail != CDDP_HIP_TIMING_ALL) stats->update_ms = 0.0;
    if (detail == CDDP_HIP_TIMING_ROLLOUT) stats->backward_ms = 0.0;
    if (detail == CDDP_HIP_TIMING_SWEEP) stats->forward_ms = 0.0;
    stats->timing_detail = detail;
    std::vector<int> nb(d.B), nf(d.B), itv(d.B), stv(d.B), nst(d.B);
    HIPCHK(hipMemcpy(nst.data(), d.n_fwd_steps, sizeof(int) * d.B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nb.data(), d.n_bwd, sizeof(int) * d.B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nf.data(), d.n_fwd, sizeof(int) * d.B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(itv.data(), d.iter, sizeof(int) * d.B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(stv.data(), d.status, sizeof(int) * d.B, hipMemcpyDeviceToHost));
    for (int b = 0; b < d.B; ++b) {
      stats->sweeps += nb[b]; stats->rollouts += nf[b]; stats->traj_iterations += itv[b]; stats->rollout_steps += nst[b];
      if (stv[b] == CDDP_HIP_STATUS_OPTIMAL || stv[b] == CDDP_HIP_STATUS_ACCEPTABLE) stats->n_converged++;
    }
    unsigned long long nl = 0;
    HIPCHK(hipMemcpy(&nl, h->d_launched, sizeof(nl), hipMemcpyDeviceToHost));
    stats->rollouts_launched = (int64_t)nl;
    stats->outer_iterations = outer; stats->kernel_launches = launches;
    return 0;
  }
};

// ---- getters -----------------------------------------------------------------------------
static int fetch(Inner *h, const double *dev, size_t n, std::vector<double> &host) {
  host.resize(n);
  HIPCHK(hipMemcpy(host.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

static int in_get_results(Inner *h, cddp_hip_result *r) {
  if (!h || !r) return fail(-1, "null argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  const int B = d.B;
  std::vector<double> v[10];
  const double *src[10] = {d.cost, d.merit, d.inf_pr, d.inf_du, d.inf_comp, d.mu, d.reg, d.alpha_pr, d.alpha_du, d.step_norm};
  for (int i = 0; i < 10; ++i) { int rc = fetch(h, src[i], B, v[i]); if (rc) return rc; }
  std::vector<int> it(B), st(B), nb(B), nf(B);
  HIPCHK(hipMemcpy(it.data(), d.iter, sizeof(int) * B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(st.data(), d.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nb.data(), d.n_bwd, sizeof(int) * B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nf.data(), d.n_fwd, sizeof(int) * B, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    r[b].final_objective = v[0][b]; r[b].merit_function = v[1][b]; r[b].inf_pr = v[2][b]; r[b].inf_du = v[3][b];
    r[b].inf_comp = v[4][b]; r[b].barrier_mu = v[5][b]; r[b].regularization = v[6][b]; r[b].alpha_pr = v[7][b];
    r[b].alpha_du = v[8][b]; r[b].step_norm = v[9][b]; r[b].iterations = it[b]; r[b].status = st[b];
    r[b].n_backward = nb[b]; r[b].n_forward = nf[b];
  }
  return 0;
}

// copies the CURRENT slot of every trajectory of a slotted array
static int fetch_current(Inner *h, const double *base, size_t plane, int T, int E, double *out) {
  const DevBuf &d = h->d;
  std::vector<int> cur(d.B);
  HIPCHK(hipMemcpy(cur.data(), d.cur, sizeof(int) * d.B, hipMemcpyDeviceToHost));
  std::vector<char> need(d.n_slots, 0);
  for (int b = 0; b < d.B; ++b) need[cur[b]] = 1;
  std::vector<double> buf;
  for (int s = 0; s < d.n_slots; ++s) {
    if (!need[s]) continue;
    int rc = fetch(h, base + (size_t)s * plane, plane, buf);
    if (rc) return rc;
    for (int b = 0; b < d.B; ++b) {
      if (cur[b] != s) continue;
      for (int t = 0; t < T; ++t)
        for (int e = 0; e < E; ++e) out[((size_t)b * T + t) * E + e] = buf[tix(t, E, e, b, d.Bp)];
    }
  }
  return 0;
}

static int in_get_trajectory(Inner *h, double *X, double *U) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  if (X) { int rc = fetch_current(h, d.X, d.planeX, d.N + 1, h->P.nx, X); if (rc) return rc; }
  if (U) { int rc = fetch_current(h, d.U, d.planeU, d.N, h->P.nu, U); if (rc) return rc; }
  return 0;
}

static int in_get_gains(Inner *h, double *K, double *k) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  std::vector<double> buf;
  if (K) { int rc = fetch(h, d.K, (size_t)d.N * h->P.nu * h->P.nx * d.Bp, buf); if (rc) return rc; from_soa(buf.data(), K, d.B, d.Bp, d.N, h->P.nu * h->P.nx); }
  if (k) { int rc = fetch(h, d.k, (size_t)d.N * h->P.nu * d.Bp, buf); if (rc) return rc; from_soa(buf.data(), k, d.B, d.Bp, d.N, h->P.nu); }
  return 0;
}

static int in_get_value(Inner *h, double *Vx, double *Vxx) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  std::vector<double> buf;
  if (Vx) { int rc = fetch(h, d.Vx, (size_t)(d.N + 1) * h->P.nx * d.Bp, buf); if (rc) return rc; from_soa(buf.data(), Vx, d.B, d.Bp, d.N + 1, h->P.nx); }
  if (Vxx) { int rc = fetch(h, d.Vxx, (size_t)(d.N + 1) * h->P.nx * h->P.nx * d.Bp, buf); if (rc) return rc; from_soa(buf.data(), Vxx, d.B, d.Bp, d.N + 1, h->P.nx * h->P.nx); }
  return 0;
}

static int in_get_linearization(Inner *h, double *A, double *Bm) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  std::vector<double> buf;
  auto conv = h->route.t4 ? &from_t4 : &from_soa;   // the handle's stack layout (0 for every solver but IPDDP)
  if (A) { int rc = fetch(h, d.A, (size_t)d.N * h->P.nx * h->P.nx * d.Bp, buf); if (rc) return rc; conv(buf.data(), A, d.B, d.Bp, d.N, h->P.nx * h->P.nx); }
  if (Bm) { int rc = fetch(h, d.Bm, (size_t)d.N * h->P.nx * h->P.nu * d.Bp, buf); if (rc) return rc; conv(buf.data(), Bm, d.B, d.Bp, d.N, h->P.nx * h->P.nu); }
  return 0;
}

static int in_get_duals(Inner *h, double *S, double *Y, double *G) {
  if (!h) return fail(-1, "null handle");
  if ((h->P.solver != CDDP_HIP_SOLVER_IPDDP && h->P.solver != CDDP_HIP_SOLVER_MSIPDDP) || h->P.m == 0) return fail(-1, "no slack/dual trajectories for this problem");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  if (S) { int rc = fetch_current(h, d.S, d.planeM, d.N, h->P.m, S); if (rc) return rc; }
  if (Y) { int rc = fetch_current(h, d.Y, d.planeM, d.N, h->P.m, Y); if (rc) return rc; }
  if (G) { int rc = fetch_current(h, d.G, d.planeM, d.N, h->P.m, G); if (rc) return rc; }
  return 0;
}

// Costate trajectory of the current iterate (Lambda_ of ipddp_solver.hpp / msipddp_solver.hpp): IPDDP N + 1 rows (k_costate / k_costate_one write
// the accepted trial's), MSIPDDP N rows (k_rows_msipddp)
static int costate_rows(const Inner *h) { return h->P.solver == CDDP_HIP_SOLVER_IPDDP ? h->d.N + 1 : h->d.N; }
static int in_get_costates(Inner *h, double *Lambda, int32_t *rows) {
  if (!h) return fail(-1, "null handle");
  if (h->P.solver != CDDP_HIP_SOLVER_IPDDP && h->P.solver != CDDP_HIP_SOLVER_MSIPDDP) return fail(-1, "no costate trajectory for this solver (IPDDP and MSIPDDP carry one)");
  if (rows) *rows = costate_rows(h);
  if (!Lambda) return 0;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return fetch_current(h, h->d.Lam, h->d.planeX, costate_rows(h), h->P.nx, Lambda);
}

static int in_get_terminal(Inner *h, double *S_T, double *Y_T, double *G_T, double *Lambda_T, int32_t *dims) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  const int mT = h->P.mT, pT = h->P.pT;
  if (dims) { dims[0] = mT; dims[1] = pT; }
  std::vector<double> buf;
  struct { const double *dev; double *host; int n; } items[] = {{d.ST, S_T, mT}, {d.YT, Y_T, mT}, {d.GT, G_T, mT}, {d.LamT, Lambda_T, pT}};
  for (auto &it : items) {
    if (!it.host || it.n == 0 || !it.dev) continue;
    int rc = fetch(h, it.dev, (size_t)it.n * d.Bp, buf); if (rc) return rc;
    for (int b = 0; b < d.B; ++b) for (int i = 0; i < it.n; ++i) it.host[(size_t)b * it.n + i] = buf[(size_t)i * d.Bp + b];
  }
  return 0;
}

static int in_get_backward_scalars(Inner *h, double *dV, double *reg) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const DevBuf &d = h->d;
  std::vector<double> a, b2;
  if (dV) {
    int rc = fetch(h, d.dV0, d.B, a); if (rc) return rc;
    rc = fetch(h, d.dV1, d.B, b2); if (rc) return rc;
    for (int b = 0; b < d.B; ++b) { dV[2 * b] = a[b]; dV[2 * b + 1] = b2[b]; }
  }
  if (reg) { int rc = fetch(h, d.reg, d.B, a); if (rc) return rc; for (int b = 0; b < d.B; ++b) reg[b] = a[b]; }
  return 0;
}

static int in_history_capacity(Inner *h) { return h ? h->d.hist_cap : -1; }

static int in_get_history(Inner *h, int hist_batch, double *hist, int32_t *counts) {
  if (!h || !hist || !counts) return fail(-1, "null argument");
  const DevBuf &d = h->d;
  if (hist_batch > d.hist_batch) return fail(-1, "history kept for %d trajectories only (options.return_iteration_info=%d)", d.hist_batch, h->P.opt.return_iteration_info);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(hist, d.hist, sizeof(double) * (size_t)hist_batch * d.hist_cap * kHistCols, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(counts, d.hist_n, sizeof(int) * hist_batch, hipMemcpyDeviceToHost));
  return 0;
}

static int in_get_plan_head(Inner *h, double *u0, double *x1) {
  if (!h) return fail(-1, "null handle");
  if (!h->has_state) return fail(-1, "cddp_hip_get_plan_head needs a solved or initialised handle");
  HIPCHK(hipSetDevice(h->device));
  const int B = h->d.B, nx = h->P.nx, nu = h->P.nu;
  const size_t n = (size_t)B * (nx + nu);
  if (h->head_cap < n) {
    if (h->d_head) hipFree(h->d_head);
    if (h->h_head) hipHostFree(h->h_head);
    h->d_head = nullptr; h->h_head = nullptr; h->head_cap = 0;
    HIPCHK(hipMalloc((void **)&h->d_head, n * sizeof(double)));
    HIPCHK(hipHostMalloc((void **)&h->h_head, n * sizeof(double)));
    h->head_cap = n;
  }
  hipLaunchKernelGGL(k_gather_plan_head, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->d, nx, nu, h->d_head);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h->h_head, h->d_head, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b) {
    const double *r = h->h_head + (size_t)b * (nx + nu);
    if (u0) for (int i = 0; i < nu; ++i) u0[(size_t)b * nu + i] = r[i];
    if (x1) for (int i = 0; i < nx; ++i) x1[(size_t)b * nx + i] = r[nu + i];
  }
  return 0;
}

static int in_write_gather_records_device(Inner *h, void *device_ptr) {
  if (!h || !device_ptr) return fail(-1, "null argument");
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_gather_records, dim3((h->d.B + 255) / 256), dim3(256), 0, h->stream, h->d, (cddp_hip_gather_record *)device_ptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- device-resident MPC step ---------------------------------------------------------------------------------------
// the refusals of cddp_hip_mpc_advance, tested for EVERY group before any group launches anything
static int in_mpc_check(Inner *h, int mode, int flags, bool need_plan = true) {
  if (!h) return fail(-1, "null handle");
  if (mode != CDDP_HIP_MPC_KEEP_PLAN && mode != CDDP_HIP_MPC_SHIFT_EXISTING && mode != CDDP_HIP_MPC_SHIFT_PROVIDED)
    return fail(-2, "cddp_hip_mpc_advance: unknown mode %d", mode);
  if (flags & ~(CDDP_HIP_MPC_SHIFT_DUALS | CDDP_HIP_MPC_X_DEVICE)) return fail(-2, "cddp_hip_mpc_advance: unknown flag bits 0x%x", flags);
  if (need_plan && (!h->have_initial || !h->has_plan))
    return fail(-1, "cddp_hip_mpc_advance needs a current plan: call cddp_hip_set_initial and cddp_hip_solve (or cddp_hip_initialize) first");
  if (flags & CDDP_HIP_MPC_SHIFT_DUALS) {
    if (mode != CDDP_HIP_MPC_SHIFT_EXISTING) return fail(-2, "cddp_hip_mpc_advance: CDDP_HIP_MPC_SHIFT_DUALS goes with CDDP_HIP_MPC_SHIFT_EXISTING only (the other modes keep or re-initialise the duals)");
    if (h->P.solver != CDDP_HIP_SOLVER_IPDDP || h->P.m <= 0) return fail(-1, "cddp_hip_mpc_advance: CDDP_HIP_MPC_SHIFT_DUALS: the problem has no path duals");
    if (need_plan && !h->has_state) return fail(-1, "cddp_hip_mpc_advance: CDDP_HIP_MPC_SHIFT_DUALS needs an initialised handle");
  }
  return 0;
}

// one group's MPC step (checked by in_mpc_check): kernels on the group's stream, host flags as the host sequence of the mode leaves them
static int in_mpc_advance(Inner *h, int mode, int flags, const double *x_next, bool sync_device_x) {
  HIPCHK(hipSetDevice(h->device));
  const DevBuf &d = h->d;
  const int nx = h->P.nx, nu = h->P.nu, m = h->P.m;
  const double *xdev = nullptr;
  const bool host_x = x_next && !(flags & CDDP_HIP_MPC_X_DEVICE);
  if (host_x) {   // the step's only upload: B * nx doubles into the staging buffer, tiled by k_mpc_state
    if (!h->d_xnext) HIPCHK(hipMalloc((void **)&h->d_xnext, (size_t)d.B * nx * sizeof(double)));
    HIPCHK(hipMemcpyAsync(h->d_xnext, x_next, (size_t)d.B * nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
    xdev = h->d_xnext;
  } else if (x_next) xdev = x_next;
  if (mode == CDDP_HIP_MPC_KEEP_PLAN) {
    hipLaunchKernelGGL(k_mpc_state, dim3((d.Bp + 255) / 256), dim3(256), 0, h->stream, d, nx, xdev, 1, h->d_Xinit);
  } else {
    const int sd = (flags & CDDP_HIP_MPC_SHIFT_DUALS) ? 1 : 0;
    hipLaunchKernelGGL(k_mpc_shift, dim3(d.NB, nx + nu + (sd ? 2 * m : 0)), dim3(64), 0, h->stream, d, nx, nu, m, sd, h->d_Xinit, h->d_Uinit);
    if (xdev) hipLaunchKernelGGL(k_mpc_state, dim3((d.Bp + 255) / 256), dim3(256), 0, h->stream, d, nx, xdev, 0, h->d_Xinit);
  }
  HIPCHK(hipGetLastError());
  // a bound reference path (cddp_hip_mpc_set_reference_path): the step moves the cursor, the next solve reads the next window
  if (h->d_path) { ++h->path_cursor; int rc = ref_install_window(h); if (rc) return rc; }
  // the caller's buffer is free again on return (a device x_next of a handle on the caller's own stream is ordered by that stream instead)
  if (host_x || (x_next && sync_device_x)) HIPCHK(hipStreamSynchronize(h->stream));
  h->initialized = false;
  if (mode != CDDP_HIP_MPC_KEEP_PLAN) { h->have_initial = true; h->initial_dirty = true; }
  if (mode == CDDP_HIP_MPC_SHIFT_PROVIDED) h->has_state = false;
  return 0;
}

// the log of cddp_hip_mpc_run: allocated on first use, grown when a longer run asks for it, cleared at the start of every run
static int in_mpc_log_begin(Inner *h, int steps) {
  HIPCHK(hipSetDevice(h->device));
  const size_t B = (size_t)h->d.B, nx = (size_t)h->P.nx, nu = (size_t)h->P.nu;
  if (h->log_steps < steps) {
    if (h->d_log_u) { hipFree(h->d_log_u); hipFree(h->d_log_x); hipFree(h->d_log_it); hipFree(h->d_log_st); }
    h->d_log_u = h->d_log_x = nullptr; h->d_log_it = h->d_log_st = nullptr; h->log_steps = 0;
    HIPCHK(hipMalloc((void **)&h->d_log_u, B * steps * nu * sizeof(double)));
    HIPCHK(hipMalloc((void **)&h->d_log_x, B * (steps + 1) * nx * sizeof(double)));
    HIPCHK(hipMalloc((void **)&h->d_log_it, B * steps * sizeof(int32_t)));
    HIPCHK(hipMalloc((void **)&h->d_log_st, B * steps * sizeof(int32_t)));
    h->log_steps = steps;
  }
  HIPCHK(hipMemsetAsync(h->d_log_u, 0, B * steps * nu * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->d_log_x, 0, B * (steps + 1) * nx * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->d_log_it, 0, B * steps * sizeof(int32_t), h->stream));
  HIPCHK(hipMemsetAsync(h->d_log_st, 0, B * steps * sizeof(int32_t), h->stream));
  return 0;
}
static int in_mpc_log(Inner *h, int steps, int k) {
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_mpc_log, dim3((h->d.B + 255) / 256), dim3(256), 0, h->stream, h->d, h->P.nx, h->P.nu, steps, k, h->d_Xinit,
                     h->d_log_u, h->d_log_x, h->d_log_it, h->d_log_st);
  HIPCHK(hipGetLastError());
  return 0;
}
// ONE copy per output: the log is kept in the outputs' own layout (batch-major, this group's trajectories contiguous)
static int in_mpc_log_fetch(Inner *h, int steps, double *U_applied, double *X_visited, int32_t *iterations, int32_t *status) {
  HIPCHK(hipSetDevice(h->device));
  const size_t B = (size_t)h->d.B, nx = (size_t)h->P.nx, nu = (size_t)h->P.nu;
  if (U_applied) HIPCHK(hipMemcpyAsync(U_applied, h->d_log_u, B * steps * nu * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (X_visited) HIPCHK(hipMemcpyAsync(X_visited, h->d_log_x, B * (steps + 1) * nx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (iterations) HIPCHK(hipMemcpyAsync(iterations, h->d_log_it, B * steps * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (status) HIPCHK(hipMemcpyAsync(status, h->d_log_st, B * steps * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}


// ================================================================================================================
// Public handle: the batch is cut into tile GROUPS (whole 64-trajectory tiles), each an independent Inner solver
// with its own device buffers, stream, counters and ladder statistics.  Trajectories are independent problems, so a
// trajectory's result does not depend on the group it lands in (tests/test_full_size.py: full batch == sub-batches,
// bit for bit); cddp_hip_solve keeps the kernels of all groups in flight at once, which lets the short, latency-bound
// sweep of one group run under the rollout of another instead of leaving three quarters of the SIMDs idle.
// CDDP_HIP_GROUPS=n pins the group count (1 = the single-stream path of round 1).
// ================================================================================================================
}  // extern "C" (reopened below)

struct cddp_hip_handle {
  Knobs knob;                // the switches, read when the handle is created (knobs.hpp); every group reads this copy
  std::vector<Inner *> g;
  std::vector<int> b0;       // first trajectory of each group
  int B = 0, device = 0;
  int conc = 1;              // groups in flight at once in cddp_hip_solve (pick_groups)
  hipEvent_t ev_pp[2] = {nullptr, nullptr};
  int nx = 0, nu = 0, N = 0, m = 0, mT = 0, pT = 0;
  hipStream_t user_stream = nullptr;   // cddp_hip_set_stream: work is ordered after / before this stream's work
  bool have_user_stream = false;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  void *d_send = nullptr;              // send buffer of cddp_hip_allgather_results (shard_capacity records)
  int send_cap = 0;
  char *d_staging = nullptr; size_t staging_cap = 0;   // the staging scratch of the host-or-device entries (struct Staging), in bytes, grown on demand
  bool staging_busy = false;                           // a call that used it returned without synchronising: the next acquisition waits for the group streams
  int32_t *d_winner = nullptr;                       // cddp_hip_seed_best: winner[B], the gather index of the seed
};

namespace {

// How the batch is cut.  Returns the group count; *conc = how many groups cddp_hip_solve keeps in flight at once.
//  * CDDP_HIP_GROUPS=n  (experiments, tests): n groups, all in flight concurrently (rounds 2-3).
//  * otherwise (round 4): CHUNKS.  A batch whose rollout launch would put more than ~2.75 wavefronts on every SIMD is solved as
//    several groups ONE AFTER THE OTHER.  Measured on MI355X at C2 (profiles/r03_batch_curve.md): 88.9 k trajectories/s at
//    B = 4096, 89.6 k at 8192, then 77.5 k at 16384 and 67.6 k at 32768 -- the rollout class grows super-linearly (51 -> 134 ->
//    333 ms) once the launch needs more than two residency rounds and the per-solve state (~0.1 MB per trajectory) is several
//    times the 256 MB Infinity Cache.  A trajectory's result does not depend on its group (bitwise, tests/test_full_size.py,
//    tests/test_determinism.py), so oversubscription costs nothing: the large batch runs at the throughput of its best chunk size
//    (profiles/r04_batch_curve.md).  CDDP_HIP_CHUNK=<trajectories> overrides the chunk size (0 = never chunk).
//  * round 5: STATIC CU PARTITION.  An IPDDP / CLDDP batch (or each chunk of a large one) of at least 32 tiles is cut into TWO groups that
//    are solved concurrently, each with every kernel of its iterations on its own symmetric half of the chip (streams created with
//    hipExtStreamCreateWithCUMask; mask bits [0, 128) and [128, 256) = half of the CUs of every XCD, see CuSpec).  Two independent
//    half-chips at half the batch run 3 - 6 % faster than the whole chip at the whole batch (profiles/r05_cumask.md: C2 45.6 -> 42.8 ms,
//    C3 81.5 -> 78.9, C4 share 955 -> 916, C5 share 1041 -> 992; CLDDP + 1.4 %, LogDDP 0, MSIPDDP - 4 %: not partitioned), while the
//    same two groups WITHOUT masks lose 3 - 5 % (their wavefronts share SIMDs) and any split that moves one kernel class to another
//    stream pays ~20 us of cross-stream events per iteration.  *part = slices (1 = no masks); CDDP_HIP_PARTITION=n overrides (1 = off).
int pick_groups(const Knobs &knob, int batch, int n_alphas, int solver, int *conc, int *part) {
  const int tiles = (batch + 63) / 64;
  int n = knob.groups;
  *part = 1;
  if (n > 0) { n = std::max(1, std::min(n, tiles)); *conc = n; return n; }
  *conc = 1;
  int chunk_tiles = std::max(16, 2816 / (2 * std::max(1, n_alphas)));     // 128 tiles (8192 trajectories) at 11 step sizes
  const bool chunking = knob.chunking;
  if (knob.chunk > 0) chunk_tiles = std::max(1, (knob.chunk + 63) / 64);
  const int chunks = chunking ? std::max(1, (tiles + chunk_tiles - 1) / chunk_tiles) : 1;
  int np = (solver == CDDP_HIP_SOLVER_IPDDP || solver == CDDP_HIP_SOLVER_CLDDP) ? 2 : 1;
  if (knob.partition && 256 % knob.partition == 0) np = knob.partition;
  if (knob.cumask_set) np = 1;                              // an explicit plan (experiments) replaces the default one
  if (np > 1 && tiles / chunks >= 16 * np) { *conc = np; *part = np; return chunks * np; }
  return chunks;
}

// ordering against a caller-supplied stream: fork = group streams wait for the user's stream, join = the reverse
int fork_from_user(cddp_hip_handle *h) {
  if (!h->have_user_stream) return 0;
  if (!h->ev_fork) { HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming)); }
  HIPCHK(hipEventRecord(h->ev_fork, h->user_stream));
  for (Inner *q : h->g) if (q->stream != h->user_stream) HIPCHK(hipStreamWaitEvent(q->stream, h->ev_fork, 0));
  return 0;
}
int join_to_user(cddp_hip_handle *h) {
  if (!h->have_user_stream) return 0;
  for (Inner *q : h->g) {
    if (q->stream == h->user_stream) continue;
    HIPCHK(hipEventRecord(h->ev_join, q->stream));
    HIPCHK(hipStreamWaitEvent(h->user_stream, h->ev_join, 0));
  }
  return 0;
}

}  // namespace

// the host loop of the groups in flight together (cddp_hip_solve), until none of them has anything left to enqueue or digest
static int drive_runs(SolveRun *run, int n) {
  for (;;) {
    bool any = false;
    for (int k = 0; k < n; ++k) {
      SolveRun &r = run[k];
      const Inner *g = r.h;
      const int ra = (g->P.opt.max_cpu_time > 0.0 || r.use_graph || r.it < g->knob->poll_every) ? 0 : g->knob->run_ahead;
      if (!r.done && r.outstanding() == 0) { int rc = r.advance(); if (rc < 0) return rc; r.ran_ahead = false; any = true; }
      else if (!r.done && r.outstanding() == 1 && ra > 0 && !r.ran_ahead) { int rc = r.advance(ra); if (rc < 0) return rc; r.ran_ahead = true; any = true; }
      else if (r.outstanding() > 0) { int rc = r.complete_poll(); if (rc) return rc; r.ran_ahead = r.outstanding() > 0; any = true; }
    }
    if (!any) break;
  }
  return 0;
}

// one solve's statistics added to the totals of an MPC run (timing_detail is a setting, not a sum)
static void stats_add(cddp_hip_stats *sum, const cddp_hip_stats &st) {
  sum->solve_ms += st.solve_ms; sum->backward_ms += st.backward_ms; sum->forward_ms += st.forward_ms; sum->update_ms += st.update_ms;
  sum->sweeps += st.sweeps; sum->rollouts += st.rollouts; sum->rollouts_launched += st.rollouts_launched;
  sum->traj_iterations += st.traj_iterations; sum->outer_iterations += st.outer_iterations; sum->n_converged += st.n_converged;
  sum->kernel_launches += st.kernel_launches; sum->timing_detail = st.timing_detail; sum->rollout_steps += st.rollout_steps;
}

extern "C" {

int cddp_hip_create(const cddp_hip_problem *problem, int batch, int device, cddp_hip_handle **out) {
  if (!problem || !out) return fail(-1, "null argument");
  if (batch <= 0) return fail(-1, "batch must be positive");
  { int rc = check_capacities(problem->solver, &problem->options); if (rc) return rc; }
  int conc = 1, part = 1;
  double ladder[CDDP_HIP_MAX_ALPHAS];
  const int n_ladder = build_ladder(problem->solver, &problem->options, ladder, CDDP_HIP_MAX_ALPHAS);   // the real ladder length (it can stop early at ls_min_step_size)
  cddp_hip_handle *h = new cddp_hip_handle();
  const Knobs &knob = h->knob;
  if (knob.fail_costate) std::fprintf(stderr, "[cddp_hip] TEST HOOK active: CDDP_HIP_TEST_FAIL_COSTATE=%d discards line-search trials -- results are not the solver's\n", knob.fail_costate);
  const int tiles = (batch + 63) / 64, ng = pick_groups(knob, batch, n_ladder, problem->solver, &conc, &part);
  h->B = batch; h->device = device; h->conc = conc;
  int t0 = 0;
  for (int k = 0; k < ng; ++k) {
    const int nt = tiles / ng + (k < tiles % ng ? 1 : 0);          // whole tiles per group, sizes differ by at most one tile
    const int first = t0 * 64, last = std::min(batch, (t0 + nt) * 64);
    t0 += nt;
    if (last <= first) continue;
    Inner *q = nullptr;
    CuSpec cus;
    bool have_cu = cu_spec_for_group(knob, k, &cus);
    if (!have_cu && part > 1) {
      // slice k of `part` equal slices of the CU-mask bits of THIS device (bit i = XCC i % 8, so a multiple of 8 bits is the same number of
      // CUs on every XCD); a device or partition mode too small for two CUs per XCD and slice runs unpartitioned
      const int w = device_cu_count(device) / part / 8 * 8;
      if (w >= 16) { cus.lo[0] = (k % part) * w; cus.hi[0] = cus.lo[0] + w; have_cu = true; }
    }
    int rc = in_create(problem, last - first, device, knob, have_cu ? &cus : nullptr, &q);
    if (rc) { for (Inner *p : h->g) in_destroy(p); delete h; return rc; }
    h->g.push_back(q); h->b0.push_back(first);
  }
  const ProblemDev &P = h->g[0]->P;
  h->nx = P.nx; h->nu = P.nu; h->N = P.N; h->m = P.m; h->mT = P.mT; h->pT = P.pT;
  *out = h;
  return 0;
}

int cddp_hip_destroy(cddp_hip_handle *h) {
  if (!h) return 0;
  for (Inner *q : h->g) in_destroy(q);
  if (h->ev_fork) { hipEventDestroy(h->ev_fork); hipEventDestroy(h->ev_join); }
  for (int k = 0; k < 2; ++k) if (h->ev_pp[k]) hipEventDestroy(h->ev_pp[k]);
  if (h->d_send) hipFree(h->d_send);
  if (h->d_staging) hipFree(h->d_staging);
  if (h->d_winner) hipFree(h->d_winner);
  delete h;
  return 0;
}

int cddp_hip_num_groups(cddp_hip_handle *h) { return h ? (int)h->g.size() : -1; }
int cddp_hip_costate_mode(cddp_hip_handle *h) {
  if (!h) return -1;
  for (Inner *q : h->g) if (!(q->ever_solved ? q->last_shadow : shadow_eligible(q, std::max(1, std::min(h->conc, (int)h->g.size()))))) return 0;
  return 1;
}
int cddp_hip_costate_redos(cddp_hip_handle *h) {
  if (!h) return -1;
  int n = 0;
  for (Inner *q : h->g) n += q->n_redo;
  return n;
}
int cddp_hip_ls_stage_counts(cddp_hip_handle *h, long long *counts) {
  if (!h || !counts) return -1;
  counts[0] = counts[1] = counts[2] = 0;
  for (Inner *q : h->g) for (int i = 0; i < 3; ++i) counts[i] += q->ls_counts[i];
  return 0;
}
int cddp_hip_concurrency(cddp_hip_handle *h) { return h ? std::max(1, std::min(h->conc, (int)h->g.size())) : -1; }

int cddp_hip_set_timing_detail(cddp_hip_handle *h, int detail) {
  if (!h) return fail(-1, "null handle");
  for (Inner *q : h->g) { int rc = in_set_timing_detail(q, detail); if (rc) return rc; }
  return 0;
}

int cddp_hip_set_stream(cddp_hip_handle *h, void *hip_stream) {
  if (!h) return fail(-1, "null handle");
  h->user_stream = (hipStream_t)hip_stream; h->have_user_stream = true;
  if (h->g.size() == 1) return in_set_stream(h->g[0], hip_stream);   // one group: it simply runs on the caller's stream
  return 0;   // several groups keep their own streams; every entry point forks from / joins to the caller's stream
}

int cddp_hip_dual_dim(cddp_hip_handle *h) { return h ? h->m : -1; }
int cddp_hip_batch(cddp_hip_handle *h) { return h ? h->B : -1; }

#define OFF(ptr, stride) ((ptr) ? (ptr) + (size_t)h->b0[gi_] * (size_t)(stride) : nullptr)
#define FOR_GROUPS(call) do { if (!h) return fail(-1, "null handle"); { int rc_ = fork_from_user(h); if (rc_) return rc_; } \
    for (size_t gi_ = 0; gi_ < h->g.size(); ++gi_) { Inner *q = h->g[gi_]; (void)q; int rc_ = (call); if (rc_) return rc_; } \
    return join_to_user(h); } while (0)

int cddp_hip_set_initial(cddp_hip_handle *h, const double *x0, const double *U0, const double *X0) {
  if (!x0) return fail(-1, "null argument");
  FOR_GROUPS(in_set_initial(q, OFF(x0, h->nx), OFF(U0, h->N * h->nu), OFF(X0, (h->N + 1) * h->nx)));
}
int cddp_hip_initialize(cddp_hip_handle *h) { FOR_GROUPS(in_initialize(q)); }
int cddp_hip_set_options(cddp_hip_handle *h, const cddp_hip_options *opt) { FOR_GROUPS(in_set_options(q, opt)); }
int cddp_hip_set_initial_state(cddp_hip_handle *h, const double *x0) {
  if (!x0) return fail(-1, "null argument");
  FOR_GROUPS(in_set_initial_state(q, OFF(x0, h->nx)));
}
int cddp_hip_forget_solver_state(cddp_hip_handle *h) {
  if (!h) return fail(-1, "null handle");
  for (Inner *q : h->g) { q->has_state = false; q->initialized = false; }   // (run_initialize: warm_start now means "provided trajectory"; the MSIPDDP factor cache stays with the handle as documented)
  return 0;
}
int cddp_hip_set_duals(cddp_hip_handle *h, const double *S, const double *Y) { FOR_GROUPS(in_set_duals(q, OFF(S, h->N * h->m), OFF(Y, h->N * h->m))); }
int cddp_hip_set_barrier_state(cddp_hip_handle *h, const double *mu, const double *reg) { FOR_GROUPS(in_set_barrier_state(q, OFF(mu, 1), OFF(reg, 1))); }
int cddp_hip_set_terminal(cddp_hip_handle *h, const double *S_T, const double *Y_T, const double *Lambda_T) {
  FOR_GROUPS(in_set_terminal(q, OFF(S_T, h->mT), OFF(Y_T, h->mT), OFF(Lambda_T, h->pT)));
}
int cddp_hip_backward(cddp_hip_handle *h, int32_t *ok) { FOR_GROUPS(in_backward(q, OFF(ok, 1))); }
int cddp_hip_forward(cddp_hip_handle *h, const double *alphas, int n_alphas, cddp_hip_trial *trials) {
  if (!alphas || !trials) return fail(-1, "null argument");
  FOR_GROUPS(in_forward(q, alphas, n_alphas, OFF(trials, n_alphas)));
}
int cddp_hip_get_results(cddp_hip_handle *h, cddp_hip_result *r) { if (!r) return fail(-1, "null argument"); FOR_GROUPS(in_get_results(q, OFF(r, 1))); }
int cddp_hip_get_plan_head(cddp_hip_handle *h, double *u0, double *x1) { FOR_GROUPS(in_get_plan_head(q, OFF(u0, h->nu), OFF(x1, h->nx))); }
int cddp_hip_get_trajectory(cddp_hip_handle *h, double *X, double *U) { FOR_GROUPS(in_get_trajectory(q, OFF(X, (h->N + 1) * h->nx), OFF(U, h->N * h->nu))); }
int cddp_hip_get_gains(cddp_hip_handle *h, double *K, double *k) { FOR_GROUPS(in_get_gains(q, OFF(K, h->N * h->nu * h->nx), OFF(k, h->N * h->nu))); }
int cddp_hip_get_value(cddp_hip_handle *h, double *Vx, double *Vxx) { FOR_GROUPS(in_get_value(q, OFF(Vx, (h->N + 1) * h->nx), OFF(Vxx, (h->N + 1) * h->nx * h->nx))); }
int cddp_hip_get_linearization(cddp_hip_handle *h, double *A, double *Bm) { FOR_GROUPS(in_get_linearization(q, OFF(A, h->N * h->nx * h->nx), OFF(Bm, h->N * h->nx * h->nu))); }
int cddp_hip_get_duals(cddp_hip_handle *h, double *S, double *Y, double *G) {
  FOR_GROUPS(in_get_duals(q, OFF(S, h->N * h->m), OFF(Y, h->N * h->m), OFF(G, h->N * h->m)));
}
int cddp_hip_get_costates(cddp_hip_handle *h, double *Lambda, int32_t *rows) {
  if (!h) return fail(-1, "null handle");
  const int r = (h->g.empty() || !h->g[0]) ? 0 : costate_rows(h->g[0]);
  FOR_GROUPS(in_get_costates(q, OFF(Lambda, r * h->nx), rows));
}
int cddp_hip_get_terminal(cddp_hip_handle *h, double *S_T, double *Y_T, double *G_T, double *Lambda_T, int32_t *dims) {
  FOR_GROUPS(in_get_terminal(q, OFF(S_T, h->mT), OFF(Y_T, h->mT), OFF(G_T, h->mT), OFF(Lambda_T, h->pT), dims));
}
int cddp_hip_get_backward_scalars(cddp_hip_handle *h, double *dV, double *reg) { FOR_GROUPS(in_get_backward_scalars(q, OFF(dV, 2), OFF(reg, 1))); }
int cddp_hip_history_capacity(cddp_hip_handle *h) { return h ? in_history_capacity(h->g[0]) : -1; }
int cddp_hip_get_history(cddp_hip_handle *h, int hist_batch, double *hist, int32_t *counts) {
  if (!h) return fail(-1, "null handle");
  // the history of the first min(batch, 64) trajectories is kept: they all live in group 0 (groups are whole tiles)
  return in_get_history(h->g[0], hist_batch, hist, counts);
}
int cddp_hip_write_gather_records_device(cddp_hip_handle *h, void *device_ptr) {
  if (!device_ptr) return fail(-1, "null argument");
  FOR_GROUPS(in_write_gather_records_device(q, (char *)device_ptr + (size_t)h->b0[gi_] * sizeof(cddp_hip_gather_record)));
}
#undef FOR_GROUPS
#undef OFF

// The single collective of the path: all-gather of the 16-byte result records over RCCL.
int cddp_hip_allgather_results(cddp_hip_handle *h, void *comm, int world, int shard_capacity, void *recv_device) {
  if (!h || !recv_device) return fail(-1, "null argument");
  if (world <= 0) return fail(-1, "world must be positive");
  if (shard_capacity < h->B) return fail(-1, "shard_capacity %d is smaller than this rank's batch %d", shard_capacity, h->B);
  if (!comm && world != 1) return fail(-1, "a NULL communicator is only valid for world == 1 (got %d)", world);
  HIPCHK(hipSetDevice(h->device));
  if (h->send_cap < shard_capacity) {
    if (h->d_send) { hipFree(h->d_send); h->d_send = nullptr; h->send_cap = 0; }
    HIPCHK(hipMalloc(&h->d_send, (size_t)shard_capacity * sizeof(cddp_hip_gather_record)));
    h->send_cap = shard_capacity;
  }
  hipStream_t cs = h->have_user_stream ? h->user_stream : h->g[0]->stream;   // the collective's stream
  // padding records of an uneven block partition: every byte 0xFF -> status = iterations = -1, cost = NaN
  if (shard_capacity > h->B)
    HIPCHK(hipMemsetAsync((char *)h->d_send + (size_t)h->B * sizeof(cddp_hip_gather_record), 0xFF,
                          (size_t)(shard_capacity - h->B) * sizeof(cddp_hip_gather_record), cs));
  for (size_t k = 0; k < h->g.size(); ++k) {   // (in_write_gather_records_device synchronises the group's stream)
    int rc = in_write_gather_records_device(h->g[k], (char *)h->d_send + (size_t)h->b0[k] * sizeof(cddp_hip_gather_record));
    if (rc) return rc;
  }
  const size_t bytes = (size_t)shard_capacity * sizeof(cddp_hip_gather_record);
  if (!comm) HIPCHK(hipMemcpyAsync(recv_device, h->d_send, bytes, hipMemcpyDeviceToDevice, cs));
  else { int rc = cddp_hip_internal_allgather(h->d_send, recv_device, bytes, comm, (void *)cs); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(cs));
  return 0;
}

int cddp_hip_solve(cddp_hip_handle *h, cddp_hip_stats *stats) {
  if (!h) return fail(-1, "null handle");
  HIPCHK(hipSetDevice(h->device));
  { int rc = fork_from_user(h); if (rc) return rc; }
  const int ng = (int)h->g.size();
  const auto solve_t0 = std::chrono::steady_clock::now();
  std::vector<SolveRun> run(ng);
  // `conc` groups are in flight at a time (all of them with CDDP_HIP_GROUPS; one with the default chunking of a large batch).
  // The whole-handle time is the span from group 0's begin to an end event group 0's stream records after it has waited for
  // every other group's end.
  const int conc = std::max(1, std::min(h->conc, ng));
  if (h->knob.pingpong && ng == 2) {   // two groups, rollouts alternating (CDDP_HIP_PINGPONG=1 with CDDP_HIP_GROUPS=2)
    // two half-batch groups in lockstep, one iteration each in turn; rollouts serialised A1 B1 A2 B2 ... by events (SolveRun::fwd_wait)
    if (!h->ev_pp[0]) for (int k = 0; k < 2; ++k) HIPCHK(hipEventCreateWithFlags(&h->ev_pp[k], hipEventDisableTiming));
    for (int k = 0; k < 2; ++k) { int rc = run[k].begin(h->g[k], stats != nullptr, 1); if (rc) return rc; run[k].fwd_wait = h->ev_pp[1 - k]; run[k].fwd_done = h->ev_pp[k]; }
    for (;;) {
      bool any = false;
      for (int k = 0; k < 2; ++k) {
        if (run[k].done || run[k].outstanding() > 0) continue;
        int rc = run[k].advance(1); if (rc < 0) return rc;
        any = any || rc != 0;
      }
      for (int k = 0; k < 2; ++k) if (run[k].outstanding() > 0) { int rc = run[k].complete_poll(); if (rc) return rc; any = true; }
      if (!any) break;
    }
  } else
  for (int base = 0; base < ng; base += conc) {
    const int top = std::min(ng, base + conc);
    for (int k = base; k < top; ++k) { int rc = run[k].begin(h->g[k], stats != nullptr, conc); if (rc) return rc; run[k].wall0 = solve_t0; }   // ONE max_cpu_time clock per solve, shared by successive chunks
    // each pass, per group: no poll outstanding -> enqueue iterations up to the next polled one; one outstanding and not yet run
    // ahead -> enqueue Knobs::run_ahead more iterations behind it; otherwise digest the oldest poll.  So a group's queue holds work while
    // the host waits for a poll, and the host never blocks on one group while another has nothing queued
    { int rc = drive_runs(&run[base], top - base);
      if (rc) { for (int k = 0; k < top; ++k) run[k].flush(); return rc; } }   // (the handle stays usable: pending costate rows and the value stacks are settled first)
  }
  for (int k = 0; k < ng; ++k) { int rc = run[k].flush(); if (rc) return rc; }
  // whole-handle device time: group 0's stream waits for the other groups' end events, then stamps the end
  std::vector<cddp_hip_stats> gs(ng);
  for (int k = 1; k < ng; ++k) {
    HIPCHK(hipEventRecord(h->g[k]->ev_end, h->g[k]->stream));
    HIPCHK(hipStreamWaitEvent(h->g[0]->stream, h->g[k]->ev_end, 0));
  }
  for (int k = 0; k < ng; ++k) { int rc = run[k].finish(stats ? &gs[k] : nullptr); if (rc) return rc; }
  // Shadow costate: a group whose deferred evaluation met a non-finite row is solved AGAIN, from the initial trajectory the handle keeps on
  // the device, with K4b on the chain (the serial move-past-the-bad-trial logic of k_update): the result of the unmodified launch sequence.
  double redo_ms = 0.0;
  for (int k = 0; k < ng; ++k) {
    if (!run[k].redo_needed) continue;
    Inner *q = h->g[k];
    q->has_state = run[k].pre_has_state;   // the same initialisation mode as the discarded attempt
    ++q->n_redo;
    SolveRun rr;
    rr.force_sync = true;
    { int rc = rr.begin(q, stats != nullptr, conc); if (rc) return rc; }   // (the same ladder heuristics and host loop as the first attempt)
    { int rc = drive_runs(&rr, 1); if (rc) return rc; }
    { int rc = rr.finish(stats ? &gs[k] : nullptr); if (rc) return rc; }
    if (stats) redo_ms += gs[k].solve_ms;
  }
  { int rc = join_to_user(h); if (rc) return rc; }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    float span_ms = 0;
    double first_begin_off = 0.0;
    // span = end(group 0, which waited for everybody) - earliest begin; the begins are enqueued back to back, so group
    // 0's begin is the earliest up to the few microseconds of its own enqueue
    hipEventElapsedTime(&span_ms, h->g[0]->ev_begin, h->g[0]->ev_end);
    (void)first_begin_off;
    stats->solve_ms = span_ms + redo_ms;
    for (int k = 0; k < ng; ++k) {
      // class times: groups that run concurrently overlap in wall time, so their per-class event spans are averaged over the
      // `conc` groups in flight together; successive chunks add up
      stats->backward_ms += gs[k].backward_ms / conc; stats->forward_ms += gs[k].forward_ms / conc; stats->update_ms += gs[k].update_ms / conc;
      stats->sweeps += gs[k].sweeps; stats->rollouts += gs[k].rollouts; stats->rollouts_launched += gs[k].rollouts_launched;
      stats->traj_iterations += gs[k].traj_iterations; stats->rollout_steps += gs[k].rollout_steps;
      stats->n_converged += gs[k].n_converged; stats->kernel_launches += gs[k].kernel_launches;
      stats->timing_detail = gs[k].timing_detail;
    }
    // outer iterations = rounds of (sweep, rollout, update) launches the handle went through one after the other: the longest group of
    // every concurrent set, summed over the successive sets (chunks) -- the divisor that matches the summed class times
    for (int base = 0; base < ng; base += conc) {
      int mx = 0;
      for (int k = base; k < std::min(ng, base + conc); ++k) mx = std::max(mx, gs[k].outer_iterations);
      stats->outer_iterations += mx;
    }
  }
  return 0;
}

// ---- device-resident MPC step: the seed of the next solve is made from the current plan where it lies (k_mpc_shift, k_mpc_state) ----
int cddp_hip_mpc_advance(cddp_hip_handle *h, int mode, int flags, const double *x_next) {
  if (!h) return fail(-1, "null handle");
  for (Inner *q : h->g) { int rc = in_mpc_check(q, mode, flags); if (rc) return rc; }   // refusals first: no kernel launched, no state changed
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    int rc = in_mpc_advance(h->g[gi], mode, flags, x_next ? x_next + (size_t)h->b0[gi] * (size_t)h->nx : nullptr, !h->have_user_stream);
    if (rc) return rc;
  }
  return join_to_user(h);
}

// ---- device-resident inputs and outputs: batch-major DEVICE arrays <-> the handle's internal layouts (inst_io.hip) ----
// what cddp_hip_get_field_device reads for one group: the buffer, slot rule, layout and extent of the field's host getter
struct IoField { int layout; const double *base; size_t plane; int T, E; };
static int io_field(const Inner *q, int field, IoField *f) {
  const DevBuf &d = q->d;
  const int N = d.N, nx = q->P.nx, nu = q->P.nu, m = q->P.m;
  const bool ipms = q->P.solver == CDDP_HIP_SOLVER_IPDDP || q->P.solver == CDDP_HIP_SOLVER_MSIPDDP;
  const int stack = q->route.t4 ? cddp_io::kT4 : cddp_io::kTiled;   // (in_get_linearization)
  switch (field) {
    case CDDP_HIP_FIELD_X: *f = IoField{cddp_io::kSlotted, d.X, d.planeX, N + 1, nx}; break;
    case CDDP_HIP_FIELD_U: *f = IoField{cddp_io::kSlotted, d.U, d.planeU, N, nu}; break;
    case CDDP_HIP_FIELD_K: *f = IoField{cddp_io::kTiled, d.K, 0, N, nu * nx}; break;
    case CDDP_HIP_FIELD_KFF: *f = IoField{cddp_io::kTiled, d.k, 0, N, nu}; break;
    case CDDP_HIP_FIELD_VX: *f = IoField{cddp_io::kTiled, d.Vx, 0, N + 1, nx}; break;
    case CDDP_HIP_FIELD_VXX: *f = IoField{cddp_io::kTiled, d.Vxx, 0, N + 1, nx * nx}; break;
    case CDDP_HIP_FIELD_A: *f = IoField{stack, d.A, 0, N, nx * nx}; break;
    case CDDP_HIP_FIELD_B: *f = IoField{stack, d.Bm, 0, N, nx * nu}; break;
    case CDDP_HIP_FIELD_S: case CDDP_HIP_FIELD_Y: case CDDP_HIP_FIELD_G:
      if (!ipms || m == 0) return fail(-1, "no slack/dual trajectories for this problem");
      *f = IoField{cddp_io::kSlotted, field == CDDP_HIP_FIELD_S ? d.S : field == CDDP_HIP_FIELD_Y ? d.Y : d.G, d.planeM, N, m}; break;
    case CDDP_HIP_FIELD_LAMBDA:
      if (!ipms) return fail(-1, "no costate trajectory for this solver (IPDDP and MSIPDDP carry one)");
      *f = IoField{cddp_io::kSlotted, d.Lam, d.planeX, costate_rows(q), nx}; break;
    default: return fail(-2, "unknown field id %d (cddp_hip_field)", field);
  }
  if (!f->base) return fail(-1, "field %d is not kept by this handle", field);
  return 0;
}

// A caller's pointer may reach a kernel only as device memory of the handle's device whose allocation holds every byte the call touches.
static int io_check_pointer(int device, const char *owner, const void *p, size_t bytes, const char *entry, const char *what) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(-2, "%s: %s is not device memory (%s)", entry, what, hipGetErrorString(e)); }
  if (at.type != hipMemoryTypeDevice)
    return fail(-2, "%s: %s is not device memory (%s)", entry, what,
                at.type == hipMemoryTypeHost ? "a pinned host address" : at.type == hipMemoryTypeUnregistered ? "a host address" : "managed or array memory");
  if (at.device != device) return fail(-2, "%s: %s lives on device %d, the %s on device %d", entry, what, at.device, owner, device);
  hipDeviceptr_t base = nullptr; size_t size = 0;
  const hipError_t e2 = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p);
  if (e2 != hipSuccess) { (void)hipGetLastError(); return fail(-2, "%s: the allocation of %s is unknown (%s)", entry, what, hipGetErrorString(e2)); }
  const size_t room = (size_t)((const char *)base + size - (const char *)p);
  if (bytes > room) return fail(-2, "%s: %s needs %zu bytes, its allocation ends after %zu", entry, what, bytes, room);
  return 0;
}
static int io_check_pointer(const cddp_hip_handle *h, const void *p, size_t bytes, const char *entry, const char *what) {
  return io_check_pointer(h->device, "handle", p, bytes, entry, what);
}

// Ordering as cddp_hip_mpc_advance with a device x_next: on the stream of cddp_hip_set_stream the kernels are ordered between the caller's
// work before and after the call (fork / join) and the call does not block; otherwise the group streams are synchronised before it returns.
static int io_finish(cddp_hip_handle *h) {
  HIPCHK(hipGetLastError());
  if (!h->have_user_stream) for (Inner *q : h->g) HIPCHK(hipStreamSynchronize(q->stream));
  return join_to_user(h);
}

// ---- staging of array arguments that are host pointers, or device pointers under the entry's *_DEVICE flag ----
// THE SCRATCH RULE.  h->d_staging is the handle's one staging scratch: grow-only, kept until cddp_hip_destroy, used by every entry below.
// It belongs to the call that acquired it until that call's work on the group streams is known to have completed.  The host forms and a
// device form without a caller's stream synchronise before they return; a device form on the stream of cddp_hip_set_stream does not (nor
// does a call that failed half-way), so the scratch stays marked busy and the NEXT acquisition first synchronises the group streams --
// the streams are non-blocking (make_stream), a null-stream hipMemcpy into the scratch would not wait for them by itself.
static int staging_acquire(cddp_hip_handle *h, size_t bytes) {
  if (h->staging_busy) { for (Inner *q : h->g) HIPCHK(hipStreamSynchronize(q->stream)); h->staging_busy = false; }
  if (h->staging_cap < bytes) {
    if (h->d_staging) hipFree(h->d_staging);
    h->d_staging = nullptr; h->staging_cap = 0;
    HIPCHK(hipMalloc((void **)&h->d_staging, bytes));
    h->staging_cap = bytes;
  }
  h->staging_busy = true;
  return 0;
}

// An entry declares its arrays in argument order; every declaration names the pointer variable ("slot") the kernels are to use, which
// begin() fills.  Device form: the caller's pointers, each checked by io_check_pointer in declaration order; scratch only for the
// internal blocks.  Host form: every array is a block of the scratch (8-byte aligned, carried by its byte count); begin() uploads the
// inputs, finish() synchronises and downloads the outputs.  An absent (NULL) array yields a NULL slot and is otherwise ignored.
}  // extern "C" (reopened below: the declarations are templates)
struct Staging {
  struct Arr { const char *name; const void *caller; size_t bytes; void *slot; size_t off; int dir; };   // dir: +1 input, -1 output, 0 internal
  static constexpr size_t kNoBlock = ~(size_t)0;                                                         // off of an array that owns no block
  cddp_hip_handle *h; const char *me; bool dev;
  std::vector<Arr> arr;
  size_t total = 0;
  Staging(cddp_hip_handle *h_, const char *me_, bool dev_) : h(h_), me(me_), dev(dev_) {}
  static void put(void *slot, const void *p) { std::memcpy(slot, &p, sizeof(p)); }
  static void *get(const void *slot) { void *p; std::memcpy(&p, slot, sizeof(p)); return p; }
  void add(const char *name, const void *caller, size_t bytes, void *slot, int dir, bool own) {
    if (dir != 0 && !caller) { if (own) put(slot, nullptr); return; }
    const bool block = own && (dir == 0 || !dev);
    if (own && !block) put(slot, caller);
    arr.push_back(Arr{name, caller, bytes, slot, block ? total : kNoBlock, dir});
    if (block) total += (bytes + 7) & ~(size_t)7;
  }
  template <class T> void in(const char *name, const T *p, size_t bytes, const T **slot) { add(name, p, bytes, slot, +1, true); }
  template <class T> void out(const char *name, T *p, size_t bytes, T **slot) { add(name, p, bytes, slot, -1, true); }
  template <class T> void scratch(size_t bytes, T **slot) { add(nullptr, nullptr, bytes, slot, 0, true); }
  // a caller's array that lives in an internal block (*block, declared before): the host form uploads to / downloads from the block,
  // the device form only checks the pointer -- the entry copies device to device, per group on the group's stream
  template <class T> void in_via(const char *name, const T *p, size_t bytes, T *const *block) { add(name, p, bytes, (void *)block, +1, false); }
  template <class T> void out_via(const char *name, T *p, size_t bytes, T *const *block) { add(name, p, bytes, (void *)block, -1, false); }
  // everything that precedes fork_from_user
  int begin() {
    if (dev) for (const Arr &a : arr) if (a.caller) { int rc = io_check_pointer(h, a.caller, a.bytes, me, a.name); if (rc) return rc; }
    if (total) { int rc = staging_acquire(h, total); if (rc) return rc; }
    for (const Arr &a : arr) if (a.off != kNoBlock) put(a.slot, h->d_staging + a.off);
    if (!dev) for (const Arr &a : arr) if (a.dir > 0) HIPCHK(hipMemcpy(get(a.slot), a.caller, a.bytes, hipMemcpyHostToDevice));
    return 0;
  }
  // everything that follows the loop over the tile groups
  int finish() {
    if (dev) { int rc = io_finish(h); if (rc) return rc; }
    else {
      HIPCHK(hipGetLastError());
      for (Inner *q : h->g) HIPCHK(hipStreamSynchronize(q->stream));
      for (const Arr &a : arr) if (a.dir < 0) HIPCHK(hipMemcpy(const_cast<void *>(a.caller), get(a.slot), a.bytes, hipMemcpyDeviceToHost));
    }
    if (!dev || !h->have_user_stream) h->staging_busy = false;   // the group streams were synchronised
    return dev ? 0 : join_to_user(h);
  }
};
extern "C" {

// the handle's own model as a plant: one step of dt, no box, the derived block of the ProblemDev on the device
static PlantDev own_model_plant(const Inner *q) {
  PlantDev pd;
  std::memset(&pd, 0, sizeof(pd));
  pd.model = q->P.model; pd.integrator = q->P.integrator; pd.substeps = 1; pd.nx = q->P.nx; pd.nu = q->P.nu; pd.Bp = q->d.Bp; pd.h = q->P.dt;
  pd.params = (const double *)((const char *)q->dP + offsetof(ProblemDev, mp));
  return pd;
}

// the result of a launch that picks its kernel by the plant's model id (what: "scoring" / "sampling"): hipErrorInvalidValue = no such kernel
static int plant_launch_rc(hipError_t e, const char *me, const char *what, const PlantDev &pd) {
  if (e == hipErrorInvalidValue) return fail(-3, "%s: the library has no %s kernel for model id %d with nx = %d, nu = %d", me, what, pd.model, pd.nx, pd.nu);
  HIPCHK(e);
  return 0;
}

// which plane of the slotted fields holds every trajectory's current iterate (the slot rule the slotted getters follow), for tests and diagnosis
int cddp_hip_get_live_slots(cddp_hip_handle *h, int32_t *slots, int32_t *n_slots) {
  if (!h) return fail(-1, "null handle");
  if (n_slots) *n_slots = h->g[0]->d.n_slots;
  if (!slots) return 0;
  HIPCHK(hipSetDevice(h->device));
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    Inner *q = h->g[gi];
    HIPCHK(hipMemcpyAsync(slots + h->b0[gi], q->d.cur, sizeof(int32_t) * (size_t)q->d.B, hipMemcpyDeviceToHost, q->stream));
    HIPCHK(hipStreamSynchronize(q->stream));
  }
  return join_to_user(h);
}

int cddp_hip_field_shape(cddp_hip_handle *h, int field, int32_t *rows, int32_t *cols) {
  if (!h) return fail(-1, "null handle");
  IoField f;
  { int rc = io_field(h->g[0], field, &f); if (rc) return rc; }
  if (rows) *rows = f.T;
  if (cols) *cols = f.E;
  return 0;
}

int cddp_hip_get_field_device(cddp_hip_handle *h, int field, double *out_dev) {
  if (!h) return fail(-1, "null handle");
  std::vector<IoField> f(h->g.size());
  for (size_t gi = 0; gi < h->g.size(); ++gi) { int rc = io_field(h->g[gi], field, &f[gi]); if (rc) return rc; }   // refusals first: nothing launched
  if (!out_dev) return fail(-1, "cddp_hip_get_field_device: null output pointer");
  HIPCHK(hipSetDevice(h->device));
  const size_t per = (size_t)f[0].T * (size_t)f[0].E;
  { int rc = io_check_pointer(h, out_dev, (size_t)h->B * per * sizeof(double), "cddp_hip_get_field_device", "the output"); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    io_untile(f[gi].layout, f[gi].base, q->d.cur, f[gi].plane, q->d.B, q->d.NB, f[gi].T, f[gi].E, out_dev + (size_t)h->b0[gi] * per, q->stream);
  }
  return io_finish(h);
}

int cddp_hip_get_results_device(cddp_hip_handle *h, double *cols_dev, int32_t *icols_dev) {
  if (!h) return fail(-1, "null handle");
  if (!cols_dev || !icols_dev) return fail(-1, "cddp_hip_get_results_device: null output pointer");
  HIPCHK(hipSetDevice(h->device));
  { int rc = io_check_pointer(h, cols_dev, (size_t)h->B * 10 * sizeof(double), "cddp_hip_get_results_device", "the double columns"); if (rc) return rc; }
  { int rc = io_check_pointer(h, icols_dev, (size_t)h->B * 4 * sizeof(int32_t), "cddp_hip_get_results_device", "the int32 columns"); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const DevBuf &d = q->d;
    const IoResultSrc src = {{d.cost, d.merit, d.inf_pr, d.inf_du, d.inf_comp, d.mu, d.reg, d.alpha_pr, d.alpha_du, d.step_norm}, {d.iter, d.status, d.n_bwd, d.n_fwd}};   // (in_get_results)
    io_results(src, d.B, cols_dev + (size_t)h->b0[gi] * 10, icols_dev + (size_t)h->b0[gi] * 4, q->stream);
  }
  return io_finish(h);
}

int cddp_hip_set_initial_device(cddp_hip_handle *h, const double *x0_dev, const double *U0_dev, const double *X0_dev) {
  if (!h) return fail(-1, "null handle");
  if (!x0_dev) return fail(-1, "cddp_hip_set_initial_device: null x0 pointer");
  HIPCHK(hipSetDevice(h->device));
  const size_t nX = (size_t)(h->N + 1) * h->nx, nU = (size_t)h->N * h->nu;
  { int rc = io_check_pointer(h, x0_dev, (size_t)h->B * h->nx * sizeof(double), "cddp_hip_set_initial_device", "x0"); if (rc) return rc; }
  if (U0_dev) { int rc = io_check_pointer(h, U0_dev, (size_t)h->B * nU * sizeof(double), "cddp_hip_set_initial_device", "U0"); if (rc) return rc; }
  if (X0_dev) { int rc = io_check_pointer(h, X0_dev, (size_t)h->B * nX * sizeof(double), "cddp_hip_set_initial_device", "X0"); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    io_tile(X0_dev ? X0_dev + b0 * nX : nullptr, x0_dev + b0 * h->nx, q->d.B, q->d.NB, h->N + 1, h->nx, q->d_Xinit, q->stream);
    io_tile(U0_dev ? U0_dev + b0 * nU : nullptr, nullptr, q->d.B, q->d.NB, h->N, h->nu, q->d_Uinit, q->stream);
    mark_seeded(q);
  }
  return io_finish(h);
}

// ---- moving the goal and the per-step reference of a live handle (include/cddp_hip.h; window kernel: inst_ref.hip) ----
static int ref_all_finite(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return 0;
  return 1;
}

int cddp_hip_set_reference(cddp_hip_handle *h, int flags, const double *x_ref, const double *x_ref_traj) {
  if (!h) return fail(-1, "cddp_hip_set_reference: null handle");
  if (flags & ~(CDDP_HIP_REF_DEVICE | CDDP_HIP_REF_CLEAR_TRAJ)) return fail(-2, "cddp_hip_set_reference: unknown flag bits 0x%x", flags);
  if ((flags & CDDP_HIP_REF_CLEAR_TRAJ) && x_ref_traj) return fail(-2, "cddp_hip_set_reference: CDDP_HIP_REF_CLEAR_TRAJ drops the per-step reference, x_ref_traj must be NULL with it");
  if (!x_ref && !x_ref_traj && !(flags & CDDP_HIP_REF_CLEAR_TRAJ)) return fail(-2, "cddp_hip_set_reference: nothing to change (x_ref and x_ref_traj are NULL and CDDP_HIP_REF_CLEAR_TRAJ is not set)");
  if (h->g[0]->d_path) return fail(-1, "cddp_hip_set_reference: a reference path is bound to this handle (cddp_hip_mpc_set_reference_path(h, NULL) unbinds it)");
  HIPCHK(hipSetDevice(h->device));
  const int nx = h->nx;
  const size_t nT = (size_t)(h->N + 1) * nx;
  if (flags & CDDP_HIP_REF_DEVICE) {
    if (x_ref) { int rc = io_check_pointer(h, x_ref, sizeof(double) * nx, "cddp_hip_set_reference", "x_ref"); if (rc) return rc; }
    if (x_ref_traj) { int rc = io_check_pointer(h, x_ref_traj, sizeof(double) * nT, "cddp_hip_set_reference", "x_ref_traj"); if (rc) return rc; }
  } else {
    if (x_ref && !ref_all_finite(x_ref, nx)) return fail(-2, "cddp_hip_set_reference: x_ref holds a non-finite value");
    if (x_ref_traj && !ref_all_finite(x_ref_traj, nT)) return fail(-2, "cddp_hip_set_reference: x_ref_traj holds a non-finite value");
    // the reference's constructor rule (objective.cpp:55-63) on the state this call leaves behind
    Inner *q = h->g[0];
    if (x_ref_traj || (q->d.xref_traj && !(flags & CDDP_HIP_REF_CLEAR_TRAJ))) {
      std::vector<double> goal(nx), last(nx);
      { int rc = fork_from_user(h); if (rc) return rc; }
      if (x_ref) for (int i = 0; i < nx; ++i) goal[i] = x_ref[i];
      else { int rc = goal_to_host(q); if (rc) return rc; for (int i = 0; i < nx; ++i) goal[i] = q->P.pool[q->P.off_xref + i]; }
      if (x_ref_traj) for (int i = 0; i < nx; ++i) last[i] = x_ref_traj[(size_t)h->N * nx + i];
      else {
        HIPCHK(hipMemcpyAsync(last.data(), q->d.xref_traj + (size_t)h->N * nx, sizeof(double) * nx, hipMemcpyDeviceToHost, q->stream));
        HIPCHK(hipStreamSynchronize(q->stream));
      }
      double s = 0.0;
      for (int i = 0; i < nx; ++i) s += (last[i] - goal[i]) * (last[i] - goal[i]);
      if (std::sqrt(s) > 1e-6) return fail(-2, "cddp_hip_set_reference: Last reference state must be same as the reference state (distance %g > 1e-6)", std::sqrt(s));
    }
  }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (Inner *q : h->g) { int rc = in_set_reference(q, flags, x_ref, x_ref_traj); if (rc) return rc; }
  return io_finish(h);
}

int cddp_hip_get_reference(cddp_hip_handle *h, double *x_ref, double *x_ref_traj, int32_t *has_traj) {
  if (!h) return fail(-1, "cddp_hip_get_reference: null handle");
  HIPCHK(hipSetDevice(h->device));
  { int rc = fork_from_user(h); if (rc) return rc; }
  const int nx = h->nx;
  const size_t nT = (size_t)(h->N + 1) * nx;
  const bool traj = h->g[0]->d.xref_traj != nullptr;
  std::vector<double> first(nx + (traj ? nT : 0)), other(first.size());
  for (size_t gi = 0; gi < h->g.size(); ++gi) {   // every tile group reads its own copy: they must all hold the same reference
    Inner *q = h->g[gi];
    std::vector<double> &o = gi == 0 ? first : other;
    if ((q->d.xref_traj != nullptr) != traj) return fail(-11, "cddp_hip_get_reference: tile group %zu disagrees on the per-step reference", gi);
    HIPCHK(hipMemcpyAsync(o.data(), goal_slot(q), sizeof(double) * nx, hipMemcpyDeviceToHost, q->stream));
    if (traj) HIPCHK(hipMemcpyAsync(o.data() + nx, q->d.xref_traj, sizeof(double) * nT, hipMemcpyDeviceToHost, q->stream));
    HIPCHK(hipStreamSynchronize(q->stream));
    if (gi > 0 && std::memcmp(first.data(), other.data(), first.size() * sizeof(double)) != 0)
      return fail(-11, "cddp_hip_get_reference: tile group %zu holds another reference than group 0", gi);
  }
  if (x_ref) std::memcpy(x_ref, first.data(), sizeof(double) * nx);
  if (x_ref_traj && traj) std::memcpy(x_ref_traj, first.data() + nx, sizeof(double) * nT);
  if (has_traj) *has_traj = traj ? 1 : 0;
  return join_to_user(h);
}

int cddp_hip_mpc_set_reference_path(cddp_hip_handle *h, const cddp_hip_ref_path *desc) {
  if (!h) return fail(-1, "cddp_hip_mpc_set_reference_path: null handle");
  if (!desc) {
    for (Inner *q : h->g) { int rc = in_unbind_path(q); if (rc) return rc; }
    return 0;
  }
  if (desc->abi_version != CDDP_HIP_ABI_VERSION) return fail(-2, "cddp_hip_mpc_set_reference_path: ABI version mismatch: got %d want %d", desc->abi_version, CDDP_HIP_ABI_VERSION);
  if (desc->flags & ~CDDP_HIP_REF_DEVICE) return fail(-2, "cddp_hip_mpc_set_reference_path: unknown flag bits 0x%x", desc->flags);
  if (desc->rows < 1) return fail(-2, "cddp_hip_mpc_set_reference_path: the path needs at least one row (rows = %lld)", (long long)desc->rows);
  if (desc->start < 0) return fail(-2, "cddp_hip_mpc_set_reference_path: the cursor cannot start before the path (start = %lld)", (long long)desc->start);
  if (!std::isfinite(desc->rows_per_step) || !(desc->rows_per_step > 0.0))
    return fail(-2, "cddp_hip_mpc_set_reference_path: rows_per_step must be finite and positive (got %g)", desc->rows_per_step);
  if (!desc->path) return fail(-1, "cddp_hip_mpc_set_reference_path: null path");
  if (desc->rows > (int64_t)1 << 40 || desc->start > (int64_t)1 << 60) return fail(-3, "cddp_hip_mpc_set_reference_path: rows or start out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t n = (size_t)desc->rows * (size_t)h->nx;
  if (desc->flags & CDDP_HIP_REF_DEVICE) { int rc = io_check_pointer(h, desc->path, n * sizeof(double), "cddp_hip_mpc_set_reference_path", "the path"); if (rc) return rc; }
  else if (!ref_all_finite(desc->path, n)) return fail(-2, "cddp_hip_mpc_set_reference_path: the path holds a non-finite value");
  { int rc = fork_from_user(h); if (rc) return rc; }
  // every group stages its copy before any group binds; a failure after that unbinds them all, so the groups never disagree
  std::vector<double *> staged(h->g.size(), nullptr);
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    int rc = in_stage_path(h->g[gi], desc, &staged[gi]);
    if (rc) { const std::string err = g_err; for (double *p : staged) if (p) hipFree(p); g_err = err; return rc; }
  }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    int rc = in_commit_path(h->g[gi], desc, staged[gi]);
    if (rc) {
      const std::string err = g_err;
      for (size_t k = gi + 1; k < staged.size(); ++k) hipFree(staged[k]);
      for (Inner *q : h->g) in_unbind_path(q);
      g_err = err;
      return rc;
    }
  }
  return io_finish(h);
}

int cddp_hip_mpc_reference_cursor(cddp_hip_handle *h, int64_t *cursor) {
  if (!h || !cursor) return fail(-1, "cddp_hip_mpc_reference_cursor: null argument");
  *cursor = h->g[0]->d_path ? (int64_t)h->g[0]->path_cursor : (int64_t)-1;
  return 0;
}

// ---- linear response of the plan to its initial state (inst_sens.hip): forward and adjoint recursions over the A / Bm / K stacks ----
// the refusals the two entries share, in the order of the header; nothing is launched and nothing changed before they have all passed
static int sens_refuse(const char *entry, const cddp_hip_handle *h, int flags, int nvec) {
  if (!h) return fail(-1, "%s: null handle", entry);
  if (flags & ~CDDP_HIP_SENS_DEVICE) return fail(-2, "%s: unknown flag bits 0x%x (CDDP_HIP_SENS_DEVICE is the only flag)", entry, (unsigned)(flags & ~CDDP_HIP_SENS_DEVICE));
  if (nvec < 1) return fail(-2, "%s: nvec = %d, at least one vector is needed", entry, nvec);
  return 0;
}
static int sens_refuse_handle(const char *entry, const cddp_hip_handle *h) {
  if (h->g[0]->P.solver == CDDP_HIP_SOLVER_MSIPDDP)
    return fail(-1, "%s: not for an MSIPDDP handle: its plan carries defects and its gains belong to the gap-closing recursion, so this recursion is not its response", entry);
  for (const Inner *q : h->g) {
    if (!q->has_plan) return fail(-1, "%s needs a solved handle: there are no A, B and K stacks before cddp_hip_solve (or cddp_hip_initialize and cddp_hip_backward)", entry);
    if (!q->d.A || !q->d.Bm || !q->d.K) return fail(-1, "%s: this handle keeps no A / B / K stacks", entry);
  }
  return 0;
}
static SensStacks sens_stacks(const Inner *q) {
  const DevBuf &d = q->d;
  return SensStacks{d.A, d.Bm, d.K, q->route.t4 ? cddp_io::kT4 : cddp_io::kTiled, d.B, d.NB, d.N, q->P.nx, q->P.nu};   // (io_field: the layout of A / Bm)
}

int cddp_hip_plan_jvp(cddp_hip_handle *h, int flags, int nvec, const double *dx0, double *dX, double *dU) {
  static const char *const me = "cddp_hip_plan_jvp";
  { int rc = sens_refuse(me, h, flags, nvec); if (rc) return rc; }
  if (!dx0) return fail(-1, "%s: null dx0 pointer", me);
  if (!dX && !dU) return fail(-1, "%s: dX and dU are both null: nothing to compute", me);
  { int rc = sens_refuse_handle(me, h); if (rc) return rc; }
  HIPCHK(hipSetDevice(h->device));
  const size_t n0 = (size_t)nvec * h->nx, nX = (size_t)nvec * (h->N + 1) * h->nx, nU = (size_t)nvec * h->N * h->nu, B = (size_t)h->B;
  Staging st(h, me, (flags & CDDP_HIP_SENS_DEVICE) != 0);
  const double *d0; double *dXd, *dUd;
  st.in("dx0", dx0, B * n0 * sizeof(double), &d0);
  st.out("dX", dX, B * nX * sizeof(double), &dXd);
  st.out("dU", dU, B * nU * sizeof(double), &dUd);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    HIPCHK(sens_jvp(sens_stacks(q), nvec, d0 + b0 * n0, dXd ? dXd + b0 * nX : nullptr, dUd ? dUd + b0 * nU : nullptr, q->stream));
  }
  return st.finish();
}

int cddp_hip_plan_vjp(cddp_hip_handle *h, int flags, int nvec, const double *gX, const double *gU, double *gx0) {
  static const char *const me = "cddp_hip_plan_vjp";
  { int rc = sens_refuse(me, h, flags, nvec); if (rc) return rc; }
  if (!gx0) return fail(-1, "%s: null gx0 pointer", me);
  { int rc = sens_refuse_handle(me, h); if (rc) return rc; }
  HIPCHK(hipSetDevice(h->device));
  const size_t n0 = (size_t)nvec * h->nx, nX = (size_t)nvec * (h->N + 1) * h->nx, nU = (size_t)nvec * h->N * h->nu, B = (size_t)h->B;
  Staging st(h, me, (flags & CDDP_HIP_SENS_DEVICE) != 0);
  const double *gXd, *gUd; double *g0;
  st.in("gX", gX, B * nX * sizeof(double), &gXd);
  st.in("gU", gU, B * nU * sizeof(double), &gUd);
  st.out("gx0", gx0, B * n0 * sizeof(double), &g0);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    HIPCHK(sens_vjp(sens_stacks(q), nvec, gXd ? gXd + b0 * nX : nullptr, gUd ? gUd + b0 * nU : nullptr, g0 + b0 * n0, q->stream));
  }
  return st.finish();
}

// ---- state and control covariance along the plan (inst_cov.hip): the closed-loop covariance recursion over the A / Bm / K stacks ----
int cddp_hip_plan_covariance(cddp_hip_handle *h, int flags, const double *Sigma0, const double *W, const double *Wu, double *SX, double *SU, double *dcost) {
  static const char *const me = "cddp_hip_plan_covariance";
  constexpr int known = CDDP_HIP_COV_DEVICE | CDDP_HIP_COV_DIAG | CDDP_HIP_COV_PER_TRAJ;
  if (!h) return fail(-1, "%s: null handle", me);
  if (flags & ~known) return fail(-2, "%s: unknown flag bits 0x%x (CDDP_HIP_COV_DEVICE, CDDP_HIP_COV_DIAG and CDDP_HIP_COV_PER_TRAJ are the flags)", me, (unsigned)(flags & ~known));
  if (!Sigma0) return fail(-1, "%s: null Sigma0 pointer", me);
  if (!SX && !SU && !dcost) return fail(-1, "%s: SX, SU and dcost are all null: nothing to compute", me);
  { int rc = sens_refuse_handle(me, h); if (rc) return rc; }
  HIPCHK(hipSetDevice(h->device));
  const bool dev = (flags & CDDP_HIP_COV_DEVICE) != 0, diag = (flags & CDDP_HIP_COV_DIAG) != 0, per = (flags & CDDP_HIP_COV_PER_TRAJ) != 0;
  const size_t nx = (size_t)h->nx, nu = (size_t)h->nu, B = (size_t)h->B;
  const size_t nS = (per ? B : 1) * nx * nx, nWu = (per ? B : 1) * nu * nu;                       // doubles of Sigma0 / W, of Wu
  const size_t eX = (size_t)(h->N + 1) * (diag ? nx : nx * nx), eU = (size_t)h->N * (diag ? nu : nu * nu);   // doubles per trajectory of SX, of SU
  Staging st(h, me, dev);
  const double *S0d, *Wd, *Wud; double *SXd, *SUd, *dcd;
  st.in("Sigma0", Sigma0, nS * sizeof(double), &S0d);
  st.in("W", W, nS * sizeof(double), &Wd);
  st.in("Wu", Wu, nWu * sizeof(double), &Wud);
  st.out("SX", SX, B * eX * sizeof(double), &SXd);
  st.out("SU", SU, B * eU * sizeof(double), &SUd);
  st.out("dcost", dcost, B * sizeof(double), &dcd);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi], p0 = per ? b0 : 0;
    const double *pool = (const double *)((const char *)q->dP + offsetof(ProblemDev, pool));
    CovArgs a;
    a.Sigma0 = S0d + p0 * nx * nx; a.W = Wd ? Wd + p0 * nx * nx : nullptr; a.Wu = Wud ? Wud + p0 * nu * nu : nullptr;
    a.SX = SXd ? SXd + b0 * eX : nullptr; a.SU = SUd ? SUd + b0 * eU : nullptr; a.dcost = dcd ? dcd + b0 : nullptr;
    a.Qdt = pool + q->P.off_Qdt; a.Rdt = pool + q->P.off_Rdt; a.Qf = pool + q->P.off_Qf;
    a.per_traj = per ? 1 : 0; a.diag = diag ? 1 : 0;
    HIPCHK(plan_cov(sens_stacks(q), a, q->stream));
  }
  return st.finish();
}

// ---- time-varying LQR gains along the plan (inst_lqr.hip): the backward Riccati recursion over the A / Bm stacks ----
int cddp_hip_plan_tvlqr(cddp_hip_handle *h, int flags, const double *Q, const double *R, const double *Qf, double *K_out, double *P_out, int32_t *info) {
  static const char *const me = "cddp_hip_plan_tvlqr";
  constexpr int known = CDDP_HIP_LQR_DEVICE | CDDP_HIP_LQR_PER_TRAJ | CDDP_HIP_LQR_INSTALL;
  if (!h) return fail(-1, "%s: null handle", me);
  if (flags & ~known) return fail(-2, "%s: unknown flag bits 0x%x (CDDP_HIP_LQR_DEVICE, CDDP_HIP_LQR_PER_TRAJ and CDDP_HIP_LQR_INSTALL are the flags)", me, (unsigned)(flags & ~known));
  const bool dev = (flags & CDDP_HIP_LQR_DEVICE) != 0, per = (flags & CDDP_HIP_LQR_PER_TRAJ) != 0, install = (flags & CDDP_HIP_LQR_INSTALL) != 0;
  if (!K_out && !P_out && !install) return fail(-1, "%s: K_out and P_out are both null and CDDP_HIP_LQR_INSTALL is not set: nothing to compute", me);
  { int rc = sens_refuse_handle(me, h); if (rc) return rc; }
  const size_t nx = (size_t)h->nx, nu = (size_t)h->nu, B = (size_t)h->B, lead = per ? B : 1;
  if (!dev) {
    if (Q && !ref_all_finite(Q, lead * nx * nx)) return fail(-2, "%s: Q holds a non-finite value", me);
    if (R && !ref_all_finite(R, lead * nu * nu)) return fail(-2, "%s: R holds a non-finite value", me);
    if (Qf && !ref_all_finite(Qf, lead * nx * nx)) return fail(-2, "%s: Qf holds a non-finite value", me);
  }
  HIPCHK(hipSetDevice(h->device));
  const size_t eK = (size_t)h->N * nu * nx, eP = (size_t)(h->N + 1) * nx * nx;     // doubles per trajectory of K_out, of P_out
  Staging st(h, me, dev);
  const double *Qd, *Rd, *Qfd; double *Kd, *Pd; int32_t *infd;
  st.in("Q", Q, lead * nx * nx * sizeof(double), &Qd);
  st.in("R", R, lead * nu * nu * sizeof(double), &Rd);
  st.in("Qf", Qf, lead * nx * nx * sizeof(double), &Qfd);
  st.out("K_out", K_out, B * eK * sizeof(double), &Kd);
  st.out("P_out", P_out, B * eP * sizeof(double), &Pd);
  st.out("info", info, B * sizeof(int32_t), &infd);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi], p0 = per ? b0 : 0;
    const double *pool = (const double *)((const char *)q->dP + offsetof(ProblemDev, pool));
    LqrArgs a;
    // a weight that is given: the caller's, times dt where it is read (Q, R); one that is not: the handle's own Q dt / R dt / Qf, shared
    a.Q = Qd ? Qd + p0 * nx * nx : pool + q->P.off_Qdt; a.q_per = Qd && per; a.q_scale = Qd ? q->P.dt : 1.0;
    a.R = Rd ? Rd + p0 * nu * nu : pool + q->P.off_Rdt; a.r_per = Rd && per; a.r_scale = Rd ? q->P.dt : 1.0;
    a.Qf = Qfd ? Qfd + p0 * nx * nx : pool + q->P.off_Qf; a.qf_per = Qfd && per;
    a.K_out = Kd ? Kd + b0 * eK : nullptr; a.P_out = Pd ? Pd + b0 * eP : nullptr; a.info = infd ? infd + b0 : nullptr;
    a.K_stack = install ? q->d.K : nullptr;
    HIPCHK(plan_lqr(sens_stacks(q), a, q->stream));
  }
  return st.finish();
}

// ---- Kalman filter gains and output-feedback covariance along the plan (inst_kf.hip): the forward dual of the recursion above ----
int cddp_hip_plan_kalman(cddp_hip_handle *h, int flags, int ny, const double *C, const double *v, const double *Sigma0, const double *W, const double *Wu,
                         double *L_out, double *SP_out, double *SF_out, double *SX, double *SU, double *dcost, int32_t *info) {
  static const char *const me = "cddp_hip_plan_kalman";
  constexpr int known = CDDP_HIP_KF_DEVICE | CDDP_HIP_KF_DIAG | CDDP_HIP_KF_PER_TRAJ;
  if (!h) return fail(-1, "%s: null handle", me);
  if (flags & ~known) return fail(-2, "%s: unknown flag bits 0x%x (CDDP_HIP_KF_DEVICE, CDDP_HIP_KF_DIAG and CDDP_HIP_KF_PER_TRAJ are the flags)", me, (unsigned)(flags & ~known));
  if (ny < 1 || ny > CDDP_HIP_KF_MAX_NY) return fail(-2, "%s: ny = %d, 1 .. %d measurement rows are expected", me, ny, CDDP_HIP_KF_MAX_NY);
  if (!C) return fail(-1, "%s: null C pointer", me);
  if (!v) return fail(-1, "%s: null v pointer", me);
  if (!Sigma0) return fail(-1, "%s: null Sigma0 pointer", me);
  if (!L_out && !SP_out && !SF_out && !SX && !SU && !dcost && !info) return fail(-1, "%s: all six outputs and info are null: nothing to compute", me);
  { int rc = sens_refuse_handle(me, h); if (rc) return rc; }
  const bool dev = (flags & CDDP_HIP_KF_DEVICE) != 0, diag = (flags & CDDP_HIP_KF_DIAG) != 0, per = (flags & CDDP_HIP_KF_PER_TRAJ) != 0;
  const size_t nx = (size_t)h->nx, nu = (size_t)h->nu, B = (size_t)h->B, lead = per ? B : 1, m = (size_t)ny;
  if (!dev) {
    for (size_t i = 0; i < lead * m; ++i)
      if (!std::isfinite(v[i]) || !(v[i] > 0.0)) return fail(-2, "%s: v holds an entry that is not finite and > 0 (a measurement variance)", me);
    if (!ref_all_finite(C, lead * m * nx)) return fail(-2, "%s: C holds a non-finite value", me);
    if (!ref_all_finite(Sigma0, lead * nx * nx)) return fail(-2, "%s: Sigma0 holds a non-finite value", me);
    if (W && !ref_all_finite(W, lead * nx * nx)) return fail(-2, "%s: W holds a non-finite value", me);
    if (Wu && !ref_all_finite(Wu, lead * nu * nu)) return fail(-2, "%s: Wu holds a non-finite value", me);
  }
  HIPCHK(hipSetDevice(h->device));
  const size_t eL = (size_t)(h->N + 1) * nx * m;                                                            // doubles per trajectory of L_out
  const size_t eX = (size_t)(h->N + 1) * (diag ? nx : nx * nx), eU = (size_t)h->N * (diag ? nu : nu * nu);   // ... of SP / SF / SX, of SU
  Staging st(h, me, dev);
  const double *Cd, *vd, *S0d, *Wd, *Wud; double *Ld, *SPd, *SFd, *SXd, *SUd, *dcd; int32_t *infd;
  st.in("C", C, lead * m * nx * sizeof(double), &Cd);
  st.in("v", v, lead * m * sizeof(double), &vd);
  st.in("Sigma0", Sigma0, lead * nx * nx * sizeof(double), &S0d);
  st.in("W", W, lead * nx * nx * sizeof(double), &Wd);
  st.in("Wu", Wu, lead * nu * nu * sizeof(double), &Wud);
  st.out("L_out", L_out, B * eL * sizeof(double), &Ld);
  st.out("SP_out", SP_out, B * eX * sizeof(double), &SPd);
  st.out("SF_out", SF_out, B * eX * sizeof(double), &SFd);
  st.out("SX", SX, B * eX * sizeof(double), &SXd);
  st.out("SU", SU, B * eU * sizeof(double), &SUd);
  st.out("dcost", dcost, B * sizeof(double), &dcd);
  st.out("info", info, B * sizeof(int32_t), &infd);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi], p0 = per ? b0 : 0;
    const double *pool = (const double *)((const char *)q->dP + offsetof(ProblemDev, pool));
    KfArgs a;
    a.ny = ny;
    a.C = Cd + p0 * m * nx; a.v = vd + p0 * m; a.Sigma0 = S0d + p0 * nx * nx;
    a.W = Wd ? Wd + p0 * nx * nx : nullptr; a.Wu = Wud ? Wud + p0 * nu * nu : nullptr;
    a.L = Ld ? Ld + b0 * eL : nullptr; a.SP = SPd ? SPd + b0 * eX : nullptr; a.SF = SFd ? SFd + b0 * eX : nullptr;
    a.SX = SXd ? SXd + b0 * eX : nullptr; a.SU = SUd ? SUd + b0 * eU : nullptr; a.dcost = dcd ? dcd + b0 : nullptr;
    a.info = infd ? infd + b0 : nullptr;
    a.Qdt = pool + q->P.off_Qdt; a.Rdt = pool + q->P.off_Rdt; a.Qf = pool + q->P.off_Qf;
    a.per_traj = per ? 1 : 0; a.diag = diag ? 1 : 0;
    HIPCHK(plan_kf(sens_stacks(q), a, q->stream));
  }
  return st.finish();
}

int cddp_hip_mpc_run(cddp_hip_handle *h, int steps, int mode, int flags, double *U_applied, double *X_visited, int32_t *iterations, int32_t *status,
                     cddp_hip_stats *stats_sum) {
  if (!h) return fail(-1, "null handle");
  if (steps <= 0) return fail(-1, "cddp_hip_mpc_run: steps must be positive (got %d)", steps);
  for (Inner *q : h->g) { int rc = in_mpc_check(q, mode, flags, false); if (rc) return rc; }   // mode and flags are refused before the first solve, not after it
  for (Inner *q : h->g) if (!q->have_initial) return fail(-1, "cddp_hip_set_initial must be called before cddp_hip_mpc_run");
  if (stats_sum) std::memset(stats_sum, 0, sizeof(*stats_sum));
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (Inner *q : h->g) { int rc = in_mpc_log_begin(q, steps); if (rc) return rc; rc = in_mpc_log(q, steps, -1); if (rc) return rc; }
  int rc_run = 0;
  std::string err_run;
  for (int k = 0; k < steps && !rc_run; ++k) {
    cddp_hip_stats st;
    rc_run = cddp_hip_solve(h, stats_sum ? &st : nullptr);
    if (rc_run) break;
    if (stats_sum) stats_add(stats_sum, st);
    for (Inner *q : h->g) { rc_run = in_mpc_log(q, steps, k); if (rc_run) break; }
    if (rc_run) break;
    rc_run = cddp_hip_mpc_advance(h, mode, flags, nullptr);
  }
  if (rc_run) err_run = g_err;
  // the steps completed so far come back even when a solve failed
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const size_t b0 = (size_t)h->b0[gi];
    int rc = in_mpc_log_fetch(h->g[gi], steps, U_applied ? U_applied + b0 * steps * h->nu : nullptr, X_visited ? X_visited + b0 * (steps + 1) * h->nx : nullptr,
                              iterations ? iterations + b0 * steps : nullptr, status ? status + b0 * steps : nullptr);
    if (rc && !rc_run) return rc;
  }
  if (rc_run) { g_err = err_run; return rc_run; }
  return join_to_user(h);
}

}  // extern "C" (reopened below)

// ================================================================================================================
// Device-resident plant (include/cddp_hip.h "closed loop against a separate plant"; kernels: inst_plant.hip).
// The object owns the derived parameter blocks, the saturation box and the staging buffers of its entry points; a handle it is
// used with is only read (cddp_hip_track_plan) or driven through its own entries (cddp_hip_mpc_run_plant).
// ================================================================================================================
struct cddp_hip_plant {
  PlantDev pd;                       // params / lower / upper point into d_params / d_box
  int B = 0, device = 0;
  hipStream_t stream = nullptr;      // cddp_hip_plant_step
  double *d_params = nullptr, *d_box = nullptr;
  double *d_stage = nullptr;         // [B][nx] batch-major: x_next of an MPC step (what k_mpc_state consumes) / x0 of a tracking rollout
  double *d_io = nullptr;            // cddp_hip_plant_step with host pointers: x | u | w | x_next
  double *d_W = nullptr; size_t W_cap = 0;                       // disturbances of a run / a tracking rollout, uploaded once
  double *d_trX = nullptr, *d_trU = nullptr; int tr_N = -1;      // wave-tiled logs of cddp_hip_track_plan (whole batch)
};

namespace {

// the descriptor checks of cddp_hip_plant_create, in the documented order; none of them looks at a device.
// blocks: the derived parameter blocks, 32 doubles each (one, or one per trajectory)
int plant_check(const cddp_hip_plant_desc *c, int batch, std::vector<double> &blocks) {
  const char *who = "cddp_hip_plant_create";
  if (c->abi_version != CDDP_HIP_ABI_VERSION) return fail(-2, "%s: ABI version mismatch: got %d want %d", who, c->abi_version, CDDP_HIP_ABI_VERSION);
  int mnx = 0, mnu = 0, discrete = 0;
  if (plant_model_dims(c->model, &mnx, &mnu, &discrete)) return fail(-2, "%s: unknown model id %d", who, c->model);
  if (c->integrator < CDDP_HIP_EULER || c->integrator > CDDP_HIP_RK4) return fail(-2, "%s: unknown integrator %d", who, c->integrator);
  const bool lti = c->model == CDDP_HIP_MODEL_LTI;
  if (lti) {
    if (!plant_lti_has(c->nx, c->nu)) return fail(-2, "%s: the LTI plant exists for (nx, nu) = (1, 1) and (2, 1) (got nx = %d, nu = %d)", who, c->nx, c->nu);
  } else if (c->nx != mnx || c->nu != mnu) {
    return fail(-2, "%s: model id %d has nx = %d, nu = %d (got nx = %d, nu = %d)", who, c->model, mnx, mnu, c->nx, c->nu);
  }
  if (c->substeps < 1) return fail(-2, "%s: substeps must be at least 1 (got %d)", who, c->substeps);
  if (c->substeps > 1 && discrete) return fail(-2, "%s: substeps = %d on a discrete plant (model id %d): its step is h = dt by definition", who, c->substeps, c->model);
  if (!(c->dt > 0.0)) return fail(-2, "%s: dt must be positive (got %g)", who, c->dt);
  if ((c->u_lower == nullptr) != (c->u_upper == nullptr)) return fail(-2, "%s: u_lower and u_upper come as a pair (u_%s is NULL)", who, c->u_lower ? "upper" : "lower");
  if (c->u_lower)
    for (int i = 0; i < c->nu; ++i)
      if (!(c->u_lower[i] <= c->u_upper[i])) return fail(-2, "%s: u_lower[%d] = %g is not below u_upper[%d] = %g", who, i, c->u_lower[i], i, c->u_upper[i]);
  if (lti) {
    if (!c->lti_A || !c->lti_B) return fail(-2, "%s: LTI plant needs lti_A and lti_B", who);
    if (c->params_per_trajectory) return fail(-2, "%s: LTI plant: lti_A / lti_B are shared by the batch (params_per_trajectory is not available)", who);
    blocks.assign(32, 0.0);
    for (int i = 0; i < c->nx * c->nx; ++i) blocks[i] = c->lti_A[i];
    for (int i = 0; i < c->nx * c->nu; ++i) blocks[c->nx * c->nx + i] = c->lti_B[i];
    blocks[c->nx * c->nx + c->nx * c->nu] = c->dt;
    return 0;
  }
  if (!c->model_params) return fail(-2, "%s: model_params is NULL", who);
  const int nblk = c->params_per_trajectory ? batch : 1;
  blocks.assign((size_t)nblk * 32, 0.0);
  for (int b = 0; b < nblk; ++b) {
    std::string err;
    double *mp = &blocks[(size_t)b * 32];
    if (cddp_host_model_params(c->model, c->nx, c->nu, c->model_params + (size_t)b * CDDP_HIP_MAX_MODEL_PARAMS, mp, err))
      return c->params_per_trajectory ? fail(-2, "%s: trajectory %d: %s", who, b, err.c_str()) : fail(-2, "%s: %s", who, err.c_str());
    if (c->model == CDDP_HIP_MODEL_CAR) mp[1] = c->dt;        // discrete plants: the timestep travels in the block (flatten())
    if (c->model == CDDP_HIP_MODEL_FORKLIFT) mp[3] = c->dt;
  }
  return 0;
}

int plant_free(cddp_hip_plant *p) {
  hipSetDevice(p->device);
  if (p->stream) { hipStreamSynchronize(p->stream); hipStreamDestroy(p->stream); }
  double *bufs[] = {p->d_params, p->d_box, p->d_stage, p->d_io, p->d_W, p->d_trX, p->d_trU};
  for (double *q : bufs) if (q) hipFree(q);
  delete p;
  return 0;
}

// the refusals the two handle entries share; nothing is launched before they have passed
int plant_fits(const char *who, cddp_hip_handle *h, cddp_hip_plant *p) {
  if (!h) return fail(-1, "%s: null handle", who);
  if (!p) return fail(-1, "%s: null plant", who);
  if (p->pd.nx != h->nx || p->pd.nu != h->nu) return fail(-2, "%s: the plant has nx = %d, nu = %d, the handle nx = %d, nu = %d", who, p->pd.nx, p->pd.nu, h->nx, h->nu);
  if (p->B != h->B) return fail(-2, "%s: the plant was created for a batch of %d, the handle for %d", who, p->B, h->B);
  if (p->device != h->device) return fail(-2, "%s: the plant lives on device %d, the handle on device %d", who, p->device, h->device);
  return 0;
}

// a feedback rollout reads the live slot and the gain stack: refused before the handle has either
int plan_tracked(const char *who, const cddp_hip_handle *h) {
  for (const Inner *q : h->g)
    if (!q->has_plan) return fail(-1, "%s needs a solved handle: there is no plan and no gain stack to track before cddp_hip_solve (or cddp_hip_initialize and cddp_hip_backward)", who);
  return 0;
}

// disturbances: one synchronous upload into the plant's buffer (grown on demand) before anything of the call is enqueued
int plant_upload_W(cddp_hip_plant *p, const double *W, size_t n) {
  if (p->W_cap < n) {
    if (p->d_W) hipFree(p->d_W);
    p->d_W = nullptr; p->W_cap = 0;
    HIPCHK(hipMalloc((void **)&p->d_W, n * sizeof(double)));
    p->W_cap = n;
  }
  HIPCHK(hipMemcpy(p->d_W, W, n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

extern "C" {

int cddp_hip_plant_create(const cddp_hip_plant_desc *desc, int batch, int device, cddp_hip_plant **out) {
  if (!desc || !out) return fail(-1, "cddp_hip_plant_create: null argument");
  if (batch <= 0) return fail(-1, "cddp_hip_plant_create: batch must be positive");
  std::vector<double> blocks;
  { int rc = plant_check(desc, batch, blocks); if (rc) return rc; }
  const int ndev = cddp_hip_device_count();
  if (ndev <= 0) return fail(-20, "no HIP device available: the cddp_hip plant has no CPU fallback (cddp_hip_model_eval is the host plant)");
  if (device < 0 || device >= ndev) return fail(-1, "device %d out of range (%d devices)", device, ndev);
  HIPCHK(hipSetDevice(device));
  cddp_hip_plant *p = new cddp_hip_plant();
  const int nx = desc->nx, nu = desc->nu, Bp = (batch + 63) / 64 * 64, per = desc->params_per_trajectory ? 1 : 0;
  p->B = batch; p->device = device;
  PlantDev &pd = p->pd;
  std::memset(&pd, 0, sizeof(pd));
  pd.model = desc->model; pd.integrator = desc->integrator; pd.substeps = desc->substeps; pd.nx = nx; pd.nu = nu; pd.per_traj = per; pd.Bp = Bp;
  pd.h = desc->dt / (double)desc->substeps;
  std::vector<double> hp;
  if (per) {   // parameter-major [32][Bp]: a wavefront loads entry i of its 64 trajectories as one line
    hp.assign((size_t)32 * Bp, 0.0);
    for (int b = 0; b < batch; ++b) for (int i = 0; i < 32; ++i) hp[(size_t)i * Bp + b] = blocks[(size_t)b * 32 + i];
  } else hp = blocks;
  hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void **)&p->d_params, hp.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(p->d_params, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void **)&p->d_stage, (size_t)batch * nx * sizeof(double));
  if (e == hipSuccess && desc->u_lower) {
    std::vector<double> box((size_t)2 * nu);
    for (int i = 0; i < nu; ++i) { box[i] = desc->u_lower[i]; box[nu + i] = desc->u_upper[i]; }
    e = hipMalloc((void **)&p->d_box, box.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(p->d_box, box.data(), box.size() * sizeof(double), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) { plant_free(p); return fail(-10, "cddp_hip_plant_create: %s", hipGetErrorString(e)); }
  pd.params = p->d_params;
  if (p->d_box) { pd.lower = p->d_box; pd.upper = p->d_box + nu; }
  *out = p;
  return 0;
}

int cddp_hip_plant_destroy(cddp_hip_plant *p) { return p ? plant_free(p) : 0; }

int cddp_hip_plant_step(cddp_hip_plant *p, int flags, const double *x, const double *u, const double *w, double *x_next) {
  if (!p) return fail(-1, "cddp_hip_plant_step: null plant");
  if (!x || !u || !x_next) return fail(-1, "cddp_hip_plant_step: null argument");
  if (flags & ~CDDP_HIP_PLANT_DEVICE) return fail(-2, "cddp_hip_plant_step: unknown flag bits 0x%x", flags);
  HIPCHK(hipSetDevice(p->device));
  const size_t nX = (size_t)p->B * p->pd.nx, nU = (size_t)p->B * p->pd.nu;
  if (flags & CDDP_HIP_PLANT_DEVICE) {
    HIPCHK(plant_launch_step(p->pd, p->B, 0, x, u, w, x_next, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return 0;
  }
  if (!p->d_io) HIPCHK(hipMalloc((void **)&p->d_io, (3 * nX + nU) * sizeof(double)));
  double *dx = p->d_io, *du = dx + nX, *dw = du + nU, *dn = dw + nX;
  HIPCHK(hipMemcpyAsync(dx, x, nX * sizeof(double), hipMemcpyHostToDevice, p->stream));
  HIPCHK(hipMemcpyAsync(du, u, nU * sizeof(double), hipMemcpyHostToDevice, p->stream));
  if (w) HIPCHK(hipMemcpyAsync(dw, w, nX * sizeof(double), hipMemcpyHostToDevice, p->stream));
  HIPCHK(plant_launch_step(p->pd, p->B, 0, dx, du, w ? dw : nullptr, dn, p->stream));
  HIPCHK(hipMemcpyAsync(x_next, dn, nX * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  return 0;
}

int cddp_hip_mpc_run_plant(cddp_hip_handle *h, cddp_hip_plant *plant, int steps, int mode, int flags, const double *W,
                           double *U_applied, double *X_visited, int32_t *iterations, int32_t *status, cddp_hip_stats *stats_sum) {
  { int rc = plant_fits("cddp_hip_mpc_run_plant", h, plant); if (rc) return rc; }
  if (steps <= 0) return fail(-1, "cddp_hip_mpc_run_plant: steps must be positive (got %d)", steps);
  for (Inner *q : h->g) { int rc = in_mpc_check(q, mode, flags, false); if (rc) return rc; }
  for (Inner *q : h->g) if (!q->have_initial) return fail(-1, "cddp_hip_set_initial must be called before cddp_hip_mpc_run_plant");
  HIPCHK(hipSetDevice(h->device));
  const size_t nx = (size_t)h->nx, nu = (size_t)h->nu;
  if (W) { int rc = plant_upload_W(plant, W, (size_t)h->B * steps * nx); if (rc) return rc; }
  if (stats_sum) std::memset(stats_sum, 0, sizeof(*stats_sum));
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (Inner *q : h->g) { int rc = in_mpc_log_begin(q, steps); if (rc) return rc; rc = in_mpc_log(q, steps, -1); if (rc) return rc; }
  const int aflags = flags | CDDP_HIP_MPC_X_DEVICE;
  int rc_run = 0;
  std::string err_run;
  for (int k = 0; k < steps && !rc_run; ++k) {
    cddp_hip_stats st;
    rc_run = cddp_hip_solve(h, stats_sum ? &st : nullptr);
    if (rc_run) break;
    if (stats_sum) stats_add(stats_sum, st);
    // per group, on its stream: iterations and status (and the model's own head, which the plant's rows then replace), the plant on row 0
    // of the live slot, the advance from the staged x_next -- no synchronisation, the next solve is ordered behind them
    for (Inner *q : h->g) { rc_run = in_mpc_check(q, mode, aflags); if (rc_run) break; }
    for (size_t gi = 0; gi < h->g.size() && !rc_run; ++gi) {
      Inner *q = h->g[gi];
      const size_t b0 = (size_t)h->b0[gi];
      rc_run = in_mpc_log(q, steps, k);
      if (rc_run) break;
      double *stage = plant->d_stage + b0 * nx;
      hipError_t e = plant_launch_head(plant->pd, q->d, (int)b0, W ? plant->d_W + b0 * steps * nx : nullptr, steps, k, stage, q->d_log_u, q->d_log_x, q->stream);
      if (e != hipSuccess) { rc_run = fail(-10, "cddp_hip_mpc_run_plant: plant step: %s", hipGetErrorString(e)); break; }
      rc_run = in_mpc_advance(q, mode, aflags, stage, false);
    }
  }
  if (rc_run) err_run = g_err;
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const size_t b0 = (size_t)h->b0[gi];
    int rc = in_mpc_log_fetch(h->g[gi], steps, U_applied ? U_applied + b0 * steps * nu : nullptr, X_visited ? X_visited + b0 * (steps + 1) * nx : nullptr,
                              iterations ? iterations + b0 * steps : nullptr, status ? status + b0 * steps : nullptr);
    if (rc && !rc_run) return rc;
  }
  if (rc_run) { g_err = err_run; return rc_run; }
  return join_to_user(h);
}

int cddp_hip_track_plan(cddp_hip_handle *h, cddp_hip_plant *plant, const double *x0, const double *W, double *X_out, double *U_out) {
  { int rc = plant_fits("cddp_hip_track_plan", h, plant); if (rc) return rc; }
  { int rc = plan_tracked("cddp_hip_track_plan", h); if (rc) return rc; }
  HIPCHK(hipSetDevice(h->device));
  const int N = h->N, nx = h->nx, nu = h->nu, Bp = plant->pd.Bp, NBlog = Bp / 64;
  const size_t nXl = (size_t)(N + 1) * nx * Bp, nUl = (size_t)N * nu * Bp;
  if (plant->tr_N != N) {
    if (plant->d_trX) hipFree(plant->d_trX);
    if (plant->d_trU) hipFree(plant->d_trU);
    plant->d_trX = plant->d_trU = nullptr; plant->tr_N = -1;
    HIPCHK(hipMalloc((void **)&plant->d_trX, nXl * sizeof(double)));
    HIPCHK(hipMalloc((void **)&plant->d_trU, nUl * sizeof(double)));
    plant->tr_N = N;
  }
  if (W) { int rc = plant_upload_W(plant, W, (size_t)h->B * N * nx); if (rc) return rc; }
  if (x0) HIPCHK(hipMemcpy(plant->d_stage, x0, (size_t)h->B * nx * sizeof(double), hipMemcpyHostToDevice));
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    HIPCHK(plant_launch_track(plant->pd, q->d, (int)b0, x0 ? plant->d_stage + b0 * nx : nullptr, W ? plant->d_W + b0 * N * nx : nullptr,
                              plant->d_trX, plant->d_trU, NBlog, q->stream));
  }
  for (Inner *q : h->g) HIPCHK(hipStreamSynchronize(q->stream));
  // the logs are wave-tiled stacks of the whole batch: one copy each, un-tiled as the getters un-tile theirs
  std::vector<double> buf;
  if (X_out) { buf.resize(nXl); HIPCHK(hipMemcpy(buf.data(), plant->d_trX, nXl * sizeof(double), hipMemcpyDeviceToHost)); from_soa(buf.data(), X_out, h->B, Bp, N + 1, nx); }
  if (U_out) { buf.resize(nUl); HIPCHK(hipMemcpy(buf.data(), plant->d_trU, nUl * sizeof(double), hipMemcpyDeviceToHost)); from_soa(buf.data(), U_out, h->B, Bp, N, nu); }
  return join_to_user(h);
}

// ---- scoring candidate control sequences (inst_score.hip) and seeding from the best of them ----
int cddp_hip_score_rollouts(cddp_hip_handle *h, cddp_hip_plant *plant, int flags, int ncand, const double *x0, const double *U,
                            double *cost, double *viol, double *X_out, double *U_out) {
  static const char *const me = "cddp_hip_score_rollouts";
  const int known = CDDP_HIP_SCORE_DEVICE | CDDP_HIP_SCORE_FEEDBACK | CDDP_HIP_SCORE_X0_PER_CANDIDATE;
  if (!h) return fail(-1, "%s: null handle", me);
  if (flags & ~known) return fail(-2, "%s: unknown flag bits 0x%x", me, (unsigned)(flags & ~known));
  if (ncand < 1) return fail(-2, "%s: ncand = %d, at least one candidate is needed", me, ncand);
  if (!cost) return fail(-1, "%s: null cost pointer", me);
  const bool dev = (flags & CDDP_HIP_SCORE_DEVICE) != 0, fb = (flags & CDDP_HIP_SCORE_FEEDBACK) != 0, xpc = (flags & CDDP_HIP_SCORE_X0_PER_CANDIDATE) != 0;
  if (!U && !fb) return fail(-1, "%s: U is NULL without CDDP_HIP_SCORE_FEEDBACK: there is nothing to roll out", me);
  if (xpc && !x0) return fail(-1, "%s: CDDP_HIP_SCORE_X0_PER_CANDIDATE with a NULL x0", me);
  if (fb) { int rc = plan_tracked(me, h); if (rc) return rc; }
  if (!x0) for (const Inner *q : h->g) if (!q->has_plan) return fail(-1, "%s: x0 is NULL and the handle has no plan whose row 0 could stand in", me);
  if (plant) { int rc = plant_fits(me, h, plant); if (rc) return rc; }
  const size_t B = (size_t)h->B, S = (size_t)ncand, nx = (size_t)h->nx, nu = (size_t)h->nu, N = (size_t)h->N;
  if (((size_t)((h->B + 63) / 64 * 64) * S + 63) / 64 > 0x7fffffffull) return fail(-2, "%s: batch * ncand = %zu exceeds what one launch holds", me, B * S);
  HIPCHK(hipSetDevice(h->device));
  const size_t n0 = xpc ? S * nx : nx, nU = S * N * nu, nX = S * (N + 1) * nx;   // per trajectory
  Staging st(h, me, dev);
  const double *x0d, *Ud;
  double *costd, *viold, *Xd, *Uod;
  st.in("x0", x0, B * n0 * sizeof(double), &x0d);
  st.in("U", U, B * nU * sizeof(double), &Ud);
  st.out("cost", cost, B * S * sizeof(double), &costd);
  st.out("viol", viol, B * S * sizeof(double), &viold);
  st.out("X_out", X_out, B * nX * sizeof(double), &Xd);
  st.out("U_out", U_out, B * nU * sizeof(double), &Uod);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    const PlantDev pd = plant ? plant->pd : own_model_plant(q);
    ScoreArgs a;
    a.S = ncand; a.b0 = (int)b0; a.feedback = fb ? 1 : 0; a.x0_per_cand = xpc ? 1 : 0;
    a.x0 = x0d ? x0d + b0 * n0 : nullptr; a.U = Ud ? Ud + b0 * nU : nullptr;
    a.cost = costd + b0 * S; a.viol = viold ? viold + b0 * S : nullptr;
    a.X_out = Xd ? Xd + b0 * nX : nullptr; a.U_out = Uod ? Uod + b0 * nU : nullptr;
    { int rc = plant_launch_rc(score_launch(pd, q->d, a, q->stream), me, "scoring", pd); if (rc) return rc; }
  }
  return st.finish();
}

int cddp_hip_seed_best(cddp_hip_handle *h, int flags, int ncand, const double *x0, const double *U, const double *cost, const double *viol,
                       double viol_tol, int32_t *winner) {
  static const char *const me = "cddp_hip_seed_best";
  if (!h) return fail(-1, "%s: null handle", me);
  if (flags & ~CDDP_HIP_SCORE_DEVICE) return fail(-2, "%s: unknown flag bits 0x%x (CDDP_HIP_SCORE_DEVICE is the only flag)", me, (unsigned)(flags & ~CDDP_HIP_SCORE_DEVICE));
  if (ncand < 1) return fail(-2, "%s: ncand = %d, at least one candidate is needed", me, ncand);
  if (!U) return fail(-1, "%s: null U pointer", me);
  if (!cost) return fail(-1, "%s: null cost pointer", me);
  if (!x0) for (const Inner *q : h->g) if (!q->have_initial) return fail(-1, "%s: x0 is NULL and the handle has no initial state to keep (cddp_hip_set_initial)", me);
  HIPCHK(hipSetDevice(h->device));
  const bool dev = (flags & CDDP_HIP_SCORE_DEVICE) != 0;
  const size_t B = (size_t)h->B, S = (size_t)ncand, nx = (size_t)h->nx, nU = (size_t)h->N * h->nu;
  Staging st(h, me, dev);
  const double *x0d, *Ud, *costd, *viold;
  st.in("x0", x0, B * nx * sizeof(double), &x0d);
  st.in("U", U, B * S * nU * sizeof(double), &Ud);
  st.in("cost", cost, B * S * sizeof(double), &costd);
  st.in("viol", viol, B * S * sizeof(double), &viold);
  st.out_via("winner", winner, B * sizeof(int32_t), &h->d_winner);   // the selection always writes the handle's own winner[B], both forms
  { int rc = st.begin(); if (rc) return rc; }
  if (!h->d_winner) HIPCHK(hipMalloc((void **)&h->d_winner, B * sizeof(int32_t)));
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    int32_t *w = h->d_winner + b0;
    score_select_launch(q->d.B, ncand, costd + b0 * S, viold ? viold + b0 * S : nullptr, viol_tol, w, q->stream);
    // the seed exactly as cddp_hip_set_initial_device(x0, U[:, winner], NULL) tiles it; only the gather index is new
    if (x0d) io_tile(nullptr, x0d + b0 * nx, q->d.B, q->d.NB, h->N + 1, h->nx, q->d_Xinit, q->stream);
    io_tile(Ud + b0 * S * nU, nullptr, q->d.B, q->d.NB, h->N, h->nu, q->d_Uinit, q->stream, w, ncand);
    if (winner && dev) HIPCHK(hipMemcpyAsync(winner + b0, w, (size_t)q->d.B * sizeof(int32_t), hipMemcpyDeviceToDevice, q->stream));
    mark_seeded(q);
  }
  return st.finish();
}

// ---- sampling-based plan refinement (inst_mppi.hip): candidates drawn in the kernels, weights and blend of csrc/mppi.hpp ----
// The refusals the three entries share, in the order of the header: those that read nothing of the handle first.  Fills the draw.
static int mppi_refuse(const char *me, const cddp_hip_handle *h, int flags, int known, const cddp_hip_mppi_desc *desc, MppiDraw *a) {
  if (!h) return fail(-1, "%s: null handle", me);
  if (flags & ~known) return fail(-2, "%s: unknown flag bits 0x%x", me, (unsigned)(flags & ~known));
  if (!desc) return fail(-1, "%s: null descriptor", me);
  if (desc->iters < 1) return fail(-2, "%s: iters = %d, at least one round is needed", me, desc->iters);
  if (desc->ncand < 1) return fail(-2, "%s: ncand = %d, at least one candidate is needed", me, desc->ncand);
  if (!(desc->lambda > 0.0) || !std::isfinite(desc->lambda)) return fail(-2, "%s: lambda = %g is not positive and finite", me, desc->lambda);
  if (desc->viol_tol != desc->viol_tol) return fail(-2, "%s: viol_tol is NaN", me);
  if (!desc->sigma) return fail(-1, "%s: null sigma pointer", me);
  if ((desc->u_lower == nullptr) != (desc->u_upper == nullptr)) return fail(-2, "%s: half a box: u_lower and u_upper are both set or both NULL", me);
  const int nu = h->nu;
  if (nu > kMppiMaxNu) return fail(-3, "%s: nu = %d, the sampling kernels hold at most %d controls", me, nu, kMppiMaxNu);
  std::memset(a, 0, sizeof(*a));
  for (int i = 0; i < nu; ++i) {
    if (!(desc->sigma[i] > 0.0) || !std::isfinite(desc->sigma[i])) return fail(-2, "%s: sigma[%d] = %g is not positive and finite", me, i, desc->sigma[i]);
    a->sigma[i] = desc->sigma[i];
    if (desc->u_lower) {
      if (!(desc->u_lower[i] <= desc->u_upper[i])) return fail(-2, "%s: u_lower[%d] = %g exceeds u_upper[%d] = %g", me, i, desc->u_lower[i], i, desc->u_upper[i]);
      a->lower[i] = desc->u_lower[i]; a->upper[i] = desc->u_upper[i];
    }
  }
  a->seed = desc->seed; a->stream = desc->stream; a->S = desc->ncand; a->keep_mean = desc->keep_mean ? 1 : 0; a->box = desc->u_lower ? 1 : 0;
  return 0;
}

static int mppi_needs_plan_U(const char *me, const cddp_hip_handle *h) {
  for (const Inner *q : h->g) if (!q->has_plan) return fail(-1, "%s: U_mean is NULL and the handle has no plan whose U could stand in", me);
  return 0;
}

// the live plan's U of one group, batch-major, as cddp_hip_get_field_device(CDDP_HIP_FIELD_U) writes it
static void mppi_plan_U(const cddp_hip_handle *h, const Inner *q, double *out) {
  io_untile(cddp_io::kSlotted, q->d.U, q->d.cur, q->d.planeU, q->d.B, q->d.NB, h->N, h->nu, out, q->stream);
}

int cddp_hip_sample_controls(cddp_hip_handle *h, int flags, const cddp_hip_mppi_desc *desc, const double *U_mean, double *U_out) {
  static const char *const me = "cddp_hip_sample_controls";
  MppiDraw a;
  { int rc = mppi_refuse(me, h, flags, CDDP_HIP_SCORE_DEVICE, desc, &a); if (rc) return rc; }
  if (!U_out) return fail(-1, "%s: null U_out pointer", me);
  if (!U_mean) { int rc = mppi_needs_plan_U(me, h); if (rc) return rc; }
  const bool dev = (flags & CDDP_HIP_SCORE_DEVICE) != 0;
  const size_t B = (size_t)h->B, S = (size_t)desc->ncand, nU = (size_t)h->N * h->nu;
  if ((B * S * ((nU + 1) / 2) + 255) / 256 > 0x7fffffffull) return fail(-2, "%s: batch * ncand * N * nu / 2 = %zu lanes exceed what one launch holds", me, B * S * ((nU + 1) / 2));
  HIPCHK(hipSetDevice(h->device));
  Staging st(h, me, dev);
  const double *meand;
  double *outd;
  if (U_mean) st.in("U_mean", U_mean, B * nU * sizeof(double), &meand);
  else st.scratch(B * nU * sizeof(double), &meand);   // the plan's U, un-tiled per group below
  st.out("U_out", U_out, B * S * nU * sizeof(double), &outd);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    if (!U_mean) mppi_plan_U(h, q, const_cast<double *>(meand) + b0 * nU);
    a.b0 = (int)b0;
    HIPCHK(mppi_sample_launch(a, q->d.B, h->N, h->nu, meand + b0 * nU, outd + b0 * S * nU, q->stream));
  }
  return st.finish();
}

int cddp_hip_mppi_blend(cddp_hip_handle *h, int flags, const cddp_hip_mppi_desc *desc, const double *U_mean, const double *U_cand, const double *cost,
                        const double *viol, double *U_out, double *stats) {
  static const char *const me = "cddp_hip_mppi_blend";
  MppiDraw a;
  { int rc = mppi_refuse(me, h, flags, CDDP_HIP_SCORE_DEVICE, desc, &a); if (rc) return rc; }
  if (!U_mean) return fail(-1, "%s: null U_mean pointer", me);
  if (!U_cand) return fail(-1, "%s: null U_cand pointer", me);
  if (!cost) return fail(-1, "%s: null cost pointer", me);
  if (!U_out) return fail(-1, "%s: null U_out pointer", me);
  const bool dev = (flags & CDDP_HIP_SCORE_DEVICE) != 0;
  const size_t B = (size_t)h->B, S = (size_t)desc->ncand, nU = (size_t)h->N * h->nu;
  HIPCHK(hipSetDevice(h->device));
  Staging st(h, me, dev);
  const double *meand, *candd, *costd, *viold;
  double *outd, *wd, *std_;
  st.scratch(B * S * sizeof(double), &wd);      // the weights [B][S]
  st.scratch(B * 3 * sizeof(double), &std_);    // the statistics [B][3], wherever the caller wants them
  st.in("U_mean", U_mean, B * nU * sizeof(double), &meand);
  st.in("U_cand", U_cand, B * S * nU * sizeof(double), &candd);
  st.in("cost", cost, B * S * sizeof(double), &costd);
  st.in("viol", viol, B * S * sizeof(double), &viold);
  st.out("U_out", U_out, B * nU * sizeof(double), &outd);
  st.out_via("stats", stats, B * 3 * sizeof(double), &std_);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    a.b0 = (int)b0;
    mppi_weights_launch(q->d.B, desc->ncand, costd + b0 * S, viold ? viold + b0 * S : nullptr, desc->viol_tol, desc->lambda, wd + b0 * S, std_ + b0 * 3, q->stream);
    HIPCHK(mppi_blend_launch(a, q->d.B, h->N, h->nu, meand + b0 * nU, candd + b0 * S * nU, wd + b0 * S, std_ + b0 * 3, outd + b0 * nU, q->stream));
    if (dev && stats) HIPCHK(hipMemcpyAsync(stats + b0 * 3, std_ + b0 * 3, (size_t)q->d.B * 3 * sizeof(double), hipMemcpyDeviceToDevice, q->stream));
  }
  return st.finish();
}

int cddp_hip_mppi_refine(cddp_hip_handle *h, cddp_hip_plant *plant, int flags, const cddp_hip_mppi_desc *desc, const double *x0, const double *U_mean,
                         double *U_out, double *cost_out, double *viol_out, double *stats) {
  static const char *const me = "cddp_hip_mppi_refine";
  MppiDraw a;
  { int rc = mppi_refuse(me, h, flags, CDDP_HIP_SCORE_DEVICE | CDDP_HIP_MPPI_SEED, desc, &a); if (rc) return rc; }
  if (!U_out) return fail(-1, "%s: null U_out pointer", me);
  const bool dev = (flags & CDDP_HIP_SCORE_DEVICE) != 0, seed = (flags & CDDP_HIP_MPPI_SEED) != 0;
  if (!x0) for (const Inner *q : h->g) if (!q->has_plan) return fail(-1, "%s: x0 is NULL and the handle has no plan whose row 0 could stand in", me);
  if (!x0 && seed) for (const Inner *q : h->g) if (!q->have_initial) return fail(-1, "%s: x0 is NULL and the handle has no initial state to keep (cddp_hip_set_initial)", me);
  if (!U_mean) { int rc = mppi_needs_plan_U(me, h); if (rc) return rc; }
  if (plant) { int rc = plant_fits(me, h, plant); if (rc) return rc; }
  const size_t B = (size_t)h->B, S = (size_t)desc->ncand, nx = (size_t)h->nx, nU = (size_t)h->N * h->nu;
  if (((size_t)((h->B + 63) / 64 * 64) * S + 63) / 64 > 0x7fffffffull) return fail(-2, "%s: batch * ncand = %zu exceeds what one launch holds", me, B * S);
  HIPCHK(hipSetDevice(h->device));
  // internal blocks: the mean ping-ponged between two [B][N][nu] buffers, cost | viol | w [B][S], stats [B][3]; the results lie in them in
  // both forms (the device form copies them out per group below)
  Staging st(h, me, dev);
  double *mean[2], *costd, *viold, *wd, *std_;
  const double *x0d;
  for (int k = 0; k < 2; ++k) st.scratch(B * nU * sizeof(double), &mean[k]);
  for (double **p : {&costd, &viold, &wd}) st.scratch(B * S * sizeof(double), p);
  st.scratch(B * 3 * sizeof(double), &std_);
  st.in("x0", x0, B * nx * sizeof(double), &x0d);
  st.in_via("U_mean", U_mean, B * nU * sizeof(double), &mean[0]);
  st.out_via("U_out", U_out, B * nU * sizeof(double), &mean[desc->iters & 1]);   // where the mean lies after the last round
  st.out_via("cost_out", cost_out, B * S * sizeof(double), &costd);
  st.out_via("viol_out", viol_out, B * S * sizeof(double), &viold);
  st.out_via("stats", stats, B * 3 * sizeof(double), &std_);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  const double *last = mean[desc->iters & 1];
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi], Bg = (size_t)q->d.B;
    const PlantDev pd = plant ? plant->pd : own_model_plant(q);
    if (!U_mean) mppi_plan_U(h, q, mean[0] + b0 * nU);
    else if (dev) HIPCHK(hipMemcpyAsync(mean[0] + b0 * nU, U_mean + b0 * nU, Bg * nU * sizeof(double), hipMemcpyDeviceToDevice, q->stream));
    a.b0 = (int)b0;
    for (int k = 0; k < desc->iters; ++k) {
      const double *in = mean[k & 1] + b0 * nU;
      double *out = mean[(k + 1) & 1] + b0 * nU;
      a.stream = desc->stream + (uint32_t)k;
      { int rc = plant_launch_rc(mppi_score_launch(pd, q->d, a, x0d ? x0d + b0 * nx : nullptr, in, costd + b0 * S, viold + b0 * S, q->stream), me, "scoring", pd); if (rc) return rc; }
      mppi_weights_launch(q->d.B, desc->ncand, costd + b0 * S, viold + b0 * S, desc->viol_tol, desc->lambda, wd + b0 * S, std_ + b0 * 3, q->stream);
      HIPCHK(mppi_blend_launch(a, q->d.B, h->N, h->nu, in, nullptr, wd + b0 * S, std_ + b0 * 3, out, q->stream));
    }
    if (seed) {   // exactly as cddp_hip_set_initial_device(x0, U_out, NULL) tiles it
      if (x0d) io_tile(nullptr, x0d + b0 * nx, q->d.B, q->d.NB, h->N + 1, h->nx, q->d_Xinit, q->stream);
      io_tile(last + b0 * nU, nullptr, q->d.B, q->d.NB, h->N, h->nu, q->d_Uinit, q->stream);
      mark_seeded(q);
    }
    if (dev) {
      HIPCHK(hipMemcpyAsync(U_out + b0 * nU, last + b0 * nU, Bg * nU * sizeof(double), hipMemcpyDeviceToDevice, q->stream));
      if (cost_out) HIPCHK(hipMemcpyAsync(cost_out + b0 * S, costd + b0 * S, Bg * S * sizeof(double), hipMemcpyDeviceToDevice, q->stream));
      if (viol_out) HIPCHK(hipMemcpyAsync(viol_out + b0 * S, viold + b0 * S, Bg * S * sizeof(double), hipMemcpyDeviceToDevice, q->stream));
      if (stats) HIPCHK(hipMemcpyAsync(stats + b0 * 3, std_ + b0 * 3, Bg * 3 * sizeof(double), hipMemcpyDeviceToDevice, q->stream));
    }
  }
  return st.finish();
}

// ---- Monte-Carlo evaluation of a solved plan under noise (inst_mc.hip): noise drawn in the kernel, sums over the samples of csrc/plan_mc.hpp ----
// The refusals the two entries share, in the order of the header: those that read nothing of the handle first.  Fills the draw and the factors.
static int mc_refuse(const char *me, const cddp_hip_handle *h, int flags, int known, const cddp_hip_mc_desc *desc, McArgs *a, McFactors *f) {
  if (!h) return fail(-1, "%s: null handle", me);
  if (!desc) return fail(-1, "%s: null descriptor", me);
  if (flags & ~known) return fail(-2, "%s: unknown flag bits 0x%x", me, (unsigned)(flags & ~known));
  if (desc->nsamp < 1) return fail(-2, "%s: nsamp = %d, at least one sample is needed", me, desc->nsamp);
  if (desc->nsamp > kMcMaxSamples) return fail(-2, "%s: nsamp = %d, one workgroup holds at most %d samples of a trajectory", me, desc->nsamp, kMcMaxSamples);
  if (desc->viol_tol != desc->viol_tol) return fail(-2, "%s: viol_tol is NaN", me);
  const int nx = h->nx, nu = h->nu;
  if (nx > kMcMaxNx || nu > kMcMaxNu) return fail(-3, "%s: nx = %d, nu = %d, the sampling kernels hold at most %d states and %d controls", me, nx, nu, kMcMaxNx, kMcMaxNu);
  std::memset(a, 0, sizeof(*a));
  std::memset(f, 0, sizeof(*f));
  const struct { const double *L; int n; double *out; const char *name; } fac[3] = {{desc->L0, nx, f->l0, "L0"}, {desc->Lw, nx, f->lw, "Lw"}, {desc->Lu, nu, f->lu, "Lu"}};
  for (const auto &m : fac) {
    if (!m.L) continue;
    for (int i = 0; i < m.n; ++i)
      for (int j = 0; j <= i; ++j) {
        const double v = m.L[i * m.n + j];
        if (!std::isfinite(v)) return fail(-2, "%s: %s[%d][%d] = %g is not finite", me, m.name, i, j, v);
        m.out[i * (i + 1) / 2 + j] = v;
      }
  }
  a->seed = desc->seed; a->stream = desc->stream; a->S = desc->nsamp; a->keep_nominal = desc->keep_nominal ? 1 : 0; a->viol_tol = desc->viol_tol;
  a->have0 = desc->L0 ? 1 : 0; a->havew = desc->Lw ? 1 : 0; a->haveu = desc->Lu ? 1 : 0;
  return 0;
}

int cddp_hip_mc_sample_noise(cddp_hip_handle *h, int flags, const cddp_hip_mc_desc *desc, double *Z0, double *E, double *Wn) {
  static const char *const me = "cddp_hip_mc_sample_noise";
  McArgs a;
  McFactors f;
  { int rc = mc_refuse(me, h, flags, CDDP_HIP_MC_DEVICE, desc, &a, &f); if (rc) return rc; }
  if (!Z0 && !E && !Wn) return fail(-1, "%s: Z0, E and Wn are all NULL: there is nothing to write", me);
  const bool dev = (flags & CDDP_HIP_MC_DEVICE) != 0;
  const size_t B = (size_t)h->B, S = (size_t)desc->nsamp, nx = (size_t)h->nx, nu = (size_t)h->nu, N = (size_t)h->N;
  const size_t n0 = S * nx, nE = S * N * nu, nW = S * N * nx;   // per trajectory
  HIPCHK(hipSetDevice(h->device));
  Staging st(h, me, dev);
  double *Zd, *Ed, *Wd;
  st.out("Z0", Z0, B * n0 * sizeof(double), &Zd);
  st.out("E", E, B * nE * sizeof(double), &Ed);
  st.out("Wn", Wn, B * nW * sizeof(double), &Wd);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    a.b0 = (int)b0;
    HIPCHK(mc_noise_launch(a, f, q->d.B, h->N, h->nx, h->nu, Zd ? Zd + b0 * n0 : nullptr, Ed ? Ed + b0 * nE : nullptr, Wd ? Wd + b0 * nW : nullptr, q->stream));
  }
  return st.finish();
}

int cddp_hip_plan_montecarlo(cddp_hip_handle *h, cddp_hip_plant *plant, int flags, const cddp_hip_mc_desc *desc, const double *x0, double *cost, double *viol,
                             double *stats, int32_t *nviol_step, double *dXmean, double *SX, double *dUmean, double *SU, double *X_out, double *U_out) {
  static const char *const me = "cddp_hip_plan_montecarlo";
  McArgs a;
  McFactors f;
  { int rc = mc_refuse(me, h, flags, CDDP_HIP_MC_DEVICE | CDDP_HIP_MC_DIAG, desc, &a, &f); if (rc) return rc; }
  if (!cost && !viol && !stats && !nviol_step && !dXmean && !SX && !dUmean && !SU && !X_out && !U_out) return fail(-1, "%s: every output is NULL: there is nothing to write", me);
  if (h->g[0]->P.solver == CDDP_HIP_SOLVER_MSIPDDP)
    return fail(-1, "%s: not for an MSIPDDP handle: its plan carries defects and its gains belong to the gap-closing recursion, so they are no tracking policy", me);
  { int rc = plan_tracked(me, h); if (rc) return rc; }
  if (plant) { int rc = plant_fits(me, h, plant); if (rc) return rc; }
  const bool dev = (flags & CDDP_HIP_MC_DEVICE) != 0, diag = (flags & CDDP_HIP_MC_DIAG) != 0;
  a.diag = diag ? 1 : 0;
  const size_t B = (size_t)h->B, S = (size_t)desc->nsamp, nx = (size_t)h->nx, nu = (size_t)h->nu, N = (size_t)h->N;
  // doubles per trajectory of every double output, in the order of the argument list
  const size_t nSX = (N + 1) * nx * (diag ? 1 : nx), nSU = N * nu * (diag ? 1 : nu), nXo = S * (N + 1) * nx, nUo = S * N * nu, nCnt = N + 1;
  double *outs[9] = {cost, viol, stats, dXmean, SX, dUmean, SU, X_out, U_out};
  const size_t per[9] = {S, S, 8, (N + 1) * nx, nSX, N * nu, nSU, nXo, nUo};
  static const char *const names[9] = {"cost", "viol", "stats", "dXmean", "SX", "dUmean", "SU", "X_out", "U_out"};
  HIPCHK(hipSetDevice(h->device));
  Staging st(h, me, dev);
  const double *x0d;
  double *od[9];
  int32_t *cntd;
  st.in("x0", x0, B * nx * sizeof(double), &x0d);
  for (int i = 0; i < 9; ++i) st.out(names[i], outs[i], B * per[i] * sizeof(double), &od[i]);
  st.out("nviol_step", nviol_step, B * nCnt * sizeof(int32_t), &cntd);
  { int rc = st.begin(); if (rc) return rc; }
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    const PlantDev pd = plant ? plant->pd : own_model_plant(q);
    a.b0 = (int)b0;
    a.x0 = x0d ? x0d + b0 * nx : nullptr;
    double *go[9];
    for (int i = 0; i < 9; ++i) go[i] = od[i] ? od[i] + b0 * per[i] : nullptr;
    a.cost = go[0]; a.viol = go[1]; a.stats = go[2]; a.dXmean = go[3]; a.SX = go[4]; a.dUmean = go[5]; a.SU = go[6]; a.X_out = go[7]; a.U_out = go[8];
    a.nviol_step = cntd ? cntd + b0 * nCnt : nullptr;
    { int rc = plant_launch_rc(mc_launch(pd, q->d, a, f, q->stream), me, "sampling", pd); if (rc) return rc; }
  }
  return st.finish();
}


// ---- Monte-Carlo evaluation under output feedback (inst_mcof.hip): the entries above with the estimator of csrc/plan_mcof.hpp in every lane ----
// The refusals of the sensor model, after mc_refuse's: fills sd[r] = sqrt(v[r]) (the host's sqrt is correctly rounded).
static int mcof_refuse(const char *me, const cddp_hip_mcof_desc *desc, int nx, bool need_C, double *sd) {
  if (desc->ny < 1 || desc->ny > CDDP_HIP_KF_MAX_NY) return fail(-2, "%s: ny = %d, 1 .. %d measurement rows are expected", me, desc->ny, CDDP_HIP_KF_MAX_NY);
  if (need_C && !desc->C) return fail(-1, "%s: null C pointer", me);
  if (!desc->v) return fail(-1, "%s: null v pointer", me);
  for (int r = 0; r < desc->ny; ++r) {
    if (!std::isfinite(desc->v[r]) || !(desc->v[r] > 0.0)) return fail(-2, "%s: v[%d] = %g is not finite and > 0 (a measurement variance)", me, r, desc->v[r]);
    sd[r] = std::sqrt(desc->v[r]);
  }
  if (need_C && !ref_all_finite(desc->C, (size_t)desc->ny * (size_t)nx)) return fail(-2, "%s: C holds a non-finite value", me);
  return 0;
}

int cddp_hip_mc_sample_meas_noise(cddp_hip_handle *h, int flags, const cddp_hip_mcof_desc *desc, double *Yn) {
  static const char *const me = "cddp_hip_mc_sample_meas_noise";
  McArgs a;
  McFactors f;
  double sd[CDDP_HIP_KF_MAX_NY];
  { int rc = mc_refuse(me, h, flags, CDDP_HIP_MC_DEVICE, desc ? &desc->mc : nullptr, &a, &f); if (rc) return rc; }
  { int rc = mcof_refuse(me, desc, h->nx, false, sd); if (rc) return rc; }
  if (!Yn) return fail(-1, "%s: Yn is NULL: there is nothing to write", me);
  const bool dev = (flags & CDDP_HIP_MC_DEVICE) != 0;
  const size_t B = (size_t)h->B, S = (size_t)desc->mc.nsamp, ny = (size_t)desc->ny, nY = S * (size_t)(h->N + 1) * ny;   // per trajectory
  HIPCHK(hipSetDevice(h->device));
  Staging st(h, me, dev);
  double *Yd, *sdd;
  st.scratch(ny * sizeof(double), &sdd);
  st.out("Yn", Yn, B * nY * sizeof(double), &Yd);
  { int rc = st.begin(); if (rc) return rc; }
  HIPCHK(hipMemcpy(sdd, sd, ny * sizeof(double), hipMemcpyHostToDevice));
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    a.b0 = (int)b0;
    HIPCHK(mcof_noise_launch(a, q->d.B, h->N, h->nx, h->nu, desc->ny, sdd, Yd + b0 * nY, q->stream));
  }
  return st.finish();
}

int cddp_hip_plan_montecarlo_of(cddp_hip_handle *h, cddp_hip_plant *plant, int flags, const cddp_hip_mcof_desc *desc, const double *x0, const double *L,
                                double *cost, double *viol, double *stats, int32_t *nviol_step, double *dXmean, double *SX, double *dUmean, double *SU,
                                double *X_out, double *U_out, double *dEmean, double *SE, double *Xh_out) {
  static const char *const me = "cddp_hip_plan_montecarlo_of";
  McArgs a;
  McFactors f;
  double sd[CDDP_HIP_KF_MAX_NY];
  { int rc = mc_refuse(me, h, flags, CDDP_HIP_MC_DEVICE | CDDP_HIP_MC_DIAG, desc ? &desc->mc : nullptr, &a, &f); if (rc) return rc; }
  { int rc = mcof_refuse(me, desc, h->nx, true, sd); if (rc) return rc; }
  if (!L) return fail(-1, "%s: null L pointer", me);
  if (!cost && !viol && !stats && !nviol_step && !dXmean && !SX && !dUmean && !SU && !X_out && !U_out && !dEmean && !SE && !Xh_out)
    return fail(-1, "%s: every output is NULL: there is nothing to write", me);
  { int rc = sens_refuse_handle(me, h); if (rc) return rc; }   // MSIPDDP, never swept: A_t and B_t are read
  { int rc = plan_tracked(me, h); if (rc) return rc; }
  if (plant) { int rc = plant_fits(me, h, plant); if (rc) return rc; }
  const bool dev = (flags & CDDP_HIP_MC_DEVICE) != 0, diag = (flags & CDDP_HIP_MC_DIAG) != 0;
  a.diag = diag ? 1 : 0;
  const size_t B = (size_t)h->B, S = (size_t)desc->mc.nsamp, nx = (size_t)h->nx, nu = (size_t)h->nu, N = (size_t)h->N, ny = (size_t)desc->ny;
  const size_t nL = (N + 1) * nx * ny;
  if (!dev && !ref_all_finite(L, B * nL)) return fail(-2, "%s: L holds a non-finite value", me);
  // doubles per trajectory of every double output, in the order of the argument list
  const size_t nSX = (N + 1) * nx * (diag ? 1 : nx), nSU = N * nu * (diag ? 1 : nu), nXo = S * (N + 1) * nx, nUo = S * N * nu, nCnt = N + 1;
  constexpr int NO = 12;
  double *outs[NO] = {cost, viol, stats, dXmean, SX, dUmean, SU, X_out, U_out, dEmean, SE, Xh_out};
  const size_t per[NO] = {S, S, 8, (N + 1) * nx, nSX, N * nu, nSU, nXo, nUo, (N + 1) * nx, nSX, nXo};
  static const char *const names[NO] = {"cost", "viol", "stats", "dXmean", "SX", "dUmean", "SU", "X_out", "U_out", "dEmean", "SE", "Xh_out"};
  HIPCHK(hipSetDevice(h->device));
  Staging st(h, me, dev);
  const double *x0d, *Ld;
  double *od[NO], *Cd, *sdd;
  int32_t *cntd;
  st.scratch(ny * nx * sizeof(double), &Cd);
  st.scratch(ny * sizeof(double), &sdd);
  st.in("x0", x0, B * nx * sizeof(double), &x0d);
  st.in("L", L, B * nL * sizeof(double), &Ld);
  for (int i = 0; i < NO; ++i) st.out(names[i], outs[i], B * per[i] * sizeof(double), &od[i]);
  st.out("nviol_step", nviol_step, B * nCnt * sizeof(int32_t), &cntd);
  { int rc = st.begin(); if (rc) return rc; }
  HIPCHK(hipMemcpy(Cd, desc->C, ny * nx * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(sdd, sd, ny * sizeof(double), hipMemcpyHostToDevice));
  { int rc = fork_from_user(h); if (rc) return rc; }
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const Inner *q = h->g[gi];
    const size_t b0 = (size_t)h->b0[gi];
    const PlantDev pd = plant ? plant->pd : own_model_plant(q);
    a.b0 = (int)b0;
    a.x0 = x0d ? x0d + b0 * nx : nullptr;
    double *go[NO];
    for (int i = 0; i < NO; ++i) go[i] = od[i] ? od[i] + b0 * per[i] : nullptr;
    a.cost = go[0]; a.viol = go[1]; a.stats = go[2]; a.dXmean = go[3]; a.SX = go[4]; a.dUmean = go[5]; a.SU = go[6]; a.X_out = go[7]; a.U_out = go[8];
    a.nviol_step = cntd ? cntd + b0 * nCnt : nullptr;
    McofArgs o;
    o.ny = desc->ny; o.t4 = q->route.t4 ? 1 : 0;   // (sens_stacks: the layout of A / Bm)
    o.C = Cd; o.sd = sdd; o.L = Ld + b0 * nL;
    o.dEmean = go[9]; o.SE = go[10]; o.Xh_out = go[11];
    { int rc = plant_launch_rc(mcof_launch(pd, q->d, a, f, o, q->stream), me, "sampling", pd); if (rc) return rc; }
  }
  return st.finish();
}

}  // extern "C" (reopened below)

// ================================================================================================================
// Device-resident extended Kalman filter (include/cddp_hip.h "extended Kalman filter on the device"; kernels: inst_ekf.hip, arithmetic:
// ekf.hpp).  The object owns its sensor and noise matrices, its state (xh, P, info, the step count) and the buffers of its entries; the
// plant it was created on is only read.  It is not tied to a handle, so its host forms are staged through a scratch of its own
// (EkfStage: the declarations, checks and order of the handle's Staging) on its own stream.
// ================================================================================================================
struct cddp_hip_ekf {
  cddp_hip_plant *plant = nullptr;
  EkfDev e;
  int nx = 0, nu = 0, B = 0, device = 0, t = 0;
  hipStream_t stream = nullptr;
  double *d_mats = nullptr;          // C | v | W | Wu
  double *d_state = nullptr;         // xh | P
  int32_t *d_info = nullptr;
  char *d_io = nullptr; size_t io_cap = 0;
  // cddp_hip_mpc_run_ekf: the true state, y, the commanded u_0, nis of the step (B each); W [steps][B][nx] | Yn [steps][B][ny]; the logs
  double *d_loop = nullptr;
  double *d_noise = nullptr; size_t noise_cap = 0;
  double *d_log = nullptr; size_t log_cap = 0;
};

namespace {

int ekf_free(cddp_hip_ekf *k) {
  hipSetDevice(k->device);
  if (k->stream) { hipStreamSynchronize(k->stream); hipStreamDestroy(k->stream); }
  void *bufs[] = {k->d_mats, k->d_state, k->d_info, k->d_io, k->d_loop, k->d_noise, k->d_log};
  for (void *q : bufs) if (q) hipFree(q);
  delete k;
  return 0;
}

int ekf_grow(double **p, size_t *cap, size_t n) {
  if (*cap >= n) return 0;
  if (*p) hipFree(*p);
  *p = nullptr; *cap = 0;
  HIPCHK(hipMalloc((void **)p, n * sizeof(double)));
  *cap = n;
  return 0;
}

struct EkfStage {
  struct Arr { const char *name; const void *caller; size_t bytes; void *slot; size_t off; int dir; };
  cddp_hip_ekf *k; const char *me; bool dev;
  std::vector<Arr> arr;
  size_t total = 0;
  EkfStage(cddp_hip_ekf *k_, const char *me_, bool dev_) : k(k_), me(me_), dev(dev_) {}
  void add(const char *name, const void *caller, size_t bytes, void *slot, int dir) {
    if (!caller) { Staging::put(slot, nullptr); return; }
    if (dev) Staging::put(slot, caller);
    arr.push_back(Arr{name, caller, bytes, slot, total, dir});
    if (!dev) total += (bytes + 7) & ~(size_t)7;
  }
  template <class T> void in(const char *name, const T *p, size_t bytes, const T **slot) { add(name, p, bytes, slot, +1); }
  template <class T> void out(const char *name, T *p, size_t bytes, T **slot) { add(name, p, bytes, slot, -1); }
  int begin() {
    if (dev) { for (const Arr &a : arr) { int rc = io_check_pointer(k->device, "estimator", a.caller, a.bytes, me, a.name); if (rc) return rc; } return 0; }
    if (k->io_cap < total) {
      if (k->d_io) hipFree(k->d_io);
      k->d_io = nullptr; k->io_cap = 0;
      HIPCHK(hipMalloc((void **)&k->d_io, total));
      k->io_cap = total;
    }
    for (const Arr &a : arr) {
      Staging::put(a.slot, k->d_io + a.off);
      if (a.dir > 0) HIPCHK(hipMemcpy(k->d_io + a.off, a.caller, a.bytes, hipMemcpyHostToDevice));
    }
    return 0;
  }
  int finish() {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(k->stream));
    if (!dev) for (const Arr &a : arr) if (a.dir < 0) HIPCHK(hipMemcpy(const_cast<void *>(a.caller), k->d_io + a.off, a.bytes, hipMemcpyDeviceToHost));
    return 0;
  }
};

int ekf_flags(const char *me, const cddp_hip_ekf *k, int flags, int known) {
  if (!k) return fail(-1, "%s: null estimator", me);
  if (flags & ~known) return fail(-2, "%s: unknown flag bits 0x%x", me, (unsigned)(flags & ~known));
  return 0;
}

// y with NaN allowed where the flag makes it a drop-out
bool ekf_meas_finite(const double *y, size_t n, bool nan_ok) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(y[i]) && !(nan_ok && y[i] != y[i])) return false;
  return true;
}

int ekf_walk(cddp_hip_ekf *k, const char *me, const EkfWalk &w, hipStream_t s) {
  const hipError_t e = ekf_launch_walk(k->plant->pd, k->e, w, s);
  if (e == hipErrorInvalidValue) return fail(-3, "%s: the library has no filter kernel for model id %d with nx = %d, nu = %d", me, k->plant->pd.model, k->nx, k->nu);
  HIPCHK(e);
  return 0;
}

}  // namespace

extern "C" {

int cddp_hip_ekf_create(cddp_hip_plant *model, const cddp_hip_ekf_desc *c, cddp_hip_ekf **out) {
  static const char *const me = "cddp_hip_ekf_create";
  if (!c || !out) return fail(-1, "%s: null argument", me);
  if (c->abi_version != CDDP_HIP_ABI_VERSION) return fail(-2, "%s: ABI version mismatch: got %d want %d", me, c->abi_version, CDDP_HIP_ABI_VERSION);
  if (c->ny < 1 || c->ny > CDDP_HIP_KF_MAX_NY) return fail(-2, "%s: ny = %d, 1 .. %d measurement rows are expected", me, c->ny, CDDP_HIP_KF_MAX_NY);
  if (!c->C) return fail(-1, "%s: null C pointer", me);
  if (!c->v) return fail(-1, "%s: null v pointer", me);
  if (!model) return fail(-1, "%s: null model plant", me);   // (what precedes needs no plant, and so no device at all; what follows reads its dimensions)
  const size_t nx = (size_t)model->pd.nx, nu = (size_t)model->pd.nu, B = (size_t)model->B, m = (size_t)c->ny, lead = c->per_trajectory ? B : 1;
  for (size_t i = 0; i < lead * m; ++i)
    if (!std::isfinite(c->v[i]) || !(c->v[i] > 0.0)) return fail(-2, "%s: v holds an entry that is not finite and > 0 (a measurement variance)", me);
  if (!ref_all_finite(c->C, lead * m * nx)) return fail(-2, "%s: C holds a non-finite value", me);
  if (c->W && !ref_all_finite(c->W, lead * nx * nx)) return fail(-2, "%s: W holds a non-finite value", me);
  if (c->Wu && !ref_all_finite(c->Wu, lead * nu * nu)) return fail(-2, "%s: Wu holds a non-finite value", me);
  if (model->pd.substeps > 1)
    return fail(-2, "%s: the model plant takes %d substeps per control interval: the filter linearises one step of dt (the product of sub-step Jacobians is not available)", me, model->pd.substeps);
  HIPCHK(hipSetDevice(model->device));
  cddp_hip_ekf *k = new cddp_hip_ekf();
  k->plant = model; k->nx = (int)nx; k->nu = (int)nu; k->B = (int)B; k->device = model->device;
  const size_t nC = lead * m * nx, nv = lead * m, nW = c->W ? lead * nx * nx : 0, nWu = c->Wu ? lead * nu * nu : 0;
  std::vector<double> mats(nC + nv + nW + nWu);
  std::memcpy(mats.data(), c->C, nC * sizeof(double));
  std::memcpy(mats.data() + nC, c->v, nv * sizeof(double));
  if (nW) std::memcpy(mats.data() + nC + nv, c->W, nW * sizeof(double));
  if (nWu) std::memcpy(mats.data() + nC + nv + nW, c->Wu, nWu * sizeof(double));
  const size_t nS = B * nx + B * nx * nx;
  hipError_t e = hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void **)&k->d_mats, mats.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(k->d_mats, mats.data(), mats.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void **)&k->d_state, nS * sizeof(double));
  if (e == hipSuccess) e = hipMemset(k->d_state, 0, nS * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&k->d_info, B * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemset(k->d_info, 0, B * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void **)&k->d_loop, B * (nx + m + nu + 1) * sizeof(double));
  if (e != hipSuccess) { ekf_free(k); return fail(-10, "%s: %s", me, hipGetErrorString(e)); }
  EkfDev &d = k->e;
  d.ny = c->ny; d.per_traj = c->per_trajectory ? 1 : 0;
  d.C = k->d_mats; d.v = d.C + nC; d.W = nW ? d.v + nv : nullptr; d.Wu = nWu ? d.v + nv + nW : nullptr;
  d.xh = k->d_state; d.P = d.xh + B * nx; d.info = k->d_info;
  *out = k;
  return 0;
}

int cddp_hip_ekf_destroy(cddp_hip_ekf *k) { return k ? ekf_free(k) : 0; }

int cddp_hip_ekf_reset(cddp_hip_ekf *k, int flags, const double *xh0, const double *P0) {
  static const char *const me = "cddp_hip_ekf_reset";
  { int rc = ekf_flags(me, k, flags, CDDP_HIP_EKF_DEVICE | CDDP_HIP_EKF_PER_TRAJ); if (rc) return rc; }
  if (!xh0) return fail(-1, "%s: null xh0 pointer", me);
  if (!P0) return fail(-1, "%s: null P0 pointer", me);
  const bool dev = (flags & CDDP_HIP_EKF_DEVICE) != 0, per = (flags & CDDP_HIP_EKF_PER_TRAJ) != 0;
  const size_t nx = (size_t)k->nx, B = (size_t)k->B, nP = (per ? B : 1) * nx * nx;
  if (!dev) {
    if (!ref_all_finite(xh0, B * nx)) return fail(-2, "%s: xh0 holds a non-finite value", me);
    if (!ref_all_finite(P0, nP)) return fail(-2, "%s: P0 holds a non-finite value", me);
  }
  HIPCHK(hipSetDevice(k->device));
  EkfStage st(k, me, dev);
  const double *xd, *Pd;
  st.in("xh0", xh0, B * nx * sizeof(double), &xd);
  st.in("P0", P0, nP * sizeof(double), &Pd);
  { int rc = st.begin(); if (rc) return rc; }
  HIPCHK(ekf_launch_reset(k->e, k->nx, k->B, xd, Pd, per ? 1 : 0, k->stream));
  k->t = 0;
  return st.finish();
}

int cddp_hip_ekf_update(cddp_hip_ekf *k, int flags, const double *y, double *nis) {
  static const char *const me = "cddp_hip_ekf_update";
  { int rc = ekf_flags(me, k, flags, CDDP_HIP_EKF_DEVICE | CDDP_HIP_EKF_SKIP_NAN); if (rc) return rc; }
  if (!y) return fail(-1, "%s: null y pointer", me);
  const bool dev = (flags & CDDP_HIP_EKF_DEVICE) != 0, skip = (flags & CDDP_HIP_EKF_SKIP_NAN) != 0;
  const size_t B = (size_t)k->B, m = (size_t)k->e.ny;
  if (!dev && !ekf_meas_finite(y, B * m, skip)) return fail(-2, "%s: y holds a non-finite value (a NaN is a missing measurement only with CDDP_HIP_EKF_SKIP_NAN)", me);
  HIPCHK(hipSetDevice(k->device));
  EkfStage st(k, me, dev);
  EkfWalk w;
  std::memset(&w, 0, sizeof(w));
  st.in("y", y, B * m * sizeof(double), &w.Y);
  st.out("nis", nis, B * sizeof(double), &w.nis_out);
  { int rc = st.begin(); if (rc) return rc; }
  w.B = k->B; w.t0 = k->t; w.upd0 = 1; w.skip_nan = skip ? 1 : 0;
  { int rc = ekf_walk(k, me, w, k->stream); if (rc) return rc; }
  return st.finish();
}

int cddp_hip_ekf_predict(cddp_hip_ekf *k, int flags, const double *u) {
  static const char *const me = "cddp_hip_ekf_predict";
  { int rc = ekf_flags(me, k, flags, CDDP_HIP_EKF_DEVICE); if (rc) return rc; }
  if (!u) return fail(-1, "%s: null u pointer", me);
  const bool dev = (flags & CDDP_HIP_EKF_DEVICE) != 0;
  const size_t B = (size_t)k->B, nu = (size_t)k->nu;
  if (!dev && !ref_all_finite(u, B * nu)) return fail(-2, "%s: u holds a non-finite value", me);
  HIPCHK(hipSetDevice(k->device));
  EkfStage st(k, me, dev);
  EkfWalk w;
  std::memset(&w, 0, sizeof(w));
  st.in("u", u, B * nu * sizeof(double), &w.U);
  { int rc = st.begin(); if (rc) return rc; }
  w.B = k->B; w.t0 = k->t; w.T = 1;
  { int rc = ekf_walk(k, me, w, k->stream); if (rc) return rc; }
  k->t += 1;
  return st.finish();
}

int cddp_hip_ekf_get(cddp_hip_ekf *k, int flags, double *xh, double *P, int32_t *info) {
  static const char *const me = "cddp_hip_ekf_get";
  { int rc = ekf_flags(me, k, flags, CDDP_HIP_EKF_DEVICE); if (rc) return rc; }
  const bool dev = (flags & CDDP_HIP_EKF_DEVICE) != 0;
  const size_t nx = (size_t)k->nx, B = (size_t)k->B;
  HIPCHK(hipSetDevice(k->device));
  struct { void *dst; const void *src; size_t bytes; const char *name; } cp[3] = {
      {xh, k->e.xh, B * nx * sizeof(double), "xh"}, {P, k->e.P, B * nx * nx * sizeof(double), "P"}, {info, k->e.info, B * sizeof(int32_t), "info"}};
  if (dev) for (const auto &c : cp) if (c.dst) { int rc = io_check_pointer(k->device, "estimator", c.dst, c.bytes, me, c.name); if (rc) return rc; }
  for (const auto &c : cp) if (c.dst) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, k->stream));
  HIPCHK(hipStreamSynchronize(k->stream));
  return 0;
}

int cddp_hip_ekf_run(cddp_hip_ekf *k, int flags, int T, const double *Y, const double *U, double *Xh_out, double *P_out, double *nis_out, int32_t *info) {
  static const char *const me = "cddp_hip_ekf_run";
  { int rc = ekf_flags(me, k, flags, CDDP_HIP_EKF_DEVICE | CDDP_HIP_EKF_SKIP_NAN | CDDP_HIP_EKF_DIAG); if (rc) return rc; }
  if (T < 0) return fail(-1, "%s: T must not be negative (got %d)", me, T);
  if (!Y) return fail(-1, "%s: null Y pointer", me);
  if (T > 0 && !U) return fail(-1, "%s: null U pointer", me);
  const bool dev = (flags & CDDP_HIP_EKF_DEVICE) != 0, skip = (flags & CDDP_HIP_EKF_SKIP_NAN) != 0, diag = (flags & CDDP_HIP_EKF_DIAG) != 0;
  const size_t nx = (size_t)k->nx, nu = (size_t)k->nu, B = (size_t)k->B, m = (size_t)k->e.ny, R = (size_t)T + 1;
  if (!dev) {
    if (!ekf_meas_finite(Y, B * R * m, skip)) return fail(-2, "%s: Y holds a non-finite value (a NaN is a missing measurement only with CDDP_HIP_EKF_SKIP_NAN)", me);
    if (T > 0 && !ref_all_finite(U, B * T * nu)) return fail(-2, "%s: U holds a non-finite value", me);
  }
  HIPCHK(hipSetDevice(k->device));
  EkfStage st(k, me, dev);
  EkfWalk w;
  std::memset(&w, 0, sizeof(w));
  st.in("Y", Y, B * R * m * sizeof(double), &w.Y);
  st.in("U", T > 0 ? U : nullptr, B * T * nu * sizeof(double), &w.U);
  st.out("Xh_out", Xh_out, B * R * nx * sizeof(double), &w.Xh_out);
  st.out("P_out", P_out, B * R * (diag ? nx : nx * nx) * sizeof(double), &w.P_out);
  st.out("nis_out", nis_out, B * R * sizeof(double), &w.nis_out);
  st.out("info", info, B * sizeof(int32_t), &w.info_out);
  { int rc = st.begin(); if (rc) return rc; }
  w.B = k->B; w.t0 = k->t; w.T = T; w.upd0 = 1; w.upd_after = 1; w.skip_nan = skip ? 1 : 0; w.diag = diag ? 1 : 0;
  { int rc = ekf_walk(k, me, w, k->stream); if (rc) return rc; }
  k->t += T;
  return st.finish();
}

int cddp_hip_mpc_run_ekf(cddp_hip_handle *h, cddp_hip_plant *plant, cddp_hip_ekf *k, int steps, int mode, int flags, const double *x0_true, const double *W,
                         const double *Yn, double *U_applied, double *X_visited, double *Xh_visited, double *nis, int32_t *iterations, int32_t *status,
                         cddp_hip_stats *stats_sum) {
  static const char *const me = "cddp_hip_mpc_run_ekf";
  { int rc = plant_fits(me, h, plant); if (rc) return rc; }
  if (!k) return fail(-1, "%s: null estimator", me);
  if (k->nx != h->nx || k->nu != h->nu) return fail(-2, "%s: the estimator has nx = %d, nu = %d, the handle nx = %d, nu = %d", me, k->nx, k->nu, h->nx, h->nu);
  if (k->B != h->B) return fail(-2, "%s: the estimator was created for a batch of %d, the handle for %d", me, k->B, h->B);
  if (k->device != h->device) return fail(-2, "%s: the estimator lives on device %d, the handle on device %d", me, k->device, h->device);
  if (steps <= 0) return fail(-1, "%s: steps must be positive (got %d)", me, steps);
  const bool skip = (flags & CDDP_HIP_MPC_EKF_SKIP_NAN) != 0;
  flags &= ~CDDP_HIP_MPC_EKF_SKIP_NAN;
  for (Inner *q : h->g) { int rc = in_mpc_check(q, mode, flags); if (rc) return rc; }
  if (!x0_true) return fail(-1, "%s: null x0_true pointer", me);
  const size_t nx = (size_t)h->nx, nu = (size_t)h->nu, B = (size_t)h->B, m = (size_t)k->e.ny, S = (size_t)steps;
  if (!ref_all_finite(x0_true, B * nx)) return fail(-2, "%s: x0_true holds a non-finite value", me);
  if (W && !ref_all_finite(W, B * S * nx)) return fail(-2, "%s: W holds a non-finite value", me);
  if (Yn && !ekf_meas_finite(Yn, B * (S + 1) * m, skip)) return fail(-2, "%s: Yn holds a non-finite value (a NaN is a missing measurement only with CDDP_HIP_MPC_EKF_SKIP_NAN)", me);
  HIPCHK(hipSetDevice(h->device));
  // the step's own arrays, and the noise step-major ([k][B][.]) so that a step reads one contiguous block, as the public entries do
  double *const dx = k->d_loop, *const dy = dx + B * nx, *const du0 = dy + B * m, *const dnis = du0 + B * nu;
  { int rc = ekf_grow(&k->d_noise, &k->noise_cap, S * B * (nx + m)); if (rc) return rc; }
  { int rc = ekf_grow(&k->d_log, &k->log_cap, B * S * (nx + 1)); if (rc) return rc; }
  double *const dW = k->d_noise, *const dYn = dW + S * B * nx, *const dXh = k->d_log, *const dNis = dXh + B * S * nx;
  {
    std::vector<double> buf(S * B * std::max(nx, m));
    if (W) {
      for (size_t b = 0; b < B; ++b) for (size_t s = 0; s < S; ++s) std::memcpy(&buf[(s * B + b) * nx], W + (b * S + s) * nx, nx * sizeof(double));
      HIPCHK(hipMemcpy(dW, buf.data(), S * B * nx * sizeof(double), hipMemcpyHostToDevice));
    }
    if (Yn) {
      for (size_t b = 0; b < B; ++b) for (size_t s = 0; s < S; ++s) std::memcpy(&buf[(s * B + b) * m], Yn + (b * (S + 1) + s) * m, m * sizeof(double));
      HIPCHK(hipMemcpy(dYn, buf.data(), S * B * m * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  HIPCHK(hipMemcpy(dx, x0_true, B * nx * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(k->d_log, 0, B * S * (nx + 1) * sizeof(double)));
  HIPCHK(hipStreamSynchronize(k->stream));   // (an earlier entry of the estimator has completed: they all synchronise; this orders a failed one)
  if (stats_sum) std::memset(stats_sum, 0, sizeof(*stats_sum));
  { int rc = fork_from_user(h); if (rc) return rc; }
  auto log_of = [&](size_t gi, int kk) {
    EkfLog l;
    std::memset(&l, 0, sizeof(l));
    l.nx = (int)nx; l.nu = (int)nu; l.b0 = h->b0[gi]; l.B = h->g[gi]->d.B; l.steps = steps; l.k = kk;
    l.Xh_log = dXh; l.nis_log = dNis; l.Ulog = h->g[gi]->d_log_u; l.Xlog = h->g[gi]->d_log_x;
    return l;
  };
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    Inner *q = h->g[gi];
    int rc = in_mpc_log_begin(q, steps); if (rc) return rc;
    EkfLog l = log_of(gi, -1);
    l.x = dx;
    HIPCHK(ekf_launch_log(l, q->stream));
  }
  const int aflags = flags | CDDP_HIP_MPC_X_DEVICE;
  int rc_run = 0;
  std::string err_run;
  for (int kk = 0; kk < steps && !rc_run; ++kk) {
    const int kmode = kk == 0 ? CDDP_HIP_MPC_KEEP_PLAN : mode, kflags = kk == 0 ? CDDP_HIP_MPC_X_DEVICE : aflags;
    for (Inner *q : h->g) { rc_run = in_mpc_check(q, kmode, kflags); if (rc_run) break; }
    // per group, on its stream: y from the true state, the update, the estimate into the log, the advance from the estimate
    for (size_t gi = 0; gi < h->g.size() && !rc_run; ++gi) {
      Inner *q = h->g[gi];
      const int b0 = h->b0[gi], Bg = q->d.B;
      hipError_t e = ekf_launch_measure(k->e, (int)nx, b0, Bg, dx, Yn ? dYn + (size_t)kk * B * m : nullptr, dy, q->stream);
      if (e != hipSuccess) { rc_run = fail(-10, "%s: measurement: %s", me, hipGetErrorString(e)); break; }
      EkfWalk w;
      std::memset(&w, 0, sizeof(w));
      w.b0 = b0; w.B = Bg; w.t0 = k->t; w.upd0 = 1; w.skip_nan = skip ? 1 : 0; w.Y = dy; w.nis_out = dnis;
      rc_run = ekf_walk(k, me, w, q->stream);
      if (rc_run) break;
      EkfLog l = log_of(gi, kk);
      l.xh = k->e.xh; l.nis = dnis;
      e = ekf_launch_log(l, q->stream);
      if (e != hipSuccess) { rc_run = fail(-10, "%s: log: %s", me, hipGetErrorString(e)); break; }
      rc_run = in_mpc_advance(q, kmode, kflags, k->e.xh + (size_t)b0 * nx, false);
    }
    if (rc_run) break;
    cddp_hip_stats st;
    rc_run = cddp_hip_solve(h, stats_sum ? &st : nullptr);
    if (rc_run) break;
    if (stats_sum) stats_add(stats_sum, st);
    // iterations and status (and the model's own head, which the rows below replace); u_0 of the plan; the plant on the true state; the
    // prediction with the commanded u_0; the saturated u_0 and x_{k+1} into the log
    for (size_t gi = 0; gi < h->g.size() && !rc_run; ++gi) {
      Inner *q = h->g[gi];
      const int b0 = h->b0[gi], Bg = q->d.B;
      rc_run = in_mpc_log(q, steps, kk);
      if (rc_run) break;
      hipError_t e = ekf_launch_head(q->d, (int)nu, b0, du0, q->stream);
      double *const xg = dx + (size_t)b0 * nx, *const ug = du0 + (size_t)b0 * nu;
      if (e == hipSuccess) e = plant_launch_step(plant->pd, Bg, b0, xg, ug, W ? dW + ((size_t)kk * B + b0) * nx : nullptr, xg, q->stream);
      if (e != hipSuccess) { rc_run = fail(-10, "%s: plant step: %s", me, hipGetErrorString(e)); break; }
      EkfLog l = log_of(gi, kk);
      l.u0 = du0; l.x = dx; l.lower = plant->pd.lower; l.upper = plant->pd.upper;
      e = ekf_launch_log(l, q->stream);
      if (e != hipSuccess) { rc_run = fail(-10, "%s: log: %s", me, hipGetErrorString(e)); break; }
      EkfWalk w;
      std::memset(&w, 0, sizeof(w));
      w.b0 = b0; w.B = Bg; w.t0 = k->t; w.T = 1; w.U = du0;
      rc_run = ekf_walk(k, me, w, q->stream);
    }
    if (!rc_run) k->t += 1;
  }
  if (rc_run) err_run = g_err;
  for (size_t gi = 0; gi < h->g.size(); ++gi) {
    const size_t b0 = (size_t)h->b0[gi];
    int rc = in_mpc_log_fetch(h->g[gi], steps, U_applied ? U_applied + b0 * S * nu : nullptr, X_visited ? X_visited + b0 * (S + 1) * nx : nullptr,
                              iterations ? iterations + b0 * S : nullptr, status ? status + b0 * S : nullptr);
    if (rc && !rc_run) return rc;
  }
  // (every group stream has been synchronised by its fetch)
  if (Xh_visited) HIPCHK(hipMemcpy(Xh_visited, dXh, B * S * nx * sizeof(double), hipMemcpyDeviceToHost));
  if (nis) HIPCHK(hipMemcpy(nis, dNis, B * S * sizeof(double), hipMemcpyDeviceToHost));
  if (rc_run) { g_err = err_run; return rc_run; }
  return join_to_user(h);
}

}  // extern "C"
