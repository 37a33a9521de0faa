// Host-side launch table: one KernelSet per (plant, constraint layout) instantiation.
#pragma once
#include <algorithm>
#include <vector>
#include "knobs.hpp"
#include "kernels_te.hpp"
#include "kernels_pcm.hpp"
#include "kernels_elem.hpp"
#include "kernels_mfma.hpp"
#include "kernels_logddp.hpp"
#include "kernels_msipddp.hpp"

namespace cddp_dev {

// CU-partitioned streams (round 5, capi.hip::CuPlan): when the calling thread has set a hop, the SERIAL sweep kernel of backward() is
// enqueued on the hop's stream (a stream created with hipExtStreamCreateWithCUMask) instead of the caller's, bracketed by two events:
// the wide (batch x N) kernels before / after it stay on the caller's stream.  nullptr (the default): everything on one stream.
struct SweepHop { hipStream_t s; hipEvent_t ev_in, ev_out; };
inline thread_local const SweepHop *tl_sweep_hop = nullptr;
// A failed event record / stream wait would leave two streams of one group unordered (kernels racing on K, k, V and the trial slots) without
// any launch failing: the first such error is latched here and cddp_hip_solve / backward return it (capi.hip::take_order_error).
inline thread_local hipError_t tl_order_error = hipSuccess;
inline void order_check(hipError_t e) { if (e != hipSuccess && tl_order_error == hipSuccess) tl_order_error = e; }
inline hipStream_t sweep_hop_in(hipStream_t s) {
  const SweepHop *h = tl_sweep_hop;
  if (!h || h->s == s) return s;
  order_check(hipEventRecord(h->ev_in, s));
  order_check(hipStreamWaitEvent(h->s, h->ev_in, 0));
  return h->s;
}
inline void sweep_hop_out(hipStream_t s) {
  const SweepHop *h = tl_sweep_hop;
  if (!h || h->s == s) return;
  order_check(hipEventRecord(h->ev_out, h->s));
  order_check(hipStreamWaitEvent(s, h->ev_out, 0));
}

// The kernel route of one handle: which form of each kernel class its launches take.  Launcher::route resolves it from the switches
// (knobs.hpp), the solver and the handle's buffers when the handle is created (and again when cddp_hip_set_options changes use_ilqr),
// so the derivative fill and the sweep of every iteration agree on it by construction.
struct Route {
  enum Sweep { kCoop, kLane, kElem, kMfma, kRowSplit, kOneWave };
  enum Rollout { kPair, kGroup2, kGroup3, kTwoConsumers, kLaneRollout };
  int sweep = kCoop;       // IPDDP / CLDDP / LogDDP sweep; kLane = the one-lane-per-trajectory kernel
  int roles_nh = 0;        // helper wavefronts of the role-split IPDDP sweep (0: the separate condensation kernel)
  bool ms_split = false;   // MSIPDDP, path-constrained iLQR: the split sweep (condense -> recursion -> post)
  int rollout = kPair;     // path-constrained IPDDP / LogDDP / MSIPDDP rollout; kPair = the producer / consumer wave pair
  int t4 = 0;              // sub-tile-minor sweep-input stacks (kernels.hpp::GT); the handle's DevBuf::t4
};

// Time-sliced wave priority of an oversubscribed two-role IPDDP rollout launch (kernels_lean.hpp::k_forward_ipddp_pc_sl; chosen per launch by
// capi.hip::SolveRun::roll_slice).  ticks: ONE bit of the 100 MHz clock, i.e. the window length as a power of two of 10-ns ticks (0 = off);
// late_from: the linear workgroup index from which a workgroup counts as late-placed.  kSliceFixedLate as `ticks`: a bit the clock never
// reaches, which gives the late class a fixed priority 3 (comparison only).
struct RollSlice { unsigned long long ticks = 0; int late_from = 0; };
constexpr unsigned long long kSliceFixedLate = 1ull << 62;

struct KernelSet {
  int model, nx, nu, m;
  int cst_size;   // per-step doubles of the condensed-term stack (lean IPDDP backward), 0 = fused sweep
  int te_rec_size, te_group;   // cooperative terminal-equality sweep: per-step record doubles (0 = none), lanes per trajectory
  const char *name;
  bool (*matches)(const ProblemDev &);
  Route (*route)(const DevBuf &, int solver, const Knobs &);
  void (*derivs)(const DevBuf &, const Route &, int force, hipStream_t);
  void (*backward)(const DevBuf &, const Route &, int solver, int force, int count_iter, hipStream_t);
  void (*forward)(const DevBuf &, const Route &, int solver, int a0, int na, int phase_req, int force, int first_only, hipStream_t, int k1, int poll_us, RollSlice);   // k1 > 0: the launch holds both line-search stages, split at step size k1 (two-role IPDDP rollout only)
  void (*costate)(const DevBuf &, const Route &, int solver, int a0, int na, int phase_req, int force, int first_only, hipStream_t);
  void (*update)(const DevBuf &, const Route &, int stage, int n1, int is_last, int do_count, hipStream_t);
  void (*init)(const DevBuf &, int mode, hipStream_t);
  void (*stage)(const DevBuf &, int copy_xu, int ipddp, hipStream_t);
  int (*sweep_blocks)(const DevBuf &);                                      // workgroups of the cooperative sweep launch
  int (*shadow_extra)(const DevBuf &, const Route &);                       // shadow costate: extra workgroups of the sweep launch (0: the layout has no role-split sweep)
  void (*shadow_flush)(const DevBuf &, const DevBuf *, hipStream_t);        // ... the rows of the stamp DevBuf::cs_want at once (and, end of a solve, the value-stack merge)
  bool logddp_ddp;   // LogDDP with use_ilqr = 0: the plant has explicit Hessian tensors (Model::kHasHess)
  bool has_msipddp;  // the MSIPDDP kernels (kernels_msipddp.hpp) are instantiated for this layout: nx <= 8, no terminal set, and -- with path
                     // constraints -- nu = 1 or nx = nu (the shapes msipddp_solver.cpp:1398 defines)
  bool has_logddp;   // the LogDDP kernels (kernels_logddp.hpp) are instantiated for this layout: one lane per trajectory, nx <= 8, no terminal set
  int ms_cst_size;   // MSIPDDP, path-constrained: per-step doubles of the condensed-term stack of the split sweep (kernels_msipddp.hpp::MsCst), 0 = none
};

// Layouts whose two-role rollout runs TWO consumer waves (k_forward_ipddp_pc<.., NC = 2>): the consumer, not the dynamics chain, sets the
// pace there (profiles/r05_rollout_roles.md: unicycle with box + ball rows, Euler producer idle 60 % of the launch).  Opt-in (k4_consumers).
template <class Model, class Cons> struct PcTwoConsumers { static constexpr bool value = false; };
template <class Cons> struct PcTwoConsumers<UnicycleModel, Cons> {
  // (the consumer's per-step record must be the ping-pong kind with one step of look-ahead: 16 < doubles <= 40, kernels_lean.hpp::StepIn)
  static constexpr int kRec = 5 * Cons::M + UnicycleModel::NU * UnicycleModel::NX + (Cons::HAS_X ? UnicycleModel::NX : 1) + (Cons::NEEDS_U ? UnicycleModel::NU : 1);
  static constexpr bool value = Cons::M >= 4 && kRec > 16 && kRec <= 40;
};

// Layouts whose two-role rollout also exists with the time-sliced wave priority (k_forward_ipddp_pc_sl; round 17): the ping-pong forms of
// the two plants it was measured and tested on.  Every other layout runs k_forward_ipddp_pc whatever the launch's size; that kernel keeps
// its signature, and no instantiation of it changed LDS, scratch or occupancy (profiles/r17_simd_sharing.md section 5).
template <class Model, class Cons> struct PcSlice { static constexpr bool value = false; };
template <class Cons> struct PcSlice<CartPoleModel, Cons> { static constexpr bool value = Cons::M > 0; };
template <class Cons> struct PcSlice<UnicycleModel, Cons> { static constexpr bool value = Cons::M > 0; };

template <class Model, class Cons, bool TERM = false>
struct Launcher {
  static bool matches(const ProblemDev &P) {
    return P.model == Model::ID && P.nx == Model::NX && P.nu == Model::NU && Cons::matches(P) && (TERM ? P.n_term > 0 : P.n_term == 0);
  }
  // path-constrained, no terminal set: condense -> lean sweep -> post (kernels_lean.hpp)
  static constexpr bool kLean = !TERM && Cons::M > 0;
  static constexpr int cst_size() { if constexpr (kLean) return CstLayout<Model, Cons>::SIZE; else return 0; }
  // terminal equality, no state-dependent path rows: cooperative reduced-LQR sweep (kernels_te.hpp) when the host
  // allocated its record stack (pT > 0, no terminal inequality, pT + 1 <= lanes per trajectory)
  static constexpr bool kTeCoop = TERM && !Cons::HAS_X;
  static constexpr int te_rec_size() { if constexpr (kTeCoop) return TeCfg<Model, Cons>::REC; else return 0; }
  // LogDDP on the device (kernels_logddp.hpp): one-lane kernels for every plant without a terminal set.  Register-resident up to
  // nx = 8; the nx >= 12 plants work through scratch in the sweep (12 KB per lane at the quadrotor: correct, slow -- the cooperative
  // LDS-operand form the IPDDP sweeps have is not built for LogDDP).  Full DDP (use_ilqr = 0) needs the explicit Hessian tensors.
  static constexpr int kLogMaxNx = 16;
  static constexpr bool kLog = !TERM && Model::NX <= kLogMaxNx;
  // MSIPDDP on the device (kernels_msipddp.hpp); with path constraints only the shapes for which the reference's recursion is defined
  // (nu = 1 or nx = nu, msipddp_solver.cpp:1398).  Round 5: up to nx = 13, i.e. the unconstrained quadrotor runs resident (one-lane sweep
  // through scratch: correct, slow -- 9 KB per lane); the reference's own MSIPDDPTest.SolveQuadrotor (test_msipddp_solver.cpp:565) adds a
  // control box with nu = 4, nx = 13 -- a shape :1398 does not define -- and stays refused on both routes.
  static constexpr int kMsMaxNx = 13;
  static constexpr bool kMs = !TERM && Model::NX <= kMsMaxNx && (Cons::M == 0 || Model::NU == 1 || Model::NX == Model::NU);
  static constexpr int ms_cst_size() { if constexpr (kMs && Cons::M > 0) return MsCst<Model, Cons>::SIZE; else return 0; }
  static dim3 gridB(const DevBuf &d) { return dim3((d.B + 63) / 64); }
  // Step sizes per rollout workgroup of the small path-constrained layouts: the two-wave form (default), CDDP_HIP_K4_NA = 2 | 3 =
  // NA producers + ONE consumer per (tile, group of NA step sizes) (kernels_pcm.hpp).  Built to cut the wavefront count of the
  // rollout launch (1408 -> 1056 / 939 at BASELINE config[1]) after round 3 traced its length to SIMD sharing; bitwise equal
  // (tests/test_gpu_parity.py::test_multi_alpha_rollout_groups_agree_bitwise) and MEASURED SLOWER on MI355X
  // (profiles/r04_k4_groups.md): C2 22.6 -> 25.5 / 30.3 ms of rollout class per solve with the trials of a group served one after
  // the other, 30.1 / 28.7 with their per-step work in one straight-line block; pendulum 3.4 -> 5.8 / 6.0; C3 33 -> 55 / 80.  The
  // consumer's per-trial work (~500 instructions per step: two logarithms, the slack / dual trials, cost, residual terms) is as long
  // as the producer's RK4 step (~650), so one consumer behind two or three producers is the chain the launch waits for.  Opt-in.
  // Consumer waves of the two-role rollout where both forms are instantiated (PcTwoConsumers).  Default ONE: the two-consumer kernel is
  // bitwise equal (tests/test_gpu_parity.py::test_two_consumer_rollout_agrees_bitwise) and 18 % faster as a kernel on the whole chip
  // (C3 ladder of 4 / 11 step sizes: 446 -> 386 / 1499 -> 1215 us), but inside the solve its third wavefront per (tile, step size) breaks the
  // one-wavefront-per-SIMD fit of the adaptive ladder on a group's half of the chip (64 tiles x 4 step sizes x 3 = 768 on 512 SIMDs): C3
  // 78.8 -> 79.7 ms per solve (profiles/r05_rollout_roles.md).  CDDP_HIP_K4_CONSUMERS=2 opts in.
  // Role-split sweep (round 6, kernels_coop.hpp::k_backward_ipddp_coop<.., NH > 0>): helper wavefronts in the sweep workgroup evaluate
  // what k_condense<.., true> evaluates and feed the recursion wave through an LDS ring -- one launch instead of two, no condensed-term
  // stack.  CDDP_HIP_SWEEP_ROLES = 0 (the separate kernels; comparison side of the bitwise test) | 1 | 2 helpers.  Default one, measured
  // (profiles/r06_sweep_roles.md): one helper 43.1 -> 39.9 ms at C2, 77.5 -> 67.5 at C3; two / three helpers: 40.4 / 41.2 and 77.9 / 80.1.
  template <int RB> static constexpr bool roles_fit() {
    if constexpr (!kLean || Model::NX > 8) return false;
    else return (size_t)RoleCfg<Model, Cons, RB>::RING * 8 + (size_t)CoopCfg<Model>::TPW * CoopCfg<Model>::STRIDE * 8 <= (size_t)72 * 1024;   // two workgroups per CU
  }
  static constexpr bool kRoles = roles_fit<2>();
  // The handle's route (Route), resolved once from the switches after in_create has allocated the buffers.  (d.cst && !d.ms && !d.lg:
  // an IPDDP handle with the condensed-term stack; an MSIPDDP handle keeps its own stack in d.cst, d.te_cst is allocated for IPDDP only.)
  static Route route(const DevBuf &d, int solver, const Knobs &k) {
    Route r;
    // full DDP (use_ilqr = 0): the one-lane IPDDP / LogDDP / MSIPDDP kernels carry the tensor terms; CLDDP's backward pass has none
    // (clddp_solver.cpp:79-204 ignores use_ilqr), so it keeps the cooperative sweep.  CDDP_HIP_SWEEP=lane: the one-lane kernels everywhere.
    const bool lane = k.sweep == Knobs::kSweepLane || (d.ddp && solver != CDDP_HIP_SOLVER_CLDDP);
    r.sweep = lane ? Route::kLane : Route::kCoop;
    r.ms_split = d.ms && d.cst && !lane;   // otherwise the fused one-lane MSIPDDP kernel
    if (solver == CDDP_HIP_SOLVER_IPDDP && !lane) {
      if constexpr (kLean && Model::NX > 8) {
        if (Model::NX <= 15 && Model::NU <= 8 && k.sweep == Knobs::kSweepMfma) r.sweep = Route::kMfma;
        else if (k.coop_h2) r.sweep = Route::kRowSplit;
        else if (Cons::HAS_X || k.coop_w1) r.sweep = Route::kOneWave;
      } else if constexpr (kLean) {
        if (Model::NX <= 4 && Model::NU <= 2 && k.sweep == Knobs::kSweepElem) r.sweep = Route::kElem;
        else if (kRoles && d.cst && !d.ms && !d.lg && k.sweep != Knobs::kSweepElem) r.roles_nh = k.sweep_roles;
      } else if constexpr (TERM) {
        if (!(kTeCoop && d.te_cst)) r.sweep = Route::kLane;   // the cooperative terminal-equality sweep needs its record stack
      }
    }
    if (solver == CDDP_HIP_SOLVER_LOGDDP) r.rollout = k.lg_lane_rollout ? Route::kLaneRollout : Route::kPair;
    if (solver == CDDP_HIP_SOLVER_MSIPDDP) r.rollout = k.ms_lane_rollout ? Route::kLaneRollout : Route::kPair;
    if constexpr (kLean) {
      if (solver == CDDP_HIP_SOLVER_IPDDP) {
        if (PcmTraits<Model, Cons>::kOk && k.k4_na >= 2) r.rollout = k.k4_na == 3 ? Route::kGroup3 : Route::kGroup2;
        else if (PcTwoConsumers<Model, Cons>::value && k.k4_consumers2) r.rollout = Route::kTwoConsumers;
      }
    }
    // Sub-tile-minor ("T4", kernels.hpp::GT) sweep-input stacks: exactly when the G = 16 cooperative sweep of this layout is the
    // consumer -- the one-lane, matrix-core and full-DDP sweeps read the wave-tiled form.  0 for every solver but IPDDP.
    if constexpr (CoopCfg<Model>::G == 16) {
      if (k.t4 && k.sweep != Knobs::kSweepLane && k.sweep != Knobs::kSweepMfma && !d.ddp) {
        if constexpr (kLean) r.t4 = (d.cst && !d.ms && !d.lg) ? 1 : 0;
        else if constexpr (kTeCoop) r.t4 = d.te_cst ? 1 : 0;
      }
    }
    return r;
  }
  static void derivs(const DevBuf &d, const Route &r, int force, hipStream_t s) {
    if constexpr (kLean) {
      if (d.cst && !d.ms && !d.lg) {   // IPDDP with path constraints: derivative fill fused into the condensation pass (small plants;
                     // for nx > 8 the two register sets together would spill)
        if (r.roles_nh > 0) return;   // ... or evaluated by the helper wavefronts of the sweep itself (backward())
        if constexpr (Model::NX <= 8) {
          hipLaunchKernelGGL((k_condense<Model, Cons, true>), dim3((d.B + 63) / 64, d.N), dim3(64), 0, s, d, d.P, d.xref_traj, force);
          return;
        } else {
          hipLaunchKernelGGL((k_derivs<Model>), dim3((d.B + 63) / 64, d.N), dim3(64), 0, s, d, d.P, d.xref_traj, force);
          hipLaunchKernelGGL((k_condense<Model, Cons, false>), dim3((d.B + 63) / 64, d.N), dim3(64), 0, s, d, d.P, d.xref_traj, force);
          return;
        }
      }
    }
    if constexpr (kMs && Cons::M > 0 && Model::NX <= 8) {   // MSIPDDP, split sweep: the derivative fill rides in k_ms_condense<.., true> (backward())
      if (r.ms_split) return;
    }
    hipLaunchKernelGGL((k_derivs<Model>), dim3((d.B + 63) / 64, d.N), dim3(64), 0, s, d, d.P, d.xref_traj, force);
    if constexpr (kTeCoop)
      if (d.te_cst) hipLaunchKernelGGL((k_te_condense<Model, Cons>), dim3((d.B + 63) / 64, d.N), dim3(64), 0, s, d, d.P, d.xref_traj, force);
  }
  static void backward(const DevBuf &d, const Route &r, int solver, int force, int count_iter, hipStream_t s) {
    // lane-cooperative sweeps (kernels_coop.hpp) wherever a layout has one; Route::kLane: the one-lane-per-trajectory kernels (route())
    if (solver == CDDP_HIP_SOLVER_LOGDDP) {
      // lane-cooperative sweep (the LogDDP mode of k_backward_coop_plain) for the register-resident shapes; the one-lane kernel carries
      // the tensor terms of full DDP, serves nx > 8 (scratch-backed) and CDDP_HIP_SWEEP=lane (comparison)
      if constexpr (kLog && Model::NX <= 8) {
        if (r.sweep == Route::kCoop) {
          hipLaunchKernelGGL((k_backward_coop_plain<Model, true, Cons>), dim3(coop_grid<CoopCfg<Model>::TPW>(d.B, d.xcd_map)), dim3(64), 0, sweep_hop_in(s), d, d.P, d.xref_traj, force, count_iter);
          sweep_hop_out(s);
          return;
        }
      }
      if constexpr (kLog) hipLaunchKernelGGL((k_backward_logddp<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
      return;
    }
    if (solver == CDDP_HIP_SOLVER_MSIPDDP) {
      if constexpr (kMs) {
        // path-constrained iLQR sweeps: condense (batch x N) -> value recursion -> post (batch x N) (round 5); the fused one-lane kernel
        // carries the tensor terms of full DDP, the unconstrained branch with its factor cache, and CDDP_HIP_SWEEP=lane (comparison)
        if constexpr (Cons::M > 0) {
          if (r.ms_split) {
            const dim3 gridW((d.B + 63) / 64, d.N);
            if constexpr (Model::NX <= 8) hipLaunchKernelGGL((k_ms_condense<Model, Cons, true>), gridW, dim3(64), 0, s, d, d.P, d.xref_traj, force);   // + A_t, B_t (derivs() skipped K1)
            else hipLaunchKernelGGL((k_ms_condense<Model, Cons, false>), gridW, dim3(64), 0, s, d, d.P, d.xref_traj, force);
            hipLaunchKernelGGL((k_backward_msipddp_lean<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
            hipLaunchKernelGGL((k_ms_post<Model, Cons>), gridW, dim3(64), 0, s, d, d.P, force);
            return;
          }
        }
        hipLaunchKernelGGL((k_backward_msipddp<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
      }
      return;
    }
    const bool lane_sweep = r.sweep == Route::kLane;
    const dim3 gridC(coop_grid<CoopCfg<Model>::TPW>(d.B, d.xcd_map));   // whole XCD super-groups when lines are shared between blocks
    if (solver == CDDP_HIP_SOLVER_CLDDP) {
      if (lane_sweep)
        hipLaunchKernelGGL((k_backward_clddp<Model>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
      else {
        hipLaunchKernelGGL((k_backward_coop_plain<Model, true>), gridC, dim3(64), 0, sweep_hop_in(s), d, d.P, d.xref_traj, force, count_iter);
        sweep_hop_out(s);
      }
    } else if constexpr (kLean) {
      if (lane_sweep)
        hipLaunchKernelGGL((k_backward_ipddp_lean<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
      else if constexpr (Model::NX > 8) {
        if (r.sweep == Route::kMfma) {   // one wavefront per trajectory on the f64 matrix core (kernels_mfma.hpp); grid = whole tiles per XCD
          if constexpr (Model::NX <= 15 && Model::NU <= 8) {
            const dim3 gridW(((d.NB + 7) / 8) * 8 * 64);
            hipLaunchKernelGGL((k_backward_ipddp_mfma<Model, Cons>), gridW, dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
            hipLaunchKernelGGL((k_dx_rollout_wave<Model>), gridW, dim3(64), 0, s, d, force);
          }
        } else if (r.sweep == Route::kRowSplit) {   // operands in LDS here and below: the register-resident form spills for nx = 12..14
          // CDDP_HIP_COOP_H=2: two lanes per column (32 lanes per trajectory, twice the wavefronts).  Bit-identical
          // (tests/test_gpu_parity.py::test_row_split_sweep_agrees_bitwise) but measured SLOWER where it was meant to help --
          // C4 share, 2048 trajectories: 512 -> 1024 wavefronts, 22 % fewer VALU instructions per wavefront, sweep class
          // 553 -> 637 ms -- the step is a chain of LDS round trips and a replicated factorisation, not issue slots.  Opt-in.
          hipLaunchKernelGGL((k_backward_ipddp_coop_big<Model, Cons, 2>), dim3(coop_grid<CoopCfg<Model>::TPW / 2>(d.B, d.xcd_map)), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
        } else {
          // default (round 5): two wavefronts per group of trajectories -- the A side and the gain side of a step run side by side
          // (k_backward_ipddp_coop_big2); CDDP_HIP_COOP_W=1 and the layouts with state-dependent rows keep the one-wave kernel (bitwise the same results)
          if constexpr (!Cons::HAS_X) {
            if (r.sweep != Route::kOneWave) hipLaunchKernelGGL((k_backward_ipddp_coop_big2<Model, Cons>), gridC, dim3(128), 0, sweep_hop_in(s), d, d.P, d.xref_traj, force, count_iter);
          }
          if (r.sweep == Route::kOneWave) hipLaunchKernelGGL((k_backward_ipddp_coop_big<Model, Cons, 1>), gridC, dim3(64), 0, sweep_hop_in(s), d, d.P, d.xref_traj, force, count_iter);
          sweep_hop_out(s);
        }
      }
      else {
        if (r.sweep == Route::kElem) {
          // CDDP_HIP_SWEEP=elem (nx <= 4, nu <= 2): element-ownership sweep (kernels_elem.hpp: 16 lanes per trajectory, four times the
          // wavefronts of the column-ownership form).  Bitwise equal, measured slower (165 vs 126 us at C2): opt-in.
          if constexpr (Model::NX <= 4 && Model::NU <= 2)
            hipLaunchKernelGGL((k_backward_ipddp_elem<Model, Cons>), dim3(coop_grid<4>(d.B, d.xcd_map)), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
        } else if (r.roles_nh > 0) {
          if constexpr (kRoles) {
            const hipStream_t ss = sweep_hop_in(s);
            const dim3 gridC(coop_grid<CoopCfg<Model>::TPW>(d.B, d.xcd_map) + (unsigned)(d.cs_extra > 0 ? d.cs_extra : 0));   // + the shadow costate's blocks (shadow_extra)
            // ring depth: helpers + the block being consumed + one of slack, while two workgroups still fit a CU
            if (r.roles_nh == 1) {
              if constexpr (roles_fit<3>()) hipLaunchKernelGGL((k_backward_ipddp_coop<Model, Cons, 1, 3>), gridC, dim3(128), 0, ss, d, d.P, d.xref_traj, force, count_iter);
              else hipLaunchKernelGGL((k_backward_ipddp_coop<Model, Cons, 1, 2>), gridC, dim3(128), 0, ss, d, d.P, d.xref_traj, force, count_iter);
            } else {
              if constexpr (roles_fit<4>()) hipLaunchKernelGGL((k_backward_ipddp_coop<Model, Cons, 2, 4>), gridC, dim3(192), 0, ss, d, d.P, d.xref_traj, force, count_iter);
              else if constexpr (roles_fit<3>()) hipLaunchKernelGGL((k_backward_ipddp_coop<Model, Cons, 2, 3>), gridC, dim3(192), 0, ss, d, d.P, d.xref_traj, force, count_iter);
              else hipLaunchKernelGGL((k_backward_ipddp_coop<Model, Cons, 2, 2>), gridC, dim3(192), 0, ss, d, d.P, d.xref_traj, force, count_iter);
            }
            sweep_hop_out(s);
          }
        } else {
          hipLaunchKernelGGL((k_backward_ipddp_coop<Model, Cons>), gridC, dim3(64), 0, sweep_hop_in(s), d, d.P, d.xref_traj, force, count_iter);
          sweep_hop_out(s);
        }
      }
      if constexpr (kRoles) { if (r.roles_nh > 0) return; }   // the role-split sweep's helpers did K3's work
      hipLaunchKernelGGL((k_post<Model, Cons>), dim3((d.B + 63) / 64, d.N), dim3(64), 0, s, d, d.P, force);
    } else if constexpr (!TERM && Cons::M == 0) {
      if (lane_sweep)
        hipLaunchKernelGGL((k_backward_ipddp<Model, Cons, TERM>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
      else {
        hipLaunchKernelGGL((k_backward_coop_plain<Model, false>), gridC, dim3(64), 0, sweep_hop_in(s), d, d.P, d.xref_traj, force, count_iter);
        sweep_hop_out(s);
      }
    } else {
      if constexpr (kTeCoop) {
        if (r.sweep == Route::kCoop) {
          hipLaunchKernelGGL((k_backward_te_coop<Model, Cons>), gridC, dim3(64), 0, sweep_hop_in(s), d, d.P, d.xref_traj, force, count_iter);
          sweep_hop_out(s);
          // steps per block: as many as keep >= ~1024 waves in the grid (1 for small batches)
          const int tiles = (d.B + 63) / 64;
          int tstep = (int)(((long long)tiles * d.N) / 1024); if (tstep < 1) tstep = 1; if (tstep > 16) tstep = 16;
          hipLaunchKernelGGL((k_te_post<Model, Cons>), dim3(tiles, (d.N + tstep - 1) / tstep), dim3(64), 0, s, d, d.P, force, tstep);
          return;
        }
      }
      hipLaunchKernelGGL((k_backward_ipddp<Model, Cons, TERM>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, force, count_iter);
    }
  }
  static void forward(const DevBuf &d, const Route &r, int solver, int a0, int na, int phase_req, int force, int first_only, hipStream_t s, int k1 = 0, int poll_us = 0, RollSlice sl = RollSlice()) {
    if (na <= 0) return;
    const dim3 grid((d.B + 63) / 64, na);
    if (solver == CDDP_HIP_SOLVER_LOGDDP) {
      // producer / consumer wave pair per (tile, alpha) (round 5); CDDP_HIP_LG_ROLLOUT=lane: the one-wave kernel (comparison: bitwise equal)
      if constexpr (kLog) {
        if (r.rollout == Route::kLaneRollout) hipLaunchKernelGGL((k_forward_logddp<Model, Cons>), grid, dim3(64), 0, s, d, d.P, d.xref_traj, a0, 0, phase_req, force);
        else hipLaunchKernelGGL((k_forward_logddp_pc<Model, Cons>), grid, dim3(128), 0, s, d, d.P, d.xref_traj, a0, phase_req, force);
      }
      return;
    }
    if (solver == CDDP_HIP_SOLVER_MSIPDDP) {
      // producer / consumer wave pair per (tile, alpha) (round 5); CDDP_HIP_MS_ROLLOUT=lane: the one-wave kernel (comparison: bitwise equal)
      if constexpr (kMs) {
        if (r.rollout == Route::kLaneRollout || !d.ladder_sorted) hipLaunchKernelGGL((k_forward_msipddp<Model, Cons>), grid, dim3(64), 0, s, d, d.P, d.xref_traj, a0, 0, phase_req, force);   // (a ladder that is not strictly decreasing: the one-wave kernel's mask form of the dual step search)
        else hipLaunchKernelGGL((k_forward_msipddp_pc<Model, Cons>), grid, dim3(128), 0, s, d, d.P, d.xref_traj, a0, phase_req, force);
      }
      return;
    }
    if (solver == CDDP_HIP_SOLVER_CLDDP)
      hipLaunchKernelGGL((k_forward_clddp<Model>), grid, dim3(64), 0, s, d, d.P, d.xref_traj, a0, 0, phase_req, force);
    else
    {
      if constexpr (kLean) {
        if constexpr (PcmTraits<Model, Cons>::kOk) {   // small layouts: NA producers + one consumer per (tile, group of NA step sizes), kernels_pcm.hpp
          if (r.rollout == Route::kGroup3) { hipLaunchKernelGGL((k_forward_ipddp_pcm<Model, Cons, 3>), dim3((d.B + 63) / 64, (na + 2) / 3), dim3(256), 0, s, d, d.P, d.xref_traj, a0, na, phase_req, force); return; }
          if (r.rollout == Route::kGroup2) { hipLaunchKernelGGL((k_forward_ipddp_pcm<Model, Cons, 2>), dim3((d.B + 63) / 64, (na + 1) / 2), dim3(192), 0, s, d, d.P, d.xref_traj, a0, na, phase_req, force); return; }
        }
        // producer / consumer wave pair per (tile, alpha); CDDP_HIP_K4_CONSUMERS=2: two consumers where instantiated (opt-in, see route())
        if constexpr (PcTwoConsumers<Model, Cons>::value) {
          if (r.rollout == Route::kTwoConsumers) { hipLaunchKernelGGL((k_forward_ipddp_pc<Model, Cons, false, 2>), grid, dim3(192), 0, s, d, d.P, d.xref_traj, a0, phase_req, force, k1, poll_us); return; }
        }
        if constexpr (PcSlice<Model, Cons>::value) {   // an oversubscribed launch: the same kernel with the time-sliced wave priority
          if (sl.ticks != 0ull) { hipLaunchKernelGGL((k_forward_ipddp_pc_sl<Model, Cons>), grid, dim3(128), 0, s, d, d.P, d.xref_traj, a0, phase_req, force, k1, poll_us, sl.ticks, sl.late_from); return; }
        }
        hipLaunchKernelGGL((k_forward_ipddp_pc<Model, Cons>), grid, dim3(128), 0, s, d, d.P, d.xref_traj, a0, phase_req, force, k1, poll_us);
      } else {
        if constexpr (kTeCoop && Cons::M > 0) {   // same rollout after the cooperative terminal-equality sweep
          if (r.sweep == Route::kCoop) {
            hipLaunchKernelGGL((k_forward_ipddp_pc<Model, Cons, true>), grid, dim3(128), 0, s, d, d.P, d.xref_traj, a0, phase_req, force, 0, 0);
            return;
          }
        }
        hipLaunchKernelGGL((k_forward_ipddp<Model, Cons, TERM>), grid, dim3(64), 0, s, d, d.P, d.xref_traj, a0, 0, phase_req, force);
      }
    }
    (void)first_only;
  }
  // K4b: costate trial of the surviving trials (kernels_lean.hpp)
  static void costate(const DevBuf &d, const Route &r, int solver, int a0, int na, int phase_req, int force, int first_only, hipStream_t s) {
    if (solver == CDDP_HIP_SOLVER_MSIPDDP) {   // slack / dual / costate / constraint rows of the trial the selection rule will take (the two-role rollout leaves them out)
      if constexpr (kMs) {
        if (na <= 0 || r.rollout == Route::kLaneRollout || !d.ladder_sorted) return;
        if (!force && first_only == 2) hipLaunchKernelGGL((k_pick_candidate<0>), dim3((d.B + 63) / 64), dim3(64), 0, s, d, a0, na, phase_req, force);
        hipLaunchKernelGGL((k_rows_msipddp<Model, Cons>), dim3((d.B + 63) / 64, d.N), dim3(64), 0, s, d, d.P, a0, na, phase_req, force, first_only);
      }
      return;
    }
    if (na <= 0 || solver == CDDP_HIP_SOLVER_CLDDP || solver == CDDP_HIP_SOLVER_LOGDDP) return;
    if (!force && first_only == 2) hipLaunchKernelGGL((k_pick_candidate<0>), dim3((d.B + 63) / 64), dim3(64), 0, s, d, a0, na, phase_req, force);
    if constexpr (Model::NX > 8) {
      if (!force && first_only != 0) {   // one trial per trajectory: the streaming kernel (2 - 4 waves per SIMD instead of one)
        hipLaunchKernelGGL((k_costate_one<Model>), dim3((d.B + 63) / 64, d.N + 1), dim3(64), 0, s, d, a0, na, phase_req, first_only);
        return;
      }
    }
    hipLaunchKernelGGL((k_costate<Model>), dim3((d.B + 63) / 64, d.N + 1), dim3(64), 0, s, d, a0, na, phase_req, force, force ? 0 : first_only);
  }
  // Shadow costate (kernels_lean.hpp, "K4b, deferred"): extra workgroups of a sweep launch -- enough wavefronts to take the (tiles x N + 1)
  // items in a few turns each, at most two per sweep workgroup (the sweep's LDS lets one of them share a CU with a sweep workgroup);
  // shadow_flush: the rows still pending after the last iteration, then the value rows of trajectories that finished on the other stack.
  static int shadow_extra(const DevBuf &d, const Route &r) {
    if constexpr (kRoles) {
      if (r.roles_nh <= 0) return 0;
      const int items = d.NB * (d.N + 1), per = 4 * (1 + r.roles_nh);
      const int own = (int)coop_grid<CoopCfg<Model>::TPW>(d.B, d.xcd_map);
      return std::max(1, std::min((items + per - 1) / per, 2 * own));
    }
    return 0;
  }
  static int sweep_blocks(const DevBuf &d) { return (int)coop_grid<CoopCfg<Model>::TPW>(d.B, d.xcd_map); }   // workgroups of the cooperative sweep launch
  static void shadow_flush(const DevBuf &d, const DevBuf *dm, hipStream_t s) {   // dm = nullptr: the pending rows only
    if constexpr (kRoles) {
      const dim3 grid((d.B + 63) / 64, d.N + 1);
      if (d.cs_want > 0) hipLaunchKernelGGL((k_costate_flush<Model>), grid, dim3(64), 0, s, d);
      if (!dm) return;
      hipLaunchKernelGGL((k_value_merge<Model::NX>), grid, dim3(64), 0, s, *dm);
    }
  }
  static void update(const DevBuf &d, const Route &r, int stage, int n1, int is_last, int do_count, hipStream_t s) {
    if (d.lg) {
      if constexpr (kLog) hipLaunchKernelGGL((k_update_logddp<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, stage, n1, is_last, do_count);
      return;
    }
    if (d.ms) {
      if constexpr (kMs) hipLaunchKernelGGL((k_update_msipddp<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, stage, n1, is_last, do_count);
      return;
    }
    DevBuf dd = d;
    if constexpr (kTeCoop && Cons::M > 0) dd.ev_valid = r.sweep == Route::kCoop ? 1 : 0;
    hipLaunchKernelGGL((k_update<Model, Cons, TERM>), gridB(d), dim3(64), 0, s, dd, d.P, d.xref_traj, stage, n1, is_last, do_count);
  }
  static void init(const DevBuf &d, int mode, hipStream_t s) {
    if (d.lg) {
      if constexpr (kLog) hipLaunchKernelGGL((k_init_logddp<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, mode);
      return;
    }
    if (d.ms) {
      if constexpr (kMs) hipLaunchKernelGGL((k_init_msipddp<Model, Cons>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, mode);
      return;
    }
    hipLaunchKernelGGL((k_init<Model, Cons, TERM>), gridB(d), dim3(64), 0, s, d, d.P, d.xref_traj, mode);
  }
  static void stage(const DevBuf &d, int copy_xu, int ipddp, hipStream_t s) {
    hipLaunchKernelGGL((k_stage<Model, Cons>), dim3((d.B + 63) / 64, d.N + 1), dim3(64), 0, s, d, copy_xu, ipddp);
  }
  static KernelSet set(const char *name) {
    KernelSet k;
    k.model = Model::ID; k.nx = Model::NX; k.nu = Model::NU; k.m = Cons::M; k.name = name; k.cst_size = cst_size(); k.te_rec_size = te_rec_size(); k.te_group = CoopCfg<Model>::G;
    k.matches = &matches; k.route = &route; k.derivs = &derivs; k.backward = &backward; k.forward = &forward;
    k.costate = &costate; k.update = &update; k.init = &init; k.stage = &stage; k.shadow_extra = &shadow_extra; k.sweep_blocks = &sweep_blocks; k.shadow_flush = &shadow_flush; k.has_logddp = kLog; k.logddp_ddp = Model::kHasHess; k.has_msipddp = kMs; k.ms_cst_size = ms_cst_size();
    return k;
  }
};

// one registration function per instantiation translation unit
void register_pendulum(std::vector<KernelSet> &);
void register_cartpole(std::vector<KernelSet> &);
void register_unicycle(std::vector<KernelSet> &);
void register_vehicles(std::vector<KernelSet> &);
void register_lti(std::vector<KernelSet> &);
void register_quadrotor(std::vector<KernelSet> &);
void register_quad12(std::vector<KernelSet> &);
void register_manipulator(std::vector<KernelSet> &);
void register_manip7(std::vector<KernelSet> &);
void register_terminal(std::vector<KernelSet> &);
void register_statebox(std::vector<KernelSet> &);
void register_spacecraft(std::vector<KernelSet> &);
void register_plants_small(std::vector<KernelSet> &);
void register_plants_nx10(std::vector<KernelSet> &);

}  // namespace cddp_dev
