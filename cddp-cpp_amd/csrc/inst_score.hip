// Kernels of cddp_hip_score_rollouts / cddp_hip_seed_best (include/cddp_hip.h "scoring candidate control sequences"): one kernel
// template on the model struct, dispatched on the model id as inst_plant.hip is -- no KernelSet, no solver kernel, no Cons type.
//
// One lane per (trajectory b, candidate c), g = b * S + c: the [B][S] arrays are indexed by g as they lie, a wavefront's lanes share x0,
// the parameter block and the plan rows of at most ceil(64 / S) + 1 trajectories, and their U streams lie N * nu * 8 bytes apart (read in
// place: a 128-byte line serves a lane for the next 16 / nu steps).  The state, the control and the parameter block stay in registers for
// the whole horizon.  Arithmetic, fixed by the header because the tests are bitwise; per step t, in this order:
//   u[i] = U[g][t][i]                                   (FEEDBACK: + s, s = 0; s += K_t[i][j] * (x[j] - X_t[j]), j ascending -- k_track_plan's line)
//   u[i] = fmin(fmax(u[i], lower[i]), upper[i])         (only a plant with a box)
//   cost += running_cost(x, u)                          (Objective<NX, NU>, (e^T Q dt) e + (u^T R dt) u, the per-step reference when there is one)
//   viol = dmax(viol, g_i), i ascending                 (the problem's path rows in stacked order: every kind's eval() of dev_constraints.hpp)
//   x <- Stepper<Model>::step(integrator, h, params, x, u), substeps times
// then cost += terminal_cost(x_N) and the terminal inequality rows folded into viol.  This is the order of k_init's warm-start loop, whose
// maxviol is the same quantity.  The handle's own model is the plant with substeps = 1, h = dt, no box and the ProblemDev's block.
//
// Constraints: P->cons[] is walked at run time and every kind struct is reached through a compile-time loop over the dimensions the model
// admits (a box and a thrust row span nu or nx, capi.hip::flatten; a ball 1 .. nx coordinates; linear rows 1 .. 4), so g[] is indexed
// statically inside every branch and the arithmetic is that of the compile-time lists by construction.
// Objective: the small plants keep Q dt | R dt | x_ref in registers, the large ones (Objective::kHoist false) in LDS, as the serial kernels do.
#include "score_fold.hpp"   // fold_path_rows, is_model: shared with the sampling rollout of inst_mppi.hip
#include "score_select.hpp"

namespace cddp_dev {
namespace {

template <class M, bool PER>
__global__ __launch_bounds__(64) void k_score(PlantDev pd, DevBuf d, const ProblemDev *__restrict__ Pk, const double *__restrict__ xrt, ScoreArgs a) {
  constexpr int NX = M::NX, NU = M::NU;
  typedef Objective<NX, NU> Obj;
  const ProblemDev *__restrict__ P = Pk;   // direct kernel argument: scalar loads
  __shared__ double obj_lds[Obj::kStage];
  Obj::stage(P, obj_lds, threadIdx.x, 64);
  __syncthreads();                         // (the only barrier: lanes past the end leave after it)
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= (size_t)d.B * (size_t)a.S) return;
  typename Obj::Ctx oc;
  Obj::load_staged(P, oc, obj_lds);
  const int b = (int)(g / (size_t)a.S), N = d.N;
  const size_t tile = (size_t)(b >> 6), lane = (size_t)(b & 63), NB = (size_t)d.NB;
  const int cur = (a.feedback || !a.x0 || !a.U) ? d.cur[b] : 0;   // the live slot: read only by the forms that use the plan
  const double *Xc = d.X + (size_t)cur * d.planeX, *Uc = d.U + (size_t)cur * d.planeU;
  double p[32], x[NX], u[NU];
#pragma unroll
  for (int i = 0; i < 32; ++i) p[i] = PER ? pd.params[(size_t)i * (size_t)pd.Bp + (size_t)(a.b0 + b)] : pd.params[i];
  const double *x0 = a.x0 ? a.x0 + (a.x0_per_cand ? g : (size_t)b) * NX : nullptr;
#pragma unroll
  for (int i = 0; i < NX; ++i) x[i] = x0 ? x0[i] : Xc[(tile * NX + i) * 64 + lane];
  const double *Ug = a.U ? a.U + g * (size_t)N * NU : nullptr;
  double *Xo = a.X_out ? a.X_out + g * (size_t)(N + 1) * NX : nullptr, *Uo = a.U_out ? a.U_out + g * (size_t)N * NU : nullptr;
  if (Xo) {
#pragma unroll
    for (int i = 0; i < NX; ++i) Xo[i] = x[i];
  }
  double cost = 0.0, viol = 0.0;
  for (int t = 0; t < N; ++t) {
    const size_t rec = (size_t)t * NB + tile;
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] = Ug ? Ug[(size_t)t * NU + i] : Uc[(rec * NU + i) * 64 + lane];
    if (a.feedback) {
      double dx[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) dx[j] = x[j] - Xc[(rec * NX + j) * 64 + lane];
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) s += d.K[(rec * (NU * NX) + i * NX + j) * 64 + lane] * dx[j];
        u[i] = u[i] + s;
      }
    }
    if (pd.lower) {
#pragma unroll
      for (int i = 0; i < NU; ++i) u[i] = fmin(fmax(u[i], pd.lower[i]), pd.upper[i]);
    }
    cost += Obj::running_cost(oc, xrt, t, x, u);
    fold_path_rows<NX, NU>(P, x, u, viol);
    for (int s = 0; s < pd.substeps; ++s) {
      double xn[NX];
      Stepper<M>::step(pd.integrator, pd.h, p, x, u, xn);
#pragma unroll
      for (int i = 0; i < NX; ++i) x[i] = xn[i];
    }
    if (Uo) {
#pragma unroll
      for (int i = 0; i < NU; ++i) Uo[(size_t)t * NU + i] = u[i];
    }
    if (Xo) {
#pragma unroll
      for (int i = 0; i < NX; ++i) Xo[(size_t)(t + 1) * NX + i] = x[i];
    }
  }
  cost += Obj::terminal_cost(P, x);
  if (P->mT > 0) {
    double gT[kMTMax];
    term_ineq_eval<NX>(P, x, gT);
    for (int i = 0; i < P->mT; ++i) viol = dmax(viol, gT[i]);
  }
  a.cost[g] = cost;
  if (a.viol) a.viol[g] = viol;
}

__global__ __launch_bounds__(256) void k_score_select(int B, int S, const double *__restrict__ cost, const double *__restrict__ viol, double viol_tol,
                                                      int32_t *__restrict__ winner) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  winner[b] = cddp_score::select(S, cost + (size_t)b * S, viol ? viol + (size_t)b * S : nullptr, viol_tol);
}

}  // namespace

hipError_t score_launch(const PlantDev &pd, const DevBuf &d, const ScoreArgs &a, hipStream_t stream) {
  const size_t blocks = ((size_t)d.B * (size_t)a.S + 63) / 64;
  if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
#define Y(M)                                                                                                                                     \
  if (is_model<M>(pd.model, pd.nx, pd.nu)) {                                                                                                     \
    if (pd.per_traj) hipLaunchKernelGGL((k_score<M, true>), dim3((unsigned)blocks), dim3(64), 0, stream, pd, d, d.P, d.xref_traj, a);            \
    else hipLaunchKernelGGL((k_score<M, false>), dim3((unsigned)blocks), dim3(64), 0, stream, pd, d, d.P, d.xref_traj, a);                       \
    return hipGetLastError();                                                                                                                    \
  }
  PLANT_MODEL_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

void score_select_launch(int B, int S, const double *cost, const double *viol, double viol_tol, int32_t *winner, hipStream_t stream) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_score_select, dim3((B + 255) / 256), dim3(256), 0, stream, B, S, cost, viol, viol_tol, winner);
}

}  // namespace cddp_dev
