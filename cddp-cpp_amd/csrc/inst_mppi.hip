// Kernels of cddp_hip_sample_controls / cddp_hip_mppi_blend / cddp_hip_mppi_refine (include/cddp_hip.h "sampling-based plan refinement"):
// a refinement round is score -> weights -> blend, and the candidate controls exist only in registers.  The arithmetic is mppi.hpp's, the
// rollout k_score's (inst_score.hip: same order, same routines, no feedback); no atomics, no cross-lane sum, every sum in a fixed order.
//
//   k_mppi_score<M, PER>   one lane per (trajectory b, candidate c), g = b * S + c as in k_score.  The lane draws the normals of its own
//                          controls as it walks the horizon: one Philox call and one Box-Muller per two elements e = t * nu + i, the odd
//                          normal carried to the next element (across the step boundary when nu is odd).  The mean row of step t is read
//                          by every lane of a trajectory (a broadcast), sigma and the box are kernel arguments (scalar registers).
//   k_mppi_weights         one lane per trajectory: cddp_mppi::weights over its S records, in place in global memory
//   k_mppi_blend           one lane per (trajectory, pair j): loops c ascending, redraws the pair of each candidate (or reads the two
//                          controls from U_cand) and adds w_c (u_c - mean) to the two sums of its elements
//   k_sample_controls      one lane per (trajectory, candidate, pair): the candidates themselves, for callers who want the array
#include "mppi_kernels.hpp"
#include "score_fold.hpp"
#include "mppi.hpp"

namespace cddp_dev {
namespace {

#define Y(M) static_assert(M::NU <= kMppiMaxNu, "MppiDraw holds sigma and the box of at most kMppiMaxNu controls");
PLANT_MODEL_LIST(Y)
#undef Y

template <class M, bool PER>
__global__ __launch_bounds__(64) void k_mppi_score(PlantDev pd, DevBuf d, const ProblemDev *__restrict__ Pk, const double *__restrict__ xrt, MppiDraw a,
                                                   const double *__restrict__ x0g, const double *__restrict__ mean, double *__restrict__ cost_out,
                                                   double *__restrict__ viol_out) {
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
  const uint32_t c = (uint32_t)(g - (size_t)b * (size_t)a.S), bg = (uint32_t)(a.b0 + b);
  const bool zero = a.keep_mean && c == 0;
  double p[32], x[NX], u[NU];
#pragma unroll
  for (int i = 0; i < 32; ++i) p[i] = PER ? pd.params[(size_t)i * (size_t)pd.Bp + (size_t)(a.b0 + b)] : pd.params[i];
  if (x0g) {
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = x0g[(size_t)b * NX + i];
  } else {
    const size_t tile = (size_t)(b >> 6), lane = (size_t)(b & 63);
    const double *Xc = d.X + (size_t)d.cur[b] * d.planeX;
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = Xc[(tile * NX + i) * 64 + lane];
  }
  const double *mb = mean + (size_t)b * (size_t)N * NU;
  double cost = 0.0, viol = 0.0, z_odd = 0.0;
  for (int t = 0; t < N; ++t) {
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const uint32_t e = (uint32_t)t * NU + i;
      double z;
      if ((e & 1u) == 0) {
        const cddp_mppi::Pair pr = cddp_mppi::normal_pair(a.seed, a.stream, bg, c, e >> 1);
        z = pr.even; z_odd = pr.odd;
      } else z = z_odd;
      z = zero ? 0.0 : z;
      u[i] = cddp_mppi::candidate(mb[(size_t)t * NU + i], a.sigma[i], z, a.box != 0, a.lower[i], a.upper[i]);
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
  }
  cost += Obj::terminal_cost(P, x);
  if (P->mT > 0) {
    double gT[kMTMax];
    term_ineq_eval<NX>(P, x, gT);
    for (int i = 0; i < P->mT; ++i) viol = dmax(viol, gT[i]);
  }
  cost_out[g] = cost;
  viol_out[g] = viol;
}

__global__ __launch_bounds__(256) void k_mppi_weights(int B, int S, const double *__restrict__ cost, const double *__restrict__ viol, double viol_tol,
                                                      double lambda, double *__restrict__ w, double *__restrict__ stats) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  cddp_mppi::weights(S, cost + (size_t)b * S, viol ? viol + (size_t)b * S : nullptr, viol_tol, lambda, w + (size_t)b * S, stats + (size_t)b * 3);
}

// the controls of pair j (elements 2j and 2j + 1, the second absent at the end of an odd N * nu) of candidate c, as drawn and clipped
DEV void draw_pair(const MppiDraw &a, uint32_t bg, uint32_t c, uint32_t j, int nu, int NE, double m0, double m1, double &u0, double &u1) {
  cddp_mppi::Pair pr = cddp_mppi::normal_pair(a.seed, a.stream, bg, c, j);
  if (a.keep_mean && c == 0) { pr.even = 0.0; pr.odd = 0.0; }
  const int e0 = 2 * (int)j, e1 = e0 + 1, i0 = e0 % nu, i1 = e1 % nu;
  u0 = cddp_mppi::candidate(m0, a.sigma[i0], pr.even, a.box != 0, a.lower[i0], a.upper[i0]);
  u1 = e1 < NE ? cddp_mppi::candidate(m1, a.sigma[i1], pr.odd, a.box != 0, a.lower[i1], a.upper[i1]) : 0.0;
}

__global__ __launch_bounds__(256) void k_mppi_blend(MppiDraw a, int B, int NE, int nu, const double *__restrict__ mean_in, const double *__restrict__ U_cand,
                                                    const double *__restrict__ w, const double *__restrict__ stats, double *__restrict__ mean_out) {
  const int NP = (NE + 1) / 2;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * (size_t)NP) return;
  const int b = (int)(idx / (size_t)NP);
  const uint32_t j = (uint32_t)(idx - (size_t)b * (size_t)NP);
  const int e0 = 2 * (int)j, e1 = e0 + 1;
  const bool two = e1 < NE;
  const size_t mo = (size_t)b * (size_t)NE;
  const double m0 = mean_in[mo + e0], m1 = two ? mean_in[mo + e1] : 0.0;
  if (stats[(size_t)b * 3] == 0.0) {   // no admissible candidate: the mean stays as it is
    mean_out[mo + e0] = m0;
    if (two) mean_out[mo + e1] = m1;
    return;
  }
  const double *wb = w + (size_t)b * (size_t)a.S;
  double s0 = 0.0, s1 = 0.0;
  for (int c = 0; c < a.S; ++c) {
    double u0, u1;
    if (U_cand) {
      const double *uc = U_cand + ((size_t)b * (size_t)a.S + (size_t)c) * (size_t)NE;
      u0 = uc[e0]; u1 = two ? uc[e1] : 0.0;
    } else draw_pair(a, (uint32_t)(a.b0 + b), (uint32_t)c, j, nu, NE, m0, m1, u0, u1);
    const double wc = wb[c];
    cddp_mppi::blend_add(s0, wc, u0, m0);
    cddp_mppi::blend_add(s1, wc, u1, m1);
  }
  const int i0 = e0 % nu, i1 = e1 % nu;
  mean_out[mo + e0] = cddp_mppi::blend_end(m0, s0, a.box != 0, a.lower[i0], a.upper[i0]);
  if (two) mean_out[mo + e1] = cddp_mppi::blend_end(m1, s1, a.box != 0, a.lower[i1], a.upper[i1]);
}

__global__ __launch_bounds__(256) void k_sample_controls(MppiDraw a, int B, int NE, int nu, const double *__restrict__ mean, double *__restrict__ U_out) {
  const int NP = (NE + 1) / 2;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * (size_t)a.S * (size_t)NP) return;
  const size_t g = idx / (size_t)NP;
  const uint32_t j = (uint32_t)(idx - g * (size_t)NP);
  const int b = (int)(g / (size_t)a.S);
  const uint32_t c = (uint32_t)(g - (size_t)b * (size_t)a.S);
  const int e0 = 2 * (int)j, e1 = e0 + 1;
  const bool two = e1 < NE;
  const size_t mo = (size_t)b * (size_t)NE;
  double u0, u1;
  draw_pair(a, (uint32_t)(a.b0 + b), c, j, nu, NE, mean[mo + e0], two ? mean[mo + e1] : 0.0, u0, u1);
  U_out[g * (size_t)NE + e0] = u0;
  if (two) U_out[g * (size_t)NE + e1] = u1;
}

bool grid_of(size_t lanes, unsigned per_block, unsigned *blocks) {
  const size_t n = (lanes + per_block - 1) / per_block;
  if (n == 0 || n > 0x7fffffffull) return false;
  *blocks = (unsigned)n;
  return true;
}

}  // namespace

hipError_t mppi_score_launch(const PlantDev &pd, const DevBuf &d, const MppiDraw &a, const double *x0, const double *mean, double *cost, double *viol,
                             hipStream_t stream) {
  unsigned blocks;
  if (!grid_of((size_t)d.B * (size_t)a.S, 64, &blocks)) return hipErrorInvalidValue;
#define Y(M)                                                                                                                                        \
  if (is_model<M>(pd.model, pd.nx, pd.nu)) {                                                                                                        \
    if (pd.per_traj) hipLaunchKernelGGL((k_mppi_score<M, true>), dim3(blocks), dim3(64), 0, stream, pd, d, d.P, d.xref_traj, a, x0, mean, cost, viol); \
    else hipLaunchKernelGGL((k_mppi_score<M, false>), dim3(blocks), dim3(64), 0, stream, pd, d, d.P, d.xref_traj, a, x0, mean, cost, viol);          \
    return hipGetLastError();                                                                                                                       \
  }
  PLANT_MODEL_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

void mppi_weights_launch(int B, int S, const double *cost, const double *viol, double viol_tol, double lambda, double *w, double *stats, hipStream_t stream) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_mppi_weights, dim3((B + 255) / 256), dim3(256), 0, stream, B, S, cost, viol, viol_tol, lambda, w, stats);
}

hipError_t mppi_blend_launch(const MppiDraw &a, int B, int N, int nu, const double *mean_in, const double *U_cand, const double *w, const double *stats,
                             double *mean_out, hipStream_t stream) {
  const int NE = N * nu;
  unsigned blocks;
  if (!grid_of((size_t)B * (size_t)((NE + 1) / 2), 256, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mppi_blend, dim3(blocks), dim3(256), 0, stream, a, B, NE, nu, mean_in, U_cand, w, stats, mean_out);
  return hipGetLastError();
}

hipError_t mppi_sample_launch(const MppiDraw &a, int B, int N, int nu, const double *mean, double *U_out, hipStream_t stream) {
  const int NE = N * nu;
  unsigned blocks;
  if (!grid_of((size_t)B * (size_t)a.S * (size_t)((NE + 1) / 2), 256, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sample_controls, dim3(blocks), dim3(256), 0, stream, a, B, NE, nu, mean, U_out);
  return hipGetLastError();
}

}  // namespace cddp_dev
