// Kernels of cddp_hip_mc_sample_noise / cddp_hip_plan_montecarlo (include/cddp_hip.h "Monte-Carlo evaluation of a solved plan"): one kernel
// template on the model struct, dispatched on the model id as inst_score.hip is -- no KernelSet, no solver kernel.  The arithmetic is
// plan_mc.hpp's, the rollout k_score's FEEDBACK form (inst_score.hip: same order, same routines) with the noise drawn in the lane.
//
//   k_mc<M, PER, NW>   one workgroup per trajectory b, one lane per sample c = threadIdx.x, ceil(S / 64) <= NW wavefronts; a wavefront is one
//                      64-sample chunk of the tree sum.  The plan rows X_t, U_t, K_t, the initial state and the parameter block are the same
//                      for every lane: wave-uniform reads of the tiled stacks in place (scalar loads through uniform_ptr), the factors are
//                      kernel arguments.  State, control and parameter block stay in registers over the horizon.  Lanes past S run a
//                      zero-noise rollout and enter every sum as +0.0 and no count.
//                      Sums over samples: inside the wavefront the butterfly v += shfl_xor(v, m), m = 1 .. 32 (every lane ends with lane 0's
//                      total; a step's values are summed together, tree_stage below), across wavefronts through LDS in chunk order.  A
//                      step's partial sums go to one of two LDS buffers in turn, so one barrier per step separates the writers of step t
//                      from its readers and the readers of step t from the writers of step t + 2.  Counts are ballots.  Nothing of size [B][S][N] exists unless X_out / U_out ask for it.
//                      NW = 4 (S <= 256: one wavefront per SIMD, the whole register file) and NW = 16 (S <= 1024: 128 registers a lane).
//   k_mc_noise         one lane per (trajectory, sample): the coloured noise itself, for callers and tests that want the arrays
#include "mc_kernels.hpp"
#include "score_fold.hpp"
#include "plan_mc.hpp"
#include "mc_reduce.hpp"

namespace cddp_dev {
namespace {

#define Y(M) static_assert(M::NX <= kMcMaxNx && M::NU <= kMcMaxNu, "McFactors holds the factors of at most kMcMaxNx states and kMcMaxNu controls");
PLANT_MODEL_LIST(Y)
#undef Y
static_assert(kMcMaxSamples == cddp_mc::kMaxSamples && kMcMaxSamples <= 1024, "one lane per sample, one workgroup per trajectory");

template <class M, bool PER, int NW>
__global__ __launch_bounds__(64 * NW) void k_mc(PlantDev pd, DevBuf d, const ProblemDev *__restrict__ Pk, const double *__restrict__ xrt, McArgs a, McFactors f) {
  constexpr int NX = M::NX, NU = M::NU, TX = NX * (NX + 1) / 2, TU = NU * (NU + 1) / 2;
  // slots of a step's partial sums: m1 of the state | q of the state | m1 of the control | q of the control | the count of v_t > viol_tol
  constexpr int oQX = NX, oMU = NX + TX, oQU = oMU + NU, oCnt = oQU + TU, NSLOT = oCnt + 1 < 8 ? 8 : oCnt + 1;
  typedef Objective<NX, NU> Obj;
  const ProblemDev *__restrict__ P = Pk;   // direct kernel argument: scalar loads
  __shared__ double obj_lds[Obj::kStage];
  __shared__ double red[2][NW][NSLOT];
  const int tid = threadIdx.x, nthr = blockDim.x;
  Obj::stage(P, obj_lds, tid, nthr);
  __syncthreads();
  typename Obj::Ctx oc;
  Obj::load_staged(P, oc, obj_lds);
  const int b = blockIdx.x, N = d.N, S = a.S;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nthr >> 6, lane = tid & 63;
  const bool live = tid < S;
  const size_t tile = (size_t)(b >> 6), bl = (size_t)(b & 63), NB = (size_t)d.NB;
  const int cur = d.cur[b];
  const double *Xc = d.X + (size_t)cur * d.planeX, *Uc = d.U + (size_t)cur * d.planeU;
  const bool wantx = a.dXmean || a.SX, wantu = a.dUmean || a.SU, per_step = wantx || wantu || a.nviol_step;
  const double fS = (double)S;
  double p[32], x[NX], u[NU];
#pragma unroll
  for (int i = 0; i < 32; ++i) p[i] = PER ? pd.params[(size_t)i * (size_t)pd.Bp + (size_t)(a.b0 + b)] : pd.params[i];
  cddp_mc::Draw dr;
  dr.begin(a.seed, a.stream, (uint32_t)(a.b0 + b), (uint32_t)tid, (a.keep_nominal && tid == 0) || !live);
  {
    double z[NX];
    if (a.have0) {
#pragma unroll
      for (int i = 0; i < NX; ++i) z[i] = dr.get(cddp_mc::elem_x0(i));
    }
    cptr_t X0 = uniform_ptr(a.x0 ? a.x0 + (size_t)b * NX : Xc + tile * NX * 64 + bl);
    const int st = a.x0 ? 1 : 64;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      x[i] = X0[i * st];
      if (a.have0) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j <= i; ++j) s += f.l0[i * (i + 1) / 2 + j] * z[j];
        x[i] = x[i] + s;
      }
    }
  }
  const size_t g = (size_t)b * (size_t)S + (size_t)tid;
  double *Xo = (a.X_out && live) ? a.X_out + g * (size_t)(N + 1) * NX : nullptr, *Uo = (a.U_out && live) ? a.U_out + g * (size_t)N * NU : nullptr;

  // totals over the wavefronts in chunk order, and what a step writes from them
  auto total = [&](int buf, int slot) {
    double s = red[buf][0][slot];
    for (int k = 1; k < nw; ++k) s = s + red[buf][k][slot];
    return s;
  };
  auto emit = [&](int buf, int t) {
    const size_t row = (size_t)b * (size_t)(N + 1) + (size_t)t, urow = (size_t)b * (size_t)N + (size_t)t;
    for (int idx = tid; idx <= oCnt; idx += nthr) {
      if (idx < oQX) {
        if (a.dXmean) a.dXmean[row * NX + idx] = cddp_mc::moment_mean(total(buf, idx), S);
      } else if (idx < oMU) {
        if (!a.SX) continue;
        int i, j;
        if (a.diag) { i = j = idx - oQX; if (i >= NX) continue; }     // (diag: the squares lie at oQX + i)
        else tri_decode(idx - oQX, i, j);
        const double cv = cddp_mc::moment_cov(total(buf, idx), total(buf, i), total(buf, j), S);
        if (a.diag) a.SX[row * NX + i] = cv;
        else { a.SX[(row * NX + i) * NX + j] = cv; a.SX[(row * NX + j) * NX + i] = cv; }
      } else if (idx < oQU) {
        if (a.dUmean && t < N) a.dUmean[urow * NU + (idx - oMU)] = cddp_mc::moment_mean(total(buf, idx), S);
      } else if (idx < oCnt) {
        if (!a.SU || t >= N) continue;
        int i, j;
        if (a.diag) { i = j = idx - oQU; if (i >= NU) continue; }
        else tri_decode(idx - oQU, i, j);
        const double cv = cddp_mc::moment_cov(total(buf, idx), total(buf, oMU + i), total(buf, oMU + j), S);
        if (a.diag) a.SU[urow * NU + i] = cv;
        else { a.SU[(urow * NU + i) * NU + j] = cv; a.SU[(urow * NU + j) * NU + i] = cv; }
      } else if (a.nviol_step) a.nviol_step[row] = (int32_t)total(buf, oCnt);
    }
  };
  auto put_state = [&](int buf, const double *dx) { put_group<NX>(dx, a.SX != nullptr, a.diag != 0, lane, live, &red[buf][wave][0]); };
  auto put_count = [&](int buf, double v) {
    const unsigned long long m = __ballot(live && v > a.viol_tol);
    if (lane == 0) red[buf][wave][oCnt] = (double)__popcll(m);
  };

  double cost = 0.0, viol = 0.0;
  int ph = 0;   // which LDS buffer the next round of sums takes
  for (int t = 0; t < N; ++t) {
    const size_t rec = (size_t)t * NB + tile;
    cptr_t Xt = uniform_ptr(Xc + rec * NX * 64 + bl), Ut = uniform_ptr(Uc + rec * NU * 64 + bl), Kt = uniform_ptr(d.K + rec * (NU * NX) * 64 + bl);
    if (Xo) {
#pragma unroll
      for (int i = 0; i < NX; ++i) Xo[(size_t)t * NX + i] = x[i];
    }
    double dx[NX], du[NU];
#pragma unroll
    for (int j = 0; j < NX; ++j) dx[j] = x[j] - Xt[j * 64];
    if (wantx) put_state(ph, dx);
    if (a.haveu) {
      double z[NU];
#pragma unroll
      for (int i = 0; i < NU; ++i) z[i] = dr.get(cddp_mc::elem_u(NX, NU, t, i));
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j <= i; ++j) s += f.lu[i * (i + 1) / 2 + j] * z[j];
        u[i] = Ut[i * 64] + s;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NU; ++i) u[i] = Ut[i * 64];
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NX; ++j) s += Kt[(i * NX + j) * 64] * dx[j];
      u[i] = u[i] + s;
    }
    if (pd.lower) {
#pragma unroll
      for (int i = 0; i < NU; ++i) u[i] = fmin(fmax(u[i], pd.lower[i]), pd.upper[i]);
    }
    if (wantu) {
#pragma unroll
      for (int i = 0; i < NU; ++i) du[i] = u[i] - Ut[i * 64];
      put_group<NU>(du, a.SU != nullptr, a.diag != 0, lane, live, &red[ph][wave][oMU]);
    }
    cost += Obj::running_cost(oc, xrt, t, x, u);
    double vt = 0.0;
    fold_path_rows<NX, NU>(P, x, u, vt);
    viol = dmax(viol, vt);
    if (per_step) {
      if (a.nviol_step) put_count(ph, vt);
      __syncthreads();
      emit(ph, t);
      ph ^= 1;
    }
    for (int s = 0; s < pd.substeps; ++s) {
      double xn[NX];
      Stepper<M>::step(pd.integrator, pd.h, p, x, u, xn);
#pragma unroll
      for (int i = 0; i < NX; ++i) x[i] = xn[i];
    }
    if (a.havew) {
      double z[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) z[i] = dr.get(cddp_mc::elem_w(NX, NU, t, i));
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j <= i; ++j) s += f.lw[i * (i + 1) / 2 + j] * z[j];
        x[i] = x[i] + s;
      }
    }
    if (Uo) {
#pragma unroll
      for (int i = 0; i < NU; ++i) Uo[(size_t)t * NU + i] = u[i];
    }
  }
  if (Xo) {
#pragma unroll
    for (int i = 0; i < NX; ++i) Xo[(size_t)N * NX + i] = x[i];
  }
  cost += Obj::terminal_cost(P, x);
  double vN = 0.0;
  if (P->mT > 0) {
    double gT[kMTMax];
    term_ineq_eval<NX>(P, x, gT);
#pragma unroll
    for (int i = 0; i < kMTMax; ++i)   // (unrolled with a guard: gT stays in registers)
      if (i < P->mT) vN = dmax(vN, gT[i]);
  }
  viol = dmax(viol, vN);
  if (per_step) {
    if (wantx) {
      const size_t rec = (size_t)N * NB + tile;
      cptr_t Xt = uniform_ptr(Xc + rec * NX * 64 + bl);
      double dx[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) dx[j] = x[j] - Xt[j * 64];
      put_state(ph, dx);
    }
    if (a.nviol_step) put_count(ph, vN);
    __syncthreads();
    emit(ph, N);
    ph ^= 1;
  }
  if (live) {
    if (a.cost) a.cost[g] = cost;
    if (a.viol) a.viol[g] = viol;
  }
  if (!a.stats) return;
  // stats: slots 0 .. 6 of one round = sum of cost, sum of viol, n_finite, n_viol, least cost, largest cost, largest viol (NaN steps aside in
  // the three scans, as a comparison with it is false; sample 0 is where a scan starts, so its NaN is the scan's result)
  {
    const double cs = wave_tree(live ? cost : 0.0), vs = wave_tree(live ? viol : 0.0);
    const unsigned long long mf = __ballot(live && cddp_mppi::is_finite(cost) && cddp_mppi::is_finite(viol)), mv = __ballot(live && viol > a.viol_tol);
    const double inf = __builtin_inf();
    const double cmin = wave_min((live && cost == cost) ? cost : inf), cmax = wave_max((live && cost == cost) ? cost : -inf);
    const double vmax = wave_max((live && viol == viol) ? viol : -inf);
    if (lane == 0) {
      red[ph][wave][0] = cs; red[ph][wave][1] = vs; red[ph][wave][2] = (double)__popcll(mf); red[ph][wave][3] = (double)__popcll(mv);
      red[ph][wave][4] = cmin; red[ph][wave][5] = cmax; red[ph][wave][6] = vmax;
    }
  }
  __syncthreads();
  const double mean = total(ph, 0) / fS;
  {
    const double e = cost - mean;
    const double sq = wave_tree(live ? e * e : 0.0);
    if (lane == 0) red[ph ^ 1][wave][0] = sq;
  }
  __syncthreads();
  if (tid == 0) {
    double *o = a.stats + (size_t)b * 8;
    double cmin = red[ph][0][4], cmax = red[ph][0][5], vmax = red[ph][0][6];
    for (int k = 1; k < nw; ++k) {
      if (cddp_mc::below(red[ph][k][4], cmin)) cmin = red[ph][k][4];
      if (cddp_mc::below(cmax, red[ph][k][5])) cmax = red[ph][k][5];
      if (cddp_mc::below(vmax, red[ph][k][6])) vmax = red[ph][k][6];
    }
    if (cost != cost) { cmin = cost; cmax = cost; }   // (thread 0 is sample 0)
    if (viol != viol) vmax = viol;
    o[0] = total(ph, 2); o[1] = total(ph, 3); o[2] = mean;
    o[3] = S == 1 ? 0.0 : total(ph ^ 1, 0) / (double)(S - 1);
    o[4] = cmin; o[5] = cmax; o[6] = total(ph, 1) / fS; o[7] = vmax;
  }
}

DEV void noise_block(cddp_mc::Draw &dr, int n, const double *L, bool have, uint32_t e0, double (*zs)[256], int tid, double *out) {
  if (!out) return;
  if (!have) {
    for (int i = 0; i < n; ++i) out[i] = 0.0;
    return;
  }
  for (int j = 0; j < n; ++j) zs[j][tid] = dr.get(e0 + (uint32_t)j);
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    for (int j = 0; j <= i; ++j) s += L[i * (i + 1) / 2 + j] * zs[j][tid];
    out[i] = s;
  }
}

__global__ __launch_bounds__(256) void k_mc_noise(McArgs a, McFactors f, int B, int N, int nx, int nu, double *__restrict__ Z0, double *__restrict__ E,
                                                  double *__restrict__ Wn) {
  __shared__ double zs[kMcMaxNx][256];   // a lane's normals of one block, in its own column
  const int tid = threadIdx.x;
  const size_t g = (size_t)blockIdx.x * 256 + tid;
  if (g >= (size_t)B * (size_t)a.S) return;
  const int b = (int)(g / (size_t)a.S);
  const uint32_t c = (uint32_t)(g - (size_t)b * (size_t)a.S);
  cddp_mc::Draw dr;
  dr.begin(a.seed, a.stream, (uint32_t)(a.b0 + b), c, a.keep_nominal && c == 0);
  noise_block(dr, nx, f.l0, a.have0 != 0, cddp_mc::elem_x0(0), zs, tid, Z0 ? Z0 + g * (size_t)nx : nullptr);
  for (int t = 0; t < N; ++t) {
    noise_block(dr, nu, f.lu, a.haveu != 0, cddp_mc::elem_u(nx, nu, t, 0), zs, tid, E ? E + (g * (size_t)N + (size_t)t) * (size_t)nu : nullptr);
    noise_block(dr, nx, f.lw, a.havew != 0, cddp_mc::elem_w(nx, nu, t, 0), zs, tid, Wn ? Wn + (g * (size_t)N + (size_t)t) * (size_t)nx : nullptr);
  }
}

template <class M>
void mc_go(const PlantDev &pd, const DevBuf &d, const McArgs &a, const McFactors &f, hipStream_t stream) {
  const int nw = (a.S + 63) / 64;
  const dim3 grid((unsigned)d.B), block((unsigned)(64 * nw));
  if (nw <= 4) {
    if (pd.per_traj) hipLaunchKernelGGL((k_mc<M, true, 4>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f);
    else hipLaunchKernelGGL((k_mc<M, false, 4>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f);
  } else {
    if (pd.per_traj) hipLaunchKernelGGL((k_mc<M, true, 16>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f);
    else hipLaunchKernelGGL((k_mc<M, false, 16>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f);
  }
}

}  // namespace

hipError_t mc_launch(const PlantDev &pd, const DevBuf &d, const McArgs &a, const McFactors &f, hipStream_t stream) {
  if (d.B <= 0 || a.S < 1 || a.S > cddp_mc::kMaxSamples) return hipErrorInvalidValue;
#define Y(M)                                     \
  if (is_model<M>(pd.model, pd.nx, pd.nu)) {     \
    mc_go<M>(pd, d, a, f, stream);               \
    return hipGetLastError();                    \
  }
  PLANT_MODEL_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

hipError_t mc_noise_launch(const McArgs &a, const McFactors &f, int B, int N, int nx, int nu, double *Z0, double *E, double *Wn, hipStream_t stream) {
  const size_t blocks = ((size_t)B * (size_t)a.S + 255) / 256;
  if (blocks == 0 || blocks > 0x7fffffffull || nx > kMcMaxNx || nu > kMcMaxNu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mc_noise, dim3((unsigned)blocks), dim3(256), 0, stream, a, f, B, N, nx, nu, Z0, E, Wn);
  return hipGetLastError();
}

}  // namespace cddp_dev
