// Kernels of cddp_hip_mc_sample_meas_noise / cddp_hip_plan_montecarlo_of (include/cddp_hip.h "Monte-Carlo evaluation of a solved plan under
// output feedback"): k_mc of inst_mc.hip with a linearised Kalman estimator carried in every lane.  One kernel template on the model struct,
// dispatched on the model id -- no KernelSet, no solver kernel.  The arithmetic is plan_mc.hpp's and plan_mcof.hpp's.
//
//   k_mcof<M, PER, NW>  k_mc's shape: one workgroup per trajectory b, one lane per sample c = threadIdx.x, ceil(S / 64) <= NW wavefronts,
//                       NW = 4 or 16.  Next to the state x a lane keeps xh, the estimate of x - X_t, in registers over the horizon.  The rows
//                       X_t, U_t, K_t, A_t, B_t of the stacks in place, C, sd and L_t are the same for every lane: wave-uniform (scalar) loads
//                       through uniform_ptr.  A_t and B_t lie wave-tiled or sub-tile-minor (route.t4); the address is uniform, so the
//                       layout is a run-time branch around two copies of the prediction with constant strides and not a template
//                       parameter: one kernel per (model, PER, NW) as in inst_mc.hip.  The measurement rows are a run-time loop
//                       (ny = 1 .. 16): row r's innovation is formed from the estimate before the update and added into every row's sum
//                       at once (update_add), so no array is indexed by r and the sums are the stated ones, r ascending from 0.
//                       The measurement normals come from a second Draw: they lie past the end of k_mc's elements and are walked
//                       ascending, so each walk draws each of its pairs once.
//                       A step's reduction carries nx + nx (nx + 1) / 2 more slots (the error's moments) behind k_mc's; still one barrier
//                       per step, two LDS buffers in turn.  Lanes past S run a zero-noise loop and enter every sum as +0.0.
//   k_mcof_noise        one lane per (trajectory, sample): the measurement noise itself, sd[r] * z
//
// Bounds: a stack access is (t < N for U, K, A, Bm; t <= N for X), element e < E, trajectory b < B of the group: inside the N * E * NB * 64
// doubles (X: N + 1 steps) every stack is allocated with, in either layout.  C at (r < ny, j < NX), sd at r < ny, L at row t <= N of
// trajectory b, element (i < NX, r < ny): the extents capi.hip allocates or checks.  Outputs at sample g = b S + c of a live lane only, row
// t <= N (X_out, Xh_out) or t < N (U_out); the reduced outputs at row t <= N (t < N for the controls) of trajectory b.  LDS: red[2][NW][NSLOT],
// slot < NSLOT, wave < nw <= NW.
#include "mcof_kernels.hpp"
#include "score_fold.hpp"
#include "io_layout.hpp"
#include "plan_mcof.hpp"
#include "mc_reduce.hpp"

namespace cddp_dev {
namespace {

#define Y(M) static_assert(M::NX <= kMcMaxNx && M::NU <= kMcMaxNu, "McFactors holds the factors of at most kMcMaxNx states and kMcMaxNu controls");
PLANT_MODEL_LIST(Y)
#undef Y

template <class M, bool PER, int NW>
__global__ __launch_bounds__(64 * NW) void k_mcof(PlantDev pd, DevBuf d, const ProblemDev *__restrict__ Pk, const double *__restrict__ xrt, McArgs a, McFactors f,
                                                  McofArgs o) {
  constexpr int NX = M::NX, NU = M::NU, TX = NX * (NX + 1) / 2, TU = NU * (NU + 1) / 2;
  // slots of a step's partial sums: k_mc's (m1, q of the state | m1, q of the control | the count of v_t > viol_tol), then m1 | q of the error
  constexpr int oQX = NX, oMU = NX + TX, oQU = oMU + NU, oCnt = oQU + TU, oME = oCnt + 1, oQE = oME + NX, kUsed = oQE + TX;
  constexpr int NSLOT = kUsed < 8 ? 8 : kUsed;   // (the stats round takes slots 0 .. 6)
  typedef Objective<NX, NU> Obj;
  const ProblemDev *__restrict__ P = Pk;   // direct kernel argument: scalar loads
  __shared__ double obj_lds[Obj::kStage];
  __shared__ double red[2][NW][NSLOT];
  const int tid = threadIdx.x, nthr = blockDim.x;
  Obj::stage(P, obj_lds, tid, nthr);
  __syncthreads();
  typename Obj::Ctx oc;
  Obj::load_staged(P, oc, obj_lds);
  const int b = blockIdx.x, N = d.N, S = a.S, ny = o.ny;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nthr >> 6, lane = tid & 63;
  const bool live = tid < S;
  const size_t tile = (size_t)(b >> 6), bl = (size_t)(b & 63), NB = (size_t)d.NB;
  const int cur = d.cur[b];
  const double *Xc = d.X + (size_t)cur * d.planeX, *Uc = d.U + (size_t)cur * d.planeU;
  const bool wantx = a.dXmean || a.SX, wantu = a.dUmean || a.SU, wante = o.dEmean || o.SE, per_step = wantx || wantu || wante || a.nviol_step;
  const double fS = (double)S;
  const int layout = o.t4 ? cddp_io::kT4 : cddp_io::kTiled;
  double p[32], x[NX], xh[NX], u[NU];
#pragma unroll
  for (int i = 0; i < 32; ++i) p[i] = PER ? pd.params[(size_t)i * (size_t)pd.Bp + (size_t)(a.b0 + b)] : pd.params[i];
#pragma unroll
  for (int i = 0; i < NX; ++i) xh[i] = 0.0;
  const bool nonoise = (a.keep_nominal && tid == 0) || !live;
  cddp_mc::Draw dr, dm;   // the walk of k_mc's elements | the walk of the measurement elements behind them
  dr.begin(a.seed, a.stream, (uint32_t)(a.b0 + b), (uint32_t)tid, nonoise);
  dm.begin(a.seed, a.stream, (uint32_t)(a.b0 + b), (uint32_t)tid, nonoise);
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
  double *Ho = (o.Xh_out && live) ? o.Xh_out + g * (size_t)(N + 1) * NX : nullptr;
  cptr_t Cm = uniform_ptr(o.C), sd = uniform_ptr(o.sd);
  const double *Lb = o.L + (size_t)b * (size_t)(N + 1) * (size_t)(NX * ny);

  // totals over the wavefronts in chunk order, and what a step writes from them
  auto total = [&](int buf, int slot) {
    double s = red[buf][0][slot];
    for (int k = 1; k < nw; ++k) s = s + red[buf][k][slot];
    return s;
  };
  // one group of moments: m1 at slot oM .. oM + n, q behind it at oQ; mean [row][n], cov [row][n][n] | diag [row][n]
  auto emit_group = [&](int buf, int idx, int oM, int oQ, int n, size_t row, double *mean, double *cov) {
    if (idx < oQ) {
      if (mean) mean[row * n + (idx - oM)] = cddp_mc::moment_mean(total(buf, idx), S);
      return;
    }
    if (!cov) return;
    int i, j;
    if (a.diag) { i = j = idx - oQ; if (i >= n) return; }     // (diag: the squares lie at oQ + i)
    else tri_decode(idx - oQ, i, j);
    const double cv = cddp_mc::moment_cov(total(buf, idx), total(buf, oM + i), total(buf, oM + j), S);
    if (a.diag) cov[row * n + i] = cv;
    else { cov[(row * n + i) * n + j] = cv; cov[(row * n + j) * n + i] = cv; }
  };
  auto emit = [&](int buf, int t) {
    const size_t row = (size_t)b * (size_t)(N + 1) + (size_t)t, urow = (size_t)b * (size_t)N + (size_t)t;
    for (int idx = tid; idx < kUsed; idx += nthr) {
      if (idx < oMU) emit_group(buf, idx, 0, oQX, NX, row, a.dXmean, a.SX);
      else if (idx < oCnt) { if (t < N) emit_group(buf, idx, oMU, oQU, NU, urow, a.dUmean, a.SU); }
      else if (idx == oCnt) { if (a.nviol_step) a.nviol_step[row] = (int32_t)total(buf, oCnt); }
      else emit_group(buf, idx, oME, oQE, NX, row, o.dEmean, o.SE);
    }
  };
  auto put_count = [&](int buf, double v) {
    const unsigned long long m = __ballot(live && v > a.viol_tol);
    if (lane == 0) red[buf][wave][oCnt] = (double)__popcll(m);
  };
  // steps 1 to 5 of plan_mcof.hpp at step t: dx, the measurement update of xh, the sums of the state and of the error, row t of Xh_out
  auto measure = [&](int buf, int t, double *dx) {
    const size_t rec = (size_t)t * NB + tile;
    cptr_t Xt = uniform_ptr(Xc + rec * NX * 64 + bl), Lt = uniform_ptr(Lb + (size_t)t * (size_t)(NX * ny));
#pragma unroll
    for (int j = 0; j < NX; ++j) dx[j] = x[j] - Xt[j * 64];
    if (wantx) put_group<NX>(dx, a.SX != nullptr, a.diag != 0, lane, live, &red[buf][wave][0]);
    double acc[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) acc[i] = 0.0;
    for (int r = 0; r < ny; ++r) {
      const double z = dm.get(cddp_mcof::elem_y(NX, NU, N, ny, t, r));
      const double inn = cddp_mcof::innovation(NX, Cm + r * NX, sd[r] * z, dx, xh);
      cddp_mcof::update_add(NX, ny, r, Lt, inn, acc);
    }
    cddp_mcof::update_end(NX, acc, xh);
    if (wante) {
      double e[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) e[i] = dx[i] - xh[i];
      put_group<NX>(e, o.SE != nullptr, a.diag != 0, lane, live, &red[buf][wave][oME]);
    }
    if (Ho) {
#pragma unroll
      for (int i = 0; i < NX; ++i) Ho[(size_t)t * NX + i] = xh[i];
    }
  };

  double cost = 0.0, viol = 0.0;
  int ph = 0;   // which LDS buffer the next round of sums takes
  for (int t = 0; t < N; ++t) {
    const size_t rec = (size_t)t * NB + tile;
    cptr_t Ut = uniform_ptr(Uc + rec * NU * 64 + bl), Kt = uniform_ptr(d.K + rec * (NU * NX) * 64 + bl);
    if (Xo) {
#pragma unroll
      for (int i = 0; i < NX; ++i) Xo[(size_t)t * NX + i] = x[i];
    }
    double dx[NX], du[NU], fb[NU];
    measure(ph, t, dx);
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
    cddp_mcof::feedback(NX, NU, Kt, 64, xh, fb);
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] = u[i] + fb[i];
    {   // the prediction, from the unclipped fb: after it only xh is carried over the plant's step
      const size_t ra = cddp_io::internal(layout, 0, 0, t, (int)NB, NX * NX, 0, b), rb = cddp_io::internal(layout, 0, 0, t, (int)NB, NX * NU, 0, b);
      cptr_t At = uniform_ptr(d.A + ra), Bt = uniform_ptr(d.Bm + rb);
      double xp[NX];
      if (o.t4) cddp_mcof::predict(NX, NU, At, Bt, 4, xh, fb, xp);
      else cddp_mcof::predict(NX, NU, At, Bt, 64, xh, fb, xp);
#pragma unroll
      for (int i = 0; i < NX; ++i) xh[i] = xp[i];
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
  if (wantx || wante || Ho) {   // the measurement of step N
    double dx[NX];
    measure(ph, N, dx);
  }
  if (per_step) {
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
  // stats: k_mc's round
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
    double *out = a.stats + (size_t)b * 8;
    double cmin = red[ph][0][4], cmax = red[ph][0][5], vmax = red[ph][0][6];
    for (int k = 1; k < nw; ++k) {
      if (cddp_mc::below(red[ph][k][4], cmin)) cmin = red[ph][k][4];
      if (cddp_mc::below(cmax, red[ph][k][5])) cmax = red[ph][k][5];
      if (cddp_mc::below(vmax, red[ph][k][6])) vmax = red[ph][k][6];
    }
    if (cost != cost) { cmin = cost; cmax = cost; }   // (thread 0 is sample 0)
    if (viol != viol) vmax = viol;
    out[0] = total(ph, 2); out[1] = total(ph, 3); out[2] = mean;
    out[3] = S == 1 ? 0.0 : total(ph ^ 1, 0) / (double)(S - 1);
    out[4] = cmin; out[5] = cmax; out[6] = total(ph, 1) / fS; out[7] = vmax;
  }
}

__global__ __launch_bounds__(256) void k_mcof_noise(McArgs a, int B, int N, int nx, int nu, int ny, const double *__restrict__ sd, double *__restrict__ Yn) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)B * (size_t)a.S) return;
  const int b = (int)(g / (size_t)a.S);
  const uint32_t c = (uint32_t)(g - (size_t)b * (size_t)a.S);
  cddp_mc::Draw dm;
  dm.begin(a.seed, a.stream, (uint32_t)(a.b0 + b), c, a.keep_nominal && c == 0);
  double *out = Yn + g * (size_t)(N + 1) * (size_t)ny;
  for (int t = 0; t <= N; ++t)
    for (int r = 0; r < ny; ++r) out[(size_t)t * (size_t)ny + (size_t)r] = sd[r] * dm.get(cddp_mcof::elem_y(nx, nu, N, ny, t, r));
}

template <class M>
void mcof_go(const PlantDev &pd, const DevBuf &d, const McArgs &a, const McFactors &f, const McofArgs &o, hipStream_t stream) {
  const int nw = (a.S + 63) / 64;
  const dim3 grid((unsigned)d.B), block((unsigned)(64 * nw));
  if (nw <= 4) {
    if (pd.per_traj) hipLaunchKernelGGL((k_mcof<M, true, 4>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f, o);
    else hipLaunchKernelGGL((k_mcof<M, false, 4>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f, o);
  } else {
    if (pd.per_traj) hipLaunchKernelGGL((k_mcof<M, true, 16>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f, o);
    else hipLaunchKernelGGL((k_mcof<M, false, 16>), grid, block, 0, stream, pd, d, d.P, d.xref_traj, a, f, o);
  }
}

}  // namespace

hipError_t mcof_launch(const PlantDev &pd, const DevBuf &d, const McArgs &a, const McFactors &f, const McofArgs &o, hipStream_t stream) {
  if (d.B <= 0 || a.S < 1 || a.S > cddp_mc::kMaxSamples || o.ny < 1 || o.ny > kMcofMaxNy || !d.A || !d.Bm || !d.K || !o.C || !o.sd || !o.L) return hipErrorInvalidValue;
#define Y(M)                                     \
  if (is_model<M>(pd.model, pd.nx, pd.nu)) {     \
    mcof_go<M>(pd, d, a, f, o, stream);          \
    return hipGetLastError();                    \
  }
  PLANT_MODEL_LIST(Y)
#undef Y
  return hipErrorInvalidValue;
}

hipError_t mcof_noise_launch(const McArgs &a, int B, int N, int nx, int nu, int ny, const double *sd, double *Yn, hipStream_t stream) {
  const size_t blocks = ((size_t)B * (size_t)a.S + 255) / 256;
  if (blocks == 0 || blocks > 0x7fffffffull || ny < 1 || ny > kMcofMaxNy || !sd || !Yn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mcof_noise, dim3((unsigned)blocks), dim3(256), 0, stream, a, B, N, nx, nu, ny, sd, Yn);
  return hipGetLastError();
}

}  // namespace cddp_dev
