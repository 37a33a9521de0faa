// The sampling front end through cddp-cpp_amd/host/cddp_hip.hpp (HipBatchSolver::sampleControls, mppiBlend, mppiRefine).  Mode "cpu": without
// a resident batch the three methods throw with a message, and the C entries answer the refusals that need no device.  Mode "gpu": a 2 x 1
// LTI batch is solved with CLDDP; the candidates of sampleControls are csrc/mppi.hpp evaluated here on the host, bit for bit (around a given
// mean and around the live plan); a two-round mppiRefine equals the loop written out over sampleControls -> scoreRollouts -> mppiBlend,
// through host pointers and through device pointers alike; with CDDP_HIP_MPPI_SEED a re-solve runs; a host pointer passed as a device
// pointer and a device allocation ONE ELEMENT short are refused with their own messages and nothing is written.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../cddp-cpp_amd/host/cddp_hip.hpp"
#include "../../cddp-cpp_amd/csrc/mppi.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { if (fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

template <class F> static std::string thrown(F f) {
  try { f(); } catch (const std::exception &e) { return e.what(); }
  return "";
}
static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }
static bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

int main(int argc, char **argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  const double sigma[1] = {0.4}, lo[1] = {-0.3}, up[1] = {0.5};
  cddp_hip_mppi_desc d;
  std::memset(&d, 0, sizeof(d));
  d.seed = 0x243F6A8885A308D3ull; d.stream = 3; d.iters = 2; d.ncand = 3; d.keep_mean = 1; d.lambda = 0.05; d.viol_tol = 0.0;
  d.sigma = sigma; d.u_lower = lo; d.u_upper = up;
  {
    cddp::HipBatchSolver s(CDDP_HIP_SOLVER_CLDDP);
    double v[4] = {0, 0, 0, 0};
    EXPECT(has(thrown([&] { s.sampleControls(0, d, v, v); }), "sampleControls needs a resident batch"));
    EXPECT(has(thrown([&] { s.mppiBlend(0, d, v, v, v, nullptr, v); }), "mppiBlend needs a resident batch"));
    EXPECT(has(thrown([&] { s.mppiRefine(nullptr, 0, d, v, v, v); }), "mppiRefine needs a resident batch"));
    EXPECT(cddp_hip_sample_controls(nullptr, 0, &d, v, v) != 0 && has(cddp_hip_last_error(), "cddp_hip_sample_controls: null handle"));
    EXPECT(cddp_hip_mppi_blend(nullptr, 0, &d, v, v, v, nullptr, v, nullptr) != 0 && has(cddp_hip_last_error(), "cddp_hip_mppi_blend: null handle"));
    EXPECT(cddp_hip_mppi_refine(nullptr, nullptr, 0, &d, v, v, v, nullptr, nullptr, nullptr) != 0 && has(cddp_hip_last_error(), "cddp_hip_mppi_refine: null handle"));
    EXPECT(CDDP_HIP_MPPI_SEED == 8 && sizeof(cddp_hip_mppi_desc) == 64);
  }
  if (gpu) {
    const int B = 70, N = 7, nx = 2, nu = 1, S = 3;     // N * nu odd: the last pair is half used
    const double dt = 0.1;
    cddp::Matrix A(2, 2), Bm(2, 1);
    A(0, 0) = 1.0; A(0, 1) = 0.1; A(1, 0) = -0.2; A(1, 1) = 0.95; Bm(0, 0) = 0.005; Bm(1, 0) = 0.1;
    cddp::Matrix Q = cddp::Matrix::Identity(2), Rm = 0.3 * cddp::Matrix::Identity(1), Qf = 5.0 * cddp::Matrix::Identity(2);
    cddp::Vector goal = {0.0, 0.0}, x0 = {1.0, -0.5};
    cddp::CDDPOptions opt; opt.max_iterations = 5; opt.verbose = false;
    cddp::CDDP ctx(x0, goal, N, dt, std::make_unique<cddp::LTISystem>(A, Bm, dt, "euler"),
                   std::make_unique<cddp::QuadraticObjective>(Q, Rm, Qf, goal, std::vector<cddp::Vector>{}, dt), opt);
    ctx.setInitialTrajectory(std::vector<cddp::Vector>(N + 1, x0), std::vector<cddp::Vector>(N, cddp::Vector{0.0}));
    std::vector<cddp::Vector> x0s;
    for (int b = 0; b < B; ++b) x0s.push_back({1.0 - 0.02 * b, -0.5 + 0.01 * b});
    cddp::HipBatchSolver s(CDDP_HIP_SOLVER_CLDDP);
    const std::vector<cddp::CDDPSolution> sols = s.solveBatch(ctx, x0s);
    EXPECT((int)sols.size() == B);
    const size_t n0 = (size_t)B * nx, nM = (size_t)B * N * nu, nU = nM * S, nC = (size_t)B * S;
    std::vector<double> xs(n0), mean(nM);
    for (int b = 0; b < B; ++b) { xs[(size_t)b * nx] = x0s[b][0]; xs[(size_t)b * nx + 1] = x0s[b][1]; }
    for (size_t i = 0; i < nM; ++i) mean[i] = 0.2 * std::sin(0.37 * (double)i);
    // the candidates are the header's, evaluated here
    std::vector<double> U(nU, -9.0), ref(nU);
    s.sampleControls(0, d, mean.data(), U.data());
    int clipped = 0;
    for (int b = 0; b < B; ++b) for (int c = 0; c < S; ++c) for (int e = 0; e < N * nu; ++e) {
      const double z = c == 0 ? 0.0 : cddp_mppi::normal(d.seed, d.stream, (uint32_t)b, (uint32_t)c, (uint32_t)e);
      const double u = cddp_mppi::candidate(mean[(size_t)b * N * nu + e], sigma[0], z, true, lo[0], up[0]);
      ref[((size_t)b * S + c) * N * nu + e] = u;
      clipped += u == lo[0] || u == up[0];
    }
    EXPECT(same(U, ref) && clipped > 0 && clipped < (int)nU);
    // the loop written out, then the one call
    std::vector<double> m = mean, cost(nC), viol(nC), out(nM), st((size_t)B * 3);
    for (int k = 0; k < d.iters; ++k) {
      cddp_hip_mppi_desc dk = d; dk.stream = d.stream + (uint32_t)k;
      s.sampleControls(0, dk, m.data(), U.data());
      s.scoreRollouts(nullptr, 0, S, xs.data(), U.data(), cost.data(), viol.data());
      s.mppiBlend(0, dk, m.data(), U.data(), cost.data(), viol.data(), out.data(), st.data());
      m = out;
    }
    std::vector<double> rU(nM, -9.0), rc(nC, -9.0), rv(nC, -9.0), rs((size_t)B * 3, -9.0);
    s.mppiRefine(nullptr, 0, d, xs.data(), mean.data(), rU.data(), rc.data(), rv.data(), rs.data());
    EXPECT(same(rU, m) && same(rc, cost) && same(rv, viol) && same(rs, st) && !same(rU, mean));
    int multi = 0;
    for (int b = 0; b < B; ++b) multi += st[(size_t)b * 3] >= 2.0;
    EXPECT(multi > 0);
    double *dx = nullptr, *dm = nullptr, *dU = nullptr, *dc = nullptr, *dshort = nullptr;
    EXPECT(hipMalloc((void **)&dx, n0 * sizeof(double)) == hipSuccess && hipMalloc((void **)&dm, nM * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dU, nM * sizeof(double)) == hipSuccess && hipMalloc((void **)&dc, nC * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dshort, (nM - 1) * sizeof(double)) == hipSuccess);
    if (fails == 0) {
      EXPECT(hipMemcpy(dx, xs.data(), n0 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dm, mean.data(), nM * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
      EXPECT(hipMemset(dU, 0, nM * sizeof(double)) == hipSuccess && hipMemset(dshort, 0, (nM - 1) * sizeof(double)) == hipSuccess);
      EXPECT(has(thrown([&] { s.mppiRefine(nullptr, CDDP_HIP_SCORE_DEVICE, d, xs.data(), dm, dU); }), "cddp_hip_mppi_refine: x0 is not device memory"));
      EXPECT(has(thrown([&] { s.mppiRefine(nullptr, CDDP_HIP_SCORE_DEVICE, d, dx, dm, dshort); }), "cddp_hip_mppi_refine: U_out needs"));
      EXPECT(has(std::string(cddp_hip_last_error()), "its allocation ends after"));
      EXPECT(has(thrown([&] { s.sampleControls(CDDP_HIP_SCORE_DEVICE, d, dshort, dU); }), "cddp_hip_sample_controls: U_mean needs"));
      std::vector<double> back(nM, -1.0);
      EXPECT(hipMemcpy(back.data(), dU, nM * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      int wrong = 0;
      for (double v : back) wrong += v != 0.0;
      EXPECT(wrong == 0);                                 // nothing written by the refused calls
      s.mppiRefine(nullptr, CDDP_HIP_SCORE_DEVICE | CDDP_HIP_MPPI_SEED, d, dx, dm, dU, dc);
      std::vector<double> backc(nC, -1.0);
      EXPECT(hipMemcpy(back.data(), dU, nM * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(backc.data(), dc, nC * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      EXPECT(same(back, rU) && same(backc, rc));
      const std::vector<cddp::CDDPSolution> again = s.resolveBatch(ctx);      // from the refined seed
      EXPECT((int)again.size() == B);
      // U_mean = nullptr: the live plan's U, which the re-solve has just left; x0 = nullptr: its row 0
      std::vector<double> planU(nM);
      for (int b = 0; b < B; ++b) for (int t = 0; t < N; ++t) planU[(size_t)b * N + t] = again[b].control_trajectory[t][0];
      std::vector<double> a1(nM), a2(nM);
      s.mppiRefine(nullptr, 0, d, xs.data(), planU.data(), a1.data());
      s.mppiRefine(nullptr, 0, d, nullptr, nullptr, a2.data());
      EXPECT(same(a1, a2));
    }
    for (void *q : {(void *)dx, (void *)dm, (void *)dU, (void *)dc, (void *)dshort}) (void)hipFree(q);
  }
  if (fails == 0) std::printf("mppi wrapper (%s): ok\n", gpu ? "gpu" : "cpu");
  return fails == 0 ? 0 : 1;
}
