// Monte-Carlo plan evaluation through cddp-cpp_amd/host/cddp_hip.hpp (HipBatchSolver::mcSampleNoise, planMonteCarlo).  Mode "cpu": without a
// resident batch both methods throw with a message, and the C entries answer the refusals that need no device.  Mode "gpu": a 2 x 1 LTI
// batch is solved with CLDDP; the noise of mcSampleNoise is csrc/plan_mc.hpp evaluated by this program, the per-sample costs of
// planMonteCarlo under initial-state and actuator noise are those of scoreRollouts(FEEDBACK | X0_PER_CANDIDATE) fed that noise, and
// stats is cddp_mc::stats of the per-sample records.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../cddp-cpp_amd/host/cddp_hip.hpp"
#include "../../cddp-cpp_amd/csrc/plan_mc.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { if (fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

template <class F> static std::string thrown(F f) {
  try { f(); } catch (const std::exception &e) { return e.what(); }
  return "";
}
static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main(int argc, char **argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  const double L0[4] = {0.05, 0.0, 0.01, 0.04}, Lu[1] = {0.05};
  cddp_hip_mc_desc desc;
  std::memset(&desc, 0, sizeof(desc));
  desc.seed = 0x1234567890ull; desc.stream = 2; desc.nsamp = 65; desc.keep_nominal = 1; desc.viol_tol = 0.0; desc.L0 = L0; desc.Lu = Lu;
  {
    cddp::HipBatchSolver s(CDDP_HIP_SOLVER_CLDDP);
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    EXPECT(has(thrown([&] { s.mcSampleNoise(0, desc, v, nullptr, nullptr); }), "mcSampleNoise needs a resident batch"));
    EXPECT(has(thrown([&] { s.planMonteCarlo(nullptr, 0, desc, nullptr, v, v, v); }), "planMonteCarlo needs a resident batch"));
    EXPECT(cddp_hip_mc_sample_noise(nullptr, 0, &desc, v, nullptr, nullptr) != 0 && has(cddp_hip_last_error(), "cddp_hip_mc_sample_noise: null handle"));
    EXPECT(cddp_hip_plan_montecarlo(nullptr, nullptr, 0, &desc, nullptr, v, v, v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0 &&
           has(cddp_hip_last_error(), "cddp_hip_plan_montecarlo: null handle"));
    EXPECT(CDDP_HIP_MC_DEVICE == 1 && CDDP_HIP_MC_DIAG == 2 && sizeof(cddp_hip_mc_desc) == 56);
  }
  if (gpu) {
    const int B = 5, N = 6, nx = 2, nu = 1, S = desc.nsamp;
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
    const size_t nC = (size_t)B * S;
    std::vector<double> Z0(nC * nx, -1.0), E(nC * N * nu, -1.0), Wn(nC * N * nx, -1.0);
    s.mcSampleNoise(0, desc, Z0.data(), E.data(), Wn.data());
    int wrong = 0;
    for (int b = 0; b < B; ++b) for (int c = 0; c < S; ++c) {
      cddp_mc::Draw dr;
      dr.begin(desc.seed, desc.stream, (uint32_t)b, (uint32_t)c, c == 0);
      const size_t g = (size_t)b * S + c;
      double z[2], v[2];
      for (int i = 0; i < nx; ++i) z[i] = dr.get(cddp_mc::elem_x0(i));
      cddp_mc::colour(nx, L0, z, v);
      wrong += !(Z0[g * nx] == v[0] && Z0[g * nx + 1] == v[1]);
      for (int t = 0; t < N; ++t) {
        z[0] = dr.get(cddp_mc::elem_u(nx, nu, t, 0));
        cddp_mc::colour(nu, Lu, z, v);
        wrong += !(E[(g * N + t) * nu] == v[0]) + !(Wn[(g * N + t) * nx] == 0.0 && Wn[(g * N + t) * nx + 1] == 0.0);
      }
    }
    EXPECT(wrong == 0);
    // the plan, then the per-sample costs against scoreRollouts fed the same noise
    std::vector<double> X((size_t)B * (N + 1) * nx), U((size_t)B * N * nu);
    for (int b = 0; b < B; ++b) {
      for (int t = 0; t <= N; ++t) for (int i = 0; i < nx; ++i) X[((size_t)b * (N + 1) + t) * nx + i] = sols[b].state_trajectory[t][i];
      for (int t = 0; t < N; ++t) U[((size_t)b * N + t) * nu] = sols[b].control_trajectory[t][0];
    }
    std::vector<double> x0c(nC * nx), Uc(nC * N * nu), cost(nC, -1.0), viol(nC, -1.0), st((size_t)B * 8, -1.0), cost2(nC, -2.0), viol2(nC, -2.0);
    for (int b = 0; b < B; ++b) for (int c = 0; c < S; ++c) {
      const size_t g = (size_t)b * S + c;
      for (int i = 0; i < nx; ++i) x0c[g * nx + i] = X[(size_t)b * (N + 1) * nx + i] + Z0[g * nx + i];
      for (int t = 0; t < N; ++t) Uc[(g * N + t) * nu] = U[((size_t)b * N + t) * nu] + E[(g * N + t) * nu];
    }
    s.planMonteCarlo(nullptr, 0, desc, nullptr, cost.data(), viol.data(), st.data());
    s.scoreRollouts(nullptr, CDDP_HIP_SCORE_FEEDBACK | CDDP_HIP_SCORE_X0_PER_CANDIDATE, S, x0c.data(), Uc.data(), cost2.data(), viol2.data());
    EXPECT(std::memcmp(cost.data(), cost2.data(), nC * sizeof(double)) == 0 && std::memcmp(viol.data(), viol2.data(), nC * sizeof(double)) == 0);
    for (int b = 0; b < B; ++b) {
      double ref[8];
      cddp_mc::stats(S, &cost[(size_t)b * S], &viol[(size_t)b * S], desc.viol_tol, ref);
      for (int i = 0; i < 8; ++i) wrong += !(st[(size_t)b * 8 + i] == ref[i]);
    }
    EXPECT(wrong == 0);
    EXPECT(has(thrown([&] { cddp_hip_mc_desc d2 = desc; d2.nsamp = 1025; s.planMonteCarlo(nullptr, 0, d2, nullptr, cost.data(), nullptr, nullptr); }), "nsamp = 1025"));
    EXPECT(has(thrown([&] { s.planMonteCarlo(nullptr, CDDP_HIP_MC_DEVICE, desc, nullptr, cost.data(), nullptr, nullptr); }), "cddp_hip_plan_montecarlo: cost is not device memory"));
  }
  if (fails == 0) std::printf("plan mc wrapper (%s): ok\n", gpu ? "gpu" : "cpu");
  return fails == 0 ? 0 : 1;
}
