// Scoring and seeding through cddp-cpp_amd/host/cddp_hip.hpp (HipBatchSolver::scoreRollouts, seedBest).  Mode "cpu": without a resident
// batch both methods throw with a message, and the C entries answer the refusals that need no device.  Mode "gpu": a 2 x 1 LTI batch is
// solved with CLDDP; three candidate control sequences per trajectory are scored through host pointers and through device pointers bit
// for bit alike, the cost of every candidate is the objective written out on the returned states, the winners follow the rule of
// csrc/score_select.hpp, a re-solve from the seed runs, and a host pointer passed as a device pointer and a device allocation ONE ELEMENT
// short are refused with their own messages and nothing is written.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../cddp-cpp_amd/host/cddp_hip.hpp"
#include "../../cddp-cpp_amd/csrc/score_select.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { if (fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

template <class F> static std::string thrown(F f) {
  try { f(); } catch (const std::exception &e) { return e.what(); }
  return "";
}
static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main(int argc, char **argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  {
    cddp::HipBatchSolver s(CDDP_HIP_SOLVER_CLDDP);
    double v[4] = {0, 0, 0, 0};
    EXPECT(has(thrown([&] { s.scoreRollouts(nullptr, 0, 1, v, v, v); }), "scoreRollouts needs a resident batch"));
    EXPECT(has(thrown([&] { s.seedBest(0, 1, v, v, v, nullptr, 0.0); }), "seedBest needs a resident batch"));
    EXPECT(cddp_hip_score_rollouts(nullptr, nullptr, 0, 1, v, v, v, nullptr, nullptr, nullptr) != 0 && has(cddp_hip_last_error(), "cddp_hip_score_rollouts: null handle"));
    EXPECT(cddp_hip_seed_best(nullptr, 0, 1, v, v, v, nullptr, 0.0, nullptr) != 0 && has(cddp_hip_last_error(), "cddp_hip_seed_best: null handle"));
    EXPECT(CDDP_HIP_SCORE_DEVICE == 1 && CDDP_HIP_SCORE_FEEDBACK == 2 && CDDP_HIP_SCORE_X0_PER_CANDIDATE == 4);
  }
  if (gpu) {
    const int B = 70, N = 8, nx = 2, nu = 1, S = 3;
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
    const size_t n0 = (size_t)B * nx, nU = (size_t)B * S * N * nu, nX = (size_t)B * S * (N + 1) * nx, nC = (size_t)B * S;
    std::vector<double> xs(n0), U(nU), cost(nC, -1.0), viol(nC, -1.0), X(nX, -1.0);
    for (int b = 0; b < B; ++b) { xs[(size_t)b * nx] = x0s[b][0]; xs[(size_t)b * nx + 1] = x0s[b][1]; }
    for (size_t i = 0; i < nU; ++i) U[i] = 0.5 * std::sin(0.37 * (double)i) * (double)(1 + (i / (N * nu)) % S);
    s.scoreRollouts(nullptr, 0, S, xs.data(), U.data(), cost.data(), viol.data(), X.data());
    int wrong = 0;
    for (int b = 0; b < B; ++b) for (int c = 0; c < S; ++c) {
      const size_t g = (size_t)b * S + c;
      const double *Xg = &X[g * (N + 1) * nx], *Ug = &U[g * N * nu];
      double J = 0.0;
      for (int t = 0; t < N; ++t) {   // Q dt = dt I, R dt = 0.3 dt: (e^T Q dt) e + (u^T R dt) u in the header's order, x_ref = 0
        double sx = 0.0;
        for (int j = 0; j < nx; ++j) { double r = 0.0; for (int i = 0; i < nx; ++i) r += Xg[t * nx + i] * ((i == j ? 1.0 : 0.0) * dt); sx += r * Xg[t * nx + j]; }
        double su = 0.0;
        { double r = 0.0; r += Ug[t] * (0.3 * dt); su += r * Ug[t]; }
        J += sx + su;
      }
      double sx = 0.0;
      for (int j = 0; j < nx; ++j) { double r = 0.0; for (int i = 0; i < nx; ++i) r += Xg[N * nx + i] * (i == j ? 5.0 : 0.0); sx += r * Xg[N * nx + j]; }
      J += sx;
      wrong += !(cost[g] == J) + !(viol[g] == 0.0) + !(Xg[0] == xs[(size_t)b * nx] && Xg[1] == xs[(size_t)b * nx + 1]);
    }
    EXPECT(wrong == 0);
    std::vector<int32_t> win(B, -2);
    s.seedBest(0, S, xs.data(), U.data(), cost.data(), viol.data(), 0.0, win.data());
    int distinct[3] = {0, 0, 0};
    for (int b = 0; b < B; ++b) {
      wrong += win[b] != cddp_score::select(S, &cost[(size_t)b * S], &viol[(size_t)b * S], 0.0);
      if (win[b] >= 0 && win[b] < S) ++distinct[win[b]];
    }
    EXPECT(wrong == 0);
    const std::vector<cddp::CDDPSolution> again = s.resolveBatch(ctx);
    EXPECT((int)again.size() == B);
    double *dx = nullptr, *dU = nullptr, *dc = nullptr, *dv = nullptr, *dX = nullptr, *dshort = nullptr;
    EXPECT(hipMalloc((void **)&dx, n0 * sizeof(double)) == hipSuccess && hipMalloc((void **)&dU, nU * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dc, nC * sizeof(double)) == hipSuccess && hipMalloc((void **)&dv, nC * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dX, nX * sizeof(double)) == hipSuccess && hipMalloc((void **)&dshort, (nC - 1) * sizeof(double)) == hipSuccess);
    if (fails == 0) {
      EXPECT(hipMemcpy(dx, xs.data(), n0 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dU, U.data(), nU * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
      EXPECT(hipMemset(dc, 0, nC * sizeof(double)) == hipSuccess && hipMemset(dshort, 0, (nC - 1) * sizeof(double)) == hipSuccess);
      EXPECT(has(thrown([&] { s.scoreRollouts(nullptr, CDDP_HIP_SCORE_DEVICE, S, xs.data(), dU, dc); }), "cddp_hip_score_rollouts: x0 is not device memory"));
      EXPECT(has(thrown([&] { s.scoreRollouts(nullptr, CDDP_HIP_SCORE_DEVICE, S, dx, dU, dshort); }), "cddp_hip_score_rollouts: cost needs"));
      EXPECT(has(std::string(cddp_hip_last_error()), "its allocation ends after"));
      EXPECT(has(thrown([&] { s.seedBest(CDDP_HIP_SCORE_DEVICE, S, dx, dU, dshort, nullptr, 0.0); }), "cddp_hip_seed_best: cost needs"));
      EXPECT(has(thrown([&] { s.scoreRollouts(nullptr, 0, 0, xs.data(), U.data(), cost.data()); }), "ncand = 0"));
      std::vector<double> back(nC, -1.0);
      EXPECT(hipMemcpy(back.data(), dc, nC * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      for (double v : back) wrong += v != 0.0;
      EXPECT(wrong == 0);
      s.scoreRollouts(nullptr, CDDP_HIP_SCORE_DEVICE, S, dx, dU, dc, dv, dX);
      std::vector<double> backv(nC, -1.0), backX(nX, -1.0);
      EXPECT(hipMemcpy(back.data(), dc, nC * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(backv.data(), dv, nC * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      EXPECT(hipMemcpy(backX.data(), dX, nX * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      EXPECT(std::memcmp(back.data(), cost.data(), nC * sizeof(double)) == 0 && std::memcmp(backv.data(), viol.data(), nC * sizeof(double)) == 0);
      EXPECT(std::memcmp(backX.data(), X.data(), nX * sizeof(double)) == 0);
    }
    for (void *q : {(void *)dx, (void *)dU, (void *)dc, (void *)dv, (void *)dX, (void *)dshort}) (void)hipFree(q);
  }
  if (fails == 0) std::printf("score wrapper (%s): ok\n", gpu ? "gpu" : "cpu");
  return fails == 0 ? 0 : 1;
}
