// The device-resident inputs and outputs of cddp-cpp_amd/host/cddp_hip.hpp (HipBatchSolver::fieldShape, getFieldDevice, resultsDevice,
// setInitialDevice, resolveBatch).  Mode "cpu": without a resident batch every method throws with a message, and the C entries refuse a NULL
// handle.  Mode "gpu": a pendulum batch is solved, its fields read into hipMalloc'ed arrays equal the host solutions bit for bit, a seed
// given from device arrays re-solves to the bits of a solver seeded from the host, and a host pointer, a pinned host pointer and an
// allocation that is too short are refused.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../cddp-cpp_amd/host/cddp_hip.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { if (fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static const double kPi = 3.14159265358979323846;

static cddp::CDDP makePendulum(const cddp::CDDPOptions &options, int horizon) {
  const double dt = 0.02;
  cddp::Vector x0 = {kPi, 0.0}, goal = {0.0, 0.0};
  cddp::Matrix Q = cddp::Matrix::Zero(2, 2), R = 0.1 * cddp::Matrix::Identity(1), Qf = 100.0 * cddp::Matrix::Identity(2);
  cddp::CDDP solver(x0, goal, horizon, dt, std::make_unique<cddp::Pendulum>(dt, 0.5, 1.0, 0.01, "euler"),
                    std::make_unique<cddp::QuadraticObjective>(Q, R, Qf, goal, std::vector<cddp::Vector>{}, dt), options);
  solver.addPathConstraint("ControlConstraint", std::make_unique<cddp::ControlConstraint>(cddp::Vector{-20.0}, cddp::Vector{20.0}));
  std::vector<cddp::Vector> X(horizon + 1, x0), U(horizon, cddp::Vector{0.0});
  solver.setInitialTrajectory(X, U);
  return solver;
}

template <class F> static std::string thrown(F f) {
  try { f(); } catch (const std::exception &e) { return e.what(); }
  return "";
}

static bool sameSolutions(const std::vector<cddp::CDDPSolution> &a, const std::vector<cddp::CDDPSolution> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    if (a[i].iterations_completed != b[i].iterations_completed || a[i].status_message != b[i].status_message) return false;
    if (std::memcmp(&a[i].final_objective, &b[i].final_objective, sizeof(double))) return false;
    if (a[i].state_trajectory != b[i].state_trajectory || a[i].control_trajectory != b[i].control_trajectory) return false;
  }
  return true;
}

int main(int argc, char **argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  {   // no resident batch yet: every method says so; the C entries refuse a NULL handle
    cddp::HipBatchSolver s(CDDP_HIP_SOLVER_IPDDP);
    EXPECT(thrown([&] { s.fieldShape(CDDP_HIP_FIELD_X); }).find("needs a resident batch") != std::string::npos);
    EXPECT(thrown([&] { s.getFieldDevice(CDDP_HIP_FIELD_X, nullptr); }).find("needs a resident batch") != std::string::npos);
    EXPECT(thrown([&] { s.resultsDevice(nullptr, nullptr); }).find("needs a resident batch") != std::string::npos);
    EXPECT(thrown([&] { s.setInitialDevice(nullptr); }).find("needs a resident batch") != std::string::npos);
    EXPECT(cddp_hip_get_field_device(nullptr, CDDP_HIP_FIELD_X, nullptr) != 0 && std::string(cddp_hip_last_error()).find("null handle") != std::string::npos);
    EXPECT(cddp_hip_set_initial_device(nullptr, nullptr, nullptr, nullptr) != 0 && std::string(cddp_hip_last_error()).find("null handle") != std::string::npos);
    EXPECT(CDDP_HIP_FIELD_X == 0 && CDDP_HIP_FIELD_LAMBDA == 11);
  }
  if (gpu) {
    const int B = 70, N = 37, nx = 2, nu = 1;
    cddp::CDDPOptions opt; opt.max_iterations = 30; opt.verbose = false;
    std::vector<cddp::Vector> x0s;
    for (int b = 0; b < B; ++b) x0s.push_back({kPi - 0.03 * b, 0.02 * b});
    cddp::CDDP ctx = makePendulum(opt, N);
    cddp::HipBatchSolver s(CDDP_HIP_SOLVER_IPDDP);
    const std::vector<cddp::CDDPSolution> sols = s.solveBatch(ctx, x0s);
    EXPECT((int)sols.size() == B && s.batch() == B);
    const cddp::HipBatchSolver::FieldShape fx = s.fieldShape(CDDP_HIP_FIELD_X), fu = s.fieldShape(CDDP_HIP_FIELD_U), fk = s.fieldShape(CDDP_HIP_FIELD_K);
    EXPECT(fx.rows == N + 1 && fx.cols == nx && fu.rows == N && fu.cols == nu && fk.rows == N && fk.cols == nu * nx);
    const size_t nX = (size_t)B * (N + 1) * nx, nU = (size_t)B * N * nu;
    double *dX = nullptr, *dU = nullptr, *dcols = nullptr, *dx0 = nullptr, *dshort = nullptr, *pinned = nullptr;
    int32_t *dicols = nullptr;
    EXPECT(hipMalloc((void **)&dX, nX * sizeof(double)) == hipSuccess && hipMalloc((void **)&dU, nU * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dcols, (size_t)B * 10 * sizeof(double)) == hipSuccess && hipMalloc((void **)&dicols, (size_t)B * 4 * sizeof(int32_t)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dx0, (size_t)B * nx * sizeof(double)) == hipSuccess && hipMalloc((void **)&dshort, nX * sizeof(double) / 2) == hipSuccess);
    EXPECT(hipHostMalloc((void **)&pinned, nX * sizeof(double), hipHostMallocDefault) == hipSuccess);
    if (fails == 0) {
      s.getFieldDevice(CDDP_HIP_FIELD_X, dX); s.getFieldDevice(CDDP_HIP_FIELD_U, dU); s.resultsDevice(dcols, dicols);
      std::vector<double> X(nX), U(nU), cols((size_t)B * 10);
      std::vector<int32_t> icols((size_t)B * 4);
      EXPECT(hipMemcpy(X.data(), dX, nX * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(U.data(), dU, nU * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      EXPECT(hipMemcpy(cols.data(), dcols, cols.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      EXPECT(hipMemcpy(icols.data(), dicols, icols.size() * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess);
      int wrong = 0;
      for (int b = 0; b < B; ++b) {
        for (int t = 0; t <= N; ++t) for (int i = 0; i < nx; ++i) wrong += std::memcmp(&X[((size_t)b * (N + 1) + t) * nx + i], &sols[b].state_trajectory[t][i], sizeof(double)) != 0;
        for (int t = 0; t < N; ++t) for (int i = 0; i < nu; ++i) wrong += std::memcmp(&U[((size_t)b * N + t) * nu + i], &sols[b].control_trajectory[t][i], sizeof(double)) != 0;
        wrong += std::memcmp(&cols[(size_t)b * 10], &sols[b].final_objective, sizeof(double)) != 0;
        wrong += icols[(size_t)b * 4] != sols[b].iterations_completed;
        wrong += std::string(cddp_hip_status_string(icols[(size_t)b * 4 + 1])) != sols[b].status_message;
      }
      EXPECT(wrong == 0);
      // refusals: a host pointer, a pinned host pointer, an allocation of half the bytes; nothing is launched
      EXPECT(thrown([&] { s.getFieldDevice(CDDP_HIP_FIELD_X, X.data()); }).find("not device memory") != std::string::npos);
      std::memset(pinned, 0, nX * sizeof(double));
      EXPECT(thrown([&] { s.getFieldDevice(CDDP_HIP_FIELD_X, pinned); }).find("not device memory") != std::string::npos);
      EXPECT(pinned[0] == 0.0 && pinned[nX - 1] == 0.0);
      EXPECT(thrown([&] { s.getFieldDevice(CDDP_HIP_FIELD_X, dshort); }).find("its allocation ends after") != std::string::npos);
      EXPECT(thrown([&] { s.setInitialDevice(dx0, nullptr, dshort); }).find("its allocation ends after") != std::string::npos);
      EXPECT(thrown([&] { s.setInitialDevice(pinned); }).find("x0 is not device memory") != std::string::npos);
      EXPECT(thrown([&] { s.getFieldDevice(99, dX); }).find("unknown field id 99") != std::string::npos);
      // the seed from device arrays: the solved plan as X0 / U0, x0 as before -- against a second solver object seeded from the host
      std::vector<double> x0((size_t)B * nx);
      for (int b = 0; b < B; ++b) for (int i = 0; i < nx; ++i) x0[(size_t)b * nx + i] = x0s[b][i];
      EXPECT(hipMemcpy(dx0, x0.data(), x0.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
      s.setInitialDevice(dx0, dU, dX);
      const std::vector<cddp::CDDPSolution> again = s.resolveBatch(ctx);
      cddp::CDDP ctx2 = makePendulum(opt, N);
      cddp::HipBatchSolver s2(CDDP_HIP_SOLVER_IPDDP);
      s2.solveBatch(ctx2, x0s);
      {   // (the host seed through the C entry the wrapper's upload uses; the handle is the wrapper's own)
        cddp_hip_handle *h2 = s2.handle();
        EXPECT(h2 != nullptr);
        if (h2) cddp::HipBatchSolver::check(cddp_hip_set_initial(h2, x0.data(), U.data(), X.data()));
      }
      const std::vector<cddp::CDDPSolution> host_again = s2.resolveBatch(ctx2);
      EXPECT(sameSolutions(again, host_again));
    }
    for (void *q : {(void *)dX, (void *)dU, (void *)dcols, (void *)dicols, (void *)dx0, (void *)dshort}) (void)hipFree(q);
    (void)hipHostFree(pinned);
  }
  if (fails == 0) std::printf("device io wrapper (%s): ok\n", gpu ? "gpu" : "cpu");
  return fails == 0 ? 0 : 1;
}
