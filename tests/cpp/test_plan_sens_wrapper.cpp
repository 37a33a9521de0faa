// The plan sensitivities of cddp-cpp_amd/host/cddp_hip.hpp (HipBatchSolver::planJvp, planVjp).  Mode "cpu": without a resident batch both
// methods throw with a message, and the C entries answer the refusals that need no device.  Mode "gpu": a 2 x 1 LTI batch is solved with
// CLDDP; the forward response of the two unit vectors and the adjoint of the two unit cotangents on row N give the same 2 x 2 matrix
// dX_N / dx0 to rounding, through host pointers and through device pointers bit for bit alike; a host pointer passed as a device pointer
// and a device allocation ONE ELEMENT short are refused with their own messages and nothing is written.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../cddp-cpp_amd/host/cddp_hip.hpp"

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
    EXPECT(has(thrown([&] { s.planJvp(0, 1, v, v, v); }), "planJvp needs a resident batch"));
    EXPECT(has(thrown([&] { s.planVjp(0, 1, v, v, v); }), "planVjp needs a resident batch"));
    EXPECT(cddp_hip_plan_jvp(nullptr, 0, 1, v, v, v) != 0 && has(cddp_hip_last_error(), "cddp_hip_plan_jvp: null handle"));
    EXPECT(cddp_hip_plan_vjp(nullptr, 0, 1, v, v, v) != 0 && has(cddp_hip_last_error(), "cddp_hip_plan_vjp: null handle"));
    EXPECT(CDDP_HIP_SENS_DEVICE == 1);
  }
  if (gpu) {
    const int B = 70, N = 8, nx = 2, nu = 1, R = 2;
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
    const size_t n0 = (size_t)B * R * nx, nX = (size_t)B * R * (N + 1) * nx, nU = (size_t)B * R * N * nu;
    std::vector<double> dx0(n0, 0.0), dX(nX, -1.0), dU(nU, -1.0), gX(nX, 0.0), g0(n0, -1.0);
    for (int b = 0; b < B; ++b) for (int r = 0; r < R; ++r) {
      dx0[((size_t)b * R + r) * nx + r] = 1.0;                                // unit vector r
      gX[(((size_t)b * R + r) * (N + 1) + N) * nx + r] = 1.0;                 // unit cotangent r on row N
    }
    s.planJvp(0, R, dx0.data(), dX.data(), dU.data());
    s.planVjp(0, R, gX.data(), nullptr, g0.data());
    int wrong = 0; double big = 0.0;
    for (int b = 0; b < B; ++b) for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) {
      const double fwd = dX[(((size_t)b * R + j) * (N + 1) + N) * nx + i];   // d X_N[i] / d x0[j]
      const double adj = g0[((size_t)b * R + i) * nx + j];
      big = std::fmax(big, std::fabs(fwd));
      // two evaluation orders of one product of N factors A + B K: they differ by at most 2 N (nx + nu + 2) 2^-53 = 9e-15 times the chain on
      // absolute values (tests/test_plan_sens.py::test_adjoint_consistency evaluates that chain; here its entries stay below 100)
      wrong += !(std::fabs(fwd - adj) <= 1e-12);
      wrong += dX[(((size_t)b * R + j) * (N + 1)) * nx + i] != (i == j ? 1.0 : 0.0);   // row 0 is dx0
    }
    EXPECT(wrong == 0 && big > 1e-3);
    double *d0 = nullptr, *dXd = nullptr, *dUd = nullptr, *dshort = nullptr, *dg = nullptr;
    EXPECT(hipMalloc((void **)&d0, n0 * sizeof(double)) == hipSuccess && hipMalloc((void **)&dXd, nX * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dUd, nU * sizeof(double)) == hipSuccess && hipMalloc((void **)&dshort, (nX - 1) * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc((void **)&dg, n0 * sizeof(double)) == hipSuccess);
    if (fails == 0) {
      EXPECT(hipMemcpy(d0, dx0.data(), n0 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
      EXPECT(hipMemset(dXd, 0, nX * sizeof(double)) == hipSuccess && hipMemset(dshort, 0, (nX - 1) * sizeof(double)) == hipSuccess);
      // refusals first, so that "nothing written" can be seen in the zeroed arrays
      EXPECT(has(thrown([&] { s.planJvp(CDDP_HIP_SENS_DEVICE, R, dx0.data(), dXd, dUd); }), "cddp_hip_plan_jvp: dx0 is not device memory"));
      EXPECT(has(thrown([&] { s.planJvp(CDDP_HIP_SENS_DEVICE, R, d0, dshort, dUd); }), "cddp_hip_plan_jvp: dX needs"));
      EXPECT(has(std::string(cddp_hip_last_error()), "its allocation ends after"));
      EXPECT(has(thrown([&] { s.planVjp(CDDP_HIP_SENS_DEVICE, R, dshort, nullptr, dg); }), "cddp_hip_plan_vjp: gX needs"));
      EXPECT(has(thrown([&] { s.planJvp(CDDP_HIP_SENS_DEVICE | 4, R, d0, dXd, dUd); }), "unknown flag bits"));
      EXPECT(has(thrown([&] { s.planJvp(CDDP_HIP_SENS_DEVICE, 0, d0, dXd, dUd); }), "nvec = 0"));
      std::vector<double> back(nX, -1.0);
      EXPECT(hipMemcpy(back.data(), dXd, nX * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      for (double v : back) wrong += v != 0.0;
      EXPECT(wrong == 0);
      // device pointers: the bits of the host-pointer call
      s.planJvp(CDDP_HIP_SENS_DEVICE, R, d0, dXd, dUd);
      std::vector<double> backU(nU, -1.0);
      EXPECT(hipMemcpy(back.data(), dXd, nX * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(backU.data(), dUd, nU * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      EXPECT(std::memcmp(back.data(), dX.data(), nX * sizeof(double)) == 0 && std::memcmp(backU.data(), dU.data(), nU * sizeof(double)) == 0);
      EXPECT(hipMemcpy(dXd, gX.data(), nX * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
      s.planVjp(CDDP_HIP_SENS_DEVICE, R, dXd, nullptr, dg);
      std::vector<double> backg(n0, -1.0);
      EXPECT(hipMemcpy(backg.data(), dg, n0 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
      EXPECT(std::memcmp(backg.data(), g0.data(), n0 * sizeof(double)) == 0);
    }
    for (void *q : {(void *)d0, (void *)dXd, (void *)dUd, (void *)dshort, (void *)dg}) (void)hipFree(q);
  }
  if (fails == 0) std::printf("plan sens wrapper (%s): ok\n", gpu ? "gpu" : "cpu");
  return fails == 0 ? 0 : 1;
}
