// The RAII Plant wrapper of cddp-cpp_amd/host/cddp_hip.hpp: a refused descriptor arrives as an exception carrying the library's message
// (mode "cpu", no device needed); on a device the plant steps a small batch and substeps compose (mode "gpu").
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../cddp-cpp_amd/host/cddp_hip.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static cddp_hip_plant_desc pendulum(const double *params, int substeps, double dt) {
  cddp_hip_plant_desc d;
  std::memset(&d, 0, sizeof(d));
  d.abi_version = CDDP_HIP_ABI_VERSION; d.model = CDDP_HIP_MODEL_PENDULUM; d.integrator = CDDP_HIP_RK4; d.substeps = substeps;
  d.nx = 2; d.nu = 1; d.dt = dt; d.model_params = params;
  return d;
}

static std::string refusal(const cddp_hip_plant_desc &d, int batch) {
  try { cddp::Plant p(d, batch); } catch (const std::exception &e) { return e.what(); }
  return "";
}

int main(int argc, char **argv) {
  const bool gpu = argc > 1 && std::string(argv[1]) == "gpu";
  double params[CDDP_HIP_MAX_MODEL_PARAMS] = {0.5, 1.0, 0.01, 9.81};
  // refusals: the descriptor is checked before the device is looked at, so these are the same with and without one
  EXPECT(refusal(pendulum(params, 0, 0.02), 3).find("substeps must be at least 1") != std::string::npos);
  EXPECT(refusal(pendulum(params, 1, 0.0), 3).find("dt must be positive") != std::string::npos);
  { cddp_hip_plant_desc d = pendulum(params, 1, 0.02); d.nx = 3; EXPECT(refusal(d, 3).find("has nx = 2, nu = 1") != std::string::npos); }
  if (!gpu) {
    if (cddp_hip_device_count() == 0) EXPECT(refusal(pendulum(params, 2, 0.02), 3).find("no HIP device") != std::string::npos);
  } else {
    const int B = 70;
    std::vector<double> x((size_t)B * 2), u((size_t)B);
    for (int b = 0; b < B; ++b) { x[2 * b] = 0.01 * b; x[2 * b + 1] = 0.3 - 0.005 * b; u[b] = 0.1 * (b % 7) - 0.3; }
    cddp::Plant whole(pendulum(params, 2, 0.02), B), half(pendulum(params, 1, 0.01), B);
    EXPECT(whole.batch() == B);
    const std::vector<double> a = whole.step(x, u), h1 = half.step(x, u), b2 = half.step(h1, u);
    EXPECT(a.size() == x.size());
    for (size_t i = 0; i < a.size(); ++i) { EXPECT(std::isfinite(a[i])); EXPECT(a[i] == b2[i]); }   // two substeps of dt / 2 == two steps of a dt / 2 plant (0.02 / 2 == 0.01 exactly)
    EXPECT(a != x);
    std::vector<double> w(x.size(), 0.25);
    const std::vector<double> aw = whole.step(x, u, w);
    for (size_t i = 0; i < a.size(); ++i) EXPECT(aw[i] == a[i] + 0.25);
    bool threw = false;
    try { whole.step(std::vector<double>(3), u); } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
  }
  if (fails == 0) std::printf("plant wrapper (%s): ok\n", gpu ? "gpu" : "cpu");
  return fails == 0 ? 0 : 1;
}
