// The step bodies of the extended Kalman filter (cddp-cpp_amd/csrc/ekf.hpp) on the host: a stand-alone program that walks a few
// trajectories through update / predict exactly as k_ekf_walk (inst_ekf.hip) does -- with the host build of the model structs of
// dev_models.hpp, as host_models.cpp compiles them -- and writes every case's inputs and results to a file, which
// tests/test_ekf_host.py holds to tests/plan_ekf_ref.py bit for bit.  Built with g++ -ffp-contract=off -DCDDP_TRIG_SHARED=1, plainly and
// with -fsanitize=address,undefined.
#define CDDP_HOST_MODELS 1
#define CDDP_TRIG_HOST 1
#define DEV inline
#include "../../cddp-cpp_amd/csrc/dev_models.hpp"
#include "../../cddp-cpp_amd/csrc/ekf.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace cddp_dev;

namespace {

struct Rng {   // a fixed 64-bit LCG: uniform in [-1, 1)
  uint64_t s;
  double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(int64_t)(s >> 11) / (double)(1ULL << 52) - 1.0; }
};

void put(FILE *f, const char *name, const std::vector<double> &v) {
  std::fprintf(f, "%s %zu", name, v.size());
  for (double x : v) std::fprintf(f, " %a", x);
  std::fprintf(f, "\n");
}

template <class M>
int run_case(FILE *f, int model, int ny, int have_w, int have_wu, int box, int dropout, int failing, const std::vector<double> &params, double dt, uint64_t seed) {
  constexpr int NX = M::NX, NU = M::NU, B = 3, T = 3, INTEG = CDDP_HIP_RK4;
  Rng rng{seed};
  std::vector<double> xh0(B * NX), P0(B * NX * NX), C(ny * NX), v(ny), W(NX * NX), Wu(NU * NU), Y(B * (T + 1) * ny), U(B * T * NU), lower(NU), upper(NU);
  for (double &x : xh0) x = 0.3 * rng.next();
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < NX; ++i)
      for (int j = 0; j < NX; ++j)   // the lower triangle is the matrix; what is above the diagonal is junk that must not be read
        P0[(b * NX + i) * NX + j] = j > i ? 7.0 + rng.next() : (i == j ? 0.5 + 0.1 * rng.next() : 0.02 * rng.next());
  if (failing)
    for (int i = 0; i < NX; ++i)
      for (int j = 0; j <= i; ++j) P0[(1 * NX + i) * NX + j] = i == j ? -1.0 : 0.0;
  for (double &x : C) x = rng.next();
  for (double &x : v) x = failing ? 1e-3 : 0.05 + 0.5 * (rng.next() + 1.0);
  for (int i = 0; i < NX; ++i)
    for (int j = 0; j < NX; ++j) W[i * NX + j] = j > i ? -3.0 : (i == j ? 0.01 + 0.002 * rng.next() : 0.0005 * rng.next());
  for (int i = 0; i < NU; ++i)
    for (int j = 0; j < NU; ++j) Wu[i * NU + j] = j > i ? 5.0 : (i == j ? 0.02 + 0.004 * rng.next() : 0.001 * rng.next());
  for (double &x : Y) x = 0.5 * rng.next();
  for (double &x : U) x = rng.next();
  if (dropout) { Y[(0 * (T + 1) + 1) * ny + 0] = std::nan(""); Y[(2 * (T + 1) + 0) * ny + (ny - 1)] = std::nan(""); }
  for (int i = 0; i < NU; ++i) { lower[i] = -0.4 - 0.05 * i; upper[i] = 0.3 + 0.05 * i; }
  double p[32];
  for (int i = 0; i < 32; ++i) p[i] = i < (int)params.size() ? params[i] : 0.0;

  std::vector<double> Xh(B * (T + 1) * NX), Pout(B * (T + 1) * NX * NX), nis(B * (T + 1)), info(B), xhN(B * NX), PN(B * NX * NX);
  const double nan = std::nan("");
  for (int b = 0; b < B; ++b) {
    double xh[NX], Pm[NX * NX], Am[NX * NX], Ym[NX * NX], Bm[NX * NU];
    const cddp_ekf::Mat<1> P{Pm, NX}, A{Am, NX}, Yb{Ym, NX}, Bb{Bm, NU};
    for (int i = 0; i < NX; ++i) xh[i] = xh0[b * NX + i];
    for (int i = 0; i < NX; ++i)
      for (int j = 0; j <= i; ++j) { const double q = P0[(b * NX + i) * NX + j]; Pm[i * NX + j] = q; Pm[j * NX + i] = q; }
    const cddp_cov::SymLower Ws{have_w ? W.data() : nullptr, NX}, Wus{have_wu ? Wu.data() : nullptr, NU};
    int inf = 0;
    for (int t = 0; t <= T; ++t) {
      if (t > 0) {
        double u[NU];
        for (int i = 0; i < NU; ++i) u[i] = U[(b * T + t - 1) * NU + i];
        cddp_ekf::predict<M, Stepper<M>, 1>(INTEG, dt, p, box ? lower.data() : nullptr, box ? upper.data() : nullptr, xh, u, P, A, Bb, Yb, Ws, Wus);
      }
      const int row = b * (T + 1) + t;
      double n = 0.0;
      for (int r = 0; r < ny; ++r) {
        const int rc = cddp_ekf::update_row<NX, 1>(cddp_kf::Row{C.data() + r * NX}, v[r], Y[row * ny + r], dropout != 0, xh, P, n);
        if (rc == cddp_ekf::kRowFailed && inf == 0) inf = t + 1;
      }
      for (int i = 0; i < NX; ++i) Xh[row * NX + i] = inf ? nan : xh[i];
      for (int i = 0; i < NX * NX; ++i) Pout[row * NX * NX + i] = inf ? nan : Pm[i];
      nis[row] = inf ? nan : n;
    }
    info[b] = inf;
    for (int i = 0; i < NX; ++i) xhN[b * NX + i] = inf ? nan : xh[i];
    for (int i = 0; i < NX * NX; ++i) PN[b * NX * NX + i] = inf ? nan : Pm[i];
  }
  std::fprintf(f, "case %d %d %d %d %d %d %d %d %d %d %d %d\n", model, NX, NU, ny, B, T, INTEG, have_w, have_wu, box, dropout, failing);
  put(f, "params", params); put(f, "dt", {dt}); put(f, "xh0", xh0); put(f, "P0", P0); put(f, "C", C); put(f, "v", v); put(f, "W", W); put(f, "Wu", Wu);
  put(f, "Y", Y); put(f, "U", U); put(f, "lower", lower); put(f, "upper", upper);
  put(f, "Xh", Xh); put(f, "P", Pout); put(f, "nis", nis); put(f, "info", info); put(f, "xhN", xhN); put(f, "PN", PN);
  return 1;
}

template <class M>
int run_model(FILE *f, int model, const std::vector<double> &params, double dt, uint64_t seed) {
  constexpr int NX = M::NX;
  const int nys[4] = {1, NX, NX + 2, 16};
  int n = 0;
  for (int k = 0; k < 4; ++k)   // W / Wu: all four combinations; a box on ny = 1 and 16; the drop-outs at ny = nx; the failing pivot at ny = nx + 2
    n += run_case<M>(f, model, nys[k], k & 1, (k >> 1) & 1, k == 0 || k == 3, k == 1, k == 2, params, dt, seed + 977 * k);
  return n;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s OUT\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "w");
  if (!f) { std::perror(argv[1]); return 2; }
  int n = 0;
  n += run_model<PendulumModel>(f, CDDP_HIP_MODEL_PENDULUM, {0.5, 1.0, 0.01, 9.81}, 0.02, 20261021);
  n += run_model<CartPoleModel>(f, CDDP_HIP_MODEL_CARTPOLE, {1.0, 0.2, 0.5, 9.81, 0.0}, 0.05, 20261022);
  n += run_model<Manip7Model>(f, CDDP_HIP_MODEL_MANIPULATOR7, {}, 0.01, 20261023);
  std::fclose(f);
  std::printf("ekf: ok (%d cases)\n", n);
  return 0;
}
