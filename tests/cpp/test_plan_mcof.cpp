// The arithmetic the output-feedback Monte-Carlo evaluation adds (cddp-cpp_amd/csrc/plan_mcof.hpp) on the host: the element-index map of the
// measurement normals (past the end of plan_mc.hpp's, for every step), steps 2 to 6 of the header on written-out sums -- the innovations
// formed before the update touches the estimate, the update's sum over the rows, the feedback, the prediction as one sum over A's and B's
// terms, with strided matrices as the kernel reads the stacks -- and keep_nominal.
// Stand-alone: built by tests/test_plan_mcof_host.py with g++ -ffp-contract=off, plainly and with -fsanitize=address,undefined.
// Usage: test_plan_mcof                                                  the checks
//        test_plan_mcof noise IN OUT seed stream B S N nx nu ny keep     IN: v [ny]; OUT: Yn [B][S][N+1][ny] as the library lays it out
//        test_plan_mcof estimate IN OUT n T nx nu ny                     the estimator's lines on given signals, n samples over T steps:
//                 IN: C [ny][nx] | L [T+1][nx][ny] | K [T][nu][nx] | A [T][nx][nx] | Bm [T][nx][nu] | DX [n][T+1][nx] | Yn [n][T+1][ny]
//                 OUT: Xh [n][T+1][nx] (after the update of step t) | FB [n][T][nu] | XP [n][T][nx] (the prediction made at step t)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cddp-cpp_amd/csrc/plan_mcof.hpp"

namespace {

int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

using Vec = std::vector<double>;
bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double rnd() {   // uniform in [-1, 1): a 64-bit LCG, its top 53 bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

void check_index_map() {
  const int shapes[3][4] = {{2, 1, 5, 1}, {3, 2, 4, 16}, {14, 7, 3, 15}};   // nx, nu, N, ny
  for (const auto &s : shapes) {
    const int nx = s[0], nu = s[1], N = s[2], ny = s[3];
    uint32_t last = 0;   // the largest element of plan_mc.hpp's walk
    for (int i = 0; i < nx; ++i) last = cddp_mc::elem_x0(i) > last ? cddp_mc::elem_x0(i) : last;
    for (int t = 0; t < N; ++t) {
      for (int i = 0; i < nu; ++i) last = cddp_mc::elem_u(nx, nu, t, i) > last ? cddp_mc::elem_u(nx, nu, t, i) : last;
      for (int i = 0; i < nx; ++i) last = cddp_mc::elem_w(nx, nu, t, i) > last ? cddp_mc::elem_w(nx, nu, t, i) : last;
    }
    uint32_t e = last + 1;   // the measurement elements follow without a gap, t then r ascending
    for (int t = 0; t <= N; ++t)
      for (int r = 0; r < ny; ++r) CHECK(cddp_mcof::elem_y(nx, nu, N, ny, t, r) == e++);
  }
  // the second walk draws what normal() gives, and keep_nominal zeroes it
  const uint64_t seed = 0x1234567890ull;
  cddp_mc::Draw dm;
  dm.begin(seed, 3, 7, 9, false);
  for (int t = 0; t <= 5; ++t) { const uint32_t e = cddp_mcof::elem_y(2, 1, 5, 1, t, 0); CHECK(e == (uint32_t)(17 + t)); CHECK(same(dm.get(e), cddp_mppi::normal(seed, 3, 7, 9, e))); }
  dm.begin(seed, 3, 7, 0, true);
  for (int t = 0; t <= 5; ++t) CHECK(dm.get(cddp_mcof::elem_y(2, 1, 5, 1, t, 0)) == 0.0);
}

// steps 2 to 6 at (nx, nu, ny) = (3, 2, 2), the matrices read with stride st (1: a host array; 4, 64: a stack in place)
void check_steps(int st) {
  const int nx = 3, nu = 2, ny = 2;
  Vec C(ny * nx), L(nx * ny), dx(nx), xh(nx), n(ny);
  for (double &x : C) x = rnd();
  for (double &x : L) x = rnd();
  for (double &x : dx) x = rnd();
  for (double &x : xh) x = rnd();
  for (double &x : n) x = 0.1 * rnd();
  Vec K((size_t)nu * nx * st, std::nan("")), A((size_t)nx * nx * st, std::nan("")), Bm((size_t)nx * nu * st, std::nan(""));   // between the strides: not read
  for (int k = 0; k < nu * nx; ++k) K[(size_t)k * st] = rnd();
  for (int k = 0; k < nx * nx; ++k) A[(size_t)k * st] = rnd();
  for (int k = 0; k < nx * nu; ++k) Bm[(size_t)k * st] = rnd();
  auto Ke = [&](int i, int j) { return K[(size_t)(i * nx + j) * st]; };
  auto Ae = [&](int i, int j) { return A[(size_t)(i * nx + j) * st]; };
  auto Be = [&](int i, int j) { return Bm[(size_t)(i * nu + j) * st]; };
  const Vec xh0 = xh;
  // steps 2 and 3, written out
  double inn[2];
  for (int r = 0; r < ny; ++r) {
    const double y = (((0.0 + C[r * nx] * dx[0]) + C[r * nx + 1] * dx[1]) + C[r * nx + 2] * dx[2]) + n[r];
    const double p = ((0.0 + C[r * nx] * xh0[0]) + C[r * nx + 1] * xh0[1]) + C[r * nx + 2] * xh0[2];
    inn[r] = y - p;
    CHECK(same(cddp_mcof::innovation(nx, C.data() + r * nx, n[r], dx.data(), xh.data()), inn[r]));
  }
  // step 4: every innovation from the estimate before the update
  Vec acc(nx, 0.0);
  for (int r = 0; r < ny; ++r) cddp_mcof::update_add(nx, ny, r, L.data(), cddp_mcof::innovation(nx, C.data() + r * nx, n[r], dx.data(), xh.data()), acc.data());
  cddp_mcof::update_end(nx, acc.data(), xh.data());
  for (int i = 0; i < nx; ++i) CHECK(same(xh[i], xh0[i] + ((0.0 + L[i * ny] * inn[0]) + L[i * ny + 1] * inn[1])));
  CHECK(!same(xh[0], xh0[0]));
  // step 6
  double fb[2], xp[3];
  cddp_mcof::feedback(nx, nu, K.data(), st, xh.data(), fb);
  for (int i = 0; i < nu; ++i) CHECK(same(fb[i], ((0.0 + Ke(i, 0) * xh[0]) + Ke(i, 1) * xh[1]) + Ke(i, 2) * xh[2]));
  cddp_mcof::predict(nx, nu, A.data(), Bm.data(), st, xh.data(), fb, xp);
  for (int i = 0; i < nx; ++i)
    CHECK(same(xp[i], ((((0.0 + Ae(i, 0) * xh[0]) + Ae(i, 1) * xh[1]) + Ae(i, 2) * xh[2]) + Be(i, 0) * fb[0]) + Be(i, 1) * fb[1]));
  // one sum, not A xh + (B fb): the two differ in the last bit for some row of a random draw, or the check above would not tell them apart
  int differs = 0;
  for (int k = 0; k < 64 && !differs; ++k) {
    double a[3], b[2], h[3], f[2];
    for (double &x : a) x = rnd();
    for (double &x : b) x = rnd();
    for (double &x : h) x = rnd();
    for (double &x : f) x = rnd();
    const double one = ((((0.0 + a[0] * h[0]) + a[1] * h[1]) + a[2] * h[2]) + b[0] * f[0]) + b[1] * f[1];
    const double two = (((0.0 + a[0] * h[0]) + a[1] * h[1]) + a[2] * h[2]) + ((0.0 + b[0] * f[0]) + b[1] * f[1]);
    differs = !same(one, two);
  }
  CHECK(differs);
}

bool read_all(const char *path, Vec &v) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  const bool ok = std::fread(v.data(), sizeof(double), v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}
bool write_all(const char *path, const Vec &v) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

int noise_mode(int argc, char **argv) {
  if (argc != 13) { std::printf("usage: test_plan_mcof noise IN OUT seed stream B S N nx nu ny keep\n"); return 2; }
  const uint64_t seed = std::strtoull(argv[4], nullptr, 0);
  const uint32_t stream = (uint32_t)std::strtoul(argv[5], nullptr, 0);
  const int B = std::atoi(argv[6]), S = std::atoi(argv[7]), N = std::atoi(argv[8]), nx = std::atoi(argv[9]), nu = std::atoi(argv[10]), ny = std::atoi(argv[11]);
  const bool keep = std::atoi(argv[12]) != 0;
  Vec v(ny), sd(ny);
  if (!read_all(argv[2], v)) { std::printf("cannot read %s\n", argv[2]); return 2; }
  for (int r = 0; r < ny; ++r) sd[r] = std::sqrt(v[r]);
  Vec Yn((size_t)B * S * (N + 1) * ny);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < S; ++c) {
      cddp_mc::Draw dm;
      dm.begin(seed, stream, (uint32_t)b, (uint32_t)c, keep && c == 0);
      double *out = &Yn[((size_t)b * S + c) * (N + 1) * ny];
      for (int t = 0; t <= N; ++t)
        for (int r = 0; r < ny; ++r) out[t * ny + r] = sd[r] * dm.get(cddp_mcof::elem_y(nx, nu, N, ny, t, r));
    }
  if (!write_all(argv[3], Yn)) { std::printf("cannot write %s\n", argv[3]); return 2; }
  return 0;
}

int estimate_mode(int argc, char **argv) {
  if (argc != 9) { std::printf("usage: test_plan_mcof estimate IN OUT n T nx nu ny\n"); return 2; }
  const int n = std::atoi(argv[4]), T = std::atoi(argv[5]), nx = std::atoi(argv[6]), nu = std::atoi(argv[7]), ny = std::atoi(argv[8]);
  const size_t oC = 0, oL = oC + (size_t)ny * nx, oK = oL + (size_t)(T + 1) * nx * ny, oA = oK + (size_t)T * nu * nx, oB = oA + (size_t)T * nx * nx,
               oD = oB + (size_t)T * nx * nu, oY = oD + (size_t)n * (T + 1) * nx, total = oY + (size_t)n * (T + 1) * ny;
  Vec in(total);
  if (!read_all(argv[2], in)) { std::printf("cannot read %s\n", argv[2]); return 2; }
  const size_t nH = (size_t)n * (T + 1) * nx, nF = (size_t)n * T * nu, nP = (size_t)n * T * nx;
  Vec out(nH + nF + nP);
  Vec xh(nx), acc(nx), fb(nu), xp(nx);
  for (int c = 0; c < n; ++c) {
    for (double &x : xh) x = 0.0;
    for (int t = 0; t <= T; ++t) {
      const double *dx = &in[oD + ((size_t)c * (T + 1) + t) * nx], *yn = &in[oY + ((size_t)c * (T + 1) + t) * ny], *Lt = &in[oL + (size_t)t * nx * ny];
      for (double &x : acc) x = 0.0;
      for (int r = 0; r < ny; ++r) cddp_mcof::update_add(nx, ny, r, Lt, cddp_mcof::innovation(nx, &in[oC + (size_t)r * nx], yn[r], dx, xh.data()), acc.data());
      cddp_mcof::update_end(nx, acc.data(), xh.data());
      for (int i = 0; i < nx; ++i) out[((size_t)c * (T + 1) + t) * nx + i] = xh[i];
      if (t == T) break;
      cddp_mcof::feedback(nx, nu, &in[oK + (size_t)t * nu * nx], 1, xh.data(), fb.data());
      cddp_mcof::predict(nx, nu, &in[oA + (size_t)t * nx * nx], &in[oB + (size_t)t * nx * nu], 1, xh.data(), fb.data(), xp.data());
      for (int i = 0; i < nu; ++i) out[nH + ((size_t)c * T + t) * nu + i] = fb[i];
      for (int i = 0; i < nx; ++i) out[nH + nF + ((size_t)c * T + t) * nx + i] = xp[i];
      xh = xp;
    }
  }
  if (!write_all(argv[3], out)) { std::printf("cannot write %s\n", argv[3]); return 2; }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "noise") == 0) return noise_mode(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "estimate") == 0) return estimate_mode(argc, argv);
  check_index_map();
  check_steps(1);
  check_steps(4);
  check_steps(64);
  if (g_fail) { std::printf("plan mcof: %d checks FAILED\n", g_fail); return 1; }
  std::printf("plan mcof: ok\n");
  return 0;
}
