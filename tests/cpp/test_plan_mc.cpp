// The arithmetic of the Monte-Carlo plan evaluation (cddp-cpp_amd/csrc/plan_mc.hpp) on the host: the element-index map (with a pair that
// straddles a step where nx + nu is odd), the triangular product, the tree sum against a tree written out, the moment and stats formulas on
// hand-built records, and the LTI (2, 1) closed loop of the GPU suite's statistical test (B = 64, S = 1024, N = 20, all three noises, the
// seed of tests/test_plan_mc.py) against the closed-form covariance recursion, inside the bounds stated there.
// Stand-alone: built by tests/test_plan_mc_cpu.py with g++ -ffp-contract=off, plainly and with -fsanitize=address,undefined.
// Usage: test_plan_mc                                              the checks
//        test_plan_mc noise IN OUT seed stream B S N nx nu keep    IN: L0 | Lw | Lu (row-major doubles); OUT: Z0 | E | Wn as the library lays them out
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cddp-cpp_amd/csrc/plan_mc.hpp"

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

// Z0 [B][S][nx], E [B][S][N][nu], Wn [B][S][N][nx] of the header, one sample at a time through Draw
void noise(uint64_t seed, uint32_t stream, int B, int S, int N, int nx, int nu, bool keep, const double *L0, const double *Lw, const double *Lu,
           Vec &Z0, Vec &E, Vec &Wn) {
  Z0.assign((size_t)B * S * nx, 0.0); E.assign((size_t)B * S * N * nu, 0.0); Wn.assign((size_t)B * S * N * nx, 0.0);
  Vec z(nx > nu ? nx : nu);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < S; ++c) {
      cddp_mc::Draw dr;
      dr.begin(seed, stream, (uint32_t)b, (uint32_t)c, keep && c == 0);
      const size_t g = (size_t)b * S + c;
      if (L0) { for (int i = 0; i < nx; ++i) z[i] = dr.get(cddp_mc::elem_x0(i)); cddp_mc::colour(nx, L0, z.data(), &Z0[g * nx]); }
      for (int t = 0; t < N; ++t) {
        if (Lu) { for (int i = 0; i < nu; ++i) z[i] = dr.get(cddp_mc::elem_u(nx, nu, t, i)); cddp_mc::colour(nu, Lu, z.data(), &E[(g * N + t) * nu]); }
        if (Lw) { for (int i = 0; i < nx; ++i) z[i] = dr.get(cddp_mc::elem_w(nx, nu, t, i)); cddp_mc::colour(nx, Lw, z.data(), &Wn[(g * N + t) * nx]); }
      }
    }
}

void check_index_map() {
  // the three blocks tile the counter space without a gap, for an even and an odd nx + nu
  for (int nx = 1; nx <= 3; ++nx)
    for (int nu = 1; nu <= 2; ++nu) {
      uint32_t e = 0;
      for (int i = 0; i < nx; ++i) CHECK(cddp_mc::elem_x0(i) == e++);
      for (int t = 0; t < 4; ++t) {
        for (int i = 0; i < nu; ++i) CHECK(cddp_mc::elem_u(nx, nu, t, i) == e++);
        for (int i = 0; i < nx; ++i) CHECK(cddp_mc::elem_w(nx, nu, t, i) == e++);
      }
    }
  // (2, 1): nx + nu = 3.  Step 0 holds e = 2 (u), 3, 4 (w); step 1 e = 5 (u), 6, 7 (w): pair 2 = (4, 5) straddles the two steps
  const uint64_t seed = 0x1234567890ull;
  CHECK(cddp_mc::elem_w(2, 1, 0, 1) == 4 && cddp_mc::elem_u(2, 1, 1, 0) == 5);
  cddp_mc::Draw dr;
  dr.begin(seed, 3, 7, 9, false);
  const cddp_mppi::Pair p2 = cddp_mppi::normal_pair(seed, 3, 7, 9, 2);
  for (uint32_t e = 0; e < 8; ++e) CHECK(same(dr.get(e), cddp_mppi::normal(seed, 3, 7, 9, e)));
  dr.begin(seed, 3, 7, 9, false);
  CHECK(same(dr.get(4), p2.even) && same(dr.get(5), p2.odd));
  // a source switched off leaves the others where they are: skipping the draws of e = 2 .. 4 does not change e = 5
  dr.begin(seed, 3, 7, 9, false);
  (void)dr.get(0); (void)dr.get(1);
  CHECK(same(dr.get(5), cddp_mppi::normal(seed, 3, 7, 9, 5)));
  // keep_nominal
  dr.begin(seed, 3, 7, 0, true);
  for (uint32_t e = 0; e < 8; ++e) CHECK(dr.get(e) == 0.0);
}

void check_colour() {
  const int n = 4;
  Vec L(n * n), z(n), v(n);
  for (double &x : L) x = rnd();
  for (double &x : z) x = rnd();
  Vec Lj = L;
  for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) Lj[i * n + j] = std::nan("");   // above the diagonal: must not be read
  cddp_mc::colour(n, Lj.data(), z.data(), v.data());
  CHECK(same(v[0], 0.0 + L[0] * z[0]));
  CHECK(same(v[1], (0.0 + L[4] * z[0]) + L[5] * z[1]));
  CHECK(same(v[2], ((0.0 + L[8] * z[0]) + L[9] * z[1]) + L[10] * z[2]));
  CHECK(same(v[3], (((0.0 + L[12] * z[0]) + L[13] * z[1]) + L[14] * z[2]) + L[15] * z[3]));
}

// the tree written out: a recursive pairwise sum over index bits, lowest bit innermost -- lane 0 of the butterfly
double tree64(const double *w, int lo, int width) {
  if (width == 1) return w[lo];
  return tree64(w, lo, width / 2) + tree64(w, lo + width / 2, width / 2);
}
double tree_written_out(int S, const double *v) {
  double total = 0.0;
  for (int k = 0; 64 * k < S; ++k) {
    double w[64], p[64];
    for (int l = 0; l < 64; ++l) w[l] = 64 * k + l < S ? v[64 * k + l] : 0.0;
    // the butterfly's lane 0: ((w0 + w1) + (w2 + w3)) + ...: bit-reversal is not involved because stage m pairs l with l ^ m, so after
    // stages 1, 2, 4 lane 0 holds the sum of lanes 0 .. 7 associated as a balanced tree over consecutive lanes
    for (int l = 0; l < 64; ++l) p[l] = w[l];
    const double c = tree64(p, 0, 64);
    total = k == 0 ? c : total + c;
  }
  return total;
}

void check_tree_and_moments() {
  const int sizes[] = {1, 2, 63, 64, 65, 130};
  for (int S : sizes) {
    Vec v(S);
    for (double &x : v) x = rnd() * 1e3 + rnd();
    CHECK(same(cddp_mc::tree_sum(S, v.data()), tree_written_out(S, v.data())));
  }
  {   // order matters: the tree is not the running sum
    Vec v = {1e16, 1.0, -1e16, 1.0};
    CHECK(same(cddp_mc::tree_sum(4, v.data()), (1e16 + 1.0) + (-1e16 + 1.0)));
  }
  // moments on hand-built records: d = 1, 2, 3, 6 -> m1 = 12, q = 50, mean 3, var (50 - 144 / 4) / 3
  {
    const double d[4] = {1.0, 2.0, 3.0, 6.0};
    double q[4];
    for (int i = 0; i < 4; ++i) q[i] = d[i] * d[i];
    const double m1 = cddp_mc::tree_sum(4, d), qq = cddp_mc::tree_sum(4, q);
    CHECK(m1 == 12.0 && qq == 50.0);
    CHECK(same(cddp_mc::moment_mean(m1, 4), 3.0));
    CHECK(same(cddp_mc::moment_cov(qq, m1, m1, 4), (50.0 - 144.0 / 4.0) / 3.0));
    CHECK(cddp_mc::moment_cov(qq, m1, m1, 1) == 0.0);
  }
  // stats on hand-built records
  {
    const double inf = INFINITY, nan = std::nan("");
    const double cost[5] = {3.0, 1.0, inf, 7.0, 1.0}, viol[5] = {0.0, 0.5, 0.0, nan, 0.2};
    double st[8];
    cddp_mc::stats(5, cost, viol, 0.1, st);
    CHECK(st[0] == 3.0 && st[1] == 2.0 && st[2] == inf && st[4] == 1.0 && st[5] == inf && st[7] == 0.5);
    CHECK(st[3] != st[3] && st[6] != st[6]);        // inf - inf and a NaN row propagate
    const double c1[1] = {2.5}, v1[1] = {0.0};
    cddp_mc::stats(1, c1, v1, 0.0, st);
    CHECK(st[0] == 1.0 && st[1] == 0.0 && st[2] == 2.5 && st[3] == 0.0 && st[4] == 2.5 && st[5] == 2.5 && st[6] == 0.0 && st[7] == 0.0);
    const double c3[3] = {nan, 1.0, 2.0}, v3[3] = {0.0, 0.0, 0.0};
    cddp_mc::stats(3, c3, v3, 0.0, st);
    CHECK(st[4] != st[4] && st[5] != st[5] && st[0] == 2.0);   // a scan that starts at a NaN stays there
  }
}

// the statistical test's closed loop on the host: same problem, factors, seed and sizes as tests/test_plan_mc.py::test_statistics
void check_lti_statistics() {
  const int B = 64, S = 1024, N = 20, nx = 2, nu = 1;
  const uint64_t seed = 20261018ull;
  const double A[4] = {1.0, 0.1, -0.2, 0.95}, Bm[2] = {0.005, 0.1}, dt = 0.1;
  const double Qdt[2] = {1.0 * dt, 0.5 * dt}, Rdt = 0.3 * dt, Qf[2] = {5.0, 2.0};
  const double L0[4] = {0.05, 0.0, 0.01, 0.04}, Lw[4] = {0.01, 0.0, 0.002, 0.015}, Lu[1] = {0.05};
  // LQR gains (what the unconstrained solve converges to): P_N = Qf, K_t = -(R + B^T P B)^-1 B^T P A
  double P[4] = {Qf[0], 0.0, 0.0, Qf[1]}, K[N][2];
  for (int t = N - 1; t >= 0; --t) {
    double PB[2] = {P[0] * Bm[0] + P[1] * Bm[1], P[2] * Bm[0] + P[3] * Bm[1]};
    double PA[4] = {P[0] * A[0] + P[1] * A[2], P[0] * A[1] + P[1] * A[3], P[2] * A[0] + P[3] * A[2], P[2] * A[1] + P[3] * A[3]};
    const double quu = Rdt + Bm[0] * PB[0] + Bm[1] * PB[1];
    const double qux[2] = {Bm[0] * PA[0] + Bm[1] * PA[2], Bm[0] * PA[1] + Bm[1] * PA[3]};
    K[t][0] = -qux[0] / quu; K[t][1] = -qux[1] / quu;
    double Acl[4] = {A[0] + Bm[0] * K[t][0], A[1] + Bm[0] * K[t][1], A[2] + Bm[1] * K[t][0], A[3] + Bm[1] * K[t][1]};
    double PAcl[4] = {P[0] * Acl[0] + P[1] * Acl[2], P[0] * Acl[1] + P[1] * Acl[3], P[2] * Acl[0] + P[3] * Acl[2], P[2] * Acl[1] + P[3] * Acl[3]};
    double Pn[4] = {Acl[0] * PAcl[0] + Acl[2] * PAcl[2], Acl[0] * PAcl[1] + Acl[2] * PAcl[3], Acl[1] * PAcl[0] + Acl[3] * PAcl[2], Acl[1] * PAcl[1] + Acl[3] * PAcl[3]};
    Pn[0] += Qdt[0] + K[t][0] * Rdt * K[t][0]; Pn[1] += K[t][0] * Rdt * K[t][1]; Pn[2] += K[t][1] * Rdt * K[t][0]; Pn[3] += Qdt[1] + K[t][1] * Rdt * K[t][1];
    std::memcpy(P, Pn, sizeof(P));
  }
  // closed-form covariance
  double Sig[N + 1][4];
  Sig[0][0] = L0[0] * L0[0]; Sig[0][1] = Sig[0][2] = L0[0] * L0[2]; Sig[0][3] = L0[2] * L0[2] + L0[3] * L0[3];
  const double W[4] = {Lw[0] * Lw[0], Lw[0] * Lw[2], Lw[0] * Lw[2], Lw[2] * Lw[2] + Lw[3] * Lw[3]}, Wu = Lu[0] * Lu[0];
  for (int t = 0; t < N; ++t) {
    const double Acl[4] = {A[0] + Bm[0] * K[t][0], A[1] + Bm[0] * K[t][1], A[2] + Bm[1] * K[t][0], A[3] + Bm[1] * K[t][1]};
    const double *s = Sig[t];
    const double AS[4] = {Acl[0] * s[0] + Acl[1] * s[2], Acl[0] * s[1] + Acl[1] * s[3], Acl[2] * s[0] + Acl[3] * s[2], Acl[2] * s[1] + Acl[3] * s[3]};
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) Sig[t + 1][i * 2 + j] = AS[i * 2] * Acl[j * 2] + AS[i * 2 + 1] * Acl[j * 2 + 1] + W[i * 2 + j] + Bm[i] * Wu * Bm[j];
  }
  // the sampled closed loop about the zero plan (an LTI loop's deviation from its plan does not depend on the plan)
  Vec meanSX((size_t)(N + 1) * 4, 0.0), meanM((size_t)(N + 1) * 2, 0.0);
  Vec d0((size_t)(N + 1) * S), d1((size_t)(N + 1) * S), q(S);
  for (int b = 0; b < B; ++b) {
    for (int c = 0; c < S; ++c) {
      cddp_mc::Draw dr;
      dr.begin(seed, 0, (uint32_t)b, (uint32_t)c, false);
      double z[2], v[2], x[2];
      for (int i = 0; i < nx; ++i) z[i] = dr.get(cddp_mc::elem_x0(i));
      cddp_mc::colour(nx, L0, z, v);
      x[0] = 0.0 + v[0]; x[1] = 0.0 + v[1];
      for (int t = 0; t <= N; ++t) {
        d0[(size_t)t * S + c] = x[0]; d1[(size_t)t * S + c] = x[1];
        if (t == N) break;
        double e[1], zu[1] = {dr.get(cddp_mc::elem_u(nx, nu, t, 0))};
        cddp_mc::colour(nu, Lu, zu, e);
        double s = 0.0;
        s += K[t][0] * x[0]; s += K[t][1] * x[1];
        const double u = (0.0 + e[0]) + s;
        const double xn[2] = {(A[0] * x[0] + A[1] * x[1]) + Bm[0] * u, (A[2] * x[0] + A[3] * x[1]) + Bm[1] * u};
        for (int i = 0; i < nx; ++i) z[i] = dr.get(cddp_mc::elem_w(nx, nu, t, i));
        cddp_mc::colour(nx, Lw, z, v);
        x[0] = xn[0] + v[0]; x[1] = xn[1] + v[1];
      }
    }
    for (int t = 0; t <= N; ++t) {
      const double *a0 = &d0[(size_t)t * S], *a1 = &d1[(size_t)t * S];
      const double m0 = cddp_mc::tree_sum(S, a0), m1 = cddp_mc::tree_sum(S, a1);
      for (int c = 0; c < S; ++c) q[c] = a0[c] * a0[c];
      const double q00 = cddp_mc::tree_sum(S, q.data());
      for (int c = 0; c < S; ++c) q[c] = a1[c] * a0[c];
      const double q10 = cddp_mc::tree_sum(S, q.data());
      for (int c = 0; c < S; ++c) q[c] = a1[c] * a1[c];
      const double q11 = cddp_mc::tree_sum(S, q.data());
      meanSX[t * 4 + 0] += cddp_mc::moment_cov(q00, m0, m0, S) / B; meanSX[t * 4 + 3] += cddp_mc::moment_cov(q11, m1, m1, S) / B;
      meanSX[t * 4 + 1] += cddp_mc::moment_cov(q10, m1, m0, S) / B; meanSX[t * 4 + 2] += cddp_mc::moment_cov(q10, m1, m0, S) / B;
      meanM[t * 2 + 0] += cddp_mc::moment_mean(m0, S) / B; meanM[t * 2 + 1] += cddp_mc::moment_mean(m1, S) / B;
    }
  }
  double worst_cov = 0.0, worst_mean = 0.0;
  for (int t = 0; t <= N; ++t)
    for (int i = 0; i < 2; ++i) {
      const double bm = 6.0 * std::sqrt(Sig[t][i * 3] / ((double)B * S));
      worst_mean = std::fmax(worst_mean, std::fabs(meanM[t * 2 + i]) / bm);
      CHECK(std::fabs(meanM[t * 2 + i]) <= bm);
      for (int j = 0; j < 2; ++j) {
        const double sij = Sig[t][i * 2 + j], bound = 6.0 * std::sqrt((Sig[t][i * 3] * Sig[t][j * 3] + sij * sij) / ((double)B * (S - 1)));
        worst_cov = std::fmax(worst_cov, std::fabs(meanSX[t * 4 + i * 2 + j] - sij) / bound);
        CHECK(std::fabs(meanSX[t * 4 + i * 2 + j] - sij) <= bound);
      }
    }
  std::printf("lti statistics: seed %llu: largest |mean SX - Sigma| / bound %.3f, largest |mean dX| / bound %.3f (bounds are 6 standard errors)\n",
              (unsigned long long)seed, worst_cov, worst_mean);
}

int noise_mode(int argc, char **argv) {
  if (argc != 12) { std::printf("usage: test_plan_mc noise IN OUT seed stream B S N nx nu keep\n"); return 2; }
  const uint64_t seed = std::strtoull(argv[4], nullptr, 0);
  const uint32_t stream = (uint32_t)std::strtoul(argv[5], nullptr, 0);
  const int B = std::atoi(argv[6]), S = std::atoi(argv[7]), N = std::atoi(argv[8]), nx = std::atoi(argv[9]), nu = std::atoi(argv[10]), keep = std::atoi(argv[11]);
  Vec in((size_t)2 * nx * nx + nu * nu);
  FILE *f = std::fopen(argv[2], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::printf("cannot read %s\n", argv[2]); return 2; }
  std::fclose(f);
  Vec Z0, E, Wn;
  noise(seed, stream, B, S, N, nx, nu, keep != 0, in.data(), in.data() + nx * nx, in.data() + 2 * nx * nx, Z0, E, Wn);
  f = std::fopen(argv[3], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[3]); return 2; }
  std::fwrite(Z0.data(), sizeof(double), Z0.size(), f); std::fwrite(E.data(), sizeof(double), E.size(), f); std::fwrite(Wn.data(), sizeof(double), Wn.size(), f);
  std::fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "noise") == 0) return noise_mode(argc, argv);
  check_index_map();
  check_colour();
  check_tree_and_moments();
  check_lti_statistics();
  if (g_fail) { std::printf("plan mc: %d checks FAILED\n", g_fail); return 1; }
  std::printf("plan mc: ok\n");
  return 0;
}
