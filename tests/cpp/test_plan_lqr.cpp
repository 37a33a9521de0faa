// The step bodies of the gain-design kernel (cddp-cpp_amd/csrc/plan_lqr.hpp) on the host, against the sums of include/cddp_hip.h written
// out longhand, bit for bit: pairs (1,1), (3,2), (4,1), (14,7), N = 3, two trajectories per case, with shared weights, with per-trajectory
// weights, and with per-trajectory weights of which the second trajectory's R is negative definite (the failure path: info, K = 0,
// P = NaN).  The bodies run owner by owner in the kernel's order of phases, on buffers laid out as the kernel's (T overlays M, Y goes over P).
// Stand-alone: built by tests/test_plan_lqr_host.py with g++ -ffp-contract=off, plainly and with -fsanitize=address,undefined.
// Usage: test_plan_lqr OUT -- every case's inputs and results go to OUT as hex floats, for the numpy restatement to be held against.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cddp-cpp_amd/csrc/plan_lqr.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double rnd() {   // uniform in [-1, 1): a 64-bit LCG, its top 53 bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

using Vec = std::vector<double>;

void fill(Vec &v, double scale) { for (double &x : v) x = scale * rnd(); }

// a symmetric positive definite n x n matrix (G G^T / n + 0.1 I, times scale) in the lower triangle, junk above the diagonal: it must not be read
void spd(double *m, int n, double scale) {
  Vec g(n * n);
  fill(g, 1.0);
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
    if (j > i) { m[i * n + j] = 7.0 * rnd(); continue; }
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += g[i * n + k] * g[j * n + k];
    m[i * n + j] = scale * (s / n + (i == j ? 0.1 : 0.0));
  }
}

bool same(const Vec &a, const Vec &b) {   // by value, NaN = NaN
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) if (!(a[i] == b[i]) && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  return true;
}

void dump(FILE *f, const char *name, const Vec &v) {
  std::fprintf(f, "%s %zu", name, v.size());
  for (double x : v) std::fprintf(f, " %a", x);
  std::fprintf(f, "\n");
}

struct Case {
  int nx, nu, N, B; bool per; double dt;
  Vec A, Bm;            // [B][N][nx][nx], [B][N][nx][nu]
  Vec Q, R, Qf;         // [B or 1][n][n], unscaled Q and R
  Vec K, P, info;       // results: [B][N][nu][nx], [B][N+1][nx][nx], [B]
};

double sym(const double *m, int n, int i, int j) { return j <= i ? m[i * n + j] : m[j * n + i]; }

// the header's sums, longhand, one trajectory
void longhand(const Case &c, int b, double *Kout, double *Pout, double *info) {
  const int nx = c.nx, nu = c.nu, N = c.N;
  const double *Q = &c.Q[(c.per ? b : 0) * nx * nx], *R = &c.R[(c.per ? b : 0) * nu * nu], *Qf = &c.Qf[(c.per ? b : 0) * nx * nx];
  Vec P(nx * nx), Qd(nx * nx), Rd(nu * nu);
  for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) { P[i * nx + j] = sym(Qf, nx, i, j); Qd[i * nx + j] = sym(Q, nx, i, j) * c.dt; }
  for (int i = 0; i < nu; ++i) for (int j = 0; j < nu; ++j) Rd[i * nu + j] = sym(R, nu, i, j) * c.dt;
  for (int e = 0; e < nx * nx; ++e) Pout[N * nx * nx + e] = P[e];
  int fail = 0;
  for (int t = N - 1; t >= 0; --t) {
    const double *A = &c.A[(b * N + t) * nx * nx], *Bm = &c.Bm[(b * N + t) * nx * nu];
    Vec M(nx * nu), Quu(nu * nu, 0.0), Qux(nu * nx), L(nu * nu, 0.0), K(nu * nx), Acl(nx * nx), Y(nx * nx), T(nu * nx), Pn(nx * nx);
    for (int i = 0; i < nx; ++i) for (int k = 0; k < nu; ++k) { double s = 0.0; for (int l = 0; l < nx; ++l) s += P[i * nx + l] * Bm[l * nu + k]; M[i * nu + k] = s; }
    for (int r = 0; r < nu; ++r) for (int cc = 0; cc <= r; ++cc) { double s = 0.0; for (int l = 0; l < nx; ++l) s += Bm[l * nu + r] * M[l * nu + cc]; s += Rd[r * nu + cc]; Quu[r * nu + cc] = s; }
    for (int k = 0; k < nu; ++k) for (int j = 0; j < nx; ++j) { double s = 0.0; for (int l = 0; l < nx; ++l) s += M[l * nu + k] * A[l * nx + j]; Qux[k * nx + j] = s; }
    bool ok = true;
    for (int r = 0; r < nu; ++r) {
      for (int cc = 0; cc < r; ++cc) { double s = Quu[r * nu + cc]; for (int m = 0; m < cc; ++m) s -= L[r * nu + m] * L[cc * nu + m]; L[r * nu + cc] = s / L[cc * nu + cc]; }
      double s = Quu[r * nu + r];
      for (int m = 0; m < r; ++m) s -= L[r * nu + m] * L[r * nu + m];
      if (!(s > 0.0)) ok = false;
      L[r * nu + r] = std::sqrt(s);
    }
    for (int j = 0; j < nx; ++j) {
      Vec y(nu), z(nu);
      for (int r = 0; r < nu; ++r) { double s = Qux[r * nx + j]; for (int m = 0; m < r; ++m) s -= L[r * nu + m] * y[m]; y[r] = s / L[r * nu + r]; }
      for (int r = nu - 1; r >= 0; --r) { double s = y[r]; for (int m = r + 1; m < nu; ++m) s -= L[m * nu + r] * z[m]; z[r] = s / L[r * nu + r]; }
      for (int r = 0; r < nu; ++r) K[r * nx + j] = -z[r];
    }
    for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) { double s = A[i * nx + j]; for (int k = 0; k < nu; ++k) s += Bm[i * nu + k] * K[k * nx + j]; Acl[i * nx + j] = s; }
    for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) { double s = 0.0; for (int l = 0; l < nx; ++l) s += P[i * nx + l] * Acl[l * nx + j]; Y[i * nx + j] = s; }
    for (int k = 0; k < nu; ++k) for (int j = 0; j < nx; ++j) { double s = 0.0; for (int m = 0; m < nu; ++m) s += Rd[k * nu + m] * K[m * nx + j]; T[k * nx + j] = s; }
    for (int i = 0; i < nx; ++i) for (int j = 0; j <= i; ++j) {
      double s = 0.0; for (int l = 0; l < nx; ++l) s += Acl[l * nx + i] * Y[l * nx + j];
      double h = 0.0; for (int k = 0; k < nu; ++k) h += K[k * nx + i] * T[k * nx + j];
      s += h; s += Qd[i * nx + j];
      Pn[i * nx + j] = s; Pn[j * nx + i] = s;
    }
    if (!ok && !fail) fail = t + 1;
    for (int e = 0; e < nu * nx; ++e) Kout[t * nu * nx + e] = fail ? 0.0 : K[e];
    for (int e = 0; e < nx * nx; ++e) Pout[t * nx * nx + e] = fail ? std::nan("") : Pn[e];
    P = Pn;
  }
  *info = (double)fail;
}

// the bodies, owner by owner, in the kernel's order of phases
template <int NX, int NU>
void bodies(const Case &c, int b, double *Kout, double *Pout, double *info) {
  using namespace cddp_lqr;
  const int N = c.N;
  const Weight Qd{&c.Q[(c.per ? b : 0) * NX * NX], NX, c.dt}, Rd{&c.R[(c.per ? b : 0) * NU * NU], NU, c.dt}, Qf{&c.Qf[(c.per ? b : 0) * NX * NX], NX, 1.0};
  Vec P(NX * NX), M(NX * NU), Qb(NU * NU, 0.0);
  for (int o = 0; o < NX; ++o) for (int j = 0; j <= o; ++j) { P[o * NX + j] = Qf(o, j); P[j * NX + o] = Qf(o, j); }
  for (int e = 0; e < NX * NX; ++e) Pout[N * NX * NX + e] = P[e];
  int fail = 0;
  for (int t = N - 1; t >= 0; --t) {
    const Dense A{&c.A[(b * N + t) * NX * NX], NX}, Bm{&c.Bm[(b * N + t) * NX * NU], NU}, Pg{P.data(), NX}, Mg{M.data(), NU}, Qg{Qb.data(), NU}, Tg{M.data(), NX};
    for (int o = 0; o < NX; ++o) m_row<NX, NU>(o, Pg, Bm, [&](int k, double v) { M[o * NU + k] = v; });
    for (int o = 0; o < NU; ++o) quu_row<NX, NU>(o, Bm, Mg, Rd, [&](int cc, double v) { Qb[o * NU + cc] = v; });
    static double kc[NX][NU], acl[NX][NX], y[NX][NX], tc[NX][NU], n[NX][NX];
    bool dead = false;
    for (int o = 0; o < NX; ++o) {
      double L[NU][NU];
      const bool ok = chol<NU>(Qg, L);        // every owner factors for itself
      if (!ok && !fail) fail = t + 1;
      dead = fail != 0;
      qux_col<NX, NU>(o, Mg, A, kc[o]);
      solve_col<NU>(L, kc[o]);
      for (int k = 0; k < NU; ++k) Kout[(t * NU + k) * NX + o] = dead ? 0.0 : kc[o][k];
      acl_col<NX, NU>(o, A, Bm, kc[o], acl[o]);
      y_col<NX>(Pg, acl[o], y[o]);
      t_col<NU>(Rd, kc[o], tc[o]);
    }
    for (int o = 0; o < NX; ++o) {
      for (int l = 0; l < NX; ++l) P[l * NX + o] = y[o][l];
      for (int k = 0; k < NU; ++k) M[k * NX + o] = tc[o][k];
    }
    for (int o = 0; o < NX; ++o) p_row<NX, NU>(o, acl[o], kc[o], Pg, Tg, Qd, [&](int j, double v) { n[o][j] = v; });
    for (int o = 0; o < NX; ++o) for (int j = 0; j <= o; ++j) {
      P[o * NX + j] = n[o][j]; P[j * NX + o] = n[o][j];
      const double v = dead ? std::nan("") : n[o][j];
      Pout[(t * NX + o) * NX + j] = v; Pout[(t * NX + j) * NX + o] = v;
    }
  }
  *info = (double)fail;
}

int g_fail = 0;

template <int NX, int NU>
void run_pair(FILE *out) {
  for (int mode = 0; mode < 3; ++mode) {
    Case c;
    c.nx = NX; c.nu = NU; c.N = 3; c.B = 2; c.per = mode >= 1; c.dt = 0.1;
    const int lead = c.per ? c.B : 1;
    c.A.resize(c.B * c.N * NX * NX); c.Bm.resize(c.B * c.N * NX * NU);
    c.Q.resize(lead * NX * NX); c.R.resize(lead * NU * NU); c.Qf.resize(lead * NX * NX);
    fill(c.A, 0.6); fill(c.Bm, 0.5);
    for (int b = 0; b < lead; ++b) { spd(&c.Q[b * NX * NX], NX, 1.0); spd(&c.R[b * NU * NU], NU, 1.0); spd(&c.Qf[b * NX * NX], NX, 3.0); }
    if (mode == 2) {   // the second trajectory's R negative definite, its Qf small: the first pivot of the last step fails
      for (int i = 0; i < NU; ++i) for (int j = 0; j <= i; ++j) c.R[NU * NU + i * NU + j] = -c.R[NU * NU + i * NU + j];
      for (int i = 0; i < NX; ++i) for (int j = 0; j <= i; ++j) c.Qf[NX * NX + i * NX + j] *= 1e-3;
    }
    const int eK = c.N * NU * NX, eP = (c.N + 1) * NX * NX;
    c.K.assign(c.B * eK, 0.0); c.P.assign(c.B * eP, 0.0); c.info.assign(c.B, 0.0);
    Vec K2(c.B * eK, 0.0), P2(c.B * eP, 0.0), i2(c.B, 0.0);
    for (int b = 0; b < c.B; ++b) {
      longhand(c, b, &c.K[b * eK], &c.P[b * eP], &c.info[b]);
      bodies<NX, NU>(c, b, &K2[b * eK], &P2[b * eP], &i2[b]);
    }
    if (!same(K2, c.K) || !same(P2, c.P) || !same(i2, c.info)) { std::printf("plan lqr: (%d, %d) mode %d: the bodies differ from the sums written out\n", NX, NU, mode); ++g_fail; }
    if (mode == 2 && (c.info[0] != 0.0 || c.info[1] != (double)c.N)) { std::printf("plan lqr: (%d, %d): the failure case does not fail at the last step (info %g %g)\n", NX, NU, c.info[0], c.info[1]); ++g_fail; }
    if (mode != 2 && (c.info[0] != 0.0 || c.info[1] != 0.0)) { std::printf("plan lqr: (%d, %d) mode %d: a pivot failed\n", NX, NU, mode); ++g_fail; }
    std::fprintf(out, "case %d %d %d %d %d\n", NX, NU, c.N, c.B, (int)c.per);
    dump(out, "dt", Vec(1, c.dt)); dump(out, "A", c.A); dump(out, "B", c.Bm); dump(out, "Q", c.Q); dump(out, "R", c.R); dump(out, "Qf", c.Qf);
    dump(out, "K", K2); dump(out, "P", P2); dump(out, "info", i2);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) { std::printf("usage: %s OUT\n", argv[0]); return 2; }
  FILE *out = std::fopen(argv[1], "w");
  if (!out) { std::printf("cannot write %s\n", argv[1]); return 2; }
  run_pair<1, 1>(out);
  run_pair<3, 2>(out);
  run_pair<4, 1>(out);
  run_pair<14, 7>(out);
  std::fclose(out);
  if (g_fail) return 1;
  std::printf("plan lqr: ok\n");
  return 0;
}
