// The step bodies of the plan-covariance kernel (cddp-cpp_amd/csrc/plan_cov.hpp) on the host, against the sums of include/cddp_hip.h
// written out longhand, bit for bit: pairs (1,1), (3,2), (4,1), (14,7), with and without W / Wu, full and diagonal output, N = 3, the
// rows taken one at a time and two at a time (the second form with a row too many where nx is odd, as the kernel's last wavefront has).
// Stand-alone: built by tests/test_plan_cov_host.py with g++ -ffp-contract=off, plainly and with -fsanitize=address,undefined.
// Usage: test_plan_cov OUT -- every case's inputs and results go to OUT as hex floats, for the numpy restatement to be held against.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cddp-cpp_amd/csrc/plan_cov.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double rnd() {   // uniform in [-1, 1): a 64-bit LCG, its top 53 bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

using Vec = std::vector<double>;

void fill(Vec &v, double scale) { for (double &x : v) x = scale * rnd(); }

bool same(const Vec &a, const Vec &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

void dump(FILE *f, const char *name, const Vec &v) {
  std::fprintf(f, "%s %zu", name, v.size());
  for (double x : v) std::fprintf(f, " %a", x);
  std::fprintf(f, "\n");
}

struct Case {
  int nx, nu, N; bool have_w, have_wu, diag;
  Vec A, Bm, K, S0, W, Wu, Q, R, Qf;     // A [N][nx][nx] ..., symmetric inputs with junk above the diagonal: it must not be read
  Vec SX, SU, dc;                        // results: SX [N+1][nx][nx] (diag: [N+1][nx]), SU [N][nu][nu] (diag: [N][nu]), dc [1]
};

double sym(const Vec &m, int n, int i, int j) { return j <= i ? m[i * n + j] : m[j * n + i]; }

// the header's sums, longhand
void longhand(Case &c) {
  const int nx = c.nx, nu = c.nu, N = c.N;
  Vec Sig(nx * nx), SXf((N + 1) * nx * nx), SUf(N * nu * nu);
  for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) Sig[i * nx + j] = sym(c.S0, nx, i, j);
  double dcost = 0.0;
  for (int t = 0; t <= N; ++t) {
    for (int e = 0; e < nx * nx; ++e) SXf[t * nx * nx + e] = Sig[e];
    if (t == N) break;
    const double *A = &c.A[t * nx * nx], *Bm = &c.Bm[t * nx * nu], *K = &c.K[t * nu * nx];
    Vec Acl(nx * nx), Z(nu * nx), SU(nu * nu), Y(nx * nx), Nx(nx * nx);
    for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) { double s = A[i * nx + j]; for (int k = 0; k < nu; ++k) s += Bm[i * nu + k] * K[k * nx + j]; Acl[i * nx + j] = s; }
    for (int i = 0; i < nu; ++i) for (int j = 0; j < nx; ++j) { double s = 0.0; for (int l = 0; l < nx; ++l) s += K[i * nx + l] * Sig[l * nx + j]; Z[i * nx + j] = s; }
    for (int i = 0; i < nu; ++i) for (int j = 0; j <= i; ++j) {
      double s = 0.0; for (int l = 0; l < nx; ++l) s += Z[i * nx + l] * K[j * nx + l];
      if (c.have_wu) s += c.Wu[i * nu + j];
      SU[i * nu + j] = s; SU[j * nu + i] = s;
    }
    for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) { double s = 0.0; for (int l = 0; l < nx; ++l) s += Acl[i * nx + l] * Sig[l * nx + j]; Y[i * nx + j] = s; }
    for (int i = 0; i < nx; ++i) for (int j = 0; j <= i; ++j) {
      double s = 0.0; for (int l = 0; l < nx; ++l) s += Acl[i * nx + l] * Y[j * nx + l];
      if (c.have_w) s += c.W[i * nx + j];
      if (c.have_wu) {
        double h = 0.0;
        for (int k = 0; k < nu; ++k) { double g = 0.0; for (int m = 0; m < nu; ++m) g += Bm[i * nu + m] * sym(c.Wu, nu, m, k); h += g * Bm[j * nu + k]; }
        s += h;
      }
      Nx[i * nx + j] = s; Nx[j * nx + i] = s;
    }
    double cc = 0.0;
    for (int i = 0; i < nx; ++i) { double r = 0.0; for (int j = 0; j < nx; ++j) r += c.Q[i * nx + j] * Sig[i * nx + j]; cc += r; }
    for (int i = 0; i < nu; ++i) { double r = 0.0; for (int j = 0; j < nu; ++j) r += c.R[i * nu + j] * SU[i * nu + j]; cc += r; }
    dcost += cc;
    for (int e = 0; e < nu * nu; ++e) SUf[t * nu * nu + e] = SU[e];
    Sig = Nx;
  }
  double cc = 0.0;
  for (int i = 0; i < nx; ++i) { double r = 0.0; for (int j = 0; j < nx; ++j) r += c.Qf[i * nx + j] * Sig[i * nx + j]; cc += r; }
  dcost += cc;
  c.dc.assign(1, dcost);
  if (!c.diag) { c.SX = SXf; c.SU = SUf; return; }
  c.SX.assign((N + 1) * nx, 0.0); c.SU.assign(N * nu, 0.0);
  for (int t = 0; t <= N; ++t) for (int i = 0; i < nx; ++i) c.SX[t * nx + i] = SXf[(t * nx + i) * nx + i];
  for (int t = 0; t < N; ++t) for (int i = 0; i < nu; ++i) c.SU[t * nu + i] = SUf[(t * nu + i) * nu + i];
}

template <int NN>
struct RowOf {
  const double (&r)[NN];
  double operator()(int, int j) const { return r[j]; }
};

// the bodies, RW rows per call, in the kernel's order of phases
template <int NX, int NU, int RW>
void bodies(const Case &c, Vec &SX, Vec &SU, Vec &dc) {
  using namespace cddp_cov;
  const int N = c.N;
  Vec Sig(NX * NX), Zb(NU * NX), Yb(NX * NX), red(NX + NU);
  const SymLower S0{c.S0.data(), NX}, W{c.have_w ? c.W.data() : nullptr, NX}, Wu{c.have_wu ? c.Wu.data() : nullptr, NU};
  const Dense Q{c.Q.data(), NX}, R{c.R.data(), NU}, Qf{c.Qf.data(), NX};
  for (int i = 0; i < NX; ++i) for (int j = 0; j <= i; ++j) { Sig[i * NX + j] = S0(i, j); Sig[j * NX + i] = S0(i, j); }
  SX.assign((N + 1) * (c.diag ? NX : NX * NX), 0.0); SU.assign(N * (c.diag ? NU : NU * NU), 0.0);
  auto sx_out = [&](int t) {
    for (int i = 0; i < NX; ++i) {
      if (c.diag) SX[t * NX + i] = Sig[i * NX + i];
      else for (int j = 0; j < NX; ++j) SX[(t * NX + i) * NX + j] = Sig[i * NX + j];
    }
  };
  constexpr int NW = (NX + RW - 1) / RW;
  double dcost = 0.0;
  for (int t = 0; t < N; ++t) {
    const Dense A{&c.A[t * NX * NX], NX}, Bm{&c.Bm[t * NX * NU], NU}, K{&c.K[t * NU * NX], NX}, Sg{Sig.data(), NX}, Zg{Zb.data(), NX};
    sx_out(t);
    static double acl[NW][RW][NX], y[NW][RW][NX];
    int row[NW][RW];
    for (int w = 0; w < NW; ++w) {
      for (int q = 0; q < RW; ++q) row[w][q] = w * RW + q < NX ? w * RW + q : NX - 1;
      auto zout = [&](int q, int k, double v) { Zb[k * NX + row[w][q]] = v; };
      if (c.have_wu || t % 2 == 0) acl_z<NX, NU, RW, true>(row[w], A, Bm, K, Sg, acl[w], zout);
      else { acl_z<NX, NU, RW, false>(row[w], A, Bm, K, Sg, acl[w], zout); z_cols<NX, NU, RW>(row[w], K, Sg, zout); }   // (the two-pass form of the staged kernel)
      for (int q = 0; q < RW; ++q) red[row[w][q]] = trace_row<NX>(row[w][q], Q, Sg);
      y_rows<NX, RW>(acl[w], Sg, y[w]);
    }
    for (int w = 0; w < NW; ++w) {
      double u[RW][NU];
      su_rows<NX, NU, RW>(row[w], Zg, K, Wu, false, u);
      for (int q = 0; q < RW; ++q) {
        const int i = row[w][q];
        if (i >= NU) continue;
        for (int j = 0; j < NU; ++j) { if (!c.diag) SU[(t * NU + i) * NU + j] = u[q][j]; else if (j == i) SU[t * NU + i] = u[q][j]; }
        red[NX + i] = trace_row<NU>(i, R, RowOf<NU>{u[q]});
      }
      if (c.diag) {   // the diagonal-only form gives the same diagonal
        double ud[RW][NU];
        su_rows<NX, NU, RW>(row[w], Zg, K, Wu, true, ud);
        for (int q = 0; q < RW; ++q) if (row[w][q] < NU && std::memcmp(&ud[q][row[w][q]], &u[q][row[w][q]], sizeof(double)) != 0) { std::printf("only_diag differs\n"); std::exit(1); }
      }
    }
    for (int w = 0; w < NW; ++w) for (int q = 0; q < RW; ++q) for (int j = 0; j < NX; ++j) Yb[row[w][q] * NX + j] = y[w][q][j];
    double cc = 0.0;
    for (int r = 0; r < NX + NU; ++r) cc += red[r];
    dcost += cc;
    const Dense Yg{Yb.data(), NX};
    for (int w = 0; w < NW; ++w) {
      if (c.have_wu) next_rows<NX, NU, RW, true>(row[w], acl[w], Yg, W, Wu, Bm, y[w]);
      else next_rows<NX, NU, RW, false>(row[w], acl[w], Yg, W, Wu, Bm, y[w]);
    }
    for (int w = 0; w < NW; ++w) for (int q = 0; q < RW; ++q) {
      const int i = row[w][q];
      for (int j = 0; j <= i; ++j) { Sig[i * NX + j] = y[w][q][j]; Sig[j * NX + i] = y[w][q][j]; }
    }
  }
  sx_out(N);
  const Dense Sg{Sig.data(), NX};
  double cc = 0.0;
  for (int i = 0; i < NX; ++i) cc += trace_row<NX>(i, Qf, Sg);
  dcost += cc;
  dc.assign(1, dcost);
}

int g_fail = 0;

template <int NX, int NU>
void run_pair(FILE *out) {
  for (int mode = 0; mode < 8; ++mode) {
    Case c;
    c.nx = NX; c.nu = NU; c.N = 3; c.have_w = mode & 1; c.have_wu = mode & 2; c.diag = mode & 4;
    c.A.resize(c.N * NX * NX); c.Bm.resize(c.N * NX * NU); c.K.resize(c.N * NU * NX);
    c.S0.resize(NX * NX); c.W.resize(NX * NX); c.Wu.resize(NU * NU); c.Q.resize(NX * NX); c.R.resize(NU * NU); c.Qf.resize(NX * NX);
    fill(c.A, 0.6); fill(c.Bm, 0.5); fill(c.K, 0.7); fill(c.S0, 1.0); fill(c.W, 0.1); fill(c.Wu, 0.2); fill(c.Q, 1.0); fill(c.R, 1.0); fill(c.Qf, 3.0);
    longhand(c);
    Vec SX1, SU1, dc1, SX2, SU2, dc2;
    bodies<NX, NU, 1>(c, SX1, SU1, dc1);
    bodies<NX, NU, 2>(c, SX2, SU2, dc2);
    const bool ok = same(SX1, c.SX) && same(SU1, c.SU) && same(dc1, c.dc) && same(SX2, c.SX) && same(SU2, c.SU) && same(dc2, c.dc);
    if (!ok) { std::printf("plan cov: (%d, %d) W %d Wu %d diag %d: the bodies differ from the sums written out\n", NX, NU, (int)c.have_w, (int)c.have_wu, (int)c.diag); ++g_fail; }
    std::fprintf(out, "case %d %d %d %d %d %d\n", NX, NU, c.N, (int)c.have_w, (int)c.have_wu, (int)c.diag);
    dump(out, "A", c.A); dump(out, "B", c.Bm); dump(out, "K", c.K); dump(out, "S0", c.S0); dump(out, "W", c.W); dump(out, "Wu", c.Wu);
    dump(out, "Q", c.Q); dump(out, "R", c.R); dump(out, "Qf", c.Qf); dump(out, "SX", SX1); dump(out, "SU", SU1); dump(out, "dc", dc1);
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
  std::printf("plan cov: ok\n");
  return 0;
}
