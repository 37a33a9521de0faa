// The step bodies of the filter kernel (cddp-cpp_amd/csrc/plan_kf.hpp, with the bodies of plan_cov.hpp it reuses) on the host, against the
// sums of include/cddp_hip.h written out longhand, bit for bit: pairs (1,1), (3,2), (4,1), (14,7), N = 3, two trajectories per case, with
// shared inputs and ny = nx + 2, with per-trajectory inputs and ny = 1, and with per-trajectory inputs, ny = nx, of which the second
// trajectory's Sigma0 is -I (the failure path: info = 1, NaN from row 0).  The bodies run owner by owner in the kernel's order of phases,
// on buffers laid out as the kernel's (Z and the trace rows, then Y, then Y' in one product buffer).
// Stand-alone: built by tests/test_plan_kf_host.py with g++ -ffp-contract=off, plainly and with -fsanitize=address,undefined.
// Usage: test_plan_kf OUT -- every case's inputs and results go to OUT as hex floats, for the numpy restatement to be held against.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cddp-cpp_amd/csrc/plan_kf.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double rnd() {   // uniform in [-1, 1): a 64-bit LCG, its top 53 bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

using Vec = std::vector<double>;

void fill(Vec &v, double scale) { for (double &x : v) x = scale * rnd(); }

// a symmetric positive definite n x n matrix (G G^T / n + 0.1 I, times scale); lower_only: junk above the diagonal, which must not be read
void spd(double *m, int n, double scale, bool lower_only) {
  Vec g(n * n);
  fill(g, 1.0);
  for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += g[i * n + k] * g[j * n + k];
    m[i * n + j] = m[j * n + i] = scale * (s / n + (i == j ? 0.1 : 0.0));
  }
  if (lower_only) for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) m[i * n + j] = 7.0 * rnd();
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
  int nx, nu, ny, N, B; bool per, have_w, have_wu;
  Vec A, Bm, K;             // [B][N][nx][nx], [B][N][nx][nu], [B][N][nu][nx]
  Vec C, v, S0, W, Wu;      // [B or 1][...]
  Vec Qdt, Rdt, Qf;         // the cost matrices, full
};

struct Out {
  Vec L, SP, SF, SX, SU, dcost, info;
  void size(const Case &c) {
    const int e = c.B * (c.N + 1) * c.nx * c.nx;
    L.assign(c.B * (c.N + 1) * c.nx * c.ny, 0.0); SP.assign(e, 0.0); SF.assign(e, 0.0); SX.assign(e, 0.0);
    SU.assign(c.B * c.N * c.nu * c.nu, 0.0); dcost.assign(c.B, 0.0); info.assign(c.B, 0.0);
  }
};

double sym(const double *m, int n, int i, int j) { return j <= i ? m[i * n + j] : m[j * n + i]; }

// M Sig M^T (+ W) (+ B Wu B^T), cddp_hip_plan_covariance's steps 4 and 5, longhand: the lower triangle, mirrored
void propagate(int nx, int nu, const Vec &M, const Vec &Sig, const double *W, const double *Wu, const double *Bm, Vec &out) {
  Vec Y(nx * nx);
  for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) { double s = 0.0; for (int l = 0; l < nx; ++l) s += M[i * nx + l] * Sig[l * nx + j]; Y[i * nx + j] = s; }
  for (int i = 0; i < nx; ++i) for (int j = 0; j <= i; ++j) {
    double s = 0.0;
    for (int l = 0; l < nx; ++l) s += M[i * nx + l] * Y[j * nx + l];
    if (W) s += sym(W, nx, i, j);
    if (Wu) {
      double h = 0.0;
      for (int k = 0; k < nu; ++k) { double g = 0.0; for (int m = 0; m < nu; ++m) g += Bm[i * nu + m] * sym(Wu, nu, m, k); h += g * Bm[j * nu + k]; }
      s += h;
    }
    out[i * nx + j] = out[j * nx + i] = s;
  }
}

// the header's sums, longhand, one trajectory
void longhand(const Case &c, int b, Out &o) {
  const int nx = c.nx, nu = c.nu, ny = c.ny, N = c.N, p = c.per ? b : 0;
  const double *C = &c.C[p * ny * nx], *v = &c.v[p * ny], *S0 = &c.S0[p * nx * nx];
  const double *W = c.have_w ? &c.W[p * nx * nx] : nullptr, *Wu = c.have_wu ? &c.Wu[p * nu * nu] : nullptr;
  double *L = &o.L[b * (N + 1) * nx * ny], *SP = &o.SP[b * (N + 1) * nx * nx], *SF = &o.SF[b * (N + 1) * nx * nx], *SX = &o.SX[b * (N + 1) * nx * nx];
  double *SU = &o.SU[b * N * nu * nu];
  const double nan = std::nan("");
  Vec Sm(nx * nx), Xm(nx * nx, 0.0);
  for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) Sm[i * nx + j] = sym(S0, nx, i, j);
  int fail = 0;
  double dc = 0.0;
  for (int t = 0; t <= N; ++t) {
    Vec S = Sm, G(nx * nx, 0.0), h(nx), g(nx), Xh(nx * nx), Sx(nx * nx);
    for (int r = 0; r < ny; ++r) {
      const double *cr = C + r * nx;
      for (int i = 0; i < nx; ++i) { double s = 0.0; for (int j = 0; j < nx; ++j) s += S[i * nx + j] * cr[j]; h[i] = s; }
      double sr = v[r];
      for (int j = 0; j < nx; ++j) sr += cr[j] * h[j];
      if (!(sr > 0.0) && !fail) fail = t + 1;
      for (int i = 0; i < nx; ++i) g[i] = h[i] / sr;
      for (int i = 0; i < nx; ++i) for (int j = 0; j <= i; ++j) {
        double e = S[i * nx + j];
        e -= g[i] * h[j]; e -= h[i] * g[j];
        const double q = sr * g[i];
        e += q * g[j];
        S[i * nx + j] = S[j * nx + i] = e;
        G[i * nx + j] += h[i] * g[j]; G[j * nx + i] = G[i * nx + j];
      }
    }
    const bool dead = fail != 0;
    for (int i = 0; i < nx; ++i) for (int r = 0; r < ny; ++r) {
      double s = 0.0;
      for (int j = 0; j < nx; ++j) s += S[i * nx + j] * C[r * nx + j];
      L[(t * nx + i) * ny + r] = dead ? nan : s / v[r];
    }
    for (int i = 0; i < nx; ++i) for (int j = 0; j <= i; ++j) Xh[i * nx + j] = Xh[j * nx + i] = Xm[i * nx + j] + G[i * nx + j];
    for (int e = 0; e < nx * nx; ++e) {
      Sx[e] = Xh[e] + S[e];
      SP[t * nx * nx + e] = dead ? nan : Sm[e]; SF[t * nx * nx + e] = dead ? nan : S[e]; SX[t * nx * nx + e] = dead ? nan : Sx[e];
    }
    double cst = 0.0;
    for (int i = 0; i < nx; ++i) { double r = 0.0; for (int j = 0; j < nx; ++j) r += (t < N ? c.Qdt : c.Qf)[i * nx + j] * Sx[i * nx + j]; cst += r; }
    if (t == N) { dc += cst; break; }
    const double *A = &c.A[(b * N + t) * nx * nx], *Bm = &c.Bm[(b * N + t) * nx * nu], *K = &c.K[(b * N + t) * nu * nx];
    Vec Acl(nx * nx), Av(A, A + nx * nx), Z(nu * nx), Su(nu * nu);
    for (int i = 0; i < nx; ++i) for (int j = 0; j < nx; ++j) { double s = A[i * nx + j]; for (int k = 0; k < nu; ++k) s += Bm[i * nu + k] * K[k * nx + j]; Acl[i * nx + j] = s; }
    for (int k = 0; k < nu; ++k) for (int j = 0; j < nx; ++j) { double s = 0.0; for (int l = 0; l < nx; ++l) s += K[k * nx + l] * Xh[l * nx + j]; Z[k * nx + j] = s; }
    for (int i = 0; i < nu; ++i) for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int l = 0; l < nx; ++l) s += Z[i * nx + l] * K[j * nx + l];
      if (Wu) s += sym(Wu, nu, i, j);
      Su[i * nu + j] = Su[j * nu + i] = s;
    }
    for (int e = 0; e < nu * nu; ++e) SU[t * nu * nu + e] = dead ? nan : Su[e];
    for (int i = 0; i < nu; ++i) { double r = 0.0; for (int j = 0; j < nu; ++j) r += c.Rdt[i * nu + j] * Su[i * nu + j]; cst += r; }
    dc += cst;
    Vec Sn(nx * nx), Xn(nx * nx);
    propagate(nx, nu, Av, S, W, Wu, Bm, Sn);
    propagate(nx, nu, Acl, Xh, nullptr, nullptr, Bm, Xn);
    Sm = Sn; Xm = Xn;
  }
  o.dcost[b] = fail ? nan : dc;
  o.info[b] = (double)fail;
}

// the bodies, owner by owner, in the kernel's order of phases
template <int NX, int NU>
void bodies(const Case &c, int b, Out &out) {
  using namespace cddp_cov;
  const int ny = c.ny, N = c.N, p = c.per ? b : 0;
  const double *C = &c.C[p * ny * NX], *v = &c.v[p * ny];
  const SymLower Sig0{&c.S0[p * NX * NX], NX}, W{c.have_w ? &c.W[p * NX * NX] : nullptr, NX}, Wu{c.have_wu ? &c.Wu[p * NU * NU] : nullptr, NU}, none{nullptr, NX};
  const Dense Qdt{c.Qdt.data(), NX}, Rdt{c.Rdt.data(), NU}, Qf{c.Qf.data(), NX};
  double *L = &out.L[b * (N + 1) * NX * ny], *SP = &out.SP[b * (N + 1) * NX * NX], *SF = &out.SF[b * (N + 1) * NX * NX], *SX = &out.SX[b * (N + 1) * NX * NX];
  double *SU = &out.SU[b * N * NU * NU];
  const double nan = std::nan("");
  constexpr int kT = NX * NX > NU * NX + NX + NU ? NX * NX : NU * NX + NX + NU;
  Vec S(NX * NX), X(NX * NX, 0.0), T(kT), H(NX);
  double *const R = T.data() + NU * NX;
  for (int o = 0; o < NX; ++o) for (int j = 0; j <= o; ++j) { S[o * NX + j] = Sig0(o, j); S[j * NX + o] = Sig0(o, j); }
  int fail = 0;
  double dc = 0.0;
  struct Vc { const double *p; double operator()(int j) const { return p[j]; } };
  for (int t = 0; t <= N; ++t) {
    const Dense Sg{S.data(), NX}, Xg{X.data(), NX}, Tg{T.data(), NX};
    const Vc Hg{H.data()};
    for (int e = 0; e < NX * NX; ++e) SP[t * NX * NX + e] = fail ? nan : S[e];
    static double gr[NX][NX];
    for (int o = 0; o < NX; ++o) for (int j = 0; j < NX; ++j) gr[o][j] = 0.0;
    for (int r = 0; r < ny; ++r) {
      const cddp_kf::Row cr{C + r * NX};
      for (int o = 0; o < NX; ++o) H[o] = cddp_kf::h_elem<NX>(o, Sg, cr);
      const double sr = cddp_kf::innovation<NX>(v[r], cr, Hg);
      if (!(sr > 0.0) && !fail) fail = t + 1;
      for (int o = 0; o < NX; ++o) cddp_kf::joseph_row<NX>(o, sr, Hg, Sg, [&](int j, double e) { S[o * NX + j] = e; S[j * NX + o] = e; }, gr[o]);
    }
    const bool dead = fail != 0;
    if (fail == t + 1) for (int e = 0; e < NX * NX; ++e) SP[t * NX * NX + e] = nan;
    for (int e = 0; e < NX * NX; ++e) SF[t * NX * NX + e] = dead ? nan : S[e];
    for (int o = 0; o < NX; ++o) for (int r = 0; r < ny; ++r) {
      const double l = cddp_kf::h_elem<NX>(o, Sg, cddp_kf::Row{C + r * NX}) / v[r];
      L[(t * NX + o) * ny + r] = dead ? nan : l;
    }
    for (int o = 0; o < NX; ++o) for (int j = 0; j <= o; ++j) { const double x = X[o * NX + j] + gr[o][j]; X[o * NX + j] = x; X[j * NX + o] = x; }
    struct RowOf { const double *r; double operator()(int, int j) const { return r[j]; } };
    for (int o = 0; o < NX; ++o) {
      double xr[NX];
      for (int j = 0; j < NX; ++j) { xr[j] = Xg(o, j) + Sg(o, j); SX[(t * NX + o) * NX + j] = dead ? nan : xr[j]; }
      R[o] = t < N ? trace_row<NX>(o, Qdt, RowOf{xr}) : trace_row<NX>(o, Qf, RowOf{xr});
    }
    if (t == N) break;
    const Dense A{&c.A[(b * N + t) * NX * NX], NX}, Bm{&c.Bm[(b * N + t) * NX * NU], NU}, K{&c.K[(b * N + t) * NU * NX], NX};
    for (int o = 0; o < NX; ++o) { const int row[1] = {o}; z_cols<NX, NU, 1>(row, K, Xg, [&](int, int k, double z) { T[k * NX + o] = z; }); }
    for (int o = 0; o < NU; ++o) {
      const int row[1] = {o};
      double u[1][NU];
      su_rows<NX, NU, 1>(row, Tg, K, Wu, false, u);
      for (int j = 0; j < NU; ++j) SU[(t * NU + o) * NU + j] = dead ? nan : u[0][j];
      R[NX + o] = trace_row<NU>(o, Rdt, RowOf{u[0]});
    }
    { double cs = 0.0; for (int r = 0; r < NX + NU; ++r) cs += R[r]; dc += cs; }
    static double a0[NX][1][NX], acl[NX][1][NX], y[NX][1][NX], y2[NX][1][NX], n[NX][1][NX];
    for (int o = 0; o < NX; ++o) {
      const int row[1] = {o};
      for (int j = 0; j < NX; ++j) a0[o][0][j] = A(o, j);
      y_rows<NX, 1>(a0[o], Sg, y[o]);
      acl_z<NX, NU, 1, false>(row, A, Bm, K, Xg, acl[o], [](int, int, double) {});
      y_rows<NX, 1>(acl[o], Xg, y2[o]);
    }
    for (int o = 0; o < NX; ++o) for (int j = 0; j < NX; ++j) T[o * NX + j] = y[o][0][j];
    for (int o = 0; o < NX; ++o) {
      const int row[1] = {o};
      if (c.have_wu) next_rows<NX, NU, 1, true>(row, a0[o], Tg, W, Wu, Bm, n[o]);
      else next_rows<NX, NU, 1, false>(row, a0[o], Tg, W, Wu, Bm, n[o]);
    }
    for (int o = 0; o < NX; ++o) for (int j = 0; j < NX; ++j) {
      if (j <= o) { S[o * NX + j] = n[o][0][j]; S[j * NX + o] = n[o][0][j]; }
      T[o * NX + j] = y2[o][0][j];
    }
    for (int o = 0; o < NX; ++o) { const int row[1] = {o}; next_rows<NX, NU, 1, false>(row, acl[o], Tg, none, none, Bm, n[o]); }
    for (int o = 0; o < NX; ++o) for (int j = 0; j <= o; ++j) { X[o * NX + j] = n[o][0][j]; X[j * NX + o] = n[o][0][j]; }
  }
  { double cs = 0.0; for (int r = 0; r < NX; ++r) cs += R[r]; dc += cs; }
  out.dcost[b] = fail ? nan : dc;
  out.info[b] = (double)fail;
}

int g_fail = 0;

template <int NX, int NU>
void run_pair(FILE *out) {
  for (int mode = 0; mode < 3; ++mode) {
    Case c;
    c.nx = NX; c.nu = NU; c.N = 3; c.B = 2; c.per = mode >= 1;
    c.ny = mode == 0 ? NX + 2 : mode == 1 ? 1 : NX;
    c.have_w = mode != 1; c.have_wu = mode != 2;
    const int lead = c.per ? c.B : 1;
    c.A.resize(c.B * c.N * NX * NX); c.Bm.resize(c.B * c.N * NX * NU); c.K.resize(c.B * c.N * NU * NX);
    c.C.resize(lead * c.ny * NX); c.v.resize(lead * c.ny); c.S0.resize(lead * NX * NX); c.W.resize(lead * NX * NX); c.Wu.resize(lead * NU * NU);
    c.Qdt.resize(NX * NX); c.Rdt.resize(NU * NU); c.Qf.resize(NX * NX);
    fill(c.A, 0.6); fill(c.Bm, 0.5); fill(c.K, 0.4); fill(c.C, 1.0);
    for (double &x : c.v) x = 0.05 + 0.25 * (rnd() + 1.0);
    for (int b = 0; b < lead; ++b) { spd(&c.S0[b * NX * NX], NX, 1.0, true); spd(&c.W[b * NX * NX], NX, 0.05, true); spd(&c.Wu[b * NU * NU], NU, 0.1, true); }
    spd(c.Qdt.data(), NX, 0.1, false); spd(c.Rdt.data(), NU, 0.05, false); spd(c.Qf.data(), NX, 3.0, false);
    if (mode == 2) {   // the second trajectory's Sigma0 = -I, its first row of C a unit vector with a small variance: row 0 of step 0 fails
      for (int i = 0; i < NX; ++i) for (int j = 0; j <= i; ++j) c.S0[NX * NX + i * NX + j] = i == j ? -1.0 : 0.0;
      for (int j = 0; j < NX; ++j) c.C[c.ny * NX + j] = j == 0 ? 1.0 : 0.0;
      c.v[c.ny] = 1e-3;
    }
    Out a, bd;
    a.size(c); bd.size(c);
    for (int b = 0; b < c.B; ++b) { longhand(c, b, a); bodies<NX, NU>(c, b, bd); }
    if (!same(a.L, bd.L) || !same(a.SP, bd.SP) || !same(a.SF, bd.SF) || !same(a.SX, bd.SX) || !same(a.SU, bd.SU) || !same(a.dcost, bd.dcost) || !same(a.info, bd.info)) {
      std::printf("plan kf: (%d, %d) mode %d: the bodies differ from the sums written out\n", NX, NU, mode); ++g_fail;
    }
    if (mode == 2 && (a.info[0] != 0.0 || a.info[1] != 1.0)) { std::printf("plan kf: (%d, %d): the failure case does not fail at step 0 (info %g %g)\n", NX, NU, a.info[0], a.info[1]); ++g_fail; }
    if (mode != 2 && (a.info[0] != 0.0 || a.info[1] != 0.0)) { std::printf("plan kf: (%d, %d) mode %d: a row failed\n", NX, NU, mode); ++g_fail; }
    std::fprintf(out, "case %d %d %d %d %d %d %d %d\n", NX, NU, c.ny, c.N, c.B, (int)c.per, (int)c.have_w, (int)c.have_wu);
    dump(out, "A", c.A); dump(out, "B", c.Bm); dump(out, "K", c.K); dump(out, "C", c.C); dump(out, "v", c.v); dump(out, "Sigma0", c.S0);
    dump(out, "W", c.W); dump(out, "Wu", c.Wu); dump(out, "Qdt", c.Qdt); dump(out, "Rdt", c.Rdt); dump(out, "Qf", c.Qf);
    dump(out, "L", bd.L); dump(out, "SP", bd.SP); dump(out, "SF", bd.SF); dump(out, "SX", bd.SX); dump(out, "SU", bd.SU); dump(out, "dcost", bd.dcost); dump(out, "info", bd.info);
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
  std::printf("plan kf: ok\n");
  return 0;
}
