// The two step bodies of cddp-cpp_amd/csrc/plan_sens.hpp on the host: random stacks of nx = 3, nu = 2, N = 5, the forward and the adjoint
// recursion walked with jvp_step / vjp_step, for one vector per call and for three at once, against the sums of include/cddp_hip.h written
// out here in their stated order -- bit for bit (built with -ffp-contract=off, as the library is).  The adjoint runs with both cotangents,
// with gX only, with gU only and with neither.  A last check ties the two recursions together: <g, J dx0> == <J^T g, dx0> to rounding.
// No GPU, no library: the header is all it includes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cddp-cpp_amd/csrc/plan_sens.hpp"

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { if (fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

constexpr int NX = 3, NU = 2, N = 5, R = 3;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {   // xorshift64*, uniform in (-1, 1)
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}
static bool same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

struct Problem {
  std::vector<double> A, Bm, K, dx0, gX, gU;   // [t][i][j] row-major; vectors [r][...]
  Problem() : A(N * NX * NX), Bm(N * NX * NU), K(N * NU * NX), dx0(R * NX), gX(R * (N + 1) * NX), gU(R * N * NU) {
    for (auto *v : {&A, &Bm, &K, &dx0, &gX, &gU}) for (double &x : *v) x = rnd();
  }
};

// the sums of the header, written out
static void jvp_reference(const Problem &p, int r, double *dX /* (N+1)*NX */, double *dU /* N*NU */) {
  for (int j = 0; j < NX; ++j) dX[j] = p.dx0[r * NX + j];
  for (int t = 0; t < N; ++t) {
    const double *A = &p.A[t * NX * NX], *B = &p.Bm[t * NX * NU], *K = &p.K[t * NU * NX], *dx = dX + t * NX;
    double *du = dU + t * NU, *dxn = dX + (t + 1) * NX;
    for (int i = 0; i < NU; ++i) { double s = 0; for (int j = 0; j < NX; ++j) s += K[i * NX + j] * dx[j]; du[i] = s; }
    for (int i = 0; i < NX; ++i) {
      double s = 0;
      for (int j = 0; j < NX; ++j) s += A[i * NX + j] * dx[j];
      for (int k = 0; k < NU; ++k) s += B[i * NU + k] * du[k];
      dxn[i] = s;
    }
  }
}
static void vjp_reference(const Problem &p, int r, bool have_gx, bool have_gu, double *gx0 /* NX */) {
  double lam[NX], mu[NU], ln[NX];
  for (int j = 0; j < NX; ++j) lam[j] = have_gx ? p.gX[(r * (N + 1) + N) * NX + j] : 0.0;
  for (int t = N - 1; t >= 0; --t) {
    const double *A = &p.A[t * NX * NX], *B = &p.Bm[t * NX * NU], *K = &p.K[t * NU * NX];
    for (int k = 0; k < NU; ++k) {
      double s = 0; for (int i = 0; i < NX; ++i) s += B[i * NU + k] * lam[i];
      mu[k] = have_gu ? p.gU[(r * N + t) * NU + k] + s : s;
    }
    for (int j = 0; j < NX; ++j) {
      double s = 0;
      for (int i = 0; i < NX; ++i) s += A[i * NX + j] * lam[i];
      for (int k = 0; k < NU; ++k) s += K[k * NX + j] * mu[k];
      ln[j] = have_gx ? p.gX[(r * (N + 1) + t) * NX + j] + s : s;
    }
    for (int j = 0; j < NX; ++j) lam[j] = ln[j];
  }
  for (int j = 0; j < NX; ++j) gx0[j] = lam[j];
}

// the recursions walked with the header's step bodies, RV vectors from vector r0 on
template <int RV>
static void jvp_header(const Problem &p, int r0, double *dX /* [RV][(N+1)*NX] */, double *dU /* [RV][N*NU] */) {
  double dx[RV][NX], du[RV][NU], dxn[RV][NX];
  for (int r = 0; r < RV; ++r) for (int j = 0; j < NX; ++j) dX[r * (N + 1) * NX + j] = dx[r][j] = p.dx0[(r0 + r) * NX + j];
  for (int t = 0; t < N; ++t) {
    cddp_sens::jvp_step<NX, NU, RV>(cddp_sens::Dense{&p.A[t * NX * NX], NX}, cddp_sens::Dense{&p.Bm[t * NX * NU], NU}, cddp_sens::Dense{&p.K[t * NU * NX], NX}, dx, du, dxn);
    for (int r = 0; r < RV; ++r) {
      for (int i = 0; i < NU; ++i) dU[(r * N + t) * NU + i] = du[r][i];
      for (int i = 0; i < NX; ++i) dX[(r * (N + 1) + t + 1) * NX + i] = dx[r][i] = dxn[r][i];
    }
  }
}
template <int RV, bool HAVE_GX, bool HAVE_GU>
static void vjp_header(const Problem &p, int r0, double *gx0 /* [RV][NX] */) {
  double lam[RV][NX], lamn[RV][NX], mu[RV][NU], gx[RV][NX] = {}, gu[RV][NU] = {};
  for (int r = 0; r < RV; ++r) for (int j = 0; j < NX; ++j) lam[r][j] = HAVE_GX ? p.gX[((r0 + r) * (N + 1) + N) * NX + j] : 0.0;
  for (int t = N - 1; t >= 0; --t) {
    for (int r = 0; r < RV; ++r) {
      if (HAVE_GX) for (int j = 0; j < NX; ++j) gx[r][j] = p.gX[((r0 + r) * (N + 1) + t) * NX + j];
      if (HAVE_GU) for (int k = 0; k < NU; ++k) gu[r][k] = p.gU[((r0 + r) * N + t) * NU + k];
    }
    cddp_sens::vjp_step<NX, NU, RV, HAVE_GX, HAVE_GU>(cddp_sens::Dense{&p.A[t * NX * NX], NX}, cddp_sens::Dense{&p.Bm[t * NX * NU], NU}, cddp_sens::Dense{&p.K[t * NU * NX], NX},
                                                      lam, gx, gu, mu, lamn);
    for (int r = 0; r < RV; ++r) for (int j = 0; j < NX; ++j) lam[r][j] = lamn[r][j];
  }
  for (int r = 0; r < RV; ++r) for (int j = 0; j < NX; ++j) gx0[r * NX + j] = lam[r][j];
}

template <bool HAVE_GX, bool HAVE_GU>
static void check_vjp(const Problem &p) {
  double ref[R][NX], one[NX], all[R * NX];
  for (int r = 0; r < R; ++r) vjp_reference(p, r, HAVE_GX, HAVE_GU, ref[r]);
  vjp_header<R, HAVE_GX, HAVE_GU>(p, 0, all);
  EXPECT(same(all, &ref[0][0], R * NX));
  for (int r = 0; r < R; ++r) { vjp_header<1, HAVE_GX, HAVE_GU>(p, r, one); EXPECT(same(one, ref[r], NX)); }
  if (!HAVE_GX && !HAVE_GU) for (int j = 0; j < R * NX; ++j) EXPECT(all[j] == 0.0);
}

int main() {
  for (int trial = 0; trial < 4; ++trial) {
    const Problem p;
    double refX[R][(N + 1) * NX], refU[R][N * NU];
    for (int r = 0; r < R; ++r) jvp_reference(p, r, refX[r], refU[r]);
    {
      std::vector<double> X(R * (N + 1) * NX), U(R * N * NU);
      jvp_header<R>(p, 0, X.data(), U.data());
      EXPECT(same(X.data(), &refX[0][0], X.size()) && same(U.data(), &refU[0][0], U.size()));
      for (int r = 0; r < R; ++r) {
        jvp_header<1>(p, r, X.data(), U.data());
        EXPECT(same(X.data(), refX[r], (N + 1) * NX) && same(U.data(), refU[r], N * NU));
      }
    }
    check_vjp<true, true>(p); check_vjp<true, false>(p); check_vjp<false, true>(p); check_vjp<false, false>(p);
    // adjoint identity, vector 0: sum_t gX_t . dx_t + sum_t gU_t . du_t == gx0 . dx0 up to rounding
    double g0[NX]; vjp_reference(p, 0, true, true, g0);
    double lhs = 0, rhs = 0, mag = 0;
    for (int i = 0; i < (N + 1) * NX; ++i) { lhs += p.gX[i] * refX[0][i]; mag += std::fabs(p.gX[i] * refX[0][i]); }
    for (int i = 0; i < N * NU; ++i) { lhs += p.gU[i] * refU[0][i]; mag += std::fabs(p.gU[i] * refU[0][i]); }
    for (int j = 0; j < NX; ++j) rhs += g0[j] * p.dx0[j];
    EXPECT(std::fabs(lhs - rhs) <= 1e-12 * (1.0 + mag));
  }
  if (fails == 0) std::printf("plan sens: ok\n");
  return fails == 0 ? 0 : 1;
}
