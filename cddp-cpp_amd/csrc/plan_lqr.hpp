// Finite-horizon LQR along a plan's linearisation (the backward Riccati recursion in Joseph form): the ONE statement of the step bodies
// that the gain-design kernel (inst_lqr.hip) runs.  Plain templates, host and device, no other header needed: tests/cpp/test_plan_lqr.cpp
// compiles this file with g++ -ffp-contract=off and checks every body bitwise against the sums written out.
//
//   M = P B;   Quu = B^T M + Rd;   Qux = M^T A;   Quu = L L^T;   K = -Quu^-1 Qux (two triangular solves per column);
//   Acl = A + B K;   Y = P Acl;   T = Rd K;   P' = Acl^T Y + K^T T + Qd        (P = P_{t+1}, P' = P_t)
//
// The bodies are written per OWNER: a row i of M and of P', a row r of Quu, a column j of Qux / K / Acl / Y / T (a group of lanes of the
// kernel owns one index), on accessors X(i, j) = X[i][j]: a kernel passes the stacks where they lie, its LDS buffers and its registers;
// the CPU test passes arrays.  Every sum is the one include/cddp_hip.h fixes: a stated start value, the index ascending -- so who computes
// an element is free, what it is worth is not.  The weights are read through Weight, which touches the lower triangle only; P' is computed
// for j <= i and mirrored by the caller.  True division and square root throughout, no reciprocals.
#pragma once

#if defined(__HIPCC__)
#define CDDP_LQR_HD __host__ __device__ __forceinline__
#else
#define CDDP_LQR_HD inline
#endif
// CDDP_LQR_FENCE(), between the iterations of the unrolled output loops: on the device the instruction scheduler may not move
// instructions across it (the loads in flight stay those of a few outputs).  No effect on values.
#if defined(__HIP_DEVICE_COMPILE__)
#define CDDP_LQR_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define CDDP_LQR_FENCE() ((void)0)
#endif

namespace cddp_lqr {

// A row-major matrix in an array: the accessor of the CPU test
struct Dense {
  const double *m; int cols;
  CDDP_LQR_HD double operator()(int i, int j) const { return m[i * cols + j]; }
};

// A symmetric n x n weight of which only the lower triangle (j <= i) is ever read: element (i, j) with j > i is element (j, i).  Every
// element is multiplied by `scale` where it is read: dt for a caller's Q and R (Qd = Q * dt, Rd = R * dt, one rounding per element,
// the same value wherever it is formed), 1 for the handle's own Q dt / R dt and for Qf (x * 1 is x).
struct Weight {
  const double *m; int n; double scale;
  CDDP_LQR_HD double operator()(int i, int j) const { return (j <= i ? m[i * n + j] : m[j * n + i]) * scale; }
};

// Step 1, row i of M:  s = 0;  for l ascending  s += P[i][l] * B[l][k];  Mout(k, s)
template <int NX, int NU, class MP, class MB, class MW>
CDDP_LQR_HD void m_row(int i, const MP &P, const MB &Bm, const MW &Mout) {
  double s[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) s[k] = 0.0;
#pragma unroll
  for (int l = 0; l < NX; ++l) {
    const double pv = P(i, l);
#pragma unroll
    for (int k = 0; k < NU; ++k) s[k] += pv * Bm(l, k);
    CDDP_LQR_FENCE();
  }
#pragma unroll
  for (int k = 0; k < NU; ++k) Mout(k, s[k]);
}

// Step 2, the elements c <= r of row r of Quu:  s = 0;  for l ascending  s += B[l][r] * M[l][c];  s += Rd[r][c];  Qout(c, s)
template <int NX, int NU, class MB, class MM, class QW>
CDDP_LQR_HD void quu_row(int r, const MB &Bm, const MM &M, const Weight &Rd, const QW &Qout) {
#pragma unroll
  for (int c = 0; c < NU; ++c) {
    if (c <= r) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < NX; ++l) s += Bm(l, r) * M(l, c);
      s += Rd(r, c);
      Qout(c, s);
    }
  }
}

// Step 3, column j of Qux:  q[k] = 0;  for l ascending  q[k] += M[l][k] * A[l][j]
template <int NX, int NU, class MM, class MA>
CDDP_LQR_HD void qux_col(int j, const MM &M, const MA &A, double (&q)[NU]) {
#pragma unroll
  for (int k = 0; k < NU; ++k) q[k] = 0.0;
#pragma unroll
  for (int l = 0; l < NX; ++l) {
    const double av = A(l, j);
#pragma unroll
    for (int k = 0; k < NU; ++k) q[k] += M(l, k) * av;
    CDDP_LQR_FENCE();
  }
}

// Step 4, Quu = L L^T from the lower triangle of Quu, rows r ascending:
//   c < r:     s = Quu[r][c];  for m < c ascending  s -= L[r][m] * L[c][m];  L[r][c] = s / L[c][c]
//   diagonal:  s = Quu[r][r];  for m < r ascending  s -= L[r][m] * L[r][m];  the pivot test is  s > 0  (false for NaN);  L[r][r] = sqrt(s)
// Returns whether every pivot passed.  After a failed pivot the rest of L is computed all the same (a NaN or garbage nobody may use):
// every lane runs the same instructions.  All indices are compile-time constants once unrolled: L is registers on the device.
template <int NU, class MQ>
CDDP_LQR_HD bool chol(const MQ &Quu, double (&L)[NU][NU]) {
  bool ok = true;
#pragma unroll
  for (int r = 0; r < NU; ++r) {
#pragma unroll
    for (int c = 0; c < r; ++c) {
      double s = Quu(r, c);
#pragma unroll
      for (int m = 0; m < c; ++m) s -= L[r][m] * L[c][m];
      L[r][c] = s / L[c][c];
    }
    double s = Quu(r, r);
#pragma unroll
    for (int m = 0; m < r; ++m) s -= L[r][m] * L[r][m];
    ok = ok && (s > 0.0);
    L[r][r] = __builtin_sqrt(s);
  }
  return ok;
}

// Step 5, one column, in place: q = column j of Qux on entry, column j of K on return
//   forward, r ascending:   s = q[r];  for m < r ascending  s -= L[r][m] * y[m];  y[r] = s / L[r][r]
//   backward, r descending: s = y[r];  for m > r ascending  s -= L[m][r] * z[m];  z[r] = s / L[r][r]
//   K[r][j] = -z[r]
template <int NU>
CDDP_LQR_HD void solve_col(const double (&L)[NU][NU], double (&q)[NU]) {
#pragma unroll
  for (int r = 0; r < NU; ++r) {
    double s = q[r];
#pragma unroll
    for (int m = 0; m < r; ++m) s -= L[r][m] * q[m];
    q[r] = s / L[r][r];
  }
#pragma unroll
  for (int r = NU - 1; r >= 0; --r) {
    double s = q[r];
#pragma unroll
    for (int m = r + 1; m < NU; ++m) s -= L[m][r] * q[m];
    q[r] = s / L[r][r];
  }
#pragma unroll
  for (int r = 0; r < NU; ++r) q[r] = -q[r];
}

// Step 6, column j of Acl (plan_cov.hpp's step 1):  a[i] = A[i][j];  for k ascending  a[i] += B[i][k] * K[k][j]      (kc = column j of K)
template <int NX, int NU, class MA, class MB>
CDDP_LQR_HD void acl_col(int j, const MA &A, const MB &Bm, const double (&kc)[NU], double (&a)[NX]) {
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    double s = A(i, j);
#pragma unroll
    for (int k = 0; k < NU; ++k) s += Bm(i, k) * kc[k];
    a[i] = s;
    CDDP_LQR_FENCE();
  }
}

// Step 7, column j of Y:  y[i] = 0;  for l ascending  y[i] += P[i][l] * Acl[l][j]      (a = column j of Acl)
template <int NX, class MP>
CDDP_LQR_HD void y_col(const MP &P, const double (&a)[NX], double (&y)[NX]) {
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < NX; ++l) s += P(i, l) * a[l];
    y[i] = s;
    CDDP_LQR_FENCE();
  }
}

// Step 8, column j of T:  t[k] = 0;  for m ascending  t[k] += Rd[k][m] * K[m][j]
template <int NU>
CDDP_LQR_HD void t_col(const Weight &Rd, const double (&kc)[NU], double (&tc)[NU]) {
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < NU; ++m) s += Rd(k, m) * kc[m];
    tc[k] = s;
  }
}

// Step 9, the elements j <= i of row i of P' (the Joseph form), each handed to Pout(j, value); a = column i of Acl, kc = column i of K:
//   s = 0;  for l ascending  s += Acl[l][i] * Y[l][j];   h = 0;  for k ascending  h += K[k][i] * T[k][j];   s += h;   s += Qd[i][j]
template <int NX, int NU, class MY, class MT, class PW>
CDDP_LQR_HD void p_row(int i, const double (&a)[NX], const double (&kc)[NU], const MY &Y, const MT &T, const Weight &Qd, const PW &Pout) {
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    if (j <= i) {
      double s = 0.0, h = 0.0;
#pragma unroll
      for (int l = 0; l < NX; ++l) s += a[l] * Y(l, j);
#pragma unroll
      for (int k = 0; k < NU; ++k) h += kc[k] * T(k, j);
      s += h;
      s += Qd(i, j);
      Pout(j, s);
    }
    CDDP_LQR_FENCE();
  }
}

}  // namespace cddp_lqr
