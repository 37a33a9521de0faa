// Covariance of a closed-loop plan under an uncertain initial state, process noise and actuator noise: the ONE statement of the step bodies
// that the covariance kernel (inst_cov.hip) runs.  Plain templates, host and device, no other header needed: tests/cpp/test_plan_cov.cpp
// compiles this file with g++ -ffp-contract=off and checks every body bitwise against the sums written out.
//
//   Acl = A + B K;   Z = K Sigma;   SU = Z K^T + Wu;   Y = Acl Sigma;   Sigma' = Acl Y^T + W + (B Wu) B^T
//   cost: sum_i sum_j Qdt[i][j] Sigma[i][j]  +  sum_i sum_j Rdt[i][j] SU[i][j]
//
// The bodies are written per ROW i (a wavefront of the kernel owns one or two rows), on accessors M(i, j) = M[i][j]: a kernel passes the stacks
// where they lie, its LDS buffers and its registers; the CPU test passes arrays.  Every sum is the one include/cddp_hip.h fixes: a stated
// start value, the index ascending -- so who computes an element is free, what it is worth is not.  Symmetric inputs (Sigma0, W, Wu) are
// read through SymLower, which touches the lower triangle only; symmetric results are computed for j <= i and mirrored by the caller.
#pragma once

#if defined(__HIPCC__)
#define CDDP_COV_HD __host__ __device__ __forceinline__
#else
#define CDDP_COV_HD inline
#endif
// CDDP_COV_FENCE(), between the iterations of the unrolled output loops: on the device the instruction scheduler may not move
// instructions across it.  By itself it does not keep loads of later iterations behind it (the order it meets is already that of the
// selected code); an accessor that passes each address through an empty asm, as inst_cov.hip's Strided<.., true> does, is ordered with
// it, and then the loads in flight are those of one output column (profiles/r17_plan_covariance.md, section 1).  No effect on values.
// CDDP_COV_PIN(x), on the results of a body: the value is in a register here.  Without it the compiler sinks the tail of the sums of one
// body into the next one and keeps their operands alive instead (1 KB of scratch per lane at nx = 14); no effect on values either.
#if defined(__HIP_DEVICE_COMPILE__)
#define CDDP_COV_FENCE() __builtin_amdgcn_sched_barrier(0)
#define CDDP_COV_PIN(x) asm volatile("" : "+v"(x))
#else
#define CDDP_COV_FENCE() ((void)0)
#define CDDP_COV_PIN(x) ((void)0)
#endif

namespace cddp_cov {

// A row-major matrix in an array: the accessor of the CPU test and of the cost matrices
struct Dense {
  const double *m; int cols;
  CDDP_COV_HD double operator()(int i, int j) const { return m[i * cols + j]; }
};

// A symmetric n x n matrix of which only the lower triangle (j <= i) is ever read: element (i, j) with j > i is element (j, i).
// m = nullptr: the matrix is not given (W, Wu), and the bodies leave its term out
struct SymLower {
  const double *m; int n;
  CDDP_COV_HD double operator()(int i, int j) const { return j <= i ? m[i * n + j] : m[j * n + i]; }
};

// The bodies take RW rows at once, row[q] < NX, ascending in q (a kernel whose wavefront has a row too many passes a row twice): an element
// of K_t, Sigma_t or Y that several rows need is fetched once and used for all of them at once.

// Steps 1 and 2 in one pass over K_t, for rows row[q] of Acl and columns row[q] of Z:
//   a[q][j] = A[i][j];  for k ascending  a[q][j] += B[i][k] * K[k][j]
//   z = 0;              for l ascending  z += K[k][l] * Sigma[l][i];   Zout(q, k, z)        (WANT_Z; otherwise Zout is not called)
// k is the outer and l the inner index, so every element of K_t is fetched once and both orders are the stated ones.
template <int NX, int NU, int RW, bool WANT_Z, class MA, class MB, class MK, class MS, class ZW>
CDDP_COV_HD void acl_z(const int (&row)[RW], const MA &A, const MB &Bm, const MK &K, const MS &Sig, double (&a)[RW][NX], const ZW &Zout) {
#pragma unroll
  for (int q = 0; q < RW; ++q) {
#pragma unroll
    for (int j = 0; j < NX; ++j) a[q][j] = A(row[q], j);
  }
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    double s[RW], b[RW];
#pragma unroll
    for (int q = 0; q < RW; ++q) { s[q] = 0.0; b[q] = Bm(row[q], k); }
#pragma unroll
    for (int l = 0; l < NX; ++l) {
      const double kv = K(k, l);
#pragma unroll
      for (int q = 0; q < RW; ++q) {
        a[q][l] += b[q] * kv;
        if (WANT_Z) s[q] += kv * Sig(l, row[q]);
      }
    }
    if (WANT_Z) {
#pragma unroll
      for (int q = 0; q < RW; ++q) Zout(q, k, s[q]);
    }
    CDDP_COV_FENCE();
  }
#pragma unroll
  for (int q = 0; q < RW; ++q) {
#pragma unroll
    for (int j = 0; j < NX; ++j) CDDP_COV_PIN(a[q][j]);
  }
}

// Step 3, the rows row[q] < NU of SU in full (only_diag: their diagonal elements alone, the rest 0); rows row[q] >= NU are left alone.
// Element (i, j) is element (r, c) = (max, min), so the row is the mirror of what the other rows' owners compute:
//   s = 0;  for l ascending  s += Z[r][l] * K[c][l];  then  s += Wu[r][c]  if given
template <int NX, int NU, int RW, class MZ, class MK>
CDDP_COV_HD void su_rows(const int (&row)[RW], const MZ &Z, const MK &K, const SymLower &Wu, bool only_diag, double (&u)[RW][NU]) {
#pragma unroll
  for (int j = 0; j < NU; ++j) {
#pragma unroll
    for (int q = 0; q < RW; ++q) {
      const int i = row[q];
      if (i >= NU) continue;
      if (only_diag && j != i) { u[q][j] = 0.0; continue; }
      const int r = j > i ? j : i, c = j > i ? i : j;
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < NX; ++l) s += Z(r, l) * K(c, l);
      if (Wu.m) s += Wu(r, c);
      u[q][j] = s;
      CDDP_COV_PIN(u[q][j]);
      CDDP_COV_FENCE();
    }
    CDDP_COV_FENCE();
  }
}

// Step 4, rows of Y:  y = 0;  for l ascending  y += Acl[i][l] * Sigma[l][j];  Yout(q, j, y)
template <int NX, int RW, class MS, class YW>
CDDP_COV_HD void y_rows_to(const double (&a)[RW][NX], const MS &Sig, const YW &Yout) {
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    double s[RW];
#pragma unroll
    for (int q = 0; q < RW; ++q) s[q] = 0.0;
#pragma unroll
    for (int l = 0; l < NX; ++l) {
      const double sv = Sig(l, j);
#pragma unroll
      for (int q = 0; q < RW; ++q) s[q] += a[q][l] * sv;
    }
#pragma unroll
    for (int q = 0; q < RW; ++q) Yout(q, j, s[q]);
    CDDP_COV_FENCE();
  }
}
// ... into an array
template <int NX, int RW, class MS>
CDDP_COV_HD void y_rows(const double (&a)[RW][NX], const MS &Sig, double (&y)[RW][NX]) {
  y_rows_to<NX, RW>(a, Sig, [&](int q, int j, double v) { y[q][j] = v; CDDP_COV_PIN(y[q][j]); });
}

// Step 2 alone, the columns row[q] of Z:  z = 0;  for l ascending  z += K[k][l] * Sigma[l][i];  Zout(q, k, z)
template <int NX, int NU, int RW, class MK, class MS, class ZW>
CDDP_COV_HD void z_cols(const int (&row)[RW], const MK &K, const MS &Sig, const ZW &Zout) {
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    double s[RW];
#pragma unroll
    for (int q = 0; q < RW; ++q) s[q] = 0.0;
#pragma unroll
    for (int l = 0; l < NX; ++l) {
      const double kv = K(k, l);
#pragma unroll
      for (int q = 0; q < RW; ++q) s[q] += kv * Sig(l, row[q]);
    }
#pragma unroll
    for (int q = 0; q < RW; ++q) Zout(q, k, s[q]);
    CDDP_COV_FENCE();
  }
}

// Step 5, the elements j <= i of rows i = row[q] (ascending in q) of Sigma', each handed to Nout(q, j, value); a = the rows of Acl, Y(j, l) = Y[j][l]:
//   s = 0;  for l ascending  s += Acl[i][l] * Y[j][l];  s += W[i][j] if given;
//   HAVE_WU (Wu is not looked at otherwise):  g[k] = 0;  for m ascending  g[k] += B[i][m] * Wu[m][k];   h = 0;  for k ascending  h += g[k] * B[j][k];  s += h
template <int NX, int NU, int RW, bool HAVE_WU, class MY, class MB, class NW>
CDDP_COV_HD void next_rows_to(const int (&row)[RW], const double (&a)[RW][NX], const MY &Y, const SymLower &W, const SymLower &Wu, const MB &Bm, const NW &Nout) {
  double g[RW][NU];
#pragma unroll
  for (int q = 0; q < RW; ++q) {
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      double s = 0.0;
      if (HAVE_WU) {
#pragma unroll
        for (int m = 0; m < NU; ++m) s += Bm(row[q], m) * Wu(m, k);
      }
      g[q][k] = s;
      CDDP_COV_PIN(g[q][k]);
    }
  }
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    // rows ascending: column j belongs to the rows from the first one with j <= row[q] on; the rows before it skip their sums
    int q0 = RW;
#pragma unroll
    for (int q = RW - 1; q >= 0; --q) if (j <= row[q]) q0 = q;
#pragma unroll
    for (int first = 0; first < RW; ++first) {
      if (q0 != first) continue;
      double s[RW], h[RW];
#pragma unroll
      for (int q = first; q < RW; ++q) { s[q] = 0.0; h[q] = 0.0; }
#pragma unroll
      for (int l = 0; l < NX; ++l) {
        const double yv = Y(j, l);
#pragma unroll
        for (int q = first; q < RW; ++q) s[q] += a[q][l] * yv;
      }
      if (HAVE_WU) {
#pragma unroll
        for (int k = 0; k < NU; ++k) {
          const double bv = Bm(j, k);
#pragma unroll
          for (int q = first; q < RW; ++q) h[q] += g[q][k] * bv;
        }
      }
#pragma unroll
      for (int q = first; q < RW; ++q) {
        double v = s[q];
        if (W.m) v += W(row[q], j);
        if (HAVE_WU) v += h[q];
        Nout(q, j, v);
      }
    }
    CDDP_COV_FENCE();
  }
}

// ... into an array (n[q][j] for j > row[q] is left alone)
template <int NX, int NU, int RW, bool HAVE_WU, class MY, class MB>
CDDP_COV_HD void next_rows(const int (&row)[RW], const double (&a)[RW][NX], const MY &Y, const SymLower &W, const SymLower &Wu, const MB &Bm, double (&n)[RW][NX]) {
  next_rows_to<NX, NU, RW, HAVE_WU>(row, a, Y, W, Wu, Bm, [&](int q, int j, double v) { n[q][j] = v; CDDP_COV_PIN(n[q][j]); });
}

// Step 6, row i of a trace:  r = 0;  for j ascending  r += Q[i][j] * M[i][j]
template <int NN, class MQ, class MM>
CDDP_COV_HD double trace_row(int i, const MQ &Q, const MM &M) {
  double r = 0.0;
#pragma unroll
  for (int j = 0; j < NN; ++j) r += Q(i, j) * M(i, j);
  return r;
}

}  // namespace cddp_cov
