// Per-item bodies of the device-routine probe (test infrastructure, never part of the product).
//
// Every case calls ONE product routine of cddp-cpp_amd/csrc (dev_linalg.hpp, dev_boxqp.hpp, dev_trig.hpp; kernels.hpp / kernels_te.hpp
// for the device-only ones) on one item of a batch and writes everything the routine returns.  Nothing of the routines' text is
// repeated here.  The same bodies are compiled twice: by hipcc for gfx950 (dev_probe.hip -> libcddp_hip_probe.so, one item per
// lane) and by g++ for the host (dev_probe_host.cpp, built by tests/dev_probe.py at test time), with the product's
// -ffp-contract=off on both sides, so the two builds can be compared bit for bit.
//
// Layout: batch-minor, element e of item i at [e * B + i], doubles only (sizes, flags, transpositions and statuses travel as doubles).
#pragma once
#ifdef CDDP_PROBE_HOST
#define CDDP_HOST_MODELS 1
#define CDDP_TRIG_HOST 1
#define DEV inline
#endif
#include "../../cddp-cpp_amd/csrc/dev_linalg.hpp"
#include "../../cddp-cpp_amd/csrc/dev_boxqp.hpp"
#include "../../cddp-cpp_amd/csrc/dev_trig.hpp"

namespace probe {
using namespace cddp_dev;

struct Io {
  const double *in;
  double *out;
  size_t B, i;
  DEV double get(int e) const { return in[(size_t)e * B + i]; }
  DEV void put(int e, double v) const { out[(size_t)e * B + i] = v; }
};

// ---- LDLT: in = n, A[NMAX * NMAX] (leading dimension NMAX), b[NMAX]; out = ok, tr[NMAX], m[NMAX * NMAX], x[NMAX] ---------------------
// (entries outside the leading n x n block, which the routines leave untouched, are reported as -1 / 0)
template <int NMAX> DEV int ldltd_tr(const LDLTd<NMAX> &f, int k) { return f.tr[k]; }
template <> DEV int ldltd_tr<2>(const LDLTd<2> &f, int k) { return (k == 0 && f.n == 2 && f.swapped) ? 1 : k; }   // the written-out form keeps one flag

template <int NMAX>
struct CaseLdltd {
  static constexpr int NIN = 1 + NMAX * NMAX + NMAX, NOUT = 1 + NMAX + NMAX * NMAX + NMAX;
  static DEV void run(const Io &io) {
    int n = (int)io.get(0);
    n = n < 0 ? 0 : (n > NMAX ? NMAX : n);
    double A[NMAX * NMAX], x[NMAX];
    for (int e = 0; e < NMAX * NMAX; ++e) A[e] = io.get(1 + e);
    for (int e = 0; e < NMAX; ++e) x[e] = io.get(1 + NMAX * NMAX + e);
    LDLTd<NMAX> f;
    f.compute(A, n);
    f.solve(x);
    io.put(0, f.ok ? 1.0 : 0.0);
    for (int k = 0; k < NMAX; ++k) io.put(1 + k, k < n ? (double)ldltd_tr<NMAX>(f, k) : -1.0);
    for (int i = 0; i < NMAX; ++i)
      for (int j = 0; j < NMAX; ++j) io.put(1 + NMAX + i * NMAX + j, (i < n && j < n) ? f.m[i * NMAX + j] : 0.0);
    for (int k = 0; k < NMAX; ++k) io.put(1 + NMAX + NMAX * NMAX + k, k < n ? x[k] : 0.0);
  }
};

template <int N>
struct CaseLdlts {   // same record as CaseLdltd<N>; the size slot is ignored (n == N)
  static constexpr int NIN = 1 + N * N + N, NOUT = 1 + N + N * N + N;
  static DEV void run(const Io &io) {
    double A[N * N], x[N];
#pragma unroll
    for (int e = 0; e < N * N; ++e) A[e] = io.get(1 + e);
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = io.get(1 + N * N + e);
    LDLTs<N> f;
    f.compute(A, N);
    f.solve(x);
    io.put(0, f.ok ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k < N; ++k) io.put(1 + k, (double)f.tr[k]);
#pragma unroll
    for (int e = 0; e < N * N; ++e) io.put(1 + N + e, f.m[e]);
#pragma unroll
    for (int k = 0; k < N; ++k) io.put(1 + N + N * N + k, x[k]);
  }
};

struct CaseLdlt1 {   // in = d, x; out = D^+ x
  static constexpr int NIN = 2, NOUT = 1;
  static DEV void run(const Io &io) { io.put(0, ldlt1_solve(io.get(0), io.get(1))); }
};

template <int N>
struct CaseInverse {   // in = A[N * N]; out = inverse[N * N]
  static constexpr int NIN = N * N, NOUT = N * N;
  static DEV void run(const Io &io) {
    double A[N * N], inv[N * N];
    for (int e = 0; e < N * N; ++e) A[e] = io.get(e);
    inverse_pplu<N>(A, inv);
    for (int e = 0; e < N * N; ++e) io.put(e, inv[e]);
  }
};

template <int N>
struct CaseMinEig {   // in = M[N * N]; out = min_real_eig
  static constexpr int NIN = N * N, NOUT = 1;
  static DEV void run(const Io &io) {
    double M[N * N];
    for (int e = 0; e < N * N; ++e) M[e] = io.get(e);
    io.put(0, min_real_eig<N>(M));
  }
};

struct CaseMadd {   // in = a, b, c; out = madd_2r
  static constexpr int NIN = 3, NOUT = 1;
  static DEV void run(const Io &io) { io.put(0, madd_2r(io.get(0), io.get(1), io.get(2))); }
};

template <int N>
struct CaseAffine {   // in = base, a, k, Krow[N], dx[N]; out = affine_2r<N>
  static constexpr int NIN = 3 + 2 * N, NOUT = 1;
  static DEV void run(const Io &io) {
    double K[N], dx[N];
    for (int j = 0; j < N; ++j) { K[j] = io.get(3 + j); dx[j] = io.get(3 + N + j); }
    io.put(0, affine_2r<N>(io.get(0), io.get(1), io.get(2), K, dx));
  }
};

struct CaseSignMinMax {   // in = a, b; out = sign_of_reduction(a), dmax(a, b), dmin(a, b), dclamp(a, b, 1), dfinite(a)
  static constexpr int NIN = 2, NOUT = 5;
  static DEV void run(const Io &io) {
    const double a = io.get(0), b = io.get(1);
    io.put(0, sign_of_reduction(a));
    io.put(1, dmax(a, b));
    io.put(2, dmin(a, b));
    io.put(3, dclamp(a, b, 1.0));
    io.put(4, dfinite(a) ? 1.0 : 0.0);
  }
};

// ---- BoxQP: in = max_iterations, H[N * N], g[N], lower[N], upper[N], x0[N], r[N];
//             out = status, free[N], x[N], size of the final free factor, y[N] = Hfree.solve(r[0 .. nf)) ----------------------------
DEV cddp_hip_options boxqp_options(int max_it) {   // boxqp.hpp:30-41 defaults, the iteration cap from the case
  cddp_hip_options o = cddp_hip_options();
  o.boxqp_max_iterations = max_it; o.boxqp_min_gradient_norm = 1e-8; o.boxqp_min_relative_improvement = 1e-8;
  o.boxqp_step_decrease_factor = 0.6; o.boxqp_min_step_size = 1e-22; o.boxqp_armijo_constant = 0.1;
  return o;
}

template <int N>
struct CaseBoxqp {
  static constexpr int NIN = 1 + N * N + 5 * N, NOUT = 2 + 3 * N;
  static DEV void run(const Io &io) {
    const cddp_hip_options o = boxqp_options((int)io.get(0));
    double H[N * N], g[N], lo[N], up[N], x[N], y[N];
    for (int e = 0; e < N * N; ++e) H[e] = io.get(1 + e);
    for (int e = 0; e < N; ++e) {
      g[e] = io.get(1 + N * N + e); lo[e] = io.get(1 + N * N + N + e); up[e] = io.get(1 + N * N + 2 * N + e);
      x[e] = io.get(1 + N * N + 3 * N + e); y[e] = io.get(1 + N * N + 4 * N + e);
    }
    int fr[N];
    LDLTd<N> Hfree;
    Hfree.n = 0;   // (no factor is formed when the first pass ends ALL_CLAMPED)
    const int status = boxqp_solve<N>(o, H, g, lo, up, x, fr, Hfree);
    Hfree.solve(y);
    io.put(0, (double)status);
    for (int e = 0; e < N; ++e) { io.put(1 + e, (double)fr[e]); io.put(1 + N + e, x[e]); io.put(2 + 2 * N + e, e < Hfree.n ? y[e] : 0.0); }
    io.put(1 + 2 * N, (double)Hfree.n);
  }
};

// the scalar trace: the records of CaseBoxqp<1> (r is not read, the factor slots are zero)
template <int FORM>   // 0: boxqp_solve1, 1: boxqp_solve1_fast (device only)
struct CaseBoxqp1 {
  static constexpr int NIN = 7, NOUT = 5;
  static DEV void run(const Io &io) {
    const cddp_hip_options o = boxqp_options((int)io.get(0));
    BoxQPConst c; c.load(o);
    double x = io.get(5);
    int fr = -1, status;
#ifndef CDDP_HOST_MODELS
    if (FORM == 1) status = boxqp_solve1_fast(c, io.get(1), io.get(2), io.get(3), io.get(4), x, fr);
    else
#endif
      status = boxqp_solve1(c, io.get(1), io.get(2), io.get(3), io.get(4), x, fr);
    io.put(0, (double)status); io.put(1, (double)fr); io.put(2, x); io.put(3, 0.0); io.put(4, 0.0);
  }
};

// ---- elementary routines --------------------------------------------------------------------------------------------------------
struct CaseSincos {   // in = x; out = sin, cos of sincos_n<1> (fast range + libm fallback), sin, cos of sincos_fast
  static constexpr int NIN = 1, NOUT = 4;
  static DEV void run(const Io &io) {
    const double a = io.get(0);
    double s, c;
    sincos_n<1>(&a, &s, &c);
    const SinCosPair p = sincos_fast(a);
    io.put(0, s); io.put(1, c); io.put(2, p.s); io.put(3, p.c);
  }
};
struct CaseLog { static constexpr int NIN = 1, NOUT = 1; static DEV void run(const Io &io) { io.put(0, log_shared(io.get(0))); } };
struct CaseExp { static constexpr int NIN = 1, NOUT = 1; static DEV void run(const Io &io) { io.put(0, exp_fast(io.get(0))); } };
struct CasePow { static constexpr int NIN = 2, NOUT = 1; static DEV void run(const Io &io) { io.put(0, pow_shared(io.get(0), io.get(1))); } };
struct CaseAsin { static constexpr int NIN = 1, NOUT = 1; static DEV void run(const Io &io) { io.put(0, asin_shared(io.get(0))); } };

}  // namespace probe

// one entry point per line: X(name, case type); both builds expand the list
#define PROBE_LANE_CASES(X) \
  X(ldltd_1, probe::CaseLdltd<1>) X(ldltd_2, probe::CaseLdltd<2>) X(ldltd_3, probe::CaseLdltd<3>) X(ldltd_4, probe::CaseLdltd<4>) \
  X(ldltd_7, probe::CaseLdltd<7>) X(ldltd_8, probe::CaseLdltd<8>) X(ldltd_16, probe::CaseLdltd<16>) \
  X(ldltd_6, probe::CaseLdltd<6>) X(ldltd_14, probe::CaseLdltd<14>) \
  X(ldlts_1, probe::CaseLdlts<1>) X(ldlts_2, probe::CaseLdlts<2>) X(ldlts_3, probe::CaseLdlts<3>) X(ldlts_4, probe::CaseLdlts<4>) \
  X(ldlts_7, probe::CaseLdlts<7>) X(ldlt1, probe::CaseLdlt1) \
  X(inverse_1, probe::CaseInverse<1>) X(inverse_2, probe::CaseInverse<2>) X(inverse_3, probe::CaseInverse<3>) \
  X(inverse_4, probe::CaseInverse<4>) X(inverse_7, probe::CaseInverse<7>) \
  X(mineig_1, probe::CaseMinEig<1>) X(mineig_2, probe::CaseMinEig<2>) X(mineig_3, probe::CaseMinEig<3>) X(mineig_4, probe::CaseMinEig<4>) \
  X(mineig_7, probe::CaseMinEig<7>) \
  X(madd, probe::CaseMadd) X(affine_1, probe::CaseAffine<1>) X(affine_2, probe::CaseAffine<2>) X(affine_4, probe::CaseAffine<4>) \
  X(signminmax, probe::CaseSignMinMax) \
  X(boxqp_1, probe::CaseBoxqp<1>) X(boxqp_2, probe::CaseBoxqp<2>) X(boxqp_3, probe::CaseBoxqp<3>) X(boxqp_4, probe::CaseBoxqp<4>) \
  X(boxqp_7, probe::CaseBoxqp<7>) X(boxqp1, probe::CaseBoxqp1<0>) \
  X(sincos, probe::CaseSincos) X(log, probe::CaseLog) X(exp, probe::CaseExp) X(pow, probe::CasePow) X(asin, probe::CaseAsin)
