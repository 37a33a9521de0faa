// Device-routine probe: extern "C" entry points that run ONE product routine per item on the GPU (libcddp_hip_probe.so; test
// infrastructure, nothing of it is linked into libcddp_hip.so).  Built by cddp-cpp_amd/csrc/Makefile with the product's FLAGS: the
// arithmetic switches (-ffp-contract=off -fno-signed-zeros -DCDDP_TRIG_SHARED=1) are what is under test.
//
// Every entry point takes host arrays in batch-minor layout (element e of item i at [e * B + i]), allocates, copies, launches,
// copies back and frees by itself, and returns the hipError_t.  One item per lane, 64 threads per block, plain loads and stores;
// the cooperative LDLT kernels run one item per group of G lanes and keep the system in LDS, as the terminal-equality sweep does.
#include <hip/hip_runtime.h>
#include "../../cddp-cpp_amd/csrc/kernels_te.hpp"   // ldlt_mem_compute_coop, ldlt_mem_solve, ldlt_lds_solve, singular_minmax_mem
#include "dev_probe_cases.hpp"

namespace probe {

// ---- device-only cases -----------------------------------------------------------------------------------------------------------
struct CaseSingular {   // in = n, A[16 * 16] (leading dimension 16); out = smax, smin of singular_minmax<16> (te_backward's instantiation), of
                        // singular_minmax_mem, and -- for n <= 8, on the block repacked to leading dimension 8 -- of singular_minmax<8> (the stack-fed sweep's)
  static constexpr int NP = 16, NS = 8, NIN = 1 + NP * NP, NOUT = 6;
  static DEV void run(const Io &io) {
    int n = (int)io.get(0);
    n = n < 0 ? 0 : (n > NP ? NP : n);
    double A[NP * NP], U[NP * NP], A8[NS * NS];
    for (int e = 0; e < NP * NP; ++e) A[e] = io.get(1 + e);
    for (int i = 0; i < NS; ++i) for (int j = 0; j < NS; ++j) A8[i * NS + j] = A[i * NP + j];
    double a, b, c, d, e8 = 0.0, f8 = 0.0;
    singular_minmax<NP>(A, n, a, b);
    singular_minmax_mem(U, A, n, NP, c, d);
    if (n <= NS) singular_minmax<NS>(A8, n, e8, f8);
    io.put(0, a); io.put(1, b); io.put(2, c); io.put(3, d); io.put(4, e8); io.put(5, f8);
  }
};

template <class C>
__global__ void __launch_bounds__(64) k_lane(const double *in, double *out, int B) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < B) C::run(Io{in, out, (size_t)B, (size_t)i});
}

// ldlt_lds_solve<N>: in = F[N * N + N] (the factor as LDLTs stores it, then the transpositions as doubles), x[N]; out = x[N].
// Each lane keeps its factor in its own slice of LDS.
template <int N>
__global__ void __launch_bounds__(64) k_lds_solve(const double *in, double *out, int B) {
  constexpr int NF = N * N + N;
  __shared__ double lds[64 * NF];
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  double *F = lds + threadIdx.x * NF;
  for (int e = 0; e < NF; ++e) F[e] = in[(size_t)e * B + i];
  double x[N];
#pragma unroll
  for (int e = 0; e < N; ++e) x[e] = in[(size_t)(NF + e) * B + i];
  lds_sync();
  ldlt_lds_solve<N>(F, x);
#pragma unroll
  for (int e = 0; e < N; ++e) out[(size_t)e * B + i] = x[e];
}

// ldlt_mem_compute_coop<G, PM> + ldlt_mem_solve: one item per group of G lanes, 64 / G items per block, leading dimension PM + 1.
// in = n, A[PM * (PM + 1)], b[PM]; out = ok, transpositions[PM] (-1 beyond n), m[PM * (PM + 1)], x[PM].
template <int G, int PM>
__global__ void __launch_bounds__(64) k_ldlt_coop(const double *in, double *out, int B) {
  constexpr int TPW = 64 / G, LD = PM + 1, NM = PM * LD, REC = NM + 3 * PM;
  __shared__ double lds[TPW * REC];
  const int tl = threadIdx.x / G, q = threadIdx.x - tl * G;
  const int i = blockIdx.x * TPW + tl;
  if (i >= B) return;   // the whole group leaves
  const unsigned long long gmask = ((G == 64) ? ~0ull : ((1ull << G) - 1ull)) << (tl * G);
  double *m = lds + tl * REC, *trd = m + NM, *temp = trd + PM, *x = temp + PM;
  int n = (int)in[i];
  n = n < 0 ? 0 : (n > PM ? PM : n);
  for (int e = q; e < NM; e += G) m[e] = in[(size_t)(1 + e) * B + i];
  for (int e = q; e < PM; e += G) { trd[e] = -1.0; temp[e] = 0.0; x[e] = in[(size_t)(1 + NM + e) * B + i]; }
  lds_sync();
  const bool ok = ldlt_mem_compute_coop<G, PM>(m, trd, temp, n, LD, q, gmask);
  if (q == 0) ldlt_mem_solve(m, trd, n, LD, x);
  lds_sync();
  if (q == 0) out[i] = ok ? 1.0 : 0.0;
  for (int e = q; e < PM; e += G) {
    out[(size_t)(1 + e) * B + i] = trd[e];
    out[(size_t)(1 + PM + NM + e) * B + i] = e < n ? x[e] : 0.0;
  }
  for (int e = q; e < NM; e += G) out[(size_t)(1 + PM + e) * B + i] = m[e];
}

template <class K>
int run(K kernel, int nin, int nout, int per_block, const double *in, double *out, int B) {
  if (B <= 0) return (int)hipErrorInvalidValue;
  double *din = nullptr, *dout = nullptr;
  const size_t bi = (size_t)nin * B * sizeof(double), bo = (size_t)nout * B * sizeof(double);
  hipError_t e = hipMalloc(&din, bi);
  if (e == hipSuccess) e = hipMalloc(&dout, bo);
  if (e == hipSuccess) e = hipMemcpy(din, in, bi, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, bo);
  if (e == hipSuccess) {
    kernel<<<dim3((B + per_block - 1) / per_block), dim3(64)>>>(din, dout, B);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

}  // namespace probe

#define PROBE_ENTRY(name, KERNEL, NIN_, NOUT_, PER_BLOCK)                                                       \
  extern "C" int probe_##name(const double *in, double *out, int B) { return probe::run(KERNEL, NIN_, NOUT_, PER_BLOCK, in, out, B); } \
  extern "C" void probe_##name##_dims(int *nin, int *nout) { *nin = NIN_; *nout = NOUT_; }
#define PROBE_LANE(name, C) PROBE_ENTRY(name, (probe::k_lane<C>), C::NIN, C::NOUT, 64)
#define PROBE_LDS_SOLVE(N) PROBE_ENTRY(lds_solve_##N, (probe::k_lds_solve<N>), (N * N + 2 * N), N, 64)
#define PROBE_COOP(G, PM) PROBE_ENTRY(ldlt_coop_##G##_##PM, (probe::k_ldlt_coop<G, PM>), (1 + PM * (PM + 1) + PM), (1 + 2 * PM + PM * (PM + 1)), (64 / G))

PROBE_LANE_CASES(PROBE_LANE)
PROBE_LANE(boxqp1_fast, probe::CaseBoxqp1<1>)
PROBE_LANE(singular, probe::CaseSingular)
PROBE_LDS_SOLVE(1) PROBE_LDS_SOLVE(2) PROBE_LDS_SOLVE(3) PROBE_LDS_SOLVE(4) PROBE_LDS_SOLVE(7)
PROBE_COOP(4, 2) PROBE_COOP(8, 6) PROBE_COOP(16, 14)   // TeCfg of the pendulum, 3-DOF arm and 7-joint arm terminal layouts
