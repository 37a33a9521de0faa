// Device I/O kernels of the resident handle: batch-major device arrays <-> the handle's internal layouts (io_layout.hpp).  No arithmetic.
//
// A [B][T][E] batch-major array and a wave-tiled stack are transposes of each other per 64-trajectory tile: with the T * E values of a
// trajectory numbered c = t * E + e ("columns"), batch-major keeps a trajectory's columns adjacent and the stack keeps a column's 64
// trajectories adjacent.  STAGED kernels (shipped): one workgroup per (tile, chunk of kIoCols consecutive columns).  It walks the source along
// ITS contiguous direction into an LDS image [64 trajectories][kIoCols columns], and walks the destination along its own out of it, so both
// sides move whole 512-byte runs.  The image's row pitch is kIoCols + 1 doubles: the column-wise side touches addresses `pitch` doubles apart
// from lane to lane, and both 64-bit LDS instructions of gfx950 are conflict-free exactly when that pitch is odd (ds_write_b64: groups of 16
// lanes over 32 dword banks, lane * pitch mod 16 must be distinct; ds_read_b64: groups of 32 lanes over 64 banks, lane * pitch mod 32); the
// row-wise side is contiguous either way.  NAIVE kernels (CDDP_HIP_IO_MAP=naive, kept for the comparison of profiles/r12_device_io.md):
// lane = trajectory walking e, as k_mpc_log does -- coalesced on the stack, 64 distinct lines per access on the batch-major side.
//
// Bounds: every batch-major access is guarded by b < B and c < T * E; a stack access by the same b and c (untile) or covers the whole padded
// tile b < NB * 64 (tile), which is the extent the seed buffers are allocated with.  A slotted read trusts cur[b] as every kernel of the solver does.
#include "io_kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace cddp_dev {

namespace {

constexpr int kIoCols = 64;              // columns per workgroup: 512 bytes of every trajectory
constexpr int kIoPitch = kIoCols + 1;    // LDS row pitch in doubles, odd (see above)
constexpr int kIoThreads = 256;          // a multiple of 64: a thread's lane on the stack side is threadIdx.x & 63 throughout
constexpr int kIoMaxGridY = 65535;

// the batch-major record trajectory b of a tile kernel reads: its own, or the selected one of its S candidates
__device__ __forceinline__ size_t io_record(const int32_t *sel, int S, int b) {
  if (!sel) return (size_t)b;
  const int w = sel[b];
  return (size_t)b * (size_t)S + (size_t)(w < 0 ? 0 : w);
}

template <int LAYOUT>
__global__ __launch_bounds__(kIoThreads) void k_io_untile(const double *__restrict__ src, const int *__restrict__ cur, size_t plane, int B, int NB, int T, int E,
                                                          int tile0, double *__restrict__ out) {
  __shared__ double img[64 * kIoPitch];
  const int tile = tile0 + (int)blockIdx.y, b0 = tile * 64;
  const int TE = T * E, c0 = (int)blockIdx.x * kIoCols, nc = min(kIoCols, TE - c0), n = nc * 64;
  int slot = 0;
  if (LAYOUT == cddp_io::kSlotted) { const int b = b0 + (int)(threadIdx.x & 63); slot = b < B ? cur[b] : 0; }
  // along the stack.  wave-tiled: a column's 64 lanes are adjacent.  sub-tile-minor: the 4 lanes of a sub-tile, then the columns of one step
  for (int i = threadIdx.x; i < n; i += kIoThreads) {
    int l, col;
    if (LAYOUT == cddp_io::kT4) { col = (i >> 2) % nc; l = (i / (4 * nc)) * 4 + (i & 3); }
    else { l = i & 63; col = i >> 6; }
    const int b = b0 + l;
    if (b >= B) continue;
    const int c = c0 + col, t = c / E, e = c - t * E;
    img[l * kIoPitch + col] = src[cddp_io::internal(LAYOUT, slot, plane, t, NB, E, e, b)];
  }
  __syncthreads();
  // along batch-major: a trajectory's nc columns are adjacent
  for (int i = threadIdx.x; i < n; i += kIoThreads) {
    const int l = i / nc, col = i - l * nc, b = b0 + l;
    if (b < B) out[(size_t)b * (size_t)TE + (size_t)(c0 + col)] = img[l * kIoPitch + col];
  }
}

// sel (cddp_hip_seed_best): trajectory b reads record b * S + max(sel[b], 0) of src instead of record b -- the only difference of the gather
__global__ __launch_bounds__(kIoThreads) void k_io_tile(const double *__restrict__ src, const double *__restrict__ row, int B, int NB, int T, int E, int tile0,
                                                        double *__restrict__ dst, const int32_t *__restrict__ sel, int S) {
  __shared__ double img[64 * kIoPitch];
  const int tile = tile0 + (int)blockIdx.y, b0 = tile * 64;
  const int TE = T * E, c0 = (int)blockIdx.x * kIoCols, nc = min(kIoCols, TE - c0), n = nc * 64;
  if (src) {
    for (int i = threadIdx.x; i < n; i += kIoThreads) {
      const int l = i / nc, col = i - l * nc, b = b0 + l;
      if (b < B) img[l * kIoPitch + col] = src[io_record(sel, S, b) * (size_t)TE + (size_t)(c0 + col)];
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < n; i += kIoThreads) {
    const int l = i & 63, col = i >> 6, b = b0 + l;
    const int c = c0 + col, t = c / E, e = c - t * E;
    double v = 0.0;                                         // padding lanes of the last tile; U without U0
    if (b < B) {
      if (row && (t == 0 || !src)) v = row[(size_t)b * (size_t)E + (size_t)e];
      else if (src) v = img[l * kIoPitch + col];
    }
    dst[cddp_io::tiled(t, NB, E, e, b)] = v;
  }
}

// ---- the lane-per-trajectory forms: blockIdx.x = row t, blockIdx.y = tile, the lane walks e
template <int LAYOUT>
__global__ __launch_bounds__(64) void k_io_untile_naive(const double *__restrict__ src, const int *__restrict__ cur, size_t plane, int B, int NB, int T, int E, int tile0,
                                                        double *__restrict__ out) {
  const int b = (tile0 + (int)blockIdx.y) * 64 + (int)threadIdx.x, t = (int)blockIdx.x;
  if (b >= B) return;
  const int slot = LAYOUT == cddp_io::kSlotted ? cur[b] : 0;
  for (int e = 0; e < E; ++e) out[cddp_io::batch_major(b, T, t, E, e)] = src[cddp_io::internal(LAYOUT, slot, plane, t, NB, E, e, b)];
}

__global__ __launch_bounds__(64) void k_io_tile_naive(const double *__restrict__ src, const double *__restrict__ row, int B, int NB, int T, int E, int tile0,
                                                      double *__restrict__ dst, const int32_t *__restrict__ sel, int S) {
  const int b = (tile0 + (int)blockIdx.y) * 64 + (int)threadIdx.x, t = (int)blockIdx.x;
  for (int e = 0; e < E; ++e) {
    double v = 0.0;
    if (b < B) {
      if (row && (t == 0 || !src)) v = row[(size_t)b * (size_t)E + (size_t)e];
      else if (src) v = src[io_record(sel, S, b) * (size_t)T * (size_t)E + (size_t)t * (size_t)E + (size_t)e];
    }
    dst[cddp_io::tiled(t, NB, E, e, b)] = v;
  }
}

__global__ void k_io_results(IoResultSrc s, int B, double *__restrict__ cols, int32_t *__restrict__ icols) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < 10; ++i) cols[(size_t)b * 10 + i] = s.d[i][b];
  for (int i = 0; i < 4; ++i) icols[(size_t)b * 4 + i] = s.i[i][b];
}

template <int LAYOUT>
void untile_launch(bool naive, const double *src, const int *cur, size_t plane, int B, int NB, int T, int E, double *out, hipStream_t stream) {
  const int tiles = (B + 63) / 64, TE = T * E;
  for (int tile0 = 0; tile0 < tiles; tile0 += kIoMaxGridY) {
    const int ny = std::min(kIoMaxGridY, tiles - tile0);
    if (naive) hipLaunchKernelGGL(k_io_untile_naive<LAYOUT>, dim3(T, ny), dim3(64), 0, stream, src, cur, plane, B, NB, T, E, tile0, out);
    else hipLaunchKernelGGL(k_io_untile<LAYOUT>, dim3((TE + kIoCols - 1) / kIoCols, ny), dim3(kIoThreads), 0, stream, src, cur, plane, B, NB, T, E, tile0, out);
  }
}

}  // namespace

bool io_map_naive() { const char *e = std::getenv("CDDP_HIP_IO_MAP"); return e && !std::strcmp(e, "naive"); }

void io_untile(int layout, const double *src, const int *cur, size_t plane, int B, int NB, int T, int E, double *out, hipStream_t stream) {
  if (B <= 0 || T <= 0 || E <= 0) return;
  const bool naive = io_map_naive();
  if (layout == cddp_io::kT4) untile_launch<cddp_io::kT4>(naive, src, cur, plane, B, NB, T, E, out, stream);
  else if (layout == cddp_io::kSlotted) untile_launch<cddp_io::kSlotted>(naive, src, cur, plane, B, NB, T, E, out, stream);
  else untile_launch<cddp_io::kTiled>(naive, src, cur, plane, B, NB, T, E, out, stream);
}

void io_tile(const double *src, const double *row, int B, int NB, int T, int E, double *dst, hipStream_t stream, const int32_t *sel, int S) {
  if (NB <= 0 || T <= 0 || E <= 0) return;
  const bool naive = io_map_naive();
  const int TE = T * E;
  for (int tile0 = 0; tile0 < NB; tile0 += kIoMaxGridY) {   // every tile of the padded batch: padding lanes are written too
    const int ny = std::min(kIoMaxGridY, NB - tile0);
    if (naive) hipLaunchKernelGGL(k_io_tile_naive, dim3(T, ny), dim3(64), 0, stream, src, row, B, NB, T, E, tile0, dst, sel, S);
    else hipLaunchKernelGGL(k_io_tile, dim3((TE + kIoCols - 1) / kIoCols, ny), dim3(kIoThreads), 0, stream, src, row, B, NB, T, E, tile0, dst, sel, S);
  }
}

void io_results(const IoResultSrc &src, int B, double *cols, int32_t *icols, hipStream_t stream) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_io_results, dim3((B + 255) / 256), dim3(256), 0, stream, src, B, cols, icols);
}

}  // namespace cddp_dev
