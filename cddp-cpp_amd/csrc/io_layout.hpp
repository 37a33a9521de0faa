// Index maps between the public batch-major layout [b][t][e] and the layouts a resident handle keeps on the device: the ONE statement of
// them that the device I/O kernels (inst_io.hip) use.  Plain functions, host and device, no other header needed: tests/cpp/test_io_layout.cpp
// compiles this file with g++ and checks every map against the formulas written out.  (capi.hip keeps its own tix / from_soa / from_t4
// for the host getters; the GPU tests hold the two against each other bit for bit.)
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define CDDP_IO_HD __host__ __device__
#else
#define CDDP_IO_HD
#endif

namespace cddp_io {

enum Layout { kTiled = 0, kSlotted = 1, kT4 = 2 };   // wave-tiled stack | plane cur[b] of a slotted field, wave-tiled | sub-tile-minor stack

// batch-major: element e of row t of trajectory b of a [B][T][E] array
CDDP_IO_HD inline size_t batch_major(int b, int T, int t, int E, int e) { return ((size_t)b * (size_t)T + (size_t)t) * (size_t)E + (size_t)e; }

// wave-tiled stack (dev_types.hpp): NB = Bp / 64 tiles of 64 trajectories; the E elements of a step of one tile are adjacent 512-byte records
CDDP_IO_HD inline size_t tiled(int t, int NB, int E, int e, int b) {
  return ((((size_t)t * (size_t)NB + (size_t)(b >> 6)) * (size_t)E + (size_t)e) * 64) + (size_t)(b & 63);
}

// slotted field (X, U, S, Y, G, Lam): the wave-tiled plane `slot` of planes `plane` doubles apart; slot = cur[b], the trajectory's live iterate
CDDP_IO_HD inline size_t slotted(int slot, size_t plane, int t, int NB, int E, int e, int b) { return (size_t)slot * plane + tiled(t, NB, E, e, b); }

// sub-tile-minor stack (kernels.hpp::GT, the A / Bm stacks of a handle with route.t4): sub-tiles of 4 trajectories, 16 per wave tile
CDDP_IO_HD inline size_t t4(int t, int NB, int E, int e, int b) {
  return ((((size_t)t * ((size_t)NB * 16) + (size_t)(b >> 2)) * (size_t)E + (size_t)e) * 4) + (size_t)(b & 3);
}

CDDP_IO_HD inline size_t internal(int layout, int slot, size_t plane, int t, int NB, int E, int e, int b) {
  return layout == kT4 ? t4(t, NB, E, e, b) : layout == kSlotted ? slotted(slot, plane, t, NB, E, e, b) : tiled(t, NB, E, e, b);
}

}  // namespace cddp_io
