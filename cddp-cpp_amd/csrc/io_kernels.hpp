// Launchers of the device I/O kernels (inst_io.hip): a resident handle's fields between its internal layouts (io_layout.hpp) and batch-major
// DEVICE arrays, for cddp_hip_get_field_device / cddp_hip_get_results_device / cddp_hip_set_initial_device (capi.hip).  Pure data movement.
// Every launcher enqueues on `stream` and returns; the pointers are device pointers the caller has checked.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "io_layout.hpp"

namespace cddp_dev {

// CDDP_HIP_IO_MAP=naive (read at every call: an experiment switch of profiles/scripts/device_io.py) selects the lane-per-trajectory kernels
// instead of the LDS-staged ones that ship; the results are the same bits.
bool io_map_naive();

// internal -> batch-major: out[b][t][e] for b < B.  layout: cddp_io::Layout; cur / plane: the slot table and plane stride of a slotted field
void io_untile(int layout, const double *src, const int *cur, size_t plane, int B, int NB, int T, int E, double *out, hipStream_t stream);

// batch-major -> wave-tiled seed buffer (d_Xinit, d_Uinit), all NB * 64 lanes of every row: padding lanes 0.0; a trajectory's row t is
// row[b][e] when `row` is given and (t == 0 or src == NULL), else src[b][t][e], else 0.0.
//   X: io_tile(X0, x0, ...)  -- row 0 is x0 (cddp_core.cpp:294), without X0 every row is;   U: io_tile(U0, NULL, ...) -- without U0 zeros
// sel / S (cddp_hip_seed_best): src is [B][S][T][E] and trajectory b takes record max(sel[b], 0) of its S (sel: B int32 on the device)
void io_tile(const double *src, const double *row, int B, int NB, int T, int E, double *dst, hipStream_t stream, const int32_t *sel = nullptr, int S = 1);

// the columns of cddp_hip_result in struct order: cols[b][10] doubles, icols[b][4] int32
struct IoResultSrc { const double *d[10]; const int *i[4]; };
void io_results(const IoResultSrc &src, int B, double *cols, int32_t *icols, hipStream_t stream);

}  // namespace cddp_dev
