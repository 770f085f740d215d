// Rows of device memory that more than one translation unit moves or folds: the 16-byte row mover of the gathers (imit.hip
// ddrl_op_gather_rows_u8, minibatch.hip ddrl_op_gather_minibatch) and the last stage of the fixed-order double sums (diag.hip's eight
// diagnostics sums, minibatch.hip's three moments).
#pragma once
#include "common.h"

namespace ddrl {

// ---- gather: dst[i][:] = src[idx[i]][:] in 16-byte units -------------------------------------------------------------------------------
// A 256-thread workgroup moves GATHER_UNROLL x 256 consecutive units of one row (both loads requested before the first store): a
// 7,056-byte frame is one workgroup, a four-frame stack four.  Workgroup blockIdx.x = i * chunks + c moves chunk c of destination row i;
// the row index is uniform per workgroup.  An index outside [0, n_rows) reads nothing and leaves a zero row.
constexpr int GATHER_THREADS = 256, GATHER_UNROLL = 2, GATHER_CHUNK = GATHER_THREADS * GATHER_UNROLL;

// the launch geometry of n rows of row_bytes: 16-byte units and workgroups per row; false when n * chunks does not fit a grid
inline bool gather_grid(int64_t row_bytes, int32_t n, int64_t* row_vecs, int* chunks) {
  *row_vecs = row_bytes / 16;
  const int64_t c = (*row_vecs + GATHER_CHUNK - 1) / GATHER_CHUNK;
  if (c > INT32_MAX / n) return false;
  *chunks = (int)c;
  return true;
}

// moves chunk c of destination row i from source row r (read only when ok)
__device__ __forceinline__ void gather_row_chunk(const uint4* __restrict__ src, int64_t r, bool ok, int64_t row_vecs, int c, int i,
                                                 uint4* __restrict__ dst) {
  const int64_t u0 = (int64_t)c * GATHER_CHUNK + threadIdx.x;
  uint4 v[GATHER_UNROLL];
#pragma unroll
  for (int t = 0; t < GATHER_UNROLL; ++t) {
    const int64_t u = u0 + t * GATHER_THREADS;
    v[t] = make_uint4(0u, 0u, 0u, 0u);
    if (ok && u < row_vecs) v[t] = src[r * row_vecs + u];
  }
#pragma unroll
  for (int t = 0; t < GATHER_UNROLL; ++t) {
    const int64_t u = u0 + t * GATHER_THREADS;
    if (u < row_vecs) dst[(int64_t)i * row_vecs + u] = v[t];
  }
}

// ---- fold of per-workgroup rows of doubles --------------------------------------------------------------------------------------------
// the larger of two non-negative doubles; a NaN stays visible
__device__ __forceinline__ double diag_max(double a, double b) { return (a > b || a != a) ? a : b; }

// part [nwg][SLOTS] -> sums [SLOTS]: one wave per slot walks the workgroups' rows (ascending, 64 apart per lane) and folds its lanes with
// the xor butterfly -- a fixed order; slot MAX_SLOT (none when < 0) takes the larger instead of the sum.  accumulate: combined with
// what `sums` holds.  One workgroup of SLOTS waves.  No atomics.
template <int SLOTS, int MAX_SLOT>
__global__ __launch_bounds__(SLOTS * 64) void rows_fold_kernel(const double* __restrict__ part, int nwg, double* __restrict__ sums,
                                                                int accumulate) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool is_max = (k == MAX_SLOT);
  double s = 0.0;
  for (int w = lane; w < nwg; w += 64) {
    const double x = part[(int64_t)w * SLOTS + k];
    s = is_max ? diag_max(s, x) : s + x;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double y = __shfl_xor(s, off, 64);
    s = is_max ? diag_max(s, y) : s + y;
  }
  if (lane == 0) {
    if (accumulate) s = is_max ? diag_max(sums[k], s) : sums[k] + s;
    sums[k] = s;
  }
}

}  // namespace ddrl
