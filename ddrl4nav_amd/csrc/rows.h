// Rows of device memory that more than one translation unit moves or folds: the 16-byte row mover of the gathers (imit.hip
// ddrl_op_gather_rows_u8, minibatch.hip ddrl_op_gather_minibatch, fpool.hip ddrl_op_gather_frame_stacks), the float columns the last two
// carry along, and the last stage of the fixed-order double sums (diag.hip's eight diagnostics sums, minibatch.hip's three moments).
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

// ---- the four float columns of Experience that ride along with a gather of frames (minibatch.hip, fpool.hip) ----------------------------
// a subtract, then a multiply (the build keeps them apart: -ffp-contract=off); the one text the column pass and both gathers apply
__device__ __forceinline__ float affine_apply(float x, float shift, float scale) { return (x - shift) * scale; }

struct MinibatchColumns {  // column k: src[k] -> dst[k], both null = not given
  const float* src[4];
  float* dst[4];
};
constexpr int COL_ADV = 2;  // actions, old_logps, advs, rets

// entry i of the four columns from sample r (read only when ok, zeros otherwise), one thread each: threads 0..3 of one workgroup per entry
__device__ __forceinline__ void gather_columns(const MinibatchColumns& cols, int64_t r, bool ok, int i, const float* __restrict__ adv_affine) {
  if (threadIdx.x >= 4) return;
  const int k = threadIdx.x;
  if (cols.dst[k] == nullptr) return;
  float v = 0.0f;
  if (ok) {
    v = cols.src[k][r];
    if (k == COL_ADV && adv_affine != nullptr) v = affine_apply(v, adv_affine[0], adv_affine[1]);
  }
  cols.dst[k][i] = v;
}

// the host's checks of the columns: a column comes with its destination, floats are 4-byte aligned, the affine pair needs the advantages
inline bool columns_ok(const MinibatchColumns& cols, const float* adv_affine) {
  for (int k = 0; k < 4; ++k) {
    if ((cols.src[k] == nullptr) != (cols.dst[k] == nullptr)) return false;
    if (((uintptr_t)cols.src[k] & 3) || ((uintptr_t)cols.dst[k] & 3)) return false;
  }
  return !adv_affine || (cols.src[COL_ADV] && !((uintptr_t)adv_affine & 3));
}

// true when nothing that is read overlaps anything that is written, nor two destinations one another (null entries are not given)
inline bool reads_and_writes_apart(const void* const* src, const uint64_t* src_b, int ns, void* const* dst, const uint64_t* dst_b, int nd) {
  for (int d = 0; d < nd; ++d) {
    if (!dst[d]) continue;
    for (int s = 0; s < ns; ++s)
      if (src[s] && overlap(src[s], dst[d], src_b[s], dst_b[d])) return false;
    for (int e = d + 1; e < nd; ++e)
      if (dst[e] && overlap(dst[d], dst[e], dst_b[d], dst_b[e])) return false;
  }
  return true;
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
