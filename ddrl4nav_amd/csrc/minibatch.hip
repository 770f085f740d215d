// PPO minibatch epochs (include/ddrl.h ddrl_op_moments / _moments_affine / _normalize / _gather_minibatch): the collation of one
// shuffled minibatch -- frame rows and the four float columns of Experience in one launch -- and the advantage normalisation
// (adv - mean) / (std + eps) with the moments, the divisor and the division's stand-in all on the device.  The reference has neither
// (USTC_lab/nn/ppo.py:77-146 runs full-batch iterations on raw advantages).  Context-free, no allocation, no
// atomics; sums in double in a fixed order (rows.h), so repeats are bit-identical.
#include "heads_common.h"
#include "rows.h"

namespace ddrl {

// ---- moments: n, sum x, sum x^2 ----------------------------------------------------------------------------------------------------------
// A thread walks the column 256 * workgroups apart with three double accumulators; lanes by the xor butterfly, the waves in turn
// (heads_common.h turn_add), one row of three doubles per workgroup; rows_fold_kernel<3> adds the rows up.
constexpr int MOM_SLOTS = 3, MOM_THREADS = 256, MOM_PER_THREAD = 4, MOM_MAX_WG = 256;

inline int moments_workgroups(int64_t n) {
  const int64_t per = (int64_t)MOM_THREADS * MOM_PER_THREAD;
  const int64_t w = (n + per - 1) / per;
  return (int)(w < MOM_MAX_WG ? w : MOM_MAX_WG);
}

__global__ __launch_bounds__(MOM_THREADS) void moments_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
  __shared__ double red[MOM_SLOTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double t[MOM_SLOTS] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * MOM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MOM_THREADS) {
    const double v = (double)x[i];
    t[0] += 1.0;
    t[1] += v;
    t[2] += v * v;
  }
#pragma unroll
  for (int k = 0; k < MOM_SLOTS; ++k)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t[k] += __shfl_xor(t[k], off, 64);
  for (int w = 0; w < MOM_THREADS / 64; ++w) {
    if (wave == w && lane == 0) {
#pragma unroll
      for (int k = 0; k < MOM_SLOTS; ++k) turn_add(w == 0, red[k], t[k]);
    }
    __syncthreads();
  }
  if (threadIdx.x < MOM_SLOTS) part[(int64_t)blockIdx.x * MOM_SLOTS + threadIdx.x] = red[threadIdx.x];
}

// ---- the affine pair of (x - mean) / (std + eps), torch's unbiased std; one lane, in double --------------------------------------------
__global__ void moments_affine_kernel(const double* __restrict__ sums3, double eps, float* __restrict__ affine2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double n = sums3[0], s1 = sums3[1], s2 = sums3[2];
  const double mean = s1 / n;
  double var = 0.0;
  if (n >= 2.0) var = fmax(0.0, (s2 - s1 * s1 / n) / (n - 1.0));
  affine2[0] = (float)mean;
  affine2[1] = (float)(1.0 / (sqrt(var) + eps));
}

__global__ __launch_bounds__(256) void normalize_kernel(const float* x, int64_t n, const float* __restrict__ affine2, float* out) {
  const float shift = affine2[0], scale = affine2[1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = affine_apply(x[i], shift, scale);
}

// ---- collation of one minibatch ---------------------------------------------------------------------------------------------------------
// The row mover of rows.h on the frames; the workgroup of a row's first chunk also gathers that row's entry of the four columns
// (rows.h gather_columns).  An index outside [0, n_rows): a zero frame row, zeros in the columns.
__global__ __launch_bounds__(GATHER_THREADS) void gather_minibatch_kernel(const uint4* __restrict__ frames, int64_t n_rows, int64_t row_vecs,
                                                                           int chunks, const int32_t* __restrict__ idx,
                                                                           uint4* __restrict__ frames_dst, MinibatchColumns cols,
                                                                           const float* __restrict__ adv_affine) {
  const int i = blockIdx.x / chunks, c = blockIdx.x % chunks;
  const int64_t r = idx[i];
  const bool ok = r >= 0 && r < n_rows;
  gather_row_chunk(frames, r, ok, row_vecs, c, i, frames_dst);
  if (c == 0) gather_columns(cols, r, ok, i, adv_affine);
}

// ---- one more float column (old_values: the four-column gathers' signatures are fixed) -------------------------------------------------
// dst[j] = src[idx[j]], or src[first + j] without an index; a sample outside [0, n_rows) reads nothing and gives zero
__global__ __launch_bounds__(256) void gather_f32_kernel(const float* __restrict__ src, int64_t n_rows, const int32_t* __restrict__ idx,
                                                         int64_t first, int n, float* __restrict__ dst) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t r = idx ? (int64_t)idx[j] : first + j;
  dst[j] = (r >= 0 && r < n_rows) ? src[r] : 0.0f;
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_moments_ws_floats(int64_t n, int64_t* floats) {
  if (!floats || n < 1) return DDRL_ERR_INVALID_ARG;
  *floats = (int64_t)moments_workgroups(n) * MOM_SLOTS * 2;
  return DDRL_OK;
}

int32_t ddrl_op_moments(const float* x, int64_t n, double* sums3, int32_t accumulate, float* ws, void* stream) {
  if (!x || !sums3 || !ws || n < 1) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)sums3 & 7) || ((uintptr_t)ws & 7)) return DDRL_ERR_INVALID_ARG;
  if (n > INT64_MAX / 4) return DDRL_ERR_INVALID_ARG;
  const int wgs = moments_workgroups(n);
  const uint64_t xb = (uint64_t)n * 4, wb = (uint64_t)wgs * MOM_SLOTS * 8, sb = MOM_SLOTS * 8;
  if (overlap(x, ws, xb, wb) || overlap(x, sums3, xb, sb) || overlap(ws, sums3, wb, sb)) return DDRL_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(moments_kernel, dim3(wgs), dim3(MOM_THREADS), 0, st, x, n, (double*)ws);
  hipLaunchKernelGGL((rows_fold_kernel<MOM_SLOTS, -1>), dim3(1), dim3(MOM_SLOTS * 64), 0, st, (const double*)ws, wgs, sums3, accumulate);
  return launch_status();
}

int32_t ddrl_op_moments_affine(const double* sums3, double eps, float* affine2, void* stream) {
  if (!sums3 || !affine2 || ((uintptr_t)sums3 & 7) || ((uintptr_t)affine2 & 3) || !(eps >= 0.0)) return DDRL_ERR_INVALID_ARG;
  if (overlap(sums3, affine2, MOM_SLOTS * 8, 8)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(moments_affine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums3, eps, affine2);
  return launch_status();
}

int32_t ddrl_op_normalize(const float* x, int64_t n, const float* affine2, float* out, void* stream) {
  if (!x || !affine2 || !out || n < 1 || n > INT64_MAX / 4) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)affine2 & 3) || ((uintptr_t)out & 3)) return DDRL_ERR_INVALID_ARG;
  const uint64_t xb = (uint64_t)n * 4;
  if ((x != out && overlap(x, out, xb, xb)) || overlap(affine2, out, 8, xb)) return DDRL_ERR_INVALID_ARG;  // in place, or apart
  const int64_t w = (n + 1023) / 1024;
  hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)(w < 1024 ? w : 1024)), dim3(256), 0, (hipStream_t)stream, x, n, affine2, out);
  return launch_status();
}

int32_t ddrl_op_gather_minibatch(const uint8_t* frames, int64_t n_rows, int64_t row_bytes, const int32_t* idx, int32_t n,
                                 uint8_t* frames_dst, const float* actions, const float* old_logps, const float* advs, const float* rets,
                                 float* actions_dst, float* old_logps_dst, float* advs_dst, float* rets_dst, const float* adv_affine,
                                 void* stream) {
  if (!frames || !idx || !frames_dst || n < 1 || n_rows < 1 || row_bytes < 16 || (row_bytes & 15)) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(frames) || !aligned16(frames_dst) || ((uintptr_t)idx & 3)) return DDRL_ERR_INVALID_ARG;
  if (n_rows > INT64_MAX / row_bytes) return DDRL_ERR_INVALID_ARG;
  const MinibatchColumns cols{{actions, old_logps, advs, rets}, {actions_dst, old_logps_dst, advs_dst, rets_dst}};
  if (!columns_ok(cols, adv_affine)) return DDRL_ERR_INVALID_ARG;
  // what is read against what is written, and the destinations against one another
  const void* src[7] = {frames, actions, old_logps, advs, rets, idx, adv_affine};
  const uint64_t src_b[7] = {(uint64_t)n_rows * row_bytes, (uint64_t)n_rows * 4, (uint64_t)n_rows * 4, (uint64_t)n_rows * 4,
                             (uint64_t)n_rows * 4, (uint64_t)n * 4, 8};
  void* dst[5] = {frames_dst, actions_dst, old_logps_dst, advs_dst, rets_dst};
  const uint64_t dst_b[5] = {(uint64_t)n * row_bytes, (uint64_t)n * 4, (uint64_t)n * 4, (uint64_t)n * 4, (uint64_t)n * 4};
  if (!reads_and_writes_apart(src, src_b, 7, dst, dst_b, 5)) return DDRL_ERR_INVALID_ARG;
  int64_t row_vecs;
  int chunks;
  if (!gather_grid(row_bytes, n, &row_vecs, &chunks)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gather_minibatch_kernel, dim3((unsigned)(n * chunks)), dim3(GATHER_THREADS), 0, (hipStream_t)stream,
                     (const uint4*)frames, n_rows, row_vecs, chunks, idx, (uint4*)frames_dst, cols, adv_affine);
  return launch_status();
}

int32_t ddrl_op_gather_f32(const float* src, int64_t n_rows, const int32_t* idx, int64_t first, int32_t n, float* dst, void* stream) {
  if (!src || !dst || n < 1 || n_rows < 1 || n_rows > INT64_MAX / 4) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)idx & 3)) return DDRL_ERR_INVALID_ARG;
  if (!idx && (first < INT64_MIN / 2 || first > INT64_MAX / 2)) return DDRL_ERR_INVALID_ARG;  // first + j cannot overflow
  const uint64_t sb = (uint64_t)n_rows * 4, db = (uint64_t)n * 4;
  if (overlap(src, dst, sb, db) || (idx && overlap(idx, dst, db, db))) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gather_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, n_rows, idx, first, n,
                     dst);
  return launch_status();
}

}  // extern "C"
