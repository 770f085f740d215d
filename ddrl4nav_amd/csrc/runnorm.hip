// Running observation and return normalisation of the device rollouts (include/ddrl.h ddrl_op_column_moments / _running_merge /
// _running_affine / _normalize_columns / _discounted_returns).  The reference defines RunningMeanStd
// (USTC_lab/env/gym_env/wrapper/warputils.py:83-109, Chan's parallel update) and uses it nowhere; here its update runs on the device, on
// per-column sums of the rows a rollout stores.  Context-free, no allocation, no atomics; sums in double in an order that the arguments
// alone fix (never the pointer's alignment), so repeats -- and an aligned and an unaligned call -- are bit-identical.
#include "rows.h"

namespace ddrl {

// ---- column moments: n, sum x_j, sum x_j^2 of x [n][ld], columns [0, d) ---------------------------------------------------------------
// A 256-thread workgroup takes one tile of CM_COLS * lanes columns x one slab of rows.  `lanes` (a power of two, 1..64: the threads
// along the columns) and `phases` = 256 / lanes (the threads along the rows) depend on d alone: d = 1 puts all 256 threads on rows,
// d >= 253 gives four waves of 64 lanes x 4 columns.  Phase p of a slab adds its rows p, p + phases, ... in ascending order into two
// doubles per column; the phases of a column are folded by a halving tree in LDS; the slab's row of 2 d doubles goes to `ws` and
// column_fold_kernel adds the slabs in slab order.  Which four columns a THREAD holds differs between the 16-byte path (four
// neighbours, one load) and the scalar path (four columns `lanes` apart, coalesced across the lanes): the order in which a COLUMN's
// terms are added does not, so both paths give the same bits.
constexpr int CM_THREADS = 256, CM_COLS = 4, CM_MAX_LANES = 64, CM_MIN_ROWS = 4, CM_MAX_SLABS = 256;

struct MomentsGrid {
  int lanes, phases, ctiles, slabs;
  int64_t slab_rows;
};

inline MomentsGrid moments_grid(int64_t n, int64_t d) {
  MomentsGrid g;
  const int64_t groups = (d + CM_COLS - 1) / CM_COLS;
  g.lanes = 1;
  while (g.lanes < CM_MAX_LANES && g.lanes < groups) g.lanes *= 2;
  g.phases = CM_THREADS / g.lanes;
  g.ctiles = (int)((d + (int64_t)g.lanes * CM_COLS - 1) / ((int64_t)g.lanes * CM_COLS));
  // rows per phase and slab: at least CM_MIN_ROWS, and as many as keep the slabs at CM_MAX_SLABS or fewer
  const int64_t per_phase = (n + g.phases - 1) / g.phases;
  int64_t k = (per_phase + CM_MAX_SLABS - 1) / CM_MAX_SLABS;
  if (k < CM_MIN_ROWS) k = CM_MIN_ROWS;
  g.slab_rows = k * g.phases;
  g.slabs = (int)((n + g.slab_rows - 1) / g.slab_rows);
  return g;
}

template <bool VEC>
__global__ __launch_bounds__(CM_THREADS) void column_moments_kernel(const float* __restrict__ x, int64_t n, int d, int64_t ld, int lanes,
                                                                    int64_t slab_rows, double* __restrict__ part) {
  __shared__ double red[2][CM_THREADS * CM_COLS];  // [sum, sum of squares][phase][column of the tile]
  const int phases = CM_THREADS / lanes, tile_cols = lanes * CM_COLS;
  const int lane = threadIdx.x % lanes, phase = threadIdx.x / lanes;
  const int64_t c0 = (int64_t)blockIdx.x * tile_cols;
  int tc[CM_COLS];  // the thread's columns inside the tile
#pragma unroll
  for (int k = 0; k < CM_COLS; ++k) tc[k] = VEC ? lane * CM_COLS + k : lane + k * lanes;
  const bool whole = c0 + tc[0] + CM_COLS <= d;  // the 16-byte load stays inside the d columns (columns [d, ld) are never read)
  double s1[CM_COLS] = {0.0, 0.0, 0.0, 0.0}, s2[CM_COLS] = {0.0, 0.0, 0.0, 0.0};
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  for (int64_t r = r0 + phase; r < r1; r += phases) {
    const float* row = x + r * ld + c0;
    float v[CM_COLS] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC && whole) {
      const float4 q = *reinterpret_cast<const float4*>(row + tc[0]);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < CM_COLS; ++k)
        if (c0 + tc[k] < d) v[k] = row[tc[k]];
    }
#pragma unroll
    for (int k = 0; k < CM_COLS; ++k) {  // a column past d adds zeros to sums nobody stores
      const double t = (double)v[k];
      s1[k] += t;
      s2[k] += t * t;
    }
  }
#pragma unroll
  for (int k = 0; k < CM_COLS; ++k) {
    red[0][phase * tile_cols + tc[k]] = s1[k];
    red[1][phase * tile_cols + tc[k]] = s2[k];
  }
  __syncthreads();
  for (int half = phases / 2; half >= 1; half /= 2) {  // phase p += phase p + half: the same tree on both paths
    if (phase < half) {
#pragma unroll
      for (int k = 0; k < CM_COLS; ++k) {
        red[0][phase * tile_cols + tc[k]] += red[0][(phase + half) * tile_cols + tc[k]];
        red[1][phase * tile_cols + tc[k]] += red[1][(phase + half) * tile_cols + tc[k]];
      }
    }
    __syncthreads();
  }
  if (phase == 0) {
    double* out = part + (int64_t)blockIdx.y * 2 * d;
#pragma unroll
    for (int k = 0; k < CM_COLS; ++k) {
      const int64_t c = c0 + tc[k];
      if (c < d) {
        out[c] = red[0][tc[k]];
        out[(int64_t)d + c] = red[1][tc[k]];
      }
    }
  }
}

// part [slabs][2 d] -> sums [1 + 2 d]: one thread per entry walks the slabs in slab order; entry 0 is the row count
__global__ __launch_bounds__(256) void column_fold_kernel(const double* __restrict__ part, int slabs, int64_t n, int d,
                                                          double* __restrict__ sums, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * (int64_t)d) return;
  double s = 0.0;
  for (int w = 0; w < slabs; ++w) s += part[(int64_t)w * 2 * d + i];
  sums[1 + i] = accumulate ? sums[1 + i] + s : s;
  if (i == 0) sums[0] = accumulate ? sums[0] + (double)n : (double)n;
}

// ---- RunningMeanStd.update (warputils.py:94-109) from a pending batch's sums, in double, one thread per feature -------------------------
// state = count, mean[d], var[d]; the count is advanced by a launch of its own, behind every thread that reads it
__global__ __launch_bounds__(256) void running_merge_kernel(const double* __restrict__ sums, int d, double* __restrict__ state) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= d) return;
  const double n = sums[0], count = state[0];
  if (!(n > 0.0)) return;
  const double bm = sums[1 + j] / n;
  const double bv = fmax(0.0, sums[1 + (int64_t)d + j] / n - bm * bm);
  const double mean = state[1 + j], var = state[1 + (int64_t)d + j];
  const double delta = bm - mean, tot = count + n;
  state[1 + j] = mean + delta * n / tot;
  state[1 + (int64_t)d + j] = (var * count + bv * n + delta * delta * count * n / tot) / tot;
}
__global__ void running_count_kernel(const double* __restrict__ sums, double* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double n = sums[0];
  if (n > 0.0) state[0] = state[0] + n;
}

// affine [2][d]: shift_j = center ? mean_j : 0, scale_j = 1 / sqrt(var_j + eps) formed in double
__global__ __launch_bounds__(256) void running_affine_kernel(const double* __restrict__ state, int d, double eps, int center,
                                                             float* __restrict__ affine) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= d) return;
  affine[j] = center ? (float)state[1 + j] : 0.0f;
  affine[(int64_t)d + j] = (float)(1.0 / sqrt(state[1 + (int64_t)d + j] + eps));
}

// ---- out[r][j] = clamp((x[r][j] - shift_j) * scale_j, -clip, clip) ----------------------------------------------------------------------
// a NaN fails both comparisons and stays; an infinity goes to the clip
__device__ __forceinline__ float clip_apply(float v, float clip) { return v < -clip ? -clip : (v > clip ? clip : v); }

// threads along the columns in groups of four (a power of two of them, at most 256), the rest of the workgroup along the rows; x and
// out are not __restrict__: out may be x
template <bool VEC>
__global__ __launch_bounds__(256) void normalize_columns_kernel(const float* x, int64_t n, int d, int64_t ld_x,
                                                                const float* __restrict__ affine, float clip, float* out, int64_t ld_out,
                                                                int lanes) {
  const int lane = threadIdx.x % lanes, rows_per = 256 / lanes;
  const int64_t c = ((int64_t)blockIdx.x * lanes + lane) * 4;
  if (c >= d) return;
  float shift[4], scale[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = c + k < d;
    shift[k] = in ? affine[c + k] : 0.0f;
    scale[k] = in ? affine[(int64_t)d + c + k] : 0.0f;
  }
  const bool whole = c + 4 <= d;
  for (int64_t r = (int64_t)blockIdx.y * rows_per + threadIdx.x / lanes; r < n; r += (int64_t)gridDim.y * rows_per) {
    const float* xr = x + r * ld_x + c;
    float* yr = out + r * ld_out + c;
    if (VEC && whole) {
      float4 q = *reinterpret_cast<const float4*>(xr);
      q.x = clip_apply(affine_apply(q.x, shift[0], scale[0]), clip);
      q.y = clip_apply(affine_apply(q.y, shift[1], scale[1]), clip);
      q.z = clip_apply(affine_apply(q.z, shift[2], scale[2]), clip);
      q.w = clip_apply(affine_apply(q.w, shift[3], scale[3]), clip);
      *reinterpret_cast<float4*>(yr) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c + k < d) yr[k] = clip_apply(affine_apply(xr[k], shift[k], scale[k]), clip);  // padding columns are never written
    }
  }
}

// ---- discounted return of every step, one lane per env, forward in time (optim.hip episode_returns_kernel's placement) -----------------
// g = carry * gamma + r[t] (a multiply, then an add); trace[t] = g; carry = dones[t] ? 0 : g; carry [N] persists between calls
__global__ __launch_bounds__(64) void discounted_returns_kernel(const float* __restrict__ rewards, const uint8_t* __restrict__ dones, int T,
                                                                int N, float gamma, float* __restrict__ carry, float* __restrict__ trace) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  float c = carry[n];
#pragma unroll 8
  for (int t = 0; t < T; ++t) {
    const int64_t i = (int64_t)t * N + n;
    const float g = __fadd_rn(__fmul_rn(c, gamma), rewards[i]);
    trace[i] = g;
    c = dones[i] ? 0.0f : g;
  }
  carry[n] = c;
}

// bytes of a [n][ld] float matrix of which columns [0, d) are touched
inline uint64_t matrix_bytes(int64_t n, int64_t d, int64_t ld) { return ((uint64_t)(n - 1) * (uint64_t)ld + (uint64_t)d) * 4; }
// n, d, ld of a matrix argument: positive, ld >= d, and small enough for the byte counts and the grids
inline bool matrix_ok(int64_t n, int64_t d, int64_t ld) {
  return n >= 1 && d >= 1 && ld >= d && d <= (1 << 28) && ld <= INT64_MAX / 8 / n;
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_column_moments_ws_floats(int64_t n, int32_t d, int64_t* floats) {
  if (!floats || n < 1 || n > INT64_MAX / 8 || d < 1 || d > (1 << 28)) return DDRL_ERR_INVALID_ARG;  // the n matrix_ok admits
  *floats = (int64_t)moments_grid(n, d).slabs * 2 * d * 2;
  return DDRL_OK;
}

int32_t ddrl_op_column_moments(const float* x, int64_t n, int32_t d, int64_t ld, double* sums, int32_t accumulate, float* ws, void* stream) {
  if (!x || !sums || !ws || !matrix_ok(n, d, ld)) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)sums & 7) || ((uintptr_t)ws & 7)) return DDRL_ERR_INVALID_ARG;
  const MomentsGrid g = moments_grid(n, d);
  const uint64_t xb = matrix_bytes(n, d, ld), wb = (uint64_t)g.slabs * 2 * d * 8, sb = (uint64_t)(1 + 2 * (int64_t)d) * 8;
  if (overlap(x, ws, xb, wb) || overlap(x, sums, xb, sb) || overlap(ws, sums, wb, sb)) return DDRL_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.ctiles, (unsigned)g.slabs);
  if (aligned16(x) && (ld & 3) == 0)
    hipLaunchKernelGGL(column_moments_kernel<true>, grid, dim3(CM_THREADS), 0, st, x, n, d, ld, g.lanes, g.slab_rows, (double*)ws);
  else
    hipLaunchKernelGGL(column_moments_kernel<false>, grid, dim3(CM_THREADS), 0, st, x, n, d, ld, g.lanes, g.slab_rows, (double*)ws);
  hipLaunchKernelGGL(column_fold_kernel, dim3((unsigned)((2 * (int64_t)d + 255) / 256)), dim3(256), 0, st, (const double*)ws, g.slabs, n, d,
                     sums, accumulate);
  return launch_status();
}

int32_t ddrl_op_running_merge(const double* sums, int32_t d, double* state, void* stream) {
  if (!sums || !state || d < 1 || d > (1 << 28) || ((uintptr_t)sums & 7) || ((uintptr_t)state & 7)) return DDRL_ERR_INVALID_ARG;
  const uint64_t b = (uint64_t)(1 + 2 * (int64_t)d) * 8;
  if (overlap(sums, state, b, b)) return DDRL_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(running_merge_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, sums, d, state);
  hipLaunchKernelGGL(running_count_kernel, dim3(1), dim3(64), 0, st, sums, state);
  return launch_status();
}

int32_t ddrl_op_running_affine(const double* state, int32_t d, double eps, int32_t center, float* affine, void* stream) {
  if (!state || !affine || d < 1 || d > (1 << 28) || ((uintptr_t)state & 7) || ((uintptr_t)affine & 3) || !(eps >= 0.0))
    return DDRL_ERR_INVALID_ARG;
  if (overlap(state, affine, (uint64_t)(1 + 2 * (int64_t)d) * 8, (uint64_t)d * 8)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(running_affine_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state, d, eps, center,
                     affine);
  return launch_status();
}

int32_t ddrl_op_normalize_columns(const float* x, int64_t n, int32_t d, int64_t ld_x, const float* affine, float clip, float* out,
                                  int64_t ld_out, void* stream) {
  if (!x || !affine || !out || !matrix_ok(n, d, ld_x) || !matrix_ok(n, d, ld_out) || !(clip > 0.0f)) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)affine & 3) || ((uintptr_t)out & 3)) return DDRL_ERR_INVALID_ARG;
  const uint64_t xb = matrix_bytes(n, d, ld_x), ob = matrix_bytes(n, d, ld_out), ab = (uint64_t)d * 8;
  const bool in_place = x == out && ld_x == ld_out;  // element for element in place, or apart
  if ((!in_place && overlap(x, out, xb, ob)) || overlap(affine, out, ab, ob)) return DDRL_ERR_INVALID_ARG;
  const int64_t groups = ((int64_t)d + 3) / 4;
  int lanes = 1;
  while (lanes < 256 && lanes < groups) lanes *= 2;
  const int rows_per = 256 / lanes;
  const int64_t row_blocks = (n + rows_per - 1) / rows_per;
  const dim3 grid((unsigned)((groups + lanes - 1) / lanes), (unsigned)(row_blocks < 1024 ? row_blocks : 1024));
  const hipStream_t st = (hipStream_t)stream;
  if (aligned16(x) && aligned16(out) && (ld_x & 3) == 0 && (ld_out & 3) == 0)
    hipLaunchKernelGGL(normalize_columns_kernel<true>, grid, dim3(256), 0, st, x, n, d, ld_x, affine, clip, out, ld_out, lanes);
  else
    hipLaunchKernelGGL(normalize_columns_kernel<false>, grid, dim3(256), 0, st, x, n, d, ld_x, affine, clip, out, ld_out, lanes);
  return launch_status();
}

int32_t ddrl_op_discounted_returns(const float* rewards, const uint8_t* dones, int32_t T, int32_t N, float gamma, float* carry, float* trace,
                                   void* stream) {
  if (!rewards || !dones || !carry || !trace || T < 1 || N < 1 || !(gamma >= 0.0f && gamma <= 1.0f)) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)rewards & 3) || ((uintptr_t)carry & 3) || ((uintptr_t)trace & 3)) return DDRL_ERR_INVALID_ARG;
  const uint64_t tn = (uint64_t)T * (uint64_t)N;
  const void* src[3] = {rewards, dones, carry};  // the carry is read and written by its own lane alone
  const uint64_t src_b[3] = {tn * 4, tn, (uint64_t)N * 4};
  void* dst[2] = {trace, carry};
  const uint64_t dst_b[2] = {tn * 4, (uint64_t)N * 4};
  for (int k = 0; k < 2; ++k)
    for (int s = 0; s < 3; ++s)
      if (!(s == 2 && k == 1) && overlap(src[s], dst[k], src_b[s], dst_b[k])) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(discounted_returns_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, rewards, dones, T, N, gamma,
                     carry, trace);
  return launch_status();
}

}  // extern "C"
