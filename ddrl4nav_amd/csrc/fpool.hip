// Single-frame experience pool (include/ddrl.h ddrl_op_frame_age / ddrl_op_gather_frame_stacks): every Atari frame is stored ONCE,
// planes uint8 [hist + T + 1][n_envs][84][84] with row hist + t the one frame that arrived for step t, and a stack is assembled where it
// is read.  age[t][i] = steps since env i's stack was last reset, saturated at C - 1; channel c of sample b = t * n_envs + i is pool row
//   hist + t - min(C - 1 - c, age[b], hist + t)
// of env i: FrameStackWrapper (USTC_lab/env/gym_env/wrapper/warputils.py:112-131; newest plane last, a reset env carries the new frame in
// every plane), what fstack.hip writes out C times.  The last term of the min is a clamp: whatever bytes age holds, no row below 0 is read.
// Context-free, no allocation, no atomics: repeats are bit-identical.
#include "rows.h"

namespace ddrl {

constexpr int PLANE_BYTES = 84 * 84;          // 7,056
constexpr int PLANE_VECS = PLANE_BYTES / 16;  // 441 units of 16 bytes: one chunk of the row mover
static_assert(PLANE_BYTES % 16 == 0 && PLANE_VECS <= GATHER_CHUNK, "a plane is one chunk of whole 16-byte units");

// ---- age[i] = reset[i] ? 0 : min(prev[i] + 1, C - 1); prev null: every env is reset --------------------------------------------------
__global__ __launch_bounds__(256) void frame_age_kernel(const uint8_t* __restrict__ prev, const uint8_t* __restrict__ reset, int n, int cap,
                                                        uint8_t* __restrict__ age) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)n) return;
  int a = 0;
  if (prev != nullptr && (reset == nullptr || reset[i] == 0)) a = (int)prev[i] + 1 < cap ? (int)prev[i] + 1 : cap;
  age[i] = (uint8_t)a;
}

// ---- stacks_dst[j][c] = the plane the rule above names, for sample idx[j] (or first + j) --------------------------------------------
// Workgroup blockIdx.x = j * C + c moves plane c of destination stack j with the row mover of rows.h (one chunk: both loads of a lane
// requested before its first store); the sample index and its age byte are uniform per workgroup.  The workgroup of plane 0 also gathers
// the sample's entry of the four columns.  A sample outside [0, n_samples): a zero stack, zeros in the columns, nothing read.
__global__ __launch_bounds__(GATHER_THREADS) void gather_frame_stacks_kernel(const uint4* __restrict__ planes, int64_t n_samples, int n_envs,
                                                                              int hist, const uint8_t* __restrict__ age, int channels,
                                                                              const int32_t* __restrict__ idx, int64_t first,
                                                                              uint4* __restrict__ stacks_dst, MinibatchColumns cols,
                                                                              const float* __restrict__ adv_affine) {
  const int j = blockIdx.x / channels, c = blockIdx.x % channels;
  const int64_t b = idx != nullptr ? (int64_t)idx[j] : first + j;
  const bool ok = b >= 0 && b < n_samples;
  int64_t r = 0;
  if (ok) {
    const int64_t t = b / n_envs, env = b % n_envs, newest = hist + t;
    int64_t back = channels - 1 - c;
    const int64_t a = age[b];
    back = a < back ? a : back;
    back = newest < back ? newest : back;  // the clamp: row >= 0 whatever age holds
    r = (newest - back) * n_envs + env;
  }
  gather_row_chunk(planes, r, ok, PLANE_VECS, 0, (int)blockIdx.x, stacks_dst);
  if (c == 0) gather_columns(cols, b, ok, j, adv_affine);
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_frame_age(const uint8_t* prev_age, const uint8_t* reset, int32_t n, int32_t channels, uint8_t* age, void* stream) {
  if (channels < 1 || channels > 4) return DDRL_ERR_UNSUPPORTED;  // the range cfg_check accepts for in_channels
  if (!age || n < 1 || (!prev_age && !reset)) return DDRL_ERR_INVALID_ARG;
  const uint64_t nb = (uint64_t)n;
  if ((prev_age && overlap(prev_age, age, nb, nb)) || (reset && overlap(reset, age, nb, nb))) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(frame_age_kernel, dim3((unsigned)((n - 1) / 256 + 1)), dim3(256), 0, (hipStream_t)stream, prev_age, reset, n, channels - 1,
                     age);
  return launch_status();
}

int32_t ddrl_op_gather_frame_stacks(const uint8_t* planes, int32_t rows, int32_t n_envs, int32_t hist, const uint8_t* age, int32_t channels,
                                    const int32_t* idx, int64_t first, int32_t n, uint8_t* stacks_dst, const float* actions,
                                    const float* old_logps, const float* advs, const float* rets, float* actions_dst, float* old_logps_dst,
                                    float* advs_dst, float* rets_dst, const float* adv_affine, void* stream) {
  if (channels < 1 || channels > 4) return DDRL_ERR_UNSUPPORTED;
  if (!planes || !age || !stacks_dst || n < 1 || n_envs < 1 || hist < channels - 1 || rows <= hist) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(planes) || !aligned16(stacks_dst) || ((uintptr_t)idx & 3)) return DDRL_ERR_INVALID_ARG;
  if (!idx && first > INT64_MAX - n) return DDRL_ERR_INVALID_ARG;
  if (n > INT32_MAX / channels) return DDRL_ERR_INVALID_ARG;  // one workgroup per plane written
  const MinibatchColumns cols{{actions, old_logps, advs, rets}, {actions_dst, old_logps_dst, advs_dst, rets_dst}};
  if (!columns_ok(cols, adv_affine)) return DDRL_ERR_INVALID_ARG;
  if ((int64_t)rows * n_envs > INT64_MAX / PLANE_BYTES) return DDRL_ERR_INVALID_ARG;
  const uint64_t n_samples = (uint64_t)(rows - hist) * n_envs, col_b = n_samples * 4;
  // what is read against what is written, and the destinations against one another
  const void* src[8] = {planes, age, actions, old_logps, advs, rets, idx, adv_affine};
  const uint64_t src_b[8] = {(uint64_t)rows * n_envs * PLANE_BYTES, n_samples, col_b, col_b, col_b, col_b, (uint64_t)n * 4, 8};
  void* dst[5] = {stacks_dst, actions_dst, old_logps_dst, advs_dst, rets_dst};
  const uint64_t dst_b[5] = {(uint64_t)n * channels * PLANE_BYTES, (uint64_t)n * 4, (uint64_t)n * 4, (uint64_t)n * 4, (uint64_t)n * 4};
  if (!reads_and_writes_apart(src, src_b, 8, dst, dst_b, 5)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gather_frame_stacks_kernel, dim3((unsigned)(n * channels)), dim3(GATHER_THREADS), 0, (hipStream_t)stream,
                     (const uint4*)planes, (int64_t)n_samples, n_envs, hist, age, channels, idx, first, (uint4*)stacks_dst, cols, adv_affine);
  return launch_status();
}

}  // extern "C"
