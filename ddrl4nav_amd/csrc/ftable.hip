// Frame tables (include/ddrl.h ddrl_op_frame_table_planes / ddrl_op_frame_table_stacks): where the frames of a training call LIE, so
// that the conv1 kernels read them in place (conv2.hip / wgrad2.hip, the indirect instantiations; api.hip ddrl_ppo_iter_indexed)
// instead of from a gathered copy.  tab int32 [n][4]: tab[j][c] = index of the 7,056-byte plane, counted from a plane base pointer, that
// holds channel c of sample j of the call; entries c >= channels repeat entry channels - 1 (the conv1 kernels re-read the last channel
// for the missing ones, so they always load four).
//   single-frame pool (fpool.hip):  (hist + t - min(C - 1 - c, age[b], hist + t)) * n_envs + env   for sample b = t * n_envs + env
//   stacked frames [n_rows][C][84][84]:  b * C + c
// The four float columns and the advantage affine of the gathers ride along (rows.h gather_columns): one launch collates a minibatch
// without touching a frame.  A sample index outside the valid range is CLAMPED to it before anything is read (the gathers return zeros
// for such a sample).  Context-free, no allocation, no atomics: repeats are bit-identical.
// ddrl_op_frame_slot: the table of ONE acting slot of the single-frame pool together with the slot's age row (fpool.hip frame_age_kernel),
// one launch per acting step, for ddrl_forward_indexed.
#include "rows.h"

namespace ddrl {

constexpr int TAB_SAMPLES = 64;  // samples per workgroup: thread (x, y) = (channel / column x, sample y)

// age null: stacked frames (n_envs, hist unused)
__global__ __launch_bounds__(4 * TAB_SAMPLES) void frame_table_kernel(int64_t n_samples, int n_envs, int hist, const uint8_t* __restrict__ age,
                                                                      int channels, const int32_t* __restrict__ idx, int64_t first, int n,
                                                                      int32_t* __restrict__ tab, MinibatchColumns cols,
                                                                      const float* __restrict__ adv_affine) {
  const int c = threadIdx.x, j = blockIdx.x * TAB_SAMPLES + threadIdx.y;
  if (j >= n) return;
  int64_t b = idx != nullptr ? (int64_t)idx[j] : first + j;
  b = b < 0 ? 0 : (b > n_samples - 1 ? n_samples - 1 : b);  // the clamp: age, the columns and the entry all use the clamped sample
  const int cc = c < channels ? c : channels - 1;
  int64_t e;
  if (age != nullptr) {
    const int64_t t = b / n_envs, env = b % n_envs, newest = hist + t;
    int64_t back = channels - 1 - cc;
    const int64_t a = age[b];
    back = a < back ? a : back;
    back = newest < back ? newest : back;  // the rule's own clamp: row >= 0 whatever age holds
    e = (newest - back) * n_envs + env;
  } else {
    e = b * channels + cc;
  }
  tab[(int64_t)j * 4 + c] = (int32_t)e;
  gather_columns(cols, b, true, j, adv_affine);  // threadIdx.x = column
}

static int32_t frame_table(int64_t n_samples, int64_t n_planes, int n_envs, int hist, const uint8_t* age, int channels, const int32_t* idx,
                           int64_t first, int32_t n, int32_t* tab, const MinibatchColumns& cols, const float* adv_affine, void* stream) {
  if (!tab || n < 1 || n_samples < 1 || ((uintptr_t)tab & 3) || ((uintptr_t)idx & 3)) return DDRL_ERR_INVALID_ARG;
  if (!idx && first > INT64_MAX - n) return DDRL_ERR_INVALID_ARG;
  if (n_planes > INT32_MAX) return DDRL_ERR_INVALID_ARG;  // an entry is an int32
  if (!columns_ok(cols, adv_affine)) return DDRL_ERR_INVALID_ARG;
  const uint64_t col_b = (uint64_t)n_samples * 4;
  // what is read against what is written, and the destinations against one another
  const void* src[7] = {age, cols.src[0], cols.src[1], cols.src[2], cols.src[3], idx, adv_affine};
  const uint64_t src_b[7] = {(uint64_t)n_samples, col_b, col_b, col_b, col_b, (uint64_t)n * 4, 8};
  void* dst[5] = {tab, cols.dst[0], cols.dst[1], cols.dst[2], cols.dst[3]};
  const uint64_t dst_b[5] = {(uint64_t)n * 16, (uint64_t)n * 4, (uint64_t)n * 4, (uint64_t)n * 4, (uint64_t)n * 4};
  if (!reads_and_writes_apart(src, src_b, 7, dst, dst_b, 5)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(frame_table_kernel, dim3((unsigned)((n - 1) / TAB_SAMPLES + 1)), dim3(4, TAB_SAMPLES), 0, (hipStream_t)stream, n_samples,
                     n_envs, hist, age, channels, idx, first, n, tab, cols, adv_affine);
  return launch_status();
}

// ---- acting slot t of the single-frame pool: age[i] by the rule of frame_age_kernel (fpool.hip), then the four entries of env i by the
// rule above with newest = hist + t, written as one 16-byte store.  One thread per env.
constexpr int SLOT_THREADS = 64;
using i4v = __attribute__((ext_vector_type(4))) int;
__global__ __launch_bounds__(SLOT_THREADS) void frame_slot_kernel(int n_envs, int newest, int channels, const uint8_t* __restrict__ prev,
                                                                  const uint8_t* __restrict__ reset, uint8_t* __restrict__ age,
                                                                  int32_t* __restrict__ tab) {
  const unsigned i = blockIdx.x * (unsigned)SLOT_THREADS + threadIdx.x;
  if (i >= (unsigned)n_envs) return;
  const int cap = channels - 1;
  int a = 0;
  if (prev != nullptr && (reset == nullptr || reset[i] == 0)) a = (int)prev[i] + 1 < cap ? (int)prev[i] + 1 : cap;
  age[i] = (uint8_t)a;
  i4v e;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int back = cap - (c < channels ? c : cap);
    back = a < back ? a : back;
    back = newest < back ? newest : back;  // the rule's own clamp: row >= 0 (a <= cap already)
    e[c] = (newest - back) * n_envs + (int)i;
  }
  *(i4v*)(tab + (int64_t)i * 4) = e;
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_frame_table_planes(int32_t rows, int32_t n_envs, int32_t hist, const uint8_t* age, int32_t channels, const int32_t* idx,
                                   int64_t first, int32_t n, int32_t* tab, const float* actions, const float* old_logps, const float* advs,
                                   const float* rets, float* actions_dst, float* old_logps_dst, float* advs_dst, float* rets_dst,
                                   const float* adv_affine, void* stream) {
  if (channels < 1 || channels > 4) return DDRL_ERR_UNSUPPORTED;
  if (!age || n_envs < 1 || hist < channels - 1 || rows <= hist) return DDRL_ERR_INVALID_ARG;
  const MinibatchColumns cols{{actions, old_logps, advs, rets}, {actions_dst, old_logps_dst, advs_dst, rets_dst}};
  return frame_table((int64_t)(rows - hist) * n_envs, (int64_t)rows * n_envs, n_envs, hist, age, channels, idx, first, n, tab, cols,
                     adv_affine, stream);
}

int32_t ddrl_op_frame_table_stacks(int64_t n_rows, int32_t channels, const int32_t* idx, int64_t first, int32_t n, int32_t* tab,
                                   const float* actions, const float* old_logps, const float* advs, const float* rets, float* actions_dst,
                                   float* old_logps_dst, float* advs_dst, float* rets_dst, const float* adv_affine, void* stream) {
  if (channels < 1 || channels > 4) return DDRL_ERR_UNSUPPORTED;
  if (n_rows < 1 || n_rows > INT32_MAX / channels) return DDRL_ERR_INVALID_ARG;
  const MinibatchColumns cols{{actions, old_logps, advs, rets}, {actions_dst, old_logps_dst, advs_dst, rets_dst}};
  return frame_table(n_rows, n_rows * channels, 1, 0, nullptr, channels, idx, first, n, tab, cols, adv_affine, stream);
}

int32_t ddrl_op_frame_slot(int32_t rows, int32_t n_envs, int32_t hist, int32_t channels, int32_t t, const uint8_t* prev_age,
                           const uint8_t* reset, uint8_t* age, int32_t* tab, void* stream) {
  if (channels < 1 || channels > 4) return DDRL_ERR_UNSUPPORTED;
  if (!age || !tab || (!prev_age && !reset) || n_envs < 1 || hist < channels - 1) return DDRL_ERR_INVALID_ARG;
  if (t < 0 || (int64_t)hist + t >= rows) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(tab)) return DDRL_ERR_INVALID_ARG;                         // an env's four entries are one 16-byte store
  if ((int64_t)rows * n_envs > INT32_MAX) return DDRL_ERR_INVALID_ARG;  // an entry is an int32
  const uint64_t nb = (uint64_t)n_envs;
  const void* src[2] = {prev_age, reset};
  const uint64_t src_b[2] = {nb, nb};
  void* dst[2] = {age, tab};
  const uint64_t dst_b[2] = {nb, nb * 16};
  if (!reads_and_writes_apart(src, src_b, 2, dst, dst_b, 2)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(frame_slot_kernel, dim3((unsigned)((n_envs - 1) / SLOT_THREADS + 1)), dim3(SLOT_THREADS), 0, (hipStream_t)stream, n_envs,
                     hist + t, channels, prev_age, reset, age, tab);
  return launch_status();
}

}  // extern "C"
