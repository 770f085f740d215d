// Navigation episode statistics on the device (include/ddrl.h ddrl_op_nav_status_*): the reference's
// Status.update_nav_status (USTC_lab/agent/statistics.py:66-116) over the info words of ddrl_op_nav_env_step_info, and the sums its
// group_logger reduces (232-254).  tests/nav_status_ref.py is the numpy model.  Every accumulated quantity is an integer or a multiple
// of 2^-6 below 2^24, so every fp32 operation below is exact and the per-env state equals the reference's bit for bit.  Context-free, no
// allocation, no atomics; the same arguments give the same bits.
#include "rows.h"

namespace ddrl {

constexpr int NST_THREADS = 256;
constexpr int NST_ROWS = DDRL_NAV_STATUS_ROWS, NST_RINGS = DDRL_NAV_STATUS_RINGS, NST_WINDOW = DDRL_NAV_STATUS_WINDOW;
constexpr int NST_SUMMARY = DDRL_NAV_STATUS_SUMMARY;
// rows of `sums` [18][N]: three families (every step, steps close to a pedestrian, steps in the open) of six
enum { NSR_V_SUM = 0, NSR_V_EPISODE, NSR_W_SUM, NSR_W_EPISODE, NSR_STEPS_SUM, NSR_STEPS_EPISODE, NSR_FAMILY };
enum { NSG_ARRIVE = 0, NSG_STATIC, NSG_PED, NSG_ROBOT, NSG_TRUNC };  // rings [5][100][N]
static_assert(NST_ROWS == 3 * NSR_FAMILY && NST_RINGS == NSG_TRUNC + 1, "layout of include/ddrl.h");
static_assert(NST_SUMMARY == 2 * 11, "four rates, six speed means, the steps: (sum, count) each");

// the ring slot of episode `ep`: numpy's non-negative remainder, so a corrupted counter cannot address outside the ring
__device__ __forceinline__ int nst_slot(int ep) {
  const int m = ep % NST_WINDOW;
  return m < 0 ? m + NST_WINDOW : m;
}

// x += add; episode = episode * (1 - d) + x * d; x *= (1 - d): the reference's three lines, in its order (no contraction: the build
// passes -ffp-contract=off)
__device__ __forceinline__ void nst_step(float& sum, float& episode, float add, float d) {
  sum += add;
  episode = episode * (1.0f - d) + sum * d;
  sum *= (1.0f - d);
}

// One lane per env: T successive update_nav_status calls.  The ring slot of the running episode is overwritten by every step in the
// reference; here it lives in registers and is stored when the episode ends and once behind the last step, which leaves the same memory.
__global__ __launch_bounds__(NST_THREADS) void nav_status_update_kernel(const int32_t* __restrict__ info, int T, int N,
                                                                        float* __restrict__ sums, int32_t* __restrict__ episode_num,
                                                                        float* __restrict__ rings) {
  const int n = blockIdx.x * NST_THREADS + threadIdx.x;
  if (n >= N) return;
  float r[NST_ROWS];
#pragma unroll
  for (int k = 0; k < NST_ROWS; ++k) r[k] = sums[(int64_t)k * N + n];
  int ep = episode_num[n];
  float slot[NST_RINGS];
  bool pending = false;
  for (int t = 0; t < T; ++t) {
    const int w = info[(int64_t)t * N + n];
    const int kind = (w >> 2) & 3;
    const float d = (float)(w & 1);
    const float close = (float)((w >> 5) & 1);
    const float av = fabsf((float)((w >> 8) & 63) * 0.03125f), aw = fabsf((float)(((w >> 16) & 255) - 64) * 0.015625f);
    slot[NSG_ARRIVE] = (float)((w >> 1) & 1);
    slot[NSG_STATIC] = kind == 1 ? 1.0f : 0.0f;
    slot[NSG_PED] = kind == 2 ? 1.0f : 0.0f;
    slot[NSG_ROBOT] = kind == 3 ? 1.0f : 0.0f;
    slot[NSG_TRUNC] = (float)((w >> 4) & 1);
    pending = true;
    if (w & 1) {
      const int64_t at = (int64_t)nst_slot(ep) * N + n;
#pragma unroll
      for (int g = 0; g < NST_RINGS; ++g) rings[(int64_t)g * NST_WINDOW * N + at] = slot[g];
      ++ep;
      pending = false;
    }
    nst_step(r[NSR_V_SUM], r[NSR_V_EPISODE], av, d);
    nst_step(r[NSR_W_SUM], r[NSR_W_EPISODE], aw, d);
    float* c = r + NSR_FAMILY;
    nst_step(c[NSR_V_SUM], c[NSR_V_EPISODE], av * close, d);
    nst_step(c[NSR_W_SUM], c[NSR_W_EPISODE], aw * close, d);
    nst_step(c[NSR_STEPS_SUM], c[NSR_STEPS_EPISODE], 1.0f * close, d);
    float* o = r + 2 * NSR_FAMILY;
    nst_step(o[NSR_V_SUM], o[NSR_V_EPISODE], av * (1.0f - close), d);
    nst_step(o[NSR_W_SUM], o[NSR_W_EPISODE], aw * (1.0f - close), d);
    nst_step(o[NSR_STEPS_SUM], o[NSR_STEPS_EPISODE], 1.0f * (1.0f - close), d);
    nst_step(r[NSR_STEPS_SUM], r[NSR_STEPS_EPISODE], 1.0f, d);
  }
  if (pending) {
    const int64_t at = (int64_t)nst_slot(ep) * N + n;
#pragma unroll
    for (int g = 0; g < NST_RINGS; ++g) rings[(int64_t)g * NST_WINDOW * N + at] = slot[g];
  }
#pragma unroll
  for (int k = 0; k < NST_ROWS; ++k) sums[(int64_t)k * N + n] = r[k];
  episode_num[n] = ep;
}

// summary [11][2] = (sum, count) of: reach, static, pedestrian and truncation rate (sum(ring) / clip(episode_num + 1, 1, 100), every
// env counts); v / steps, w / steps of the latest finished episode over all its steps, its close steps and its open steps (fp32
// quotients as the reference forms them, only envs whose steps are > 0 count); steps_episode (every env counts).  One workgroup: a
// thread walks envs tid, tid + 256, ... in ascending order, the lanes fold with the xor butterfly and the four waves in index order.
__global__ __launch_bounds__(NST_THREADS) void nav_status_reduce_kernel(const float* __restrict__ sums,
                                                                        const int32_t* __restrict__ episode_num,
                                                                        const float* __restrict__ rings, int N,
                                                                        double* __restrict__ summary) {
  __shared__ double part[NST_THREADS / 64][NST_SUMMARY];
  double acc[NST_SUMMARY];
#pragma unroll
  for (int k = 0; k < NST_SUMMARY; ++k) acc[k] = 0.0;
  for (int n = threadIdx.x; n < N; n += NST_THREADS) {
    int window = episode_num[n] + 1;
    window = window < 1 ? 1 : (window > NST_WINDOW ? NST_WINDOW : window);
    const int ring_of[4] = {NSG_ARRIVE, NSG_STATIC, NSG_PED, NSG_TRUNC};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* ring = rings + (int64_t)ring_of[q] * NST_WINDOW * N + n;
      float s = 0.0f;  // at most 100 ones: exact in any order
      for (int e = 0; e < NST_WINDOW; ++e) s += ring[(int64_t)e * N];
      acc[2 * q] += (double)s / (double)window;
      acc[2 * q + 1] += 1.0;
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const float* row = sums + (int64_t)f * NSR_FAMILY * N + n;
      const float steps = row[(int64_t)NSR_STEPS_EPISODE * N];
      if (steps > 0.0f) {
        acc[8 + 4 * f] += (double)(row[(int64_t)NSR_V_EPISODE * N] / steps);
        acc[8 + 4 * f + 1] += 1.0;
        acc[8 + 4 * f + 2] += (double)(row[(int64_t)NSR_W_EPISODE * N] / steps);
        acc[8 + 4 * f + 3] += 1.0;
      }
    }
    acc[20] += (double)sums[(int64_t)NSR_STEPS_EPISODE * N + n];
    acc[21] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < NST_SUMMARY; ++k) {
    double s = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NST_SUMMARY) {
    double s = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < NST_THREADS / 64; ++w) s += part[w][threadIdx.x];
    summary[threadIdx.x] = s;
  }
}

// the three state buffers of both operators: given, aligned, apart from one another
inline bool nst_state_ok(const float* sums, const int32_t* episode_num, const float* rings, int32_t N, const void* other, uint64_t other_b,
                         bool other_is_read) {
  if (!sums || !episode_num || !rings || N < 1) return false;
  if (((uintptr_t)sums & 3) || ((uintptr_t)episode_num & 3) || ((uintptr_t)rings & 3)) return false;
  const void* src[1] = {other_is_read ? other : nullptr};
  const uint64_t src_b[1] = {other_b};
  void* dst[4] = {(void*)sums, (void*)episode_num, (void*)rings, other_is_read ? nullptr : (void*)other};
  const uint64_t dst_b[4] = {(uint64_t)NST_ROWS * N * 4, (uint64_t)N * 4, (uint64_t)NST_RINGS * NST_WINDOW * N * 4, other_b};
  return reads_and_writes_apart(src, src_b, 1, dst, dst_b, 4);
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_nav_status_update(const int32_t* info, int32_t T, int32_t N, float* sums, int32_t* episode_num, float* rings,
                                  void* stream) {
  if (T < 0 || (T > 0 && (!info || ((uintptr_t)info & 3)))) return DDRL_ERR_INVALID_ARG;
  if (!nst_state_ok(sums, episode_num, rings, N, T > 0 ? info : nullptr, (uint64_t)T * (uint64_t)(N > 0 ? N : 0) * 4, true))
    return DDRL_ERR_INVALID_ARG;
  if (T == 0) return DDRL_OK;
  hipLaunchKernelGGL(nav_status_update_kernel, dim3((unsigned)((N + NST_THREADS - 1) / NST_THREADS)), dim3(NST_THREADS), 0,
                     (hipStream_t)stream, info, T, N, sums, episode_num, rings);
  return launch_status();
}

int32_t ddrl_op_nav_status_reduce(const float* sums, const int32_t* episode_num, const float* rings, int32_t N, double* summary,
                                  void* stream) {
  if (!summary || ((uintptr_t)summary & 7)) return DDRL_ERR_INVALID_ARG;
  if (!nst_state_ok(sums, episode_num, rings, N, summary, (uint64_t)NST_SUMMARY * 8, false)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(nav_status_reduce_kernel, dim3(1), dim3(NST_THREADS), 0, (hipStream_t)stream, sums, episode_num, rings, N, summary);
  return launch_status();
}

}  // extern "C"
