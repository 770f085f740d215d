// Frame stack on the device: FrameStackWrapper (USTC_lab/env/gym_env/wrapper/warputils.py:112-131) as one streaming launch per
// acting step.  The stacked observation of step t+1 is the stack of step t shifted by one plane plus the one new frame per env
// (deque append, :118-121; newest plane LAST, :123-125); a reset env gets the new frame in every plane (:127-131).
#include "common.h"

namespace {

constexpr int PLANE_BYTES = 84 * 84;        // 7,056
constexpr int PLANE_VECS = PLANE_BYTES / 16;  // 441 units of 16 bytes: no tail, and every plane of a 16-byte aligned base is aligned
constexpr int WAVES_PER_ENV = (PLANE_VECS + 63) / 64;  // 7 one-wave workgroups per env (448 lanes, 441 at work)
static_assert(PLANE_BYTES % 16 == 0, "a plane is a whole number of 16-byte units");

// One lane moves unit u of EVERY plane of its env: all C loads (C-1 shifted planes of prev, the new frame) and the env's reset flag
// are issued before the first store, unconditionally -- the flag only selects among values that are already on their way, so there is
// no load behind a load.  The flag's address is uniform per workgroup (one env per workgroup).  Grid: n * 7 workgroups of one wave:
// 1,792 waves of 4 KiB each at n = 256, C = 4 (7 per CU), still 7 waves at n = 1.
template <int C>
__global__ __launch_bounds__(64) void frame_stack_push_kernel(const uint4* __restrict__ prev, const uint4* __restrict__ newest,
                                                              const uint8_t* __restrict__ reset, uint4* __restrict__ next) {
  const int64_t env = blockIdx.x / WAVES_PER_ENV;
  const int u = (blockIdx.x % WAVES_PER_ENV) * 64 + threadIdx.x;
  if (u >= PLANE_VECS) return;
  uint4 v[C];
#pragma unroll
  for (int c = 0; c < C - 1; ++c) v[c] = prev[(env * C + c + 1) * PLANE_VECS + u];
  v[C - 1] = newest[env * PLANE_VECS + u];
  // all-ones for a reset env: the planes are blended bit-wise with the new frame (the compiler makes it one v_cndmask_b32 per dword).  A select between v[c]
  // and v[C - 1] instead becomes an indexed array that the compiler parks in LDS, a branch makes it sink the loads behind the flag.
  const uint32_t m = reset != nullptr && reset[env] != 0 ? 0xffffffffu : 0u;
  const uint4 f = v[C - 1];
  uint4* __restrict__ o = next + env * C * PLANE_VECS + u;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const uint4 p = v[c];
    o[c * PLANE_VECS] = make_uint4((f.x & m) | (p.x & ~m), (f.y & m) | (p.y & ~m), (f.z & m) | (p.z & ~m), (f.w & m) | (p.w & ~m));
  }
}

}  // namespace

extern "C" int32_t ddrl_frame_stack_push(const uint8_t* prev, const uint8_t* newest, const uint8_t* reset, int32_t n,
                                         int32_t channels, uint8_t* next, void* stream) {
  // every check comes before the first HIP call: a host without a GPU gets the same answers
  if (channels < 1 || channels > 4) return DDRL_ERR_UNSUPPORTED;  // the range cfg_check accepts for in_channels
  if (n < 1 || n > INT32_MAX / WAVES_PER_ENV) return DDRL_ERR_INVALID_ARG;
  if (!newest || !next || !ddrl::aligned16(newest) || !ddrl::aligned16(next)) return DDRL_ERR_INVALID_ARG;
  const uint64_t stack_bytes = (uint64_t)n * channels * PLANE_BYTES;
  if (ddrl::overlap(newest, next, (uint64_t)n * PLANE_BYTES, stack_bytes)) return DDRL_ERR_INVALID_ARG;
  if (channels > 1) {  // C = 1: next = newest, prev is not read
    if (!prev || !ddrl::aligned16(prev) || ddrl::overlap(prev, next, stack_bytes, stack_bytes)) return DDRL_ERR_INVALID_ARG;
  }
  const dim3 grid((unsigned)n * WAVES_PER_ENV), block(64);
  const hipStream_t st = (hipStream_t)stream;
  const uint4 *p = (const uint4*)prev, *f = (const uint4*)newest;
  uint4* o = (uint4*)next;
  switch (channels) {
    case 1: hipLaunchKernelGGL(frame_stack_push_kernel<1>, grid, block, 0, st, p, f, reset, o); break;
    case 2: hipLaunchKernelGGL(frame_stack_push_kernel<2>, grid, block, 0, st, p, f, reset, o); break;
    case 3: hipLaunchKernelGGL(frame_stack_push_kernel<3>, grid, block, 0, st, p, f, reset, o); break;
    default: hipLaunchKernelGGL(frame_stack_push_kernel<4>, grid, block, 0, st, p, f, reset, o); break;
  }
  return ddrl::launch_status();
}
