// Device navigation env: a differential-drive robot, up to 10 static circular obstacles and up to 5 walking pedestrians in a round
// arena, stepped and observed on the GPU (include/ddrl.h ddrl_op_nav_env_*).  tests/nav_env_ref.py is the rule
// book: integer arithmetic only (the one double-precision square root is an estimate that an integer fix-up makes the exact floor), so
// every state word, lidar range, vector entry, map cell, reward and done equals the model's.  Context-free, no allocation, no atomics;
// the same arguments give the same bits.
//
// One 256-thread workgroup per env.  Threads 0..63 load one state word each, bring it into its range and park it in LDS; after a barrier
// thread 0 plays the (workgroup-uniform) step on the LDS copy -- pedestrians, robot, collision, goal, the new episode of a finished env
// -- and stores the reward and the done; after a second barrier thread 0 stores the 256 bytes of state and every thread renders from
// the LDS copy: a thread owns 4 consecutive beams (240 threads, one 16-byte store each) and 16-byte chunks of the 3 x 48 x 48 map (1,728
// chunks).  Render is a gather: every address written is a function of the env index alone, and no table index depends on a word that
// has not been through nav_sanitize_word.
//
// ddrl_op_nav_env_step_final is a third instantiation of the step kernel: a workgroup whose step truncated its
// episode renders the state the episode ended in into final_* before thread 0 draws the next episode, so the rules are played in two
// halves -- nav_advance (rules 1 to 6) and nav_new_episode -- with that render and one barrier between them.  The other two
// instantiations play both halves back to back in thread 0.
#include <cstring>

#include "navcore.h"

namespace ddrl {

// the copy of the Q14 table ddrl_op_nav_env_trig hands out (the kernels index navcore.h's)
static const int32_t nav_trig_host[2 * NAV_HEADINGS] = {
#include "nav_trig.inc"
};

__device__ __forceinline__ uint32_t nav_draw(int* s, uint32_t seed, uint32_t genv) {
  const uint32_t h = nav_hash(seed, genv, (uint32_t)s[NS_EVENTS]);
  s[NS_EVENTS] = (int)((uint32_t)s[NS_EVENTS] + 1u);
  return h;
}

__device__ __forceinline__ int nav_distance(const int* s) {
  const int64_t dx = s[NS_GX] - s[NS_X], dy = s[NS_GY] - s[NS_Y];
  return (int)nav_isqrt(dx * dx + dy * dy);
}

// NavEnvRef._new_episode on the LDS copy: 3 + n_obs + n_peds draws, every slot in a cell of its own
__device__ void nav_new_episode(int* s, int n_obs, int n_peds, uint32_t seed, uint32_t genv) {
  uint32_t h = nav_draw(s, seed, genv);
  const uint32_t m = h % 20u;
  const int a = (int)(1u + m + m / 4u);  // the m-th of 1..24 that is no multiple of 5
  const int b = (int)((h >> 8) % 25u);
  int slot = 0;
  auto centre = [&](int* cx, int* cy) {
    const int cell = (a * slot + b) % 25;
    ++slot;
    *cx = (cell % 5 - 2) * NAV_CELL;
    *cy = (cell / 5 - 2) * NAV_CELL;
  };
  int cx, cy;
  for (int k = 0; k < n_obs; ++k) {
    h = nav_draw(s, seed, genv);
    centre(&cx, &cy);
    s[NS_OBS0 + 3 * k] = cx + (int)((h >> 8) % 257u) - 128;
    s[NS_OBS0 + 3 * k + 1] = cy + (int)((h >> 17) % 257u) - 128;
    s[NS_OBS0 + 3 * k + 2] = NAV_OBS_R_MIN + (int)(h % 52u);
  }
  h = nav_draw(s, seed, genv);
  centre(&cx, &cy);
  s[NS_X] = cx;
  s[NS_Y] = cy;
  s[NS_H] = (int)(h % (uint32_t)NAV_HEADINGS);
  h = nav_draw(s, seed, genv);
  centre(&cx, &cy);
  s[NS_GX] = cx + (int)((h >> 8) % 257u) - 128;
  s[NS_GY] = cy + (int)((h >> 17) % 257u) - 128;
  for (int j = 0; j < n_peds; ++j) {
    h = nav_draw(s, seed, genv);
    centre(&cx, &cy);
    s[NS_PED0 + 4 * j] = cx;
    s[NS_PED0 + 4 * j + 1] = cy;
    s[NS_PED0 + 4 * j + 2] = (int)(h % (uint32_t)NAV_HEADINGS);
    s[NS_PED0 + 4 * j + 3] = NAV_SPEED_MIN + (int)((h >> 12) % 17u);
  }
  s[NS_V] = s[NS_W] = s[NS_STEPS] = 0;
  s[NS_DPREV] = nav_distance(s);
}

// rules 1 to 6 of one step on the LDS copy (NavEnvRef.step): everything but the new episode of a finished env, which the caller draws
// (nav_new_episode) when *done_out is set; every product fits 32 bits.
// INFO: *info_out receives the info word; the state, the units and the done are the same either way.
template <bool INFO>
__device__ void nav_advance(int* s, float a0, float a1, int n_obs, int n_peds, int max_steps, uint32_t seed, uint32_t genv, int* units_out,
                            int* done_out, int* info_out) {
  int v, w;
  nav_decode(a0, a1, &v, &w);
  // 1. the pedestrians, in index order
  for (int j = 0; j < n_peds; ++j) {
    int* p = s + NS_PED0 + 4 * j;
    const int cx = p[0] + ((p[3] * nav_cos(p[2])) >> NAV_Q), cy = p[1] + ((p[3] * nav_sin(p[2])) >> NAV_Q);
    bool refused = cx * cx + cy * cy > (NAV_ARENA_R - NAV_PED_R) * (NAV_ARENA_R - NAV_PED_R);
    for (int k = 0; k < n_obs; ++k) {
      const int dx = cx - s[NS_OBS0 + 3 * k], dy = cy - s[NS_OBS0 + 3 * k + 1], rr = NAV_PED_R + s[NS_OBS0 + 3 * k + 2];
      refused = refused || dx * dx + dy * dy < rr * rr;
    }
    if (refused) {
      p[2] = (int)(nav_draw(s, seed, genv) % (uint32_t)NAV_HEADINGS);
    } else {
      p[0] = cx;
      p[1] = cy;
    }
  }
  // 2. the robot
  const int h = nav_heading(s[NS_H] + w);
  const int x = s[NS_X] + ((v * nav_cos(h)) >> NAV_Q), y = s[NS_Y] + ((v * nav_sin(h)) >> NAV_Q);
  s[NS_X] = x;
  s[NS_Y] = y;
  s[NS_H] = h;
  s[NS_V] = v;
  s[NS_W] = w;
  s[NS_STEPS] = (int)((uint32_t)s[NS_STEPS] + 1u);
  // 3. distance and reward units
  const int d = nav_distance(s);
  int units = 2 * (s[NS_DPREV] - d);
  s[NS_DPREV] = d;
  // 4. collision  5. goal  6. truncation
  // one flag per cause: the info word names them (INFO), the plain instantiation only needs their union
  const bool wall = x * x + y * y > (NAV_ARENA_R - NAV_ROBOT_R) * (NAV_ARENA_R - NAV_ROBOT_R);
  bool hit_o = false, hit_p = false, close = false;
  for (int k = 0; k < n_obs; ++k) {
    const int dx = x - s[NS_OBS0 + 3 * k], dy = y - s[NS_OBS0 + 3 * k + 1], rr = NAV_ROBOT_R + s[NS_OBS0 + 3 * k + 2];
    hit_o = hit_o || dx * dx + dy * dy < rr * rr;
  }
  for (int j = 0; j < n_peds; ++j) {
    const int dx = x - s[NS_PED0 + 4 * j], dy = y - s[NS_PED0 + 4 * j + 1], dd = dx * dx + dy * dy;
    hit_p = hit_p || dd < (NAV_ROBOT_R + NAV_PED_R) * (NAV_ROBOT_R + NAV_PED_R);
    if (INFO) close = close || dd <= NAV_CLOSE * NAV_CLOSE;
  }
  const bool collision = wall || hit_o || hit_p;
  bool done = collision;
  if (collision) {
    units -= NAV_BONUS;
  } else if (d <= NAV_GOAL_TOL) {
    units += NAV_BONUS;
    done = true;
  } else if (s[NS_STEPS] >= max_steps) {
    done = true;
  }
  if (INFO) {
    const int kind = (wall || hit_o) ? 1 : (hit_p ? 2 : 0);  // static wins
    const bool goal = !collision && d <= NAV_GOAL_TOL;
    *info_out = (done ? NI_DONE : 0) | (goal ? NI_GOAL : 0) | (kind << NI_KIND_SHIFT) | ((done && !collision && !goal) ? NI_TRUNC : 0) |
                (close ? NI_CLOSE : 0) | (wall ? NI_WALL : 0) | (hit_o ? NI_OBSTACLE : 0) | (v << NI_V_SHIFT) |
                ((w + NAV_W_MAX) << NI_W_SHIFT);
  }
  *units_out = units;
  *done_out = done ? 1 : 0;
}

// thread 0 stores the 256 bytes of the LDS copy `s`, behind a barrier that made it final
__device__ __forceinline__ void nav_store_state(const int* s, int32_t* __restrict__ st) {
  if (threadIdx.x == 0) {
    int4* o = reinterpret_cast<int4*>(st);
#pragma unroll
    for (int k = 0; k < NAV_STATE_INTS / 4; ++k) o[k] = make_int4(s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
  }
}

// All threads render the observation of the LDS copy `s`.  `ped` is LDS scratch [NAV_MAX_PEDS][4].  Called by every thread of the
// workgroup, behind a barrier after which nobody writes `s` or reads `ped`; holds one barrier of its own.
__device__ __forceinline__ void nav_render(const int* s, int (*ped)[4], int n_obs, int n_peds, float* __restrict__ laser,
                                           float* __restrict__ vector, float* __restrict__ image) {
  const int tid = threadIdx.x;
  const int x = s[NS_X], y = s[NS_Y], h = s[NS_H];
  const int c = nav_cos(h), sn = nav_sin(h);
  if (tid < n_peds) {  // pedestrian tid in the robot's frame: position, velocity in ticks / step
    const int* p = s + NS_PED0 + 4 * tid;
    const int qx = p[0] - x, qy = p[1] - y, rel = nav_heading(p[2] - h);
    ped[tid][0] = (qx * c + qy * sn) >> NAV_Q;
    ped[tid][1] = (-qx * sn + qy * c) >> NAV_Q;
    ped[tid][2] = (p[3] * nav_cos(rel)) >> NAV_Q;
    ped[tid][3] = (p[3] * nav_sin(rel)) >> NAV_Q;
  }
  __syncthreads();
  // laser: beams 4 tid .. 4 tid + 3
  if (tid < NAV_BEAMS / 4) {
    int dx[4], dy[4], rng[4];
    nav_beams(x, y, h, tid, dx, dy, rng);
    for (int k = 0; k < n_obs; ++k) nav_cast(s[NS_OBS0 + 3 * k] - x, s[NS_OBS0 + 3 * k + 1] - y, s[NS_OBS0 + 3 * k + 2], dx, dy, rng);
    for (int j = 0; j < n_peds; ++j) nav_cast(s[NS_PED0 + 4 * j] - x, s[NS_PED0 + 4 * j + 1] - y, NAV_PED_R, dx, dy, rng);
    nav_store_ranges(rng, reinterpret_cast<float4*>(laser) + tid);
  } else if (tid == NAV_THREADS - 1) {  // vector: goal in the robot's frame, the last action, the distance
    const int gx = s[NS_GX] - x, gy = s[NS_GY] - y;
    vector[0] = (float)((gx * c + gy * sn) >> NAV_Q) * 0.00390625f;
    vector[1] = (float)((-gx * sn + gy * c) >> NAV_Q) * 0.00390625f;
    vector[2] = (float)s[NS_V] * 0.03125f;
    vector[3] = (float)s[NS_W] * 0.015625f;
    vector[4] = (float)s[NS_DPREV] * 0.00390625f;
  }
  // pedestrian map: chunk = 4 consecutive cells of one row of one channel; the lowest pedestrian index that covers a cell wins
  for (int ck = tid; ck < NAV_MAP_CHUNKS; ck += NAV_THREADS) {
    const int ch = ck / (NAV_MAP * NAV_MAP / 4), rem = ck - ch * (NAV_MAP * NAV_MAP / 4);
    const int row = rem / (NAV_MAP / 4), col0 = (rem - row * (NAV_MAP / 4)) * 4;
    const int fwd = (NAV_MAP / 2 - row) * NAV_MAP_CELL - NAV_MAP_CELL / 2;
    float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = n_peds - 1; j >= 0; --j) {
      const int df = fwd - ped[j][0];
      const float pv = ch == 0 ? 1.0f : (float)ped[j][ch + 1] * 0.03125f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int dl = (NAV_MAP / 2 - (col0 + q)) * NAV_MAP_CELL - NAV_MAP_CELL / 2 - ped[j][1];
        if (df * df + dl * dl <= NAV_PED_R * NAV_PED_R) val[q] = pv;
      }
    }
    reinterpret_cast<float4*>(image)[ck] = make_float4(val[0], val[1], val[2], val[3]);
  }
}

// INFO: the instantiation behind ddrl_op_nav_env_step_info; `info` is not touched otherwise.  FINAL (with INFO): the one behind
// ddrl_op_nav_env_step_final -- a truncated env (uniform over its workgroup) also renders the state rule 6 left into final_*, and only
// behind a further barrier does thread 0 draw the next episode; final_* are not touched otherwise.
template <bool INFO, bool FINAL>
__global__ __launch_bounds__(NAV_THREADS) void nav_env_step_kernel(int32_t* __restrict__ state, int64_t env0, uint32_t seed, int n_obs,
                                                                   int n_peds, int max_steps, const float* __restrict__ actions,
                                                                   float* __restrict__ laser, float* __restrict__ vector,
                                                                   float* __restrict__ image, float* __restrict__ reward,
                                                                   uint8_t* __restrict__ done, int32_t* __restrict__ info,
                                                                   float* __restrict__ final_laser, float* __restrict__ final_vector,
                                                                   float* __restrict__ final_image) {
  static_assert(INFO || !FINAL, "the terminal render is chosen by the info word");
  __shared__ int s[NAV_STATE_INTS];
  __shared__ int ped[NAV_MAX_PEDS][4];
  __shared__ int truncated;  // FINAL: rule 6 ended the episode, for every thread
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t genv = (uint32_t)(env0 + i);
  int32_t* st = state + i * NAV_STATE_INTS;
  if (tid < NAV_STATE_INTS) s[tid] = nav_sanitize_word(tid, st[tid], n_obs, n_peds);
  __syncthreads();  // the old state is in LDS: nothing reads the env's global words after this, thread 0 alone writes them
  if (tid == 0) {
    int units, d, word = 0;
    nav_advance<INFO>(s, actions[2 * i], actions[2 * i + 1], n_obs, n_peds, max_steps, seed, genv, &units, &d, &word);
    const bool held = FINAL && (word & NI_TRUNC);  // the state the episode ended in is rendered before the next one is drawn
    if (d && !held) nav_new_episode(s, n_obs, n_peds, seed, genv);
    reward[i] = (float)units * 0.00390625f;
    done[i] = (uint8_t)d;
    if (INFO) info[i] = word;
    if (FINAL) truncated = held ? 1 : 0;
  }
  __syncthreads();  // the new state is final (FINAL, truncated: the state the episode ended in)
  if (FINAL && truncated) {  // uniform over the workgroup
    nav_render(s, ped, n_obs, n_peds, final_laser + i * NAV_BEAMS, final_vector + i * NAV_VECTOR, final_image + i * NAV_MAP_FLOATS);
    __syncthreads();  // every thread has read `s` and `ped` for the terminal render
    if (tid == 0) nav_new_episode(s, n_obs, n_peds, seed, genv);
    __syncthreads();  // the new state is final
  }
  nav_store_state(s, st);
  nav_render(s, ped, n_obs, n_peds, laser + i * NAV_BEAMS, vector + i * NAV_VECTOR, image + i * NAV_MAP_FLOATS);
}

__global__ __launch_bounds__(NAV_THREADS) void nav_env_reset_kernel(int32_t* __restrict__ state, int64_t env0, uint32_t seed, int n_obs,
                                                                    int n_peds, const uint8_t* __restrict__ mask,
                                                                    float* __restrict__ laser, float* __restrict__ vector,
                                                                    float* __restrict__ image) {
  __shared__ int s[NAV_STATE_INTS];
  __shared__ int ped[NAV_MAX_PEDS][4];
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x;
  if (mask != nullptr && mask[i] == 0) return;  // uniform over the workgroup; the env's state and observation stay as they are
  if (tid < NAV_STATE_INTS) s[tid] = 0;
  __syncthreads();
  if (tid == 0) nav_new_episode(s, n_obs, n_peds, seed, (uint32_t)(env0 + i));
  __syncthreads();
  nav_store_state(s, state + i * NAV_STATE_INTS);
  nav_render(s, ped, n_obs, n_peds, laser + i * NAV_BEAMS, vector + i * NAV_VECTOR, image + i * NAV_MAP_FLOATS);
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_nav_env_state_ints(void) { return NAV_STATE_INTS; }

int32_t ddrl_op_nav_env_trig(int32_t* cos_sin_host) {
  if (!cos_sin_host) return DDRL_ERR_INVALID_ARG;
  memcpy(cos_sin_host, nav_trig_host, sizeof(nav_trig_host));
  return DDRL_OK;
}

int32_t ddrl_op_nav_env_reset(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                              const uint8_t* mask, float* laser, float* vector, float* image, void* stream) {
  if (!state || !laser || !vector || !image || !nav_range_ok(n, env0, n_obstacles, n_peds)) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(state) || !aligned16(laser) || !aligned16(image) || ((uintptr_t)vector & 3)) return DDRL_ERR_INVALID_ARG;
  const void* src[1] = {mask};
  const uint64_t src_b[1] = {(uint64_t)n};
  void* dst[4] = {state, laser, vector, image};
  const uint64_t dst_b[4] = {(uint64_t)n * NAV_STATE_INTS * 4, (uint64_t)n * NAV_BEAMS * 4, (uint64_t)n * NAV_VECTOR * 4,
                             (uint64_t)n * NAV_MAP_FLOATS * 4};
  if (!reads_and_writes_apart(src, src_b, 1, dst, dst_b, 4)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(nav_env_reset_kernel, dim3((unsigned)n), dim3(NAV_THREADS), 0, (hipStream_t)stream, state, env0, seed, n_obstacles,
                     n_peds, mask, laser, vector, image);
  return launch_status();
}

// the three step entries: `info` is given (and checked like the other outputs) by ddrl_op_nav_env_step_info and _final, `final_obs`
// (laser, vector, image) by ddrl_op_nav_env_step_final alone
static int32_t nav_env_step_launch(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                   int32_t max_steps, const float* actions, float* laser, float* vector, float* image, float* reward,
                                   uint8_t* done, int32_t* info, bool with_info, float* const* final_obs, void* stream) {
  if (!state || !actions || !laser || !vector || !image || !reward || !done || !nav_range_ok(n, env0, n_obstacles, n_peds))
    return DDRL_ERR_INVALID_ARG;
  if (with_info && (!info || ((uintptr_t)info & 3))) return DDRL_ERR_INVALID_ARG;
  if (max_steps < 1) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(state) || !aligned16(laser) || !aligned16(image) || ((uintptr_t)vector & 3) || ((uintptr_t)actions & 3) ||
      ((uintptr_t)reward & 3))
    return DDRL_ERR_INVALID_ARG;
  float* fl = final_obs ? final_obs[0] : nullptr;
  float* fv = final_obs ? final_obs[1] : nullptr;
  float* fi = final_obs ? final_obs[2] : nullptr;
  if (final_obs && (!fl || !fv || !fi || !aligned16(fl) || !aligned16(fi) || ((uintptr_t)fv & 3))) return DDRL_ERR_INVALID_ARG;
  const void* src[1] = {actions};
  const uint64_t src_b[1] = {(uint64_t)n * 8};
  void* dst[10] = {state, laser, vector, image, reward, done, with_info ? info : nullptr, fl, fv, fi};
  const uint64_t dst_b[10] = {(uint64_t)n * NAV_STATE_INTS * 4, (uint64_t)n * NAV_BEAMS * 4, (uint64_t)n * NAV_VECTOR * 4,
                              (uint64_t)n * NAV_MAP_FLOATS * 4, (uint64_t)n * 4, (uint64_t)n, (uint64_t)n * 4,
                              (uint64_t)n * NAV_BEAMS * 4, (uint64_t)n * NAV_VECTOR * 4, (uint64_t)n * NAV_MAP_FLOATS * 4};
  if (!reads_and_writes_apart(src, src_b, 1, dst, dst_b, 10)) return DDRL_ERR_INVALID_ARG;
  const dim3 grid((unsigned)n), block(NAV_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (final_obs)
    hipLaunchKernelGGL((nav_env_step_kernel<true, true>), grid, block, 0, st, state, env0, seed, n_obstacles, n_peds, max_steps, actions,
                       laser, vector, image, reward, done, info, fl, fv, fi);
  else if (with_info)
    hipLaunchKernelGGL((nav_env_step_kernel<true, false>), grid, block, 0, st, state, env0, seed, n_obstacles, n_peds, max_steps, actions,
                       laser, vector, image, reward, done, info, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  else
    hipLaunchKernelGGL((nav_env_step_kernel<false, false>), grid, block, 0, st, state, env0, seed, n_obstacles, n_peds, max_steps, actions,
                       laser, vector, image, reward, done, (int32_t*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  return launch_status();
}

int32_t ddrl_op_nav_env_step(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds, int32_t max_steps,
                             const float* actions, float* laser, float* vector, float* image, float* reward, uint8_t* done, void* stream) {
  return nav_env_step_launch(state, n, env0, seed, n_obstacles, n_peds, max_steps, actions, laser, vector, image, reward, done, nullptr,
                             false, nullptr, stream);
}

int32_t ddrl_op_nav_env_step_info(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                  int32_t max_steps, const float* actions, float* laser, float* vector, float* image, float* reward,
                                  uint8_t* done, int32_t* info, void* stream) {
  return nav_env_step_launch(state, n, env0, seed, n_obstacles, n_peds, max_steps, actions, laser, vector, image, reward, done, info, true,
                             nullptr, stream);
}

int32_t ddrl_op_nav_env_step_final(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                   int32_t max_steps, const float* actions, float* laser, float* vector, float* image, float* reward,
                                   uint8_t* done, int32_t* info, float* final_laser, float* final_vector, float* final_image, void* stream) {
  float* const final_obs[3] = {final_laser, final_vector, final_image};
  return nav_env_step_launch(state, n, env0, seed, n_obstacles, n_peds, max_steps, actions, laser, vector, image, reward, done, info, true,
                             final_obs, stream);
}

}  // extern "C"
