// The scripted expert of the device navigation env (include/ddrl.h ddrl_op_nav_expert): for every env the action a
// short look-ahead over 51 constant-(v, w) arcs prefers, as a label for DAgger, and the played action mixed from it and the policy's.
// tests/nav_expert_ref.py is the rule book: integer arithmetic only, so labels and played actions equal the model's bit for bit.
//
// One wavefront per env, four envs per 256-thread workgroup.  Lane l loads state word l of its env, brings it into its range by index
// (navcore.h nav_sanitize_word, what the step kernel does to the words it loads) and parks it in LDS; behind the barrier lanes 0..50 roll
// one candidate arc each over the LDS copy (obstacles and pedestrians are wave-uniform reads), lanes 51..63 hold the largest key, the
// wave takes the minimum with the butterfly of ppo_math.h (every key is an integer below 2^24, so fminf on floats is exact) and lane 0
// stores the label and the played action.  No atomics, no scratch, no state write: the expert only reads the env.
#include "navcore.h"
#include "ppo_math.h"

namespace ddrl {

constexpr int NX_ENVS = NAV_THREADS / 64;  // envs per workgroup
constexpr int NX_CANDIDATES = 51, NX_TURNS = 17, NX_HORIZON = 10, NX_NO_HIT = NX_HORIZON + 1;
constexpr int NX_MARGIN_STATIC = 24, NX_MARGIN_PED = 48, NX_HIT_COST = 4096;
constexpr float NX_KEY_IDLE = 8388608.0f;  // 2^23: above every key (< 2^22), what the lanes without a candidate hold

__device__ __forceinline__ int nx_speed(int c) { return c < NX_TURNS ? 32 : (c < 2 * NX_TURNS ? 16 : 4); }
__device__ __forceinline__ int nx_turn(int c) { return -64 + 8 * (c % NX_TURNS); }

// key of candidate c on the sanitised state `s` (nav_expert_ref.expert_keys); every product fits 32 bits: |x|, |y| <= 2560 + 10 * 32, a
// predicted pedestrian within 2560 + 10 * 24
__device__ __forceinline__ int nx_key(const int* s, int c, int n_obs, int n_peds) {
  const int v = nx_speed(c), w = nx_turn(c);
  int x = s[NS_X], y = s[NS_Y], h = s[NS_H];
  const int gx = s[NS_GX], gy = s[NS_GY];
  int kc = NX_NO_HIT, best = NAV_DPREV_MAX;
  for (int k = 1; k <= NX_HORIZON; ++k) {
    h = nav_heading(h + w);
    x += (v * nav_cos(h)) >> NAV_Q;
    y += (v * nav_sin(h)) >> NAV_Q;
    constexpr int RW = NAV_ARENA_R - NAV_ROBOT_R - NX_MARGIN_STATIC;
    bool hit = x * x + y * y > RW * RW;
    for (int o = 0; o < n_obs; ++o) {
      const int dx = x - s[NS_OBS0 + 3 * o], dy = y - s[NS_OBS0 + 3 * o + 1], rr = NAV_ROBOT_R + NX_MARGIN_STATIC + s[NS_OBS0 + 3 * o + 2];
      hit = hit || dx * dx + dy * dy < rr * rr;
    }
    for (int j = 0; j < n_peds; ++j) {
      const int* p = s + NS_PED0 + 4 * j;
      const int qx = p[0] + k * ((p[3] * nav_cos(p[2])) >> NAV_Q), qy = p[1] + k * ((p[3] * nav_sin(p[2])) >> NAV_Q);
      const int dx = x - qx, dy = y - qy;
      constexpr int RP = NAV_ROBOT_R + NAV_PED_R + NX_MARGIN_PED;
      hit = hit || dx * dx + dy * dy < RP * RP;
    }
    kc = (kc == NX_NO_HIT && hit) ? k : kc;
    const int d = nav_distance(gx, gy, x, y);
    best = (kc == NX_NO_HIT) ? min(best, d) : best;
  }
  const int dx = gx - x, dy = gy - y, cs = nav_cos(h), sn = nav_sin(h);
  const int ex = (dx * cs + dy * sn) >> NAV_Q, ey = (-dx * sn + dy * cs) >> NAV_Q;
  const int dend = nav_distance(gx, gy, x, y);
  const int bear = ex <= 0 ? dend : min(abs(ey), dend);
  const int cost = (best <= NAV_GOAL_TOL ? 0 : best + (bear >> 1)) + NX_HIT_COST * (NX_NO_HIT - kc);
  return 64 * cost + c;
}

__global__ __launch_bounds__(NAV_THREADS) void nav_expert_kernel(const int32_t* __restrict__ state, int n, int64_t env0, uint32_t seed,
                                                                 int n_obs, int n_peds, const float* __restrict__ policy, uint32_t step,
                                                                 uint32_t threshold, float* __restrict__ label,
                                                                 float* __restrict__ played) {
  __shared__ int s[NX_ENVS][NAV_STATE_INTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * NX_ENVS + wave;
  const bool mine = i < n;  // uniform over the wave; the last workgroup's idle waves still meet the barrier
  s[wave][lane] = mine ? nav_sanitize_word(lane, state[i * NAV_STATE_INTS + lane], n_obs, n_peds) : 0;
  __syncthreads();
  if (!mine) return;
  float key = NX_KEY_IDLE;
  if (lane < NX_CANDIDATES) key = (float)nx_key(s[wave], lane, n_obs, n_peds);
  key = wave_butterfly(key, [](float a, float b) { return fminf(a, b); });
  if (lane != 0) return;
  const int c = (int)key & 63;
  const float l0 = (float)nx_speed(c) * 0.03125f, l1 = (float)nx_turn(c) * 0.015625f;
  if (label != nullptr) {
    label[2 * i] = l0;
    label[2 * i + 1] = l1;
  }
  if (played != nullptr) {
    const bool expert = policy == nullptr || nav_hash(seed, (uint32_t)(env0 + i), step) < threshold;
    played[2 * i] = expert ? l0 : policy[2 * i];
    played[2 * i + 1] = expert ? l1 : policy[2 * i + 1];
  }
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers
int32_t ddrl_op_nav_expert(const int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                           const float* policy, uint32_t step, uint32_t threshold, float* label, float* played, void* stream) {
  if (!nav_range_ok(n, env0, n_obstacles, n_peds) || !state || !aligned16(state)) return DDRL_ERR_INVALID_ARG;
  if (!policy && !played && !label) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)policy & 3) || ((uintptr_t)label & 3) || ((uintptr_t)played & 3)) return DDRL_ERR_INVALID_ARG;
  const uint64_t rows = (uint64_t)n;
  const void* src[2] = {state, policy};
  const uint64_t src_b[2] = {rows * NAV_STATE_INTS * 4, rows * 8};
  void* dst[2] = {label, played};
  const uint64_t dst_b[2] = {rows * 8, rows * 8};
  if (!reads_and_writes_apart(src, src_b, 2, dst, dst_b, 2)) return DDRL_ERR_INVALID_ARG;
  if (policy && overlap(state, policy, src_b[0], src_b[1])) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(nav_expert_kernel, dim3((unsigned)((n + NX_ENVS - 1) / NX_ENVS)), dim3(NAV_THREADS), 0, (hipStream_t)stream, state, n,
                     env0, seed, n_obstacles, n_peds, policy, step, threshold, label, played);
  return launch_status();
}

}  // extern "C"
