// What the navigation env (navenv.hip) and the multi-robot one (fleetenv.hip, section 6.11) share: the sizes of
// the rule books (tests/nav_env_ref.py), the Q14 trig table, the counter-based hash, the exact integer square root, the ranges of a loaded
// state word, the action decoding, the info word's layout and the cast of four beams on a circle.  Integer arithmetic only.
#pragma once
#include "rows.h"

namespace ddrl {

constexpr int NAV_STATE_INTS = 64, NAV_THREADS = 256;
constexpr int NAV_HEADINGS = 3840, NAV_BEAMS = 960, NAV_BEAM_STEP = 4, NAV_Q = 14;
constexpr int NAV_MAX_OBS = 10, NAV_MAX_PEDS = 5;
constexpr int NAV_ARENA_R = 2560, NAV_ROBOT_R = 64, NAV_PED_R = 77, NAV_OBS_R_MIN = 77, NAV_OBS_R_MAX = 128;
constexpr int NAV_RANGE_MAX = 1536, NAV_GOAL_TOL = 77, NAV_CELL = 608;
constexpr int NAV_V_MAX = 32, NAV_W_MAX = 64, NAV_SPEED_MIN = 8, NAV_SPEED_MAX = 24, NAV_DPREV_MAX = 8191;
constexpr int NAV_BONUS = 15 * 256;
constexpr int NAV_MAP = 48, NAV_MAP_CELL = 64, NAV_MAP_FLOATS = 3 * NAV_MAP * NAV_MAP, NAV_MAP_CHUNKS = NAV_MAP_FLOATS / 4;
constexpr int NAV_VECTOR = 5;
enum { NS_X = 0, NS_Y, NS_H, NS_V, NS_W, NS_GX, NS_GY, NS_DPREV, NS_STEPS, NS_EVENTS, NS_OBS0 = 10, NS_PED0 = 40, NS_USED = 60 };
static_assert(NAV_BEAMS == 4 * 240 && NAV_BEAMS * NAV_BEAM_STEP == NAV_HEADINGS, "four beams a thread, one turn");
static_assert(NS_OBS0 + 3 * NAV_MAX_OBS == NS_PED0 && NS_PED0 + 4 * NAV_MAX_PEDS == NS_USED, "state layout");

// Q14 cos[3840] then sin[3840] (tools/gen_nav_trig.py): the copy the kernels of a translation unit index (one per unit that includes this)
static __device__ const int32_t nav_trig_dev[2 * NAV_HEADINGS] = {
#include "nav_trig.inc"
};

__device__ __forceinline__ int nav_cos(int h) { return nav_trig_dev[h]; }  // h in 0..3839: sanitised or reduced by the caller
__device__ __forceinline__ int nav_sin(int h) { return nav_trig_dev[NAV_HEADINGS + h]; }
__device__ __forceinline__ int nav_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int nav_heading(int v) {  // any int -> 0..3839
  const int m = v % NAV_HEADINGS;
  return m < 0 ? m + NAV_HEADINGS : m;
}

// section 6.7's counter-based hash (denv.hip env_hash, tests/device_env_ref.py hash32), word for word
__device__ __forceinline__ uint32_t nav_hash(uint32_t seed, uint32_t env, uint32_t counter) {
  uint32_t x = seed ^ (env * 0x9E3779B1u) ^ (counter * 0x85EBCA77u);
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 16;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// floor(sqrt(x)), 0 <= x < 2^62: the double estimate is within one of it, the loops settle the rest in either direction
__device__ __forceinline__ int64_t nav_isqrt(int64_t x) {
  int64_t r = (int64_t)sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// word k of a loaded 64-word state brought into its range (NavEnvRef.sanitize): a no-op on every state the rules produce
__device__ __forceinline__ int nav_sanitize_word(int k, int v, int n_obs, int n_peds) {
  if (k == NS_X || k == NS_Y || k == NS_GX || k == NS_GY) return nav_clamp(v, -NAV_ARENA_R, NAV_ARENA_R);
  if (k == NS_H) return nav_heading(v);
  if (k == NS_V) return nav_clamp(v, 0, NAV_V_MAX);
  if (k == NS_W) return nav_clamp(v, -NAV_W_MAX, NAV_W_MAX);
  if (k == NS_DPREV) return nav_clamp(v, 0, NAV_DPREV_MAX);
  if (k == NS_STEPS || k == NS_EVENTS) return v;
  if (k < NS_PED0) {
    const int q = k - NS_OBS0, o = q / 3, f = q - 3 * o;
    if (o >= n_obs) return 0;
    return f < 2 ? nav_clamp(v, -NAV_ARENA_R, NAV_ARENA_R) : nav_clamp(v, NAV_OBS_R_MIN, NAV_OBS_R_MAX);
  }
  if (k < NS_USED) {
    const int q = k - NS_PED0, p = q >> 2, f = q & 3;
    if (p >= n_peds) return 0;
    if (f < 2) return nav_clamp(v, -NAV_ARENA_R, NAV_ARENA_R);
    return f == 2 ? nav_heading(v) : nav_clamp(v, NAV_SPEED_MIN, NAV_SPEED_MAX);
  }
  return 0;
}

__device__ __forceinline__ bool nav_finite(float a) { return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u; }

// an action as the Gaussian actor writes it -> v in 0..32 ticks, w in -64..64 heading steps (decode_actions): one fp32 multiply each
__device__ __forceinline__ void nav_decode(float a0, float a1, int* v, int* w) {
  a0 = nav_finite(a0) ? a0 : 0.0f;
  a1 = nav_finite(a1) ? a1 : 0.0f;
  a0 = a0 < 0.0f ? 0.0f : (a0 > 1.0f ? 1.0f : a0);
  a1 = a1 < -1.0f ? -1.0f : (a1 > 1.0f ? 1.0f : a1);
  *v = (int)floorf(a0 * 32.0f);
  *w = (int)truncf(a1 * 64.0f);
}

// The info word of a step (include/ddrl.h; tests/nav_status_ref.py spells it out): what the step just played did, read off the moved
// robot and pedestrians before a finished robot's new episode is drawn.
constexpr int NAV_CLOSE = 512;  // "close to a pedestrian": centres within 2 m
enum {
  NI_DONE = 1 << 0, NI_GOAL = 1 << 1, NI_KIND_SHIFT = 2, NI_TRUNC = 1 << 4, NI_CLOSE = 1 << 5, NI_WALL = 1 << 6, NI_OBSTACLE = 1 << 7,
  NI_V_SHIFT = 8, NI_W_SHIFT = 16
};

// the nearest hit of four beams on the circle at (mx, my) from the robot, radius rad (NavEnvRef.lidar; |d|^2 counts as 2^28)
__device__ __forceinline__ void nav_cast(int mx, int my, int rad, const int* dx, const int* dy, int* rng) {
  const int cc = mx * mx + my * my - rad * rad;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int t = NAV_RANGE_MAX;
    if (cc <= 0) {
      t = 0;
    } else {
      const int64_t b = (int64_t)mx * dx[q] + (int64_t)my * dy[q];
      const int64_t disc = b * b - (int64_t)cc * ((int64_t)1 << 28);
      if (b > 0 && disc >= 0) t = (int)((b - nav_isqrt(disc)) >> NAV_Q);
    }
    rng[q] = min(rng[q], t);
  }
}

// the four beams 4 t .. 4 t + 3 of a robot at (x, y) heading h: their directions and their ranges to the wall seen from inside
__device__ __forceinline__ void nav_beams(int x, int y, int h, int t, int* dx, int* dy, int* rng) {
  const int cw = x * x + y * y - NAV_ARENA_R * NAV_ARENA_R;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int hb = h + NAV_BEAM_STEP * (4 * t + q);  // below 2 * 3840
    hb = hb >= NAV_HEADINGS ? hb - NAV_HEADINGS : hb;
    dx[q] = nav_cos(hb);
    dy[q] = nav_sin(hb);
    int r = 0;
    if (cw < 0) {  // the wall from inside
      const int64_t b = -((int64_t)x * dx[q] + (int64_t)y * dy[q]);
      r = (int)((b + nav_isqrt(b * b - (int64_t)cw * ((int64_t)1 << 28))) >> NAV_Q);
    }
    rng[q] = r;
  }
}

// the four ranges in metres, one 16-byte store
__device__ __forceinline__ void nav_store_ranges(const int* rng, float4* out) {
  float4 o;
  o.x = (float)nav_clamp(rng[0], 0, NAV_RANGE_MAX) * 0.00390625f;
  o.y = (float)nav_clamp(rng[1], 0, NAV_RANGE_MAX) * 0.00390625f;
  o.z = (float)nav_clamp(rng[2], 0, NAV_RANGE_MAX) * 0.00390625f;
  o.w = (float)nav_clamp(rng[3], 0, NAV_RANGE_MAX) * 0.00390625f;
  *out = o;
}

// what the operators check of n, env0 and the populations: 1 <= n, global env indices inside 32 bits
inline bool nav_range_ok(int32_t n, int64_t env0, int32_t n_obs, int32_t n_peds) {
  return n >= 1 && env0 >= 0 && env0 + (int64_t)n <= ((int64_t)1 << 32) && n_obs >= 0 && n_obs <= NAV_MAX_OBS && n_peds >= 0 &&
         n_peds <= NAV_MAX_PEDS;
}

}  // namespace ddrl
