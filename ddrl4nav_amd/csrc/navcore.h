// The arena core of the navigation env (navenv.hip) and the multi-robot one (fleetenv.hip, section 6.11): the sizes
// of the rule books (tests/nav_env_ref.py, tests/fleet_env_ref.py), the Q14 trig table, the counter-based hash, the exact integer square
// root, the ranges of a loaded state word, the action decoding -- and every rule and every piece of the render the two envs share
// (section 6.13), written against pointers to an arena's parts, not against one state layout:
//   a robot block   words NS_X .. NS_STEPS of one robot (both layouts lay a robot out this way)
//   obs             3 words an obstacle: x, y, radius
//   peds            4 words a pedestrian: x, y, heading, speed
//   events          the counter of the draws
// The draw, the pedestrian walk (rule 1), the robot's move (rules 2 and 3), the outcome tests, the info word, the placement of an
// episode and the render of one row, then the argument checks of the host entry points.  The units / done decision (rules 4 to 6) is
// the one piece each env keeps for itself.  Integer
// arithmetic only; every device function is __forceinline__ (section 6.12 has the price of one that was not).
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

// ---- the rules of a step --------------------------------------------------------------------------------------------------------------
// one draw of the arena's counter-based stream: the hash of (seed, global index, events), and the counter goes up
__device__ __forceinline__ uint32_t nav_draw(int* events, uint32_t seed, uint32_t gidx) {
  const uint32_t h = nav_hash(seed, gidx, (uint32_t)*events);
  *events = (int)((uint32_t)*events + 1u);
  return h;
}

__device__ __forceinline__ int nav_distance(int gx, int gy, int x, int y) {
  const int64_t dx = gx - x, dy = gy - y;
  return (int)nav_isqrt(dx * dx + dy * dy);
}

// rule 1: the pedestrians walk in index order; one whose step would leave the arena or enter an obstacle draws a new heading instead
__device__ __forceinline__ void nav_walk_peds(const int* obs, int* peds, int* events, int n_obs, int n_peds, uint32_t seed, uint32_t gidx) {
  for (int j = 0; j < n_peds; ++j) {
    int* p = peds + 4 * j;
    const int cx = p[0] + ((p[3] * nav_cos(p[2])) >> NAV_Q), cy = p[1] + ((p[3] * nav_sin(p[2])) >> NAV_Q);
    bool refused = cx * cx + cy * cy > (NAV_ARENA_R - NAV_PED_R) * (NAV_ARENA_R - NAV_PED_R);
    for (int k = 0; k < n_obs; ++k) {
      const int dx = cx - obs[3 * k], dy = cy - obs[3 * k + 1], rr = NAV_PED_R + obs[3 * k + 2];
      refused = refused || dx * dx + dy * dy < rr * rr;
    }
    if (refused) {
      p[2] = (int)(nav_draw(events, seed, gidx) % (uint32_t)NAV_HEADINGS);
    } else {
      p[0] = cx;
      p[1] = cy;
    }
  }
}

// Rule 1 under the pedestrian model "avoid" (tests/ped_avoid_ref.py is the rule book): a pedestrian gives way to
// the other pedestrians and to the robots.  Its candidates are its step under the heading offsets 0, +D, -D, +2D, -2D, +3D, -3D, ranks
// 0..6 in preference order.  A candidate is statically refused by nav_walk_peds' test, and agent-blocked when it is within NAV_KEEP of
// another pedestrian or a robot and nearer to it than the pedestrian stands now.  Rank 0 statically refused: the pedestrian stays and
// draws a heading, as in nav_walk_peds.  Else the lowest rank that is neither refused nor blocked moves it and its turn persists; no
// such rank: it stays and draws a heading.
constexpr int NAV_KEEP = 192, NAV_AVOID_D = 320, NAV_AVOID_RANKS = 7;
static_assert(3 * NAV_AVOID_D < NAV_HEADINGS, "one wrap brings a candidate's heading into range");

// By all 64 lanes of one wave in uniform control flow, as fleet_respawn: lane r < 7 tests the candidate of rank r, lanes 7..63 vote
// "not free", and the first set bit of the ballot is the winning rank.  Every lane reads the pedestrians and the robots (MAXR blocks,
// `stride` words apart at `robots`, R of them in use; where they stand before this step's moves) from LDS once, before anything is
// written, and keeps them in registers (the loops over j, k and q are unrolled, so no register index is run-time); every lane applies
// the winner's move to its own copy, the event counter advances uniformly in a register, and lane 0 alone writes the pedestrians'
// words and the counter back when the walk is over.  Every product fits 32 bits (|coordinate| <= 2560 + 24).
template <int MAXR>
__device__ __forceinline__ void nav_walk_peds_avoid(const int* obs, int* peds, const int* robots, int stride, int R, int* events, int n_obs,
                                                    int n_peds, uint32_t seed, uint32_t gidx, int lane) {
  int px[NAV_MAX_PEDS], py[NAV_MAX_PEDS], ph[NAV_MAX_PEDS], ps[NAV_MAX_PEDS], rx[MAXR], ry[MAXR];
#pragma unroll
  for (int j = 0; j < NAV_MAX_PEDS; ++j) {
    px[j] = peds[4 * j];
    py[j] = peds[4 * j + 1];
    ph[j] = peds[4 * j + 2];
    ps[j] = peds[4 * j + 3];
  }
#pragma unroll
  for (int q = 0; q < MAXR; ++q) {
    rx[q] = robots[stride * q + NS_X];
    ry[q] = robots[stride * q + NS_Y];
  }
  uint32_t counter = (uint32_t)*events;
  const bool ranks = lane < NAV_AVOID_RANKS;
  const int turn = ranks ? ((lane + 1) >> 1) * ((lane & 1) ? NAV_AVOID_D : -NAV_AVOID_D) : 0;  // 0, +D, -D, +2D, -2D, +3D, -3D
#pragma unroll
  for (int j = 0; j < NAV_MAX_PEDS; ++j) {
    if (j >= n_peds) continue;  // uniform over the wave
    int h = ph[j] + turn;       // -960 .. 3839 + 960
    h = h < 0 ? h + NAV_HEADINGS : (h >= NAV_HEADINGS ? h - NAV_HEADINGS : h);
    const int cx = px[j] + ((ps[j] * nav_cos(h)) >> NAV_Q), cy = py[j] + ((ps[j] * nav_sin(h)) >> NAV_Q);
    bool refused = cx * cx + cy * cy > (NAV_ARENA_R - NAV_PED_R) * (NAV_ARENA_R - NAV_PED_R);
    for (int k = 0; k < n_obs; ++k) {
      const int dx = cx - obs[3 * k], dy = cy - obs[3 * k + 1], rr = NAV_PED_R + obs[3 * k + 2];
      refused = refused || dx * dx + dy * dy < rr * rr;
    }
    bool blocked = false;
#pragma unroll
    for (int k = 0; k < NAV_MAX_PEDS; ++k) {
      if (k == j || k >= n_peds) continue;  // uniform over the wave
      const int dx = cx - px[k], dy = cy - py[k], ex = px[j] - px[k], ey = py[j] - py[k], dd = dx * dx + dy * dy;
      blocked = blocked || (dd < NAV_KEEP * NAV_KEEP && dd < ex * ex + ey * ey);
    }
#pragma unroll
    for (int q = 0; q < MAXR; ++q) {
      if (q >= R) continue;  // uniform over the wave
      const int dx = cx - rx[q], dy = cy - ry[q], ex = px[j] - rx[q], ey = py[j] - ry[q], dd = dx * dx + dy * dy;
      blocked = blocked || (dd < NAV_KEEP * NAV_KEEP && dd < ex * ex + ey * ey);
    }
    const unsigned long long stat = __ballot(refused), vote = __ballot(ranks && !refused && !blocked);
    if (!(stat & 1ull) && vote != 0ull) {  // uniform over the wave: the lowest free rank moves the pedestrian, and its turn persists
      const int win = __ffsll((long long)vote) - 1;
      px[j] = __shfl(cx, win);
      py[j] = __shfl(cy, win);
      ph[j] = __shfl(h, win);
    } else {  // the way ahead is refused, or every rank is taken: the pedestrian stays and draws a heading
      ph[j] = (int)(nav_hash(seed, gidx, counter++) % (uint32_t)NAV_HEADINGS);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NAV_MAX_PEDS; ++j) {
      if (j >= n_peds) continue;
      peds[4 * j] = px[j];
      peds[4 * j + 1] = py[j];
      peds[4 * j + 2] = ph[j];
    }
    *events = (int)counter;
  }
}

// rules 2 and 3 on the robot block `rb`: the action (v, w) as nav_decode gives it turns and moves it; -> the reward units of its progress
// towards the goal
__device__ __forceinline__ int nav_move_robot(int* rb, int v, int w) {
  const int h = nav_heading(rb[NS_H] + w);
  const int x = rb[NS_X] + ((v * nav_cos(h)) >> NAV_Q), y = rb[NS_Y] + ((v * nav_sin(h)) >> NAV_Q);
  rb[NS_X] = x;
  rb[NS_Y] = y;
  rb[NS_H] = h;
  rb[NS_V] = v;
  rb[NS_W] = w;
  rb[NS_STEPS] = (int)((uint32_t)rb[NS_STEPS] + 1u);
  const int d = nav_distance(rb[NS_GX], rb[NS_GY], x, y);
  const int units = 2 * (rb[NS_DPREV] - d);
  rb[NS_DPREV] = d;
  return units;
}

// The info word of a step (include/ddrl.h; tests/nav_status_ref.py spells it out): what the step just played did, read off the moved
// robot and pedestrians before a finished robot's new episode is drawn.
constexpr int NAV_CLOSE = 512;  // "close to a pedestrian": centres within 2 m
enum {
  NI_DONE = 1 << 0, NI_GOAL = 1 << 1, NI_KIND_SHIFT = 2, NI_TRUNC = 1 << 4, NI_CLOSE = 1 << 5, NI_WALL = 1 << 6, NI_OBSTACLE = 1 << 7,
  NI_V_SHIFT = 8, NI_W_SHIFT = 16
};

// what a robot at (x, y) touches: one flag per cause (the info word names them) and `close`; every product fits 32 bits.  The flags are
// gathered in locals and handed out through `hit`: returned by value the four bools are packed and unpacked, which costs the nav kernels
// 3 to 9 instructions and changes the fleet kernels' register allocation.
struct NavHits {
  bool wall, obstacle, ped, close;
};
__device__ __forceinline__ void nav_hits(int x, int y, const int* obs, const int* peds, int n_obs, int n_peds, NavHits* hit) {
  const bool wall = x * x + y * y > (NAV_ARENA_R - NAV_ROBOT_R) * (NAV_ARENA_R - NAV_ROBOT_R);
  bool hit_o = false, hit_p = false, close = false;
  for (int k = 0; k < n_obs; ++k) {
    const int dx = x - obs[3 * k], dy = y - obs[3 * k + 1], rr = NAV_ROBOT_R + obs[3 * k + 2];
    hit_o = hit_o || dx * dx + dy * dy < rr * rr;
  }
  for (int j = 0; j < n_peds; ++j) {
    const int dx = x - peds[4 * j], dy = y - peds[4 * j + 1], dd = dx * dx + dy * dy;
    hit_p = hit_p || dd < (NAV_ROBOT_R + NAV_PED_R) * (NAV_ROBOT_R + NAV_PED_R);
    close = close || dd <= NAV_CLOSE * NAV_CLOSE;
  }
  hit->wall = wall;
  hit->obstacle = hit_o;
  hit->ped = hit_p;
  hit->close = close;
}

// the collision kind of the info word: static wins, then the pedestrian, then (the fleet's) another robot
__device__ __forceinline__ int nav_hit_kind(const NavHits& hit, bool other_robot) {
  return (hit.wall || hit.obstacle) ? 1 : (hit.ped ? 2 : (other_robot ? 3 : 0));
}

// Rules 4 to 6 -- the collision costs the bonus, else the goal earns it, else max_steps truncates -- are NOT here: nav_advance
// (navenv.hip) keeps them as an if-chain and fleet_play (fleetenv.hip) as four expressions, as before.  One shared spelling of either
// form made the kernels of the other env slower than the parent's, so this piece stays unshared.

// the one place the NI_* fields are combined
__device__ __forceinline__ int nav_info_word(bool fini, bool goal, int kind, bool trunc, bool close, bool wall, bool obstacle, int v, int w) {
  return (fini ? NI_DONE : 0) | (goal ? NI_GOAL : 0) | (kind << NI_KIND_SHIFT) | (trunc ? NI_TRUNC : 0) | (close ? NI_CLOSE : 0) |
         (wall ? NI_WALL : 0) | (obstacle ? NI_OBSTACLE : 0) | (v << NI_V_SHIFT) | ((w + NAV_W_MAX) << NI_W_SHIFT);
}

// ---- the placement of an episode ---------------------------------------------------------------------------------------------------------
// The 5 x 5 grid of cells an episode is laid out on.  Slot k of a new world stands in cell (a k + b) % 25 with a no multiple of 5, so
// every slot has a cell of its own.
constexpr int NAV_GRID = 5, NAV_CELLS = NAV_GRID * NAV_GRID;
struct NavCells {
  int a, b, slot;
};
__device__ __forceinline__ NavCells nav_cells(uint32_t h) {
  const uint32_t m = h % 20u;
  return {(int)(1u + m + m / 4u), (int)((h >> 8) % 25u), 0};  // a: the m-th of 1..24 that is no multiple of 5
}
__device__ __forceinline__ int nav_next_cell(NavCells* c) { return (c->a * c->slot++ + c->b) % NAV_CELLS; }

__device__ __forceinline__ int nav_cell_x(int cell) { return (cell % NAV_GRID - 2) * NAV_CELL; }
__device__ __forceinline__ int nav_cell_y(int cell) { return (cell / NAV_GRID - 2) * NAV_CELL; }
__device__ __forceinline__ int nav_jitter_x(uint32_t h) { return (int)((h >> 8) % 257u) - 128; }
__device__ __forceinline__ int nav_jitter_y(uint32_t h) { return (int)((h >> 17) % 257u) - 128; }

// n_obs obstacles, a draw and a cell each: jittered off the cell's centre, radius 77..128
__device__ __forceinline__ void nav_place_obstacles(int* obs, int n_obs, NavCells* cells, int* events, uint32_t seed, uint32_t gidx) {
  for (int k = 0; k < n_obs; ++k) {
    const uint32_t h = nav_draw(events, seed, gidx);
    const int cell = nav_next_cell(cells);
    obs[3 * k] = nav_cell_x(cell) + nav_jitter_x(h);
    obs[3 * k + 1] = nav_cell_y(cell) + nav_jitter_y(h);
    obs[3 * k + 2] = NAV_OBS_R_MIN + (int)(h % 52u);
  }
}

// the first episode of the robot block `rb` in a new world, two draws and two cells: the start and the heading, then the jittered goal
__device__ __forceinline__ void nav_place_robot(int* rb, NavCells* cells, int* events, uint32_t seed, uint32_t gidx) {
  uint32_t h = nav_draw(events, seed, gidx);
  int cell = nav_next_cell(cells);
  rb[NS_X] = nav_cell_x(cell);
  rb[NS_Y] = nav_cell_y(cell);
  rb[NS_H] = (int)(h % (uint32_t)NAV_HEADINGS);
  h = nav_draw(events, seed, gidx);
  cell = nav_next_cell(cells);
  rb[NS_GX] = nav_cell_x(cell) + nav_jitter_x(h);
  rb[NS_GY] = nav_cell_y(cell) + nav_jitter_y(h);
}

// a placed robot stands still at step 0, its distance to the goal taken
__device__ __forceinline__ void nav_begin_episode(int* rb) {
  rb[NS_V] = rb[NS_W] = rb[NS_STEPS] = 0;
  rb[NS_DPREV] = nav_distance(rb[NS_GX], rb[NS_GY], rb[NS_X], rb[NS_Y]);
}

// n_peds pedestrians, a draw and a cell each: on the cell's centre, any heading, 8..24 ticks a step
__device__ __forceinline__ void nav_place_peds(int* peds, int n_peds, NavCells* cells, int* events, uint32_t seed, uint32_t gidx) {
  for (int j = 0; j < n_peds; ++j) {
    const uint32_t h = nav_draw(events, seed, gidx);
    const int cell = nav_next_cell(cells);
    peds[4 * j] = nav_cell_x(cell);
    peds[4 * j + 1] = nav_cell_y(cell);
    peds[4 * j + 2] = (int)(h % (uint32_t)NAV_HEADINGS);
    peds[4 * j + 3] = NAV_SPEED_MIN + (int)((h >> 12) % 17u);
  }
}

// ---- the render --------------------------------------------------------------------------------------------------------------------------

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

// One row of the observation -- laser, vector, map -- as the robot block `me` sees the arena, by the 256 threads t = 0..255 of that row.
// OTHERS: `me` is block r of the R blocks `robots`, `stride` words apart; the others are cast in the lidar and drawn into the map behind
// the pedestrians, by index.  Without it there is no other robot and robots, stride, R and r are not looked at.  `disc` is LDS scratch
// [n_peds + R - 1][4]: what the map holds, in the robot's frame, in the order that wins.  Called by every thread of the workgroup, behind
// a barrier after which nobody writes the arena or reads `disc`; holds one barrier of its own, which a thread whose row is not `mine`
// (uniform over the row's four waves) meets too before it leaves with nothing written.
template <bool OTHERS>
__device__ __forceinline__ void nav_render_row(const int* me, const int* obs, const int* peds, const int* robots, int stride, int R, int r,
                                               int (*disc)[4], int n_obs, int n_peds, int t, bool mine, float* __restrict__ laser,
                                               float* __restrict__ vector, float* __restrict__ image) {
  const int x = me[NS_X], y = me[NS_Y], h = me[NS_H];
  const int c = nav_cos(h), sn = nav_sin(h);
  const int n_discs = OTHERS ? n_peds + R - 1 : n_peds;
  if (mine && t < n_discs) {  // disc t in the robot's frame: position, velocity in ticks / step
    int ax, ay, ah, av;
    if (!OTHERS || t < n_peds) {
      const int* p = peds + 4 * t;
      ax = p[0], ay = p[1], ah = p[2], av = p[3];
    } else {
      const int o = t - n_peds, q = o < r ? o : o + 1;  // the o-th robot other than r
      const int* p = robots + stride * q;
      ax = p[NS_X], ay = p[NS_Y], ah = p[NS_H], av = p[NS_V];
    }
    const int qx = ax - x, qy = ay - y, rel = nav_heading(ah - h);
    disc[t][0] = (qx * c + qy * sn) >> NAV_Q;
    disc[t][1] = (-qx * sn + qy * c) >> NAV_Q;
    disc[t][2] = (av * nav_cos(rel)) >> NAV_Q;
    disc[t][3] = (av * nav_sin(rel)) >> NAV_Q;
  }
  __syncthreads();
  if (!mine) return;
  // laser: beams 4 t .. 4 t + 3 over the wall, the obstacles, the pedestrians and the other robots
  if (t < NAV_BEAMS / 4) {
    int dx[4], dy[4], rng[4];
    nav_beams(x, y, h, t, dx, dy, rng);
    for (int k = 0; k < n_obs; ++k) nav_cast(obs[3 * k] - x, obs[3 * k + 1] - y, obs[3 * k + 2], dx, dy, rng);
    for (int j = 0; j < n_peds; ++j) nav_cast(peds[4 * j] - x, peds[4 * j + 1] - y, NAV_PED_R, dx, dy, rng);
    if (OTHERS)
      for (int q = 0; q < R; ++q)
        if (q != r) nav_cast(robots[stride * q + NS_X] - x, robots[stride * q + NS_Y] - y, NAV_ROBOT_R, dx, dy, rng);
    nav_store_ranges(rng, reinterpret_cast<float4*>(laser) + t);
  } else if (t == NAV_THREADS - 1) {  // vector: goal in the robot's frame, the last action, the distance
    const int gx = me[NS_GX] - x, gy = me[NS_GY] - y;
    vector[0] = (float)((gx * c + gy * sn) >> NAV_Q) * 0.00390625f;
    vector[1] = (float)((-gx * sn + gy * c) >> NAV_Q) * 0.00390625f;
    vector[2] = (float)me[NS_V] * 0.03125f;
    vector[3] = (float)me[NS_W] * 0.015625f;
    vector[4] = (float)me[NS_DPREV] * 0.00390625f;
  }
  // map: chunk = 4 consecutive cells of one row of one channel; the lowest disc index that covers a cell wins
  for (int ck = t; ck < NAV_MAP_CHUNKS; ck += NAV_THREADS) {
    const int ch = ck / (NAV_MAP * NAV_MAP / 4), rem = ck - ch * (NAV_MAP * NAV_MAP / 4);
    const int row = rem / (NAV_MAP / 4), col0 = (rem - row * (NAV_MAP / 4)) * 4;
    const int fwd = (NAV_MAP / 2 - row) * NAV_MAP_CELL - NAV_MAP_CELL / 2;
    float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = n_discs - 1; j >= 0; --j) {
      const int df = fwd - disc[j][0], rr = (OTHERS && j >= n_peds) ? NAV_ROBOT_R * NAV_ROBOT_R : NAV_PED_R * NAV_PED_R;
      const float pv = ch == 0 ? 1.0f : (float)disc[j][ch + 1] * 0.03125f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int dl = (NAV_MAP / 2 - (col0 + q)) * NAV_MAP_CELL - NAV_MAP_CELL / 2 - disc[j][1];
        if (df * df + dl * dl <= rr) val[q] = pv;
      }
    }
    reinterpret_cast<float4*>(image)[ck] = make_float4(val[0], val[1], val[2], val[3]);
  }
}

// ---- the host's argument checks: all of them ahead of the first HIP call ------------------------------------------------------------------
// what the operators check of n, env0 and the populations: 1 <= n, global env indices inside 32 bits
inline bool nav_range_ok(int32_t n, int64_t env0, int32_t n_obs, int32_t n_peds) {
  return n >= 1 && env0 >= 0 && env0 + (int64_t)n <= ((int64_t)1 << 32) && n_obs >= 0 && n_obs <= NAV_MAX_OBS && n_peds >= 0 &&
         n_peds <= NAV_MAX_PEDS;
}

// the pedestrian model of a ddrl_op_*_env_step_model call: DDRL_PED_WALK or DDRL_PED_AVOID
inline bool nav_ped_model_ok(int32_t ped_model) { return ped_model == DDRL_PED_WALK || ped_model == DDRL_PED_AVOID; }

// the optional terminal triple of a ddrl_op_*_env_step_model call: 1 all three given, 0 all three null, -1 given in part
inline int nav_final_given(float* const* final_obs) {
  const int given = (final_obs[0] != nullptr) + (final_obs[1] != nullptr) + (final_obs[2] != nullptr);
  return given == 3 ? 1 : (given == 0 ? 0 : -1);
}

// what a call writes, for reads_and_writes_apart: the state, an observation triple, the step's scalars, the terminal triple
struct NavWrites {
  void* ptr[10];
  uint64_t bytes[10];
  int n;
};
inline void nav_writes(NavWrites* w, void* p, uint64_t bytes) {
  w->ptr[w->n] = p;
  w->bytes[w->n++] = bytes;
}

// an observation triple of `rows` rows: all three given, laser and image 16-byte aligned, the vector a float's; noted in `w`
inline bool nav_obs_ok(float* laser, float* vector, float* image, uint64_t rows, NavWrites* w) {
  if (!laser || !vector || !image || !aligned16(laser) || !aligned16(image) || ((uintptr_t)vector & 3)) return false;
  nav_writes(w, laser, rows * NAV_BEAMS * 4);
  nav_writes(w, vector, rows * NAV_VECTOR * 4);
  nav_writes(w, image, rows * NAV_MAP_FLOATS * 4);
  return true;
}

// a reset's pointers: the state of state_bytes, the observation of `rows` rows, the optional mask of mask_bytes; nothing written
// overlaps anything else
inline bool nav_reset_args_ok(int32_t* state, uint64_t state_bytes, uint64_t rows, const uint8_t* mask, uint64_t mask_bytes, float* laser,
                              float* vector, float* image) {
  NavWrites w = {};
  if (!state || !aligned16(state)) return false;
  nav_writes(&w, state, state_bytes);
  if (!nav_obs_ok(laser, vector, image, rows, &w)) return false;
  const void* src[1] = {mask};
  return reads_and_writes_apart(src, &mask_bytes, 1, w.ptr, w.bytes, w.n);
}

// a step's pointers: a reset's without the mask, then actions [rows][2], reward and done [rows], `info` [rows] (may be null unless
// info_required) and `final_obs` (null, or a second observation triple)
inline bool nav_step_args_ok(int32_t* state, uint64_t state_bytes, uint64_t rows, const float* actions, float* laser, float* vector,
                             float* image, float* reward, uint8_t* done, int32_t* info, bool info_required, float* const* final_obs) {
  NavWrites w = {};
  if (!state || !aligned16(state) || !actions || !reward || !done || (info_required && !info)) return false;
  if (((uintptr_t)actions & 3) || ((uintptr_t)reward & 3) || ((uintptr_t)info & 3)) return false;
  nav_writes(&w, state, state_bytes);
  nav_writes(&w, reward, rows * 4);
  nav_writes(&w, done, rows);
  nav_writes(&w, info, rows * 4);
  if (!nav_obs_ok(laser, vector, image, rows, &w)) return false;
  if (final_obs && !nav_obs_ok(final_obs[0], final_obs[1], final_obs[2], rows, &w)) return false;
  const void* src[1] = {actions};
  const uint64_t src_b[1] = {rows * 8};
  return reads_and_writes_apart(src, src_b, 1, w.ptr, w.bytes, w.n);
}

}  // namespace ddrl
