// The device side of a step of the multi-robot navigation env (fleetenv.hip has the description, the reset and the entry points; DESIGN.md
// sections 6.11 to 6.13 and 6.16): the 96-word layout, a step's rules, the respawn, the render and the step kernel, and the launches of
// one pedestrian model.  A header, because the step kernel is instantiated in two translation units: fleetenv.hip holds the "walk"
// instantiations and fleetavoid.hip the "avoid" ones.  With all four in one unit the compiler generated other code for the "walk"
// terminal-render kernel than it does for that kernel alone (three instructions more, 0.3 to 0.4 us per launch; section 6.16), and the
// "walk" kernels are to stay what they were.
#pragma once
#include "navcore.h"

namespace ddrl {

constexpr int FL_STATE_INTS = 96, FL_MAX_ROBOTS = 4, FL_ROBOT_INTS = 10, FL_ROBOT_USED = 9;
constexpr int FL_OBS0 = 40, FL_PED0 = 70, FL_EVENTS = 90;
constexpr int FL_CLEAR = 300;
constexpr int FL_DISCS = NAV_MAX_PEDS + FL_MAX_ROBOTS - 1;  // what one robot's map can hold: the pedestrians, then the other robots
constexpr int FL_MAX_THREADS = NAV_THREADS * FL_MAX_ROBOTS;
static_assert(FL_MAX_ROBOTS * FL_ROBOT_INTS == FL_OBS0 && FL_OBS0 + 3 * NAV_MAX_OBS == FL_PED0 && FL_PED0 + 4 * NAV_MAX_PEDS == FL_EVENTS &&
                  FL_EVENTS < FL_STATE_INTS && FL_STATE_INTS % 4 == 0,
              "state layout");
static_assert(NAV_CELLS <= 64 && FL_DISCS <= NAV_THREADS && 2 * FL_CLEAR < NAV_CELL, "one cell a lane; one circle blocks one cell at most");

// word k of a loaded state brought into its range (FleetEnvRef.sanitize): a no-op on every state the rules produce
__device__ __forceinline__ int fleet_sanitize_word(int k, int v, int R, int n_obs, int n_peds) {
  if (k < FL_OBS0) {
    const int r = k / FL_ROBOT_INTS, f = k - FL_ROBOT_INTS * r;  // f < 9: X .. STEPS, the words of section 6.8's robot
    return (r < R && f < FL_ROBOT_USED) ? nav_sanitize_word(f, v, 0, 0) : 0;
  }
  if (k < FL_PED0) return nav_sanitize_word(k - FL_OBS0 + NS_OBS0, v, n_obs, n_peds);
  if (k < FL_EVENTS) return nav_sanitize_word(k - FL_PED0 + NS_PED0, v, n_obs, n_peds);
  return k == FL_EVENTS ? v : 0;
}

// Steps 1 to 5 of FleetEnvRef.step on the LDS copy, by one thread: the pedestrians, every robot's move, then every robot's outcome from
// the positions after all moves (R (n_obs + n_peds + R) circle tests).  `act`, `reward`, `done`, `info` are the world's R rows; `units`
// is LDS scratch [R].  Returns the mask of finished robots; their respawn is fleet_respawn's.  Every product fits 32 bits.
// FINAL: bits FL_MAX_ROBOTS.. of the result are the mask of truncated robots (a subset of the finished ones).
// AVOID: step 1 is not played here -- wave 0 has played it (nav_walk_peds_avoid) before this thread goes on.
template <bool FINAL, bool AVOID>
__device__ int fleet_play(int* s, int* units, int R, int n_obs, int n_peds, int max_steps, uint32_t seed, uint32_t gworld,
                          const float* __restrict__ act, float* __restrict__ reward, uint8_t* __restrict__ done, int32_t* __restrict__ info) {
  if (!AVOID) nav_walk_peds(s + FL_OBS0, s + FL_PED0, s + FL_EVENTS, n_obs, n_peds, seed, gworld);
  for (int r = 0; r < R; ++r) {
    int v, w;
    nav_decode(act[2 * r], act[2 * r + 1], &v, &w);
    units[r] = nav_move_robot(s + FL_ROBOT_INTS * r, v, w);
  }
  int fin = 0;
  for (int r = 0; r < R; ++r) {
    const int* p = s + FL_ROBOT_INTS * r;
    const int x = p[NS_X], y = p[NS_Y];
    NavHits hit;
    nav_hits(x, y, s + FL_OBS0, s + FL_PED0, n_obs, n_peds, &hit);
    bool hit_r = false;  // what the fleet adds: another robot
    for (int q = 0; q < R; ++q) {
      const int dx = x - s[FL_ROBOT_INTS * q + NS_X], dy = y - s[FL_ROBOT_INTS * q + NS_Y];
      hit_r = hit_r || (q != r && dx * dx + dy * dy < 4 * NAV_ROBOT_R * NAV_ROBOT_R);
    }
    // this env's spelling of rules 4 to 6 (navcore.h says why the decision is not shared)
    const bool collision = hit.wall || hit.obstacle || hit.ped || hit_r;
    const bool goal = !collision && p[NS_DPREV] <= NAV_GOAL_TOL;
    const bool trunc = !collision && !goal && p[NS_STEPS] >= max_steps;
    const bool fini = collision || goal || trunc;
    const int u = units[r] - (collision ? NAV_BONUS : 0) + (goal ? NAV_BONUS : 0);
    reward[r] = (float)u * 0.00390625f;
    done[r] = fini ? 1 : 0;
    if (info != nullptr)
      info[r] = nav_info_word(fini, goal, nav_hit_kind(hit, hit_r), trunc, hit.close, hit.wall, hit.obstacle, p[NS_V], p[NS_W]);
    fin |= (fini ? 1 : 0) << r;
    if (FINAL) fin |= (trunc ? 1 : 0) << (FL_MAX_ROBOTS + r);
  }
  return fin;
}

// the first lane in scan order whose cell holds; a free cell always exists in a sanitised state (the rule book asserts it), 0 otherwise
__device__ __forceinline__ int fleet_first(bool ok) {
  const unsigned long long vote = __ballot(ok);
  return vote ? __ffsll((long long)vote) - 1 : 0;
}

// Step 6 of FleetEnvRef.step, by all 64 lanes of one wave in uniform control flow: the robots of `fin` respawn in index order, two draws
// each.  Lane l < 25 tests cell (c0 + l) % 25 of a scan, so the first set bit of the ballot is the rule book's first free cell.  `s` is
// only read; the positions earlier respawns left are kept in registers (px, py: the loop over r is unrolled, so no index is run-time);
// lane 0 writes the new episodes to fresh[r] and the advanced event counter to *events.  __forceinline__: with two step
// kernels calling it the compiler would otherwise call it out of line, which costs the plain step 0.4 us at R = 2.
__device__ __forceinline__ void fleet_respawn(const int* s, int (*fresh)[FL_ROBOT_USED], int* events, int fin, int R, int n_obs, int n_peds,
                                              uint32_t seed, uint32_t gworld, int lane) {
  uint32_t counter = (uint32_t)s[FL_EVENTS];
  int px[FL_MAX_ROBOTS], py[FL_MAX_ROBOTS];
#pragma unroll
  for (int q = 0; q < FL_MAX_ROBOTS; ++q) {
    px[q] = s[FL_ROBOT_INTS * q + NS_X];
    py[q] = s[FL_ROBOT_INTS * q + NS_Y];
  }
  const bool scans = lane < NAV_CELLS;
#pragma unroll
  for (int r = 0; r < FL_MAX_ROBOTS; ++r) {
    if (r >= R || !((fin >> r) & 1)) continue;  // uniform over the wave
    // the start: the first cell that is clear of every obstacle centre, every pedestrian and every other robot
    const uint32_t h1 = nav_hash(seed, gworld, counter++);
    int c0 = (int)(h1 % (uint32_t)NAV_CELLS);
    int cell = (c0 + lane) % NAV_CELLS;
    int cx = nav_cell_x(cell), cy = nav_cell_y(cell);
    bool ok = scans;
    for (int k = 0; k < n_obs; ++k) {
      const int dx = cx - s[FL_OBS0 + 3 * k], dy = cy - s[FL_OBS0 + 3 * k + 1];
      ok = ok && dx * dx + dy * dy >= FL_CLEAR * FL_CLEAR;
    }
    for (int j = 0; j < n_peds; ++j) {
      const int dx = cx - s[FL_PED0 + 4 * j], dy = cy - s[FL_PED0 + 4 * j + 1];
      ok = ok && dx * dx + dy * dy >= FL_CLEAR * FL_CLEAR;
    }
#pragma unroll
    for (int q = 0; q < FL_MAX_ROBOTS; ++q) {
      const int dx = cx - px[q], dy = cy - py[q];
      ok = ok && (q == r || q >= R || dx * dx + dy * dy >= FL_CLEAR * FL_CLEAR);
    }
    const int start = (c0 + fleet_first(ok)) % NAV_CELLS;
    const int sx = nav_cell_x(start), sy = nav_cell_y(start);
    px[r] = sx;
    py[r] = sy;
    // the goal: the first cell other than the start's whose jittered goal is clear of every obstacle centre
    const uint32_t h2 = nav_hash(seed, gworld, counter++);
    const int jx = nav_jitter_x(h2), jy = nav_jitter_y(h2);
    c0 = (int)(h2 % (uint32_t)NAV_CELLS);
    cell = (c0 + lane) % NAV_CELLS;
    cx = nav_cell_x(cell) + jx;
    cy = nav_cell_y(cell) + jy;
    ok = scans && cell != start;
    for (int k = 0; k < n_obs; ++k) {
      const int dx = cx - s[FL_OBS0 + 3 * k], dy = cy - s[FL_OBS0 + 3 * k + 1];
      ok = ok && dx * dx + dy * dy >= FL_CLEAR * FL_CLEAR;
    }
    const int gcell = (c0 + fleet_first(ok)) % NAV_CELLS;
    const int gx = nav_cell_x(gcell) + jx, gy = nav_cell_y(gcell) + jy;
    if (lane == 0) {
      int* f = fresh[r];
      f[NS_X] = sx;
      f[NS_Y] = sy;
      f[NS_H] = (int)((h1 >> 8) % (uint32_t)NAV_HEADINGS);
      f[NS_V] = f[NS_W] = f[NS_STEPS] = 0;
      f[NS_GX] = gx;
      f[NS_GY] = gy;
      f[NS_DPREV] = nav_distance(gx, gy, sx, sy);
    }
  }
  if (lane == 0) *events = (int)counter;
}

// threads 0..23 store the world's state (16 bytes each) from the LDS copy `s`, behind a barrier that made it final
__device__ __forceinline__ void fleet_store_state(const int* s, int32_t* __restrict__ st) {
  const int tid = threadIdx.x;
  if (tid < FL_STATE_INTS / 4) reinterpret_cast<int4*>(st)[tid] = make_int4(s[4 * tid], s[4 * tid + 1], s[4 * tid + 2], s[4 * tid + 3]);
}

// The 256 threads of robot r render row r of the world's observation from the LDS copy `s`: navcore.h's row render, the other R - 1
// robots in sight.  `disc` is LDS scratch [R][FL_DISCS][4], a robot's map discs each.  Called by every thread of the workgroup, behind a
// barrier after which nobody writes `s` or reads `disc`; holds one barrier of its own.
// MASKED: only the robots of the mask `rows` render (uniform over a robot's four waves; every thread still meets the barrier), the
// rows of the others are not written.
template <bool MASKED>
__device__ __forceinline__ void fleet_render(const int* s, int (*disc)[FL_DISCS][4], int R, int n_obs, int n_peds, int rows,
                                             float* __restrict__ laser, float* __restrict__ vector, float* __restrict__ image) {
  const int tid = threadIdx.x, r = tid / NAV_THREADS, t = tid - r * NAV_THREADS;
  nav_render_row<true>(s + FL_ROBOT_INTS * r, s + FL_OBS0, s + FL_PED0, s, FL_ROBOT_INTS, R, r, disc[r], n_obs, n_peds, t,
                       !MASKED || ((rows >> r) & 1), laser + (int64_t)r * NAV_BEAMS, vector + (int64_t)r * NAV_VECTOR,
                       image + (int64_t)r * NAV_MAP_FLOATS);
}

// FINAL: the instantiation behind ddrl_op_fleet_env_step_final -- between barrier 2 and the respawn the 256
// threads of every truncated robot also render its row of final_* from `s`, which then holds every robot where it is after all moves
// and before any respawn (FleetEnvRef.played); `s` stays read-only until barrier 3, and the last reader of that render's `disc` is
// through before barrier 3, long before the render behind barrier 4 writes it again.  final_* are not touched otherwise.
// AVOID: the pedestrian model "avoid"  -- behind barrier 1 wave 0 walks the pedestrians, giving way to every
// robot where it stands before its move, before thread 0, one of its lanes, plays the rest of the step on the words lane 0 wrote.
template <bool FINAL, bool AVOID>
__global__ __launch_bounds__(FL_MAX_THREADS) void fleet_env_step_kernel(int32_t* __restrict__ state, int R, int64_t world0, uint32_t seed,
                                                                        int n_obs, int n_peds, int max_steps,
                                                                        const float* __restrict__ actions, float* __restrict__ laser,
                                                                        float* __restrict__ vector, float* __restrict__ image,
                                                                        float* __restrict__ reward, uint8_t* __restrict__ done,
                                                                        int32_t* __restrict__ info, float* __restrict__ final_laser,
                                                                        float* __restrict__ final_vector, float* __restrict__ final_image) {
  __shared__ int s[FL_STATE_INTS];
  __shared__ int fresh[FL_MAX_ROBOTS][FL_ROBOT_USED];
  __shared__ int disc[FL_MAX_ROBOTS][FL_DISCS][4];
  __shared__ int units[FL_MAX_ROBOTS];
  __shared__ int ctl[2];  // the mask of finished robots (FINAL: and of the truncated ones above it), the event counter after their respawns
  const int64_t i = blockIdx.x, row0 = i * R;
  const int tid = threadIdx.x;
  const uint32_t gworld = (uint32_t)(world0 + i);
  int32_t* st = state + i * FL_STATE_INTS;
  if (tid < FL_STATE_INTS) s[tid] = fleet_sanitize_word(tid, st[tid], R, n_obs, n_peds);
  __syncthreads();  // 1: the old state is in LDS; nothing reads the world's global words after this
  if (AVOID && tid < 64)  // wave 0, uniform
    nav_walk_peds_avoid<FL_MAX_ROBOTS>(s + FL_OBS0, s + FL_PED0, s, FL_ROBOT_INTS, R, s + FL_EVENTS, n_obs, n_peds, seed, gworld, tid);
  if (tid == 0)
    ctl[0] = fleet_play<FINAL, AVOID>(s, units, R, n_obs, n_peds, max_steps, seed, gworld, actions + 2 * row0, reward + row0, done + row0,
                               info != nullptr ? info + row0 : nullptr);
  __syncthreads();  // 2: every robot has moved and knows its outcome
  const int fin = FINAL ? (ctl[0] & ((1 << FL_MAX_ROBOTS) - 1)) : ctl[0];
  if (FINAL) {
    const int trunc = ctl[0] >> FL_MAX_ROBOTS;
    if (trunc != 0)  // uniform over the workgroup
      fleet_render<true>(s, disc, R, n_obs, n_peds, trunc, final_laser + row0 * NAV_BEAMS, final_vector + row0 * NAV_VECTOR,
                         final_image + row0 * NAV_MAP_FLOATS);
  }
  if (fin != 0) {  // uniform over the workgroup
    if (tid < 64) fleet_respawn(s, fresh, &ctl[1], fin, R, n_obs, n_peds, seed, gworld, tid);
    __syncthreads();  // 3: the new episodes wait in `fresh`
    if (tid < FL_OBS0) {
      const int r = tid / FL_ROBOT_INTS, f = tid - FL_ROBOT_INTS * r;
      if (f < FL_ROBOT_USED && ((fin >> r) & 1)) s[tid] = fresh[r][f];
    } else if (tid == FL_EVENTS) {
      s[tid] = ctl[1];
    }
    __syncthreads();  // 4: the new state is final
  }
  fleet_store_state(s, st);
  fleet_render<false>(s, disc, R, n_obs, n_peds, 0, laser + row0 * NAV_BEAMS, vector + row0 * NAV_VECTOR, image + row0 * NAV_MAP_FLOATS);
}

// the launches of one pedestrian model: the step kernel behind each set of outputs
template <bool AVOID>
static void fleet_env_step_forms(dim3 grid, dim3 block, hipStream_t st, int32_t* state, int32_t n_robots, int64_t world0, uint32_t seed,
                                 int32_t n_obstacles, int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector,
                                 float* image, float* reward, uint8_t* done, int32_t* info, float* const* final_obs) {
  if (final_obs)
    hipLaunchKernelGGL((fleet_env_step_kernel<true, AVOID>), grid, block, 0, st, state, n_robots, world0, seed, n_obstacles, n_peds,
                       max_steps, actions, laser, vector, image, reward, done, info, final_obs[0], final_obs[1], final_obs[2]);
  else
    hipLaunchKernelGGL((fleet_env_step_kernel<false, AVOID>), grid, block, 0, st, state, n_robots, world0, seed, n_obstacles, n_peds,
                       max_steps, actions, laser, vector, image, reward, done, info, (float*)nullptr, (float*)nullptr, (float*)nullptr);
}

// fleet_env_step_forms<true>, from the translation unit that holds those instantiations (fleetavoid.hip)
void fleet_env_step_avoid(dim3 grid, dim3 block, hipStream_t st, int32_t* state, int32_t n_robots, int64_t world0, uint32_t seed,
                          int32_t n_obstacles, int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector,
                          float* image, float* reward, uint8_t* done, int32_t* info, float* const* final_obs);

}  // namespace ddrl
