// Multi-robot navigation env: R = 1..4 differential-drive robots share one arena with up to 10 static circular obstacles and up to 5
// walking pedestrians, see each other in their lidar and dynamic-agent map and collide with each other (include/ddrl.h
// ddrl_op_fleet_env_*).  tests/fleet_env_ref.py is the rule book, in integers only, so every state word, lidar
// range, vector entry, map cell, reward, done and info word equals the model's.  Context-free, no allocation, no atomics; the same
// arguments give the same bits.  The arena is section 6.8's: the sizes, the tables, every rule of a step, the placement of a new world and
// the render of a row come from navcore.h (section 6.13).  What is written here is what a fleet adds -- the 96-word layout, the order of a
// step (all moves, then all outcomes), the robot-robot test, the respawn of a finished robot alone -- and the kernels.
//
// A world is one arena, a row is one robot: row i * R + r is robot r of world i.  One workgroup of 256 R threads per world, and nobody
// else touches that world's state.  Threads 0..95 load one state word each, bring it into its range and park it in LDS `s`.  Behind
// barrier 1 thread 0 plays the step on `s` -- pedestrians, every robot's move, every robot's outcome from the positions after all
// moves -- and stores the rows' reward, done and info and the mask of finished robots.  Behind barrier 2 wave 0 respawns the finished
// robots in index order: `s` is only read, one lane tests one cell of a scan and a ballot finds the first free one in scan order, the
// positions earlier respawns left live in registers, and lane 0 writes the new episodes into `fresh`, not into `s`.  Behind barrier 3
// threads 0..39 and 90 move `fresh` and the event counter into `s`; behind barrier 4 threads 0..23 store the 384 bytes of state
// (16 bytes each) and the 256 threads of robot r render row i * R + r from `s`, as section 6.8's render does.  So no thread reads a word
// of LDS or of global state that another thread writes in the same phase: the global words are read before barrier 1 and written
// after barrier 4, `s` is written by thread 0 alone between barriers 1 and 2, read-only between 2 and 3, and final after 4.
// ddrl_op_fleet_env_step_final's instantiation renders the truncated robots' terminal observations in that read-only phase.
//
// The device side of a step -- layout, rules, respawn, render, the step kernel -- is in fleetcore.h; this file holds the new world, the
// reset kernel, the "walk" instantiations of the step kernel and every entry point.  Under the pedestrian model "avoid" (DESIGN.md
// section 6.16) wave 0 walks the pedestrians behind barrier 1 before thread 0 plays the rest; those instantiations are fleetavoid.hip's.
#include "fleetcore.h"

namespace ddrl {

// FleetEnvRef._new_world on the zeroed LDS copy, by one thread: 1 + n_obs + 2 R + n_peds draws -- the cells, the obstacles, every robot
// and its goal, the pedestrians -- every slot in a cell of its own
__device__ void fleet_new_world(int* s, int R, int n_obs, int n_peds, uint32_t seed, uint32_t gworld) {
  NavCells cells = nav_cells(nav_draw(s + FL_EVENTS, seed, gworld));
  nav_place_obstacles(s + FL_OBS0, n_obs, &cells, s + FL_EVENTS, seed, gworld);
  for (int r = 0; r < R; ++r) {
    nav_place_robot(s + FL_ROBOT_INTS * r, &cells, s + FL_EVENTS, seed, gworld);
    nav_begin_episode(s + FL_ROBOT_INTS * r);
  }
  nav_place_peds(s + FL_PED0, n_peds, &cells, s + FL_EVENTS, seed, gworld);
}

__global__ __launch_bounds__(FL_MAX_THREADS) void fleet_env_reset_kernel(int32_t* __restrict__ state, int R, int64_t world0, uint32_t seed,
                                                                         int n_obs, int n_peds, const uint8_t* __restrict__ mask,
                                                                         float* __restrict__ laser, float* __restrict__ vector,
                                                                         float* __restrict__ image) {
  __shared__ int s[FL_STATE_INTS];
  __shared__ int disc[FL_MAX_ROBOTS][FL_DISCS][4];
  const int64_t i = blockIdx.x, row0 = i * R;
  const int tid = threadIdx.x;
  if (mask != nullptr && mask[i] == 0) return;  // uniform over the workgroup; the world's state and observations stay as they are
  if (tid < FL_STATE_INTS) s[tid] = 0;
  __syncthreads();
  if (tid == 0) fleet_new_world(s, R, n_obs, n_peds, seed, (uint32_t)(world0 + i));
  __syncthreads();
  fleet_store_state(s, state + i * FL_STATE_INTS);
  fleet_render<false>(s, disc, R, n_obs, n_peds, 0, laser + row0 * NAV_BEAMS, vector + row0 * NAV_VECTOR, image + row0 * NAV_MAP_FLOATS);
}

// what both operators check of the sizes: the worlds as section 6.8's envs, 1..4 robots, the rows inside int32
inline bool fleet_range_ok(int32_t n_worlds, int32_t n_robots, int64_t world0, int32_t n_obs, int32_t n_peds) {
  return nav_range_ok(n_worlds, world0, n_obs, n_peds) && n_robots >= 1 && n_robots <= FL_MAX_ROBOTS &&
         (int64_t)n_worlds * n_robots <= INT32_MAX;
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_fleet_env_state_ints(void) { return FL_STATE_INTS; }

int32_t ddrl_op_fleet_env_reset(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                                int32_t n_peds, const uint8_t* mask, float* laser, float* vector, float* image, void* stream) {
  if (!fleet_range_ok(n_worlds, n_robots, world0, n_obstacles, n_peds) ||
      !nav_reset_args_ok(state, (uint64_t)n_worlds * FL_STATE_INTS * 4, (uint64_t)n_worlds * n_robots, mask, (uint64_t)n_worlds, laser,
                         vector, image))
    return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(fleet_env_reset_kernel, dim3((unsigned)n_worlds), dim3(NAV_THREADS * n_robots), 0, (hipStream_t)stream, state,
                     n_robots, world0, seed, n_obstacles, n_peds, mask, laser, vector, image);
  return launch_status();
}

// the step entries: `final_obs` (laser, vector, image) is given by ddrl_op_fleet_env_step_final, which also requires `info`, and by
// ddrl_op_fleet_env_step_model when it is handed one; that entry also chooses the pedestrian model
static int32_t fleet_env_step_launch(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                                     int32_t n_peds, int32_t max_steps, int32_t ped_model, const float* actions, float* laser,
                                     float* vector, float* image, float* reward, uint8_t* done, int32_t* info, float* const* final_obs,
                                     void* stream) {
  if (!fleet_range_ok(n_worlds, n_robots, world0, n_obstacles, n_peds) || max_steps < 1 || !nav_ped_model_ok(ped_model) ||
      !nav_step_args_ok(state, (uint64_t)n_worlds * FL_STATE_INTS * 4, (uint64_t)n_worlds * n_robots, actions, laser, vector, image, reward,
                        done, info, final_obs != nullptr, final_obs))
    return DDRL_ERR_INVALID_ARG;
  const dim3 grid((unsigned)n_worlds), block(NAV_THREADS * n_robots);
  if (ped_model == DDRL_PED_WALK)
    fleet_env_step_forms<false>(grid, block, (hipStream_t)stream, state, n_robots, world0, seed, n_obstacles, n_peds, max_steps, actions,
                                laser, vector, image, reward, done, info, final_obs);
  else
    fleet_env_step_avoid(grid, block, (hipStream_t)stream, state, n_robots, world0, seed, n_obstacles, n_peds, max_steps, actions, laser,
                         vector, image, reward, done, info, final_obs);
  return launch_status();
}

int32_t ddrl_op_fleet_env_step(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                               int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector, float* image,
                               float* reward, uint8_t* done, int32_t* info, void* stream) {
  return fleet_env_step_launch(state, n_worlds, n_robots, world0, seed, n_obstacles, n_peds, max_steps, DDRL_PED_WALK, actions, laser,
                               vector, image, reward, done, info, nullptr, stream);
}

int32_t ddrl_op_fleet_env_step_final(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                                     int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector, float* image,
                                     float* reward, uint8_t* done, int32_t* info, float* final_laser, float* final_vector,
                                     float* final_image, void* stream) {
  float* const final_obs[3] = {final_laser, final_vector, final_image};
  return fleet_env_step_launch(state, n_worlds, n_robots, world0, seed, n_obstacles, n_peds, max_steps, DDRL_PED_WALK, actions, laser,
                               vector, image, reward, done, info, final_obs, stream);
}

int32_t ddrl_op_fleet_env_step_model(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                                     int32_t n_peds, int32_t max_steps, int32_t ped_model, const float* actions, float* laser,
                                     float* vector, float* image, float* reward, uint8_t* done, int32_t* info, float* final_laser,
                                     float* final_vector, float* final_image, void* stream) {
  float* const final_obs[3] = {final_laser, final_vector, final_image};
  const int given = nav_final_given(final_obs);
  if (given < 0 || (given && !info)) return DDRL_ERR_INVALID_ARG;
  return fleet_env_step_launch(state, n_worlds, n_robots, world0, seed, n_obstacles, n_peds, max_steps, ped_model, actions, laser, vector,
                               image, reward, done, info, given ? final_obs : nullptr, stream);
}

}  // extern "C"
