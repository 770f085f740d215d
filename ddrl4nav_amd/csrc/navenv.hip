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
// has not been through nav_sanitize_word.  The rules, the placement of an episode and the row render are navcore.h's (DESIGN.md section
// 6.13), shared with fleetenv.hip; this file orders them on the 64-word layout and holds the kernels.
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

// NavEnvRef._new_episode on the LDS copy: 3 + n_obs + n_peds draws -- the cells, the obstacles, the robot and its goal, the pedestrians
// -- every slot in a cell of its own
__device__ void nav_new_episode(int* s, int n_obs, int n_peds, uint32_t seed, uint32_t genv) {
  NavCells cells = nav_cells(nav_draw(s + NS_EVENTS, seed, genv));
  nav_place_obstacles(s + NS_OBS0, n_obs, &cells, s + NS_EVENTS, seed, genv);
  nav_place_robot(s, &cells, s + NS_EVENTS, seed, genv);
  nav_place_peds(s + NS_PED0, n_peds, &cells, s + NS_EVENTS, seed, genv);
  nav_begin_episode(s);
}

// rules 1 to 6 of one step on the LDS copy (NavEnvRef.step): everything but the new episode of a finished env, which the caller draws
// (nav_new_episode) when *done_out is set.
// INFO: *info_out receives the info word; the state, the units and the done are the same either way.
// AVOID: rule 1 is not played here -- wave 0 has played it (nav_walk_peds_avoid) before this thread goes on with rules 2 to 6.
template <bool INFO, bool AVOID>
__device__ void nav_advance(int* s, float a0, float a1, int n_obs, int n_peds, int max_steps, uint32_t seed, uint32_t genv, int* units_out,
                            int* done_out, int* info_out) {
  int v, w;
  nav_decode(a0, a1, &v, &w);
  if (!AVOID) nav_walk_peds(s + NS_OBS0, s + NS_PED0, s + NS_EVENTS, n_obs, n_peds, seed, genv);
  int units = nav_move_robot(s, v, w);
  NavHits hit;
  nav_hits(s[NS_X], s[NS_Y], s + NS_OBS0, s + NS_PED0, n_obs, n_peds, &hit);
  // 4. collision  5. goal  6. truncation: this env's spelling of the decision (navcore.h says why it is not shared)
  const bool collision = hit.wall || hit.obstacle || hit.ped;
  bool done = collision;
  if (collision) {
    units -= NAV_BONUS;
  } else if (s[NS_DPREV] <= NAV_GOAL_TOL) {
    units += NAV_BONUS;
    done = true;
  } else if (s[NS_STEPS] >= max_steps) {
    done = true;
  }
  if (INFO) {
    const bool goal = !collision && s[NS_DPREV] <= NAV_GOAL_TOL;
    *info_out = nav_info_word(done, goal, nav_hit_kind(hit, false), done && !collision && !goal, hit.close, hit.wall, hit.obstacle, v, w);
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

// All threads render the observation of the LDS copy `s`: navcore.h's row render with no other robot.  `ped` is LDS scratch
// [NAV_MAX_PEDS][4].  Called by every thread of the workgroup, behind a barrier after which nobody writes `s` or reads `ped`; holds one
// barrier of its own.
__device__ __forceinline__ void nav_render(const int* s, int (*ped)[4], int n_obs, int n_peds, float* __restrict__ laser,
                                           float* __restrict__ vector, float* __restrict__ image) {
  nav_render_row<false>(s, s + NS_OBS0, s + NS_PED0, nullptr, 0, 1, 0, ped, n_obs, n_peds, threadIdx.x, true, laser, vector, image);
}

// INFO: the instantiation behind ddrl_op_nav_env_step_info; `info` is not touched otherwise.  FINAL (with INFO): the one behind
// ddrl_op_nav_env_step_final -- a truncated env (uniform over its workgroup) also renders the state rule 6 left into final_*, and only
// behind a further barrier does thread 0 draw the next episode; final_* are not touched otherwise.  AVOID: the pedestrian model "avoid"
//  -- wave 0 walks the pedestrians before thread 0, one of its lanes, plays the rest of the step: lane 0 wrote the
// words it then reads, and nobody else reads them before the barrier.
template <bool INFO, bool FINAL, bool AVOID>
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
  if (AVOID && tid < 64)  // wave 0, uniform
    nav_walk_peds_avoid<1>(s + NS_OBS0, s + NS_PED0, s, 0, 1, s + NS_EVENTS, n_obs, n_peds, seed, genv, tid);
  if (tid == 0) {
    int units, d, word = 0;
    nav_advance<INFO, AVOID>(s, actions[2 * i], actions[2 * i + 1], n_obs, n_peds, max_steps, seed, genv, &units, &d, &word);
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

// the launches of one pedestrian model: the step kernel behind each set of outputs
template <bool AVOID>
static void nav_env_step_forms(dim3 grid, dim3 block, hipStream_t st, int32_t* state, int64_t env0, uint32_t seed, int32_t n_obstacles,
                               int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector, float* image,
                               float* reward, uint8_t* done, int32_t* info, bool with_info, float* const* final_obs) {
  if (final_obs)
    hipLaunchKernelGGL((nav_env_step_kernel<true, true, AVOID>), grid, block, 0, st, state, env0, seed, n_obstacles, n_peds, max_steps,
                       actions, laser, vector, image, reward, done, info, final_obs[0], final_obs[1], final_obs[2]);
  else if (with_info)
    hipLaunchKernelGGL((nav_env_step_kernel<true, false, AVOID>), grid, block, 0, st, state, env0, seed, n_obstacles, n_peds, max_steps,
                       actions, laser, vector, image, reward, done, info, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  else
    hipLaunchKernelGGL((nav_env_step_kernel<false, false, AVOID>), grid, block, 0, st, state, env0, seed, n_obstacles, n_peds, max_steps,
                       actions, laser, vector, image, reward, done, (int32_t*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
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
  if (!nav_range_ok(n, env0, n_obstacles, n_peds) ||
      !nav_reset_args_ok(state, (uint64_t)n * NAV_STATE_INTS * 4, (uint64_t)n, mask, (uint64_t)n, laser, vector, image))
    return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(nav_env_reset_kernel, dim3((unsigned)n), dim3(NAV_THREADS), 0, (hipStream_t)stream, state, env0, seed, n_obstacles,
                     n_peds, mask, laser, vector, image);
  return launch_status();
}

// the step entries: `info` is given (and checked like the other outputs) by ddrl_op_nav_env_step_info and _final, `final_obs` (laser,
// vector, image) by ddrl_op_nav_env_step_final alone; ddrl_op_nav_env_step_model chooses among the three forms by what it is given, and
// the pedestrian model
static int32_t nav_env_step_launch(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                   int32_t max_steps, int32_t ped_model, const float* actions, float* laser, float* vector, float* image,
                                   float* reward, uint8_t* done, int32_t* info, bool with_info, float* const* final_obs, void* stream) {
  if (!nav_range_ok(n, env0, n_obstacles, n_peds) || max_steps < 1 || !nav_ped_model_ok(ped_model) ||
      !nav_step_args_ok(state, (uint64_t)n * NAV_STATE_INTS * 4, (uint64_t)n, actions, laser, vector, image, reward, done, info,
                        with_info, final_obs))
    return DDRL_ERR_INVALID_ARG;
  const dim3 grid((unsigned)n), block(NAV_THREADS);
  if (ped_model == DDRL_PED_WALK)
    nav_env_step_forms<false>(grid, block, (hipStream_t)stream, state, env0, seed, n_obstacles, n_peds, max_steps, actions, laser, vector,
                              image, reward, done, info, with_info, final_obs);
  else
    nav_env_step_forms<true>(grid, block, (hipStream_t)stream, state, env0, seed, n_obstacles, n_peds, max_steps, actions, laser, vector,
                             image, reward, done, info, with_info, final_obs);
  return launch_status();
}

int32_t ddrl_op_nav_env_step(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds, int32_t max_steps,
                             const float* actions, float* laser, float* vector, float* image, float* reward, uint8_t* done, void* stream) {
  return nav_env_step_launch(state, n, env0, seed, n_obstacles, n_peds, max_steps, DDRL_PED_WALK, actions, laser, vector, image, reward,
                             done, nullptr, false, nullptr, stream);
}

int32_t ddrl_op_nav_env_step_info(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                  int32_t max_steps, const float* actions, float* laser, float* vector, float* image, float* reward,
                                  uint8_t* done, int32_t* info, void* stream) {
  return nav_env_step_launch(state, n, env0, seed, n_obstacles, n_peds, max_steps, DDRL_PED_WALK, actions, laser, vector, image, reward,
                             done, info, true, nullptr, stream);
}

int32_t ddrl_op_nav_env_step_final(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                   int32_t max_steps, const float* actions, float* laser, float* vector, float* image, float* reward,
                                   uint8_t* done, int32_t* info, float* final_laser, float* final_vector, float* final_image, void* stream) {
  float* const final_obs[3] = {final_laser, final_vector, final_image};
  return nav_env_step_launch(state, n, env0, seed, n_obstacles, n_peds, max_steps, DDRL_PED_WALK, actions, laser, vector, image, reward,
                             done, info, true, final_obs, stream);
}

int32_t ddrl_op_nav_env_step_model(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                   int32_t max_steps, int32_t ped_model, const float* actions, float* laser, float* vector, float* image,
                                   float* reward, uint8_t* done, int32_t* info, float* final_laser, float* final_vector,
                                   float* final_image, void* stream) {
  float* const final_obs[3] = {final_laser, final_vector, final_image};
  const int given = nav_final_given(final_obs);
  if (given < 0 || (given && !info)) return DDRL_ERR_INVALID_ARG;
  return nav_env_step_launch(state, n, env0, seed, n_obstacles, n_peds, max_steps, ped_model, actions, laser, vector, image, reward, done,
                             info, info != nullptr, given ? final_obs : nullptr, stream);
}

}  // extern "C"
