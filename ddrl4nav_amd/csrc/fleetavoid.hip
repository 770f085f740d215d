// The step kernels of the multi-robot navigation env under the pedestrian model "avoid" (DESIGN.md section 6.16), in a translation unit of
// their own: fleetcore.h says why.  ddrl_op_fleet_env_step_model (fleetenv.hip) checks the arguments and comes here for DDRL_PED_AVOID.
#include "fleetcore.h"

namespace ddrl {

void fleet_env_step_avoid(dim3 grid, dim3 block, hipStream_t st, int32_t* state, int32_t n_robots, int64_t world0, uint32_t seed,
                          int32_t n_obstacles, int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector,
                          float* image, float* reward, uint8_t* done, int32_t* info, float* const* final_obs) {
  fleet_env_step_forms<true>(grid, block, st, state, n_robots, world0, seed, n_obstacles, n_peds, max_steps, actions, laser, vector, image,
                             reward, done, info, final_obs);
}

}  // namespace ddrl
