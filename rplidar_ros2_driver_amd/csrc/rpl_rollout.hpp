// rpl_rollout.hpp — E27 (include/rplgpu_msg.h, rplgpu_rollout_dev): what rpl_rollout.hip (the kernels) and
// rplgpu_rollout_stages.hip (the doors) share.  A call is two launches on one stream and nothing on the handle:
// tiles (a workgroup per RPLGPU_ROLLOUT_TILE candidates of one group: the candidates' eight words, their end poses
// and the tile's record of eight words in the scratch) and close (a workgroup per group folds the records into the
// result words).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rpl {

struct RolloutK {  // a checked rplgpu_rollout_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  uint32_t lethal, unknown_value;
  uint32_t steps, min_steps;
  uint32_t a_end, a_min, a_sum, a_max;
};

// scratch: 8 * ceil(K / RPLGPU_ROLLOUT_TILE) * G words, the record of tile t of group g at 8 (g * tiles + t):
// the lowest score (64 bit), the smallest k that has it, how many have it, the admissible, the blocked, the
// off-range candidates, 0
hipError_t launch_rollout(hipStream_t s, const RolloutK &k, const float *start, uint32_t start_per_group,
                          const float *delta, unsigned long long delta_stride, uint32_t delta_per_group,
                          uint32_t delta_per_step, const float *footprint, uint32_t F, const int8_t *grid,
                          unsigned long long grid_stride, const uint32_t *potential,
                          unsigned long long potential_stride, uint32_t grid_per_group, uint32_t G, uint32_t K,
                          uint32_t *out, unsigned long long out_stride, float *end_poses,
                          unsigned long long end_stride, uint32_t *result, uint32_t *scratch);

}  // namespace rpl
