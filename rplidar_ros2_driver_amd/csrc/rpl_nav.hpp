// rpl_nav.hpp — E26 (include/rplgpu_msg.h, rplgpu_nav_field_dev / rplgpu_nav_paths_dev): what rpl_nav.hip (the
// kernels) and rplgpu_nav_stages.hip (the doors) share.  A call of the field is launches on one stream and nothing
// on the handle: init (the field filled, the dirty words and the result words cleared), goals (D = 0, their tiles
// dirty, result words 2 and 3), `rounds` times relax (one workgroup a tile, a tile that is not dirty leaves at once),
// close (the dirty tiles left, the live plane of dirty words moved to plane 0) and stats (result words 4 and 5).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rpl {

struct NavK {  // a checked rplgpu_nav_field_t
  uint32_t width, height;
  uint32_t lethal, neutral, factor, unknown_cost;
  uint32_t cap;
  uint32_t tiles_x, tiles_y;
};

// flags: 2 * tiles * G words, plane p of grid g at (g * 2 + p) * tiles
hipError_t launch_nav_init(hipStream_t s, const NavK &k, uint32_t G, uint32_t *potential,
                           unsigned long long potential_stride, uint32_t *flags, uint32_t resume, uint32_t *result);
hipError_t launch_nav_goals(hipStream_t s, const NavK &k, uint32_t G, const uint32_t *goals,
                            unsigned long long goal_stride, const uint32_t *n_goals, uint32_t *potential,
                            unsigned long long potential_stride, uint32_t *flags, uint32_t resume, uint32_t *result);
// round: 0 .. rounds - 1; reads plane round & 1, marks plane (round + 1) & 1
hipError_t launch_nav_relax(hipStream_t s, const NavK &k, uint32_t G, const int8_t *grid,
                            unsigned long long grid_stride, uint32_t *potential, unsigned long long potential_stride,
                            uint32_t *flags, uint32_t round, uint32_t *result);
hipError_t launch_nav_close(hipStream_t s, const NavK &k, uint32_t G, const uint32_t *potential,
                            unsigned long long potential_stride, uint32_t *flags, uint32_t rounds, uint32_t *result);
hipError_t launch_nav_paths(hipStream_t s, const NavK &k, uint32_t G, const int8_t *grid,
                            unsigned long long grid_stride, const uint32_t *potential,
                            unsigned long long potential_stride, const uint32_t *starts, uint32_t S, uint32_t *paths,
                            uint32_t max_len, uint32_t *info);

}  // namespace rpl
