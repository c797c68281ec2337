// rpl_grid.hpp — the E11 cell rule, the one place where a position becomes a grid cell: E11 (rpl_occ.hip), E13
// (rpl_match.hip), E14 (rpl_map.hip), E15 (rpl_pose.hip), E19 (rpl_seed.hip), E22 (rpl_cast.hip) and, through the
// look-ups below and rpl_front.hpp, E23 - E25 all call this.  Behind it, the two look-ups into an int8 field: field_look
// (a cell's byte: E13, E24, E25) and pose_look (the cell rule at a pose, then field_look: E15, E23).  It needs nothing
// of the scan front end (rpl_xf.hpp, rpl_front.hpp); of rpl_launch.hpp it takes OccK, whose first five fields are the
// grid pose_look reads.
#pragma once
#include <hip/hip_runtime.h>

#include "rpl_launch.hpp"  // OccK

namespace rpl {

constexpr float kGridCellLimit = 1048576.0f;

// float32, every operation rounded once (the units that include this are built with -ffp-contract=off; `/` is the
// IEEE divide): two subtractions, two divides, two floors, the two compares.  false: the position has no cell (NaN
// fails the compares too)
__device__ __forceinline__ bool grid_cell(float x, float y, float origin_x, float origin_y, float resolution, int *cx,
                                          int *cy) {
  const float fu = floorf((x - origin_x) / resolution);
  const float fv = floorf((y - origin_y) / resolution);
  if (!(fabsf(fu) < kGridCellLimit && fabsf(fv) < kGridCellLimit)) return false;
  *cx = (int)fu;
  *cy = (int)fv;
  return true;
}

// field value at the cell (cx, cy): 0 outside the grid and for an unknown (negative) byte
__device__ __forceinline__ uint32_t field_look(const int8_t *__restrict__ field, int cx, int cy, uint32_t W,
                                               uint32_t H) {
  if ((uint32_t)cx >= W || (uint32_t)cy >= H) return 0u;
  const int v = field[(uint32_t)cy * W + (uint32_t)cx];  // < W * H <= the field's stride
  return (uint32_t)max(v, 0);
}

// field value under the cell of (c*x - s*y + tx, s*x + c*y + ty): 0 without a cell (and *cell_range), else
// field_look's; of k the cell rule's part is read
__device__ __forceinline__ uint32_t pose_look(float x, float y, float c, float s, float tx, float ty, const OccK &k,
                                              const int8_t *__restrict__ field, bool *cell_range) {
  const float rx = (c * x - s * y) + tx;
  const float ry = (s * x + c * y) + ty;
  int cx, cy;
  if (!grid_cell(rx, ry, k.origin_x, k.origin_y, k.resolution, &cx, &cy)) {
    *cell_range = true;
    return 0u;
  }
  return field_look(field, cx, cy, k.width, k.height);
}

}  // namespace rpl
