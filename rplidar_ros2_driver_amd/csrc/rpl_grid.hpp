// rpl_grid.hpp — the E11 cell rule, the one place where a position becomes a grid cell: E11 (rpl_occ.hip), E13
// (rpl_match.hip), E14 (rpl_map.hip), E15 (rpl_pose.hip), E19 (rpl_seed.hip) and E22 (rpl_cast.hip) all call this.
// It needs nothing of the scan front end (rpl_xf.hpp).
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace rpl
