// rpl_frontier.hpp — E29 (include/rplgpu_msg.h, rplgpu_frontiers_dev): what rpl_frontier.hip (the kernels),
// rplgpu_frontier_stages.hip (the doors) and rplgpu_frontier_rules.cpp (the rules, plain C++: this header names
// nothing of HIP unless a HIP unit includes it) share.  A call is seven launches on one stream and nothing on the
// handle: init (the header and the table rows), tile (a workgroup per 64 x 64 tile: the frontier mask and the
// tile's own components in LDS, the parent plane written), seam (the pairs across tile borders through global
// atomics), flatten (every cell to its root, the roots counted per 1024 cells), rank (the counts scanned, N against
// comp_cap), sums (a tile's cells folded per root in LDS, then one set of atomics per (tile, root)) and close (a
// workgroup per grid: min_size, the rows, BEST, the result words and the goal).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif
#include <cstdint>

#include "rplgpu_msg.h"
#include "rpl_rules.hpp"

namespace rpl {

constexpr uint32_t kFrHdrWords = 16u;
constexpr uint32_t kFrRankBlock = 1024u;  // cells per count of roots

// THE SCRATCH of a grid (uint32 words; every part a multiple of four words, so the table rows are 16-byte aligned):
//   hdr 16 | rbase up4(ceil(cells / 1024)) | parent up4(cells) | ord up4(cells) | table 8 comp_cap
// hdr: 0 F, 1 N, 2 flags (bits 2 and 3), 3 N is above comp_cap.  A table row: n, label, sum cx (64 bits), sum cy,
// the key.
struct FrLayout {
  uint32_t tiles_x, tiles_y, blocks;
  uint64_t cells, rbase, parent, ord, table, total;
};

// false: the shape is refused; *capacity says whether only G x tiles refuses it
inline bool frontier_layout(uint32_t width, uint32_t height, uint32_t G, uint32_t comp_cap, FrLayout *l,
                            bool *capacity = nullptr) {
  if (capacity) *capacity = false;
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM || G == 0 ||
      G > 65535u || comp_cap == 0 || comp_cap > RPLGPU_FRONTIER_MAX_COMPS)
    return false;
  if (!nav_tiles(width, height, G, &l->tiles_x, &l->tiles_y)) {
    if (capacity) *capacity = true;
    return false;
  }
  l->cells = (uint64_t)width * height;
  l->blocks = (uint32_t)((l->cells + kFrRankBlock - 1u) / kFrRankBlock);
  const uint64_t up_cells = (l->cells + 3ull) & ~3ull;
  l->rbase = kFrHdrWords;
  l->parent = l->rbase + (((uint64_t)l->blocks + 3ull) & ~3ull);
  l->ord = l->parent + up_cells;
  l->table = l->ord + up_cells;
  l->total = l->table + 8ull * comp_cap;
  return true;
}

#ifdef __HIP__
struct FrontierK {  // a checked rplgpu_frontiers_t
  uint32_t width, height, lethal, min_size, dist_weight, size_weight;
};

hipError_t launch_frontiers(hipStream_t s, const FrontierK &k, const int8_t *grid, unsigned long long grid_stride,
                            const uint32_t *potential, unsigned long long potential_stride, uint32_t G,
                            uint32_t comp_cap, uint32_t *labels, unsigned long long label_stride, uint32_t *rows,
                            unsigned long long row_stride, uint32_t row_cap, uint32_t *goal,
                            unsigned long long goal_stride, uint32_t *n_goal, uint32_t *result, uint32_t *scratch);
#endif

}  // namespace rpl
