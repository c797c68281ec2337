// rpl_cells.hpp — the rules of the cell exchange (include/rplgpu_comm.h, rplgpu_cell_t), written once for
// the merge kernel (rpl_cells.hip) and its host twin rplgpu_merge_cells_host (rplgpu_api.hip), the way
// rpl_comm_layout.hpp does it for the point exchange: the CPU tests drive the same code the kernel runs.
#pragma once
#include <stdint.h>

#include "rplgpu_comm.h"
#include "rpl_comm_layout.hpp"

namespace rpl {
namespace cells {

typedef unsigned long long u64;
static_assert(sizeof(rplgpu_cell_t) == 32, "rplgpu_cell_t is 32 bytes");

constexpr uint32_t kMaxWorld = 256;  // ranks rplgpu_merge_cells_dev / _host accept

// rank r's records of group g: [*start, *start + *n) of its slot.  Entries beyond the rank's groups
// are empty; an entry is cut to the slot (as meta_scan cuts it on the sending side, here again so
// that a META block from any transport never makes a read leave the slot).
RPL_HD inline void group_extent(const uint32_t *m, uint32_t g, uint32_t n_groups, u64 slot_cells,
                                u64 *start, u64 *n) {
  u64 st;
  uint32_t np;
  layout::scan_row(m, g, n_groups, 0ull, &st, &np);
  u64 c = np;
  if (st >= slot_cells) c = 0ull;
  else if (c > slot_cells - st) c = slot_cells - st;
  *start = c ? st : 0ull;
  *n = c;
}

// the rank's slot was cut (META flag bit 0) and it holds group g: that group may have lost cells
RPL_HD inline bool group_cut(const uint32_t *m, uint32_t g) { return (m[3] & 1u) && g < m[2]; }

// first record of the sorted list c[0 .. n) whose key is not below `key`
RPL_HD inline u64 lower_bound(const rplgpu_cell_t *c, u64 n, uint32_t key) {
  u64 lo = 0ull, hi = n;
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (c[mid].key < key) lo = mid + 1ull; else hi = mid;
  }
  return lo;
}

// the point of a cell (x, y, z = 0, intensity): IEEE fp64 quotients, i.e. the correctly rounded
// value the voxel kernel's Markstein step produces.  unit = 2^-K (1 / KParams::vox_scale)
RPL_HD inline void cell_point(uint32_t count, uint32_t isum, double sx, double sy, double unit,
                              float *xyzi) {
  const double dc = (double)count;
  xyzi[0] = (float)((sx / dc) * unit);
  xyzi[1] = (float)((sy / dc) * unit);
  xyzi[2] = 0.0f;
  xyzi[3] = (float)((double)isum / dc);
}

}  // namespace cells
}  // namespace rpl
