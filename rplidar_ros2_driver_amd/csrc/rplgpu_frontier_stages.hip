// rplgpu_frontier_stages.hip — the extern "C" entry points of E29, a map's frontiers found, grouped and the next goal
// picked (include/rplgpu_msg.h): rplgpu_frontiers_dev and the host-buffer door rplgpu_frontiers.
//
// Host side only: argument checks, the launches and the door; the kernels are in rpl_frontier.hip, the spec's rules
// and the host twin in rplgpu_frontier_rules.cpp.  The handle and the door's per-call buffer come from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_rules.hpp"
#include "rpl_frontier.hpp"

using namespace rpl::host;

extern "C" {

int32_t rplgpu_frontiers_dev(rplgpu_handle_t h, const rplgpu_frontiers_t *f, const int8_t *d_grid,
                             uint64_t grid_stride, const uint32_t *d_potential, uint64_t potential_stride, uint32_t G,
                             uint32_t comp_cap, uint32_t *d_labels_out, uint64_t label_stride, uint32_t *d_rows,
                             uint64_t row_stride, uint32_t row_cap, uint32_t *d_goal_out, uint64_t goal_stride,
                             uint32_t *d_n_goal_out, uint32_t *d_result, uint32_t *d_scratch) {
  const char *fn = "rplgpu_frontiers_dev";
  const std::string at = std::string(fn) + ": ";
  if (!h || !f) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_frontiers_check(f) != RPLGPU_OK) return refuse_spec(h, fn, "rplgpu_frontiers_t");
  const PoseListDoor door{h, fn};
  if (!door.groups(G)) return RPLGPU_ERR_INVALID_ARG;
  if (comp_cap == 0 || comp_cap > RPLGPU_FRONTIER_MAX_COMPS) {
    h->err = at + "comp_cap must be in 1 .. RPLGPU_FRONTIER_MAX_COMPS";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_grid || !d_result || !d_scratch || (row_cap != 0 && !d_rows) || (!d_goal_out) != (!d_n_goal_out)) {
    h->err = at + "d_grid, d_result and d_scratch must be given, d_rows with row_cap != 0, d_goal_out and "
                  "d_n_goal_out both or neither";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (misaligned(d_labels_out, 3u) || misaligned(d_rows, 3u) || misaligned(d_goal_out, 3u) ||
      misaligned(d_n_goal_out, 3u) || misaligned(d_result, 3u) || misaligned(d_scratch, 15u)) {
    h->err = at + "every pointer must be 4-byte aligned, d_scratch 16-byte";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t cells = (uint64_t)f->width * f->height;
  if (!planes_ok(h, fn, cells, d_grid, grid_stride, d_potential, potential_stride)) return RPLGPU_ERR_INVALID_ARG;
  if ((d_labels_out && label_stride < cells) || (d_rows && row_stride < 8ull * row_cap) ||
      (d_goal_out && goal_stride == 0)) {
    h->err = at + "label_stride >= width * height, row_stride >= 8 row_cap and goal_stride >= 1 are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  rpl::FrLayout l;
  bool capacity = false;
  if (!rpl::frontier_layout(f->width, f->height, G, comp_cap, &l, &capacity)) {
    h->err = at + (capacity ? "G x tiles above RPLGPU_NAV_MAX_TILES" : "the shape is out of range");
    return capacity ? RPLGPU_ERR_CAPACITY : RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t last = G - 1u;
  const Range ranges[] = {
      {d_grid, last * grid_stride + cells, false},
      {d_potential, d_potential ? 4ull * (last * potential_stride + cells) : 0ull, false},
      {d_labels_out, d_labels_out ? 4ull * (last * label_stride + cells) : 0ull, true},
      {d_rows, d_rows ? 4ull * (last * row_stride + 8ull * row_cap) : 0ull, true},
      {d_goal_out, d_goal_out ? 4ull * (last * goal_stride + 1ull) : 0ull, true},
      {d_n_goal_out, d_n_goal_out ? 4ull * G : 0ull, true},
      {d_result, 4ull * RPLGPU_FRONTIER_WORDS * G, true},
      {d_scratch, 4ull * l.total * G, true}};
  if (ranges_clash(ranges)) {
    h->err = at + "an output overlaps an input or another output";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_grid, "d_grid", true}, {d_result, "d_result", true}, {d_scratch, "d_scratch", true},
                           {d_potential, "d_potential", false}, {d_labels_out, "d_labels_out", false},
                           {d_rows, "d_rows", false}, {d_goal_out, "d_goal_out", false},
                           {d_n_goal_out, "d_n_goal_out", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  const rpl::FrontierK k{f->width, f->height, f->lethal, f->min_size, f->dist_weight, f->size_weight};
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_frontiers(h->stream, k, d_grid, grid_stride, d_potential, potential_stride, G, comp_cap,
                                   d_labels_out, label_stride, d_rows, row_stride, row_cap, d_goal_out, goal_stride,
                                   d_n_goal_out, d_result, d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_frontiers(rplgpu_handle_t h, const rplgpu_frontiers_t *f, const int8_t *grid, const uint32_t *potential,
                         uint32_t comp_cap, uint32_t *labels_out, uint32_t *rows, uint32_t row_cap, uint32_t *goal_out,
                         uint32_t *n_goal_out, uint32_t result[16]) {
  const char *fn = "rplgpu_frontiers";
  if (!h || !f || !grid || !result || (row_cap != 0 && !rows) || (!goal_out) != (!n_goal_out))
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_frontiers_check(f) != RPLGPU_OK || rplgpu_frontiers_scratch_words(f, 1, comp_cap) == 0)
    return refuse_spec(h, fn, "rplgpu_frontiers_t or comp_cap");
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells = (size_t)f->width * f->height, stride = (cells + 3u) & ~(size_t)3u;
  const size_t row_bytes = 32u * (size_t)row_cap;
  // grid | field | labels | rows | goal | its count | result | scratch
  DoorBuffer buf(h, fn);
  const size_t o_grid = buf.part(stride), o_pot = buf.part_if(potential, 4u * cells);
  const size_t o_lab = buf.part_if(labels_out, 4u * cells), o_rows = buf.part_if(row_cap != 0, row_bytes);
  const size_t o_goal = buf.part_if(goal_out, 4), o_n = buf.part_if(goal_out, 4);
  const size_t o_res = buf.part(4u * RPLGPU_FRONTIER_WORDS);
  const size_t o_scr = buf.part(4u * (size_t)rplgpu_frontiers_scratch_words(f, 1, comp_cap));
  // the small outputs are staged and filled behind the synchronise: a call that fails writes none of them
  uint32_t words[RPLGPU_FRONTIER_WORDS], goal[2] = {0u, 0u};
  std::vector<uint32_t> row_stage(8u * (size_t)row_cap);
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, buf.put(o_grid, grid, cells));
    RPL_HIP(h, buf.put(o_pot, potential, 4u * cells));
    RPL_HIP(h, buf.put(o_rows, rows, row_bytes));
    RPL_HIP(h, buf.put(o_goal, goal_out, 4));
    const int32_t irc = rplgpu_frontiers_dev(h, f, buf.at<const int8_t>(o_grid), stride,
                                             buf.at<const uint32_t>(o_pot), cells, 1, comp_cap,
                                             buf.at<uint32_t>(o_lab), cells, buf.at<uint32_t>(o_rows),
                                             8ull * row_cap, row_cap, buf.at<uint32_t>(o_goal), 1,
                                             buf.at<uint32_t>(o_n), buf.at<uint32_t>(o_res), buf.at<uint32_t>(o_scr));
    if (irc) return irc;
    RPL_HIP(h, buf.get(labels_out, o_lab, 4u * cells));
    RPL_HIP(h, buf.get(row_stage.data(), o_rows, row_bytes));
    RPL_HIP(h, buf.get(&goal[0], o_goal, 4));
    RPL_HIP(h, buf.get(&goal[1], o_n, 4));
    RPL_HIP(h, buf.get(words, o_res, sizeof(words)));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  if (row_cap) std::memcpy(rows, row_stage.data(), row_bytes);
  if (goal_out) {
    *goal_out = goal[0];
    *n_goal_out = goal[1];
  }
  std::memcpy(result, words, sizeof(words));
  return RPLGPU_OK;
}

}  // extern "C"
