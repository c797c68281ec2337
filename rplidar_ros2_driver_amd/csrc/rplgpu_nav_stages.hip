// rplgpu_nav_stages.hip — the extern "C" entry points of E26, the cost-to-goal field over a costmap and the paths
// down it (include/rplgpu_msg.h): rplgpu_nav_field_dev, rplgpu_nav_paths_dev and the host-buffer door
// rplgpu_nav_field.
//
// Host side only: argument checks, the launches and the door; the kernels are in rpl_nav.hip, the spec's rules and the
// host twins in rplgpu_nav_rules.cpp.  The handle and the doors' per-call buffer come from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_nav.hpp"

using namespace rpl::host;

namespace {

rpl::NavK nav_k(const rplgpu_nav_field_t *f) {
  rpl::NavK k{f->width, f->height, f->lethal, f->neutral, f->factor, f->unknown_cost, f->cap, 0u, 0u};
  (void)rpl::nav_tiles(f->width, f->height, 1, &k.tiles_x, &k.tiles_y);
  return k;
}

// the spec, the groups, the grids and the fields, which both calls take alike
int32_t field_check(rplgpu_handle_t h, const char *fn, const rplgpu_nav_field_t *f, const int8_t *d_grid,
                    uint64_t grid_stride, const uint32_t *d_potential, uint64_t potential_stride, uint32_t G) {
  if (!f || !d_grid || !d_potential) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_nav_field_check(f) != RPLGPU_OK) return refuse_spec(h, fn, "rplgpu_nav_field_t");
  const PoseListDoor door{h, fn};
  if (!door.groups(G) ||
      !planes_ok(h, fn, (uint64_t)f->width * f->height, d_grid, grid_stride, d_potential, potential_stride))
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

}  // namespace

extern "C" {

int32_t rplgpu_nav_field_dev(rplgpu_handle_t h, const rplgpu_nav_field_t *f, const int8_t *d_grid,
                             uint64_t grid_stride, uint32_t G, const uint32_t *d_goals, uint64_t goal_stride,
                             const uint32_t *d_n_goals, uint32_t *d_potential, uint64_t potential_stride,
                             uint32_t *d_scratch, uint32_t resume, uint32_t *d_result) {
  const char *fn = "rplgpu_nav_field_dev";
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (int32_t rc = field_check(h, fn, f, d_grid, grid_stride, d_potential, potential_stride, G)) return rc;
  if (!d_goals || !d_n_goals || !d_scratch || !d_result || resume > 1u) {
    h->err = std::string(fn) + ": d_goals, d_n_goals, d_scratch and d_result must be given and resume be 0 or 1";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (goal_stride == 0 || misaligned(d_goals, 3u) || misaligned(d_n_goals, 3u) || misaligned(d_scratch, 3u) ||
      misaligned(d_result, 3u)) {
    h->err = std::string(fn) + ": goal_stride must be >= 1, every pointer 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (rplgpu_nav_field_scratch_words(f, G) == 0) {
    h->err = std::string(fn) + ": G x tiles above RPLGPU_NAV_MAX_TILES";
    return RPLGPU_ERR_CAPACITY;
  }
  if (!device_readable(h, {{d_grid, "d_grid", true}, {d_goals, "d_goals", true}, {d_n_goals, "d_n_goals", true},
                           {d_potential, "d_potential", true}, {d_scratch, "d_scratch", true},
                           {d_result, "d_result", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  const rpl::NavK k = nav_k(f);
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_nav_init(h->stream, k, G, d_potential, potential_stride, d_scratch, resume, d_result));
  RPL_HIP(h, rpl::launch_nav_goals(h->stream, k, G, d_goals, goal_stride, d_n_goals, d_potential, potential_stride,
                                   d_scratch, resume, d_result));
  for (uint32_t round = 0; round < f->rounds; ++round)
    RPL_HIP(h, rpl::launch_nav_relax(h->stream, k, G, d_grid, grid_stride, d_potential, potential_stride, d_scratch,
                                     round, d_result));
  RPL_HIP(h, rpl::launch_nav_close(h->stream, k, G, d_potential, potential_stride, d_scratch, f->rounds, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_nav_paths_dev(rplgpu_handle_t h, const rplgpu_nav_field_t *f, const int8_t *d_grid,
                             uint64_t grid_stride, const uint32_t *d_potential, uint64_t potential_stride,
                             uint32_t G, const uint32_t *d_starts, uint32_t S, uint32_t *d_paths, uint32_t max_len,
                             uint32_t *d_info) {
  const char *fn = "rplgpu_nav_paths_dev";
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (int32_t rc = field_check(h, fn, f, d_grid, grid_stride, d_potential, potential_stride, G)) return rc;
  if (!d_starts || !d_paths || !d_info || S == 0 || S > RPLGPU_NAV_MAX_STARTS || max_len == 0) {
    h->err = std::string(fn) + ": d_starts, d_paths and d_info must be given, S be 1 .. RPLGPU_NAV_MAX_STARTS, max_len >= 1";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (misaligned(d_starts, 3u) || misaligned(d_paths, 3u) || misaligned(d_info, 3u)) {
    h->err = std::string(fn) + ": every pointer must be 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_grid, "d_grid", true}, {d_potential, "d_potential", true}, {d_starts, "d_starts", true},
                           {d_paths, "d_paths", true}, {d_info, "d_info", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_nav_paths(h->stream, nav_k(f), G, d_grid, grid_stride, d_potential, potential_stride,
                                   d_starts, S, d_paths, max_len, d_info));
  return RPLGPU_OK;
}

int32_t rplgpu_nav_field(rplgpu_handle_t h, const rplgpu_nav_field_t *f, const int8_t *grid, const uint32_t *goals,
                         uint32_t n_goals, uint32_t *potential, uint32_t result[8], const uint32_t *starts,
                         uint32_t S, uint32_t *paths, uint32_t max_len, uint32_t *info) {
  const char *fn = "rplgpu_nav_field";
  if (!h || !f || !grid || !potential || !result || (n_goals != 0 && !goals)) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_nav_field_check(f) != RPLGPU_OK) return refuse_spec(h, fn, "rplgpu_nav_field_t");
  if (starts && (!paths || !info || S == 0 || S > RPLGPU_NAV_MAX_STARTS || max_len == 0)) {
    h->err = std::string(fn) + ": with starts, paths and info must be given, S be 1 .. RPLGPU_NAV_MAX_STARTS, max_len >= 1";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells = (size_t)f->width * f->height, stride = (cells + 3u) & ~(size_t)3u;
  const size_t path_bytes = starts ? 4u * (size_t)S * max_len : 0u;
  // grid | goals | their number | field | scratch | result | starts | paths | info
  DoorBuffer buf(h, fn);
  const size_t o_grid = buf.part(stride), o_goals = buf.part(4u * (size_t)std::max(n_goals, 1u)), o_n = buf.part(4);
  const size_t o_pot = buf.part(4u * cells), o_scr = buf.part(4u * (size_t)rplgpu_nav_field_scratch_words(f, 1));
  const size_t o_res = buf.part(32);
  const size_t o_starts = buf.part_if(starts, 4u * (size_t)S), o_paths = buf.part_if(starts, path_bytes);
  const size_t o_info = buf.part_if(starts, 16u * (size_t)S);
  uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, buf.put(o_grid, grid, cells));
    RPL_HIP(h, buf.put(o_goals, goals, 4u * (size_t)n_goals));
    RPL_HIP(h, buf.put(o_n, &n_goals, 4));
    uint32_t visits = 0, rounds = 0;
    for (uint32_t call = 0; call < 64u; ++call) {
      const int32_t irc = rplgpu_nav_field_dev(h, f, buf.at<const int8_t>(o_grid), stride, 1,
                                               buf.at<const uint32_t>(o_goals), std::max(n_goals, 1u),
                                               buf.at<const uint32_t>(o_n), buf.at<uint32_t>(o_pot), cells,
                                               buf.at<uint32_t>(o_scr), call ? 1u : 0u, buf.at<uint32_t>(o_res));
      if (irc) return irc;
      RPL_HIP(h, buf.get(words, o_res, 32));
      RPL_HIP(h, hipStreamSynchronize(h->stream));
      visits += words[6];
      rounds += words[7];
      if (words[0] == 0) break;
    }
    words[6] = visits;
    words[7] = rounds;
    RPL_HIP(h, buf.get(potential, o_pot, 4u * cells));
    if (starts) {
      RPL_HIP(h, buf.put(o_starts, starts, 4u * (size_t)S));
      RPL_HIP(h, buf.put(o_paths, paths, path_bytes));
      const int32_t prc = rplgpu_nav_paths_dev(h, f, buf.at<const int8_t>(o_grid), stride,
                                               buf.at<const uint32_t>(o_pot), cells, 1,
                                               buf.at<const uint32_t>(o_starts), S, buf.at<uint32_t>(o_paths), max_len,
                                               buf.at<uint32_t>(o_info));
      if (prc) return prc;
      RPL_HIP(h, buf.get(paths, o_paths, path_bytes));
      RPL_HIP(h, buf.get(info, o_info, 16u * (size_t)S));
    }
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, words, 32);
  return RPLGPU_OK;
}

}  // extern "C"
