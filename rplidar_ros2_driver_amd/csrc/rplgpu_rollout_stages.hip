// rplgpu_rollout_stages.hip — the extern "C" entry points of E27, candidate motions rolled out of a pose and scored
// (include/rplgpu_msg.h): rplgpu_rollout_dev and the host-buffer door rplgpu_rollout.
//
// Host side only: argument checks, the launches and the door; the kernels are in rpl_rollout.hip, the spec's rules and
// the host twin in rplgpu_rollout_rules.cpp.  The handle and the doors' per-call buffer come from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_rules.hpp"
#include "rpl_rollout.hpp"

using namespace rpl::host;

namespace {

// K, the steps, F and delta_per_step, which the call and its door take alike
bool counts_ok(rplgpu_ctx *h, const char *fn, uint32_t K, uint32_t T, uint32_t F, uint32_t delta_per_step) {
  return (K != 0 && K <= RPLGPU_MAX_POSES && (uint64_t)K * T <= (1ull << 24) && F != 0 &&
          F <= RPLGPU_ROLLOUT_MAX_FOOTPRINT && delta_per_step <= 1u) ||
         refuse(h, fn, "K must be in 1 .. RPLGPU_MAX_POSES with K * steps <= 2^24, F in 1 .. "
                       "RPLGPU_ROLLOUT_MAX_FOOTPRINT, delta_per_step 0 or 1");
}

}  // namespace

extern "C" {

int32_t rplgpu_rollout_dev(rplgpu_handle_t h, const rplgpu_rollout_t *r, const float *d_start,
                           uint32_t start_per_group, const float *d_delta, uint64_t delta_stride,
                           uint32_t delta_per_group, uint32_t delta_per_step, const float *d_footprint, uint32_t F,
                           const int8_t *d_grid, uint64_t grid_stride, const uint32_t *d_potential,
                           uint64_t potential_stride, uint32_t grid_per_group, uint32_t G, uint32_t K,
                           uint32_t *d_out, uint64_t out_stride, float *d_end_poses, uint64_t end_stride,
                           uint32_t *d_result, uint32_t *d_scratch) {
  const char *fn = "rplgpu_rollout_dev";
  if (!h || !r) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_rollout_check(r) != RPLGPU_OK) return refuse_spec(h, fn, "rplgpu_rollout_t");
  const PoseListDoor door{h, fn};
  const uint32_t T = r->steps;
  if (!door.groups(G) || !counts_ok(h, fn, K, T, F, delta_per_step)) return RPLGPU_ERR_INVALID_ARG;
  if (!d_start || !d_delta || !d_footprint || !d_grid || !d_out || !d_result || !d_scratch ||
      misaligned(d_start, 15u) || misaligned(d_delta, 15u) || misaligned(d_out, 15u) || misaligned(d_end_poses, 15u) ||
      misaligned(d_scratch, 15u) || misaligned(d_footprint, 7u) || misaligned(d_result, 3u)) {
    refuse(h, fn, "a required pointer is missing or a pointer is misaligned (16 bytes: d_start, d_delta, d_out, "
                  "d_end_poses, d_scratch; 8: d_footprint; 4: d_result)");
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t cells = (uint64_t)r->width * r->height, n_delta = (uint64_t)K * (delta_per_step ? T : 1u);
  if (!planes_ok(h, fn, cells, d_grid, grid_stride, d_potential, potential_stride)) return RPLGPU_ERR_INVALID_ARG;
  if (delta_stride < 4ull * n_delta || (delta_stride & 3u) || out_stride < 8ull * K || (out_stride & 3u) ||
      (d_end_poses && (end_stride < 4ull * K || (end_stride & 3u)))) {
    refuse(h, fn, "delta_stride >= 4 K (4 K steps per step), out_stride >= 8 K and end_stride >= 4 K (all multiples "
                  "of 4) are required");
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t scratch_words = rplgpu_rollout_scratch_words(G, K);
  if (scratch_words == 0) {
    refuse(h, fn, "G x tiles above RPLGPU_ROLLOUT_MAX_TILES");
    return RPLGPU_ERR_CAPACITY;
  }
  const uint64_t last = G - 1u, maps = grid_per_group ? last : 0ull;
  const Range ranges[] = {
      {d_start, 16ull * (start_per_group ? G : 1u), false},
      {d_delta, 4ull * ((delta_per_group ? last * delta_stride : 0ull) + 4ull * n_delta), false},
      {d_footprint, 8ull * F, false},
      {d_grid, maps * grid_stride + cells, false},
      {d_potential, d_potential ? 4ull * (maps * potential_stride + cells) : 0ull, false},
      {d_out, 4ull * (last * out_stride + 8ull * K), true},
      {d_end_poses, d_end_poses ? 4ull * (last * end_stride + 4ull * K) : 0ull, true},
      {d_result, 32ull * G, true},
      {d_scratch, 4ull * scratch_words, true}};
  if (ranges_clash(ranges)) {
    refuse(h, fn, "an output overlaps an input or another output");
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_start, "d_start", true}, {d_delta, "d_delta", true}, {d_footprint, "d_footprint", true},
                           {d_grid, "d_grid", true}, {d_out, "d_out", true}, {d_result, "d_result", true},
                           {d_scratch, "d_scratch", true}, {d_potential, "d_potential", false},
                           {d_end_poses, "d_end_poses", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  const rpl::RolloutK k{r->origin_x, r->origin_y, r->resolution, r->width, r->height, r->lethal, r->unknown_value,
                        r->steps,    r->min_steps, r->a_end,      r->a_min, r->a_sum,  r->a_max};
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_rollout(h->stream, k, d_start, start_per_group, d_delta, delta_stride, delta_per_group,
                                 delta_per_step, d_footprint, F, d_grid, grid_stride, d_potential, potential_stride,
                                 grid_per_group, G, K, d_out, out_stride, d_end_poses, end_stride, d_result,
                                 d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_rollout(rplgpu_handle_t h, const rplgpu_rollout_t *r, const float *start, const float *delta,
                       uint32_t delta_per_step, const float *footprint, uint32_t F, const int8_t *grid,
                       const uint32_t *potential, uint32_t K, uint32_t *out, float *end_poses, uint32_t result[8]) {
  const char *fn = "rplgpu_rollout";
  if (!h || !r || !start || !delta || !footprint || !grid || !out || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_rollout_check(r) != RPLGPU_OK) return refuse_spec(h, fn, "rplgpu_rollout_t");
  if (!counts_ok(h, fn, K, r->steps, F, delta_per_step)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells = (size_t)r->width * r->height, stride = (cells + 3u) & ~(size_t)3u;
  const size_t n_delta = (size_t)K * (delta_per_step ? r->steps : 1u);
  // start | deltas | footprint | grid | field | out | end poses | result | scratch
  DoorBuffer buf(h, fn);
  const size_t o_start = buf.part(16), o_delta = buf.part(16u * n_delta), o_fp = buf.part(8u * (size_t)F);
  const size_t o_grid = buf.part(stride), o_pot = buf.part_if(potential, 4u * cells);
  const size_t o_out = buf.part(32u * (size_t)K), o_end = buf.part_if(end_poses, 16u * (size_t)K);
  const size_t o_res = buf.part(32), o_scr = buf.part(4u * (size_t)rplgpu_rollout_scratch_words(1, K));
  uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, buf.put(o_start, start, 16));
    RPL_HIP(h, buf.put(o_delta, delta, 16u * n_delta));
    RPL_HIP(h, buf.put(o_fp, footprint, 8u * (size_t)F));
    RPL_HIP(h, buf.put(o_grid, grid, cells));
    RPL_HIP(h, buf.put(o_pot, potential, 4u * cells));
    const int32_t irc = rplgpu_rollout_dev(
        h, r, buf.at<const float>(o_start), 0, buf.at<const float>(o_delta), 4u * n_delta, 0, delta_per_step,
        buf.at<const float>(o_fp), F, buf.at<const int8_t>(o_grid), stride, buf.at<const uint32_t>(o_pot), cells, 0,
        1, K, buf.at<uint32_t>(o_out), 8ull * K, buf.at<float>(o_end), 4ull * K, buf.at<uint32_t>(o_res),
        buf.at<uint32_t>(o_scr));
    if (irc) return irc;
    RPL_HIP(h, buf.get(out, o_out, 32u * (size_t)K));
    RPL_HIP(h, buf.get(end_poses, o_end, 16u * (size_t)K));
    RPL_HIP(h, buf.get(words, o_res, 32));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, words, 32);
  return RPLGPU_OK;
}

}  // extern "C"
