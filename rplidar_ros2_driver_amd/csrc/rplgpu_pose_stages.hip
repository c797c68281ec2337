// rplgpu_pose_stages.hip — the doors of the stages that work on pose lists (include/rplgpu_msg.h): E15 scoring, E16
// resampling, E17 the pose estimate, E18 motion noise, E19 seeding, E20 occupied bins, E21 clusters of those bins, E22
// the beam fan cast into a grid, E23 scoring without the beams the list disagrees with.
//
// Everything here takes a handle or sizes a launch: the rplgpu_*_dev entry points (pointer, stride and overlap checks,
// then rpl::launch_*), the host-buffer forms that copy through a DoorBuffer, and the rplgpu_*_scratch_words wrappers.
// The rules those doors check against (defaults, spec checks, tables, the host twins) are plain C++ in
// rplgpu_pose_rules.cpp and are called through their public prototypes; rplgpu_cast_beams alone stays here, because
// it calls rplgpu_scan_merge_edges of rplgpu_scan_stages.hip.  The kernels are in rpl_pose.hip, rpl_resample.hip,
// rpl_estimate.hip, rpl_motion.hip, rpl_seed.hip, rpl_bins.hip, rpl_clusters.hip, rpl_cast.hip and rpl_agree.hip.  The
// handle, the helpers of rplgpu_api.hip, the scan-stage prologue and the doors' per-call buffer come from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_agree.hpp"

using namespace rpl::host;

extern "C" {

// ---- E15: a list of arbitrary poses weighed against a likelihood field (include/rplgpu_msg.h) ------------------

// The argument checks E15 and E23 share behind check_batch, in E15's order; fn names the entry point in the texts.
// spec_ok: the stage's own spec check passed; cells: width * height of that spec (read only when spec_ok).
static int32_t score_args_check(rplgpu_handle_t h, const char *fn, const char *spec_name, bool spec_ok, uint64_t cells,
                                uint32_t group, const float *d_poses, uint32_t P, uint64_t pose_stride,
                                const int8_t *d_field, uint64_t field_stride, const uint32_t *d_weights,
                                uint64_t weight_stride, const uint32_t *d_result, const uint32_t *d_status) {
  const std::string at = std::string(fn) + ": ";
  if (!d_poses || !d_field || !d_weights || !d_result || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (!spec_ok) {
    h->err = at + "invalid " + spec_name + " (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, fn}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (pose_stride < 4ull * P || (pose_stride & 3u) || (reinterpret_cast<uintptr_t>(d_poses) & 15u)) {
    h->err = at + "pose_stride must be >= 4 P floats and a multiple of 4, d_poses 16-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (field_stride < cells || (field_stride & 3u) || (reinterpret_cast<uintptr_t>(d_field) & 3u)) {
    h->err = at + "field_stride must be >= width * height and a multiple of 4, d_field 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (weight_stride < P || (reinterpret_cast<uintptr_t>(d_weights) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_result) & 3u) || (reinterpret_cast<uintptr_t>(d_status) & 3u)) {
    h->err = at + "weight_stride must be >= P, d_weights / d_result / d_status 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  return RPLGPU_OK;
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t pose_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                         const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                         const float *d_motion, const float *d_pose2d, const float *d_t0,
                         const rplgpu_pose_score_t *s, const float *d_poses, uint32_t P, uint64_t pose_stride,
                         uint32_t poses_per_group, const int8_t *d_field, uint64_t field_stride,
                         uint32_t field_per_group, uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_result,
                         uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !s) return RPLGPU_ERR_INVALID_ARG;
  if ((rc = score_args_check(h, "rplgpu_score_poses_dev", "rplgpu_pose_score_t", rplgpu_pose_score_check(s) == RPLGPU_OK,
                             (uint64_t)s->width * s->height, group, d_poses, P, pose_stride, d_field, field_stride,
                             d_weights, weight_stride, d_result, d_status)))
    return rc;
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_poses, "d_poses", true},
                           {d_field, "d_field", true}, {d_weights, "d_weights", true}, {d_result, "d_result", true},
                           {d_status, "d_status", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  ScanPrologue pro;
  if ((rc = pro.admit(h, "rplgpu_score_poses_dev", p, d_motion, d_t0, B, group))) return rc;
  if ((uint64_t)pro.group * n_stride > (1ull << 24)) {  // 127 x points stays below 2^32: no weight wraps
    h->err = "rplgpu_score_poses_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((uint64_t)pro.G * ((P + 255u) / 256u) > 0x7FFFFFFFull) {  // (launch_pose_prepare's grid; before anything is queued)
    h->err = "rplgpu_score_poses_dev: groups x P too large for one call";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const rpl::PoseK k{s->origin_x, s->origin_y, s->resolution, s->width, s->height};
  if ((rc = pro.begin(h, d_nodes, n_stride, d_n_per_scan, B, p, d_t0, d_status))) return rc;
  RPL_HIP(h, rpl::launch_pose_prepare(h->stream, d_weights, weight_stride, pro.G, P, d_result));
  RPL_HIP(h, rpl::launch_pose_score(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T, pro.mask,
                                    kMaskStride, d_motion, d_pose2d, k, d_poses, P, pose_stride, poses_per_group,
                                    d_field, field_stride, field_per_group, d_weights, weight_stride, d_result,
                                    d_status));
  RPL_HIP(h, rpl::launch_pose_best(h->stream, d_weights, weight_stride, pro.G, P, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_score_poses_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const rplgpu_pose_score_t *s,
                               const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                               const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group,
                               uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_result,
                               uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return pose_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, s, d_poses, P,
                   pose_stride, poses_per_group, d_field, field_stride, field_per_group, d_weights, weight_stride,
                   d_result, d_status);
}

int32_t rplgpu_score_poses(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                           const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                           const float *motion, const float *pose2d, const float *t0,
                           const rplgpu_pose_score_t *s, const float *poses, uint32_t P, const int8_t *field,
                           uint32_t *weights_out, uint32_t result[8], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !s || !poses || !field || !result || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_score_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_score_poses: invalid rplgpu_pose_score_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_score_poses"}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)s->width * s->height, stride = (cells_n + 3u) & ~(size_t)3u;
  // field | poses | weights | the scans | result + status
  DoorBuffer buf(h, "rplgpu_score_poses");
  const size_t o_field = buf.part(stride), o_ps = buf.part(16u * (size_t)P), o_wt = buf.part(4u * (size_t)P);
  DoorScans scans(buf, nodes, n_stride, n_per_scan, n_scans, motion, pose2d, t0);
  const size_t o_small = buf.part(48);
  uint32_t small[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_field), field, cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_ps), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (int32_t urc = scans.upload(h, buf)) return urc;
    uint32_t *d_small = buf.at<uint32_t>(o_small);
    const int32_t irc = pose_impl(h, scans.d_nodes, n_stride, scans.d_n_per_scan, n_scans, n_scans, p, scans.d_motion,
                                  scans.d_pose2d, scans.d_t0, s, buf.at<const float>(o_ps), P, 4ull * P, 0,
                                  buf.at<const int8_t>(o_field), stride, 0, buf.at<uint32_t>(o_wt), P, d_small,
                                  d_small + 8);
    if (irc) return irc;
    if (weights_out)
      RPL_HIP(h, hipMemcpyAsync(weights_out, buf.at(o_wt), 4u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 36, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, small, 32);
  if (status) *status = small[8];
  return RPLGPU_OK;
}

// ---- E16: a weighted pose list resampled and moved (include/rplgpu_msg.h) ---------------------------------------

uint64_t rplgpu_resample_scratch_words(uint32_t G, uint32_t P) { return rpl::resample_scratch_words(G, P); }

int32_t rplgpu_resample_poses_dev(rplgpu_handle_t h, const uint32_t *d_weights, uint64_t weight_stride,
                                  const float *d_poses, uint64_t pose_stride, uint32_t poses_per_group, uint32_t G,
                                  uint32_t P, uint32_t M, const uint32_t *d_u, const float *d_delta,
                                  uint32_t n_delta, uint64_t delta_stride, uint32_t delta_per_group,
                                  float *d_poses_out, uint64_t out_stride, uint32_t *d_ancestors,
                                  uint64_t anc_stride, uint32_t *d_result, uint32_t *d_scratch) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (!PoseListDoor{h, "rplgpu_resample_poses_dev"}.groups(G)) return RPLGPU_ERR_INVALID_ARG;
  if (P == 0 || P > RPLGPU_MAX_POSES || M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_resample_poses_dev: P and M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_weights || !d_poses || !d_poses_out || !d_result || !d_scratch || misaligned(d_weights, 3) || misaligned(d_poses, 15) ||
      misaligned(d_poses_out, 15) || misaligned(d_result, 3) || misaligned(d_scratch, 7) || misaligned(d_u, 3) || misaligned(d_delta, 15) ||
      misaligned(d_ancestors, 3)) {
    h->err = "rplgpu_resample_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for pose "
             "lists and deltas, 8 for d_scratch, 4 otherwise)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (weight_stride < P || pose_stride < 4ull * P || (pose_stride & 3u) || out_stride < 4ull * M ||
      (out_stride & 3u) || (d_ancestors && anc_stride < M)) {
    h->err = "rplgpu_resample_poses_dev: weight_stride >= P, pose_stride >= 4 P, out_stride >= 4 M (both multiples "
             "of 4) and anc_stride >= M are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_delta && ((n_delta != 1u && n_delta != M) || delta_stride < 4ull * n_delta || (delta_stride & 3u))) {
    h->err = "rplgpu_resample_poses_dev: n_delta must be 1 or M, delta_stride >= 4 n_delta and a multiple of 4";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t in_bytes = 4ull * ((poses_per_group ? (uint64_t)(G - 1u) * pose_stride : 0ull) + 4ull * P);
  const uint64_t out_bytes = 4ull * ((uint64_t)(G - 1u) * out_stride + 4ull * M);
  if (rpl::ranges_overlap(d_poses, in_bytes, d_poses_out, out_bytes)) {
    h->err = "rplgpu_resample_poses_dev: d_poses_out overlaps d_poses";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_weights, "d_weights", true}, {d_poses, "d_poses", true},
                           {d_poses_out, "d_poses_out", true}, {d_result, "d_result", true},
                           {d_scratch, "d_scratch", true}, {d_u, "d_u", false}, {d_delta, "d_delta", false},
                           {d_ancestors, "d_ancestors", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_resample(h->stream, d_weights, weight_stride, d_poses, pose_stride, poses_per_group, G, P,
                                  M, d_u, d_delta, d_delta ? n_delta : 1u, delta_stride, delta_per_group,
                                  d_poses_out, out_stride, d_ancestors, anc_stride, d_result, d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_resample_poses(rplgpu_handle_t h, const uint32_t *weights, uint32_t P, uint32_t M, uint32_t u,
                              const float *poses, const float *delta, uint32_t n_delta, float *poses_out,
                              uint32_t *ancestors_out, uint32_t result[8]) {
  if (!h || !weights || !poses || !poses_out || !result) return RPLGPU_ERR_INVALID_ARG;
  if (P == 0 || P > RPLGPU_MAX_POSES || M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_resample_poses: P and M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (delta && n_delta != 1u && n_delta != M) {
    h->err = "rplgpu_resample_poses: n_delta must be 1 or M";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (rpl::ranges_overlap(poses, 16ull * P, poses_out, 16ull * M)) {
    h->err = "rplgpu_resample_poses: poses_out overlaps poses";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // poses | out | deltas | weights | ancestors | scratch | u + result
  const size_t nd = delta ? n_delta : 0u;
  DoorBuffer buf(h, "rplgpu_resample_poses");
  const size_t o_in = buf.part(16u * (size_t)P), o_out = buf.part(16u * (size_t)M), o_dl = buf.part_if(delta, 16u * nd),
               o_wt = buf.part(4u * (size_t)P), o_anc = buf.part(4u * (size_t)M),
               o_scr = buf.part(4u * (size_t)rplgpu_resample_scratch_words(1, P)), o_small = buf.part(48);
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    uint32_t *d_small = buf.at<uint32_t>(o_small);  // u, then the result at + 4 words
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_in), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_wt), weights, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d_small, &u, 4, hipMemcpyHostToDevice, h->stream));
    if (delta) RPL_HIP(h, hipMemcpyAsync(buf.at(o_dl), delta, 16u * nd, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_resample_poses_dev(
        h, buf.at<const uint32_t>(o_wt), P, buf.at<const float>(o_in), 4ull * P, 0, 1, P, M, d_small,
        buf.at<const float>(o_dl), n_delta, 4ull * nd, 0, buf.at<float>(o_out), 4ull * M, buf.at<uint32_t>(o_anc), M,
        d_small + 4, buf.at<uint32_t>(o_scr));
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(poses_out, buf.at(o_out), 16u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    if (ancestors_out)
      RPL_HIP(h, hipMemcpyAsync(ancestors_out, buf.at(o_anc), 4u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small + 4, 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

// ---- E17: a weighted pose list reduced to a pose estimate (include/rplgpu_msg.h) -------------------------------------

uint64_t rplgpu_estimate_scratch_words(uint32_t G, uint32_t P) { return rpl::estimate_scratch_words(G, P); }

int32_t rplgpu_estimate_poses_dev(rplgpu_handle_t h, const float *d_poses, uint64_t pose_stride,
                                  uint32_t poses_per_group, const uint32_t *d_weights, uint64_t weight_stride,
                                  uint32_t G, uint32_t P, const rplgpu_pose_estimate_t *s, const uint32_t *d_center,
                                  uint64_t center_stride, uint32_t *d_result, uint32_t *d_scratch) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_estimate_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_estimate_poses_dev: invalid rplgpu_pose_estimate_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const PoseListDoor door{h, "rplgpu_estimate_poses_dev"};
  if (!door.groups(G) || !door.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (!d_poses || !d_result || !d_scratch || misaligned(d_poses, 15) || misaligned(d_result, 3) || misaligned(d_scratch, 7) ||
      misaligned(d_weights, 3) || misaligned(d_center, 3)) {
    h->err = "rplgpu_estimate_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for the "
             "pose list, 8 for d_scratch, 4 otherwise)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!door.strides(P, pose_stride, d_weights, weight_stride)) return RPLGPU_ERR_INVALID_ARG;
  if (d_center && center_stride == 0 && G > 1u) {
    h->err = "rplgpu_estimate_poses_dev: center_stride must not be 0 with more than one group";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_poses, "d_poses", true}, {d_result, "d_result", true}, {d_scratch, "d_scratch", true},
                           {d_weights, "d_weights", false}, {d_center, "d_center", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_estimate(h->stream, d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P,
                                  s->xy_scale, s->gate_r2, s->gate_dot, d_center, center_stride, d_result,
                                  d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_estimate_poses(rplgpu_handle_t h, const float *poses, uint32_t P, const uint32_t *weights,
                              const rplgpu_pose_estimate_t *s, uint32_t center, uint32_t result[72]) {
  if (!h || !poses || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_estimate_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_estimate_poses: invalid rplgpu_pose_estimate_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_estimate_poses"}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  // poses | weights | scratch | centre + result
  DoorBuffer buf(h, "rplgpu_estimate_poses");
  const size_t o_in = buf.part(16u * (size_t)P), o_wt = buf.part_if(weights, 4u * (size_t)P),
               o_scr = buf.part(4u * (size_t)rplgpu_estimate_scratch_words(1, P)),
               o_small = buf.part(16u + 4u * RPLGPU_ESTIMATE_WORDS);
  uint32_t words[RPLGPU_ESTIMATE_WORDS];
  const int32_t rc = buf.run([&]() -> int32_t {
    uint32_t *d_small = buf.at<uint32_t>(o_small);  // the centre word, then the result at + 4 words
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_in), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (weights) RPL_HIP(h, hipMemcpyAsync(buf.at(o_wt), weights, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d_small, &center, 4, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_estimate_poses_dev(h, buf.at<const float>(o_in), 4ull * P, 0,
                                                  buf.at<const uint32_t>(o_wt), P, 1, P, s, d_small, 0, d_small + 4,
                                                  buf.at<uint32_t>(o_scr));
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(words, d_small + 4, sizeof(words), hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, words, sizeof(words));
  return RPLGPU_OK;
}

// ---- E18: a pose list's motion noise drawn on the device (include/rplgpu_msg.h) --------------------------------------

int32_t rplgpu_sample_motion_dev(rplgpu_handle_t h, const float *d_odom, uint32_t odom_per_group, uint32_t G,
                                 uint32_t M, const rplgpu_motion_noise_t *s, float *d_delta, uint64_t delta_stride,
                                 uint32_t *d_result) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (!s) {
    h->err = "rplgpu_sample_motion_dev: the rplgpu_motion_noise_t is missing";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_sample_motion_dev"}.groups(G)) return RPLGPU_ERR_INVALID_ARG;
  if (M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_sample_motion_dev: M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_odom || !d_delta || !d_result || misaligned(d_odom, 15) || misaligned(d_delta, 15) || misaligned(d_result, 3)) {
    h->err = "rplgpu_sample_motion_dev: a required pointer is missing or a pointer is misaligned (16 bytes for d_odom "
             "and d_delta, 4 for d_result)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (delta_stride < 4ull * M || (delta_stride & 3u)) {
    h->err = "rplgpu_sample_motion_dev: delta_stride >= 4 M and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_odom, "d_odom", true}, {d_delta, "d_delta", true}, {d_result, "d_result", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_motion(h->stream, d_odom, odom_per_group, G, M, s->seed, s->step, s->first, d_delta,
                                delta_stride, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_sample_motion(rplgpu_handle_t h, const float odom[8], uint32_t M, const rplgpu_motion_noise_t *s,
                             float *delta_out, uint32_t result[8]) {
  if (!h || !odom || !s || !delta_out || !result) return RPLGPU_ERR_INVALID_ARG;
  if (M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_sample_motion: M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  DoorBuffer buf(h, "rplgpu_sample_motion");
  const size_t o_odom = buf.part(32), o_res = buf.part(32), o_dl = buf.part(16u * (size_t)M);
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_odom), odom, 32, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_sample_motion_dev(h, buf.at<const float>(o_odom), 0, 1, M, s, buf.at<float>(o_dl),
                                                 4ull * M, buf.at<uint32_t>(o_res));
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(delta_out, buf.at(o_dl), 16u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, buf.at(o_res), 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

// ---- E19: a pose list seeded over a grid's free cells on the device (include/rplgpu_msg.h) ---------------------------

uint64_t rplgpu_seed_scratch_words(uint32_t G_f, uint32_t width, uint32_t height) {
  return rpl::seed_scratch_words(G_f, width, height);
}

int32_t rplgpu_seed_poses_dev(rplgpu_handle_t h, const rplgpu_pose_seed_t *s, const int8_t *d_grid,
                              uint64_t grid_stride, uint32_t grid_per_group, const float *d_headings, uint32_t H,
                              uint32_t G, uint32_t M, const rplgpu_motion_noise_t *noise, float *d_poses_out,
                              uint64_t out_stride, uint32_t *d_cells_out, uint64_t cell_stride, uint32_t *d_result,
                              uint32_t *d_scratch) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_seed_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_seed_poses_dev: the rplgpu_pose_seed_t is missing or rplgpu_pose_seed_check refuses it";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!noise) {
    h->err = "rplgpu_seed_poses_dev: the rplgpu_motion_noise_t is missing";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_seed_poses_dev"}.groups(G)) return RPLGPU_ERR_INVALID_ARG;
  if (M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_seed_poses_dev: M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (H == 0 || H > 65536u) {
    h->err = "rplgpu_seed_poses_dev: H must be in 1 .. 65536";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_grid || !d_headings || !d_poses_out || !d_result || !d_scratch || misaligned(d_grid, 3) || misaligned(d_headings, 7) ||
      misaligned(d_poses_out, 15) || misaligned(d_cells_out, 3) || misaligned(d_result, 3) || misaligned(d_scratch, 7)) {
    h->err = "rplgpu_seed_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for "
             "d_poses_out, 8 for d_headings and d_scratch, 4 for d_grid, d_cells_out and d_result)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t cells = (uint64_t)s->width * s->height;
  if (grid_stride < cells || (grid_stride & 3u)) {
    h->err = "rplgpu_seed_poses_dev: grid_stride >= width * height and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (out_stride < 4ull * M || (out_stride & 3u)) {
    h->err = "rplgpu_seed_poses_dev: out_stride >= 4 M and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_cells_out && cell_stride < M) {
    h->err = "rplgpu_seed_poses_dev: cell_stride >= M is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_grid, "d_grid", true}, {d_headings, "d_headings", true},
                           {d_poses_out, "d_poses_out", true}, {d_result, "d_result", true},
                           {d_scratch, "d_scratch", true}, {d_cells_out, "d_cells_out", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  rpl::SeedK k;
  k.origin_x = s->origin_x;
  k.origin_y = s->origin_y;
  k.resolution = s->resolution;
  k.width = s->width;
  k.height = s->height;
  k.free_lo = s->free_lo;
  k.free_hi = s->free_hi;
  k.centres = s->flags & 1u;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_seed(h->stream, k, d_grid, grid_stride, grid_per_group, d_headings, H, G, M, noise->seed,
                              noise->step, noise->first, d_poses_out, out_stride, d_cells_out, cell_stride, d_result,
                              d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_seed_poses(rplgpu_handle_t h, const rplgpu_pose_seed_t *s, const int8_t *grid, const float *headings,
                          uint32_t H, uint32_t M, const rplgpu_motion_noise_t *noise, float *poses_out,
                          uint32_t *cells_out, uint32_t result[8]) {
  if (!h || !grid || !headings || !noise || !poses_out || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_seed_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_seed_poses: the rplgpu_pose_seed_t is missing or rplgpu_pose_seed_check refuses it";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (M == 0 || M > RPLGPU_MAX_POSES || H == 0 || H > 65536u) {
    h->err = "rplgpu_seed_poses: M must be in 1 .. RPLGPU_MAX_POSES and H in 1 .. 65536";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // result | headings | grid | scratch | cells | poses
  const size_t cells = (size_t)s->width * s->height, gstride = (cells + 3u) & ~(size_t)3u;
  DoorBuffer buf(h, "rplgpu_seed_poses");
  const size_t o_res = buf.part(32), o_head = buf.part(8u * (size_t)H), o_grid = buf.part(gstride),
               o_scr = buf.part(4u * (size_t)rplgpu_seed_scratch_words(1, s->width, s->height)),
               o_cells = buf.part(4u * (size_t)M), o_poses = buf.part(16u * (size_t)M);
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemsetAsync(buf.at(o_grid), 0, up16(gstride), h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_head), headings, 8u * (size_t)H, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_grid), grid, cells, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_seed_poses_dev(h, s, buf.at<const int8_t>(o_grid), gstride, 0,
                                              buf.at<const float>(o_head), H, 1, M, noise, buf.at<float>(o_poses),
                                              4ull * M, buf.at<uint32_t>(o_cells), M, buf.at<uint32_t>(o_res),
                                              buf.at<uint32_t>(o_scr));
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(poses_out, buf.at(o_poses), 16u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    if (cells_out)
      RPL_HIP(h, hipMemcpyAsync(cells_out, buf.at(o_cells), 4u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, buf.at(o_res), 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

// ---- E20: a pose list's occupied bins counted on the device (include/rplgpu_msg.h) -----------------------------------

int32_t rplgpu_bin_poses_dev(rplgpu_handle_t h, const rplgpu_pose_bins_t *s, const float *d_poses,
                             uint64_t pose_stride, uint32_t poses_per_group, const uint32_t *d_weights,
                             uint64_t weight_stride, uint32_t G, uint32_t P, const float *d_edges, uint32_t T,
                             uint32_t *d_map, uint64_t map_stride, uint32_t *d_bins_out, uint64_t bin_stride,
                             uint32_t *d_result) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_bins_check(s, T) != RPLGPU_OK) {
    h->err = "rplgpu_bin_poses_dev: the rplgpu_pose_bins_t is missing or rplgpu_pose_bins_check refuses it or T";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const PoseListDoor door{h, "rplgpu_bin_poses_dev"};
  if (!door.groups(G) || !door.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (!d_poses || !d_edges || !d_map || !d_result || misaligned(d_poses, 15) || misaligned(d_edges, 7) || misaligned(d_map, 7) ||
      misaligned(d_weights, 3) || misaligned(d_bins_out, 3) || misaligned(d_result, 3)) {
    h->err = "rplgpu_bin_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for d_poses, "
             "8 for d_edges and d_map, 4 for d_weights, d_bins_out and d_result)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!door.strides(P, pose_stride, d_weights, weight_stride)) return RPLGPU_ERR_INVALID_ARG;
  const uint64_t words = rpl::bin_map_words(s->nx * s->ny * T);
  if (map_stride < words || (map_stride & 1u)) {
    h->err = "rplgpu_bin_poses_dev: map_stride >= ceil(nx * ny * T / 32) and even is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_bins_out && bin_stride < P) {
    h->err = "rplgpu_bin_poses_dev: bin_stride >= P is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_poses, "d_poses", true}, {d_edges, "d_edges", true}, {d_map, "d_map", true},
                           {d_result, "d_result", true}, {d_weights, "d_weights", false},
                           {d_bins_out, "d_bins_out", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  rpl::BinsK k;
  k.origin_x = s->origin_x;
  k.origin_y = s->origin_y;
  k.inv_size = s->inv_size;
  k.nx = s->nx;
  k.ny = s->ny;
  k.keep = s->flags & 1u;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_bins(h->stream, k, d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P,
                              d_edges, T, d_map, map_stride, d_bins_out, bin_stride, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_bin_poses(rplgpu_handle_t h, const rplgpu_pose_bins_t *s, const float *poses, uint32_t P,
                         const uint32_t *weights, const float *edges, uint32_t T, uint32_t *map, uint32_t *bins_out,
                         uint32_t result[8]) {
  if (!h || !poses || !edges || !map || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_bins_check(s, T) != RPLGPU_OK) {
    h->err = "rplgpu_bin_poses: the rplgpu_pose_bins_t is missing or rplgpu_pose_bins_check refuses it or T";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_bin_poses"}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  // result | edges | map | weights | bins | poses
  const size_t words = rpl::bin_map_words(s->nx * s->ny * T), stride = (size_t)rplgpu_bin_map_words(s->nx, s->ny, T);
  DoorBuffer buf(h, "rplgpu_bin_poses");
  const size_t o_res = buf.part(32), o_edge = buf.part(8u * (size_t)T), o_map = buf.part(4u * stride),
               o_wt = buf.part_if(weights, 4u * (size_t)P), o_bins = buf.part_if(bins_out, 4u * (size_t)P),
               o_poses = buf.part(16u * (size_t)P);
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> map_back(words), bins_back(bins_out ? P : 0u);
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_poses), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_edge), edges, 8u * (size_t)T, hipMemcpyHostToDevice, h->stream));
    if (weights) RPL_HIP(h, hipMemcpyAsync(buf.at(o_wt), weights, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (s->flags & 1u) RPL_HIP(h, hipMemcpyAsync(buf.at(o_map), map, 4u * words, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_bin_poses_dev(h, s, buf.at<const float>(o_poses), 4ull * P, 0,
                                             buf.at<const uint32_t>(o_wt), P, 1, P, buf.at<const float>(o_edge), T,
                                             buf.at<uint32_t>(o_map), stride, buf.at<uint32_t>(o_bins), P,
                                             buf.at<uint32_t>(o_res));
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(map_back.data(), buf.at(o_map), 4u * words, hipMemcpyDeviceToHost, h->stream));
    if (bins_out)
      RPL_HIP(h, hipMemcpyAsync(bins_back.data(), buf.at(o_bins), 4u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, buf.at(o_res), 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;  // (no output changed)
  std::memcpy(map, map_back.data(), 4u * words);
  if (bins_out) std::memcpy(bins_out, bins_back.data(), 4u * (size_t)P);
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

// ---- E21: a binned pose list clustered, the heaviest cluster summed (include/rplgpu_msg.h) ----------------------------

uint64_t rplgpu_cluster_scratch_words(uint32_t G, uint32_t P, uint32_t nx, uint32_t ny, uint32_t T) {
  return rpl::clusters_scratch_words(G, P, nx, ny, T);
}

int32_t rplgpu_cluster_poses_dev(rplgpu_handle_t h, const rplgpu_pose_clusters_t *s, const float *d_poses,
                                 uint64_t pose_stride, uint32_t poses_per_group, const uint32_t *d_weights,
                                 uint64_t weight_stride, uint32_t G, uint32_t P, uint32_t T, const uint32_t *d_map,
                                 uint64_t map_stride, const uint32_t *d_bins, uint64_t bin_stride,
                                 uint32_t *d_labels_out, uint64_t label_stride, uint32_t *d_clusters,
                                 uint64_t cluster_stride, uint32_t cluster_cap, uint32_t *d_result,
                                 uint32_t *d_scratch) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_clusters_check(s, T) != RPLGPU_OK) {
    h->err = "rplgpu_cluster_poses_dev: the rplgpu_pose_clusters_t is missing or rplgpu_pose_clusters_check refuses it or T";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const PoseListDoor door{h, "rplgpu_cluster_poses_dev"};
  if (!door.groups(G) || !door.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (!d_poses || !d_map || !d_bins || !d_result || !d_scratch || misaligned(d_poses, 15) || misaligned(d_map, 7) ||
      misaligned(d_scratch, 7) || misaligned(d_weights, 3) || misaligned(d_bins, 3) || misaligned(d_labels_out, 3) ||
      misaligned(d_clusters, 3) || misaligned(d_result, 3)) {
    h->err = "rplgpu_cluster_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for d_poses, "
             "8 for d_map and d_scratch, 4 otherwise)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!door.strides(P, pose_stride, d_weights, weight_stride)) return RPLGPU_ERR_INVALID_ARG;
  const uint64_t words = rpl::bin_map_words(s->nx * s->ny * T);
  if (map_stride < words || (map_stride & 1u)) {
    h->err = "rplgpu_cluster_poses_dev: map_stride >= ceil(nx * ny * T / 32) and even is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const bool table = d_clusters && cluster_cap != 0;
  if (bin_stride < P || (d_labels_out && label_stride < P) || (table && cluster_stride < 4ull * cluster_cap)) {
    h->err = "rplgpu_cluster_poses_dev: bin_stride >= P, label_stride >= P and cluster_stride >= 4 cluster_cap are "
             "required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  // no output may share a byte with an input or with another output
  const uint64_t scratch_words = rplgpu_cluster_scratch_words(G, P, s->nx, s->ny, T);
  const Range ranges[] = {
      {d_poses, 4ull * ((poses_per_group ? (uint64_t)(G - 1u) * pose_stride : 0ull) + 4ull * P), false},
      {d_weights, d_weights ? 4ull * ((uint64_t)(G - 1u) * weight_stride + P) : 0ull, false},
      {d_map, 4ull * ((uint64_t)(G - 1u) * map_stride + words), false},
      {d_bins, 4ull * ((uint64_t)(G - 1u) * bin_stride + P), false},
      {d_labels_out, d_labels_out ? 4ull * ((uint64_t)(G - 1u) * label_stride + P) : 0ull, true},
      {d_clusters, table ? 4ull * ((uint64_t)(G - 1u) * cluster_stride + 4ull * cluster_cap) : 0ull, true},
      {d_result, 4ull * RPLGPU_CLUSTER_WORDS * G, true},
      {d_scratch, 4ull * scratch_words, true}};
  if (ranges_clash(ranges)) {
    h->err = "rplgpu_cluster_poses_dev: an output overlaps an input or another output";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_poses, "d_poses", true}, {d_map, "d_map", true}, {d_bins, "d_bins", true},
                           {d_result, "d_result", true}, {d_scratch, "d_scratch", true},
                           {d_weights, "d_weights", false}, {d_labels_out, "d_labels_out", false},
                           {d_clusters, "d_clusters", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  const rpl::ClustersK k{s->nx, s->ny, s->xy_scale, s->flags & 1u};
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_clusters(h->stream, k, d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P,
                                  T, d_map, map_stride, d_bins, bin_stride, d_labels_out, label_stride,
                                  table ? d_clusters : nullptr, cluster_stride, table ? cluster_cap : 0u, d_result,
                                  d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_cluster_poses(rplgpu_handle_t h, const rplgpu_pose_clusters_t *s, const float *poses, uint32_t P,
                             const uint32_t *weights, uint32_t T, const uint32_t *map, const uint32_t *bins,
                             uint32_t *labels_out, uint32_t *clusters_out, uint32_t cluster_cap,
                             uint32_t result[80]) {
  if (!h || !poses || !map || !bins || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_clusters_check(s, T) != RPLGPU_OK) {
    h->err = "rplgpu_cluster_poses: the rplgpu_pose_clusters_t is missing or rplgpu_pose_clusters_check refuses it or T";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_cluster_poses"}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  // result | map | weights | bins | labels | table | scratch | poses
  const size_t words = rpl::bin_map_words(s->nx * s->ny * T), stride = (size_t)rplgpu_bin_map_words(s->nx, s->ny, T);
  const bool table = clusters_out && cluster_cap != 0;
  DoorBuffer buf(h, "rplgpu_cluster_poses");
  const size_t o_res = buf.part(4u * RPLGPU_CLUSTER_WORDS), o_map = buf.part(4u * stride),
               o_wt = buf.part_if(weights, 4u * (size_t)P), o_bins = buf.part(4u * (size_t)P),
               o_lab = buf.part_if(labels_out, 4u * (size_t)P), o_tab = buf.part_if(table, 16u * (size_t)cluster_cap),
               o_scr = buf.part(4u * (size_t)rplgpu_cluster_scratch_words(1, P, s->nx, s->ny, T)),
               o_poses = buf.part(16u * (size_t)P);
  uint32_t small[RPLGPU_CLUSTER_WORDS];
  std::vector<uint32_t> lab_back(labels_out ? P : 0u), tab_back(table ? 4u * (size_t)cluster_cap : 0u);
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_poses), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_map), map, 4u * words, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_bins), bins, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (weights) RPL_HIP(h, hipMemcpyAsync(buf.at(o_wt), weights, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (table)  // the rows beyond N_c keep what the caller has there
      RPL_HIP(h, hipMemcpyAsync(buf.at(o_tab), clusters_out, 16u * (size_t)cluster_cap, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_cluster_poses_dev(
        h, s, buf.at<const float>(o_poses), 4ull * P, 0, buf.at<const uint32_t>(o_wt), P, 1, P, T,
        buf.at<const uint32_t>(o_map), stride, buf.at<const uint32_t>(o_bins), P, buf.at<uint32_t>(o_lab), P,
        buf.at<uint32_t>(o_tab), 4ull * cluster_cap, table ? cluster_cap : 0u, buf.at<uint32_t>(o_res),
        buf.at<uint32_t>(o_scr));
    if (irc) return irc;
    if (labels_out)
      RPL_HIP(h, hipMemcpyAsync(lab_back.data(), buf.at(o_lab), 4u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    if (table)
      RPL_HIP(h, hipMemcpyAsync(tab_back.data(), buf.at(o_tab), 16u * (size_t)cluster_cap, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, buf.at(o_res), sizeof(small), hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;  // (no output changed)
  if (labels_out) std::memcpy(labels_out, lab_back.data(), 4u * (size_t)P);
  if (table) std::memcpy(clusters_out, tab_back.data(), 16u * (size_t)cluster_cap);
  std::memcpy(result, small, sizeof(small));
  return RPLGPU_OK;
}

// ---- E22: a beam fan cast from every pose of a list into a grid (include/rplgpu_msg.h) --------------------------------

int32_t rplgpu_cast_beams(const rplgpu_scan_merge_t *m, uint32_t first, uint32_t step, uint32_t A, float *cs) {
  float inc = 0.0f;
  if (!cs || !m || A == 0 || A > RPLGPU_MAX_MERGE_BEAMS || rplgpu_scan_merge_edges(m, nullptr, &inc) != RPLGPU_OK ||
      (uint64_t)first + (uint64_t)(A - 1u) * step >= m->count)
    return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t a = 0; a < A; ++a) {
    const double k = (double)(first + a * step);
    const double phi = (double)m->angle_min + (k + 0.5) * (double)inc;
    cs[2u * a] = (float)std::cos(phi);
    cs[2u * a + 1u] = (float)std::sin(phi);
  }
  return RPLGPU_OK;
}

int32_t rplgpu_cast_ranges_dev(rplgpu_handle_t h, const rplgpu_range_cast_t *s, const float *d_poses,
                               uint64_t pose_stride, uint32_t poses_per_group, uint32_t G, uint32_t P,
                               const float *d_beams, uint32_t A, const int8_t *d_grid, uint64_t grid_stride,
                               uint32_t grid_per_group, const float *d_measured, uint64_t meas_stride,
                               uint32_t meas_first, uint32_t meas_step, const uint8_t *d_table,
                               uint32_t *d_ranges_out, uint64_t range_stride, uint32_t *d_weights,
                               uint64_t weight_stride, uint32_t *d_result, uint32_t *d_cast) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_range_cast_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_cast_ranges_dev: the rplgpu_range_cast_t is missing or rplgpu_range_cast_check refuses it";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_cast_ranges_dev"}.groups(G)) return RPLGPU_ERR_INVALID_ARG;
  if (P == 0 || P > RPLGPU_MAX_POSES || A == 0 || A > RPLGPU_MAX_MERGE_BEAMS ||
      (uint64_t)P * A > RPLGPU_MAX_CAST_RAYS) {
    h->err = "rplgpu_cast_ranges_dev: P must be in 1 .. RPLGPU_MAX_POSES, A in 1 .. RPLGPU_MAX_MERGE_BEAMS and "
             "P * A at most 2^28";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_ranges_out && !d_measured) {
    h->err = "rplgpu_cast_ranges_dev: at least one of d_ranges_out and d_measured is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_poses || !d_beams || !d_grid || !d_cast || (d_measured && (!d_table || !d_weights || !d_result)) ||
      misaligned(d_poses, 15) || misaligned(d_beams, 7) || misaligned(d_grid, 3) || misaligned(d_measured, 3) ||
      misaligned(d_ranges_out, 3) || misaligned(d_cast, 3) ||
      (d_measured && (misaligned(d_weights, 3) || misaligned(d_result, 3)))) {
    h->err = "rplgpu_cast_ranges_dev: a required pointer is missing (d_table, d_weights and d_result with d_measured) "
             "or a pointer is misaligned (16 bytes for d_poses, 8 for d_beams, 4 for d_grid, d_measured, "
             "d_ranges_out, d_weights, d_result and d_cast)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (pose_stride < 4ull * P || (pose_stride & 3u)) {
    h->err = "rplgpu_cast_ranges_dev: pose_stride >= 4 P and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (grid_stride < (uint64_t)s->width * s->height || (grid_stride & 3u)) {
    h->err = "rplgpu_cast_ranges_dev: grid_stride >= width * height and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_ranges_out && range_stride < (uint64_t)P * A) {
    h->err = "rplgpu_cast_ranges_dev: range_stride >= P * A is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_measured &&
      (weight_stride < P || (uint64_t)meas_first + (uint64_t)(A - 1u) * meas_step >= meas_stride)) {
    h->err = "rplgpu_cast_ranges_dev: weight_stride >= P and meas_first + (A - 1) * meas_step < meas_stride are "
             "required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_poses, "d_poses", true}, {d_beams, "d_beams", true}, {d_grid, "d_grid", true},
                           {d_cast, "d_cast", true}, {d_measured, "d_measured", false},
                           {d_ranges_out, "d_ranges_out", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  if (d_measured && !device_readable(h, {{d_table, "d_table", true}, {d_weights, "d_weights", true},
                                         {d_result, "d_result", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  rpl::CastK k;
  k.origin_x = s->origin_x;
  k.origin_y = s->origin_y;
  k.resolution = s->resolution;
  k.width = s->width;
  k.height = s->height;
  k.max_steps = s->max_steps;
  k.hit_lo = s->hit_lo;
  k.unknown_stops = s->unknown_stops;
  k.table_half = s->table_half;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_cast(h->stream, k, d_poses, pose_stride, poses_per_group, G, P, d_beams, A, d_grid,
                              grid_stride, grid_per_group, d_measured, meas_stride, meas_first, meas_step,
                              d_measured ? d_table : nullptr, d_ranges_out, range_stride,
                              d_measured ? d_weights : nullptr, weight_stride, d_measured ? d_result : nullptr,
                              d_cast));
  return RPLGPU_OK;
}

int32_t rplgpu_cast_ranges(rplgpu_handle_t h, const rplgpu_range_cast_t *s, const float *poses, uint32_t P,
                           const float *beams, uint32_t A, const int8_t *grid, const float *measured,
                           uint32_t meas_count, uint32_t meas_first, uint32_t meas_step, const uint8_t *table,
                           uint32_t *ranges_out, uint32_t *weights_out, uint32_t result[8], uint32_t cast[8]) {
  if (!h || !poses || !beams || !grid || !cast) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_range_cast_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_cast_ranges: the rplgpu_range_cast_t is missing or rplgpu_range_cast_check refuses it";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES || A == 0 || A > RPLGPU_MAX_MERGE_BEAMS ||
      (uint64_t)P * A > RPLGPU_MAX_CAST_RAYS) {
    h->err = "rplgpu_cast_ranges: P must be in 1 .. RPLGPU_MAX_POSES, A in 1 .. RPLGPU_MAX_MERGE_BEAMS and P * A at "
             "most 2^28";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((!ranges_out && !measured) || (measured && (!table || !weights_out || !result || meas_count == 0))) {
    h->err = "rplgpu_cast_ranges: ranges_out or measured is required, and table, weights_out and result with measured";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // result | cast | beams | table | measured | grid | weights | ranges | poses
  const size_t cells = (size_t)s->width * s->height, gstride = (cells + 3u) & ~(size_t)3u;
  const size_t rays = (size_t)P * A, tbytes = 2u * (size_t)s->table_half + 2u;
  DoorBuffer buf(h, "rplgpu_cast_ranges");
  const size_t o_res = buf.part(32), o_cast = buf.part(32), o_beams = buf.part(8u * (size_t)A),
               o_tab = buf.part_if(measured, tbytes), o_meas = buf.part_if(measured, 4u * (size_t)meas_count),
               o_grid = buf.part(gstride), o_wt = buf.part_if(measured, 4u * (size_t)P),
               o_rng = buf.part_if(ranges_out, 4u * rays), o_poses = buf.part(16u * (size_t)P);
  uint32_t small[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> wt_back(measured ? P : 0u);
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemsetAsync(buf.at(o_grid), 0, up16(gstride), h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_poses), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_beams), beams, 8u * (size_t)A, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_grid), grid, cells, hipMemcpyHostToDevice, h->stream));
    if (measured) {
      RPL_HIP(h, hipMemcpyAsync(buf.at(o_tab), table, tbytes, hipMemcpyHostToDevice, h->stream));
      RPL_HIP(h, hipMemcpyAsync(buf.at(o_meas), measured, 4u * (size_t)meas_count, hipMemcpyHostToDevice, h->stream));
    }
    const int32_t irc = rplgpu_cast_ranges_dev(
        h, s, buf.at<const float>(o_poses), 4ull * P, 0, 1, P, buf.at<const float>(o_beams), A,
        buf.at<const int8_t>(o_grid), gstride, 0, buf.at<const float>(o_meas), meas_count, meas_first, meas_step,
        buf.at<const uint8_t>(o_tab), buf.at<uint32_t>(o_rng), rays, buf.at<uint32_t>(o_wt), P,
        measured ? buf.at<uint32_t>(o_res) : nullptr, buf.at<uint32_t>(o_cast));
    if (irc) return irc;
    // (the range words may be a gigabyte: straight into the caller's buffer, which a refused call never reaches)
    if (ranges_out)
      RPL_HIP(h, hipMemcpyAsync(ranges_out, buf.at(o_rng), 4u * rays, hipMemcpyDeviceToHost, h->stream));
    if (measured)
      RPL_HIP(h, hipMemcpyAsync(wt_back.data(), buf.at(o_wt), 4u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, buf.at(o_res), 64, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  if (measured) {
    std::memcpy(weights_out, wt_back.data(), 4u * (size_t)P);
    std::memcpy(result, small, 32);
  }
  std::memcpy(cast, small + 8, 32);
  return RPLGPU_OK;
}

// ---- E23: the beams a pose list disagrees with are left out of the weights (include/rplgpu_msg.h) -------------------

// d_t0: as pose_impl
static int32_t agree_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                          const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                          const float *d_motion, const float *d_pose2d, const float *d_t0,
                          const rplgpu_beam_agree_t *s, const float *d_poses, uint32_t P, uint64_t pose_stride,
                          uint32_t poses_per_group, const int8_t *d_field, uint64_t field_stride,
                          uint32_t field_per_group, uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_result,
                          uint32_t *d_status, uint32_t *d_counts, uint64_t count_stride, uint32_t *d_mask,
                          uint64_t mask_stride, uint32_t *d_agree) {
  const char *fn = "rplgpu_score_poses_agree_dev";
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !s) return RPLGPU_ERR_INVALID_ARG;
  if ((rc = score_args_check(h, fn, "rplgpu_beam_agree_t", rplgpu_beam_agree_check(s) == RPLGPU_OK,
                             (uint64_t)s->width * s->height, group, d_poses, P, pose_stride, d_field, field_stride,
                             d_weights, weight_stride, d_result, d_status)))
    return rc;
  if (!d_counts || !d_mask || !d_agree || misaligned(d_counts, 3) || misaligned(d_mask, 3) || misaligned(d_agree, 3)) {
    h->err = std::string(fn) + ": d_counts, d_mask and d_agree are required and 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (count_stride < n_stride || mask_stride < (n_stride + 31u) / 32u) {
    h->err = std::string(fn) + ": count_stride must be >= n_stride and mask_stride >= ceil(n_stride / 32)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_poses, "d_poses", true},
                           {d_field, "d_field", true}, {d_weights, "d_weights", true}, {d_result, "d_result", true},
                           {d_status, "d_status", false}, {d_counts, "d_counts", true}, {d_mask, "d_mask", true},
                           {d_agree, "d_agree", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  ScanPrologue pro;
  if ((rc = pro.admit(h, fn, p, d_motion, d_t0, B, group))) return rc;
  if ((uint64_t)pro.group * n_stride > (1ull << 24)) {  // 127 x points stays below 2^32: no weight wraps
    h->err = std::string(fn) + ": group x n_stride above 2^24 samples";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((uint64_t)pro.G * ((P + 255u) / 256u) > 0x7FFFFFFFull) {  // (E15's limit, kept: the calls take the same lists)
    h->err = std::string(fn) + ": groups x P too large for one call";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const rpl::AgreeK k{s->origin_x, s->origin_y, s->resolution, s->width,   s->height,
                      (uint32_t)s->agree_lo, s->keep_num, s->keep_den,   s->err_num, s->err_den};
  if ((rc = pro.begin(h, d_nodes, n_stride, d_n_per_scan, B, p, d_t0, d_status))) return rc;
  RPL_HIP(h, rpl::launch_agree(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.G, pro.kp, pro.T, pro.mask,
                               kMaskStride, d_motion, d_pose2d, k, d_poses, P, pose_stride, poses_per_group, d_field,
                               field_stride, field_per_group, d_weights, weight_stride, d_result, d_status, d_counts,
                               count_stride, d_mask, mask_stride, d_agree));
  RPL_HIP(h, rpl::launch_pose_best(h->stream, d_weights, weight_stride, pro.G, P, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_score_poses_agree_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                     const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                                     const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                                     const rplgpu_beam_agree_t *s, const float *d_poses, uint32_t P,
                                     uint64_t pose_stride, uint32_t poses_per_group, const int8_t *d_field,
                                     uint64_t field_stride, uint32_t field_per_group, uint32_t *d_weights,
                                     uint64_t weight_stride, uint32_t *d_result, uint32_t *d_status,
                                     uint32_t *d_counts, uint64_t count_stride, uint32_t *d_mask,
                                     uint64_t mask_stride, uint32_t *d_agree) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return agree_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, s, d_poses, P,
                    pose_stride, poses_per_group, d_field, field_stride, field_per_group, d_weights, weight_stride,
                    d_result, d_status, d_counts, count_stride, d_mask, mask_stride, d_agree);
}

int32_t rplgpu_score_poses_agree(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                                 const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                                 const float *motion, const float *pose2d, const float *t0,
                                 const rplgpu_beam_agree_t *s, const float *poses, uint32_t P, const int8_t *field,
                                 uint32_t *weights_out, uint32_t result[8], uint32_t *status, uint32_t *counts_out,
                                 uint32_t *mask_out, uint32_t agree[8]) {
  if (!h || !nodes || !n_per_scan || !p || !s || !poses || !field || !result || !agree || n_scans == 0 ||
      n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_beam_agree_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_score_poses_agree: invalid rplgpu_beam_agree_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_score_poses_agree"}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)s->width * s->height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t mask_words = (n_stride + 31u) / 32u;
  const size_t cnt_bytes = 4u * (size_t)n_scans * n_stride, mask_bytes = 4u * (size_t)n_scans * mask_words;
  // field | poses | weights | counts | mask | the scans | result + agree + status
  DoorBuffer buf(h, "rplgpu_score_poses_agree");
  const size_t o_field = buf.part(stride), o_ps = buf.part(16u * (size_t)P), o_wt = buf.part(4u * (size_t)P),
               o_cnt = buf.part(cnt_bytes), o_mask = buf.part(mask_bytes);
  DoorScans scans(buf, nodes, n_stride, n_per_scan, n_scans, motion, pose2d, t0);
  const size_t o_small = buf.part(80);
  uint32_t small[17] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_field), field, cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_ps), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (int32_t urc = scans.upload(h, buf)) return urc;
    uint32_t *d_small = buf.at<uint32_t>(o_small);  // result, agree, status
    const int32_t irc = agree_impl(h, scans.d_nodes, n_stride, scans.d_n_per_scan, n_scans, n_scans, p, scans.d_motion,
                                   scans.d_pose2d, scans.d_t0, s, buf.at<const float>(o_ps), P, 4ull * P, 0,
                                   buf.at<const int8_t>(o_field), stride, 0, buf.at<uint32_t>(o_wt), P, d_small,
                                   d_small + 16, buf.at<uint32_t>(o_cnt), n_stride, buf.at<uint32_t>(o_mask),
                                   mask_words, d_small + 8);
    if (irc) return irc;
    if (weights_out)
      RPL_HIP(h, hipMemcpyAsync(weights_out, buf.at(o_wt), 4u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    if (counts_out) RPL_HIP(h, hipMemcpyAsync(counts_out, buf.at(o_cnt), cnt_bytes, hipMemcpyDeviceToHost, h->stream));
    if (mask_out) RPL_HIP(h, hipMemcpyAsync(mask_out, buf.at(o_mask), mask_bytes, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 68, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, small, 32);
  std::memcpy(agree, small + 8, 32);
  if (status) *status = small[16];
  return RPLGPU_OK;
}

}  // extern "C"
