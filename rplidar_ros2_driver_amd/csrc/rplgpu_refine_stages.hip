// rplgpu_refine_stages.hip — the extern "C" entry points of E25, poses refined below a cell (include/rplgpu_msg.h):
// rplgpu_refine_sums_dev, rplgpu_refine_step_dev, rplgpu_refine_poses_dev, the host-buffer door rplgpu_refine_poses and
// the two joints rplgpu_match_poses_dev and rplgpu_compose_poses_dev.
//
// Host side only: argument checks, the launches and the door; the kernels are in rpl_refine.hip, the spec's rules and
// the host twins in rplgpu_refine_rules.cpp.  The handle, the scan-stage prologue and the doors' per-call buffer come
// from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_refine.hpp"

using namespace rpl::host;

namespace {

rpl::RefineK refine_k(const rplgpu_pose_refine_t *r) {
  return rpl::RefineK{r->origin_x, r->origin_y, r->resolution, r->width,   r->height,
                      r->target,   r->damping,  r->max_step_cells, r->max_rot, r->min_points};
}

// what the sums take, in E15's order behind check_batch
int32_t sums_args_check(rplgpu_handle_t h, const char *fn, const rplgpu_pose_refine_t *r, uint32_t group,
                        const float *d_poses, uint32_t P, uint64_t pose_stride, const int8_t *d_field,
                        uint64_t field_stride, const uint32_t *d_sums, uint64_t sums_stride, const uint32_t *d_scratch,
                        const uint32_t *d_result, const uint32_t *d_status) {
  const std::string at = std::string(fn) + ": ";
  if (!d_poses || !d_field || !d_sums || !d_scratch || !d_result || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_refine_check(r) != RPLGPU_OK) {
    h->err = at + "invalid rplgpu_pose_refine_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, fn}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (pose_stride < 4ull * P || (pose_stride & 3u) || misaligned(d_poses, 15u)) {
    h->err = at + "pose_stride must be >= 4 P floats and a multiple of 4, d_poses 16-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (field_stride < (uint64_t)r->width * r->height || (field_stride & 3u) || misaligned(d_field, 3u)) {
    h->err = at + "field_stride must be >= width * height and a multiple of 4, d_field 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (sums_stride < 32ull * P || (sums_stride & 3u) || misaligned(d_sums, 15u) || misaligned(d_scratch, 7u) ||
      misaligned(d_result, 3u) || misaligned(d_status, 3u)) {
    h->err = at + "sums_stride must be >= 32 P words and a multiple of 4, d_sums 16-byte, d_scratch 8-byte, d_result / "
                  "d_status 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  return RPLGPU_OK;
}

// what the step takes; G: the number of groups
int32_t step_args_check(rplgpu_handle_t h, const char *fn, const rplgpu_pose_refine_t *r, const uint32_t *d_sums,
                        uint64_t sums_stride, const float *d_poses, uint64_t pose_stride, uint32_t poses_per_group,
                        uint32_t G, uint32_t P, const float *d_poses_out, uint64_t out_stride, const uint32_t *d_step,
                        uint64_t step_stride, const uint32_t *d_result) {
  const std::string at = std::string(fn) + ": ";
  if (!d_sums || !d_poses || !d_poses_out || !d_result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_refine_check(r) != RPLGPU_OK) {
    h->err = at + "invalid rplgpu_pose_refine_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const PoseListDoor door{h, fn};
  if (!door.groups(G) || !door.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (pose_stride < 4ull * P || (pose_stride & 3u) || out_stride < 4ull * P || (out_stride & 3u) ||
      sums_stride < 32ull * P || (sums_stride & 3u) || (d_step && (step_stride < 4ull * P || (step_stride & 3u)))) {
    h->err = at + "pose_stride, out_stride and step_stride must be >= 4 P, sums_stride >= 32 P, all multiples of 4";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (misaligned(d_sums, 15u) || misaligned(d_poses, 15u) || misaligned(d_poses_out, 15u) || misaligned(d_step, 15u) ||
      misaligned(d_result, 3u)) {
    h->err = at + "d_sums, d_poses, d_poses_out and d_step must be 16-byte, d_result 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t in_bytes = 4u * ((uint64_t)(poses_per_group ? G - 1u : 0u) * pose_stride + 4ull * P);
  const uint64_t out_bytes = 4u * ((uint64_t)(G - 1u) * out_stride + 4ull * P);
  const bool in_place = d_poses_out == d_poses && out_stride == pose_stride && (poses_per_group || G == 1u);
  if (!in_place && rpl::ranges_overlap(d_poses, in_bytes, d_poses_out, out_bytes)) {
    h->err = at + "d_poses_out overlaps d_poses (allowed only in place: equal pointers and strides, every group its own list)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  return RPLGPU_OK;
}

// iters = 0: the sums alone (rplgpu_refine_sums_dev).  d_t0: the per-scan time offsets of E6 for this call, or NULL
int32_t refine_impl(rplgpu_handle_t h, const char *fn, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                    const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                    const float *d_motion, const float *d_pose2d, const float *d_t0, const rplgpu_pose_refine_t *r,
                    const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                    const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group, uint32_t iters,
                    float *d_poses_out, uint64_t out_stride, uint32_t *d_sums, uint64_t sums_stride, uint32_t *d_step,
                    uint64_t step_stride, uint32_t *d_scratch, uint32_t *d_result, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !r) return RPLGPU_ERR_INVALID_ARG;
  if ((rc = sums_args_check(h, fn, r, group, d_poses, P, pose_stride, d_field, field_stride, d_sums, sums_stride,
                            d_scratch, d_result, d_status)))
    return rc;
  if (B == 0) return RPLGPU_OK;
  ScanPrologue pro;
  if ((rc = pro.admit(h, fn, p, d_motion, d_t0, B, group))) return rc;
  if (iters && (rc = step_args_check(h, fn, r, d_sums, sums_stride, d_poses, pose_stride, poses_per_group, pro.G, P,
                                     d_poses_out, out_stride, d_step, step_stride, d_result)))
    return rc;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_poses, "d_poses", true},
                           {d_field, "d_field", true}, {d_sums, "d_sums", true}, {d_scratch, "d_scratch", true},
                           {d_result, "d_result", true}, {d_status, "d_status", false},
                           {d_poses_out, "d_poses_out", iters != 0}, {d_step, "d_step", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  const std::string at = std::string(fn) + ": ";
  if ((uint64_t)pro.group * n_stride > (1ull << 24)) {  // the bounds of the header's table
    h->err = at + "group x n_stride above 2^24 samples";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (pro.G > 65535u) {  // (the groups are the second dimension of the per-pose grids)
    h->err = at + "more than 65535 groups";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const rpl::RefineK k = refine_k(r);
  if ((rc = pro.begin(h, d_nodes, n_stride, d_n_per_scan, B, p, d_t0, d_status))) return rc;
  const uint32_t rounds = std::max(iters, 1u);
  for (uint32_t it = 0; it < rounds; ++it) {
    // round 0 reads the caller's list, every later round the list the round before left: every group its own
    const float *list = it ? d_poses_out : d_poses;
    const uint64_t stride = it ? out_stride : pose_stride;
    const uint32_t per_group = it ? 1u : poses_per_group;
    RPL_HIP(h, rpl::launch_refine_prepare(h->stream, pro.G, P, d_scratch, d_result));
    RPL_HIP(h, rpl::launch_refine_sums(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T,
                                       pro.mask, kMaskStride, d_motion, d_pose2d, k, list, P, stride, per_group,
                                       d_field, field_stride, field_per_group, d_scratch, d_result, d_status));
    RPL_HIP(h, rpl::launch_refine_finish(h->stream, pro.G, P, d_scratch, d_sums, sums_stride, d_result));
    if (iters)
      RPL_HIP(h, rpl::launch_refine_step(h->stream, d_sums, sums_stride, k, list, stride, per_group, pro.G, P,
                                         d_poses_out, out_stride, d_step, step_stride, d_result, false));
  }
  return RPLGPU_OK;
}

}  // namespace

extern "C" {

int32_t rplgpu_refine_sums_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const rplgpu_pose_refine_t *r,
                               const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                               const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group,
                               uint32_t *d_sums, uint64_t sums_stride, uint32_t *d_scratch, uint32_t *d_result,
                               uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return refine_impl(h, "rplgpu_refine_sums_dev", d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d,
                     h->scan_t0, r, d_poses, P, pose_stride, poses_per_group, d_field, field_stride, field_per_group,
                     0, nullptr, 0, d_sums, sums_stride, nullptr, 0, d_scratch, d_result, d_status);
}

int32_t rplgpu_refine_step_dev(rplgpu_handle_t h, const uint32_t *d_sums, uint64_t sums_stride,
                               const rplgpu_pose_refine_t *r, const float *d_poses, uint64_t pose_stride,
                               uint32_t poses_per_group, uint32_t G, uint32_t P, float *d_poses_out,
                               uint64_t out_stride, uint32_t *d_step, uint64_t step_stride, uint32_t *d_result) {
  if (!h || !r) return RPLGPU_ERR_INVALID_ARG;
  if (int32_t rc = step_args_check(h, "rplgpu_refine_step_dev", r, d_sums, sums_stride, d_poses, pose_stride,
                                   poses_per_group, G, P, d_poses_out, out_stride, d_step, step_stride, d_result))
    return rc;
  if (!device_readable(h, {{d_sums, "d_sums", true}, {d_poses, "d_poses", true}, {d_poses_out, "d_poses_out", true},
                           {d_step, "d_step", false}, {d_result, "d_result", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_refine_step(h->stream, d_sums, sums_stride, refine_k(r), d_poses, pose_stride,
                                     poses_per_group, G, P, d_poses_out, out_stride, d_step, step_stride, d_result,
                                     true));
  return RPLGPU_OK;
}

int32_t rplgpu_refine_poses_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                                const float *d_motion, const float *d_pose2d, const rplgpu_pose_refine_t *r,
                                const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                                const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group,
                                uint32_t iters, float *d_poses_out, uint64_t out_stride, uint32_t *d_sums,
                                uint64_t sums_stride, uint32_t *d_step, uint64_t step_stride, uint32_t *d_scratch,
                                uint32_t *d_result, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (iters == 0 || iters > RPLGPU_REFINE_MAX_ITERS) {
    h->err = "rplgpu_refine_poses_dev: iters must be in 1 .. RPLGPU_REFINE_MAX_ITERS";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_poses_out) return RPLGPU_ERR_INVALID_ARG;
  return refine_impl(h, "rplgpu_refine_poses_dev", d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d,
                     h->scan_t0, r, d_poses, P, pose_stride, poses_per_group, d_field, field_stride, field_per_group,
                     iters, d_poses_out, out_stride, d_sums, sums_stride, d_step, step_stride, d_scratch, d_result,
                     d_status);
}

int32_t rplgpu_refine_poses(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                            const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                            const float *motion, const float *pose2d, const float *t0,
                            const rplgpu_pose_refine_t *r, const float *poses, uint32_t P, const int8_t *field,
                            uint32_t iters, float *poses_out, uint32_t *sums_out, uint32_t *step_out,
                            uint32_t result[8], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !r || !poses || !field || !poses_out || !result || n_scans == 0 ||
      n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_refine_check(r) != RPLGPU_OK) {
    h->err = "rplgpu_refine_poses: invalid rplgpu_pose_refine_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_refine_poses"}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (iters == 0 || iters > RPLGPU_REFINE_MAX_ITERS) {
    h->err = "rplgpu_refine_poses: iters must be in 1 .. RPLGPU_REFINE_MAX_ITERS";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)r->width * r->height, stride = (cells_n + 3u) & ~(size_t)3u;
  // field | poses | poses out | sums | step | scratch | the scans | result + status
  DoorBuffer buf(h, "rplgpu_refine_poses");
  const size_t o_field = buf.part(stride), o_ps = buf.part(16u * (size_t)P), o_po = buf.part(16u * (size_t)P);
  const size_t o_sums = buf.part(128u * (size_t)P), o_step = buf.part(16u * (size_t)P);
  const size_t o_scr = buf.part(4u * (size_t)rplgpu_refine_scratch_words(1, P));
  DoorScans scans(buf, nodes, n_stride, n_per_scan, n_scans, motion, pose2d, t0);
  const size_t o_small = buf.part(48);
  uint32_t small[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_field), field, cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_ps), poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (int32_t urc = scans.upload(h, buf)) return urc;
    uint32_t *d_small = buf.at<uint32_t>(o_small);
    const int32_t irc =
        refine_impl(h, "rplgpu_refine_poses", scans.d_nodes, n_stride, scans.d_n_per_scan, n_scans, n_scans, p,
                    scans.d_motion, scans.d_pose2d, scans.d_t0, r, buf.at<const float>(o_ps), P, 4ull * P, 0,
                    buf.at<const int8_t>(o_field), stride, 0, iters, buf.at<float>(o_po), 4ull * P,
                    buf.at<uint32_t>(o_sums), 32ull * P, buf.at<uint32_t>(o_step), 4ull * P, buf.at<uint32_t>(o_scr),
                    d_small, d_small + 8);
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(poses_out, buf.at(o_po), 16u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    if (sums_out)
      RPL_HIP(h, hipMemcpyAsync(sums_out, buf.at(o_sums), 128u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    if (step_out)
      RPL_HIP(h, hipMemcpyAsync(step_out, buf.at(o_step), 16u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 36, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(result, small, 32);
  if (status) *status = small[8];
  return RPLGPU_OK;
}

int32_t rplgpu_match_poses_dev(rplgpu_handle_t h, const uint32_t *d_best, const rplgpu_scan_match_t *m,
                               const float *d_pivot, const float *d_prior, uint32_t G, float *d_poses_out,
                               uint64_t out_stride) {
  if (!h || !d_best || !m || !d_poses_out) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_match_poses_dev: invalid rplgpu_scan_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!PoseListDoor{h, "rplgpu_match_poses_dev"}.groups(G)) return RPLGPU_ERR_INVALID_ARG;
  if (misaligned(d_best, 3u) || misaligned(d_pivot, 3u) || misaligned(d_prior, 15u) || misaligned(d_poses_out, 15u) ||
      out_stride < 4u || (out_stride & 3u)) {
    h->err = "rplgpu_match_poses_dev: d_best / d_pivot 4-byte, d_prior / d_poses_out 16-byte aligned, out_stride >= 4 "
             "and a multiple of 4 are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_best, "d_best", true}, {d_pivot, "d_pivot", false}, {d_prior, "d_prior", false},
                           {d_poses_out, "d_poses_out", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  const rpl::MatchK k{m->origin_x, m->origin_y, m->resolution, m->width, m->height,
                      m->shift_x,  m->shift_y,  m->rot_steps};
  rpl::MatchRot rot;  // by value, as k_apply_match takes it
  std::memset(&rot, 0, sizeof(rot));
  if (rplgpu_scan_match_rotations(m, rot.cs) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_match_poses(h->stream, d_best, k, rot, d_pivot, d_prior, G, d_poses_out, out_stride));
  return RPLGPU_OK;
}

int32_t rplgpu_compose_poses_dev(rplgpu_handle_t h, const float *d_poses, uint64_t pose_stride,
                                 uint32_t poses_per_group, uint32_t P, const uint32_t *d_result, uint32_t q,
                                 const float *d_pose2d_in, uint32_t B, uint32_t group, float *d_pose2d_out) {
  if (!h || !d_poses || !d_pose2d_out || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (!PoseListDoor{h, "rplgpu_compose_poses_dev"}.poses(P)) return RPLGPU_ERR_INVALID_ARG;
  if (pose_stride < 4ull * P || (pose_stride & 3u) || misaligned(d_poses, 15u) || misaligned(d_result, 3u) ||
      misaligned(d_pose2d_in, 3u) || misaligned(d_pose2d_out, 3u)) {
    h->err = "rplgpu_compose_poses_dev: pose_stride must be >= 4 P floats and a multiple of 4, d_poses 16-byte, the "
             "other pointers 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B > h->max_b) {
    h->err = "batch larger than max_batch given to rplgpu_create";
    return RPLGPU_ERR_CAPACITY;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_poses, "d_poses", true}, {d_result, "d_result", false},
                           {d_pose2d_in, "d_pose2d_in", false}, {d_pose2d_out, "d_pose2d_out", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_compose_poses(h->stream, d_poses, pose_stride, poses_per_group, P, d_result, q, d_pose2d_in, B,
                                       std::min(group, B), d_pose2d_out));
  return RPLGPU_OK;
}

}  // extern "C"
