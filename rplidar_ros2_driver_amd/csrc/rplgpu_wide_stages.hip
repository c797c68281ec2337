// rplgpu_wide_stages.hip — the extern "C" entry points of E24, the wide-window scan matcher (include/rplgpu_msg.h):
// rplgpu_pool_field_dev, rplgpu_match_wide_dev and the host-buffer door rplgpu_match_wide.
//
// Host side only: argument checks, the launches and the door; the kernels are in rpl_wide.hip, the spec's rules in
// rplgpu_wide_rules.cpp.  The handle, the scan-stage prologue and the doors' per-call buffer come from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_wide.hpp"

using namespace rpl::host;

namespace {

rpl::WideK wide_k(const rplgpu_wide_match_t *m) {
  const uint32_t s = RPLGPU_WIDE_MATCH_BLOCK;
  rpl::WideK wk;
  wk.k = rpl::MatchK{m->origin_x, m->origin_y, m->resolution, m->width, m->height,
                     m->shift_x,  m->shift_y,  m->rot_steps};
  wk.nbx = (2u * m->shift_x + s) / s;
  wk.nby = (2u * m->shift_y + s) / s;
  wk.max_blocks = m->max_blocks;
  return wk;
}

uint64_t pooled_cells(const rplgpu_wide_match_t *m) {
  return (uint64_t)(m->width + RPLGPU_WIDE_MATCH_BLOCK - 1u) * (m->height + RPLGPU_WIDE_MATCH_BLOCK - 1u);
}

int32_t pool_impl(rplgpu_handle_t h, const rplgpu_wide_match_t *m, const int8_t *d_field, uint64_t field_stride,
                  uint32_t F, int8_t *d_pooled, uint64_t pooled_stride) {
  if (!m || !d_field || !d_pooled) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_wide_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_pool_field_dev: invalid rplgpu_wide_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (field_stride < (uint64_t)m->width * m->height || (field_stride & 3u) || misaligned(d_field, 3u)) {
    h->err = "rplgpu_pool_field_dev: field_stride must be >= width * height and a multiple of 4, d_field 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (pooled_stride < pooled_cells(m) || (pooled_stride & 3u) || misaligned(d_pooled, 3u)) {
    h->err = "rplgpu_pool_field_dev: pooled_stride must be >= (width + 7) * (height + 7) and a multiple of 4, d_pooled 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (F > 65535u) {
    h->err = "rplgpu_pool_field_dev: F above 65535";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (F == 0) return RPLGPU_OK;
  if (rpl::ranges_overlap(d_field, (uint64_t)(F - 1u) * field_stride + (uint64_t)m->width * m->height, d_pooled,
                          (uint64_t)(F - 1u) * pooled_stride + pooled_cells(m))) {
    h->err = "rplgpu_pool_field_dev: d_pooled overlaps d_field";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_field, "d_field", true}, {d_pooled, "d_pooled", true}})) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_pool_field(h->stream, d_field, field_stride, F, m->width, m->height, d_pooled, pooled_stride));
  return RPLGPU_OK;
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
int32_t wide_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride, const uint32_t *d_n_per_scan,
                  uint32_t B, uint32_t group, const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                  const float *d_t0, const float *d_pivot, const rplgpu_wide_match_t *m, const int8_t *d_field,
                  uint64_t field_stride, uint32_t field_per_group, const int8_t *d_pooled, uint64_t pooled_stride,
                  uint32_t *d_bounds, uint64_t bounds_stride, uint32_t *d_scratch, uint32_t *d_best, uint32_t *d_work,
                  uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !m || !d_field || !d_pooled || !d_bounds || !d_scratch || !d_best || !d_work || group == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_wide_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_match_wide_dev: invalid rplgpu_wide_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (field_stride < (uint64_t)m->width * m->height || (field_stride & 3u) || misaligned(d_field, 3u)) {
    h->err = "rplgpu_match_wide_dev: field_stride must be >= width * height and a multiple of 4, d_field 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (pooled_stride < pooled_cells(m) || (pooled_stride & 3u) || misaligned(d_pooled, 3u)) {
    h->err = "rplgpu_match_wide_dev: pooled_stride must be >= (width + 7) * (height + 7) and a multiple of 4, d_pooled 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint32_t blocks = rplgpu_wide_match_blocks(m);
  if (bounds_stride < blocks || misaligned(d_bounds, 3u) || misaligned(d_best, 3u) || misaligned(d_work, 3u) ||
      misaligned(d_status, 3u) || misaligned(d_scratch, 7u)) {
    h->err = "rplgpu_match_wide_dev: bounds_stride must be >= the volume size, d_bounds / d_best / d_work / d_status 4-byte and d_scratch 8-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_pivot, "d_pivot", false},
                           {d_field, "d_field", true}, {d_pooled, "d_pooled", true}, {d_bounds, "d_bounds", true},
                           {d_scratch, "d_scratch", true}, {d_best, "d_best", true}, {d_work, "d_work", true},
                           {d_status, "d_status", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  ScanPrologue pro;
  if ((rc = pro.admit(h, "rplgpu_match_wide_dev", p, d_motion, d_t0, B, group))) return rc;
  if ((uint64_t)pro.group * n_stride > (1ull << 24)) {  // 127 x points stays below 2^32: no bound or score wraps
    h->err = "rplgpu_match_wide_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const rpl::WideK wk = wide_k(m);
  // the rotation table is E13's, by E13's own function
  const rplgpu_scan_match_t m13{m->origin_x, m->origin_y, m->resolution, m->width, m->height, 0, 0, m->rot_steps,
                                m->rot_step};
  rpl::MatchRot rot;  // at most 129 pairs, handed to the kernels by value: no copy on the stream
  std::memset(&rot, 0, sizeof(rot));
  if (rplgpu_scan_match_rotations(&m13, rot.cs) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  if ((rc = pro.begin(h, d_nodes, n_stride, d_n_per_scan, B, p, d_t0, d_status))) return rc;
  RPL_HIP(h, rpl::launch_wide_prepare(h->stream, d_bounds, bounds_stride, pro.G, wk, d_scratch, d_best, d_work));
  RPL_HIP(h, rpl::launch_wide_bound(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T, pro.mask,
                                    kMaskStride, d_motion, d_pose2d, d_pivot, wk, rot, d_pooled, pooled_stride,
                                    field_per_group, d_bounds, bounds_stride, d_best, d_status));
  RPL_HIP(h, rpl::launch_wide_seed(h->stream, d_bounds, bounds_stride, pro.G, wk, d_scratch, d_work));
  RPL_HIP(h, rpl::launch_wide_refine(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T, pro.mask,
                                     kMaskStride, d_motion, d_pose2d, d_pivot, wk, rot, d_field, field_stride,
                                     field_per_group, d_scratch, 1u));
  RPL_HIP(h, rpl::launch_wide_list(h->stream, d_bounds, bounds_stride, pro.G, wk, d_scratch, d_work));
  RPL_HIP(h, rpl::launch_wide_refine(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T, pro.mask,
                                     kMaskStride, d_motion, d_pose2d, d_pivot, wk, rot, d_field, field_stride,
                                     field_per_group, d_scratch, 0u));
  RPL_HIP(h, rpl::launch_wide_best(h->stream, pro.G, wk, d_scratch, d_best));
  return RPLGPU_OK;
}

}  // namespace

extern "C" {

int32_t rplgpu_pool_field_dev(rplgpu_handle_t h, const rplgpu_wide_match_t *m, const int8_t *d_field,
                              uint64_t field_stride, uint32_t F, int8_t *d_pooled, uint64_t pooled_stride) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return pool_impl(h, m, d_field, field_stride, F, d_pooled, pooled_stride);
}

int32_t rplgpu_match_wide_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                              const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                              const float *d_motion, const float *d_pose2d, const float *d_pivot,
                              const rplgpu_wide_match_t *m, const int8_t *d_field, uint64_t field_stride,
                              uint32_t field_per_group, const int8_t *d_pooled, uint64_t pooled_stride,
                              uint32_t *d_bounds, uint64_t bounds_stride, uint32_t *d_scratch, uint32_t *d_best,
                              uint32_t *d_work, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return wide_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, d_pivot, m, d_field,
                   field_stride, field_per_group, d_pooled, pooled_stride, d_bounds, bounds_stride, d_scratch, d_best,
                   d_work, d_status);
}

int32_t rplgpu_match_wide(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                          const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                          const float *motion, const float *pose2d, const float *t0, const float *pivot,
                          const rplgpu_wide_match_t *m, const int8_t *field, uint32_t *bounds_out, uint32_t best[8],
                          uint32_t work[8], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !m || !field || !best || !work || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_wide_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_match_wide: invalid rplgpu_wide_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)m->width * m->height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t pstride = ((size_t)pooled_cells(m) + 3u) & ~(size_t)3u;
  const size_t blocks = rplgpu_wide_match_blocks(m);
  // field | pooled | bounds | scratch | the scans | pivot | best + work + status
  DoorBuffer buf(h, "rplgpu_match_wide");
  const size_t o_field = buf.part(stride), o_pool = buf.part(pstride), o_bd = buf.part(4u * blocks);
  const size_t o_scr = buf.part(4u * (size_t)rplgpu_wide_match_scratch_words(m, 1));
  DoorScans scans(buf, nodes, n_stride, n_per_scan, n_scans, motion, pose2d, t0);
  const size_t o_pv = buf.part_if(pivot, 8), o_small = buf.part(80);
  uint32_t small[17];
  std::memset(small, 0, sizeof(small));
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_field), field, cells_n, hipMemcpyHostToDevice, h->stream));
    if (int32_t urc = scans.upload(h, buf)) return urc;
    if (pivot) RPL_HIP(h, hipMemcpyAsync(buf.at(o_pv), pivot, 8u, hipMemcpyHostToDevice, h->stream));
    if (int32_t prc = pool_impl(h, m, buf.at<const int8_t>(o_field), stride, 1, buf.at<int8_t>(o_pool), pstride))
      return prc;
    uint32_t *d_small = buf.at<uint32_t>(o_small);
    const int32_t irc = wide_impl(h, scans.d_nodes, n_stride, scans.d_n_per_scan, n_scans, n_scans, p, scans.d_motion,
                                  scans.d_pose2d, scans.d_t0, buf.at<const float>(o_pv), m,
                                  buf.at<const int8_t>(o_field), stride, 0, buf.at<const int8_t>(o_pool), pstride,
                                  buf.at<uint32_t>(o_bd), blocks, buf.at<uint32_t>(o_scr), d_small, d_small + 8,
                                  d_small + 16);
    if (irc) return irc;
    if (bounds_out)
      RPL_HIP(h, hipMemcpyAsync(bounds_out, buf.at(o_bd), 4u * blocks, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 68, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(best, small, 32);
  std::memcpy(work, small + 8, 32);
  if (status) *status = small[16];
  return RPLGPU_OK;
}

}  // extern "C"
