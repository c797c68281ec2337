// rplgpu_scan_stages.hip — the extern "C" entry points of the stages that consume scans or the grids made from
// them (include/rplgpu_msg.h): E9 merged LaserScans, E10 scan filters, E11 occupancy grids, E12 inflation, E13 scan
// matching, E14 the hit / miss map.
//
// Host side only: argument checks, the launches and the host-buffer doors; the kernels are in rpl_merge.hip,
// rpl_filter.hip, rpl_occ.hip, rpl_inflate.hip, rpl_match.hip and rpl_map.hip.  The handle, the helpers of
// rplgpu_api.hip and the doors' per-call buffer come from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_msg.hpp"

using namespace rpl::host;

// ---- the scan-stage prologue (rpl_host.hpp) ----------------------------------------------------------------------------

int32_t ScanPrologue::admit(rplgpu_ctx *h, const char *fn, const rplgpu_params_t *p, const float *d_motion,
                            const float *d_t0, uint32_t B, uint32_t group_asked) {
  if (d_t0 && !d_motion) {
    h->err = std::string(fn) + ": scan time offsets are set (rplgpu_set_scan_time_offsets_dev) but d_motion is NULL";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (p->ror_enable && !(p->ror_radius > 0.0f && p->ror_radius <= 1.0e6f)) {
    h->err = "ror_radius must be in (0, 1e6] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  group = std::min(group_asked, B);
  G = (B + group - 1u) / group;
  return RPLGPU_OK;
}

int32_t ScanPrologue::begin(rplgpu_ctx *h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                            const uint32_t *d_n_per_scan, uint32_t B, const rplgpu_params_t *p, const float *d_t0,
                            uint32_t *d_status) {
  RPL_HIP(h, hipSetDevice(h->device));
  kp = to_kparams(*p);
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  T = tables_of(h);
  T.scan_t0 = d_t0;
  if (p->ror_enable) {  // E1 AND E5 keep bits, the mask E8's two-kernel path applies
    RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, T, h->d_rormask, kMaskStride));
    mask = h->d_rormask;
  }
  if (d_status) RPL_HIP(h, hipMemsetAsync(d_status, 0, (size_t)G * 4u, h->stream));
  return RPLGPU_OK;
}

extern "C" {

// ---- E9: one merged LaserScan per group of scans (include/rplgpu_msg.h) ---------------------------

int32_t rplgpu_scan_merge_edges(const rplgpu_scan_merge_t *m, float *edges, float *inc) {
  if (!m) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(m->angle_min) || !std::isfinite(m->angle_max) || !std::isfinite(m->range_min) ||
      !std::isfinite(m->range_max) || !std::isfinite(m->scan_time))
    return RPLGPU_ERR_INVALID_ARG;
  if (m->count == 0 || m->count > RPLGPU_MAX_MERGE_BEAMS) return RPLGPU_ERR_INVALID_ARG;
  const double span = (double)m->angle_max - (double)m->angle_min;
  const float f_inc = (float)(span / (double)m->count);
  if (!(f_inc > 0.0f) || f_inc > (float)(M_PI / 2)) return RPLGPU_ERR_INVALID_ARG;
  if (span > 2.0 * M_PI * (1.0 + 0x1p-20)) return RPLGPU_ERR_INVALID_ARG;
  if (!(0.0f <= m->range_min && m->range_min < m->range_max)) return RPLGPU_ERR_INVALID_ARG;
  if (edges)
    for (uint32_t k = 0; k <= m->count; ++k) {
      const double phi = (double)m->angle_min + (double)k * (double)f_inc;
      edges[2 * k] = (float)std::cos(phi);
      edges[2 * k + 1] = (float)std::sin(phi);
    }
  if (inc) *inc = f_inc;
  return RPLGPU_OK;
}

namespace {

// e_a -> e_b turns by an angle in (0, pi): the exact sign of the fp64 cross product of float vectors
bool turns_left(float2 a, float2 b) { return (double)a.x * (double)b.y - (double)a.y * (double)b.x > 0.0; }

// the edge table of spec `m` on the device and the kernel's view of it (cached per spec)
int32_t merge_spec_upload(rplgpu_ctx *c, const rplgpu_scan_merge_t &m, rpl::MergeK *out) {
  if (c->mspec_valid && std::memcmp(&c->mspec, &m, sizeof(m)) == 0) {
    *out = c->mspec_k;
    return RPLGPU_OK;
  }
  std::vector<float2> e(m.count + 1u);
  float inc = 0.0f;
  if (rplgpu_scan_merge_edges(&m, reinterpret_cast<float *>(e.data()), &inc) != RPLGPU_OK) {
    c->err = "rplgpu_scan_merge_t: invalid spec (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  // the table in use may still be read by queued launches
  RPL_HIP(c, hipStreamSynchronize(c->stream));
  c->mspec_valid = false;
  if (e.size() > c->medges_cap) {
    if (c->d_medges) (void)hipFree(c->d_medges);
    c->d_medges = nullptr;
    c->medges_cap = 0;
    RPL_HIP(c, hipMalloc((void **)&c->d_medges, e.size() * sizeof(float2)));
    c->medges_cap = e.size();
  }
  RPL_HIP(c, hipMemcpy(c->d_medges, e.data(), e.size() * sizeof(float2), hipMemcpyHostToDevice));
  rpl::MergeK k;
  k.edges = c->d_medges;
  k.count = m.count;
  bool mono = true;
  for (uint32_t i = 0; i < m.count && mono; ++i) mono = turns_left(e[i], e[i + 1]);
  for (int q = 0; q < 5; ++q) {
    k.qb[q] = (uint32_t)((uint64_t)q * m.count / 4u);
    k.qe[q] = e[k.qb[q]];
  }
  for (int q = 0; q < 4 && mono; ++q)
    if (k.qb[q] != k.qb[q + 1]) mono = turns_left(k.qe[q], k.qe[q + 1]);
  k.monotone = mono ? 1u : 0u;
  double a0 = std::fmod((double)m.angle_min, 2.0 * M_PI);
  if (a0 < 0.0) a0 += 2.0 * M_PI;
  k.a0 = (float)a0;
  k.rinc = 1.0f / inc;
  k.range_min = m.range_min;
  k.range_max = m.range_max;
  c->mspec = m;
  c->mspec_k = k;
  c->mspec_valid = true;
  *out = k;
  return RPLGPU_OK;
}

}  // namespace

int32_t rplgpu_merge_scans_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                               const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                               const rplgpu_scan_merge_t *m, float *d_ranges, float *d_intensities,
                               uint32_t *d_beams_hit, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !m || !d_ranges || !d_intensities || !d_beams_hit || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_merge_edges(m, nullptr, nullptr) != RPLGPU_OK) {
    h->err = "rplgpu_merge_scans_dev: invalid rplgpu_scan_merge_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_ranges, "d_ranges", true},
                           {d_intensities, "d_intensities", true}, {d_beams_hit, "d_beams_hit", true},
                           {d_status, "d_status", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  // admit() only: this stage sets up its edge table and key rows between hipSetDevice and the keep mask
  ScanPrologue pro;
  if ((rc = pro.admit(h, "rplgpu_merge_scans_dev", p, d_motion, h->scan_t0, B, group))) return rc;
  group = pro.group;
  if ((uint64_t)group * std::min(n_stride, rpl::kMaxN) > (1ull << 24) || group > (1u << rpl::kMergeSlotBits)) {
    h->err = "rplgpu_merge_scans_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_CAPACITY;
  }
  const uint32_t G = pro.G;
  RPL_HIP(h, hipSetDevice(h->device));
  rpl::MergeK mk;
  if ((rc = merge_spec_upload(h, *m, &mk))) return rc;
  const size_t need = (size_t)G * m->count;
  if (need > h->mkeys_cap) {  // (only ever grows; fresh rows are empty)
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    if (h->d_mkeys) (void)hipFree(h->d_mkeys);
    h->d_mkeys = nullptr;
    h->mkeys_cap = 0;
    if (hipMalloc((void **)&h->d_mkeys, need * sizeof(unsigned long long)) != hipSuccess) {
      h->err = "merge key rows allocation failed";
      (void)hipGetLastError();
      return RPLGPU_ERR_HIP;
    }
    h->mkeys_cap = need;
    h->mkeys_clean = false;
  }
  if (!h->mkeys_clean)  // a new allocation, or a call that failed between the two launches
    RPL_HIP(h, hipMemsetAsync(h->d_mkeys, 0xFF, h->mkeys_cap * sizeof(unsigned long long), h->stream));
  rpl::KParams kp = to_kparams(*p);
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  const rpl::Tables T = tables_of(h);
  const uint32_t *mask = nullptr;
  if (p->ror_enable) {  // E1 AND E5 keep bits, the mask E8's two-kernel path applies
    RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, T, h->d_rormask,
                                    kMaskStride));
    mask = h->d_rormask;
  }
  RPL_HIP(h, hipMemsetAsync(d_beams_hit, 0, (size_t)G * 4u, h->stream));
  if (d_status) RPL_HIP(h, hipMemsetAsync(d_status, 0, (size_t)G * 4u, h->stream));
  h->mkeys_clean = false;
  RPL_HIP(h, rpl::launch_merge_scans(h->stream, d_nodes, n_stride, d_n_per_scan, B, group, kp, T, mask,
                                     kMaskStride, d_motion, d_pose2d, mk, h->d_mkeys, d_status));
  RPL_HIP(h, rpl::launch_merge_finish(h->stream, h->d_mkeys, G, m->count, d_nodes, n_stride, group,
                                      p->is_new_protocol, d_ranges, d_intensities, d_beams_hit));
  h->mkeys_clean = true;
  return RPLGPU_OK;
}

int32_t rplgpu_merged_laserscan_msgs_dev(rplgpu_handle_t h, const float *d_ranges,
                                         const float *d_intensities, uint32_t G,
                                         const rplgpu_scan_merge_t *m, const char *frame_id,
                                         const rplgpu_stamp_t *d_stamps, uint8_t *d_msgs,
                                         uint32_t msg_stride, uint32_t *d_msg_len, uint32_t *d_status) {
  if (!h || !m || !frame_id) return RPLGPU_ERR_INVALID_ARG;
  float inc = 0.0f;
  if (rplgpu_scan_merge_edges(m, nullptr, &inc) != RPLGPU_OK) {
    h->err = "rplgpu_merged_laserscan_msgs_dev: invalid rplgpu_scan_merge_t";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_stamps || !d_msgs || !d_msg_len || (msg_stride & 3u))
    return RPLGPU_ERR_INVALID_ARG;
  const size_t fl = std::strlen(frame_id);
  if (fl > rplmsg::kMaxFrameId) {
    h->err = "frame_id longer than 255 bytes";
    return RPLGPU_ERR_INVALID_ARG;
  }
  rplgpu_scan_meta_t meta;
  std::memset(&meta, 0, sizeof(meta));
  meta.angle_min = m->angle_min;
  meta.angle_max = m->angle_max;
  meta.angle_increment = inc;
  meta.time_increment = 0.0f;  // every point is already moved to the fused instant
  meta.scan_time = m->scan_time;
  meta.range_min = m->range_min;
  meta.range_max = m->range_max;
  meta.count = m->count;
  meta.published = 1;
  rplmsg::Prefix P;
  std::memset(&P, 0, sizeof(P));
  rplmsg::Writer w(reinterpret_cast<uint8_t *>(P.words), sizeof(P.words));
  rplgpu_laserscan_layout_t L;
  rplmsg::write_laserscan(w, frame_id, fl, rplgpu_stamp_t{0, 0}, meta, &L);
  P.stamp_off = 4;
  P.len = L.ranges_off;  // every scalar and the ranges length word come with the template
  P.a_off = L.scalars_off;
  P.b_off = L.ranges_len_off;
  if (P.len > sizeof(P.words) || (P.len & 3u)) {
    h->err = "message prefix does not fit the device template";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_msg_merged(h->stream, d_ranges, d_intensities, m->count, G, d_stamps, P, d_msgs,
                                    msg_stride, d_msg_len, d_status));
  return RPLGPU_OK;
}

// ---- E10: scan-shadow and speckle filters on LaserScan arrays (include/rplgpu_msg.h) ---------------

void rplgpu_default_scan_filter(rplgpu_scan_filter_t *f) {
  if (!f) return;
  f->shadow_enable = 1;
  f->shadow_min_angle = (float)(10.0 * M_PI / 180.0);
  f->shadow_max_angle = (float)(170.0 * M_PI / 180.0);
  f->shadow_window = 2;
  f->shadow_neighbors = 1;
  f->speckle_enable = 1;
  f->speckle_max_range_difference = 0.05f;
  f->speckle_min_run = 4;
  f->circular = 1;
}

int32_t rplgpu_scan_filter_check(const rplgpu_scan_filter_t *f, float dirs[4]) {
  if (!f) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(f->shadow_min_angle) || !std::isfinite(f->shadow_max_angle) ||
      !std::isfinite(f->speckle_max_range_difference))
    return RPLGPU_ERR_INVALID_ARG;
  const double lo = (double)f->shadow_min_angle, hi = (double)f->shadow_max_angle;
  if (!(0.0 < lo && lo < M_PI / 2 && M_PI / 2 < hi && hi < M_PI)) return RPLGPU_ERR_INVALID_ARG;
  if (f->shadow_window < 1u || f->shadow_window > RPLGPU_MAX_FILTER_WINDOW ||
      f->shadow_neighbors > RPLGPU_MAX_FILTER_WINDOW || f->speckle_min_run < 1u ||
      f->speckle_min_run > RPLGPU_MAX_FILTER_WINDOW || !(f->speckle_max_range_difference >= 0.0f))
    return RPLGPU_ERR_INVALID_ARG;
  if (dirs) {
    dirs[0] = (float)std::cos(lo);
    dirs[1] = (float)std::sin(lo);
    dirs[2] = (float)std::cos(hi);
    dirs[3] = (float)std::sin(hi);
  }
  return RPLGPU_OK;
}

namespace {

int32_t filter_kernel_args(rplgpu_ctx *c, const rplgpu_scan_filter_t *f, rpl::FilterK *k) {
  float dirs[4];
  if (rplgpu_scan_filter_check(f, dirs) != RPLGPU_OK) {
    c->err = "invalid rplgpu_scan_filter_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  std::memset(k, 0, sizeof(*k));
  k->shadow = f->shadow_enable ? 1u : 0u;
  k->speckle = f->speckle_enable ? 1u : 0u;
  k->circular = f->circular ? 1u : 0u;
  k->W = f->shadow_window;
  k->N = f->shadow_neighbors;
  k->L = f->speckle_min_run;
  k->D = f->speckle_max_range_difference;
  k->cmin = dirs[0];
  k->smin = dirs[1];
  k->cmax = dirs[2];
  k->smax = dirs[3];
  return RPLGPU_OK;
}

}  // namespace

int32_t rplgpu_filter_laserscan_batch_dev(rplgpu_handle_t h, const float *d_ranges, const float *d_intensities,
                                          uint32_t n_stride, const uint32_t *d_beam_count, uint32_t B,
                                          const rplgpu_params_t *p, const rplgpu_scan_filter_t *f,
                                          float *d_ranges_out, float *d_intensities_out, uint32_t *d_removed) {
  if (!h || !p || !f) return RPLGPU_ERR_INVALID_ARG;
  rpl::FilterK k;
  if (int32_t rc = filter_kernel_args(h, f, &k)) return rc;
  if (B == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_beam_count || !d_ranges_out || !d_intensities_out || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (d_ranges_out == d_ranges || d_intensities_out == d_intensities) {
    h->err = "rplgpu_filter_laserscan_batch_dev: the filters do not work in place";
    return RPLGPU_ERR_INVALID_ARG;
  }
  k.inc_mode = p->scan_processing ? rpl::kFilterIncModeA : rpl::kFilterIncModeB;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_removed) RPL_HIP(h, hipMemsetAsync(d_removed, 0, (size_t)B * 8u, h->stream));
  RPL_HIP(h, rpl::launch_filter_scans(h->stream, d_ranges, d_intensities, n_stride, d_beam_count, B, k,
                                      d_ranges_out, d_intensities_out, d_removed));
  return RPLGPU_OK;
}

int32_t rplgpu_filter_merged_scans_dev(rplgpu_handle_t h, const float *d_ranges, const float *d_intensities,
                                       uint32_t G, const rplgpu_scan_merge_t *m, const rplgpu_scan_filter_t *f,
                                       float *d_ranges_out, float *d_intensities_out, uint32_t *d_removed) {
  if (!h || !m || !f) return RPLGPU_ERR_INVALID_ARG;
  rpl::FilterK k;
  if (int32_t rc = filter_kernel_args(h, f, &k)) return rc;
  float inc = 0.0f;
  if (rplgpu_scan_merge_edges(m, nullptr, &inc) != RPLGPU_OK) {
    h->err = "rplgpu_filter_merged_scans_dev: invalid rplgpu_scan_merge_t";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_ranges_out || !d_intensities_out) return RPLGPU_ERR_INVALID_ARG;
  if (d_ranges_out == d_ranges || d_intensities_out == d_intensities) {
    h->err = "rplgpu_filter_merged_scans_dev: the filters do not work in place";
    return RPLGPU_ERR_INVALID_ARG;
  }
  k.inc_mode = rpl::kFilterIncGiven;
  k.inc = inc;
  k.count = m->count;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_removed) RPL_HIP(h, hipMemsetAsync(d_removed, 0, (size_t)G * 8u, h->stream));
  RPL_HIP(h, rpl::launch_filter_scans(h->stream, d_ranges, d_intensities, m->count, nullptr, G, k,
                                      d_ranges_out, d_intensities_out, d_removed));
  return RPLGPU_OK;
}

int32_t rplgpu_filter_laserscan(rplgpu_handle_t h, const float *ranges, const float *intensities, uint32_t count,
                                float angle_increment, const rplgpu_scan_filter_t *f, float *ranges_out,
                                float *intensities_out, uint32_t removed[2]) {
  if (!h || !f) return RPLGPU_ERR_INVALID_ARG;
  rpl::FilterK k;
  if (int32_t rc = filter_kernel_args(h, f, &k)) return rc;
  if (!std::isfinite(angle_increment) || !(angle_increment > 0.0f)) {
    h->err = "rplgpu_filter_laserscan: angle_increment must be finite and positive";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (count && (!ranges || !intensities || !ranges_out || !intensities_out)) return RPLGPU_ERR_INVALID_ARG;
  if (count && (ranges_out == ranges || intensities_out == intensities)) {
    h->err = "rplgpu_filter_laserscan: the filters do not work in place";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (count > h->max_n) return RPLGPU_ERR_CAPACITY;
  if (removed) removed[0] = removed[1] = 0u;
  if (count == 0) return RPLGPU_OK;
  k.inc_mode = rpl::kFilterIncGiven;
  k.inc = angle_increment;
  k.count = count;
  RPL_HIP(h, hipSetDevice(h->device));
  // staging as rplgpu_laserscan_to_cloud: ranges | intensities in (d_nodes holds 8 B per sample),
  // ranges | intensities | the two counts out (d_out holds 16 B per sample)
  const size_t n = count;
  std::memcpy(h->h_pin, ranges, n * 4);
  std::memcpy(h->h_pin + n * 4, intensities, n * 4);
  RPL_HIP(h, hipMemcpyAsync(h->d_nodes, h->h_pin, n * 8, hipMemcpyHostToDevice, h->stream));
  const float *d_r = reinterpret_cast<const float *>(h->d_nodes);
  float *d_o = reinterpret_cast<float *>(h->d_out);
  uint32_t *d_rm = reinterpret_cast<uint32_t *>(h->d_out + n * 8);
  RPL_HIP(h, hipMemsetAsync(d_rm, 0, 8, h->stream));
  RPL_HIP(h, rpl::launch_filter_scans(h->stream, d_r, d_r + n, count, nullptr, 1, k, d_o, d_o + n, d_rm));
  unsigned char *h_out = stage_out(h);
  RPL_HIP(h, hipMemcpyAsync(h_out, h->d_out, n * 8 + 8, hipMemcpyDeviceToHost, h->stream));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  std::memcpy(ranges_out, h_out, n * 4);
  std::memcpy(intensities_out, h_out + n * 4, n * 4);
  if (removed) std::memcpy(removed, h_out + n * 8, 8);
  return RPLGPU_OK;
}

// ---- E11: one ray-cast occupancy grid per group of scans (include/rplgpu_msg.h) ---------------------

void rplgpu_default_occ_grid(rplgpu_occ_grid_t *grid) {
  if (!grid) return;
  grid->origin_x = -25.6f;
  grid->origin_y = -25.6f;
  grid->resolution = 0.05f;
  grid->width = 1024;
  grid->height = 1024;
  grid->range_min = 0.0f;
  grid->obstacle_max = 25.0f;
  grid->raytrace_max = 30.0f;
}

int32_t rplgpu_occ_grid_check(const rplgpu_occ_grid_t *g) {
  if (!g) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(g->origin_x) || !std::isfinite(g->origin_y) || !std::isfinite(g->resolution) ||
      !std::isfinite(g->range_min) || !std::isfinite(g->obstacle_max) || !std::isfinite(g->raytrace_max))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(g->resolution > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (g->width == 0 || g->width > RPLGPU_MAX_OCC_DIM || g->height == 0 || g->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (!(0.0f <= g->range_min && g->range_min < g->obstacle_max && g->obstacle_max <= g->raytrace_max))
    return RPLGPU_ERR_INVALID_ARG;
  if ((double)g->raytrace_max / (double)g->resolution > (double)RPLGPU_MAX_OCC_STEPS) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

static rpl::OccK occ_kernel_args(const rplgpu_occ_grid_t &g) {
  return rpl::OccK{g.origin_x, g.origin_y, g.resolution, g.width, g.height, g.range_min, g.obstacle_max,
                   g.raytrace_max};
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t occ_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                        const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                        const float *d_motion, const float *d_pose2d, const float *d_t0,
                        const rplgpu_occ_grid_t *grid, const int8_t *d_prev, int8_t *d_grid,
                        uint64_t grid_stride, uint32_t *d_cells, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !grid || !d_grid || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_occupancy_grid_dev: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (grid_stride < (uint64_t)grid->width * grid->height || (grid_stride & 3u) ||
      (reinterpret_cast<uintptr_t>(d_grid) & 3u)) {
    h->err = "rplgpu_occupancy_grid_dev: grid_stride must be >= width * height and a multiple of 4, d_grid 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_prev == d_grid) {
    h->err = "rplgpu_occupancy_grid_dev: d_prev must not be d_grid (the grid is its own scratch)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_prev, "d_prev", false},
                           {d_grid, "d_grid", true}, {d_cells, "d_cells", false}, {d_status, "d_status", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  ScanPrologue pro;
  if ((rc = pro.admit(h, "rplgpu_occupancy_grid_dev", p, d_motion, d_t0, B, group))) return rc;
  if ((uint64_t)pro.group * std::min(n_stride, rpl::kMaxN) > (1ull << 24)) {
    h->err = "rplgpu_occupancy_grid_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_CAPACITY;
  }
  if ((rc = pro.begin(h, d_nodes, n_stride, d_n_per_scan, B, p, d_t0, d_status))) return rc;
  const rpl::OccK k = occ_kernel_args(*grid);
  if (d_cells) RPL_HIP(h, hipMemsetAsync(d_cells, 0, (size_t)pro.G * 12u, h->stream));
  RPL_HIP(h, rpl::launch_occ_prepare(h->stream, d_grid, grid_stride, pro.G, k));
  RPL_HIP(h, rpl::launch_occ_walk(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T, pro.mask,
                                  kMaskStride, d_motion, d_pose2d, k, d_grid, grid_stride, d_status));
  RPL_HIP(h, rpl::launch_occ_finish(h->stream, d_grid, grid_stride, pro.G, k, d_prev, d_cells));
  return RPLGPU_OK;
}

int32_t rplgpu_occupancy_grid_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                  const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                                  const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                                  const rplgpu_occ_grid_t *grid, const int8_t *d_prev, int8_t *d_grid,
                                  uint64_t grid_stride, uint32_t *d_cells, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return occ_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, grid, d_prev,
                  d_grid, grid_stride, d_cells, d_status);
}

int32_t rplgpu_occupancy_grid(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                              const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                              const float *motion, const float *pose2d, const float *t0,
                              const rplgpu_occ_grid_t *grid, const int8_t *prev, int8_t *grid_out,
                              uint32_t cells[3], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !grid || !grid_out || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_occupancy_grid: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)grid->width * grid->height, stride = (cells_n + 3u) & ~(size_t)3u;
  // grid | prev | the scans | cells + status
  DoorBuffer buf(h, "rplgpu_occupancy_grid");
  const size_t o_grid = buf.part(stride), o_prev = buf.part_if(prev, stride);
  DoorScans scans(buf, nodes, n_stride, n_per_scan, n_scans, motion, pose2d, t0);
  const size_t o_small = buf.part(16);
  uint32_t small[4] = {0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    if (prev) RPL_HIP(h, hipMemcpyAsync(buf.at(o_prev), prev, cells_n, hipMemcpyHostToDevice, h->stream));
    if (int32_t urc = scans.upload(h, buf)) return urc;
    uint32_t *d_small = buf.at<uint32_t>(o_small);
    const int32_t irc = occ_impl(h, scans.d_nodes, n_stride, scans.d_n_per_scan, n_scans, n_scans, p, scans.d_motion,
                                 scans.d_pose2d, scans.d_t0, grid, buf.at<const int8_t>(o_prev),
                                 buf.at<int8_t>(o_grid), stride, d_small, d_small + 3);
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(grid_out, buf.at(o_grid), cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 16, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  if (cells) std::memcpy(cells, small, 12);
  if (status) *status = small[3];
  return RPLGPU_OK;
}

int32_t rplgpu_msg_occupancy_layout(size_t frame_id_len, uint32_t width, uint32_t height,
                                    rplgpu_occupancy_layout_t *out) {
  if (!out || frame_id_len > (1u << 20) || width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 ||
      height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  rplmsg::Writer w(nullptr, 0);
  std::string fid(frame_id_len, 'x');
  rplmsg::write_occupancy(w, fid.data(), frame_id_len, rplgpu_stamp_t{0, 0}, 1.0f, width, height, 0.0f, 0.0f, out);
  return RPLGPU_OK;
}

int32_t rplgpu_occupancy_grid_msgs_dev(rplgpu_handle_t h, const int8_t *d_grid, uint64_t grid_stride, uint32_t G,
                                       const rplgpu_occ_grid_t *grid, const char *frame_id,
                                       const rplgpu_stamp_t *d_stamps, uint8_t *d_msgs, uint32_t msg_stride,
                                       uint32_t *d_msg_len, uint32_t *d_status) {
  if (!h || !grid || !frame_id) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_occupancy_grid_msgs_dev: invalid rplgpu_occ_grid_t";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0) return RPLGPU_OK;
  if (!d_grid || !d_stamps || !d_msgs || !d_msg_len || (msg_stride & 3u) || (grid_stride & 3u) ||
      grid_stride < (uint64_t)grid->width * grid->height || (reinterpret_cast<uintptr_t>(d_grid) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_msgs) & 3u))
    return RPLGPU_ERR_INVALID_ARG;
  const size_t fl = std::strlen(frame_id);
  if (fl > rplmsg::kMaxFrameId) {
    h->err = "frame_id longer than 255 bytes";
    return RPLGPU_ERR_INVALID_ARG;
  }
  rplmsg::Prefix P;
  std::memset(&P, 0, sizeof(P));
  rplmsg::Writer w(reinterpret_cast<uint8_t *>(P.words), sizeof(P.words));
  rplgpu_occupancy_layout_t L;
  rplmsg::write_occupancy(w, frame_id, fl, rplgpu_stamp_t{0, 0}, grid->resolution, grid->width, grid->height,
                          grid->origin_x, grid->origin_y, &L);
  P.stamp_off = 4;
  P.len = L.data_off;  // every scalar and the data length word come with the template
  P.a_off = L.map_load_time_off;
  if (P.len > sizeof(P.words) || (P.len & 3u)) {
    h->err = "message prefix does not fit the device template";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_msg_occupancy(h->stream, d_grid, grid_stride, grid->width * grid->height, G, d_stamps, P,
                                       d_msgs, msg_stride, d_msg_len, d_status));
  return RPLGPU_OK;
}

// ---- E12: the grids of E11 inflated into costmaps (include/rplgpu_msg.h) -------------------------------

void rplgpu_default_inflation(rplgpu_inflation_t *f) {
  if (!f) return;
  f->inscribed_radius = 0.22f;
  f->inflation_radius = 0.55f;
  f->cost_scaling_factor = 3.0f;
  f->inflate_unknown = 0;
}

// the check, and Rc of a spec that passes it
static int32_t inflation_reach(const rplgpu_inflation_t *f, float resolution, uint32_t *rc) {
  if (!f) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(f->inscribed_radius) || !std::isfinite(f->inflation_radius) ||
      !std::isfinite(f->cost_scaling_factor) || !std::isfinite(resolution))
    return RPLGPU_ERR_INVALID_ARG;
  if (f->inscribed_radius < 0.0f || f->inflation_radius < 0.0f || f->cost_scaling_factor < 0.0f ||
      !(resolution > 0.0f) || f->inflation_radius < f->inscribed_radius || f->inflate_unknown > 1u)
    return RPLGPU_ERR_INVALID_ARG;
  const double cells = std::ceil((double)f->inflation_radius / (double)resolution);
  if (!(cells <= (double)RPLGPU_MAX_INFLATION_CELLS)) return RPLGPU_ERR_INVALID_ARG;
  *rc = (uint32_t)cells;
  return RPLGPU_OK;
}

int32_t rplgpu_inflation_check(const rplgpu_inflation_t *f, float resolution) {
  uint32_t rc = 0;
  return inflation_reach(f, resolution, &rc);
}

int32_t rplgpu_inflation_table(const rplgpu_inflation_t *f, float resolution, uint8_t *table, uint32_t table_cap,
                               uint32_t *rc_out) {
  uint32_t rc = 0;
  if (inflation_reach(f, resolution, &rc) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  if (rc_out) *rc_out = rc;
  if (!table) return RPLGPU_ERR_INVALID_ARG;
  if (table_cap < rc * rc + 1u) return RPLGPU_ERR_CAPACITY;
  const double res = (double)resolution, inscribed = (double)f->inscribed_radius;
  table[0] = 100;
  for (uint32_t k = 1; k <= rc * rc; ++k) {
    const double d = std::sqrt((double)k) * res;
    table[k] = d <= inscribed
                   ? (uint8_t)99
                   : (uint8_t)(int)(98.0 * std::exp(-(double)f->cost_scaling_factor * (d - inscribed)));
  }
  return RPLGPU_OK;
}

int32_t rplgpu_inflate_grids_dev(rplgpu_handle_t h, const int8_t *d_in, uint64_t in_stride, int8_t *d_out,
                                 uint64_t out_stride, uint32_t G, uint32_t width, uint32_t height,
                                 const uint8_t *d_table, uint32_t rc, uint32_t inflate_unknown, uint32_t *d_cells) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (!d_in || !d_out || !d_table || G == 0) {
    h->err = "rplgpu_inflate_grids_dev: d_in, d_out and d_table must be given and G >= 1";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_in == d_out) {
    h->err = "rplgpu_inflate_grids_dev: d_out must not be d_in (a tile reads the cells around it)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (rc > RPLGPU_MAX_INFLATION_CELLS || inflate_unknown > 1u) {
    h->err = "rplgpu_inflate_grids_dev: rc above RPLGPU_MAX_INFLATION_CELLS or inflate_unknown above 1";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_inflate_grids_dev: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t n_cells = (uint64_t)width * height;
  if (in_stride < n_cells || (in_stride & 3u) || out_stride < n_cells || (out_stride & 3u) ||
      (reinterpret_cast<uintptr_t>(d_in) & 3u) || (reinterpret_cast<uintptr_t>(d_out) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_table) & 3u) || (reinterpret_cast<uintptr_t>(d_cells) & 3u)) {
    h->err = "rplgpu_inflate_grids_dev: strides must be >= width * height and multiples of 4, pointers 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t tiles = (uint64_t)((width + 63u) / 64u) * ((height + 63u) / 64u);
  if (G * tiles > 0x7FFFFFFFull) {
    h->err = "rplgpu_inflate_grids_dev: G x tiles above 2^31";
    return RPLGPU_ERR_CAPACITY;
  }
  if (!device_readable(h, {{d_in, "d_in", true}, {d_out, "d_out", true}, {d_table, "d_table", true},
                           {d_cells, "d_cells", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_cells) RPL_HIP(h, hipMemsetAsync(d_cells, 0, (size_t)G * 16u, h->stream));
  RPL_HIP(h, rpl::launch_inflate(h->stream, d_in, in_stride, d_out, out_stride, G, width, height, d_table, rc,
                                 inflate_unknown, d_cells));
  return RPLGPU_OK;
}

int32_t rplgpu_inflate_grid(rplgpu_handle_t h, const int8_t *in, uint32_t width, uint32_t height, float resolution,
                            const rplgpu_inflation_t *f, int8_t *out, uint32_t cells[4]) {
  if (!h || !in || !out || !f || in == out) return RPLGPU_ERR_INVALID_ARG;
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_inflate_grid: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  std::vector<uint8_t> table((size_t)RPLGPU_MAX_INFLATION_CELLS * RPLGPU_MAX_INFLATION_CELLS + 1u);
  uint32_t reach = 0;
  if (rplgpu_inflation_table(f, resolution, table.data(), (uint32_t)table.size(), &reach) != RPLGPU_OK) {
    h->err = "rplgpu_inflate_grid: invalid rplgpu_inflation_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)width * height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t n_table = (size_t)reach * reach + 1u;
  DoorBuffer buf(h, "rplgpu_inflate_grid");
  const size_t o_in = buf.part(stride), o_out = buf.part(stride), o_table = buf.part(n_table), o_cells = buf.part(16);
  uint32_t small[4] = {0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_in), in, cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_table), table.data(), n_table, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_inflate_grids_dev(h, buf.at<const int8_t>(o_in), stride, buf.at<int8_t>(o_out), stride,
                                                 1, width, height, buf.at(o_table), reach, f->inflate_unknown,
                                                 buf.at<uint32_t>(o_cells));
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(out, buf.at(o_out), cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, buf.at(o_cells), 16, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  if (cells) std::memcpy(cells, small, 16);
  return RPLGPU_OK;
}

// ---- E13: a time step's scans matched to a likelihood field (include/rplgpu_msg.h) ---------------------------

void rplgpu_default_scan_match(rplgpu_scan_match_t *m) {
  if (!m) return;
  m->origin_x = -25.6f;
  m->origin_y = -25.6f;
  m->resolution = 0.05f;
  m->width = 1024;
  m->height = 1024;
  m->shift_x = 6;
  m->shift_y = 6;
  m->rot_steps = 10;
  m->rot_step = (float)(0.25 * M_PI / 180.0);
}

int32_t rplgpu_scan_match_check(const rplgpu_scan_match_t *m) {
  return rpl::match_spec_check(m, RPLGPU_MAX_MATCH_SHIFT);
}

int32_t rplgpu_scan_match_rotations(const rplgpu_scan_match_t *m, float *cs) {
  if (!cs || rplgpu_scan_match_check(m) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  const int K = (int)m->rot_steps;
  for (int k = -K; k <= K; ++k) {
    const double a = (double)k * (double)m->rot_step;
    cs[2 * (k + K)] = (float)std::cos(a);
    cs[2 * (k + K) + 1] = (float)std::sin(a);
  }
  return RPLGPU_OK;
}

uint32_t rplgpu_scan_match_volume(const rplgpu_scan_match_t *m) {
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) return 0;
  return (2u * m->rot_steps + 1u) * (2u * m->shift_y + 1u) * (2u * m->shift_x + 1u);
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t match_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                          const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                          const float *d_motion, const float *d_pose2d, const float *d_t0, const float *d_pivot,
                          const rplgpu_scan_match_t *m, const int8_t *d_field, uint64_t field_stride,
                          uint32_t field_per_group, uint32_t *d_scores, uint64_t score_stride, uint32_t *d_best,
                          uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !m || !d_field || !d_scores || !d_best || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_match_scans_dev: invalid rplgpu_scan_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (field_stride < (uint64_t)m->width * m->height || (field_stride & 3u) ||
      (reinterpret_cast<uintptr_t>(d_field) & 3u)) {
    h->err = "rplgpu_match_scans_dev: field_stride must be >= width * height and a multiple of 4, d_field 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint32_t volume = rplgpu_scan_match_volume(m);
  if (score_stride < volume || (reinterpret_cast<uintptr_t>(d_scores) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_best) & 3u) || (reinterpret_cast<uintptr_t>(d_status) & 3u)) {
    h->err = "rplgpu_match_scans_dev: score_stride must be >= the volume size, d_scores / d_best / d_status 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_pivot, "d_pivot", false},
                           {d_field, "d_field", true}, {d_scores, "d_scores", true}, {d_best, "d_best", true},
                           {d_status, "d_status", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  ScanPrologue pro;
  if ((rc = pro.admit(h, "rplgpu_match_scans_dev", p, d_motion, d_t0, B, group))) return rc;
  if ((uint64_t)pro.group * n_stride > (1ull << 24)) {  // 127 x points stays below 2^32: no score wraps
    h->err = "rplgpu_match_scans_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const rpl::MatchK k{m->origin_x, m->origin_y, m->resolution, m->width, m->height,
                      m->shift_x, m->shift_y, m->rot_steps};
  rpl::MatchRot rot;  // at most 129 pairs, handed to the kernel by value: no copy on the stream
  std::memset(&rot, 0, sizeof(rot));
  if (rplgpu_scan_match_rotations(m, rot.cs) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  if ((rc = pro.begin(h, d_nodes, n_stride, d_n_per_scan, B, p, d_t0, d_status))) return rc;
  RPL_HIP(h, rpl::launch_match_prepare(h->stream, d_scores, score_stride, pro.G, k, d_best));
  RPL_HIP(h, rpl::launch_match_score(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T, pro.mask,
                                     kMaskStride, d_motion, d_pose2d, d_pivot, k, rot, d_field, field_stride,
                                     field_per_group, d_scores, score_stride, d_best, d_status));
  RPL_HIP(h, rpl::launch_match_best(h->stream, d_scores, score_stride, pro.G, k, d_best));
  return RPLGPU_OK;
}

int32_t rplgpu_match_scans_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const float *d_pivot,
                               const rplgpu_scan_match_t *m, const int8_t *d_field, uint64_t field_stride,
                               uint32_t field_per_group, uint32_t *d_scores, uint64_t score_stride,
                               uint32_t *d_best, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return match_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, d_pivot, m,
                    d_field, field_stride, field_per_group, d_scores, score_stride, d_best, d_status);
}

int32_t rplgpu_match_scans(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                           const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                           const float *motion, const float *pose2d, const float *t0, const float *pivot,
                           const rplgpu_scan_match_t *m, const int8_t *field, uint32_t *scores_out,
                           uint32_t best[8], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !m || !field || !best || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_match_scans: invalid rplgpu_scan_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)m->width * m->height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t volume = rplgpu_scan_match_volume(m);
  // field | scores | the scans | pivot | best + status
  DoorBuffer buf(h, "rplgpu_match_scans");
  const size_t o_field = buf.part(stride), o_sc = buf.part(4u * volume);
  DoorScans scans(buf, nodes, n_stride, n_per_scan, n_scans, motion, pose2d, t0);
  const size_t o_pv = buf.part_if(pivot, 8), o_small = buf.part(48);
  uint32_t small[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_field), field, cells_n, hipMemcpyHostToDevice, h->stream));
    if (int32_t urc = scans.upload(h, buf)) return urc;
    if (pivot) RPL_HIP(h, hipMemcpyAsync(buf.at(o_pv), pivot, 8u, hipMemcpyHostToDevice, h->stream));
    uint32_t *d_small = buf.at<uint32_t>(o_small);
    const int32_t irc = match_impl(h, scans.d_nodes, n_stride, scans.d_n_per_scan, n_scans, n_scans, p, scans.d_motion,
                                   scans.d_pose2d, scans.d_t0, buf.at<const float>(o_pv), m,
                                   buf.at<const int8_t>(o_field), stride, 0, buf.at<uint32_t>(o_sc), volume, d_small,
                                   d_small + 8);
    if (irc) return irc;
    if (scores_out)
      RPL_HIP(h, hipMemcpyAsync(scores_out, buf.at(o_sc), 4u * volume, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 36, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(best, small, 32);
  if (status) *status = small[8];
  return RPLGPU_OK;
}

// ---- E14: time steps accumulated into a hit / miss map at matched poses (include/rplgpu_msg.h) ----------------

void rplgpu_default_map_rule(rplgpu_map_rule_t *rule) {
  if (!rule) return;
  rule->min_observations = 2;
  rule->occupied_percent = 10;
  rule->mode = 0;
}

int32_t rplgpu_map_rule_check(const rplgpu_map_rule_t *rule) {
  if (!rule || rule->min_observations == 0 || rule->occupied_percent > 100u || rule->mode > 1u)
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t map_update_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const float *d_t0,
                               const rplgpu_occ_grid_t *grid, uint32_t *d_counts, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !grid || !d_counts || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_map_update_dev: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(d_counts) & 7u) || (reinterpret_cast<uintptr_t>(d_status) & 3u)) {
    h->err = "rplgpu_map_update_dev: d_counts must be 8-byte aligned, d_status 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_motion, "d_motion", false}, {d_pose2d, "d_pose2d", false}, {d_counts, "d_counts", true},
                           {d_status, "d_status", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  ScanPrologue pro;
  if ((rc = pro.admit(h, "rplgpu_map_update_dev", p, d_motion, d_t0, B, group))) return rc;
  if ((uint64_t)pro.group * std::min(n_stride, rpl::kMaxN) > (1ull << 24)) {
    h->err = "rplgpu_map_update_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_CAPACITY;
  }
  if ((rc = pro.begin(h, d_nodes, n_stride, d_n_per_scan, B, p, d_t0, d_status))) return rc;
  RPL_HIP(h, rpl::launch_map_walk(h->stream, d_nodes, n_stride, d_n_per_scan, B, pro.group, pro.kp, pro.T, pro.mask,
                                  kMaskStride, d_motion, d_pose2d, occ_kernel_args(*grid), d_counts, d_status));
  return RPLGPU_OK;
}

int32_t rplgpu_map_update_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                              const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                              const float *d_motion, const float *d_pose2d, const rplgpu_occ_grid_t *grid,
                              uint32_t *d_counts, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return map_update_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, grid,
                         d_counts, d_status);
}

int32_t rplgpu_map_grid_dev(rplgpu_handle_t h, const uint32_t *d_counts, uint32_t width, uint32_t height,
                            const rplgpu_map_rule_t *rule, const int8_t *d_prev, int8_t *d_grid,
                            uint64_t grid_stride, uint32_t *d_cells) {
  if (!h || !d_counts || !rule || !d_grid) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_map_rule_check(rule) != RPLGPU_OK) {
    h->err = "rplgpu_map_grid_dev: invalid rplgpu_map_rule_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_map_grid_dev: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (grid_stride < (uint64_t)width * height || (grid_stride & 3u) || (reinterpret_cast<uintptr_t>(d_grid) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_counts) & 7u) || (reinterpret_cast<uintptr_t>(d_cells) & 3u)) {
    h->err = "rplgpu_map_grid_dev: grid_stride must be >= width * height and a multiple of 4, d_grid / d_cells 4-byte and d_counts 8-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_prev == d_grid) {
    h->err = "rplgpu_map_grid_dev: d_prev must not be d_grid";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_counts, "d_counts", true}, {d_prev, "d_prev", false}, {d_grid, "d_grid", true},
                           {d_cells, "d_cells", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_cells) RPL_HIP(h, hipMemsetAsync(d_cells, 0, 16u, h->stream));
  RPL_HIP(h, rpl::launch_map_grid(h->stream, d_counts, width, height, rule->min_observations,
                                  rule->occupied_percent, rule->mode, d_prev, d_grid, d_cells));
  return RPLGPU_OK;
}

int32_t rplgpu_apply_match_dev(rplgpu_handle_t h, const uint32_t *d_best, const rplgpu_scan_match_t *m,
                               const float *d_pivot, const float *d_pose2d_in, uint32_t B, uint32_t group,
                               uint32_t flags, float *d_pose2d_out, float *d_pivot_out) {
  if (!h || !d_best || !m || !d_pose2d_out || group == 0 || flags > 1u) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_apply_match_dev: invalid rplgpu_scan_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(d_best) & 3u) || (reinterpret_cast<uintptr_t>(d_pivot) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_pose2d_in) & 3u) || (reinterpret_cast<uintptr_t>(d_pose2d_out) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_pivot_out) & 3u)) {
    h->err = "rplgpu_apply_match_dev: every pointer must be 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_pivot_out && d_pivot_out == d_pivot) {
    h->err = "rplgpu_apply_match_dev: d_pivot_out must not be d_pivot (every scan of a group reads the pivot)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B > h->max_b) {
    h->err = "batch larger than max_batch given to rplgpu_create";
    return RPLGPU_ERR_CAPACITY;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, {{d_best, "d_best", true}, {d_pivot, "d_pivot", false}, {d_pose2d_in, "d_pose2d_in", false},
                           {d_pose2d_out, "d_pose2d_out", true}, {d_pivot_out, "d_pivot_out", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  group = std::min(group, B);
  const rpl::MatchK k{m->origin_x, m->origin_y, m->resolution, m->width, m->height,
                      m->shift_x, m->shift_y, m->rot_steps};
  rpl::MatchRot rot;  // by value, as k_match_score takes it
  std::memset(&rot, 0, sizeof(rot));
  if (rplgpu_scan_match_rotations(m, rot.cs) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_apply_match(h->stream, d_best, k, rot, d_pivot, d_pose2d_in, B, group, flags, d_pose2d_out,
                                     d_pivot_out));
  return RPLGPU_OK;
}

int32_t rplgpu_map_update(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                          const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                          const float *motion, const float *pose2d, const float *t0, const rplgpu_occ_grid_t *grid,
                          uint32_t *counts, uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !grid || !counts || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_map_update: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)grid->width * grid->height;
  // counts | the scans | status
  DoorBuffer buf(h, "rplgpu_map_update");
  const size_t o_counts = buf.part(8u * cells_n);
  DoorScans scans(buf, nodes, n_stride, n_per_scan, n_scans, motion, pose2d, t0);
  const size_t o_small = buf.part(16);
  uint32_t small = 0;
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_counts), counts, 8u * cells_n, hipMemcpyHostToDevice, h->stream));
    if (int32_t urc = scans.upload(h, buf)) return urc;
    uint32_t *d_small = buf.at<uint32_t>(o_small);
    const int32_t irc = map_update_impl(h, scans.d_nodes, n_stride, scans.d_n_per_scan, n_scans, n_scans, p,
                                        scans.d_motion, scans.d_pose2d, scans.d_t0, grid, buf.at<uint32_t>(o_counts),
                                        d_small);
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(counts, buf.at(o_counts), 8u * cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(&small, d_small, 4, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  if (status) *status = small;
  return RPLGPU_OK;
}

int32_t rplgpu_map_grid(rplgpu_handle_t h, const uint32_t *counts, uint32_t width, uint32_t height,
                        const rplgpu_map_rule_t *rule, const int8_t *prev, int8_t *grid_out, uint32_t cells[4]) {
  if (!h || !counts || !rule || !grid_out) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_map_rule_check(rule) != RPLGPU_OK) {
    h->err = "rplgpu_map_grid: invalid rplgpu_map_rule_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_map_grid: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)width * height, stride = (cells_n + 3u) & ~(size_t)3u;
  DoorBuffer buf(h, "rplgpu_map_grid");
  const size_t o_counts = buf.part(8u * cells_n), o_grid = buf.part(stride), o_prev = buf.part_if(prev, stride),
               o_small = buf.part(16);
  uint32_t small[4] = {0, 0, 0, 0};
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_counts), counts, 8u * cells_n, hipMemcpyHostToDevice, h->stream));
    if (prev) RPL_HIP(h, hipMemcpyAsync(buf.at(o_prev), prev, cells_n, hipMemcpyHostToDevice, h->stream));
    const int32_t irc = rplgpu_map_grid_dev(h, buf.at<const uint32_t>(o_counts), width, height, rule,
                                            buf.at<const int8_t>(o_prev), buf.at<int8_t>(o_grid), stride,
                                            buf.at<uint32_t>(o_small));
    if (irc) return irc;
    RPL_HIP(h, hipMemcpyAsync(grid_out, buf.at(o_grid), cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, buf.at(o_small), 16, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  if (cells) std::memcpy(cells, small, 16);
  return RPLGPU_OK;
}

}  // extern "C"
