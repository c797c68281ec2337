// rpl_launch.hpp — host-callable launchers of the gfx950 kernels (rpl_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rplgpu_comm.h"
#include "rpl_device.hpp"
#include "rpl_msg.hpp"
#include "rpl_rules.hpp"

namespace rplmsg {
struct Prefix;
}

namespace rpl {

// Internal status bits, what a kernel leaves in a status word for the host code behind it.  kAscendUnsorted: a
// scan that launch_ascend(..., defer_sort) left for launch_ascend_sort (the sorting kernel rewrites the word
// without it).  kRorListedBit: a work item the voxel kernel's ROR instance left to the two kernels (the listed
// launches overwrite it; the single-scan entry points look for it instead of launching them blind).  The shared
// value is safe: the one is only ever written to an ascend status word, the other to a cloud status word, and
// both are cleared before the word reaches the caller.
constexpr uint32_t kAscendUnsorted = 0x80000000u;
constexpr uint32_t kRorListedBit = 0x80000000u;
constexpr uint32_t kScanStatusBits =
    RPLGPU_SCAN_ALL_INVALID | RPLGPU_SCAN_CELL_RANGE | RPLGPU_SCAN_TABLE_FULL | RPLGPU_SCAN_OUT_TRUNCATED;
static_assert((kAscendUnsorted & kScanStatusBits) == 0, "internal ascend bit overlaps RPLGPU_SCAN_*");
static_assert((kRorListedBit & kScanStatusBits) == 0, "internal cloud bit overlaps RPLGPU_SCAN_*");
// `need_sort`: B + 1 words of scratch (how many / which scans the second, sorting kernel has to redo)
hipError_t launch_ascend(hipStream_t s, void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                         uint32_t B, uint32_t *status, uint32_t *need_sort, bool defer_sort = false,
                         uint32_t *sort_stat = nullptr);
hipError_t launch_ascend_sort(hipStream_t s, void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                              uint32_t B, uint32_t *status, uint32_t *need_sort,
                              uint32_t *sort_stat = nullptr);
// publish_scan Mode A (rpl_laserscan.hip); `fast`: the mul+2*FMA divides were validated
// A single scan straight into its serialised sensor_msgs/LaserScan (Mode A, validated fast
// divides): the kernel writes the message prefix, patches stamp / scalars / array lengths and
// flushes its bins to the two arrays' places inside the message — no ranges / intensities in HBM,
// no second kernel.  msg: device view of a (pinned, 4-byte aligned) buffer that holds the worst
// case; msg_len: device word receiving the length (0: nothing published).
struct LsMsgOut {
  rplmsg::Prefix P;
  uint32_t *msg;
  uint32_t *msg_len;
  int32_t sec;
  uint32_t nanosec;
  double scan_duration;
};
hipError_t launch_laserscan_a(hipStream_t s, const void *nodes, uint32_t n_stride,
                              const uint32_t *n_per_scan, uint32_t B, const KParams &p,
                              const Tables &T, const float *inc_table, const float *rinc_table,
                              bool fast, float *ranges, float *intens, uint32_t *beam_count,
                              uint32_t n_given = 0xFFFFFFFFu, const LsMsgOut *msg_out = nullptr);
hipError_t launch_validate_idx(hipStream_t s, const Tables &T, const float *inc_table,
                               const float *rinc_table, uint32_t max_count,
                               uint32_t *d_mismatches);
// publish_scan Mode B (rpl_kernels.hip)
hipError_t launch_laserscan_raw(hipStream_t s, const void *nodes, uint32_t n_stride,
                                const uint32_t *n_per_scan, uint32_t B, const KParams &p,
                                float *ranges, float *intens, uint32_t *beam_count);
// The plain cloud (E1 .. E3, E5 by mask; the voxelised one: launch_cloud_voxel).
// `keepmask` (optional): one bit per sample from launch_ror_mask, `mask_stride` words per scan.
hipError_t launch_cloud(hipStream_t s, const void *nodes, uint32_t n_stride,
                        const uint32_t *n_per_scan, uint32_t B, const KParams &p, const Tables &T,
                        const uint32_t *keepmask, uint32_t mask_stride, float *xyzi,
                        uint32_t out_stride, uint32_t *n_points, uint32_t *status,
                        const float *motion = nullptr);  // E6 de-skew
// One launch of the voxel kernel (rpl_voxel.hip).  What the arena holds: 16-byte points, 12-byte points
// (x, y, intensity: the exchange payload), 32-byte cell records (rplgpu_cell_t)
enum class ArenaForm : int { kXyzi = 0, kXyi = 1, kCells = 2 };
// E5 (round 6): not in the kernel (`keepmask`, if given, is all of it), inside the pass (validated divides; items
// it cannot settle go on T.redo), the items of T.redo with `keepmask`
enum class RorMode : int { kNone = 0, kInside = 1, kListed = 2 };
struct VoxelLaunch {
  // input: B scans of n_per_scan[b] samples, n_stride apart (the first four members, in this order)
  const void *nodes = nullptr;
  uint32_t n_stride = 0;
  const uint32_t *n_per_scan = nullptr;
  uint32_t B = 0;
  // E8: `group` consecutive scans share one grid; per-scan motion (vx, vy, wz, dt) and planar pose
  // (r00 r01 tx r10 r11 ty), optional
  uint32_t group = 1;
  const float *motion = nullptr, *pose2d = nullptr;
  // (optional) one bit per sample from launch_ror_mask, `mask_stride` words per scan
  const uint32_t *keepmask = nullptr;
  uint32_t mask_stride = 0;
  RorMode ror = RorMode::kNone;
  // output: per-scan regions xyzi + b * out_stride, or (arena given) one arena in which item b is
  // arena[scan_start[b] .. + n_points[b]) and *arena_cursor ends up as the total
  float *xyzi = nullptr;
  uint32_t out_stride = 0;
  float *arena = nullptr;
  uint64_t arena_capacity = 0;
  uint64_t *arena_cursor = nullptr, *scan_start = nullptr;
  ArenaForm form = ArenaForm::kXyzi;
  uint32_t *n_points = nullptr, *status = nullptr;  // per work item
};
hipError_t launch_cloud_voxel(hipStream_t s, const VoxelLaunch &v, const KParams &p, const Tables &T);
// record stores k_cloud_voxel needs: one per resident workgroup (two per CU) ...
uint32_t voxel_max_workgroups(uint32_t n_cu);
// ... of this many 16-byte entries for work items of `group` scans of `n_stride` samples: every
// sample can end a run record, and every block of 128 samples adds one marker entry
// (two per block: the noisy-batch instance aggregates a block in two classes, each behind its own marker)
// (round 6: the ROR instance's blocks own 124 samples, and a sample E5 settles late brings its own marker:
// at most 2 x (256 + 8) entries per scan)
inline uint64_t voxel_store_need(uint32_t group, uint32_t n_stride) {
  const uint64_t s = n_stride < kMaxN ? n_stride : kMaxN;
  return (uint64_t)(group ? group : 1u) * (s + 2u * ((s + 123u) / 124u) + 1u + 528u);
}
// `listed`: the scans of the work items on T.redo (count word, then item numbers; an item = `group`
// consecutive scans) instead of all B scans: a persistent grid that reads the count on the device
hipError_t launch_ror_mask(hipStream_t s, const void *nodes, uint32_t n_stride,
                           const uint32_t *n_per_scan, uint32_t B, const KParams &p,
                           const Tables &T, uint32_t *mask, uint32_t mask_stride,
                           bool listed = false, uint32_t group = 1);
hipError_t launch_validate_div(hipStream_t s, float d, float rd, uint32_t e_lo, uint32_t e_hi,
                               uint32_t *d_mismatches);
hipError_t launch_pack(hipStream_t s, const float *xyzi, uint32_t out_stride,
                       const uint32_t *n_points, uint32_t B, float *packed, uint64_t *offsets);

// E7: the binned LaserScan as a cloud (rpl_project.hip)
hipError_t launch_laserscan_to_cloud(hipStream_t s, const float *ranges, const float *intens,
                                     uint32_t n_stride, const uint32_t *beam_count, uint32_t B,
                                     const KParams &p, float *xyzi, uint32_t out_stride,
                                     uint32_t *n_points, uint32_t *status);

// multi-GPU exchange, device side (rpl_comm.hip)
hipError_t launch_signal(hipStream_t s, uint32_t *flag, uint32_t seq);
hipError_t launch_stage_in(hipStream_t s, const void *src, void *dst, uint32_t n_words2);  // 8-byte words
hipError_t launch_pack_meta(hipStream_t s, const unsigned long long *cursor,
                            const unsigned long long *scan_start, const uint32_t *n_points,
                            uint32_t B, unsigned long long slot_points, uint32_t max_scans,
                            uint32_t *meta);
hipError_t launch_unpack_gathered(hipStream_t s, const float *points_all,
                                  unsigned long long slot_points, const uint32_t *meta_all,
                                  uint32_t meta_words, uint32_t world, uint32_t max_scans,
                                  float *packed, unsigned long long *total,
                                  unsigned long long *scan_start_all, uint32_t *n_points_all,
                                  uint32_t *status, uint32_t n_cu, bool xyi = false);
// rpl_cells.hip: gathered cell records (rplgpu_cell_t) -> one fused grid per group; `unit` = 2^-K,
// `scratch` = world x slot_cells words (see rplgpu_merge_cells_dev)
hipError_t launch_merge_cells(hipStream_t s, const void *cells_all, unsigned long long slot_cells,
                              const uint32_t *meta_all, uint32_t meta_words, uint32_t world,
                              uint32_t n_groups, double unit, float *arena,
                              unsigned long long capacity, unsigned long long *cursor,
                              unsigned long long *group_start, uint32_t *n_points, uint32_t *status,
                              uint32_t *scratch, uint32_t n_cu);
hipError_t launch_pack_xyi(hipStream_t s, const float *arena, const unsigned long long *cursor,
                           unsigned long long slot_points, float *slot, uint32_t n_cu);

// decode stage (rpl_decode.hip)
// One decode call (k_decode): B recorded answer streams of one answer type.
struct DecodeLaunch {
  int ans = 0;
  // input: stream b at bytes + b * stream_stride, n_frames[b] <= max_frames frames; back to back, or
  // (frame_off given) at frame_off[b * max_frames + k], gap[..] != 0 where bytes were rejected in front
  const uint8_t *bytes = nullptr;
  uint64_t stream_stride = 0;
  const uint32_t *frame_off = nullptr;
  const uint8_t *gap = nullptr;
  const uint32_t *n_frames = nullptr;
  uint32_t max_frames = 0, B = 0, sample_duration_us = 0;
  // decoder state carried from call to call, four words per stream (optional)
  const int32_t *state_in = nullptr;
  int32_t *state_out = nullptr;
  // launch_decode: the node streams, node_stride apart, with the reset-request list and (optional)
  // the sync-node list of each
  void *nodes = nullptr;
  uint32_t node_stride = 0;
  uint32_t *n_nodes = nullptr;
  uint32_t *reset_at = nullptr;
  uint32_t reset_stride = 0;
  uint32_t *n_reset = nullptr;
  uint32_t *sync_at = nullptr;
  uint32_t sync_stride = 0;
  uint32_t *n_sync = nullptr;
  // per stream (optional)
  uint32_t *n_errors = nullptr, *status = nullptr;
  // launch_decode_fused: completed scans of at most max_count nodes straight into the batch (scan s of
  // stream b at slot b * scan_cap + s, n_stride nodes apart); todo[b] = 1 for a stream it could not
  // take (more sync nodes or reset requests than its tables hold)
  uint32_t max_count = 0;
  void *batch = nullptr;
  uint32_t n_stride = 0, scan_cap = 0;
  uint32_t *n_per_scan = nullptr, *n_scans = nullptr, *todo = nullptr;
  // launch_decode: streams with only[b] == 0 are skipped (null: all)
  const uint32_t *only = nullptr;
  // capsule streams that fit: the LDS-staged instance (rpl_decode.hip); with frame offsets
  // launch_decode needs B words of scratch for the streams it leaves to the plain kernel
  bool staged_ok = true;
  uint32_t *stage_todo = nullptr;
};
hipError_t launch_decode(hipStream_t s, const DecodeLaunch &d);
bool decode_fusable(int ans);
hipError_t launch_decode_fused(hipStream_t s, const DecodeLaunch &d);
hipError_t launch_segment(hipStream_t s, const void *nodes, uint32_t node_stride,
                          const uint32_t *n_nodes, const uint32_t *reset_at, uint32_t reset_stride,
                          const uint32_t *n_reset, uint32_t B, uint32_t max_count, void *out_nodes,
                          uint32_t out_stride, uint32_t *scan_off, uint32_t scan_cap,
                          uint32_t *n_scans, uint32_t *status, const uint32_t *sync_at = nullptr,
                          uint32_t sync_stride = 0, const uint32_t *n_sync = nullptr);
// decoder's sync list + node stream -> completed scans in batch slots b*scan_cap + s
hipError_t launch_assemble(hipStream_t s, const void *nodes, uint32_t node_stride,
                           const uint32_t *n_nodes, const uint32_t *sync_at, uint32_t sync_stride,
                           const uint32_t *n_sync, const uint32_t *reset_at, uint32_t reset_stride,
                           const uint32_t *n_reset, uint32_t B, uint32_t max_count, void *batch,
                           uint32_t n_stride, uint32_t scan_cap, uint32_t *n_per_scan,
                           uint32_t *n_scans, uint32_t *status, const uint32_t *only = nullptr,
                           // the scan open at a call boundary (rplgpu_decode_scans_carry_dev), or nulls
                           const void *carry_in = nullptr, void *carry_out = nullptr,
                           const uint32_t *carry_len_in = nullptr, uint32_t *carry_len_out = nullptr,
                           uint32_t carry_stride = 0);
uint32_t decode_sync_stride();
hipError_t launch_scans_to_batch(hipStream_t s, const void *seg_nodes, uint32_t seg_stride,
                                 const uint32_t *scan_off, uint32_t scan_cap,
                                 const uint32_t *n_scans, uint32_t B, uint32_t *scan_base,
                                 void *batch, uint32_t n_stride, uint32_t max_scans,
                                 uint32_t *n_per_scan);
uint32_t decode_max_frames(int ans);
uint32_t decode_staged_frames(int ans);  // largest max_frames of a back-to-back call the LDS-staged decoder takes

// serialised-message assembly (rpl_msg.hip)
hipError_t launch_msg_laserscan(hipStream_t s, const float *ranges, const float *intens,
                                uint32_t n_stride, const uint32_t *beam_count, uint32_t B,
                                int scan_processing, const rplgpu_stamp_t *stamps,
                                const double *scan_duration, const rplmsg::Prefix &P,
                                uint8_t *msgs, uint32_t msg_stride, uint32_t *msg_len,
                                uint32_t *status);
hipError_t launch_msg_cloud(hipStream_t s, const float *xyzi, uint32_t out_stride,
                            uint32_t max_points, const unsigned long long *scan_start,
                            const uint32_t *n_points, uint32_t B, const rplgpu_stamp_t *stamps,
                            const rplmsg::Prefix &P, uint8_t *msgs, uint32_t msg_stride,
                            uint32_t *msg_len, uint32_t *status);

hipError_t launch_msg_fused(hipStream_t s, const float *arena,
                            const unsigned long long *total_points,
                            unsigned long long arena_capacity, rplgpu_stamp_t stamp,
                            const rplmsg::Prefix &P, uint8_t *msg, unsigned long long msg_capacity,
                            unsigned long long *msg_len, uint32_t *status);
// several sensors into one frame (rpl_fuse.hip)
hipError_t launch_transform_clouds(hipStream_t s, float *xyzi, uint32_t out_stride,
                                   uint32_t max_points, const unsigned long long *scan_start,
                                   const uint32_t *n_points, uint32_t B, const float *pose);

// E9: the scans of a group merged into one LaserScan (rpl_merge.hip, include/rplgpu_msg.h)
constexpr uint32_t kMergeMaxBeams = RPLGPU_MAX_MERGE_BEAMS;
constexpr uint32_t kMergeSlotBits = 17;  // key: r2 bits << 32 | slot << 15 | sample index
struct MergeK {
  const float2 *edges;  // e_0 .. e_count (host-built, rplgpu_scan_merge_edges)
  uint32_t count;
  uint32_t monotone;    // 1: every step e_k -> e_k+1 and every quarter below turns by (0, pi) (host-checked)
  uint32_t qb[5];       // quarter boundaries k = q * count / 4
  float2 qe[5];         // their edge vectors
  float a0;             // angle_min reduced to [0, 2 pi) (the first guess only)
  float rinc;           // 1 / inc (the first guess only)
  float range_min, range_max;
};
hipError_t launch_merge_scans(hipStream_t s, const void *nodes, uint32_t n_stride,
                              const uint32_t *n_per_scan, uint32_t B, uint32_t group, const KParams &p,
                              const Tables &T, const uint32_t *keepmask, uint32_t mask_stride,
                              const float *motion, const float *pose2d, const MergeK &mk,
                              unsigned long long *keys, uint32_t *status);
hipError_t launch_merge_finish(hipStream_t s, unsigned long long *keys, uint32_t G, uint32_t count,
                               const void *nodes, uint32_t n_stride, uint32_t group, int is_new_protocol,
                               float *ranges, float *intens, uint32_t *beams_hit);
hipError_t launch_msg_merged(hipStream_t s, const float *ranges, const float *intens, uint32_t count,
                             uint32_t G, const rplgpu_stamp_t *stamps, const rplmsg::Prefix &P,
                             uint8_t *msgs, uint32_t msg_stride, uint32_t *msg_len, uint32_t *status);

// E10: scan-shadow and speckle filters on LaserScan arrays (rpl_filter.hip, include/rplgpu_msg.h)
constexpr uint32_t kFilterIncModeB = 0;  // inc per scan from its beam count, denominator max(count - 1, 1)
constexpr uint32_t kFilterIncModeA = 1;  // ... denominator count
constexpr uint32_t kFilterIncGiven = 2;  // FilterK::inc as it stands
struct FilterK {
  uint32_t shadow, speckle, circular;
  uint32_t W, N, L;
  float D;
  float cmin, smin, cmax, smax;  // rplgpu_scan_filter_check's dirs
  uint32_t inc_mode;
  float inc;
  uint32_t count;                // beams of every scan when there is no beam_count array
};
// beam_count == nullptr: B scans of k.count beams each, n_stride apart (the E9 layout with n_stride = count);
// removed (optional): 2 words per scan, cleared by the caller
hipError_t launch_filter_scans(hipStream_t s, const float *ranges, const float *intens, uint32_t n_stride,
                               const uint32_t *beam_count, uint32_t B, const FilterK &k, float *ranges_out,
                               float *intens_out, uint32_t *removed);

// E11: one ray-cast occupancy grid per group of scans (rpl_occ.hip, include/rplgpu_msg.h).  The grid is its
// own scratch: prepare zeroes the cells, walk ORs clear / mark bits into their bytes, finish maps the bytes
// to 100 / 0 / prev-or--1 and counts them (cells: 3 words per group, cleared by the caller; may be null).
struct OccK {  // a checked rplgpu_occ_grid_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  float range_min, obstacle_max, raytrace_max;
};
hipError_t launch_occ_prepare(hipStream_t s, int8_t *grid, unsigned long long grid_stride, uint32_t G,
                              const OccK &k);
hipError_t launch_occ_walk(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                           uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                           const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                           const float *pose2d, const OccK &k, int8_t *grid, unsigned long long grid_stride,
                           uint32_t *status);
hipError_t launch_occ_finish(hipStream_t s, int8_t *grid, unsigned long long grid_stride, uint32_t G,
                             const OccK &k, const int8_t *prev, uint32_t *cells);
hipError_t launch_msg_occupancy(hipStream_t s, const int8_t *grid, unsigned long long grid_stride,
                                uint32_t n_cells, uint32_t G, const rplgpu_stamp_t *stamps,
                                const rplmsg::Prefix &P, uint8_t *msgs, uint32_t msg_stride, uint32_t *msg_len,
                                uint32_t *status);

// E12: the costmap inflation layer over G grids (rpl_inflate.hip, include/rplgpu_msg.h): one gather launch,
// `table` rc * rc + 1 cost bytes by squared cell distance, cells: 4 words per grid, cleared by the caller;
// may be null.
hipError_t launch_inflate(hipStream_t s, const int8_t *in, unsigned long long in_stride, int8_t *out,
                          unsigned long long out_stride, uint32_t G, uint32_t width, uint32_t height,
                          const uint8_t *table, uint32_t rc, uint32_t inflate_unknown, uint32_t *cells);

// E13: correlative scan matching of groups of scans against a likelihood field (rpl_match.hip,
// include/rplgpu_msg.h).  The score volume is the call's scratch: prepare zeroes the volumes and the eight
// result words of every group, score adds the field values under the points into the volumes (and the finite
// points into result word 4), best reduces a volume to the other seven words.
struct MatchK {  // a checked rplgpu_scan_match_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  uint32_t tx, ty, rot;
};
struct MatchRot {  // rplgpu_scan_match_rotations: (cos, sin) of k * rot_step at 2 (k + K), by value
  float cs[2u * (2u * RPLGPU_MAX_MATCH_ROT + 1u)];
};
uint32_t match_volume(const MatchK &k);
hipError_t launch_match_prepare(hipStream_t s, uint32_t *scores, unsigned long long score_stride, uint32_t G,
                                const MatchK &k, uint32_t *best);
hipError_t launch_match_score(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                              uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                              const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                              const float *pose2d, const float *pivot, const MatchK &k, const MatchRot &rot,
                              const int8_t *field, unsigned long long field_stride, uint32_t field_per_group,
                              uint32_t *scores, unsigned long long score_stride, uint32_t *best,
                              uint32_t *status);
hipError_t launch_match_best(hipStream_t s, const uint32_t *scores, unsigned long long score_stride, uint32_t G,
                             const MatchK &k, uint32_t *best);

// E14: the persistent hit / miss count map, its cell rule and E13's result applied to the poses (rpl_map.hip,
// include/rplgpu_msg.h).  walk ADDS the rays of all B scans into the one map (two uint32 per cell, misses then
// hits; `group` only picks the status word); grid turns the counts into the int8 grid of E11's layout (cells:
// 4 words, cleared by the caller; may be null); apply composes each group's (k, j, i) in front of its poses.
hipError_t launch_map_walk(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                           uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                           const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                           const float *pose2d, const OccK &k, uint32_t *counts, uint32_t *status);
hipError_t launch_map_grid(hipStream_t s, const uint32_t *counts, uint32_t width, uint32_t height,
                           uint32_t min_observations, uint32_t occupied_percent, uint32_t mode, const int8_t *prev,
                           int8_t *grid, uint32_t *cells);
hipError_t launch_apply_match(hipStream_t s, const uint32_t *best, const MatchK &k, const MatchRot &rot,
                              const float *pivot, const float *pose_in, uint32_t B, uint32_t group, uint32_t flags,
                              float *pose_out, float *pivot_out);

// E15: a list of arbitrary poses weighed against a likelihood field (rpl_pose.hip, include/rplgpu_msg.h).  The
// weights are the call's scratch and result: prepare zeroes the P weights and the eight result words of every
// group, score adds the field values under the points into the weights (and the finite points into result word
// 4), best reduces the weights to the other seven words.
struct PoseK {  // a checked rplgpu_pose_score_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
};
hipError_t launch_pose_prepare(hipStream_t s, uint32_t *weights, unsigned long long weight_stride, uint32_t G,
                               uint32_t P, uint32_t *result);
hipError_t launch_pose_score(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                             uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                             const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                             const float *pose2d, const PoseK &k, const float *poses, uint32_t P,
                             unsigned long long pose_stride, uint32_t poses_per_group, const int8_t *field,
                             unsigned long long field_stride, uint32_t field_per_group, uint32_t *weights,
                             unsigned long long weight_stride, uint32_t *result, uint32_t *status);
hipError_t launch_pose_best(hipStream_t s, const uint32_t *weights, unsigned long long weight_stride, uint32_t G,
                            uint32_t P, uint32_t *result);

// E16: a weighted pose list resampled and moved (rpl_resample.hip, include/rplgpu_msg.h).  Three launches on the
// stream: per-tile sums into the scratch, one workgroup per group for the scan, the tile boundaries and result
// words 0 - 5 and 7, then the outputs, the ancestors and word 6.  The scratch holds resample_scratch_words(G, P)
// uint32 words (0 for a G or P that the call refuses) and is 8-byte aligned.
unsigned long long resample_scratch_words(uint32_t G, uint32_t P);
hipError_t launch_resample(hipStream_t s, const uint32_t *weights, unsigned long long weight_stride,
                           const float *poses, unsigned long long pose_stride, uint32_t poses_per_group, uint32_t G,
                           uint32_t P, uint32_t M, const uint32_t *u, const float *delta, uint32_t n_delta,
                           unsigned long long delta_stride, uint32_t delta_per_group, float *out,
                           unsigned long long out_stride, uint32_t *ancestors, unsigned long long anc_stride,
                           uint32_t *result, uint32_t *scratch);

// E17: a weighted pose list reduced to the sums of a pose estimate (rpl_estimate.hip, include/rplgpu_msg.h).  Two
// launches on the stream: per-tile sums and counts into the scratch, then one workgroup per group for the
// RPLGPU_ESTIMATE_WORDS result words.  weights and center may be null (w = 1, centre 0).  The scratch holds
// estimate_scratch_words(G, P) uint32 words (0 for a G or P that the call refuses) and is 8-byte aligned.
unsigned long long estimate_scratch_words(uint32_t G, uint32_t P);
hipError_t launch_estimate(hipStream_t s, const float *poses, unsigned long long pose_stride,
                           uint32_t poses_per_group, const uint32_t *weights, unsigned long long weight_stride,
                           uint32_t G, uint32_t P, float xy_scale, unsigned long long gate_r2, long long gate_dot,
                           const uint32_t *center, unsigned long long center_stride, uint32_t *result,
                           uint32_t *scratch);

// E18: a pose list's motion noise drawn on the device (rpl_motion.hip, include/rplgpu_msg.h).  Two launches on the
// stream: the eight result words of every group zeroed, then one thread per output — three Philox4x32-10 blocks, the
// float32 steps of the header, one 16-byte store — and the tile's statistics added to the words with integer atomics.
hipError_t launch_motion(hipStream_t s, const float *odom, uint32_t odom_per_group, uint32_t G, uint32_t M,
                         unsigned long long seed, unsigned long long step, uint32_t first, float *delta,
                         unsigned long long delta_stride, uint32_t *result);

// E19: a pose list seeded over a grid's free cells (rpl_seed.hip, include/rplgpu_msg.h).  Three launches on the
// stream: the free cells of every grid indexed as bit masks with running counts (the scratch), the block counts
// scanned and the result words started, then one thread per output — one Philox4x32-10 block, three bisections to the
// r-th free cell, the float32 steps of the header, one 16-byte store — and the tile's statistics added to the words
// with integer atomics.  seed_scratch_words: uint32 words for n_grids grids; 0 for arguments launch_seed refuses.
struct SeedK {
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  int32_t free_lo, free_hi;
  uint32_t centres;  // flags bit 0: no jitter
};
unsigned long long seed_scratch_words(uint32_t n_grids, uint32_t width, uint32_t height);
hipError_t launch_seed(hipStream_t s, const SeedK &k, const int8_t *grid, unsigned long long grid_stride,
                       uint32_t grid_per_group, const float *headings, uint32_t H, uint32_t G, uint32_t M,
                       unsigned long long seed, unsigned long long step, uint32_t first, float *poses_out,
                       unsigned long long out_stride, uint32_t *cells_out, unsigned long long cell_stride,
                       uint32_t *result, uint32_t *scratch);

// E20: a pose list's occupied bins (rpl_bins.hip, include/rplgpu_msg.h).  Two launches on the stream: the map words
// cleared (not under KEEP) and the result words started, then one thread per pose — one 16-byte load, the float32
// position bin, a bounded bisection over the quantised edge table in LDS, the wave's marks merged per map word, a
// device-scope read and a returning atomic OR only where a bit is missing — and the tile's statistics added to the
// words with integer atomics.  No scratch.  (bin_map_words(nb), the words of a map, is in rpl_rules.hpp.)
struct BinsK {
  float origin_x, origin_y, inv_size;
  uint32_t nx, ny;
  uint32_t keep;  // flags bit 0: OR into the map, do not clear it
};
hipError_t launch_bins(hipStream_t s, const BinsK &k, const float *poses, unsigned long long pose_stride,
                       uint32_t poses_per_group, const uint32_t *weights, unsigned long long weight_stride,
                       uint32_t G, uint32_t P, const float *edges, uint32_t T, uint32_t *map,
                       unsigned long long map_stride, uint32_t *bins_out, unsigned long long bin_stride,
                       uint32_t *result);

// E21: a binned pose list clustered (rpl_clusters.hip, include/rplgpu_msg.h).  Nine launches on the stream: the map's
// words indexed (popcounts and running counts), the block counts scanned, a thread per bin to start and then to link
// the occupied bins' ranks in a parent array (agent-scope atomics only, the larger root hooked under the smaller), the
// roots flattened and counted, a thread per pose for its label and its cluster's weight, one workgroup per group for
// BEST, SECOND and the table rows, then E17's tile reduction and finish over the poses of BEST.  labels and clusters
// may be null.  The scratch holds clusters_scratch_words(G, P, nx, ny, T) uint32 words (0 for arguments the call
// refuses) and is 8-byte aligned.
struct ClustersK {
  uint32_t nx, ny;
  float xy_scale;
  uint32_t wrap;  // flags bit 0: heading bin T - 1 is next to bin 0
};
unsigned long long clusters_scratch_words(uint32_t G, uint32_t P, uint32_t nx, uint32_t ny, uint32_t T);
hipError_t launch_clusters(hipStream_t s, const ClustersK &k, const float *poses, unsigned long long pose_stride,
                           uint32_t poses_per_group, const uint32_t *weights, unsigned long long weight_stride,
                           uint32_t G, uint32_t P, uint32_t T, const uint32_t *map, unsigned long long map_stride,
                           const uint32_t *bins, unsigned long long bin_stride, uint32_t *labels,
                           unsigned long long label_stride, uint32_t *clusters, unsigned long long cluster_stride,
                           uint32_t cluster_cap, uint32_t *result, uint32_t *scratch);

// E22: a beam fan cast from every pose of a list into a grid (rpl_cast.hip, include/rplgpu_msg.h).  Two launches on
// the stream — the cast words of every group started (and result word 4, the measured beams that are not NaN), then
// one thread per ray: the float32 set-up of the header, E11's walk with one grid byte per visit, the range word, the
// beam's table term added to its pose's weight in LDS, the tile's counts by ballots and integer atomics — between
// E15's launch_pose_prepare and launch_pose_best when `measured` is set.  ranges may be null, or measured (with it
// table, weights and result), not both.  No scratch.
struct CastK {  // a checked rplgpu_range_cast_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  uint32_t max_steps;
  int32_t hit_lo;
  uint32_t unknown_stops;
  uint32_t table_half;
};
hipError_t launch_cast(hipStream_t s, const CastK &k, const float *poses, unsigned long long pose_stride,
                       uint32_t poses_per_group, uint32_t G, uint32_t P, const float *beams, uint32_t A,
                       const int8_t *grid, unsigned long long grid_stride, uint32_t grid_per_group,
                       const float *measured, unsigned long long meas_stride, uint32_t meas_first, uint32_t meas_step,
                       const uint8_t *table, uint32_t *ranges, unsigned long long range_stride, uint32_t *weights,
                       unsigned long long weight_stride, uint32_t *result, uint32_t *cast);

}  // namespace rpl
