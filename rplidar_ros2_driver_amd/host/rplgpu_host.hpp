// rplgpu_host.hpp — C++ host side of the MI355X scan path, mirroring the reference's own
// call sites so that the node keeps its ROS 2 surface and only the per-sample loops move.
//
// Reference seams (citations relative to the reference tree):
//   S1  drv_->ascendScanData(buf, count)            src/lidar_driver_wrapper.cpp:329
//         -> rplgpu_host::ScanPath::ascendScanData(buf, count)
//   S3  RPlidarNode::publish_scan body :568-680      src/rplidar_node.cpp
//         -> rplgpu_host::ScanPath::fill_laser_scan(nodes, ..., scan_msg)   (everything up to,
//            but not including, scan_pub_->publish(scan_msg) at :682)
//   ext PointCloud2 (x, y, z, intensity FLOAT32; point_step 16) with clip / radius-outlier /
//         voxel grid -> rplgpu_host::ScanPath::fill_point_cloud2(nodes, ..., cloud_msg)
//   msg the same two, but ending in scan_pub_->publish(const rclcpp::SerializedMessage &):
//         the device results land by DMA inside the serialised (CDR) message, no typed message,
//         no std::vector fills, no middleware serialisation pass (include/rplgpu_msg.h)
//         -> rplgpu_host::ScanPath::fill_serialized_laser_scan / fill_serialized_point_cloud2
//   pre LIDARSampleDataUnpacker::onSampleData -> LIDARSampleDataListener callbacks
//         (src/sdk/src/dataunpacker/dataunpacker.h:48-88) and ScanDataHolder
//         (src/sdk/src/sl_lidar_driver.cpp:272-315), for RECORDED answer streams
//         -> rplgpu_host::ScanPath::replay_recording(ans, bytes, n, listener) /
//            rplgpu_host::ScanAssembler
//   occ the consumer's first loop (a costmap obstacle layer's mark-and-clear over the beams of a time step):
//         -> rplgpu_host::ScanPath::fill_occupancy_grid(scans, ..., grid_msg)   (E11)
//   inf the consumer's second loop (a costmap inflation layer over that grid):
//         -> rplgpu_host::ScanPath::inflate_grid(grid_msg, inflation, costmap_msg)  (E12)
//   nav the planning side's first loop (a navigation function over that costmap, and the paths down it):
//         -> rplgpu_host::ScanPath::nav_field(costmap_msg, rule, goals, potential, result, starts, ...)  (E26)
//         -> rplgpu_host::ScanPath::rollout(costmap_msg, rule, start, deltas, per_step, footprint, potential, ...)  (E27)
//         -> rplgpu_host::ScanPath::mppi_update(rule, rollout_out, rollout_words, deltas, table, nominal, ...)  (E28)
//         -> rplgpu_host::ScanPath::mppi_spread(nominal, noise, K, shift, keep_first, candidates)  (E28)
//         -> rplgpu_host::ScanPath::frontiers(grid_msg, rule, potential, comp_cap, row_cap, result, rows, labels)  (E29)
//   mat the localisation side's loop (a correlative scan matcher's search window over a likelihood field):
//         -> rplgpu_host::ScanPath::match_scans(scans, ..., field_msg, window, result)  (E13)
//         -> rplgpu_host::ScanPath::match_wide(scans, ..., field_msg, window, result)   (E24: up to 256 cells a side)
//         -> rplgpu_host::ScanPath::refine_poses(scans, ..., field_msg, rule, iters, poses, result)   (E25: below a cell)
//   map the mapping side's loop (a map that many time steps vote on, each at its matched pose):
//         -> rplgpu_host::ScanPath::update_map(scans, ..., counts) and fill_map_grid(counts, ..., grid_msg)  (E14)
//   pf  the localisation side's other loop (a particle filter's sensor update over a list of arbitrary poses):
//         -> rplgpu_host::ScanPath::score_poses(scans, ..., field_msg, xyt, weights, result)  (E15)
//         and its step between two sensor updates (the list redrawn by its weights and moved by the odometry):
//         -> rplgpu_host::ScanPath::resample_poses(weights, poses, count, u, delta, poses_out, ancestors, result)  (E16)
//         and what the filter publishes (the weighted list reduced to one pose with a covariance):
//         -> rplgpu_host::ScanPath::estimate_pose(poses, weights, spec, center, estimate)  (E17)
//         and the motion noise that step needs (one delta per output, drawn from the odometry increment):
//         -> rplgpu_host::ScanPath::sample_motion(dx, dy, dtheta, alpha, spec, count, delta, result)  (E18)
//         and the list the loop starts from, or the poses a recovery injects (uniform over a grid's free cells):
//         -> rplgpu_host::ScanPath::seed_poses(spec, grid, headings, noise, count, poses, result)  (E19)
//         and the size of the next list from the bins the list occupies (AMCL's KLD sampling):
//         -> rplgpu_host::ScanPath::bin_poses(spec, poses, weights, headings, map, result)  (E20)
//         and the pose AMCL publishes, the mean of the heaviest cluster of those bins (pf_cluster_stats):
//         -> rplgpu_host::ScanPath::cluster_poses(spec, poses, weights, headings, map, bins, max, clusters, result)  (E21)
//         and the filter's other sensor model, the beam model (a ray from every pose along every beam, map_calc_range):
//         -> rplgpu_host::ScanPath::cast_ranges(spec, poses, beams, grid, measured, first, step, table, ranges, weights, result)  (E22)
//
// Header only, no ROS dependency: the message types are template parameters, so the same
// code compiles against sensor_msgs::msg::LaserScan / PointCloud2 in the node and against
// plain stand-ins in tests.  Everything goes through the C ABI of librplgpu.so
// (include/rplgpu.h); there is no CPU implementation here — on any error the functions return
// false and leave the message untouched, and the caller keeps its own CPU loop as fallback
// (INTEGRATION.md).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace rplgpu_host {

// Any 8-byte node type with the SDK layout (sl_lidar_response_measurement_node_hq_t,
// src/sdk/include/sl_lidar_cmd.h:272-278) can be passed; it is reinterpreted, never copied
// field by field.
template <class NodeT>
inline const rplgpu_node_t *as_nodes(const NodeT *p) {
  static_assert(sizeof(NodeT) == sizeof(rplgpu_node_t), "node must be the packed 8-byte SDK record");
  return reinterpret_cast<const rplgpu_node_t *>(p);
}
template <class NodeT>
inline rplgpu_node_t *as_nodes(NodeT *p) {
  static_assert(sizeof(NodeT) == sizeof(rplgpu_node_t), "node must be the packed 8-byte SDK record");
  return reinterpret_cast<rplgpu_node_t *>(p);
}

// The scalars publish_scan reads from the node (params_, driver_, cached range).
struct ScanConfig {
  bool is_new_protocol = false;     // RealLidarDriver && NEW_TYPE, src/rplidar_node.cpp:577-581
  bool inverted = false;            // params_.inverted, :646,:676
  bool scan_processing = true;      // params_.scan_processing, :632 (code default :280)
  float cached_current_max_range = 12.0f;  // :626
  // extensions (all off == the reference's behaviour)
  bool clip_enable = false;
  uint32_t q_min = 0;
  float range_min = 0.15f;
  bool ror_enable = false;
  float ror_radius = 0.10f;
  uint32_t ror_min_neighbors = 2;
  bool voxel_enable = false;
  float voxel_leaf = 0.05f;

  rplgpu_params_t to_params() const {
    rplgpu_params_t p;
    rplgpu_default_params(&p);
    p.is_new_protocol = is_new_protocol;
    p.inverted = inverted;
    p.scan_processing = scan_processing;
    p.clip_enable = clip_enable;
    p.q_min = q_min;
    p.range_min = range_min;
    p.range_max = cached_current_max_range;
    p.ror_enable = ror_enable;
    p.ror_radius = ror_radius;
    p.ror_min_neighbors = ror_min_neighbors;
    p.voxel_enable = voxel_enable;
    p.voxel_leaf = voxel_leaf;
    return p;
  }
};

// One per node instance (created in on_configure, destroyed in on_cleanup): owns one
// rplgpu handle, i.e. one HIP stream and its staging.  Not thread safe: the node calls it
// from its single scan thread (src/rplidar_node.cpp:222).
class ScanPath {
 public:
  ScanPath() = default;
  ScanPath(const ScanPath &) = delete;
  ScanPath &operator=(const ScanPath &) = delete;
  ~ScanPath() { cleanup(); }

  // on_configure (src/rplidar_node.cpp:116): bind to a device.  The SDK never hands out more
  // than 8192 nodes per scan (src/lidar_driver_wrapper.cpp:316-318).
  // `max_scans`: how many scans one call may hand in (only fill_occupancy_grid takes more than one).
  bool configure(int device_id = 0, uint32_t max_samples_per_scan = 8192, uint32_t max_scans = 1) {
    cleanup();
    const int32_t rc = rplgpu_create(device_id, max_samples_per_scan, max_scans ? max_scans : 1, &h_);
    if (rc != RPLGPU_OK) {
      last_error_ = std::string("rplgpu_create failed (") + std::to_string(rc) + "): " +
                    rplgpu_last_error(nullptr);
      h_ = nullptr;
      return false;
    }
    max_n_ = max_samples_per_scan;
    ranges_.resize(max_n_);
    intens_.resize(max_n_);
    xyzi_.resize(static_cast<size_t>(max_n_) * 4);
    return true;
  }
  // on_cleanup (:244)
  void cleanup() {
    if (h_) rplgpu_destroy(h_);
    h_ = nullptr;
  }
  bool ready() const { return h_ != nullptr; }
  // One scan per call pays a fixed ~21 us (launch + completion flag over PCIe) whatever its size;
  // the reference's loop needs ~7 us for the 360 samples of an A1 and overtakes the device path
  // below ~1700 samples.  Scans shorter than `n` are DECLINED:
  // fill_laser_scan / fill_point_cloud2 return false with last_error() set, i.e. the caller's own
  // CPU loop runs, exactly as after a device error.  0 (the default) declines nothing.
  void set_min_samples(uint32_t n) { min_samples_ = n; }
  uint32_t min_samples() const { return min_samples_; }
  const std::string &last_error() const { return last_error_; }

  // == sl::ILidarDriver::ascendScanData (src/sdk/include/sl_lidar_driver.h:477): in place,
  // returns the SDK's sl_result (0 = SL_RESULT_OK, 0x80008001 = SL_RESULT_OPERATION_FAIL when
  // every node is invalid, buffer untouched).  0x80008000 | other on a device error.
  template <class NodeT>
  uint32_t ascendScanData(NodeT *nodebuffer, size_t count) {
    uint32_t sl_result = 0x80008001u;
    last_error_.clear();
    if (count < min_samples_) {  // declined: the SDK's own loop is faster for a scan this small
      last_error_ = "scan below the configured minimum (CPU loop is faster)";
      return 0x80008002u;
    }
    if (!h_ || rplgpu_ascend(h_, as_nodes(nodebuffer), count, &sl_result) != RPLGPU_OK) {
      note_error();
      return 0x80008002u;  // SL_RESULT_OPERATION_TIMEOUT class: "did not happen"
    }
    return sl_result;
  }

  // == the body of RPlidarNode::publish_scan, src/rplidar_node.cpp:561-680.  Fills every
  // field of `scan_msg` that the reference fills except header.stamp / header.frame_id
  // (:620-621, the caller has them).  Returns false when the reference would have returned
  // without publishing (:561-563, :611-613) or on a device error (see last_error()).
  template <class NodeT, class LaserScanT>
  bool fill_laser_scan(const std::vector<NodeT> &nodes, const ScanConfig &cfg,
                       double scan_duration, LaserScanT &scan_msg) {
    if (nodes.empty()) return false;  // :561-563
    if (!h_ || nodes.size() > max_n_) return fail("scan larger than the configured capacity");
    if (nodes.size() < min_samples_) return fail("scan below the configured minimum (CPU loop is faster)");
    last_error_.clear();
    const rplgpu_params_t p = cfg.to_params();
    rplgpu_scan_meta_t meta;
    if (rplgpu_scan_to_laserscan(h_, as_nodes(nodes.data()), nodes.size(), &p, scan_duration,
                                 ranges_.data(), intens_.data(), &meta) != RPLGPU_OK)
      return note_error();
    if (!meta.published) return false;  // :611-613
    scan_msg.angle_min = meta.angle_min;              // :623
    scan_msg.angle_max = meta.angle_max;              // :624
    scan_msg.range_min = meta.range_min;              // :625
    scan_msg.range_max = meta.range_max;              // :626
    scan_msg.scan_time = meta.scan_time;              // :627
    scan_msg.angle_increment = meta.angle_increment;  // :635 / :666
    scan_msg.time_increment = meta.time_increment;    // :637 / :668
    scan_msg.ranges.assign(ranges_.begin(), ranges_.begin() + meta.count);
    scan_msg.intensities.assign(intens_.begin(), intens_.begin() + meta.count);
    return true;
  }

  // == publish_scan :561-682 for a publisher that sends serialised messages: `out` is an
  // rclcpp::SerializedMessage (or anything with reserve(size_t) and
  // get_rcl_serialized_message() -> {uint8_t *buffer; size_t buffer_length, buffer_capacity}).
  // On success `out` holds the complete CDR-serialised sensor_msgs/msg/LaserScan — header
  // stamp / frame_id (:620-621) included — ready for publish(out).  Same return rule as
  // fill_laser_scan.
  template <class NodeT, class SerializedT>
  bool fill_serialized_laser_scan(const std::vector<NodeT> &nodes, const ScanConfig &cfg,
                                  double scan_duration, const std::string &frame_id, int32_t sec,
                                  uint32_t nanosec, SerializedT &out) {
    if (nodes.empty()) return false;  // :561-563
    if (!h_ || nodes.size() > max_n_) return fail("scan larger than the configured capacity");
    if (nodes.size() < min_samples_) return fail("scan below the configured minimum (CPU loop is faster)");
    last_error_.clear();
    rplgpu_laserscan_layout_t L;
    if (rplgpu_msg_laserscan_layout(frame_id.size(), static_cast<uint32_t>(nodes.size()), &L))
      return fail("frame_id too long");
    out.reserve(L.total_len);  // worst case: every node becomes a beam
    auto &raw = out.get_rcl_serialized_message();
    const rplgpu_params_t p = cfg.to_params();
    rplgpu_scan_meta_t meta;
    size_t len = 0;
    if (rplgpu_scan_to_laserscan_msg(h_, as_nodes(nodes.data()), nodes.size(), &p, scan_duration,
                                     frame_id.c_str(), rplgpu_stamp_t{sec, nanosec}, raw.buffer,
                                     raw.buffer_capacity, &len, &meta) != RPLGPU_OK)
      return note_error();
    raw.buffer_length = len;
    return meta.published != 0;  // :611-613
  }

  // ext: the serialised sensor_msgs/msg/PointCloud2 of fill_point_cloud2.
  template <class NodeT, class SerializedT>
  bool fill_serialized_point_cloud2(const std::vector<NodeT> &nodes, const ScanConfig &cfg,
                                    const std::string &frame_id, int32_t sec, uint32_t nanosec,
                                    SerializedT &out) {
    if (nodes.empty()) return false;
    if (!h_ || nodes.size() > max_n_) return fail("scan larger than the configured capacity");
    if (nodes.size() < min_samples_) return fail("scan below the configured minimum (CPU loop is faster)");
    last_error_.clear();
    rplgpu_cloud_layout_t L;
    if (rplgpu_msg_cloud_layout(frame_id.size(), static_cast<uint32_t>(nodes.size()), &L))
      return fail("frame_id too long");
    out.reserve(L.total_len);
    auto &raw = out.get_rcl_serialized_message();
    const rplgpu_params_t p = cfg.to_params();
    size_t len = 0;
    uint32_t n_points = 0, status = 0;
    if (rplgpu_scan_to_cloud_msg(h_, as_nodes(nodes.data()), nodes.size(), &p, frame_id.c_str(),
                                 rplgpu_stamp_t{sec, nanosec}, raw.buffer, raw.buffer_capacity,
                                 &len, &n_points, &status) != RPLGPU_OK)
      return note_error();
    raw.buffer_length = len;
    return true;
  }

  // == feeding a whole recording of answer type `ans_type` to a fresh
  // sl::internal::LIDARSampleDataUnpacker (onSampleData, dataunpacker.h:79): `listener` gets the
  // calls the SDK's listener would get, in the same order — onHQNodeScanResetReq() and
  // onHQNodeDecoded(timestamp_uS, const node*) (dataunpacker.h:52-56; SlamtecLidarDriver's own
  // implementation is src/sdk/src/sl_lidar_driver.cpp:1645-1653).  Timestamps are 0: the SDK
  // stamps nodes with the decoding host's wall clock, which a recording does not contain.
  // `state` = {last sync bit, last dist_q2, 0, 0} carried between recordings of one sensor
  // (all zero for a fresh unpacker).  `sample_duration_us` = SlamtecLidarTimingDesc::
  // sample_duration_uS.  n_checksum_errors counts ERR_EVENT_ON_EXP_CHECKSUM_ERR events.
  template <class ListenerT>
  bool replay_recording(uint8_t ans_type, uint32_t sample_duration_us, const uint8_t *bytes,
                        size_t nbytes, ListenerT &listener, int32_t state[4],
                        uint32_t *n_checksum_errors = nullptr) {
    if (!h_) return fail("rplgpu handle not configured");
    const size_t S = rplgpu_frame_size(ans_type), npf = rplgpu_nodes_per_frame(ans_type);
    if (!S) return fail("unknown answer type");
    const size_t max_frames = nbytes / S;
    dec_nodes_.resize(max_frames * npf + 1);
    dec_resets_.resize(max_frames + 2);
    size_t n_nodes = 0, n_reset = 0;
    uint32_t n_err = 0;
    int32_t zero[4] = {0, 0, 0, 0};
    if (rplgpu_decode_stream(h_, ans_type, sample_duration_us, bytes, nbytes, state ? state : zero,
                             dec_nodes_.data(), dec_nodes_.size(), &n_nodes, dec_resets_.data(),
                             dec_resets_.size(), &n_reset, &n_err) != RPLGPU_OK)
      return note_error();
    if (n_checksum_errors) *n_checksum_errors = n_err;
    size_t r = 0;
    for (size_t i = 0; i <= n_nodes; ++i) {
      while (r < n_reset && dec_resets_[r] == i) {
        listener.onHQNodeScanResetReq();
        ++r;
      }
      if (i < n_nodes) listener.onHQNodeDecoded(0ull, &dec_nodes_[i]);
    }
    return true;
  }

  // ext: fills a sensor_msgs/PointCloud2-shaped message (fields x, y, z, intensity FLOAT32 at
  // offsets 0/4/8/12, point_step 16, height 1, is_dense, little endian).  `PointFieldT` is
  // sensor_msgs::msg::PointField (datatype 7 == FLOAT32).
  template <class NodeT, class PointCloud2T>
  bool fill_point_cloud2(const std::vector<NodeT> &nodes, const ScanConfig &cfg,
                         PointCloud2T &cloud_msg) {
    if (nodes.empty()) return false;
    if (!h_ || nodes.size() > max_n_) return fail("scan larger than the configured capacity");
    if (nodes.size() < min_samples_) return fail("scan below the configured minimum (CPU loop is faster)");
    last_error_.clear();
    const rplgpu_params_t p = cfg.to_params();
    uint32_t n_points = 0, status = 0;
    const int32_t rc = rplgpu_scan_to_cloud(h_, as_nodes(nodes.data()), nodes.size(), &p,
                                            xyzi_.data(), &n_points, &status);
    if (rc != RPLGPU_OK) return note_error();
    using FieldT = typename std::remove_reference<decltype(cloud_msg.fields)>::type::value_type;
    cloud_msg.fields.clear();
    static const char *const names[4] = {"x", "y", "z", "intensity"};
    for (uint32_t f = 0; f < 4; ++f) {
      FieldT pf;
      pf.name = names[f];
      pf.offset = 4 * f;
      pf.datatype = 7;  // sensor_msgs/PointField FLOAT32
      pf.count = 1;
      cloud_msg.fields.push_back(pf);
    }
    cloud_msg.height = 1;
    cloud_msg.width = n_points;
    cloud_msg.point_step = 16;
    cloud_msg.row_step = 16 * n_points;
    cloud_msg.is_bigendian = false;
    cloud_msg.is_dense = true;
    cloud_msg.data.resize(static_cast<size_t>(n_points) * 16);
    if (n_points) std::memcpy(cloud_msg.data.data(), xyzi_.data(), static_cast<size_t>(n_points) * 16);
    return true;
  }

  // ext E11 (include/rplgpu_msg.h): the scans of ONE time step (one per sensor, at most the `max_scans` of
  // configure) ray-cast into a nav_msgs/OccupancyGrid-shaped message — what a costmap obstacle layer's
  // raytraceFreespace + mark loop does per observation.  pose2d: 6 floats per scan (r00 r01 tx r10 r11 ty,
  // sensor in the grid's frame), motion: 4 per scan (vx vy wz time_increment), t0: 1 per scan; each may be
  // null.  `grid_msg.data` of the right size is the previous grid (cells no ray touches keep their value);
  // any other size starts from unknown (-1).  Fills info.resolution / width / height / origin and data;
  // header and info.map_load_time are the caller's.
  template <class NodeT, class OccupancyGridT>
  bool fill_occupancy_grid(const std::vector<std::vector<NodeT>> &scans, const ScanConfig &cfg,
                           const rplgpu_occ_grid_t &grid, const float *pose2d, const float *motion,
                           const float *t0, OccupancyGridT &grid_msg, uint32_t cells[3] = nullptr,
                           uint32_t *status = nullptr) {
    if (scans.empty()) return false;
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    size_t stride = 1;
    for (const auto &s : scans) stride = s.size() > stride ? s.size() : stride;
    if (stride > max_n_) return fail("scan larger than the configured capacity");
    occ_nodes_.assign(scans.size() * stride, rplgpu_node_t{});
    occ_len_.resize(scans.size());
    for (size_t b = 0; b < scans.size(); ++b) {
      if (!scans[b].empty()) std::memcpy(&occ_nodes_[b * stride], scans[b].data(), scans[b].size() * 8);
      occ_len_[b] = static_cast<uint32_t>(scans[b].size());
    }
    const size_t n_cells = static_cast<size_t>(grid.width) * grid.height;
    const bool has_prev = n_cells != 0 && grid_msg.data.size() == n_cells;
    if (has_prev) occ_prev_.assign(grid_msg.data.begin(), grid_msg.data.end());
    occ_out_.resize(n_cells ? n_cells : 1);
    const rplgpu_params_t p = cfg.to_params();
    if (rplgpu_occupancy_grid(h_, occ_nodes_.data(), static_cast<uint32_t>(stride), occ_len_.data(),
                              static_cast<uint32_t>(scans.size()), &p, motion, pose2d, t0, &grid,
                              has_prev ? occ_prev_.data() : nullptr, occ_out_.data(), cells, status) != RPLGPU_OK)
      return note_error();
    grid_msg.info.resolution = grid.resolution;
    grid_msg.info.width = grid.width;
    grid_msg.info.height = grid.height;
    grid_msg.info.origin.position.x = grid.origin_x;
    grid_msg.info.origin.position.y = grid.origin_y;
    grid_msg.info.origin.position.z = 0.0;
    grid_msg.info.origin.orientation.x = 0.0;
    grid_msg.info.origin.orientation.y = 0.0;
    grid_msg.info.origin.orientation.z = 0.0;
    grid_msg.info.origin.orientation.w = 1.0;
    grid_msg.data.assign(occ_out_.begin(), occ_out_.begin() + n_cells);
    return true;
  }

  // ext E12 (include/rplgpu_msg.h): `grid_msg` (what fill_occupancy_grid left) inflated into `costmap_msg` —
  // what a costmap inflation layer does per update: 100 lethal, 99 within the inscribed radius, 1 .. 98
  // decaying out to the inflation radius, in the scale Nav2 publishes a costmap as an OccupancyGrid.  Copies
  // info and fills data (the header is the caller's); cells (optional): result cells that are 100, 99, 1 .. 98 and -1.
  // costmap_msg may not be grid_msg.
  template <class OccupancyGridT>
  bool inflate_grid(const OccupancyGridT &grid_msg, const rplgpu_inflation_t &inflation,
                    OccupancyGridT &costmap_msg, uint32_t cells[4] = nullptr) {
    if (!h_) return fail("rplgpu handle not configured");
    if (&grid_msg == &costmap_msg) return fail("inflate_grid: the costmap may not be the grid");
    last_error_.clear();
    const size_t n_cells = static_cast<size_t>(grid_msg.info.width) * grid_msg.info.height;
    if (n_cells == 0 || grid_msg.data.size() != n_cells) return fail("inflate_grid: data is not width x height");
    occ_prev_.assign(grid_msg.data.begin(), grid_msg.data.end());
    occ_out_.resize(n_cells);
    if (rplgpu_inflate_grid(h_, occ_prev_.data(), grid_msg.info.width, grid_msg.info.height,
                            grid_msg.info.resolution, &inflation, occ_out_.data(), cells) != RPLGPU_OK)
      return note_error();
    costmap_msg.info = grid_msg.info;
    costmap_msg.data.assign(occ_out_.begin(), occ_out_.end());
    return true;
  }

  // ext E13 (include/rplgpu_msg.h): the scans of ONE time step matched to `field_msg`, a likelihood field in a
  // nav_msgs/OccupancyGrid-shaped message (e.g. what inflate_grid left for a map) — what a correlative scan
  // matcher does per update.  pose2d is the PRIOR of every sensor in the field's frame, pivot (2 floats or null)
  // the base's prior position; shift_x / shift_y / rot_steps / rot_step of `window` are used, its grid comes
  // from field_msg.info (origin orientation must be the identity).  result: the eight words of the header's BEST
  // table — score, k, j, i, finite points, score of (0, 0, 0), candidates that tie, 0.
  struct MatchResult {
    uint32_t score = 0;
    int32_t k = 0, j = 0, i = 0;
    uint32_t points = 0, score_at_prior = 0, ties = 0;
  };
  template <class NodeT, class OccupancyGridT>
  bool match_scans(const std::vector<std::vector<NodeT>> &scans, const ScanConfig &cfg, const float *pose2d,
                   const float *motion, const float *t0, const float *pivot, const OccupancyGridT &field_msg,
                   const rplgpu_scan_match_t &window, MatchResult &result, uint32_t *status = nullptr) {
    if (scans.empty()) return false;
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    rplgpu_scan_match_t m = window;
    m.origin_x = static_cast<float>(field_msg.info.origin.position.x);
    m.origin_y = static_cast<float>(field_msg.info.origin.position.y);
    m.resolution = field_msg.info.resolution;
    m.width = field_msg.info.width;
    m.height = field_msg.info.height;
    const size_t n_cells = static_cast<size_t>(m.width) * m.height;
    if (n_cells == 0 || field_msg.data.size() != n_cells) return fail("match_scans: data is not width x height");
    size_t stride = 1;
    for (const auto &s : scans) stride = s.size() > stride ? s.size() : stride;
    if (stride > max_n_) return fail("scan larger than the configured capacity");
    occ_nodes_.assign(scans.size() * stride, rplgpu_node_t{});
    occ_len_.resize(scans.size());
    for (size_t b = 0; b < scans.size(); ++b) {
      if (!scans[b].empty()) std::memcpy(&occ_nodes_[b * stride], scans[b].data(), scans[b].size() * 8);
      occ_len_[b] = static_cast<uint32_t>(scans[b].size());
    }
    occ_prev_.assign(field_msg.data.begin(), field_msg.data.end());
    const rplgpu_params_t p = cfg.to_params();
    uint32_t best[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_match_scans(h_, occ_nodes_.data(), static_cast<uint32_t>(stride), occ_len_.data(),
                           static_cast<uint32_t>(scans.size()), &p, motion, pose2d, t0, pivot, &m, occ_prev_.data(),
                           nullptr, best, status) != RPLGPU_OK)
      return note_error();
    result.score = best[0];
    result.k = static_cast<int32_t>(best[1]);
    result.j = static_cast<int32_t>(best[2]);
    result.i = static_cast<int32_t>(best[3]);
    result.points = best[4];
    result.score_at_prior = best[5];
    result.ties = best[6];
    return true;
  }

  // ext E24 (include/rplgpu_msg.h): match_scans over a window of up to 256 cells a side, by bound and refine — what
  // a loop closer or a relocaliser asks of a stored map.  Arguments as match_scans; shift_x / shift_y / rot_steps /
  // rot_step / max_blocks of `window` are used.  result.proven false: the list was longer than max_blocks, the
  // answer is the best of the two seed blocks only, and result.listed says which max_blocks proves it.  The result
  // goes into rplgpu_apply_match_dev with an E13 spec of the same grid, rot_steps and rot_step.
  struct WideMatchResult : MatchResult {
    bool proven = false;
    uint32_t blocks = 0, greatest_bound = 0, floor = 0, listed = 0;  // work words 0, 1, 3, 4
  };
  template <class NodeT, class OccupancyGridT>
  bool match_wide(const std::vector<std::vector<NodeT>> &scans, const ScanConfig &cfg, const float *pose2d,
                  const float *motion, const float *t0, const float *pivot, const OccupancyGridT &field_msg,
                  const rplgpu_wide_match_t &window, WideMatchResult &result, uint32_t *status = nullptr) {
    if (scans.empty()) return false;
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    rplgpu_wide_match_t m = window;
    m.origin_x = static_cast<float>(field_msg.info.origin.position.x);
    m.origin_y = static_cast<float>(field_msg.info.origin.position.y);
    m.resolution = field_msg.info.resolution;
    m.width = field_msg.info.width;
    m.height = field_msg.info.height;
    const size_t n_cells = static_cast<size_t>(m.width) * m.height;
    if (n_cells == 0 || field_msg.data.size() != n_cells) return fail("match_wide: data is not width x height");
    size_t stride = 1;
    for (const auto &s : scans) stride = s.size() > stride ? s.size() : stride;
    if (stride > max_n_) return fail("scan larger than the configured capacity");
    occ_nodes_.assign(scans.size() * stride, rplgpu_node_t{});
    occ_len_.resize(scans.size());
    for (size_t b = 0; b < scans.size(); ++b) {
      if (!scans[b].empty()) std::memcpy(&occ_nodes_[b * stride], scans[b].data(), scans[b].size() * 8);
      occ_len_[b] = static_cast<uint32_t>(scans[b].size());
    }
    occ_prev_.assign(field_msg.data.begin(), field_msg.data.end());
    const rplgpu_params_t p = cfg.to_params();
    uint32_t best[8] = {0, 0, 0, 0, 0, 0, 0, 0}, work[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_match_wide(h_, occ_nodes_.data(), static_cast<uint32_t>(stride), occ_len_.data(),
                          static_cast<uint32_t>(scans.size()), &p, motion, pose2d, t0, pivot, &m, occ_prev_.data(),
                          nullptr, best, work, status) != RPLGPU_OK)
      return note_error();
    result.score = best[0];
    result.k = static_cast<int32_t>(best[1]);
    result.j = static_cast<int32_t>(best[2]);
    result.i = static_cast<int32_t>(best[3]);
    result.points = best[4];
    result.score_at_prior = best[5];
    result.ties = best[6];
    result.proven = (best[7] & RPLGPU_WIDE_MATCH_UNPROVEN) == 0;
    result.blocks = work[0];
    result.greatest_bound = work[1];
    result.floor = work[3];
    result.listed = work[4];
    return true;
  }

  // ext E25 (include/rplgpu_msg.h): a list of poses of the BASE, four floats (cos, sin, x, y) each in the field's
  // frame, refined below a cell by `iters` Gauss-Newton steps against the bilinearly interpolated `field_msg` — what
  // Hector's matcher does, and Cartographer's last stage behind its correlative matcher.  pose2d: every sensor's MOUNT
  // pose in the base frame (null: identity); target / damping / max_step_cells / max_rot / min_points of `rule` are
  // used, its grid comes from field_msg.info (origin orientation must be the identity).  poses is stepped in place;
  // sums (optional): the last round's 32 words per pose, what rplgpu_refine_covariance takes.
  struct RefineResult {
    uint32_t stepped = 0, too_few = 0, singular = 0, clamped = 0, best_index = 0, points = 0;
    uint64_t best_sum = 0;  // the greatest S V of the last round's sums
  };
  template <class NodeT, class OccupancyGridT>
  bool refine_poses(const std::vector<std::vector<NodeT>> &scans, const ScanConfig &cfg, const float *pose2d,
                    const float *motion, const float *t0, const OccupancyGridT &field_msg,
                    const rplgpu_pose_refine_t &rule, uint32_t iters, std::vector<float> &poses, RefineResult &result,
                    std::vector<uint32_t> *sums = nullptr, uint32_t *status = nullptr) {
    if (scans.empty()) return false;
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    if (poses.empty() || poses.size() % 4 != 0) return fail("refine_poses: poses must hold four floats a pose");
    rplgpu_pose_refine_t r = rule;
    r.origin_x = static_cast<float>(field_msg.info.origin.position.x);
    r.origin_y = static_cast<float>(field_msg.info.origin.position.y);
    r.resolution = field_msg.info.resolution;
    r.width = field_msg.info.width;
    r.height = field_msg.info.height;
    const size_t n_cells = static_cast<size_t>(r.width) * r.height;
    if (n_cells == 0 || field_msg.data.size() != n_cells) return fail("refine_poses: data is not width x height");
    size_t stride = 1;
    for (const auto &s : scans) stride = s.size() > stride ? s.size() : stride;
    if (stride > max_n_) return fail("scan larger than the configured capacity");
    occ_nodes_.assign(scans.size() * stride, rplgpu_node_t{});
    occ_len_.resize(scans.size());
    for (size_t b = 0; b < scans.size(); ++b) {
      if (!scans[b].empty()) std::memcpy(&occ_nodes_[b * stride], scans[b].data(), scans[b].size() * 8);
      occ_len_[b] = static_cast<uint32_t>(scans[b].size());
    }
    occ_prev_.assign(field_msg.data.begin(), field_msg.data.end());
    const rplgpu_params_t p = cfg.to_params();
    const uint32_t P = static_cast<uint32_t>(poses.size() / 4);
    std::vector<float> out(poses.size());
    if (sums) sums->assign(static_cast<size_t>(RPLGPU_REFINE_WORDS) * P, 0u);
    uint32_t res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_refine_poses(h_, occ_nodes_.data(), static_cast<uint32_t>(stride), occ_len_.data(),
                            static_cast<uint32_t>(scans.size()), &p, motion, pose2d, t0, &r, poses.data(), P,
                            occ_prev_.data(), iters, out.data(), sums ? sums->data() : nullptr, nullptr, res,
                            status) != RPLGPU_OK)
      return note_error();
    poses.swap(out);
    result.stepped = res[0];
    result.too_few = res[1];
    result.singular = res[2];
    result.clamped = res[3];
    result.best_index = res[4];
    result.best_sum = (static_cast<uint64_t>(res[6]) << 32) | res[5];
    result.points = res[7];
    return true;
  }

  // ext E26 (include/rplgpu_msg.h): the cost-to-goal field over `costmap_msg` (E12's output, or any OccupancyGrid) —
  // NavFn's potential — and, with `starts`, the paths down it.  goals and starts are cell indices (y * width + x);
  // lethal / neutral / factor / unknown_cost / cap / rounds of `rule` are used, its size comes from costmap_msg.info.
  // potential: width x height words, RPLGPU_NAV_UNREACHED where no goal is in reach.  paths (with starts): one list of
  // cells per start, the start first; info: the four words per path.  The door resumes until the field is finished.
  struct NavResult {
    uint32_t dirty_tiles = 0, goals_taken = 0, goals_ignored = 0, reached = 0, greatest = 0, tile_visits = 0, rounds = 0;
    bool finished = false;
  };
  template <class OccupancyGridT>
  bool nav_field(const OccupancyGridT &costmap_msg, const rplgpu_nav_field_t &rule, const std::vector<uint32_t> &goals,
                 std::vector<uint32_t> &potential, NavResult &result, const std::vector<uint32_t> *starts = nullptr,
                 uint32_t max_len = 0, std::vector<std::vector<uint32_t>> *paths = nullptr,
                 std::vector<uint32_t> *info = nullptr) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    rplgpu_nav_field_t f = rule;
    f.width = costmap_msg.info.width;
    f.height = costmap_msg.info.height;
    const size_t n_cells = static_cast<size_t>(f.width) * f.height;
    if (n_cells == 0 || costmap_msg.data.size() != n_cells) return fail("nav_field: data is not width x height");
    const bool with_paths = starts && !starts->empty();
    if (with_paths && (!paths || !info || max_len == 0)) return fail("nav_field: starts need paths, info and max_len");
    occ_prev_.assign(costmap_msg.data.begin(), costmap_msg.data.end());
    potential.assign(n_cells, RPLGPU_NAV_UNREACHED);
    const uint32_t S = with_paths ? static_cast<uint32_t>(starts->size()) : 0u;
    std::vector<uint32_t> flat(static_cast<size_t>(S) * max_len, RPLGPU_NAV_UNREACHED);
    if (with_paths) info->assign(4u * static_cast<size_t>(S), 0u);
    uint32_t res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_nav_field(h_, &f, occ_prev_.data(), goals.empty() ? nullptr : goals.data(),
                         static_cast<uint32_t>(goals.size()), potential.data(), res,
                         with_paths ? starts->data() : nullptr, S, with_paths ? flat.data() : nullptr, max_len,
                         with_paths ? info->data() : nullptr) != RPLGPU_OK)
      return note_error();
    if (with_paths) {
      paths->assign(S, std::vector<uint32_t>());
      for (uint32_t s = 0; s < S; ++s)
        (*paths)[s].assign(flat.begin() + static_cast<size_t>(s) * max_len,
                           flat.begin() + static_cast<size_t>(s) * max_len + (*info)[4u * s]);
    }
    result.dirty_tiles = res[0];
    result.finished = res[0] == 0;
    result.goals_taken = res[2];
    result.goals_ignored = res[3];
    result.reached = res[4];
    result.greatest = res[5];
    result.tile_visits = res[6];
    result.rounds = res[7];
    return true;
  }

  // ext E29 (include/rplgpu_msg.h): the frontier cells of a grid (free, reachable, next to unknown space) grouped into
  // 8-connected components and the next goal picked — explore_lite's search.  lethal / min_size / dist_weight /
  // size_weight of `rule` are used, its size comes from grid_msg.info.  potential: E26's field with the robot's own
  // cell as the goal (nav_field's output), or null: every free cell then counts as reached.  rows: up to row_cap
  // kept components in ascending label order; labels (optional): one word per cell.
  struct FrontierRow {
    uint32_t label = 0, cells = 0, nearest = 0, nearest_cell = 0;
    uint64_t sum_x = 0, sum_y = 0;
  };
  struct FrontierResult {
    uint32_t flags = 0, frontier_cells = 0, components = 0, kept = 0, dropped_cells = 0, greatest = 0;
    bool has_goal = false;
    uint32_t goal_cell = 0;
    FrontierRow best;
  };
  template <class OccupancyGridT>
  bool frontiers(const OccupancyGridT &grid_msg, const rplgpu_frontiers_t &rule, const std::vector<uint32_t> *potential,
                 uint32_t comp_cap, uint32_t row_cap, FrontierResult &result, std::vector<FrontierRow> *rows = nullptr,
                 std::vector<uint32_t> *labels = nullptr) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    rplgpu_frontiers_t f = rule;
    f.width = grid_msg.info.width;
    f.height = grid_msg.info.height;
    const size_t n_cells = static_cast<size_t>(f.width) * f.height;
    if (n_cells == 0 || grid_msg.data.size() != n_cells) return fail("frontiers: data is not width x height");
    if (potential && potential->size() != n_cells) return fail("frontiers: the potential is not width x height");
    if (row_cap != 0 && !rows) return fail("frontiers: row_cap needs rows");
    occ_prev_.assign(grid_msg.data.begin(), grid_msg.data.end());
    if (labels) labels->assign(n_cells, RPLGPU_FRONTIER_NO_LABEL);
    std::vector<uint32_t> flat(8u * static_cast<size_t>(row_cap), 0u);
    uint32_t res[RPLGPU_FRONTIER_WORDS] = {0}, goal = 0, n_goal = 0;
    if (rplgpu_frontiers(h_, &f, occ_prev_.data(), potential ? potential->data() : nullptr, comp_cap,
                         labels ? labels->data() : nullptr, row_cap ? flat.data() : nullptr, row_cap, &goal, &n_goal,
                         res) != RPLGPU_OK)
      return note_error();
    const auto row_of = [](const uint32_t *w) {
      FrontierRow r;
      r.label = w[0];
      r.cells = w[1];
      r.sum_x = (static_cast<uint64_t>(w[3]) << 32) | w[2];
      r.sum_y = (static_cast<uint64_t>(w[5]) << 32) | w[4];
      r.nearest = w[6];
      r.nearest_cell = w[7];
      return r;
    };
    if (rows) {
      rows->clear();
      for (uint32_t i = 0; i < res[14]; ++i) rows->push_back(row_of(&flat[8u * i]));
    }
    result.flags = res[0];
    result.frontier_cells = res[1];
    result.components = res[2];
    result.kept = res[3];
    result.dropped_cells = res[4];
    result.greatest = res[13];
    result.has_goal = n_goal != 0;
    result.goal_cell = goal;
    const uint32_t best[8] = {res[5], res[6], res[9], res[10], res[11], res[12], res[7], res[8]};
    result.best = row_of(best);
    return true;
  }

  // ext E27 (include/rplgpu_msg.h): candidate motions rolled out of the pose `start_xyt` (x, y, theta in the costmap's
  // frame; it goes through rplgpu_pose_list) and scored — DWB's / MPPI's inner loop.  deltas: four floats per
  // candidate (rplgpu_rollout_deltas makes them from body velocities), or per candidate and step with per_step;
  // footprint: (x, y) pairs in the base frame; potential: E26's field over the same grid (nav_field's output), or null.
  // lethal / unknown_value / steps / min_steps and the four scales of `rule` are used, its grid comes from
  // costmap_msg.info (origin orientation must be the identity).  out: the eight words per candidate; end_poses
  // (optional): four floats per candidate.
  struct RolloutResult {
    uint32_t admissible = 0, best_index = RPLGPU_ROLLOUT_NONE, ties = 0, blocked = 0, cell_range = 0;
    uint64_t best_score = ~0ull;
    bool none = true;
  };
  template <class OccupancyGridT>
  bool rollout(const OccupancyGridT &costmap_msg, const rplgpu_rollout_t &rule, const double start_xyt[3],
               const std::vector<float> &deltas, bool per_step, const std::vector<float> &footprint,
               const std::vector<uint32_t> *potential, std::vector<uint32_t> &out, RolloutResult &result,
               std::vector<float> *end_poses = nullptr) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    rplgpu_rollout_t r = rule;
    r.origin_x = static_cast<float>(costmap_msg.info.origin.position.x);
    r.origin_y = static_cast<float>(costmap_msg.info.origin.position.y);
    r.resolution = costmap_msg.info.resolution;
    r.width = costmap_msg.info.width;
    r.height = costmap_msg.info.height;
    const size_t n_cells = static_cast<size_t>(r.width) * r.height;
    if (n_cells == 0 || costmap_msg.data.size() != n_cells) return fail("rollout: data is not width x height");
    if (potential && potential->size() != n_cells) return fail("rollout: the potential is not width x height");
    const size_t per = 4u * (per_step ? static_cast<size_t>(r.steps) : 1u);
    if (per == 0 || deltas.empty() || deltas.size() % per != 0) return fail("rollout: deltas must be 4 floats per candidate (and step)");
    if (footprint.empty() || footprint.size() % 2 != 0) return fail("rollout: footprint must be (x, y) pairs");
    const uint32_t K = static_cast<uint32_t>(deltas.size() / per);
    float start[4];
    if (rplgpu_pose_list(start_xyt, 1, start) != RPLGPU_OK) return fail("rollout: start pose");
    occ_prev_.assign(costmap_msg.data.begin(), costmap_msg.data.end());
    out.assign(8u * static_cast<size_t>(K), 0u);
    if (end_poses) end_poses->assign(4u * static_cast<size_t>(K), 0.0f);
    uint32_t res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_rollout(h_, &r, start, deltas.data(), per_step ? 1u : 0u, footprint.data(),
                       static_cast<uint32_t>(footprint.size() / 2), occ_prev_.data(),
                       potential ? potential->data() : nullptr, K, out.data(), end_poses ? end_poses->data() : nullptr,
                       res) != RPLGPU_OK)
      return note_error();
    result.admissible = res[0];
    result.best_index = res[1];
    result.best_score = (static_cast<uint64_t>(res[3]) << 32) | res[2];
    result.ties = res[4];
    result.blocked = res[5];
    result.cell_range = res[6];
    result.none = (res[7] & 1u) != 0;
    return true;
  }

  // ext E28 (include/rplgpu_msg.h): MPPI's update behind rollout().  rollout_out: the eight words per candidate and
  // rollout_words: the eight result words rplgpu_rollout left (RolloutResult is made from them); deltas: what was
  // rolled (four floats per candidate, or per candidate and step with rule.delta_per_step); table: rule.table_len
  // entries (rplgpu_mppi_table); nominal: the sequence kept where no candidate has weight at a step, or null.
  // weights: one word per candidate; nominal_out: four floats per step (it may be *nominal).
  struct MppiResult {
    uint32_t weighted = 0, clamped = 0, off_range = 0;
    uint64_t sum_w = 0, sum_w2 = 0;
    bool no_weight = true, empty_step = false;
  };
  bool mppi_update(const rplgpu_mppi_t &rule, const std::vector<uint32_t> &rollout_out, const uint32_t rollout_words[8],
                   const std::vector<float> &deltas, const std::vector<uint16_t> &table,
                   const std::vector<float> *nominal, std::vector<uint32_t> &weights, std::vector<float> &nominal_out,
                   MppiResult &result, std::vector<uint32_t> *sums = nullptr) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    const size_t T_e = rule.delta_per_step ? rule.steps : 1u;
    if (rollout_out.empty() || rollout_out.size() % 8 != 0) return fail("mppi_update: rollout_out must be 8 words per candidate");
    const uint32_t K = static_cast<uint32_t>(rollout_out.size() / 8);
    if (T_e == 0 || deltas.size() != 4u * K * T_e) return fail("mppi_update: deltas must be 4 floats per candidate (and step)");
    if (table.size() != rule.table_len) return fail("mppi_update: the table is not table_len entries");
    if (nominal && nominal->size() != 4u * T_e) return fail("mppi_update: nominal must be 4 floats per step");
    std::vector<float> nout(4u * T_e, 0.0f);
    std::vector<uint32_t> s(8u * T_e, 0u);
    weights.assign(K, 0u);
    uint32_t res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_mppi_update(h_, &rule, rollout_out.data(), rollout_words, deltas.data(), table.data(),
                           nominal ? nominal->data() : nullptr, K, weights.data(), s.data(), nout.data(), res) != RPLGPU_OK)
      return note_error();
    nominal_out = nout;
    if (sums) *sums = s;
    result.weighted = res[0];
    result.clamped = res[1];
    result.sum_w = (static_cast<uint64_t>(res[3]) << 32) | res[2];
    result.sum_w2 = (static_cast<uint64_t>(res[5]) << 32) | res[4];
    result.off_range = res[6];
    result.no_weight = (res[7] & RPLGPU_MPPI_NO_WEIGHT) != 0;
    result.empty_step = (res[7] & RPLGPU_MPPI_EMPTY_STEP) != 0;
    return true;
  }

  // ext E28: the next candidates, K sequences of noise.size() / (4 K) steps around the nominal sequence moved `shift`
  // steps on (the receding horizon); candidates is rollout()'s per-step `deltas`.
  bool mppi_spread(const std::vector<float> &nominal, const std::vector<float> &noise, uint32_t K, uint32_t shift,
                   bool keep_first, std::vector<float> &candidates) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    if (nominal.empty() || nominal.size() % 4 != 0) return fail("mppi_spread: nominal must be 4 floats per step");
    if (K == 0 || noise.empty() || noise.size() % (4u * static_cast<size_t>(K)) != 0)
      return fail("mppi_spread: noise must be 4 floats per candidate and step");
    std::vector<float> out(noise.size(), 0.0f);
    if (rplgpu_mppi_spread(h_, nominal.data(), static_cast<uint32_t>(nominal.size() / 4), noise.data(), K,
                           static_cast<uint32_t>(noise.size() / (4u * static_cast<size_t>(K))), shift, keep_first ? 1u : 0u,
                           out.data()) != RPLGPU_OK)
      return note_error();
    candidates.swap(out);
    return true;
  }

  // ext E15 (include/rplgpu_msg.h): a list of poses of the BASE weighed against `field_msg` by the scans of ONE time
  // step — what a particle filter's sensor update does.  xyt: (x, y, theta) per pose, in the field's frame (they go
  // through rplgpu_pose_list); pose2d: every sensor's MOUNT pose in the base frame (null: identity); the grid comes
  // from field_msg.info (origin orientation must be the identity).  weights: one per pose; result: the eight
  // words of the header's RESULT table.
  struct PoseResult {
    uint32_t best = 0, best_index = 0, ties = 0, zeros = 0, points = 0, weight_of_first = 0;
    uint64_t sum = 0;
  };
  template <class NodeT, class OccupancyGridT>
  bool score_poses(const std::vector<std::vector<NodeT>> &scans, const ScanConfig &cfg, const float *pose2d,
                   const float *motion, const float *t0, const OccupancyGridT &field_msg,
                   const std::vector<double> &xyt, std::vector<uint32_t> &weights, PoseResult &result,
                   uint32_t *status = nullptr) {
    if (scans.empty()) return false;
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    rplgpu_pose_score_t spec;
    spec.origin_x = static_cast<float>(field_msg.info.origin.position.x);
    spec.origin_y = static_cast<float>(field_msg.info.origin.position.y);
    spec.resolution = field_msg.info.resolution;
    spec.width = field_msg.info.width;
    spec.height = field_msg.info.height;
    const size_t n_cells = static_cast<size_t>(spec.width) * spec.height;
    if (n_cells == 0 || field_msg.data.size() != n_cells) return fail("score_poses: data is not width x height");
    const size_t n_poses = xyt.size() / 3;
    if (n_poses == 0 || xyt.size() != 3 * n_poses || n_poses > RPLGPU_MAX_POSES)
      return fail("score_poses: xyt must hold 1 .. RPLGPU_MAX_POSES poses of 3 values");
    size_t stride = 1;
    for (const auto &s : scans) stride = s.size() > stride ? s.size() : stride;
    if (stride > max_n_) return fail("scan larger than the configured capacity");
    occ_nodes_.assign(scans.size() * stride, rplgpu_node_t{});
    occ_len_.resize(scans.size());
    for (size_t b = 0; b < scans.size(); ++b) {
      if (!scans[b].empty()) std::memcpy(&occ_nodes_[b * stride], scans[b].data(), scans[b].size() * 8);
      occ_len_[b] = static_cast<uint32_t>(scans[b].size());
    }
    occ_prev_.assign(field_msg.data.begin(), field_msg.data.end());
    pose_list_.resize(4 * n_poses);
    if (rplgpu_pose_list(xyt.data(), static_cast<uint32_t>(n_poses), pose_list_.data()) != RPLGPU_OK)
      return fail("score_poses: rplgpu_pose_list refused the list");
    weights.assign(n_poses, 0u);
    const rplgpu_params_t p = cfg.to_params();
    uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_score_poses(h_, occ_nodes_.data(), static_cast<uint32_t>(stride), occ_len_.data(),
                           static_cast<uint32_t>(scans.size()), &p, motion, pose2d, t0, &spec, pose_list_.data(),
                           static_cast<uint32_t>(n_poses), occ_prev_.data(), weights.data(), words,
                           status) != RPLGPU_OK)
      return note_error();
    result.best = words[0];
    result.best_index = words[1];
    result.ties = words[2];
    result.zeros = words[3];
    result.points = words[4];
    result.weight_of_first = words[5];
    result.sum = static_cast<uint64_t>(words[6]) | (static_cast<uint64_t>(words[7]) << 32);
    return true;
  }

  // ext E23 (include/rplgpu_msg.h): score_poses without the samples the pose list disagrees with (AMCL's beam skip).
  // rule: agree_lo and the keep and err ratios (its grid fields are taken from field_msg.info).  counts and mask come
  // back per scan at `stride` (the longest scan) and ceil(stride / 32) words: mask bit i of scan b is 0 for a finite
  // sample the map does not explain.  agree: the header's d_agree table.
  struct AgreeResult {
    uint32_t finite = 0, kept = 0, fell_back = 0, entered = 0, count_max = 0, count_min = 0;
    uint64_t count_sum = 0;
    uint32_t stride = 0;  // samples per scan in counts; (stride + 31) / 32 words per scan in mask
  };
  template <class NodeT, class OccupancyGridT>
  bool score_poses_agree(const std::vector<std::vector<NodeT>> &scans, const ScanConfig &cfg, const float *pose2d,
                         const float *motion, const float *t0, const OccupancyGridT &field_msg,
                         const rplgpu_beam_agree_t &rule, const std::vector<double> &xyt,
                         std::vector<uint32_t> &weights, PoseResult &result, std::vector<uint32_t> &counts,
                         std::vector<uint32_t> &mask, AgreeResult &agree, uint32_t *status = nullptr) {
    if (scans.empty()) return false;
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    rplgpu_beam_agree_t spec = rule;
    spec.origin_x = static_cast<float>(field_msg.info.origin.position.x);
    spec.origin_y = static_cast<float>(field_msg.info.origin.position.y);
    spec.resolution = field_msg.info.resolution;
    spec.width = field_msg.info.width;
    spec.height = field_msg.info.height;
    const size_t n_cells = static_cast<size_t>(spec.width) * spec.height;
    if (n_cells == 0 || field_msg.data.size() != n_cells)
      return fail("score_poses_agree: data is not width x height");
    const size_t n_poses = xyt.size() / 3;
    if (n_poses == 0 || xyt.size() != 3 * n_poses || n_poses > RPLGPU_MAX_POSES)
      return fail("score_poses_agree: xyt must hold 1 .. RPLGPU_MAX_POSES poses of 3 values");
    size_t stride = 1;
    for (const auto &s : scans) stride = s.size() > stride ? s.size() : stride;
    if (stride > max_n_) return fail("scan larger than the configured capacity");
    occ_nodes_.assign(scans.size() * stride, rplgpu_node_t{});
    occ_len_.resize(scans.size());
    for (size_t b = 0; b < scans.size(); ++b) {
      if (!scans[b].empty()) std::memcpy(&occ_nodes_[b * stride], scans[b].data(), scans[b].size() * 8);
      occ_len_[b] = static_cast<uint32_t>(scans[b].size());
    }
    occ_prev_.assign(field_msg.data.begin(), field_msg.data.end());
    pose_list_.resize(4 * n_poses);
    if (rplgpu_pose_list(xyt.data(), static_cast<uint32_t>(n_poses), pose_list_.data()) != RPLGPU_OK)
      return fail("score_poses_agree: rplgpu_pose_list refused the list");
    weights.assign(n_poses, 0u);
    counts.assign(scans.size() * stride, 0u);
    mask.assign(scans.size() * ((stride + 31) / 32), 0u);
    const rplgpu_params_t p = cfg.to_params();
    uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0}, aw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_score_poses_agree(h_, occ_nodes_.data(), static_cast<uint32_t>(stride), occ_len_.data(),
                                 static_cast<uint32_t>(scans.size()), &p, motion, pose2d, t0, &spec,
                                 pose_list_.data(), static_cast<uint32_t>(n_poses), occ_prev_.data(), weights.data(),
                                 words, status, counts.data(), mask.data(), aw) != RPLGPU_OK)
      return note_error();
    result.best = words[0];
    result.best_index = words[1];
    result.ties = words[2];
    result.zeros = words[3];
    result.points = words[4];
    result.weight_of_first = words[5];
    result.sum = static_cast<uint64_t>(words[6]) | (static_cast<uint64_t>(words[7]) << 32);
    agree.finite = aw[0];
    agree.kept = aw[1];
    agree.fell_back = aw[2];
    agree.entered = aw[3];
    agree.count_max = aw[4];
    agree.count_min = aw[5];
    agree.count_sum = static_cast<uint64_t>(aw[6]) | (static_cast<uint64_t>(aw[7]) << 32);
    agree.stride = static_cast<uint32_t>(stride);
    return true;
  }

  // ext E16 (include/rplgpu_msg.h): the list `poses` (four floats per pose, as rplgpu_pose_list writes them)
  // redrawn by `weights` (what score_poses returned) into `count` poses — systematic resampling from the caller's
  // one random word u — and moved by `delta` (dc, ds, dx, dy): empty for a plain copy, 4 floats for one odometry
  // increment, 4 x count for one per output.  ancestors: the index each new pose descends from; result: the
  // header's RESULT table.  The new list goes into score_poses's device call as it is, or back through xyt.
  struct ResampleResult {
    uint64_t sum = 0;           // S
    double sum_squares = 0.0;   // the 96-bit sum of the squared weights, rounded
    double n_eff = 0.0;         // S^2 / sum of squares (0 when every weight is 0)
    uint32_t alive = 0, distinct = 0;
    bool all_dead = false;
  };
  bool resample_poses(const std::vector<uint32_t> &weights, const std::vector<float> &poses, uint32_t count,
                      uint32_t u, const std::vector<float> &delta, std::vector<float> &poses_out,
                      std::vector<uint32_t> &ancestors, ResampleResult &result) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    const size_t n_poses = weights.size();
    if (n_poses == 0 || n_poses > RPLGPU_MAX_POSES || poses.size() != 4 * n_poses)
      return fail("resample_poses: 1 .. RPLGPU_MAX_POSES weights and four floats per pose");
    if (count == 0 || count > RPLGPU_MAX_POSES) return fail("resample_poses: count must be in 1 .. RPLGPU_MAX_POSES");
    if (!delta.empty() && delta.size() != 4 && delta.size() != 4 * static_cast<size_t>(count))
      return fail("resample_poses: delta must hold 0, 1 or count increments of four floats");
    poses_out.assign(4 * static_cast<size_t>(count), 0.0f);
    ancestors.assign(count, 0u);
    uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_resample_poses(h_, weights.data(), static_cast<uint32_t>(n_poses), count, u, poses.data(),
                              delta.empty() ? nullptr : delta.data(), static_cast<uint32_t>(delta.size() / 4),
                              poses_out.data(), ancestors.data(), words) != RPLGPU_OK)
      return note_error();
    result.sum = static_cast<uint64_t>(words[0]) | (static_cast<uint64_t>(words[1]) << 32);
    result.sum_squares = static_cast<double>(words[2]) + 4294967296.0 * static_cast<double>(words[3]) +
                         18446744073709551616.0 * static_cast<double>(words[4]);
    const double s = static_cast<double>(result.sum);
    result.n_eff = result.sum_squares > 0.0 ? s * s / result.sum_squares : 0.0;
    result.alive = words[5];
    result.distinct = words[6];
    result.all_dead = (words[7] & 1u) != 0;
    return true;
  }

  // ext E17 (include/rplgpu_msg.h): the list `poses` weighed by `weights` (what score_poses returned; empty: every
  // weight 1, the list as resample_poses leaves it) reduced to a pose with a covariance — what AMCL publishes as
  // PoseWithCovarianceStamped.  The gate of `spec` is laid around pose `center` (score_poses's best_index).  `all`
  // is formed over every pose in range, `gated` over the gate; a part whose weight is 0 has valid == false.
  struct PoseMoments {
    bool valid = false;
    double x = 0.0, y = 0.0, theta = 0.0;          // the means; theta = atan2(sum w sin, sum w cos)
    double cov_xx = 0.0, cov_xy = 0.0, cov_yy = 0.0;
    double resultant = 0.0;                        // the mean resultant length of the headings (1: all equal)
    double weight = 0.0;                           // W
    uint32_t poses = 0, alive = 0;                 // the poses of the set; those with a weight that is not 0
  };
  struct PoseEstimateResult {
    PoseMoments all, gated;
    uint32_t center = 0;                           // q_c
    bool center_out_of_range = false, some_out_of_range = false;
    uint32_t words[RPLGPU_ESTIMATE_WORDS] = {};    // the exact integers (the header's RESULT table)
  };
  bool estimate_pose(const std::vector<float> &poses, const std::vector<uint32_t> &weights,
                     const rplgpu_pose_estimate_t &spec, uint32_t center, PoseEstimateResult &result) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    const size_t n_poses = poses.size() / 4;
    if (n_poses == 0 || n_poses > RPLGPU_MAX_POSES || poses.size() != 4 * n_poses)
      return fail("estimate_pose: 1 .. RPLGPU_MAX_POSES poses of four floats");
    if (!weights.empty() && weights.size() != n_poses) return fail("estimate_pose: one weight per pose, or none");
    if (rplgpu_estimate_poses(h_, poses.data(), static_cast<uint32_t>(n_poses),
                              weights.empty() ? nullptr : weights.data(), &spec, center, result.words) != RPLGPU_OK)
      return note_error();
    result.center = result.words[1];
    result.center_out_of_range = (result.words[0] & 1u) != 0;
    result.some_out_of_range = (result.words[0] & 2u) != 0;
    PoseMoments *parts[2] = {&result.all, &result.gated};
    for (uint32_t k = 0; k < 2; ++k) {
      PoseMoments &m = *parts[k];
      m = PoseMoments();
      m.poses = result.words[2 + 2 * k];
      m.alive = result.words[3 + 2 * k];
      double v[8];
      if (rplgpu_estimate_pose(result.words, spec.xy_scale, k, v) != RPLGPU_OK) continue;  // W = 0
      m.valid = true;
      m.x = v[0];
      m.y = v[1];
      m.theta = v[2];
      m.cov_xx = v[3];
      m.cov_xy = v[4];
      m.cov_yy = v[5];
      m.resultant = v[6];
      m.weight = v[7];
    }
    return true;
  }

  // ext E18 (include/rplgpu_msg.h): `count` deltas (dc, ds, dx, dy) for resample_poses, each the odometry increment
  // (dx, dy, dtheta in the old base frame) with its own motion noise — the differential-drive model's four alphas
  // through rplgpu_motion_odometry, the draws from Philox4x32-10 under `spec` (seed; step: the time-step number, a
  // new stream per step; first: where this call's outputs start in a list made in pieces).  result: the health of
  // the draws, whose mean is 0 and whose variance is 2863311530.
  struct MotionNoiseResult {
    uint32_t nan_outputs = 0;   // deltas with a NaN entry (stored as 0x7FC00000)
    uint32_t max_abs = 0;       // the largest |Z| (at most 262140)
    int64_t sum = 0;            // the sum of Z over the 3 x count draws
    uint64_t sum_squares = 0;   // the sum of Z^2
    double mean = 0.0, variance = 0.0;
  };
  bool sample_motion(double dx, double dy, double dtheta, const double alpha[4], const rplgpu_motion_noise_t &spec,
                     uint32_t count, std::vector<float> &delta, MotionNoiseResult &result) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    if (count == 0 || count > RPLGPU_MAX_POSES) return fail("sample_motion: count must be in 1 .. RPLGPU_MAX_POSES");
    float odom[8];
    if (rplgpu_motion_odometry(dx, dy, dtheta, alpha, odom) != RPLGPU_OK) return fail("sample_motion: alpha is missing");
    delta.assign(4 * static_cast<size_t>(count), 0.0f);
    uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_sample_motion(h_, odom, count, &spec, delta.data(), words) != RPLGPU_OK) return note_error();
    result.nan_outputs = words[0];
    result.max_abs = words[1];
    result.sum = static_cast<int64_t>(static_cast<uint64_t>(words[2]) | (static_cast<uint64_t>(words[3]) << 32));
    result.sum_squares = static_cast<uint64_t>(words[4]) | (static_cast<uint64_t>(words[5]) << 32);
    const double n = 3.0 * static_cast<double>(count);
    result.mean = static_cast<double>(result.sum) / n;
    result.variance = static_cast<double>(result.sum_squares) / n - result.mean * result.mean;
    return true;
  }

  // ext E19 (include/rplgpu_msg.h): `count` poses (c, s, x, y) for score_poses / resample_poses, drawn uniformly over
  // the free cells of `grid` (width x height int8 cells as occupancy_grid or map_grid give them; free: spec.free_lo
  // <= cell <= spec.free_hi, by default the cells that are 0), each at one of `headings` evenly spaced headings
  // (rplgpu_seed_headings) and at a random place inside its cell, from Philox4x32-10 under `noise` (draw index 3: the
  // stream never meets sample_motion's under the same seed and step; first: where this call's outputs start in a list
  // made in pieces).  To inject count poses into a resampled list of M, seed with first = M - count and copy the
  // result over the list's last count poses.
  struct SeedResult {
    uint32_t free_cells = 0;    // F (width x height when no cell was free)
    uint32_t off_cell = 0;      // outputs float32 rounding put into a neighbouring cell (an origin far from 0)
    uint32_t min_cell = 0;      // the smallest and the largest chosen cell index cy * width + cx
    uint32_t max_cell = 0;
    bool none_free = false;     // no cell was free: the poses lie anywhere on the grid
  };
  bool seed_poses(const rplgpu_pose_seed_t &spec, const std::vector<int8_t> &grid, uint32_t headings,
                  const rplgpu_motion_noise_t &noise, uint32_t count, std::vector<float> &poses, SeedResult &result) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    if (rplgpu_pose_seed_check(&spec) != RPLGPU_OK) return fail("seed_poses: rplgpu_pose_seed_check refuses the spec");
    if (grid.size() != static_cast<size_t>(spec.width) * spec.height)
      return fail("seed_poses: the grid must hold width x height cells");
    if (count == 0 || count > RPLGPU_MAX_POSES) return fail("seed_poses: count must be in 1 .. RPLGPU_MAX_POSES");
    std::vector<float> table(2 * static_cast<size_t>(headings ? headings : 1));
    if (rplgpu_seed_headings(headings, table.data()) != RPLGPU_OK)
      return fail("seed_poses: headings must be in 1 .. 65536");
    poses.assign(4 * static_cast<size_t>(count), 0.0f);
    uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_seed_poses(h_, &spec, grid.data(), table.data(), headings, count, &noise, poses.data(), nullptr,
                          words) != RPLGPU_OK)
      return note_error();
    result.free_cells = words[0];
    result.off_cell = words[1];
    result.min_cell = words[2];
    result.max_cell = words[3];
    result.none_free = (words[7] & 1u) != 0;
    return true;
  }

  // ext E20 (include/rplgpu_msg.h): the poses (c, s, x, y) of score_poses / resample_poses binned in (x, y, heading) —
  // spec.inv_size bins per metre from the corner (origin_x, origin_y), `headings` evenly spaced heading bins
  // (rplgpu_seed_headings' table as the edges) — and marked in the bit map `map` (bin b: bit b & 31 of word b >> 5);
  // a pose whose weight is 0 is skipped (weights empty: every pose counts).  With spec.flags bit 0 (KEEP) the bits
  // are ORed into `map` as it stands, so a list can be counted in pieces.  result.samples(...) is the size AMCL's
  // KLD sampling gives the next list (the M of resample_poses).
  struct BinResult {
    uint32_t new_bins = 0;      // K: the bits this call set (without KEEP: the occupied bins)
    uint32_t counted = 0;       // poses binned
    uint32_t out_of_range = 0;  // poses outside the bins, or with a heading that has no direction
    uint32_t skipped = 0;       // poses whose weight is 0
    uint32_t min_bin = 0;       // the smallest and the largest bin id of a counted pose
    uint32_t max_bin = 0;
    bool none_counted = false;
    uint32_t samples(double epsilon = 0.01, double z = 3.0, uint32_t m_min = 500, uint32_t m_max = 100000) const {
      return rplgpu_kld_samples(new_bins, epsilon, z, m_min, m_max);
    }
  };
  bool bin_poses(const rplgpu_pose_bins_t &spec, const std::vector<float> &poses, const std::vector<uint32_t> &weights,
                 uint32_t headings, std::vector<uint32_t> &map, BinResult &result) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    if (rplgpu_pose_bins_check(&spec, headings) != RPLGPU_OK)
      return fail("bin_poses: rplgpu_pose_bins_check refuses the spec or the number of heading bins");
    const size_t count = poses.size() / 4;
    if (count == 0 || count > RPLGPU_MAX_POSES || poses.size() != 4 * count)
      return fail("bin_poses: poses must hold 1 .. RPLGPU_MAX_POSES entries of four floats");
    if (!weights.empty() && weights.size() != count) return fail("bin_poses: one weight per pose, or none");
    std::vector<float> table(2 * static_cast<size_t>(headings));
    if (rplgpu_seed_headings(headings, table.data()) != RPLGPU_OK) return fail("bin_poses: no heading table");
    const size_t words = (static_cast<size_t>(spec.nx) * spec.ny * headings + 31) / 32;
    if (map.size() != words) map.assign(words, 0u);  // (any other size starts an empty map)
    uint32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_bin_poses(h_, &spec, poses.data(), static_cast<uint32_t>(count),
                         weights.empty() ? nullptr : weights.data(), table.data(), headings, map.data(), nullptr,
                         out) != RPLGPU_OK)
      return note_error();
    result.new_bins = out[0];
    result.counted = out[1];
    result.out_of_range = out[2];
    result.skipped = out[3];
    result.min_bin = out[4];
    result.max_bin = out[5];
    result.none_counted = (out[7] & 1u) != 0;
    return true;
  }

  // ext E21 (include/rplgpu_msg.h): the occupied bins of bin_poses' `map` clustered (26 neighbours, the heading axis
  // wrapping with spec.flags bit 0), each pose given the cluster of its bin (`bins`: rplgpu_bin_poses' bin ids, one
  // per pose) and the HEAVIEST cluster reduced to a pose — what AMCL publishes (pf_cluster_stats).  best is the mean
  // over the heaviest cluster, whole the mean over every clustered pose; `clusters` receives up to max_clusters rows
  // in ascending label order.
  struct Cluster {
    uint32_t label = 0;         // the cluster's smallest bin id
    uint32_t poses = 0;
    uint64_t weight = 0;
  };
  struct ClusterResult {
    uint32_t clusters = 0;      // N_c
    uint32_t occupied_bins = 0;  // K
    uint32_t best_label = 0xFFFFFFFFu, second_label = 0xFFFFFFFFu;
    uint32_t best_poses = 0, second_poses = 0;
    uint64_t second_weight = 0;
    uint32_t stray = 0, unlabelled = 0;
    uint32_t flags = 0;         // result word 0
    bool best_valid = false, whole_valid = false;  // W of the set is not 0
    double best[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // rplgpu_estimate_pose's eight values for set 1
    double whole[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ... and for set 0
  };
  bool cluster_poses(const rplgpu_pose_clusters_t &spec, const std::vector<float> &poses,
                     const std::vector<uint32_t> &weights, uint32_t headings, const std::vector<uint32_t> &map,
                     const std::vector<uint32_t> &bins, uint32_t max_clusters, std::vector<Cluster> &clusters,
                     ClusterResult &result) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    if (rplgpu_pose_clusters_check(&spec, headings) != RPLGPU_OK)
      return fail("cluster_poses: rplgpu_pose_clusters_check refuses the spec or the number of heading bins");
    const size_t count = poses.size() / 4;
    if (count == 0 || count > RPLGPU_MAX_POSES || poses.size() != 4 * count)
      return fail("cluster_poses: poses must hold 1 .. RPLGPU_MAX_POSES entries of four floats");
    if (!weights.empty() && weights.size() != count) return fail("cluster_poses: one weight per pose, or none");
    if (bins.size() != count) return fail("cluster_poses: one bin id per pose");
    if (map.size() != (static_cast<size_t>(spec.nx) * spec.ny * headings + 31) / 32)
      return fail("cluster_poses: the map must hold ceil(nx * ny * headings / 32) words");
    std::vector<uint32_t> rows(4 * static_cast<size_t>(max_clusters), 0u);
    uint32_t out[RPLGPU_CLUSTER_WORDS];
    if (rplgpu_cluster_poses(h_, &spec, poses.data(), static_cast<uint32_t>(count),
                             weights.empty() ? nullptr : weights.data(), headings, map.data(), bins.data(), nullptr,
                             max_clusters ? rows.data() : nullptr, max_clusters, out) != RPLGPU_OK)
      return note_error();
    result = ClusterResult();
    result.flags = out[0];
    result.best_label = out[1];
    result.best_poses = out[4];
    result.clusters = out[6];
    result.occupied_bins = out[7];
    result.second_label = out[72];
    result.second_poses = out[73];
    result.second_weight = static_cast<uint64_t>(out[74]) | (static_cast<uint64_t>(out[75]) << 32);
    result.stray = out[76];
    result.unlabelled = out[77];
    result.whole_valid = rplgpu_estimate_pose(out, spec.xy_scale, 0, result.whole) == RPLGPU_OK;
    result.best_valid = rplgpu_estimate_pose(out, spec.xy_scale, 1, result.best) == RPLGPU_OK;
    clusters.clear();
    for (uint32_t c = 0; c < max_clusters && c < result.clusters; ++c) {
      Cluster row;
      row.label = rows[4 * c];
      row.poses = rows[4 * c + 1];
      row.weight = static_cast<uint64_t>(rows[4 * c + 2]) | (static_cast<uint64_t>(rows[4 * c + 3]) << 32);
      clusters.push_back(row);
    }
    return true;
  }

  // ext E22 (include/rplgpu_msg.h): a ray from every pose (c, s, x, y) along every beam (cb, sb) of `beams` through the
  // int8 grid to the first cell that stops it (AMCL's map_calc_range) — the beam model's expected ranges.  `ranges`
  // (optional) receives poses x beams range words (rplgpu_cast_range_m turns one into metres).  With `measured` not
  // empty (a merged LaserScan's ranges; beam a is entry meas_first + a * meas_step) each ray is compared with its
  // beam's measured range through `table` (2 * spec.table_half + 2 bytes) and the terms are summed into `weights`, one
  // per pose, in score_poses' layout: resample_poses, estimate_pose and bin_poses take them unchanged.
  struct CastResult {
    uint32_t hit = 0, unknown = 0, left = 0, none = 0, dropped = 0;  // rays by how they ended
    uint32_t max_hit_d2 = 0;    // the largest squared distance (cells) among the rays that hit
    uint64_t steps = 0;         // cell steps walked
    uint32_t best_weight = 0, best_index = 0, best_count = 0, zero_weights = 0, beams_used = 0;
    uint64_t weight_sum = 0;
  };
  bool cast_ranges(const rplgpu_range_cast_t &spec, const std::vector<float> &poses, const std::vector<float> &beams,
                   const std::vector<int8_t> &grid, const std::vector<float> &measured, uint32_t meas_first,
                   uint32_t meas_step, const std::vector<uint8_t> &table, std::vector<uint32_t> *ranges,
                   std::vector<uint32_t> &weights, CastResult &result) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    if (rplgpu_range_cast_check(&spec) != RPLGPU_OK) return fail("cast_ranges: rplgpu_range_cast_check refuses the spec");
    const size_t count = poses.size() / 4, n_beams = beams.size() / 2;
    if (count == 0 || count > RPLGPU_MAX_POSES || poses.size() != 4 * count)
      return fail("cast_ranges: poses must hold 1 .. RPLGPU_MAX_POSES entries of four floats");
    if (n_beams == 0 || n_beams > RPLGPU_MAX_MERGE_BEAMS || beams.size() != 2 * n_beams ||
        count * n_beams > RPLGPU_MAX_CAST_RAYS)
      return fail("cast_ranges: beams must hold 1 .. RPLGPU_MAX_MERGE_BEAMS entries of two floats, poses x beams <= 2^28");
    if (grid.size() != static_cast<size_t>(spec.width) * spec.height) return fail("cast_ranges: grid is not width x height");
    const bool weigh = !measured.empty();
    if (!weigh && !ranges) return fail("cast_ranges: neither ranges nor a measured scan");
    if (weigh && table.size() != 2 * static_cast<size_t>(spec.table_half) + 2)
      return fail("cast_ranges: table must hold 2 * table_half + 2 bytes");
    std::vector<uint32_t> r_out(ranges ? count * n_beams : 0), w_out(weigh ? count : 0);
    uint32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cast[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rplgpu_cast_ranges(h_, &spec, poses.data(), static_cast<uint32_t>(count), beams.data(),
                           static_cast<uint32_t>(n_beams), grid.data(), weigh ? measured.data() : nullptr,
                           static_cast<uint32_t>(measured.size()), meas_first, meas_step, weigh ? table.data() : nullptr,
                           ranges ? r_out.data() : nullptr, weigh ? w_out.data() : nullptr, out, cast) != RPLGPU_OK)
      return note_error();
    result = CastResult();
    result.hit = cast[0];
    result.unknown = cast[1];
    result.left = cast[2];
    result.none = cast[3];
    result.dropped = cast[4];
    result.max_hit_d2 = cast[5];
    result.steps = static_cast<uint64_t>(cast[6]) | (static_cast<uint64_t>(cast[7]) << 32);
    if (weigh) {
      result.best_weight = out[0];
      result.best_index = out[1];
      result.best_count = out[2];
      result.zero_weights = out[3];
      result.beams_used = out[4];
      result.weight_sum = static_cast<uint64_t>(out[6]) | (static_cast<uint64_t>(out[7]) << 32);
      weights.swap(w_out);
    }
    if (ranges) ranges->swap(r_out);
    return true;
  }

  // ext E14 (include/rplgpu_msg.h): the scans of ONE time step ADDED into a persistent hit / miss count map at the
  // poses given (e.g. the ones match_scans corrected) — what a mapper's map update does per accepted scan.
  // `counts` holds two words per cell (misses, hits); any other size than 2 x width x height starts a zeroed map.
  // pose2d / motion / t0 as in fill_occupancy_grid.
  template <class NodeT>
  bool update_map(const std::vector<std::vector<NodeT>> &scans, const ScanConfig &cfg, const rplgpu_occ_grid_t &grid,
                  const float *pose2d, const float *motion, const float *t0, std::vector<uint32_t> &counts,
                  uint32_t *status = nullptr) {
    if (scans.empty()) return false;
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    size_t stride = 1;
    for (const auto &s : scans) stride = s.size() > stride ? s.size() : stride;
    if (stride > max_n_) return fail("scan larger than the configured capacity");
    occ_nodes_.assign(scans.size() * stride, rplgpu_node_t{});
    occ_len_.resize(scans.size());
    for (size_t b = 0; b < scans.size(); ++b) {
      if (!scans[b].empty()) std::memcpy(&occ_nodes_[b * stride], scans[b].data(), scans[b].size() * 8);
      occ_len_[b] = static_cast<uint32_t>(scans[b].size());
    }
    const size_t n_words = 2 * static_cast<size_t>(grid.width) * grid.height;
    if (n_words == 0) return fail("update_map: the grid has no cells");
    if (counts.size() != n_words) counts.assign(n_words, 0u);
    const rplgpu_params_t p = cfg.to_params();
    if (rplgpu_map_update(h_, occ_nodes_.data(), static_cast<uint32_t>(stride), occ_len_.data(),
                          static_cast<uint32_t>(scans.size()), &p, motion, pose2d, t0, &grid, counts.data(),
                          status) != RPLGPU_OK)
      return note_error();
    return true;
  }

  // ext E14: the count map through the cell rule into a nav_msgs/OccupancyGrid-shaped message, which inflate_grid,
  // match_scans and fill_occupancy_grid (as the previous grid) take.  `grid_msg.data` of the right size is the
  // previous grid (cells seen fewer than rule.min_observations times keep their value); any other size starts
  // from unknown (-1).  cells (optional): result cells that are -1, 0, 100 and anything else.
  template <class OccupancyGridT>
  bool fill_map_grid(const std::vector<uint32_t> &counts, const rplgpu_occ_grid_t &grid,
                     const rplgpu_map_rule_t &rule, OccupancyGridT &grid_msg, uint32_t cells[4] = nullptr) {
    if (!h_) return fail("rplgpu handle not configured");
    last_error_.clear();
    const size_t n_cells = static_cast<size_t>(grid.width) * grid.height;
    if (n_cells == 0 || counts.size() != 2 * n_cells) return fail("fill_map_grid: counts is not 2 x width x height");
    const bool has_prev = grid_msg.data.size() == n_cells;
    if (has_prev) occ_prev_.assign(grid_msg.data.begin(), grid_msg.data.end());
    occ_out_.resize(n_cells);
    if (rplgpu_map_grid(h_, counts.data(), grid.width, grid.height, &rule, has_prev ? occ_prev_.data() : nullptr,
                        occ_out_.data(), cells) != RPLGPU_OK)
      return note_error();
    grid_msg.info.resolution = grid.resolution;
    grid_msg.info.width = grid.width;
    grid_msg.info.height = grid.height;
    grid_msg.info.origin.position.x = grid.origin_x;
    grid_msg.info.origin.position.y = grid.origin_y;
    grid_msg.info.origin.position.z = 0.0;
    grid_msg.info.origin.orientation.x = 0.0;
    grid_msg.info.origin.orientation.y = 0.0;
    grid_msg.info.origin.orientation.z = 0.0;
    grid_msg.info.origin.orientation.w = 1.0;
    grid_msg.data.assign(occ_out_.begin(), occ_out_.begin() + n_cells);
    return true;
  }

 private:
  bool fail(const char *msg) {
    last_error_ = msg;
    return false;
  }
  bool note_error() {
    last_error_ = h_ ? rplgpu_last_error(h_) : "rplgpu handle not configured";
    return false;
  }
  rplgpu_handle_t h_ = nullptr;
  uint32_t max_n_ = 0;
  std::vector<float> ranges_, intens_, xyzi_;
  std::vector<rplgpu_node_t> dec_nodes_;
  std::vector<uint32_t> dec_resets_;
  std::vector<rplgpu_node_t> occ_nodes_;
  std::vector<uint32_t> occ_len_;
  std::vector<int8_t> occ_prev_, occ_out_;
  std::vector<float> pose_list_;
  std::string last_error_;
  uint32_t min_samples_ = 0;
};

// == ScanDataHolder<T> as SlamtecLidarDriver drives it (src/sdk/src/sl_lidar_driver.cpp:236-360,
// :1645-1653): a listener for replay_recording that assembles scans.  A node with flag bit 0
// closes the scan being built and opens the next one; nodes before the first sync node, or after
// a rewind until the next sync node, are discarded; a scan that reached max_count nodes keeps
// overwriting its last slot.  `on_scan(std::vector<rplgpu_node_t>&)` receives every completed
// scan (the SDK instead parks it for grabScanDataHq).  Host-side bookkeeping, no arithmetic: for
// batches the same rules run on the device (rplgpu_segment_batch_dev).
template <class OnScan>
class ScanAssembler {
 public:
  explicit ScanAssembler(OnScan on_scan, size_t max_count = 8192)
      : on_scan_(on_scan), max_count_(max_count ? max_count : 1) {}
  void onHQNodeScanResetReq() { cur_.clear(); }
  void onHQNodeDecoded(unsigned long long, const rplgpu_node_t *node) {
    if (node->flag & 1u) {
      if (!cur_.empty()) {
        on_scan_(cur_);
        cur_.clear();
      }
    } else if (cur_.empty()) {
      return;
    }
    if (cur_.size() >= max_count_) cur_.back() = *node;
    else cur_.push_back(*node);
  }

 private:
  OnScan on_scan_;
  size_t max_count_;
  std::vector<rplgpu_node_t> cur_;
};

// == DummyLidarDriver::grab_scan_data's synthetic ring (src/lidar_driver_wrapper.cpp:441-471),
// the reference's only fake backend (config 1): 360 nodes, one per degree, 2 m +- 0.5 m,
// quality 200, phase advancing 0.1 rad per scan.  `phase` is the caller's copy of the
// reference's function-static accumulator.
template <class NodeT>
inline void dummy_scan(float &phase, std::vector<NodeT> &nodes) {
  static_assert(sizeof(NodeT) == 8, "node must be the packed 8-byte SDK record");
  const int count = 360;
  nodes.clear();
  nodes.reserve(count);
  phase += 0.1f;  // :450
  for (int i = 0; i < count; ++i) {
    rplgpu_node_t nd;
    nd.angle_z_q14 = static_cast<uint16_t>(static_cast<float>(i) * 16384.0f / 90.0f);  // :456
    const float dist_meters = 2.0f + 0.5f * std::sin(static_cast<float>(i) * 3.141592f / 180.0f + phase);
    nd.dist_mm_q2 = static_cast<uint32_t>(dist_meters * 1000.0f * 4.0f);               // :463
    nd.quality = 200;                                                                  // :464
    nd.flag = 0;
    NodeT out;
    std::memcpy(&out, &nd, 8);
    nodes.push_back(out);
  }
}

}  // namespace rplgpu_host
