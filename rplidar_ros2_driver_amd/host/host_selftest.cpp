// host_selftest — drives the C++ host mirror (rplgpu_host.hpp) exactly the way the patched
// node would: grab_scan_data-style ascend, then the publish_scan body and the
// PointCloud2 extension, on a raw scan read from a file (8-byte nodes), and dumps the
// resulting messages as flat binary so that a test can compare them with the oracle.
//
//   host_selftest <nodes.bin> <out.bin> <is_new> <inverted> <scan_processing> <ascend 0|1> <cloud 0|1|2>
//   out.bin: u32 published, 7 x f32 meta, u32 count, ranges[count], intensities[count],
//            u32 sl_result, u32 n_points, xyzi[4*n_points]
//   host_selftest replay <ans_type> <sample_duration_us> <stream.bin> <out.bin>
//   out.bin: u32 n_nodes, u32 n_reset_calls, u32 n_err, u32 n_scans, nodes[n_nodes],
//            reset positions, then per scan: u32 len, nodes[len]   (replay_recording + ScanAssembler)
//   host_selftest serialized <nodes.bin> <out.bin> <is_new> <inverted> <scan_processing> <cloud 1|2>
//   out.bin: u32 published, u32 len_scan, LaserScan message bytes, u32 len_cloud, PointCloud2
//            message bytes   (frame_id "laser_frame", stamp 1727000000.123456789, duration 0.125)
//   no arguments: config-1 smoke run (3 Dummy scans through the whole path), then the E11 mirror call once
//   against a three-ray known answer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "rplgpu_host.hpp"

namespace {
struct PointField {
  std::string name;
  uint32_t offset = 0;
  uint8_t datatype = 0;
  uint32_t count = 0;
};
struct LaserScan {  // field names of sensor_msgs/msg/LaserScan
  float angle_min = 0, angle_max = 0, angle_increment = 0, time_increment = 0, scan_time = 0;
  float range_min = 0, range_max = 0;
  std::vector<float> ranges, intensities;
};
struct PointCloud2 {  // field names of sensor_msgs/msg/PointCloud2
  uint32_t height = 0, width = 0;
  std::vector<PointField> fields;
  bool is_bigendian = false;
  uint32_t point_step = 0, row_step = 0;
  std::vector<uint8_t> data;
  bool is_dense = false;
};
struct OccupancyGrid {  // field names of nav_msgs/msg/OccupancyGrid (header left out)
  struct {
    float resolution = 0;
    uint32_t width = 0, height = 0;
    struct {
      struct { double x = 0, y = 0, z = 0; } position;
      struct { double x = 0, y = 0, z = 0, w = 0; } orientation;
    } origin;
  } info;
  std::vector<int8_t> data;
};
struct RclSerialized {  // the fields of rcl_serialized_message_t (rcutils_uint8_array_t) used here
  uint8_t *buffer = nullptr;
  size_t buffer_length = 0, buffer_capacity = 0;
};
class SerializedMessage {  // the two rclcpp::SerializedMessage members the host mirror calls
 public:
  void reserve(size_t capacity) {
    if (capacity > store_.size()) store_.resize(capacity);
    raw_.buffer = store_.data();
    raw_.buffer_capacity = store_.size();
  }
  RclSerialized &get_rcl_serialized_message() { return raw_; }
 private:
  std::vector<uint8_t> store_;
  RclSerialized raw_;
};
std::vector<rplgpu_node_t> read_nodes(const char *path, bool *ok) {
  std::vector<rplgpu_node_t> nodes;
  *ok = false;
  std::FILE *f = std::fopen(path, "rb");
  if (!f) return nodes;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  nodes.resize(static_cast<size_t>(bytes) / 8);
  *ok = nodes.empty() || std::fread(nodes.data(), 8, nodes.size(), f) == nodes.size();
  std::fclose(f);
  return nodes;
}
}  // namespace

int main(int argc, char **argv) {
  rplgpu_host::ScanPath path;
  if (!path.configure(0, 32768)) {
    std::fprintf(stderr, "configure failed: %s\n", path.last_error().c_str());
    return 2;
  }
  if (argc == 6 && std::string(argv[1]) == "replay") {
    struct Recorder {  // what SlamtecLidarDriver's listener would see, plus the scan assembly
      std::vector<rplgpu_node_t> nodes;
      std::vector<uint32_t> resets;
      std::vector<std::vector<rplgpu_node_t>> scans;
    } rec;
    auto on_scan = [&](std::vector<rplgpu_node_t> &s) { rec.scans.push_back(s); };
    rplgpu_host::ScanAssembler<decltype(on_scan)> assembler(on_scan, 8192);
    struct Tee {
      Recorder &r;
      rplgpu_host::ScanAssembler<decltype(on_scan)> &a;
      void onHQNodeScanResetReq() {
        r.resets.push_back(static_cast<uint32_t>(r.nodes.size()));
        a.onHQNodeScanResetReq();
      }
      void onHQNodeDecoded(unsigned long long ts, const rplgpu_node_t *n) {
        r.nodes.push_back(*n);
        a.onHQNodeDecoded(ts, n);
      }
    } tee{rec, assembler};
    std::FILE *f = std::fopen(argv[4], "rb");
    if (!f) return 4;
    std::fseek(f, 0, SEEK_END);
    const long nb = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> bytes(static_cast<size_t>(nb));
    if (nb && std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 4;
    std::fclose(f);
    int32_t state[4] = {0, 0, 0, 0};
    uint32_t n_err = 0;
    if (!path.replay_recording(static_cast<uint8_t>(std::strtoul(argv[2], nullptr, 0)),
                               static_cast<uint32_t>(std::atoi(argv[3])), bytes.data(), bytes.size(),
                               tee, state, &n_err)) {
      std::fprintf(stderr, "replay failed: %s\n", path.last_error().c_str());
      return 5;
    }
    std::FILE *o = std::fopen(argv[5], "wb");
    if (!o) return 6;
    const uint32_t hdr[4] = {static_cast<uint32_t>(rec.nodes.size()), static_cast<uint32_t>(rec.resets.size()),
                             n_err, static_cast<uint32_t>(rec.scans.size())};
    std::fwrite(hdr, 4, 4, o);
    std::fwrite(rec.nodes.data(), 8, rec.nodes.size(), o);
    std::fwrite(rec.resets.data(), 4, rec.resets.size(), o);
    for (auto &s : rec.scans) {
      const uint32_t len = static_cast<uint32_t>(s.size());
      std::fwrite(&len, 4, 1, o);
      std::fwrite(s.data(), 8, s.size(), o);
    }
    std::fclose(o);
    return 0;
  }
  if (argc == 8 && std::string(argv[1]) == "serialized") {
    bool ok = false;
    const std::vector<rplgpu_node_t> nodes = read_nodes(argv[2], &ok);
    if (!ok) return 4;
    rplgpu_host::ScanConfig cfg;
    cfg.is_new_protocol = std::atoi(argv[4]) != 0;
    cfg.inverted = std::atoi(argv[5]) != 0;
    cfg.scan_processing = std::atoi(argv[6]) != 0;
    cfg.cached_current_max_range = 40.0f;
    SerializedMessage scan_msg, cloud_msg;
    scan_msg.reserve(16);
    cloud_msg.reserve(16);
    const bool published = path.fill_serialized_laser_scan(nodes, cfg, 0.125, "laser_frame",
                                                           1727000000, 123456789u, scan_msg);
    cfg.clip_enable = true;
    cfg.voxel_enable = std::atoi(argv[7]) == 2;
    if (!path.fill_serialized_point_cloud2(nodes, cfg, "laser_frame", 1727000000, 123456789u,
                                           cloud_msg) && !nodes.empty()) {
      std::fprintf(stderr, "cloud failed: %s\n", path.last_error().c_str());
      return 5;
    }
    std::FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 6;
    const uint32_t pub = published ? 1u : 0u;
    const auto &a = scan_msg.get_rcl_serialized_message();
    const auto &c = cloud_msg.get_rcl_serialized_message();
    const uint32_t la = static_cast<uint32_t>(a.buffer_length), lc = static_cast<uint32_t>(c.buffer_length);
    std::fwrite(&pub, 4, 1, o);
    std::fwrite(&la, 4, 1, o);
    std::fwrite(a.buffer, 1, la, o);
    std::fwrite(&lc, 4, 1, o);
    std::fwrite(c.buffer, 1, lc, o);
    std::fclose(o);
    return 0;
  }
  if (argc < 8) {
    float phase = 0.0f;
    std::vector<rplgpu_node_t> nodes;
    rplgpu_host::ScanConfig cfg;
    cfg.cached_current_max_range = 40.0f;  // Dummy hw limit, src/lidar_driver_wrapper.cpp:439
    for (int s = 0; s < 3; ++s) {
      rplgpu_host::dummy_scan(phase, nodes);
      LaserScan msg;
      if (!path.fill_laser_scan(nodes, cfg, 0.1, msg) || msg.ranges.size() != 360) {
        std::fprintf(stderr, "dummy scan %d failed: %s\n", s, path.last_error().c_str());
        return 3;
      }
      std::printf("dummy scan %d: %zu beams, ranges[0]=%.6f intensities[0]=%.1f\n", s,
                  msg.ranges.size(), msg.ranges[0], msg.intensities[0]);
    }
    // E11, three rays along +x from a sensor in cell (0, 1) of an 8 x 3 grid of 1 m cells: the return at 2 m
    // marks cell 2, the one at 4 m (beyond obstacle_max) only clears up to cell 3, the one at 7 m is cut at
    // 5 m and clears up to cell 5 — the cut end included.
    std::vector<std::vector<rplgpu_node_t>> step(1);
    for (uint32_t d : {8000u, 16000u, 28000u}) {
      rplgpu_node_t nd{};
      nd.dist_mm_q2 = d;
      nd.quality = 200;
      step[0].push_back(nd);
    }
    const rplgpu_occ_grid_t og = {-0.5f, -1.5f, 1.0f, 8, 3, 0.0f, 3.2f, 5.0f};
    OccupancyGrid grid_msg;
    uint32_t cells[3] = {0, 0, 0}, status = 99;
    if (!path.fill_occupancy_grid(step, rplgpu_host::ScanConfig(), og, nullptr, nullptr, nullptr, grid_msg, cells,
                                  &status)) {
      std::fprintf(stderr, "occupancy grid failed: %s\n", path.last_error().c_str());
      return 7;
    }
    static const int8_t want[24] = {-1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 100, 0, 0, 0, -1, -1,
                                    -1, -1, -1, -1, -1, -1, -1, -1};
    if (grid_msg.data.size() != 24 || std::memcmp(grid_msg.data.data(), want, 24) != 0 || cells[0] != 5 ||
        cells[1] != 1 || cells[2] != 18 || status != 0 || grid_msg.info.width != 8 ||
        grid_msg.info.origin.orientation.w != 1.0) {
      std::fprintf(stderr, "occupancy grid: wrong answer\n");
      return 8;
    }
    std::printf("occupancy grid: 3 rays, cells 0/100/-1 = %u/%u/%u\n", cells[0], cells[1], cells[2]);
    // E12 over that grid: its one lethal cell (2, 1) with 1 m cells, inscribed 1 m, inflation 2 m, scaling 1 / m.
    // The cleared cells 1 and 3 of its row become 99 and cells 0 and 4 become 36 (98 exp(-1) = 36.05); the
    // unknown cells above and below it (distance 1) become 99, every other unknown cell stays -1 (64 < 99).
    const rplgpu_inflation_t inf = {1.0f, 2.0f, 1.0f, 0};
    OccupancyGrid cost_msg;
    uint32_t icells[4] = {9, 9, 9, 9};
    if (!path.inflate_grid(grid_msg, inf, cost_msg, icells)) {
      std::fprintf(stderr, "inflation failed: %s\n", path.last_error().c_str());
      return 9;
    }
    static const int8_t cost_want[24] = {-1, -1, 99, -1, -1, -1, -1, -1, 36, 99, 100, 99, 36, 0, -1, -1,
                                         -1, -1, 99, -1, -1, -1, -1, -1};
    if (cost_msg.data.size() != 24 || std::memcmp(cost_msg.data.data(), cost_want, 24) != 0 || icells[0] != 1 ||
        icells[1] != 4 || icells[2] != 2 || icells[3] != 16 || cost_msg.info.width != 8) {
      std::fprintf(stderr, "inflation: wrong answer\n");
      return 10;
    }
    std::printf("inflation: cells 100/99/1..98/-1 = %u/%u/%u/%u\n", icells[0], icells[1], icells[2], icells[3]);
    // E13 against that costmap: the return at 2 m alone, seen from a prior 1 m behind the true pose (sensor in
    // cell (-1, 1)), lands in cell (1, 1) = 99; one cell to the right it meets the lethal cell (2, 1) = 100, and
    // no other shift of a 2 x 1 window reaches 100: best (k, j, i) = (0, 0, 1), unambiguous.
    std::vector<std::vector<rplgpu_node_t>> one(1);
    one[0].push_back(step[0][0]);
    const float prior[6] = {1.0f, 0.0f, -1.0f, 0.0f, 1.0f, 0.0f};
    rplgpu_scan_match_t win;
    rplgpu_default_scan_match(&win);
    win.shift_x = 2;
    win.shift_y = 1;
    win.rot_steps = 0;
    rplgpu_host::ScanPath::MatchResult mr;
    uint32_t mstatus = 99;
    if (!path.match_scans(one, rplgpu_host::ScanConfig(), prior, nullptr, nullptr, nullptr, cost_msg, win, mr,
                          &mstatus)) {
      std::fprintf(stderr, "scan match failed: %s\n", path.last_error().c_str());
      return 11;
    }
    if (mr.score != 100 || mr.k != 0 || mr.j != 0 || mr.i != 1 || mr.points != 1 || mr.score_at_prior != 99 ||
        mr.ties != 1 || mstatus != 0) {
      std::fprintf(stderr, "scan match: wrong answer (%u at %d %d %d, %u points, %u at the prior, %u ties)\n", mr.score,
                   mr.k, mr.j, mr.i, mr.points, mr.score_at_prior, mr.ties);
      return 12;
    }
    std::printf("scan match: best %u at (k, j, i) = (%d, %d, %d), %u at the prior\n", mr.score, mr.k, mr.j, mr.i,
                mr.score_at_prior);
    // E24 on the same return and costmap with a window of 12 x 9 cells (4 x 3 blocks of 8 x 8 shifts): only the
    // block of shifts i in [-4, 3], j in [-1, 6] has the lethal cell under its pooled look-up, it is both seeds, its
    // best score 100 is the floor and no other bound reaches it: one block listed, E13's answer, proven.
    rplgpu_wide_match_t wide;
    rplgpu_default_wide_match(&wide);
    wide.shift_x = 12;
    wide.shift_y = 9;
    wide.rot_steps = 0;
    rplgpu_host::ScanPath::WideMatchResult wr;
    uint32_t wstatus = 99;
    if (!path.match_wide(one, rplgpu_host::ScanConfig(), prior, nullptr, nullptr, nullptr, cost_msg, wide, wr,
                         &wstatus)) {
      std::fprintf(stderr, "wide scan match failed: %s\n", path.last_error().c_str());
      return 11;
    }
    if (wr.score != 100 || wr.k != 0 || wr.j != 0 || wr.i != 1 || wr.points != 1 || wr.score_at_prior != 99 ||
        wr.ties != 1 || !wr.proven || wr.blocks != 12 || wr.greatest_bound != 100 || wr.floor != 100 ||
        wr.listed != 1 || wstatus != 0) {
      std::fprintf(stderr, "wide scan match: wrong answer (%u at %d %d %d, %u ties, proven %d, %u of %u blocks, bound %u, floor %u)\n",
                   wr.score, wr.k, wr.j, wr.i, wr.ties, (int)wr.proven, wr.listed, wr.blocks, wr.greatest_bound,
                   wr.floor);
      return 12;
    }
    std::printf("wide scan match: best %u at (k, j, i) = (%d, %d, %d), %u of %u blocks scored\n", wr.score, wr.k, wr.j,
                wr.i, wr.listed, wr.blocks);
    // E25 on the same return and costmap: one point is fewer than min_points, so the one pose is not stepped and
    // comes back bit for bit; the sums still count the point.
    rplgpu_pose_refine_t refine;
    rplgpu_default_pose_refine(&refine);
    refine.target = 100;
    std::vector<float> fposes = {1.0f, 0.0f, 0.25f, -0.5f};
    std::vector<uint32_t> fsums;
    rplgpu_host::ScanPath::RefineResult fr;
    uint32_t fstatus = 99;
    if (!path.refine_poses(one, rplgpu_host::ScanConfig(), prior, nullptr, nullptr, cost_msg, refine, 2, fposes, fr,
                           &fsums, &fstatus)) {
      std::fprintf(stderr, "pose refinement failed: %s\n", path.last_error().c_str());
      return 11;
    }
    if (fr.stepped != 0 || fr.too_few != 1 || fr.singular != 0 || fr.clamped != 0 || fr.best_index != 0 ||
        fr.points != 1 || fsums.size() != 32 || fsums[27] + fsums[28] != 1 || fposes[0] != 1.0f ||
        fposes[1] != 0.0f || fposes[2] != 0.25f || fposes[3] != -0.5f || fstatus != 0) {
      std::fprintf(stderr, "pose refinement: wrong answer (%u stepped, %u too few, %u points)\n", fr.stepped,
                   fr.too_few, fr.points);
      return 12;
    }
    std::printf("pose refinement: %u of 1 poses stepped on %u point(s), %u too few\n", fr.stepped, fr.points,
                fr.too_few);
    // E26 over that costmap with lethal 100 and unknown cells at 60: the goal in the free cell (5, 1).  Cell (0, 1)
    // (byte 36, weight 122) cannot pass the lethal cell (2, 1) along its row; steps 4 (+1, +1) and 6 (+1, -1) both cost
    // 2260 + 7 * 122 = 3114 and the lower number wins, so its path runs below the row: cells 8 17 18 19 20 13.
    rplgpu_nav_field_t nav;
    rplgpu_default_nav_field(&nav);
    nav.lethal = 100;
    nav.unknown_cost = 60;
    nav.rounds = 1;  // one tile: the door's second call finds nothing dirty
    std::vector<uint32_t> potential, ninfo;
    std::vector<std::vector<uint32_t>> npaths;
    const std::vector<uint32_t> ngoals = {13u, 24u}, nstarts = {8u, 10u};
    rplgpu_host::ScanPath::NavResult nr;
    if (!path.nav_field(cost_msg, nav, ngoals, potential, nr, &nstarts, 16, &npaths, &ninfo)) {
      std::fprintf(stderr, "cost-to-goal field failed: %s\n", path.last_error().c_str());
      return 11;
    }
    static const uint32_t path_want[6] = {8, 17, 18, 19, 20, 13};
    if (!nr.finished || nr.goals_taken != 1 || nr.goals_ignored != 1 || nr.reached != 23 || nr.greatest != 3500 ||
        potential.size() != 24 || potential[8] != 3114 || potential[10] != RPLGPU_NAV_UNREACHED || potential[13] != 0 ||
        npaths.size() != 2 || npaths[0].size() != 6 || std::memcmp(npaths[0].data(), path_want, 24) != 0 ||
        ninfo[1] != RPLGPU_NAV_PATH_REACHED || ninfo[2] != 3114 || !npaths[1].empty() ||
        ninfo[5] != RPLGPU_NAV_PATH_UNREACHED) {
      std::fprintf(stderr, "cost-to-goal field: wrong answer (%u reached, greatest %u, %u from cell 8)\n", nr.reached,
                   nr.greatest, potential.size() == 24 ? potential[8] : 0u);
      return 12;
    }
    std::printf("cost-to-goal field: %u cells reached, %u from cell 8 over %zu cells, %u tile visit(s)\n", nr.reached,
                potential[8], npaths[0].size(), nr.tile_visits);
    // E27 over that costmap and field: from the goal cell (5, 1) heading west, candidate 0 moves a cell a step — cell 4
    // (36), cell 3 (99, below lethal 100), then the lethal cell 2: D_end is the field at cell 11, D_min at cell 12 —
    // and candidate 1 stays where D = 0 and the cost is 0.
    rplgpu_rollout_t roll;
    rplgpu_default_rollout(&roll);
    roll.lethal = 100;
    roll.unknown_value = 60;
    roll.steps = 4;
    roll.min_steps = 2;
    const double roll_start[3] = {5.0, 0.0, 3.14159265358979323846};
    const std::vector<float> roll_deltas = {1.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f}, roll_fp = {0.0f, 0.0f};
    std::vector<uint32_t> roll_out;
    std::vector<float> roll_ends;
    rplgpu_host::ScanPath::RolloutResult ro_res;
    if (!path.rollout(cost_msg, roll, roll_start, roll_deltas, false, roll_fp, &potential, roll_out, ro_res, &roll_ends)) {
      std::fprintf(stderr, "rollout failed: %s\n", path.last_error().c_str());
      return 11;
    }
    if (roll_out.size() != 16 || roll_out[0] != 2 || roll_out[1] != (RPLGPU_ROLLOUT_BLOCKED | RPLGPU_ROLLOUT_ADMISSIBLE) ||
        roll_out[2] != 135 || roll_out[3] != 99 || roll_out[4] != potential[11] || roll_out[5] != potential[12] ||
        roll_out[6] != potential[11] + 135 || roll_out[8] != 4 || roll_out[9] != RPLGPU_ROLLOUT_ADMISSIBLE ||
        roll_out[14] != 0 || ro_res.admissible != 2 || ro_res.best_index != 1 || ro_res.best_score != 0 || ro_res.ties != 1 ||
        ro_res.blocked != 1 || ro_res.cell_range != 0 || ro_res.none || roll_ends[2] != 3.0f || roll_ends[6] != 5.0f) {
      std::fprintf(stderr, "rollout: wrong answer (n %u, cost %u, D %u, best %u)\n", roll_out.empty() ? 0u : roll_out[0],
                   roll_out.empty() ? 0u : roll_out[2], roll_out.empty() ? 0u : roll_out[4], ro_res.best_index);
      return 12;
    }
    std::printf("rollout: candidate 0 blocked after %u poses (cost %u, D %u), candidate %u wins of %u admissible\n",
                roll_out[0], roll_out[2], roll_out[4], ro_res.best_index, ro_res.admissible);
    // E28 behind it: both candidates are admissible; with shift 0 and a table of two the winner (candidate 1, score 0)
    // has index 0 and candidate 0 (a score far above 1) is clamped to index 1.  The table (1, 3) gives them the
    // weights 1 and 3, so the deltas (1, 0, 1, 0) and (1, 0, 0, 0) blend into dx = 0.75.
    rplgpu_mppi_t mp;
    rplgpu_default_mppi(&mp);
    mp.steps = roll.steps;
    mp.delta_per_step = 0;
    mp.table_len = 2;
    const uint32_t roll_words[8] = {ro_res.admissible, ro_res.best_index, 0, 0, ro_res.ties, ro_res.blocked, ro_res.cell_range, 0};
    const std::vector<uint16_t> mp_table = {1, 3};
    std::vector<uint32_t> mp_weights;
    std::vector<float> mp_nominal, mp_next;
    rplgpu_host::ScanPath::MppiResult mp_res;
    if (!path.mppi_update(mp, roll_out, roll_words, roll_deltas, mp_table, nullptr, mp_weights, mp_nominal, mp_res)) {
      std::fprintf(stderr, "mppi_update failed: %s\n", path.last_error().c_str());
      return 11;
    }
    if (mp_weights.size() != 2 || mp_weights[0] != 3 || mp_weights[1] != 1 || mp_res.weighted != 2 || mp_res.clamped != 1 ||
        mp_res.sum_w != 4 || mp_res.sum_w2 != 10 || mp_res.no_weight || mp_res.empty_step || mp_nominal.size() != 4 ||
        mp_nominal[0] != 1.0f || mp_nominal[1] != 0.0f || mp_nominal[2] != 0.75f || mp_nominal[3] != 0.0f) {
      std::fprintf(stderr, "mppi_update: wrong answer (weights %u %u, dx %g)\n", mp_weights.empty() ? 0u : mp_weights[0],
                   mp_weights.size() < 2 ? 0u : mp_weights[1], mp_nominal.size() < 3 ? 0.0 : (double)mp_nominal[2]);
      return 12;
    }
    if (!path.mppi_spread(mp_nominal, roll_deltas, 2, 0, true, mp_next) || mp_next.size() != 8 || mp_next[2] != 0.75f ||
        mp_next[6] != 0.75f) {
      std::fprintf(stderr, "mppi_spread: wrong answer: %s\n", path.last_error().c_str());
      return 12;
    }
    std::printf("mppi: weights %u and %u, the blended step moves %g, spread around it %g and %g\n", mp_weights[0],
                mp_weights[1], (double)mp_nominal[2], (double)mp_next[2], (double)mp_next[6]);
    // E29 over that costmap with the field of E26 above (its goal standing in for the robot): the door against the
    // library's own host twin, word for word, and the goal it picks is a frontier cell of the labels.
    rplgpu_frontiers_t fro;
    rplgpu_default_frontiers(&fro);
    fro.width = cost_msg.info.width;
    fro.height = cost_msg.info.height;
    fro.min_size = 1;
    rplgpu_host::ScanPath::FrontierResult fres;
    std::vector<rplgpu_host::ScanPath::FrontierRow> frows;
    std::vector<uint32_t> flabels;
    if (!path.frontiers(cost_msg, fro, &potential, 64, 4, fres, &frows, &flabels)) {
      std::fprintf(stderr, "frontiers failed: %s\n", path.last_error().c_str());
      return 11;
    }
    {
      std::vector<int8_t> bytes(cost_msg.data.begin(), cost_msg.data.end());
      uint32_t twin[RPLGPU_FRONTIER_WORDS], twin_goal = 0, twin_n = 0;
      std::vector<uint32_t> twin_labels(bytes.size()), twin_rows(32);
      if (rplgpu_frontiers_host(&fro, bytes.data(), potential.data(), 64, twin_labels.data(), twin_rows.data(), 4,
                                &twin_goal, &twin_n, twin) != RPLGPU_OK ||
          twin[1] != fres.frontier_cells || twin[2] != fres.components || twin[3] != fres.kept ||
          twin[5] != fres.best.label || twin[8] != fres.best.nearest_cell || (twin_n != 0) != fres.has_goal ||
          (twin_n && twin_goal != fres.goal_cell) || twin_labels != flabels || frows.size() != twin[14] ||
          (fres.has_goal && flabels[fres.goal_cell] != fres.best.label)) {
        std::fprintf(stderr, "frontiers: wrong answer (%u cells, %u components, %u kept)\n", fres.frontier_cells,
                     fres.components, fres.kept);
        return 12;
      }
    }
    std::printf("frontiers: %u cells in %u component(s), %u kept, the goal %s cell %u\n", fres.frontier_cells,
                fres.components, fres.kept, fres.has_goal ? "is" : "would be", fres.goal_cell);
    // E14: the three rays of the E11 leg added twice into a count map.  Per call the row of the sensor gets
    // misses 3 3 2 2 1 1 (the whole ray beyond obstacle_max leaves its end cell 4 alone, the cut one counts its
    // end cell 5) and one hit in cell 2; after two calls the default rule (2 observations, 10 %) gives the E11 row.
    std::vector<uint32_t> counts;
    uint32_t ustatus = 99;
    for (int call = 0; call < 2; ++call) {
      if (!path.update_map(step, rplgpu_host::ScanConfig(), og, nullptr, nullptr, nullptr, counts, &ustatus)) {
        std::fprintf(stderr, "map update failed: %s\n", path.last_error().c_str());
        return 13;
      }
    }
    static const uint32_t row_want[16] = {6, 0, 6, 0, 4, 2, 4, 0, 2, 0, 2, 0, 0, 0, 0, 0};
    rplgpu_map_rule_t rule;
    rplgpu_default_map_rule(&rule);
    OccupancyGrid map_msg;
    uint32_t mcells[4] = {9, 9, 9, 9};
    if (!path.fill_map_grid(counts, og, rule, map_msg, mcells)) {
      std::fprintf(stderr, "map grid failed: %s\n", path.last_error().c_str());
      return 14;
    }
    if (counts.size() != 48 || std::memcmp(&counts[16], row_want, 64) != 0 || ustatus != 0 ||
        map_msg.data.size() != 24 || std::memcmp(map_msg.data.data(), want, 24) != 0 || mcells[0] != 18 ||
        mcells[1] != 5 || mcells[2] != 1 || mcells[3] != 0 || rplgpu_map_rule_check(&rule) != RPLGPU_OK) {
      std::fprintf(stderr, "map update / map grid: wrong answer\n");
      return 15;
    }
    std::printf("map: 2 x 3 rays, cells -1/0/100/other = %u/%u/%u/%u\n", mcells[0], mcells[1], mcells[2], mcells[3]);
    // E15 against the E12 costmap, whose row of the sensor is 36 99 100 99 36 0 -1 -1: the three returns at 2, 4 and
    // 7 m on an identity mount.  At the base pose (0, 0, 0) they lie in cells 2, 4 and 7: 100 + 36 + 0 (unknown);
    // one metre back in cells 1, 3, 6: 99 + 99 + 0; two metres back in cells 0, 2, 5: 36 + 100 + 0; turned by pi they
    // leave the grid.  Best 198 at pose 1, alone; one pose weighs nothing; the sum is 470.
    const std::vector<double> xyt = {0.0, 0.0, 0.0, -1.0, 0.0, 0.0, -2.0, 0.0, 0.0, 0.0, 0.0, 3.14159265358979323846};
    std::vector<uint32_t> weights;
    rplgpu_host::ScanPath::PoseResult pr;
    uint32_t pstatus = 99;
    if (!path.score_poses(step, rplgpu_host::ScanConfig(), nullptr, nullptr, nullptr, cost_msg, xyt, weights, pr,
                          &pstatus)) {
      std::fprintf(stderr, "pose score failed: %s\n", path.last_error().c_str());
      return 16;
    }
    if (weights.size() != 4 || weights[0] != 136 || weights[1] != 198 || weights[2] != 136 || weights[3] != 0 ||
        pr.best != 198 || pr.best_index != 1 || pr.ties != 1 || pr.zeros != 1 || pr.points != 3 ||
        pr.weight_of_first != 136 || pr.sum != 470 || pstatus != 0) {
      std::fprintf(stderr, "pose score: wrong answer (%u at %u, %u ties, %u zeros, %u points, sum %llu)\n", pr.best,
                   pr.best_index, pr.ties, pr.zeros, pr.points, static_cast<unsigned long long>(pr.sum));
      return 17;
    }
    std::printf("pose score: best %u at pose %u of 4, sum %llu\n", pr.best, pr.best_index,
                static_cast<unsigned long long>(pr.sum));
    // E23 on the same poses with agree_lo 99, keep 1 / 4, err 9 / 10.  The look-ups of the return at 2 m are 100, 99,
    // 36, 0 at the four poses, of the one at 4 m 36, 99, 100, 0: two poses agree with each, 2 * 4 > 1 * 4 keeps them.
    // The return at 7 m agrees nowhere (unknown cells, a free one) and is skipped; 1 of 3 is no fallback.  It added
    // nothing, so the weights are E15's.  The door against the library's host-only twin over the same three points.
    rplgpu_beam_agree_t arule;
    rplgpu_default_beam_agree(&arule);
    arule.agree_lo = 99;
    arule.keep_num = 1;
    arule.keep_den = 4;
    std::vector<uint32_t> aweights, acounts, amask;
    rplgpu_host::ScanPath::PoseResult apr;
    rplgpu_host::ScanPath::AgreeResult ar;
    uint32_t astatus = 99;
    if (!path.score_poses_agree(step, rplgpu_host::ScanConfig(), nullptr, nullptr, nullptr, cost_msg, arule, xyt,
                                aweights, apr, acounts, amask, ar, &astatus)) {
      std::fprintf(stderr, "pose score (agree) failed: %s\n", path.last_error().c_str());
      return 90;
    }
    {
      rplgpu_beam_agree_t spec = arule;
      spec.origin_x = og.origin_x;
      spec.origin_y = og.origin_y;
      spec.resolution = og.resolution;
      spec.width = og.width;
      spec.height = og.height;
      const float px[3] = {2.0f, 4.0f, 7.0f}, py[3] = {0.0f, 0.0f, 0.0f};
      const uint32_t slot[3] = {0, 0, 0}, index[3] = {0, 1, 2};
      std::vector<float> list(16);
      uint32_t tc[3], tm[1], tw[4], tres[8], tagr[8], tstatus = 99;
      if (rplgpu_pose_list(xyt.data(), 4, list.data()) != RPLGPU_OK ||
          rplgpu_beam_agree_points_host(px, py, slot, index, 3, 1, 3, list.data(), 4, cost_msg.data.data(), &spec, tc,
                                        tm, tw, tres, tagr, &tstatus) != RPLGPU_OK) {
        std::fprintf(stderr, "pose score (agree): the host twin refused\n");
        return 91;
      }
      if (aweights.size() != 4 || std::memcmp(aweights.data(), tw, 16) != 0 || acounts.size() != 3 ||
          std::memcmp(acounts.data(), tc, 12) != 0 || amask.size() != 1 || amask[0] != tm[0] || astatus != tstatus ||
          ar.finite != tagr[0] || ar.kept != tagr[1] || ar.fell_back != tagr[2] || ar.entered != tagr[3] ||
          ar.count_max != tagr[4] || ar.count_min != tagr[5] || ar.count_sum != tagr[6] || apr.best != tres[0] ||
          apr.best_index != tres[1] || apr.sum != tres[6] || aweights != weights || acounts[0] != 2 ||
          acounts[1] != 2 || acounts[2] != 0 || amask[0] != 3 || ar.finite != 3 || ar.kept != 2 || ar.fell_back != 0) {
        std::fprintf(stderr, "pose score (agree): wrong answer (counts %u %u %u, mask %u, F %u K %u back %u)\n",
                     acounts.size() > 2 ? acounts[0] : 0, acounts.size() > 2 ? acounts[1] : 0,
                     acounts.size() > 2 ? acounts[2] : 0, amask.empty() ? 0 : amask[0], ar.finite, ar.kept,
                     ar.fell_back);
        return 92;
      }
    }
    std::printf("pose score (agree): %u of %u samples kept, counts %u %u %u, equal to the host twin\n", ar.kept,
                ar.finite, acounts[0], acounts[1], acounts[2]);
    // E16 on those weights (136, 198, 136, 0; S = 470), four outputs, u = 0: t = (0, 117, 235, 352) against
    // C = (136, 334, 470, 470) gives the ancestors (0, 0, 1, 2): the dead pose is gone and pose 0 is there twice.
    // The device call against the library's own host-only twin, byte for byte, with one metre ahead as the delta.
    std::vector<float> plist(16), moved, twin(16);
    if (rplgpu_pose_list(xyt.data(), 4, plist.data()) != RPLGPU_OK) return 18;
    const std::vector<float> ahead = {1.0f, 0.0f, 1.0f, 0.0f};
    std::vector<uint32_t> anc, twin_anc(4);
    uint32_t twin_words[8];
    rplgpu_host::ScanPath::ResampleResult rr;
    if (!path.resample_poses(weights, plist, 4, 0u, ahead, moved, anc, rr)) {
      std::fprintf(stderr, "resample failed: %s\n", path.last_error().c_str());
      return 18;
    }
    if (rplgpu_resample_host(weights.data(), 4, 4, 0u, plist.data(), ahead.data(), 1, twin.data(), twin_anc.data(),
                             twin_words) != RPLGPU_OK)
      return 19;
    if (anc != std::vector<uint32_t>({0, 0, 1, 2}) || anc != twin_anc ||
        std::memcmp(moved.data(), twin.data(), 64) != 0 || rr.sum != 470 || rr.alive != 3 || rr.distinct != 3 ||
        rr.all_dead || rr.sum_squares != 76196.0 || moved[2] != 1.0f || moved[10] != 0.0f || twin_words[6] != 3) {
      std::fprintf(stderr, "resample: wrong answer (ancestors %u %u %u %u, S %llu, %u alive, %u distinct)\n", anc[0],
                   anc[1], anc[2], anc[3], static_cast<unsigned long long>(rr.sum), rr.alive, rr.distinct);
      return 19;
    }
    std::printf("resample: ancestors %u %u %u %u, N_eff %.3f of 4\n", anc[0], anc[1], anc[2], anc[3], rr.n_eff);
    // E17 on the same weights and list, the open gate: W = 470 over four poses of which three are alive; the device
    // call against the library's own host-only twin, word for word, then the resampled list with every weight 1.
    rplgpu_pose_estimate_t est;
    rplgpu_default_pose_estimate(&est);
    est.gate_r2 = ~0ull;
    est.gate_dot = INT64_MIN;
    rplgpu_host::ScanPath::PoseEstimateResult er, er2;
    uint32_t est_twin[RPLGPU_ESTIMATE_WORDS];
    if (!path.estimate_pose(plist, weights, est, pr.best_index, er) ||
        !path.estimate_pose(moved, std::vector<uint32_t>(), est, 0u, er2)) {
      std::fprintf(stderr, "estimate failed: %s\n", path.last_error().c_str());
      return 20;
    }
    if (rplgpu_estimate_host(plist.data(), 4, weights.data(), &est, pr.best_index, est_twin) != RPLGPU_OK) return 21;
    if (std::memcmp(er.words, est_twin, sizeof(est_twin)) != 0 || !er.all.valid || er.all.weight != 470.0 ||
        er.all.poses != 4 || er.all.alive != 3 || er.center != pr.best_index || !er.gated.valid ||
        std::memcmp(er.words + 8, er.words + 40, 128) != 0 || !er2.all.valid || er2.all.weight != 4.0 ||
        er2.all.alive != 4) {
      std::fprintf(stderr, "estimate: wrong answer (W %.0f, %u poses, %u alive, centre %u)\n", er.all.weight,
                   er.all.poses, er.all.alive, er.center);
      return 21;
    }
    std::printf("estimate: (%.4f, %.4f) heading %.4f, R %.4f; after the move (%.4f, %.4f)\n", er.all.x, er.all.y,
                er.all.theta, er.all.resultant, er2.all.x, er2.all.y);
    // E18: one metre ahead with every alpha 0 is the delta (1, 0, 1, 0) four times — what the E16 leg above used; with
    // noise the device call against the library's own host-only twin, byte for byte, and the noisy deltas through
    // E16's one-delta-per-output path against its twin.
    const double no_noise[4] = {0.0, 0.0, 0.0, 0.0}, some_noise[4] = {0.05, 0.02, 0.04, 0.01};
    rplgpu_motion_noise_t mspec;
    rplgpu_default_motion_noise(&mspec);
    mspec.seed = 2026;
    mspec.step = 18;
    std::vector<float> quiet, noisy, noisy_twin(16), moved2, twin2(16);
    rplgpu_host::ScanPath::MotionNoiseResult noise0, noise1;
    if (!path.sample_motion(1.0, 0.0, 0.0, no_noise, mspec, 4, quiet, noise0) ||
        !path.sample_motion(1.0, 0.0, 0.1, some_noise, mspec, 4, noisy, noise1)) {
      std::fprintf(stderr, "sample motion failed: %s\n", path.last_error().c_str());
      return 22;
    }
    float odom[8];
    uint32_t motion_twin[8];
    if (rplgpu_motion_odometry(1.0, 0.0, 0.1, some_noise, odom) != RPLGPU_OK ||
        rplgpu_sample_motion_host(odom, 0, 4, &mspec, noisy_twin.data(), motion_twin) != RPLGPU_OK)
      return 23;
    bool quiet_ok = quiet.size() == 16;
    for (size_t k = 0; quiet_ok && k < 16; ++k) quiet_ok = quiet[k] == ahead[k % 4];
    if (!quiet_ok || noisy.size() != 16 || std::memcmp(noisy.data(), noisy_twin.data(), 64) != 0 ||
        noise1.nan_outputs != 0 || noise1.max_abs != motion_twin[1] || noise1.max_abs == 0 || noise1.max_abs > 262140 ||
        noise1.sum != noise0.sum || noise1.sum_squares != noise0.sum_squares || std::memcmp(noisy.data(), noisy.data() + 4, 16) == 0) {
      std::fprintf(stderr, "sample motion: wrong answer (%u NaN, max |Z| %u)\n", noise1.nan_outputs, noise1.max_abs);
      return 23;
    }
    if (!path.resample_poses(weights, plist, 4, 0u, noisy, moved2, anc, rr) ||
        rplgpu_resample_host(weights.data(), 4, 4, 0u, plist.data(), noisy.data(), 4, twin2.data(), twin_anc.data(),
                             twin_words) != RPLGPU_OK ||
        std::memcmp(moved2.data(), twin2.data(), 64) != 0 || std::memcmp(moved2.data(), moved.data(), 64) == 0) {
      std::fprintf(stderr, "sample motion -> resample: wrong answer\n");
      return 24;
    }
    std::printf("motion noise: 4 deltas, max |Z| %u, first (%.4f, %.4f, %.4f, %.4f)\n", noise1.max_abs, noisy[0], noisy[1],
                noisy[2], noisy[3]);
    // E19: 64 poses over a 16 x 8 grid whose only free cells are its top row, against the library's own host-only
    // twin byte for byte; with no free cell the poses lie anywhere and the result says so.
    rplgpu_pose_seed_t sspec;
    rplgpu_default_pose_seed(&sspec);
    sspec.origin_x = -0.4f;
    sspec.origin_y = -0.2f;
    sspec.width = 16;
    sspec.height = 8;
    std::vector<int8_t> sgrid(128, 100);
    for (int cx = 0; cx < 16; ++cx) sgrid[7 * 16 + cx] = 0;
    std::vector<float> seeded, seeded_twin(256), anywhere, table(2 * 8);
    uint32_t seed_twin[8];
    rplgpu_host::ScanPath::SeedResult sr, sr_none;
    if (!path.seed_poses(sspec, sgrid, 8, mspec, 64, seeded, sr) ||
        !path.seed_poses(sspec, std::vector<int8_t>(128, 100), 8, mspec, 64, anywhere, sr_none)) {
      std::fprintf(stderr, "seed poses failed: %s\n", path.last_error().c_str());
      return 25;
    }
    if (rplgpu_seed_headings(8, table.data()) != RPLGPU_OK ||
        rplgpu_seed_poses_host(&sspec, sgrid.data(), table.data(), 8, 0, 64, &mspec, seeded_twin.data(), nullptr,
                               seed_twin) != RPLGPU_OK)
      return 26;
    bool seed_ok = seeded.size() == 256 && std::memcmp(seeded.data(), seeded_twin.data(), 1024) == 0 &&
                   sr.free_cells == 16 && sr.free_cells == seed_twin[0] && sr.off_cell == 0 && !sr.none_free &&
                   sr.min_cell >= 112 && sr.max_cell <= 127 && sr_none.none_free && sr_none.free_cells == 128;
    for (size_t k = 0; seed_ok && k < 64; ++k)  // the top row: y in [0.15, 0.2), x inside the grid
      seed_ok = seeded[4 * k + 3] >= 0.15f && seeded[4 * k + 3] < 0.2f && seeded[4 * k + 2] >= -0.4f &&
                seeded[4 * k + 2] < 0.4f;
    if (!seed_ok) {
      std::fprintf(stderr, "seed poses: wrong answer (F %u, off-cell %u, cells %u .. %u)\n", sr.free_cells, sr.off_cell,
                   sr.min_cell, sr.max_cell);
      return 26;
    }
    std::printf("seed poses: 64 poses over %u free cells (%u .. %u), first (%.4f, %.4f, %.4f, %.4f)\n", sr.free_cells,
                sr.min_cell, sr.max_cell, seeded[0], seeded[1], seeded[2], seeded[3]);
    // E20: those 64 poses lie in the grid's top row (0.8 m x 0.05 m) at 8 headings: with 0.5 m bins from the grid's
    // corner they occupy at most 2 x 1 x 8 bins; against the library's own host-only twin byte for byte, then the
    // same list again under KEEP (nothing new) and the size KLD sampling gives the next list.
    rplgpu_pose_bins_t bspec;
    rplgpu_default_pose_bins(&bspec);
    bspec.origin_x = -0.4f;
    bspec.origin_y = -0.2f;
    bspec.nx = 2;
    bspec.ny = 1;
    std::vector<uint32_t> bmap, bmap_twin(1, 0xFFFFFFFFu), no_weights;
    uint32_t bin_twin[8];
    rplgpu_host::ScanPath::BinResult br, br_again;
    if (!path.bin_poses(bspec, seeded, no_weights, 8, bmap, br)) {
      std::fprintf(stderr, "bin poses failed: %s\n", path.last_error().c_str());
      return 27;
    }
    if (rplgpu_bin_poses_host(&bspec, seeded.data(), 64, nullptr, table.data(), 8, bmap_twin.data(), nullptr,
                              bin_twin) != RPLGPU_OK)
      return 28;
    bspec.flags = 1;  // KEEP
    std::vector<uint32_t> bmap_again = bmap;
    if (!path.bin_poses(bspec, seeded, no_weights, 8, bmap_again, br_again)) {
      std::fprintf(stderr, "bin poses (KEEP) failed: %s\n", path.last_error().c_str());
      return 27;
    }
    const bool bin_ok = bmap.size() == 1 && bmap == bmap_twin && bmap_again == bmap && br.new_bins == bin_twin[0] &&
                        br.counted == 64 && br.counted == bin_twin[1] && br.out_of_range == 0 && br.skipped == 0 &&
                        br.min_bin == bin_twin[4] && br.max_bin == bin_twin[5] && br.new_bins >= 1 &&
                        br.new_bins <= 16 && br.max_bin < 16 && !br.none_counted && br_again.new_bins == 0 &&
                        br_again.counted == 64 && rplgpu_kld_samples(2, 0.01, 3.0, 1, 1000000) == 527 &&
                        br.samples() >= 500;
    if (!bin_ok) {
      std::fprintf(stderr, "bin poses: wrong answer (K %u / %u, counted %u, map %08x / %08x, again K %u)\n",
                   br.new_bins, bin_twin[0], br.counted, bmap.empty() ? 0u : bmap[0], bmap_twin[0], br_again.new_bins);
      return 28;
    }
    std::printf("bin poses: 64 poses in %u bins (%u .. %u), map %08x, next list %u poses\n", br.new_bins, br.min_bin,
                br.max_bin, bmap[0], br.samples());
    // E21: six poses in two bins of a 6 x 1 x 4 map that do not touch — four of weight 1 in bin 0, two of weight 5 in
    // bin 4: two clusters, the heavier one (W = 10, label 4) has fewer poses and its mean is (2.25, 0.25, 0); against
    // the library's own host-only twin word for word.
    rplgpu_pose_clusters_t cspec;
    rplgpu_default_pose_clusters(&cspec);
    cspec.nx = 6;
    cspec.ny = 1;
    std::vector<float> cposes;
    for (int k = 0; k < 6; ++k) {
      const float pose[4] = {1.0f, 0.0f, k < 4 ? 0.25f : 2.25f, 0.25f};
      cposes.insert(cposes.end(), pose, pose + 4);
    }
    const std::vector<uint32_t> cweights = {1, 1, 1, 1, 5, 5}, cmap = {0x11u}, cbins = {0, 0, 0, 0, 4, 4};
    std::vector<rplgpu_host::ScanPath::Cluster> rows;
    rplgpu_host::ScanPath::ClusterResult cr;
    uint32_t cluster_twin[RPLGPU_CLUSTER_WORDS], rows_twin[8];
    if (!path.cluster_poses(cspec, cposes, cweights, 4, cmap, cbins, 2, rows, cr)) {
      std::fprintf(stderr, "cluster poses failed: %s\n", path.last_error().c_str());
      return 29;
    }
    if (rplgpu_cluster_poses_host(&cspec, cposes.data(), 6, cweights.data(), 4, cmap.data(), cbins.data(), nullptr,
                                  rows_twin, 2, cluster_twin) != RPLGPU_OK)
      return 30;
    const bool cluster_ok =
        cr.clusters == 2 && cr.occupied_bins == 2 && cr.best_label == 4 && cr.best_poses == 2 && cr.second_label == 0 &&
        cr.second_poses == 4 && cr.second_weight == 4 && cr.stray == 0 && cr.unlabelled == 0 && cr.flags == 0 &&
        cr.flags == cluster_twin[0] && cr.best_label == cluster_twin[1] && cr.clusters == cluster_twin[6] &&
        cr.best_valid && cr.whole_valid && cr.best[0] == 2.25 && cr.best[1] == 0.25 && cr.best[2] == 0.0 &&
        cr.best[7] == 10.0 && cr.whole[7] == 14.0 && rows.size() == 2 && rows[0].label == rows_twin[0] &&
        rows[0].label == 0 && rows[0].poses == 4 && rows[0].weight == 4 && rows[1].label == rows_twin[4] &&
        rows[1].label == 4 && rows[1].poses == 2 && rows[1].weight == 10;
    if (!cluster_ok) {
      std::fprintf(stderr, "cluster poses: wrong answer (N_c %u, best %u with %u poses at (%.4f, %.4f), flags %u)\n",
                   cr.clusters, cr.best_label, cr.best_poses, cr.best[0], cr.best[1], cr.flags);
      return 30;
    }
    std::printf("cluster poses: %u clusters, the heaviest (label %u, %u poses, W %.0f) at (%.4f, %.4f, %.4f)\n",
                cr.clusters, cr.best_label, cr.best_poses, cr.best[7], cr.best[0], cr.best[1], cr.best[2]);
    // E22: one pose in the middle of a 9 x 9 room of 1 m cells with a wall around it, four beams along the axes: every
    // ray hits the wall after 4 cells (D2 16).  Measured 4 m, 4.6 m, no return and a removed beam: terms table[K],
    // table[K] (floorf(0.6) = 0), table[2K] and nothing; against the library's own host-only twin word for word.
    rplgpu_range_cast_t rspec;
    rplgpu_default_range_cast(&rspec);
    rspec.origin_x = rspec.origin_y = 0.0f;
    rspec.resolution = 1.0f;
    rspec.width = rspec.height = 9;
    rspec.max_steps = 20;
    rspec.table_half = 3;
    std::vector<int8_t> room(81, 0);
    for (int k = 0; k < 9; ++k) room[k] = room[72 + k] = room[9 * k] = room[9 * k + 8] = 100;
    const std::vector<float> rposes = {1.0f, 0.0f, 4.5f, 4.5f}, rbeams = {1, 0, 0, 1, -1, 0, 0, -1};
    const std::vector<float> rscan = {4.0f, 4.6f, HUGE_VALF, std::nanf("")};
    const std::vector<uint8_t> rtable = {10, 11, 12, 13, 14, 15, 16, 99};
    std::vector<uint32_t> rwords, rweights;
    rplgpu_host::ScanPath::CastResult cres;
    uint32_t words_twin[4], weight_twin[1], result_twin[8], cast_twin[8];
    if (!path.cast_ranges(rspec, rposes, rbeams, room, rscan, 0, 1, rtable, &rwords, rweights, cres)) {
      std::fprintf(stderr, "cast ranges failed: %s\n", path.last_error().c_str());
      return 31;
    }
    if (rplgpu_cast_ranges_host(&rspec, rposes.data(), 1, rbeams.data(), 4, room.data(), rscan.data(), 4, 0, 1,
                                rtable.data(), words_twin, weight_twin, result_twin, cast_twin) != RPLGPU_OK)
      return 32;
    bool cast_ok = rwords.size() == 4 && rweights.size() == 1 && rweights[0] == 13 + 13 + 16 &&
                   rweights[0] == weight_twin[0] && cres.hit == 4 && cres.hit == cast_twin[0] && cres.unknown == 0 &&
                   cres.left == 0 && cres.none == 0 && cres.dropped == 0 && cres.max_hit_d2 == 16 && cres.steps == 16 &&
                   cres.steps == cast_twin[6] && cres.beams_used == 3 && cres.beams_used == result_twin[4] &&
                   cres.best_weight == rweights[0] && cres.best_index == 0 && cres.best_count == 1 && cres.zero_weights == 0 &&
                   cres.weight_sum == rweights[0] && rplgpu_cast_range_m(rwords.empty() ? 0u : rwords[0], 1.0f) == 4.0;
    for (size_t k = 0; cast_ok && k < 4; ++k) cast_ok = rwords[k] == 16u && rwords[k] == words_twin[k];
    if (!cast_ok) {
      std::fprintf(stderr, "cast ranges: wrong answer (weight %u / %u, hits %u, steps %llu, word %08x)\n",
                   rweights.empty() ? 0u : rweights[0], weight_twin[0], cres.hit, (unsigned long long)cres.steps,
                   rwords.empty() ? 0u : rwords[0]);
      return 32;
    }
    std::printf("cast ranges: 4 rays hit after %.1f m, weight %u from %u beams, %llu cell steps\n",
                rplgpu_cast_range_m(rwords[0], 1.0f), rweights[0], cres.beams_used, (unsigned long long)cres.steps);
    return 0;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 4;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<rplgpu_node_t> nodes(static_cast<size_t>(bytes) / 8);
  if (!nodes.empty() && std::fread(nodes.data(), 8, nodes.size(), f) != nodes.size()) return 4;
  std::fclose(f);

  rplgpu_host::ScanConfig cfg;
  cfg.is_new_protocol = std::atoi(argv[3]) != 0;
  cfg.inverted = std::atoi(argv[4]) != 0;
  cfg.scan_processing = std::atoi(argv[5]) != 0;
  cfg.cached_current_max_range = 40.0f;
  uint32_t sl_result = 0;
  if (std::atoi(argv[6])) sl_result = path.ascendScanData(nodes.data(), nodes.size());  // S1

  LaserScan msg;
  const bool published = path.fill_laser_scan(nodes, cfg, 0.125, msg);  // S3
  PointCloud2 cloud;
  const int cloud_mode = std::atoi(argv[7]);
  if (cloud_mode) {
    cfg.clip_enable = true;
    cfg.voxel_enable = cloud_mode == 2;
    if (!path.fill_point_cloud2(nodes, cfg, cloud) && !nodes.empty()) {
      std::fprintf(stderr, "cloud failed: %s\n", path.last_error().c_str());
      return 5;
    }
  }
  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  const uint32_t pub = published ? 1u : 0u, count = static_cast<uint32_t>(msg.ranges.size());
  const float meta[7] = {msg.angle_min, msg.angle_max, msg.angle_increment, msg.time_increment,
                         msg.scan_time, msg.range_min, msg.range_max};
  std::fwrite(&pub, 4, 1, o);
  std::fwrite(meta, 4, 7, o);
  std::fwrite(&count, 4, 1, o);
  std::fwrite(msg.ranges.data(), 4, count, o);
  std::fwrite(msg.intensities.data(), 4, count, o);
  std::fwrite(&sl_result, 4, 1, o);
  std::fwrite(&cloud.width, 4, 1, o);
  std::fwrite(cloud.data.data(), 1, cloud.data.size(), o);
  // the (possibly ascended) nodes, so the caller can check S1 as well
  std::fwrite(nodes.data(), 8, nodes.size(), o);
  std::fclose(o);
  return 0;
}
