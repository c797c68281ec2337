// tools/dev/pose_rules_asan.cpp — the rules of the pose-list stages (csrc/rplgpu_pose_rules.cpp: the eight host twins,
// every rplgpu_default_* / rplgpu_*_check and the small tables) under the host sanitizers, a stand-alone program: every
// buffer is a heap block of exactly the size the header names, so a word written or read beside one is reported.  Host
// code only; two source files, no other object, no hipcc, no device, no LD_PRELOAD.  From the repository root, with
// C = rplidar_ros2_driver_amd/csrc (one command line):
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_pose_rules.cpp tools/dev/pose_rules_asan.cpp -o /tmp/pose_rules_asan
//   /tmp/pose_rules_asan
//
// prints one line per twin and exits 0; a call refused that should have been accepted, or a result word that
// contradicts another, makes it exit 1.  tests/test_host_cpp.py builds the same two files with g++ and no sanitizer
// to keep the rules unit plain C++.  (rplgpu_cast_beams is not here: it lives with the doors, see DESIGN.md.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace {

const int32_t OK = RPLGPU_OK, REFUSED = RPLGPU_ERR_INVALID_ARG;
const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}
float unit() { return (float)(rnd() >> 8) / 16777216.0f; }

// exact-size heap blocks, freed together
struct Heap {
  std::vector<void *> all;
  template <class T>
  T *get(size_t n) {
    void *p = std::malloc(n ? n * sizeof(T) : 1);
    all.push_back(p);
    return static_cast<T *>(p);
  }
  ~Heap() {
    for (void *p : all) std::free(p);
  }
};

int failures = 0;
void need(bool ok, const char *what) {
  if (ok) return;
  ++failures;
  std::printf("  WRONG: %s\n", what);
}

struct Grid {
  uint32_t W, H;
};
const Grid kGrids[2] = {{3, 2}, {33, 5}};
const uint32_t kCounts[3] = {1, 2, 65};
const float kRes = 0.25f, kOx = -1.0f, kOy = -0.5f;

// P poses (c, s, x, y) over the grid and a little beyond it; with `odd`, entries the rules define without a cell
float *make_poses(Heap &heap, uint32_t P, Grid g, bool odd) {
  float *poses = heap.get<float>(4u * (size_t)P);
  for (uint32_t q = 0; q < P; ++q) {
    const float th = unit() * 6.2831853f;
    poses[4u * q] = std::cos(th);
    poses[4u * q + 1u] = std::sin(th);
    poses[4u * q + 2u] = kOx + (unit() * 1.2f - 0.1f) * kRes * (float)g.W;
    poses[4u * q + 3u] = kOy + (unit() * 1.2f - 0.1f) * kRes * (float)g.H;
  }
  if (odd && P > 2) {
    poses[2] = kNaN;
    poses[4u * 1u + 3u] = -kInf;
    poses[4u * 2u] = 1.0e30f;
  }
  return poses;
}

int8_t *make_grid(Heap &heap, Grid g, int kind) {  // 0: free, occupied and unknown cells; 1: no free cell
  int8_t *grid = heap.get<int8_t>((size_t)g.W * g.H);
  const int8_t values[4] = {0, 0, 100, -1};
  for (size_t c = 0; c < (size_t)g.W * g.H; ++c) grid[c] = kind ? (int8_t)100 : values[rnd() & 3u];
  if (!kind) grid[rnd() % (g.W * g.H)] = 0;  // (at least one free cell)
  return grid;
}

void specs_and_tables() {
  rplgpu_pose_score_t ps;
  rplgpu_pose_estimate_t pe;
  rplgpu_motion_noise_t mn;
  rplgpu_pose_seed_t sd;
  rplgpu_pose_bins_t pb;
  rplgpu_pose_clusters_t pc;
  rplgpu_range_cast_t rc;
  rplgpu_beam_agree_t ba;
  rplgpu_default_pose_score(&ps);
  rplgpu_default_pose_estimate(&pe);
  rplgpu_default_motion_noise(&mn);
  rplgpu_default_pose_seed(&sd);
  rplgpu_default_pose_bins(&pb);
  rplgpu_default_pose_clusters(&pc);
  rplgpu_default_range_cast(&rc);
  rplgpu_default_beam_agree(&ba);
  rplgpu_default_pose_score(nullptr);
  rplgpu_default_beam_agree(nullptr);
  need(rplgpu_pose_score_check(&ps) == OK && rplgpu_pose_estimate_check(&pe) == OK && rplgpu_pose_seed_check(&sd) == OK &&
           rplgpu_pose_bins_check(&pb, 36) == OK && rplgpu_pose_clusters_check(&pc, 36) == OK &&
           rplgpu_range_cast_check(&rc) == OK && rplgpu_beam_agree_check(&ba) == OK,
       "a default spec is refused");
  need(rplgpu_pose_score_check(nullptr) == REFUSED && rplgpu_pose_estimate_check(nullptr) == REFUSED &&
           rplgpu_pose_seed_check(nullptr) == REFUSED && rplgpu_pose_bins_check(nullptr, 1) == REFUSED &&
           rplgpu_pose_clusters_check(nullptr, 1) == REFUSED && rplgpu_range_cast_check(nullptr) == REFUSED &&
           rplgpu_beam_agree_check(nullptr) == REFUSED,
       "a NULL spec is accepted");
  ps.width = 0;
  pe.xy_scale = kNaN;
  sd.free_lo = 1;
  pb.inv_size = 0.0f;
  pc.flags = 2;
  rc.hit_lo = 0;
  ba.keep_den = 0;
  need(rplgpu_pose_score_check(&ps) == REFUSED && rplgpu_pose_estimate_check(&pe) == REFUSED &&
           rplgpu_pose_seed_check(&sd) == REFUSED && rplgpu_pose_bins_check(&pb, 1) == REFUSED &&
           rplgpu_pose_clusters_check(&pc, 1) == REFUSED && rplgpu_range_cast_check(&rc) == REFUSED &&
           rplgpu_beam_agree_check(&ba) == REFUSED && rplgpu_pose_clusters_check(&pc, 0) == REFUSED,
       "a broken spec is accepted");
  need(rplgpu_bin_map_words(3, 2, 1) == 2 && rplgpu_bin_map_words(33, 5, 3) == 16 && rplgpu_bin_map_words(0, 1, 1) == 0,
       "rplgpu_bin_map_words");
  need(rplgpu_kld_samples(1, 0.05, 2.33, 100, 5000) == 5000 && rplgpu_kld_samples(2, 0.05, 2.33, 100, 5000) == 100,
       "rplgpu_kld_samples at its ends");
  need(std::isnan(rplgpu_cast_range_m(RPLGPU_CAST_DROPPED, kRes)) &&
           rplgpu_cast_range_m((uint32_t)RPLGPU_CAST_NONE << 28, kRes) == HUGE_VAL &&
           rplgpu_cast_range_m(((uint32_t)RPLGPU_CAST_HIT << 28) | 16u, kRes) == 1.0,
       "rplgpu_cast_range_m");
  Heap heap;
  for (uint32_t n : kCounts) {
    double *xyt = heap.get<double>(3u * (size_t)n);
    float *out = heap.get<float>(4u * (size_t)n);
    for (uint32_t k = 0; k < 3u * n; ++k) xyt[k] = (double)unit() - 0.5;
    xyt[2] = 0.0;
    need(rplgpu_pose_list(xyt, n, out) == OK && out[0] == 1.0f && out[1] == 0.0f, "rplgpu_pose_list");
  }
  need(rplgpu_pose_list(nullptr, 0, nullptr) == OK && rplgpu_pose_list(nullptr, 1, nullptr) == REFUSED,
       "rplgpu_pose_list's refusals");
  uint32_t *ctr = heap.get<uint32_t>(4), *key = heap.get<uint32_t>(2), *block = heap.get<uint32_t>(4);
  std::memset(ctr, 0, 16);
  std::memset(key, 0, 8);
  need(rplgpu_philox4x32(ctr, key, block) == OK && block[0] == 0x6627e8d5u && rplgpu_philox4x32(ctr, nullptr, block) == REFUSED,
       "rplgpu_philox4x32 (Random123's known answer for zeros)");
  for (uint32_t T : {1u, 3u}) {
    float *edges = heap.get<float>(2u * (size_t)T);
    need(rplgpu_seed_headings(T, edges) == OK && rplgpu_heading_edges_check(edges, T) == OK, "heading tables");
    edges[0] = 0.0f;
    need(rplgpu_heading_edges_check(edges, T) == REFUSED, "an edge table that does not start at (1, 0)");
  }
  const double alpha[4] = {0.2, 0.2, 0.2, 0.2};
  float *odom = heap.get<float>(8);
  need(rplgpu_motion_odometry(0.25, 0.05, 0.1, alpha, odom) == OK && rplgpu_motion_odometry(0, 0, 0, nullptr, odom) == REFUSED,
       "rplgpu_motion_odometry");
  std::printf("specs and tables: defaults, checks and conversions, %s\n", failures ? "WRONG" : "ok");
}

void resample() {
  int runs = 0;
  for (uint32_t P : kCounts)
    for (uint32_t M : kCounts)
      for (int form = 0; form < 4; ++form) {  // no delta, one delta, M deltas, all weights zero
        Heap heap;
        uint32_t *weights = heap.get<uint32_t>(P), *result = heap.get<uint32_t>(8);
        uint32_t *anc = (runs & 1) ? heap.get<uint32_t>(M) : nullptr;
        const uint32_t n_delta = form == 1 ? 1u : M;
        const float *poses = make_poses(heap, P, kGrids[0], form == 2);
        const float *delta = (form == 1 || form == 2) ? make_poses(heap, n_delta, kGrids[0], false) : nullptr;
        float *out = heap.get<float>(4u * (size_t)M);
        for (uint32_t i = 0; i < P; ++i) weights[i] = form == 3 ? 0u : (rnd() & 1u) * (rnd() >> (rnd() & 31u));
        need(rplgpu_resample_host(weights, P, M, rnd(), poses, delta, n_delta, out, anc, result) == OK, "resample refused");
        need(result[7] == (result[0] == 0 && result[1] == 0 ? 1u : 0u) && result[6] >= 1 && result[6] <= (M < P ? M : P),
             "resample: the distinct count or the empty flag");
        for (uint32_t j = 0; anc && j < M; ++j) need(anc[j] < P, "resample: an ancestor beyond the list");
        need(rplgpu_resample_host(weights, P, M, 0, poses, delta, 3, out, anc, result) == (delta && M != 3 ? REFUSED : OK) &&
                 rplgpu_resample_host(weights, P, M, 0, out, nullptr, 0, out, anc, result) == REFUSED,
             "resample: a wrong n_delta or an output over its input");
        ++runs;
      }
  std::printf("resample twin: %d runs, %s\n", runs, failures ? "WRONG" : "ok");
}

void estimate() {
  int runs = 0;
  for (uint32_t P : kCounts)
    for (int form = 0; form < 4; ++form) {  // bit 0: weights, bit 1: odd poses and a centre beyond the list
      Heap heap;
      rplgpu_pose_estimate_t s;
      rplgpu_default_pose_estimate(&s);
      const float *poses = make_poses(heap, P, kGrids[1], (form & 2) != 0);
      uint32_t *weights = (form & 1) ? heap.get<uint32_t>(P) : nullptr, *result = heap.get<uint32_t>(RPLGPU_ESTIMATE_WORDS);
      for (uint32_t i = 0; weights && i < P; ++i) weights[i] = rnd() >> 8;
      need(rplgpu_estimate_host(poses, P, weights, &s, (form & 2) ? 0xFFFFFFFFu : 0u, result) == OK, "estimate refused");
      need(result[1] == ((form & 2) ? P - 1u : 0u) && result[2] <= P && result[4] <= result[2], "estimate: centre or counts");
      double *out = heap.get<double>(8);
      for (uint32_t set = 0; set < 2; ++set) {
        const bool empty = ((result[0] >> (2 + set)) & 1u) != 0;
        need(rplgpu_estimate_pose(result, s.xy_scale, set, out) == (empty ? REFUSED : OK), "estimate_pose against the W = 0 bit");
      }
      need(rplgpu_estimate_host(poses, 0, weights, &s, 0, result) == REFUSED &&
               rplgpu_estimate_pose(result, s.xy_scale, 2, out) == REFUSED,
           "estimate: P = 0 or set 2 accepted");
      ++runs;
    }
  std::printf("estimate twin: %d runs, %s\n", runs, failures ? "WRONG" : "ok");
}

void sample_motion() {
  int runs = 0;
  const double alpha[4] = {0.2, 0.2, 0.2, 0.2};
  for (uint32_t M : kCounts)
    for (int form = 0; form < 2; ++form) {  // 1: an odometry that makes NaNs, the last group
      Heap heap;
      rplgpu_motion_noise_t s;
      rplgpu_default_motion_noise(&s);
      s.seed = 0x0123456789ABCDEFull;
      s.first = 0xFFFFFFFFu;  // (the counter word wraps)
      float *odom = heap.get<float>(8), *delta = heap.get<float>(4u * (size_t)M);
      uint32_t *result = heap.get<uint32_t>(8);
      need(rplgpu_motion_odometry(0.25, 0.05, 0.1, alpha, odom) == OK, "odometry refused");
      if (form) odom[2] = kNaN;
      need(rplgpu_sample_motion_host(odom, form ? 65534u : 0u, M, &s, delta, result) == OK, "sample_motion refused");
      need(result[0] == (form ? M : 0u) && result[7] == (form ? 1u : 0u) && result[1] <= 262140u, "sample_motion: NaN count or |Z|");
      need(rplgpu_sample_motion_host(odom, 65535u, M, &s, delta, result) == REFUSED &&
               rplgpu_sample_motion_host(odom, 0, 0, &s, delta, result) == REFUSED,
           "sample_motion: group 65535 or M = 0 accepted");
      ++runs;
    }
  std::printf("sample_motion twin: %d runs, %s\n", runs, failures ? "WRONG" : "ok");
}

void seed_poses() {
  int runs = 0;
  for (Grid g : kGrids)
    for (uint32_t M : kCounts)
      for (int form = 0; form < 4; ++form) {  // bit 0: cell centres and cells_out, bit 1: no free cell
        Heap heap;
        rplgpu_pose_seed_t s;
        rplgpu_default_pose_seed(&s);
        s.origin_x = kOx;
        s.origin_y = kOy;
        s.resolution = kRes;
        s.width = g.W;
        s.height = g.H;
        s.flags = form & 1;
        rplgpu_motion_noise_t noise;
        rplgpu_default_motion_noise(&noise);
        noise.seed = rnd();
        const uint32_t H = (form & 1) ? 1u : 7u;
        const int8_t *grid = make_grid(heap, g, form >> 1);
        float *headings = heap.get<float>(2u * (size_t)H), *poses = heap.get<float>(4u * (size_t)M);
        uint32_t *cells = (form & 1) ? heap.get<uint32_t>(M) : nullptr, *result = heap.get<uint32_t>(8);
        need(rplgpu_seed_headings(H, headings) == OK, "seed_headings refused");
        need(rplgpu_seed_poses_host(&s, grid, headings, H, 3, M, &noise, poses, cells, result) == OK, "seed_poses refused");
        need((result[7] & 1u) == (uint32_t)(form >> 1) && result[3] < g.W * g.H && result[2] <= result[3] &&
                 result[0] >= 1 && result[0] <= g.W * g.H,
             "seed_poses: the free count, the cell range or the no-free-cell bit");
        for (uint32_t j = 0; cells && j < M; ++j)
          need(cells[j] < g.W * g.H && ((form >> 1) || grid[cells[j]] == 0), "seed_poses: a cell that is not free");
        need(rplgpu_seed_poses_host(&s, grid, headings, 0, 3, M, &noise, poses, cells, result) == REFUSED &&
                 rplgpu_seed_poses_host(&s, nullptr, headings, H, 3, M, &noise, poses, cells, result) == REFUSED,
             "seed_poses: H = 0 or no grid accepted");
        ++runs;
      }
  std::printf("seed_poses twin: %d runs, %s\n", runs, failures ? "WRONG" : "ok");
}

// E20 then E21 on its map and bin ids, as the stages are chained
void bins_and_clusters() {
  int runs = 0;
  for (Grid g : kGrids)
    for (uint32_t T : {1u, 3u})
      for (uint32_t P : kCounts)
        for (int form = 0; form < 4; ++form) {  // bit 0: weights and labels, bit 1: odd poses, no heading wrap
          Heap heap;
          rplgpu_pose_bins_t s;
          rplgpu_default_pose_bins(&s);
          s.origin_x = kOx;
          s.origin_y = kOy;
          s.inv_size = 1.0f / kRes;
          s.nx = g.W;
          s.ny = g.H;
          const uint32_t nb = g.W * g.H * T, words = (nb + 31u) / 32u, none = 0xFFFFFFFFu;
          need(rplgpu_bin_map_words(g.W, g.H, T) == ((words + 1u) & ~1u), "bin_map_words");
          const float *poses = make_poses(heap, P, g, (form & 2) != 0);
          float *edges = heap.get<float>(2u * (size_t)T);
          uint32_t *weights = (form & 1) ? heap.get<uint32_t>(P) : nullptr;
          uint32_t *map = heap.get<uint32_t>(words), *bins = heap.get<uint32_t>(P), *result = heap.get<uint32_t>(8);
          for (uint32_t i = 0; weights && i < P; ++i) weights[i] = (rnd() % 5u) ? rnd() >> 12 : 0u;
          need(rplgpu_seed_headings(T, edges) == OK, "seed_headings refused");
          need(rplgpu_bin_poses_host(&s, poses, P, weights, edges, T, map, nullptr, result) == OK, "bin_poses refused");
          const uint32_t K = result[0];
          s.flags = 1;  // KEEP: the same list again turns no bit on
          need(rplgpu_bin_poses_host(&s, poses, P, weights, edges, T, map, bins, result) == OK, "bin_poses (KEEP) refused");
          uint32_t set_bits = 0;
          for (uint32_t w = 0; w < words; ++w) set_bits += (uint32_t)__builtin_popcount(map[w]);
          need(result[0] == 0 && set_bits == K && result[1] + result[2] + result[3] == P && (result[7] & 4u) != 0,
               "bin_poses: K, the map's bits or the counts");
          for (uint32_t i = 0; i < P; ++i) need(bins[i] == none || bins[i] < nb, "bin_poses: a bin id beyond the map");
          need(rplgpu_bin_poses_host(&s, poses, P, weights, edges, 0, map, bins, result) == REFUSED, "bin_poses: T = 0 accepted");

          rplgpu_pose_clusters_t c;
          rplgpu_default_pose_clusters(&c);
          c.nx = g.W;
          c.ny = g.H;
          c.flags = (form & 2) ? 0u : 1u;
          uint32_t *labels = (form & 1) ? heap.get<uint32_t>(P) : nullptr, *cres = heap.get<uint32_t>(RPLGPU_CLUSTER_WORDS);
          need(rplgpu_cluster_poses_host(&c, poses, P, weights, T, map, bins, labels, nullptr, 7, cres) == OK, "cluster_poses refused");
          const uint32_t nc = cres[6];
          need(cres[7] == K && nc <= K && (nc == 0) == ((cres[0] & 1u) != 0) && cres[76] == 0 && cres[77] == P - result[1],
               "cluster_poses: the cluster count, the bin count or the unlabelled poses");
          for (uint32_t cap : {0u, nc ? nc - 1u : 0u, nc}) {  // none, one row short, all
            uint32_t *table = heap.get<uint32_t>(4u * (size_t)cap), *again = heap.get<uint32_t>(RPLGPU_CLUSTER_WORDS);
            need(rplgpu_cluster_poses_host(&c, poses, P, weights, T, map, bins, labels, table, cap, again) == OK,
                 "cluster_poses with a table refused");
            need(std::memcmp(again, cres, 4u * RPLGPU_CLUSTER_WORDS) == 0, "cluster_poses: the result depends on the table");
            for (uint32_t k = 0; k < cap; ++k) need(table[4u * k] < nb && table[4u * k + 1u] <= P, "cluster_poses: a table row");
          }
          need(rplgpu_cluster_poses_host(&c, poses, P, weights, T, nullptr, bins, labels, nullptr, 0, cres) == REFUSED,
               "cluster_poses: no map accepted");
          ++runs;
        }
  std::printf("bin_poses and cluster_poses twins: %d runs each, %s\n", runs, failures ? "WRONG" : "ok");
}

void cast_ranges() {
  int runs = 0;
  for (Grid g : kGrids)
    for (uint32_t P : kCounts)
      for (uint32_t A : {1u, 4u})
        for (int form = 0; form < 3; ++form) {  // range words alone, weights alone, both
          Heap heap;
          rplgpu_range_cast_t s;
          rplgpu_default_range_cast(&s);
          s.origin_x = kOx;
          s.origin_y = kOy;
          s.resolution = kRes;
          s.width = g.W;
          s.height = g.H;
          s.max_steps = 6;
          s.hit_lo = 50;
          s.unknown_stops = runs & 1;
          s.table_half = 2;
          const uint32_t step = 1u + (runs % 3u), first = runs & 1, count = first + (A - 1u) * step + 1u;
          const float *poses = make_poses(heap, P, g, form == 2);
          const int8_t *grid = make_grid(heap, g, 0);
          float *beams = heap.get<float>(2u * (size_t)A), *measured = form ? heap.get<float>(count) : nullptr;
          uint8_t *table = form ? heap.get<uint8_t>(2u * s.table_half + 2u) : nullptr;
          uint32_t *ranges = form != 1 ? heap.get<uint32_t>((size_t)P * A) : nullptr;
          uint32_t *weights = form ? heap.get<uint32_t>(P) : nullptr, *result = form ? heap.get<uint32_t>(8) : nullptr;
          uint32_t *cast = heap.get<uint32_t>(8);
          for (uint32_t a = 0; a < A; ++a) {
            beams[2u * a] = std::cos(1.5f * (float)a);
            beams[2u * a + 1u] = std::sin(1.5f * (float)a);
          }
          for (uint32_t k = 0; measured && k < count; ++k) measured[k] = unit() * 2.0f;
          if (measured && A > 1) {
            measured[first] = kInf;
            measured[first + step] = kNaN;
          }
          for (uint32_t k = 0; table && k < 2u * s.table_half + 2u; ++k) table[k] = (uint8_t)(rnd() & 0xFFu);
          need(rplgpu_cast_ranges_host(&s, poses, P, beams, A, grid, measured, count, first, step, table, ranges, weights,
                                       result, cast) == OK,
               "cast_ranges refused");
          need((uint64_t)cast[0] + cast[1] + cast[2] + cast[3] + cast[4] == (uint64_t)P * A, "cast_ranges: the kinds do not add up");
          if (form) {
            uint64_t sum = 0;
            for (uint32_t q = 0; q < P; ++q) sum += weights[q];
            need(sum == ((uint64_t)result[6] | (uint64_t)result[7] << 32) && result[4] == (A > 1 ? A - 1u : 1u) &&
                     result[5] == weights[0] && result[1] < P && weights[result[1]] == result[0],
                 "cast_ranges: E15's result words");
            need(rplgpu_cast_ranges_host(&s, poses, P, beams, A, grid, measured, count - 1u, first, step, table, ranges,
                                         weights, result, cast) == REFUSED,
                 "cast_ranges: a measured scan one beam short accepted");
          }
          need(rplgpu_cast_ranges_host(&s, poses, P, beams, A, grid, nullptr, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, cast) ==
                   REFUSED,
               "cast_ranges: neither output accepted");
          ++runs;
        }
  std::printf("cast_ranges twin: %d runs, %s\n", runs, failures ? "WRONG" : "ok");
}

void beam_agree(uint32_t n_scans, uint32_t n_stride, uint32_t P, Grid g, uint32_t err_num, bool odd_values, bool with_status) {
  Heap heap;
  rplgpu_beam_agree_t s;
  rplgpu_default_beam_agree(&s);
  s.origin_x = kOx;
  s.origin_y = kOy;
  s.resolution = kRes;
  s.width = g.W;
  s.height = g.H;
  s.agree_lo = 50;
  s.err_num = err_num;
  need(rplgpu_beam_agree_check(&s) == OK, "beam_agree spec refused");
  const uint32_t words = (n_stride + 31u) / 32u;
  // every second sample of every scan is a point, and always the last one of the stride
  std::vector<uint32_t> sl, ix;
  for (uint32_t b = 0; b < n_scans; ++b)
    for (uint32_t i = 0; i < n_stride; ++i)
      if ((i & 1u) == 0 || i + 1u == n_stride) {
        sl.push_back(b);
        ix.push_back(i);
      }
  const uint32_t m = (uint32_t)sl.size();
  float *x = heap.get<float>(m), *y = heap.get<float>(m), *poses = make_poses(heap, P, g, false);
  uint32_t *slot = heap.get<uint32_t>(m), *index = heap.get<uint32_t>(m);
  int8_t *field = heap.get<int8_t>((size_t)g.W * g.H);
  uint32_t *counts = heap.get<uint32_t>((size_t)n_scans * n_stride), *mask = heap.get<uint32_t>((size_t)n_scans * words);
  uint32_t *weights = heap.get<uint32_t>(P), *result = heap.get<uint32_t>(8), *agree = heap.get<uint32_t>(8);
  std::memcpy(slot, sl.data(), 4u * m);
  std::memcpy(index, ix.data(), 4u * m);
  for (uint32_t k = 0; k < m; ++k) {
    x[k] = -1.0f + unit() * (kRes * (float)g.W + 1.0f);
    y[k] = -1.0f + unit() * (kRes * (float)g.H + 1.0f);
  }
  for (size_t c = 0; c < (size_t)g.W * g.H; ++c) field[c] = (int8_t)(rnd() & 0xFFu);
  const bool odd = odd_values && m > 3 && P > 2;
  if (odd) {  // points and poses the rule defines without a cell
    x[1] = kNaN;
    y[2] = kInf;
    x[3] = 3.0e38f;
    poses[2] = kNaN;
    poses[4u * 1u + 3u] = -kInf;
    poses[4u * 2u + 2u] = 1.0e30f;
  }
  uint32_t status = 99, *st = with_status ? &status : nullptr;
  need(rplgpu_beam_agree_points_host(x, y, slot, index, m, n_scans, n_stride, poses, P, field, &s, counts, mask, weights,
                                     result, agree, st) == OK,
       "beam_agree refused");
  uint64_t total = 0;
  uint32_t bits = 0;
  for (size_t c = 0; c < (size_t)n_scans * n_stride; ++c) total += counts[c];
  for (size_t c = 0; c < (size_t)n_scans * words; ++c) bits += (uint32_t)__builtin_popcount(mask[c]);
  need(total == ((uint64_t)agree[6] | ((uint64_t)agree[7] << 32)) && bits == agree[1] && agree[0] == result[4] &&
           agree[1] <= agree[0] && agree[3] == (agree[2] ? agree[0] : agree[1]) && !(odd && with_status && status == 0),
       "beam_agree: the agree words contradict the counts, the mask or the status");
  if (err_num == 0) need(agree[0] == 0 || agree[2] == 1, "beam_agree: err_num 0 does not fall back");
  // the refusals write nothing and read nothing beside the blocks
  uint32_t far_slot = n_scans, keep = counts[0];
  need(rplgpu_beam_agree_points_host(x, y, &far_slot, index, 1, n_scans, n_stride, poses, P, field, &s, counts, mask,
                                     weights, result, agree, nullptr) == REFUSED &&
           rplgpu_beam_agree_points_host(x, y, slot, index, m, n_scans, n_stride, poses, 0, field, &s, counts, mask,
                                         weights, result, agree, nullptr) == REFUSED &&
           rplgpu_beam_agree_points_host(nullptr, nullptr, nullptr, nullptr, 0, n_scans, n_stride, poses, P, field,
                                         nullptr, counts, mask, weights, result, agree, nullptr) == REFUSED &&
           counts[0] == keep,
       "beam_agree: a slot beyond the scans, P = 0 or no spec accepted, or a refusal wrote");
  // no points at all: every output written, every word 0 but P zero weights
  need(rplgpu_beam_agree_points_host(nullptr, nullptr, nullptr, nullptr, 0, n_scans, n_stride, poses, P, field, &s,
                                     counts, mask, weights, result, agree, &status) == OK &&
           agree[0] == 0 && agree[2] == 0 && agree[5] == 0 && result[3] == P && status == 0,
       "beam_agree: the call without points");
}

}  // namespace

int main() {
  specs_and_tables();
  resample();
  estimate();
  sample_motion();
  seed_poses();
  bins_and_clusters();
  cast_ranges();
  int runs = 0;
  for (Grid g : kGrids)
    for (uint32_t n_stride : {1u, 32u, 33u})
      for (uint32_t P : kCounts)
        for (uint32_t err_num : {0u, 9u, 11u}) {
          beam_agree(1u + n_stride % 3u, n_stride, P, g, err_num, (runs & 1) != 0, (runs & 2) != 0);
          ++runs;
        }
  std::printf("beam_agree_points twin: %d runs, %s\n", runs, failures ? "WRONG" : "ok");
  std::printf("pose rules: %d failures\n", failures);
  return failures ? 1 : 0;
}
