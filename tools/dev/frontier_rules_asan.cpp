// tools/dev/frontier_rules_asan.cpp — the rules of E29 (csrc/rplgpu_frontier_rules.cpp: the host twin, the default, the
// check and the scratch size) under the host sanitizers, a stand-alone program: every buffer is a heap block of exactly
// the size the header names, so a byte written or read beside one is reported.  Host code only; two source files, no
// other object, no hipcc, no device, no LD_PRELOAD.  From the repository root, with C = rplidar_ros2_driver_amd/csrc
// (one command line):
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_frontier_rules.cpp tools/dev/frontier_rules_asan.cpp -o /tmp/frontier_rules_asan
//   /tmp/frontier_rules_asan
//
// prints one line per part and exits 0; a call refused that should have been accepted, or a known answer missed,
// makes it exit 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace {

const int32_t OK = RPLGPU_OK, REFUSED = RPLGPU_ERR_INVALID_ARG;

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

int failures = 0;
void need(bool ok, const char *what) {
  if (ok) return;
  ++failures;
  std::printf("  WRONG: %s\n", what);
}

rplgpu_frontiers_t spec_of(uint32_t w, uint32_t h, uint32_t min_size) {
  rplgpu_frontiers_t f;
  rplgpu_default_frontiers(&f);
  f.width = w;
  f.height = h;
  f.min_size = min_size;
  return f;
}

// one random map over exact-size blocks; what holds for every answer is checked
void random_once(uint32_t w, uint32_t h, bool with_potential, uint32_t comp_cap, uint32_t row_cap) {
  const size_t cells = (size_t)w * h;
  const rplgpu_frontiers_t f = spec_of(w, h, 1u + rnd() % 3u);
  static const int8_t kinds[8] = {-128, -1, -1, 0, 0, 98, 99, 127};
  std::vector<int8_t> grid(cells);
  std::vector<uint32_t> pot(with_potential ? cells : 0), labels(cells), rows(8u * (size_t)row_cap), result(16);
  for (size_t c = 0; c < cells; ++c) grid[c] = kinds[rnd() & 7u];
  for (size_t c = 0; c < pot.size(); ++c) pot[c] = (rnd() & 15u) ? rnd() % 50u : RPLGPU_NAV_UNREACHED;
  std::vector<uint32_t> goal(1, 77u), n_goal(1, 77u);
  need(rplgpu_frontiers_host(&f, grid.data(), with_potential ? pot.data() : nullptr, comp_cap, labels.data(),
                             row_cap ? rows.data() : nullptr, row_cap, goal.data(), n_goal.data(),
                             result.data()) == OK, "a random map accepted");
  uint32_t frontier = 0, roots = 0;
  for (size_t c = 0; c < cells; ++c) {
    if (labels[c] == RPLGPU_FRONTIER_NO_LABEL) continue;
    ++frontier;
    need(labels[c] <= c && labels[labels[c]] == labels[c], "a label is the component's least cell");
    roots += labels[c] == c;
  }
  need(result[1] == frontier && result[2] == roots, "F and N count the labels");
  const bool bound = roots > comp_cap;
  need(((result[0] & RPLGPU_FRONTIER_BOUND) != 0) == bound, "the bound flag");
  need(n_goal[0] == ((result[0] & RPLGPU_FRONTIER_NO_KEPT) ? 0u : 1u), "the goal count follows the flags");
  if (n_goal[0]) need(goal[0] == result[8] && labels[goal[0]] == result[5], "the goal is BEST's cell");
  else need(goal[0] == 77u, "no BEST: the goal word untouched");
  if (!bound) need(result[3] + 0u <= roots && result[14] == (result[3] < row_cap ? result[3] : row_cap), "the rows");
  for (uint32_t r = 0; r + 1 < result[14]; ++r) need(rows[8u * r] < rows[8u * (r + 1u)], "rows ascend by label");
}

void hand() {
  // the 6 x 5 answer of tests/test_frontier_cpu.py
  static const char *text[5] = {"..?.#.", "....#.", "....#.", "###..?", "..#..."};
  std::vector<int8_t> grid(30);
  std::vector<uint32_t> pot(30), labels(30), rows(16), result(16), goal(1), n_goal(1);
  for (int y = 0; y < 5; ++y)
    for (int x = 0; x < 6; ++x) {
      grid[6 * y + x] = text[y][x] == '.' ? 0 : text[y][x] == '?' ? -1 : 100;
      pot[6 * y + x] = 10u * x + y + 1u;
    }
  const rplgpu_frontiers_t f = spec_of(6, 5, 2);
  need(rplgpu_frontiers_host(&f, grid.data(), pot.data(), 16, labels.data(), rows.data(), 2, goal.data(),
                             n_goal.data(), result.data()) == OK, "the answer by hand accepted");
  static const uint32_t want[16] = {0, 6, 2, 2, 0, 1, 3, 11, 1, 6, 0, 1, 0, 3, 2, 0};
  static const uint32_t want_rows[16] = {1, 3, 6, 0, 1, 0, 11, 1, 17, 3, 14, 0, 9, 0, 44, 22};
  need(std::memcmp(result.data(), want, 64) == 0 && std::memcmp(rows.data(), want_rows, 64) == 0, "the answer by hand");
  need(goal[0] == 1 && n_goal[0] == 1 && labels[8] == 1 && labels[29] == 17 && labels[0] == RPLGPU_FRONTIER_NO_LABEL,
       "its labels and goal");
}

void refusals() {
  rplgpu_frontiers_t f = spec_of(4, 4, 1);
  std::vector<int8_t> grid(16, -1);
  std::vector<uint32_t> result(16, 5u), one(1, 5u);
  need(rplgpu_frontiers_check(nullptr) == REFUSED && rplgpu_frontiers_check(&f) == OK, "the check");
  rplgpu_default_frontiers(nullptr);
  need(rplgpu_frontiers_host(nullptr, grid.data(), nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, result.data()) == REFUSED, "no spec");
  need(rplgpu_frontiers_host(&f, nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, result.data()) == REFUSED, "no grid");
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == REFUSED, "no result");
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, result.data()) == REFUSED, "comp_cap 0");
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, RPLGPU_FRONTIER_MAX_COMPS + 1u, nullptr, nullptr, 0, nullptr, nullptr, result.data()) == REFUSED, "comp_cap above");
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, 1, nullptr, nullptr, 1, nullptr, nullptr, result.data()) == REFUSED, "row_cap without rows");
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, 1, nullptr, nullptr, 0, one.data(), nullptr, result.data()) == REFUSED, "a goal without its count");
  f.lethal = 101;
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, result.data()) == REFUSED, "lethal 101");
  need(result[0] == 5u && one[0] == 5u, "a refused call writes nothing");
  f = spec_of(4, 4, 1);
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, result.data()) == OK &&
       result[0] == (RPLGPU_FRONTIER_NONE | RPLGPU_FRONTIER_NO_KEPT), "no free cell");
  need(rplgpu_frontiers_scratch_words(&f, 1, 1) == 16u + 4u + 32u + 8u && rplgpu_frontiers_scratch_words(&f, 0, 1) == 0 &&
       rplgpu_frontiers_scratch_words(&f, 1, 0) == 0 && rplgpu_frontiers_scratch_words(nullptr, 1, 1) == 0, "the scratch size");
  f = spec_of(4096, 4096, 1);
  need(rplgpu_frontiers_scratch_words(&f, 2048, 1) != 0 && rplgpu_frontiers_scratch_words(&f, 2049, 1) == 0, "G x tiles");
}

}  // namespace

int main() {
  hand();
  std::printf("the answer by hand\n");
  refusals();
  std::printf("the refusals, the check, the scratch size\n");
  static const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {64, 64}, {65, 65}, {131, 70}, {4096, 3}, {3, 4096}};
  for (const auto &s : shapes)
    for (int round = 0; round < 4; ++round)
      random_once(s[0], s[1], (round & 1) != 0, round < 2 ? s[0] * s[1] : 3u, round == 3 ? 0u : 5u);
  std::printf("32 random maps\n");
  if (failures) std::printf("%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
