// tools/dev/nav_rules_asan.cpp — the rules of E26 (csrc/rplgpu_nav_rules.cpp: the field's and the path's host twins, the
// default, the check, the default rounds and the scratch size) under the host sanitizers, a stand-alone program:
// every buffer is a heap block of exactly the size the header names, so a byte written or read beside one is reported.
// Host code only; two source files, no other object, no hipcc, no device, no LD_PRELOAD.  From the repository root,
// with C = rplidar_ros2_driver_amd/csrc (one command line):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_nav_rules.cpp tools/dev/nav_rules_asan.cpp -o /tmp/nav_rules_asan
//   /tmp/nav_rules_asan
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

rplgpu_nav_field_t spec_of(uint32_t w, uint32_t h) {
  rplgpu_nav_field_t f;
  rplgpu_default_nav_field(&f);
  f.width = w;
  f.height = h;
  f.rounds = rplgpu_nav_field_default_rounds(w, h);
  return f;
}

}  // namespace

int main() {
  // the default, the check, the rounds, the scratch size
  rplgpu_nav_field_t d;
  rplgpu_default_nav_field(&d);
  rplgpu_default_nav_field(nullptr);
  need(rplgpu_nav_field_check(&d) == OK && rplgpu_nav_field_check(nullptr) == REFUSED && d.rounds == 66, "default / NULL");
  rplgpu_nav_field_t bad = d;
  bad.lethal = 101;
  need(rplgpu_nav_field_check(&bad) == REFUSED, "lethal 101");
  bad = d;
  bad.cap = RPLGPU_NAV_MAX_CAP + 1u;
  need(rplgpu_nav_field_check(&bad) == REFUSED, "cap above the maximum");
  bad = d;
  bad.rounds = 0;
  need(rplgpu_nav_field_check(&bad) == REFUSED && rplgpu_nav_field_scratch_words(&bad, 1) == 0, "rounds 0");
  need(rplgpu_nav_field_default_rounds(1, 1) == 6 && rplgpu_nav_field_default_rounds(4096, 65) == 134 &&
           rplgpu_nav_field_default_rounds(0, 1) == 0 && rplgpu_nav_field_default_rounds(1, 4097) == 0,
       "default rounds");
  need(rplgpu_nav_field_scratch_words(&d, 3) == 2u * 256u * 3u && rplgpu_nav_field_scratch_words(&d, 0) == 0 &&
           rplgpu_nav_field_scratch_words(nullptr, 1) == 0,
       "scratch words");
  std::printf("spec: default, check, rounds and scratch size\n");

  // fields and paths over grids of odd sizes, every kind of byte, goals in and out of range, every start
  for (uint32_t w : {1u, 2u, 63u, 64u, 65u, 130u}) {
    const uint32_t h = w == 64u ? 1u : w + 3u;
    for (int variant = 0; variant < 3; ++variant) {
      rplgpu_nav_field_t f = spec_of(w, h);
      if (variant == 1) f.unknown_cost = RPLGPU_NAV_MAX_COST;
      if (variant == 2) {
        f.lethal = 100;
        f.neutral = 255;
        f.factor = 16;
        f.cap = 200000;
      }
      const size_t cells = (size_t)w * h;
      std::vector<int8_t> grid(cells);
      for (auto &b : grid) b = (rnd() % 4u) ? (int8_t)0 : (int8_t)(rnd() & 0xFF);
      std::vector<uint32_t> goals = {0u, (uint32_t)cells - 1u, (uint32_t)cells, 0xFFFFFFFFu, (uint32_t)(cells / 2u), 0u};
      std::vector<uint32_t> pot(cells, 0xA5A5A5A5u), result(8, 0xA5A5A5A5u);
      need(rplgpu_nav_field_host(&f, grid.data(), goals.data(), (uint32_t)goals.size(), pot.data(), result.data()) == OK,
           "field accepted");
      need(result[2] == 4 && result[3] == 2 && pot[0] == 0 && pot[cells - 1u] == 0 && result[4] >= 1 &&
               result[0] == 0 && result[1] == 0 && result[6] == 0 && result[7] == 0,
           "goals taken and ignored, the goals' words");
      uint32_t reached = 0;
      for (size_t c = 0; c < cells; ++c) {
        if (pot[c] != RPLGPU_NAV_UNREACHED) ++reached;
        need(pot[c] == RPLGPU_NAV_UNREACHED || pot[c] <= f.cap, "a reached word is at most cap");
      }
      need(reached == result[4], "reached cells");
      const uint32_t max_len = 2u * (w + h);
      for (uint32_t start = 0; start <= cells; start += 1u + (uint32_t)(cells / 97u)) {
        std::vector<uint32_t> path(max_len, 0xA5A5A5A5u), info(4);
        const int32_t flags = rplgpu_nav_path_host(&f, grid.data(), pot.data(), start, path.data(), max_len, info.data());
        need(flags > 0 && (uint32_t)flags == info[1] && info[0] <= max_len, "path flags");
        need((flags & RPLGPU_NAV_PATH_BROKEN) == 0, "a finished field's path is never broken");
        if (flags == (int32_t)RPLGPU_NAV_PATH_REACHED) need(pot[path[info[0] - 1u]] == 0 && path[0] == start, "path ends on a goal");
        for (uint32_t i = info[0]; i < max_len; ++i) need(path[i] == 0xA5A5A5A5u, "words beyond a path untouched");
        std::vector<uint32_t> one(1, 7u);
        (void)rplgpu_nav_path_host(&f, grid.data(), pot.data(), start, one.data(), 1, info.data());
      }
      need(rplgpu_nav_field_host(&f, grid.data(), nullptr, 0, pot.data(), nullptr) == OK && pot[0] == RPLGPU_NAV_UNREACHED,
           "no goals");
      need(rplgpu_nav_field_host(&f, grid.data(), nullptr, 1, pot.data(), nullptr) == REFUSED, "goals missing refused");
      need(rplgpu_nav_path_host(&f, grid.data(), pot.data(), 0, pot.data(), 0, result.data()) == REFUSED, "max_len 0 refused");
    }
    std::printf("field and paths: %u x %u cells, three specs\n", w, h);
  }

  // more goals than are read: a whole heap block of 1100, the last 76 ignored
  {
    rplgpu_nav_field_t f = spec_of(40, 40);
    std::vector<int8_t> grid(1600, 0);
    std::vector<uint32_t> goals(1100), pot(1600), result(8);
    for (uint32_t i = 0; i < 1100; ++i) goals[i] = i;
    need(rplgpu_nav_field_host(&f, grid.data(), goals.data(), 1100, pot.data(), result.data()) == OK && result[2] == 1024 &&
             result[3] == 76 && pot[1023] == 0 && pot[1024] != 0,
         "the first 1024 goals");
    std::printf("goals: 1100 given, 1024 read\n");
  }

  // known answers: an open 3 x 3 with the goal in the middle; a two-cell diagonal gap
  {
    rplgpu_nav_field_t f = spec_of(3, 3);
    std::vector<int8_t> grid(9, 0);
    std::vector<uint32_t> goal = {4}, pot(9);
    need(rplgpu_nav_field_host(&f, grid.data(), goal.data(), 1, pot.data(), nullptr) == OK, "known accepted");
    need(pot[0] == 350 && pot[1] == 250 && pot[2] == 350 && pot[3] == 250 && pot[4] == 0 && pot[8] == 350, "250 and 350");
    rplgpu_nav_field_t g2 = spec_of(2, 2);
    std::vector<int8_t> gap = {0, 100, 100, 0};
    std::vector<uint32_t> goal2 = {3}, pot2(4);
    need(rplgpu_nav_field_host(&g2, gap.data(), goal2.data(), 1, pot2.data(), nullptr) == OK &&
             pot2[0] == RPLGPU_NAV_UNREACHED && pot2[3] == 0,
         "no corner cutting");
    std::printf("known answers\n");
  }
  if (failures) {
    std::printf("%d wrong\n", failures);
    return 1;
  }
  std::printf("all parts passed\n");
  return 0;
}
