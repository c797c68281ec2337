// tools/dev/wide_rules_asan.cpp — the rules of E24 (csrc/rplgpu_wide_rules.cpp: the pooled field's host twin, the
// default, the check and the two size functions) under the host sanitizers, a stand-alone program: every buffer is a
// heap block of exactly the size the header names, so a byte written or read beside one is reported.  Host code only;
// two source files, no other object, no hipcc, no device, no LD_PRELOAD.  From the repository root, with
// C = rplidar_ros2_driver_amd/csrc (one command line):
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_wide_rules.cpp tools/dev/wide_rules_asan.cpp -o /tmp/wide_rules_asan
//   /tmp/wide_rules_asan
//
// prints one line per part and exits 0; a call refused that should have been accepted, or a pooled byte that is not the
// maximum the header defines, makes it exit 1.  tests/test_wide_cpu.py builds and runs the same two files.
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

// P(x, y) by the header's words: the maximum of max(byte, 0) over [x, x + s) x [y, y + s), 0 outside the grid
int8_t pooled_at(const int8_t *field, int W, int H, int x, int y) {
  const int s = (int)RPLGPU_WIDE_MATCH_BLOCK;
  int best = 0;
  for (int b = 0; b < s; ++b)
    for (int a = 0; a < s; ++a) {
      const int fx = x + a, fy = y + b;
      if (fx < 0 || fx >= W || fy < 0 || fy >= H) continue;
      if (field[(size_t)fy * W + fx] > best) best = field[(size_t)fy * W + fx];
    }
  return (int8_t)best;
}

void pool_case(uint32_t W, uint32_t H) {
  const uint32_t s = RPLGPU_WIDE_MATCH_BLOCK, Wp = W + s - 1u, Hp = H + s - 1u;
  const int8_t bytes[5] = {-128, -1, 0, 1, 127};
  int8_t *field = static_cast<int8_t *>(std::malloc((size_t)W * H));
  int8_t *pooled = static_cast<int8_t *>(std::malloc((size_t)Wp * Hp));
  for (size_t c = 0; c < (size_t)W * H; ++c) field[c] = (rnd() & 3u) ? (int8_t)(rnd() % 100u) : bytes[rnd() % 5u];
  std::memset(pooled, 0x5A, (size_t)Wp * Hp);
  need(rplgpu_pool_field_host(field, W, H, pooled) == OK, "pool accepted");
  bool same = true;
  for (uint32_t py = 0; py < Hp && same; ++py)
    for (uint32_t px = 0; px < Wp; ++px)
      if (pooled[(size_t)py * Wp + px] != pooled_at(field, (int)W, (int)H, (int)px - (int)(s - 1u), (int)py - (int)(s - 1u))) {
        same = false;
        break;
      }
  need(same, "every pooled byte is the maximum of its 8 x 8 cells");
  std::free(field);
  std::free(pooled);
  std::printf("pool %u x %u: %s\n", W, H, same ? "ok" : "WRONG");
}

}  // namespace

int main() {
  rplgpu_wide_match_t m;
  rplgpu_default_wide_match(&m);
  rplgpu_default_wide_match(nullptr);
  need(rplgpu_wide_match_check(&m) == OK, "the default spec passes");
  need(m.shift_x == 64 && m.shift_y == 64 && m.rot_steps == 10 && m.max_blocks == 1024, "the default's values");
  need(rplgpu_wide_match_blocks(&m) == 21u * 17u * 17u, "17 x 17 blocks a rotation at T 64");
  need(rplgpu_wide_match_scratch_words(&m, 3) == 3ull * (272ull + 65ull * 1024ull), "scratch words");
  need(rplgpu_wide_match_scratch_words(&m, 0) == 0, "no groups, no scratch");
  need(rplgpu_wide_match_check(nullptr) == REFUSED && rplgpu_wide_match_blocks(nullptr) == 0, "NULL refused");
  rplgpu_wide_match_t bad = m;
  bad.shift_x = RPLGPU_MAX_WIDE_SHIFT + 1u;
  need(rplgpu_wide_match_check(&bad) == REFUSED && rplgpu_wide_match_blocks(&bad) == 0 &&
           rplgpu_wide_match_scratch_words(&bad, 1) == 0, "a shift above the limit refused everywhere");
  bad = m;
  bad.max_blocks = 0;
  need(rplgpu_wide_match_check(&bad) == REFUSED, "max_blocks 0 refused");
  bad.max_blocks = RPLGPU_MAX_WIDE_BLOCKS + 1u;
  need(rplgpu_wide_match_check(&bad) == REFUSED, "max_blocks above the limit refused");
  bad = m;
  bad.resolution = std::numeric_limits<float>::quiet_NaN();
  need(rplgpu_wide_match_check(&bad) == REFUSED, "NaN refused");
  rplgpu_wide_match_t top = m;
  top.shift_x = top.shift_y = RPLGPU_MAX_WIDE_SHIFT;
  top.rot_steps = RPLGPU_MAX_MATCH_ROT;
  top.rot_step = 0.01f;
  top.max_blocks = RPLGPU_MAX_WIDE_BLOCKS;
  need(rplgpu_wide_match_check(&top) == OK && rplgpu_wide_match_blocks(&top) == 129u * 65u * 65u, "the largest window");
  std::printf("spec: %s\n", failures ? "WRONG" : "ok");
  int8_t one = 5, out[64];
  need(rplgpu_pool_field_host(nullptr, 1, 1, out) == REFUSED && rplgpu_pool_field_host(&one, 1, 1, nullptr) == REFUSED &&
           rplgpu_pool_field_host(&one, 0, 1, out) == REFUSED && rplgpu_pool_field_host(&one, 1, 4097, out) == REFUSED,
       "pool refusals");
  const uint32_t dims[][2] = {{1, 1}, {1, 9}, {9, 1}, {7, 8}, {8, 7}, {61, 40}, {64, 33}, {200, 3}, {4096, 1}, {1, 4096}};
  for (const auto &d : dims) pool_case(d[0], d[1]);
  if (failures) std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
