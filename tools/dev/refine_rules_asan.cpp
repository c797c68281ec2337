// tools/dev/refine_rules_asan.cpp — the rules of E25 (csrc/rplgpu_refine_rules.cpp: the sums' and the step's host twins,
// the covariance, the default, the check and the scratch size) under the host sanitizers, a stand-alone program:
// every buffer is a heap block of exactly the size the header names, so a byte written or read beside one is reported.
// Host code only; two source files, no other object, no hipcc, no device, no LD_PRELOAD.  From the repository root,
// with C = rplidar_ros2_driver_amd/csrc (one command line):
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_refine_rules.cpp tools/dev/refine_rules_asan.cpp -o /tmp/refine_rules_asan
//   /tmp/refine_rules_asan
//
// prints one line per part and exits 0; a call refused that should have been accepted, or a known answer missed,
// makes it exit 1.
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
float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) / 16777216.0f; }

int failures = 0;
void need(bool ok, const char *what) {
  if (ok) return;
  ++failures;
  std::printf("  WRONG: %s\n", what);
}

rplgpu_pose_refine_t small_spec(uint32_t w, uint32_t h) {
  rplgpu_pose_refine_t r;
  rplgpu_default_pose_refine(&r);
  r.origin_x = -1.0f;
  r.origin_y = -2.0f;
  r.resolution = 0.05f;
  r.width = w;
  r.height = h;
  r.min_points = 3;
  return r;
}

}  // namespace

int main() {
  // the default, the check, the scratch size
  rplgpu_pose_refine_t d;
  rplgpu_default_pose_refine(&d);
  rplgpu_default_pose_refine(nullptr);
  need(rplgpu_pose_refine_check(&d) == OK && rplgpu_pose_refine_check(nullptr) == REFUSED, "default / NULL");
  rplgpu_pose_refine_t bad = d;
  bad.target = 128;
  need(rplgpu_pose_refine_check(&bad) == REFUSED, "target 128");
  bad = d;
  bad.damping = std::numeric_limits<float>::quiet_NaN();
  need(rplgpu_pose_refine_check(&bad) == REFUSED, "damping NaN");
  need(rplgpu_refine_scratch_words(3, 5) == 870 && rplgpu_refine_scratch_words(0, 5) == 0 &&
           rplgpu_refine_scratch_words(65535, RPLGPU_MAX_POSES) == 58ull * 65535ull * RPLGPU_MAX_POSES,
       "scratch words");
  std::printf("spec: default, check and scratch size\n");

  // the sums over grids of odd sizes: points inside, on every border, far outside, NaN and Inf, poses that scale
  for (uint32_t w : {1u, 5u, 64u, 67u}) {
    const uint32_t h = w == 64u ? 3u : w + 2u, n = 500, P = 7;
    const rplgpu_pose_refine_t r = small_spec(w, h);
    std::vector<int8_t> field((size_t)w * h);
    for (auto &b : field) b = (int8_t)(rnd() & 0xFF);
    std::vector<float> x(n), y(n), poses(4u * P);
    for (uint32_t i = 0; i < n; ++i) {
      x[i] = uniform(-1.5f, -0.5f + 0.05f * w);
      y[i] = uniform(-2.5f, -1.5f + 0.05f * h);
    }
    x[3] = std::numeric_limits<float>::quiet_NaN();
    y[4] = std::numeric_limits<float>::infinity();
    x[5] = 3.0e38f;
    const float list[7][4] = {{1, 0, 0, 0},       {0.8f, 0.6f, 0.1f, -0.1f}, {0, 0, -1.0f, -2.0f}, {1, 0, 1.0e7f, 0},
                              {9000, 0, 0, 0},    {1, 0, std::numeric_limits<float>::quiet_NaN(), 0},
                              {-1, 0, -2.0f + 0.05f * w, -4.0f + 0.05f * h}};
    std::memcpy(poses.data(), list, sizeof(list));
    std::vector<uint32_t> sums(32u * P, 0xA5A5A5A5u);
    uint32_t result[8], status = 99;
    need(rplgpu_refine_sums_host(x.data(), y.data(), n, poses.data(), P, field.data(), &r, sums.data(), result,
                                 &status) == OK, "sums accepted");
    need(result[7] == n - 2 && status == RPLGPU_SCAN_CELL_RANGE, "finite points and status");
    for (uint32_t q = 0; q < P; ++q) {
      const uint32_t *s = &sums[32u * q];
      need(s[27] + s[28] == n - 2 && s[29] == 0 && s[30] == 0 && s[31] == 0, "n + dropped = finite points");
      std::vector<float> out(4);
      std::vector<uint32_t> step(4);
      const int32_t flags = rplgpu_refine_step_host(s, &r, &poses[4u * q], out.data(), step.data());
      need(flags > 0 && (uint32_t)flags == step[3], "step flags");
      std::vector<double> cov(9);
      (void)rplgpu_refine_covariance(s, &r, cov.data());
    }
    need(rplgpu_refine_sums_host(x.data(), y.data(), n, poses.data(), 0, field.data(), &r, sums.data(), result,
                                 &status) == REFUSED, "P = 0 refused");
    need(rplgpu_refine_sums_host(nullptr, nullptr, 0, poses.data(), P, field.data(), &r, sums.data(), nullptr,
                                 nullptr) == OK && sums[27] == 0, "no points");
    std::printf("sums, step and covariance: %u x %u cells, %u points, %u poses\n", w, h, n, P);
  }

  // a known answer: the centre of cell (2, 1) of a 5 x 5 grid of 1 m cells
  {
    rplgpu_pose_refine_t r = small_spec(5, 5);
    r.origin_x = r.origin_y = 0.0f;
    r.resolution = 1.0f;
    r.target = 100;
    std::vector<int8_t> f(25);
    for (int i = 0; i < 25; ++i) f[i] = (int8_t)(10 * (i % 5 + 1) + i / 5);
    const std::vector<float> x = {2.5f}, y = {1.5f}, pose = {1, 0, 0, 0};
    std::vector<uint32_t> s(32);
    need(rplgpu_refine_sums_host(x.data(), y.data(), 1, pose.data(), 1, f.data(), &r, s.data(), nullptr, nullptr) == OK,
         "known accepted");
    need(s[10] == 31u * 65536u && s[11] == 0 && s[0] == 2560u * 2560u && s[4] == 256u * 256u && s[27] == 1,
         "known answer at a cell centre");
    std::printf("known answer\n");
  }
  if (failures) {
    std::printf("%d wrong\n", failures);
    return 1;
  }
  std::printf("all parts passed\n");
  return 0;
}
