// tools/dev/rollout_rules_asan.cpp — the rules of E27 (csrc/rplgpu_rollout_rules.cpp: the host twin, the deltas of
// constant velocities, the default, the check and the scratch size) under the host sanitizers, a stand-alone program:
// every buffer is a heap block of exactly the size the header names, so a byte written or read beside one is reported.
// Host code only; two source files, no other object, no hipcc, no device, no LD_PRELOAD.  From the repository root,
// with C = rplidar_ros2_driver_amd/csrc (one command line):
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_rollout_rules.cpp tools/dev/rollout_rules_asan.cpp -o /tmp/rollout_rules_asan
//   /tmp/rollout_rules_asan
//
// prints one line per part and exits 0; a call refused that should have been accepted, or a known answer missed,
// makes it exit 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
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
float unit() { return (float)(rnd() >> 8) / 16777216.0f; }

int failures = 0;
void need(bool ok, const char *what) {
  if (ok) return;
  ++failures;
  std::printf("  WRONG: %s\n", what);
}

rplgpu_rollout_t spec_of(uint32_t w, uint32_t h, uint32_t T) {
  rplgpu_rollout_t r;
  rplgpu_default_rollout(&r);
  r.origin_x = 0.0f;
  r.origin_y = 0.0f;
  r.resolution = 1.0f;
  r.width = w;
  r.height = h;
  r.steps = T;
  r.min_steps = T;
  return r;
}

}  // namespace

int main() {
  // the default, the check, the scratch size
  rplgpu_rollout_t d;
  rplgpu_default_rollout(&d);
  rplgpu_default_rollout(nullptr);
  need(rplgpu_rollout_check(&d) == OK && rplgpu_rollout_check(nullptr) == REFUSED && d.steps == 32 && d.lethal == 99,
       "default / NULL");
  rplgpu_rollout_t bad = d;
  bad.min_steps = 33;
  need(rplgpu_rollout_check(&bad) == REFUSED, "min_steps above steps");
  bad = d;
  bad.resolution = std::numeric_limits<float>::quiet_NaN();
  need(rplgpu_rollout_check(&bad) == REFUSED, "resolution NaN");
  need(rplgpu_rollout_scratch_words(3, 33) == 48 && rplgpu_rollout_scratch_words(0, 1) == 0 &&
           rplgpu_rollout_scratch_words(65535, 4097) == 0,
       "scratch words");
  std::printf("check, default, scratch words: done\n");

  // by hand: three unit steps into a wall
  {
    rplgpu_rollout_t r = spec_of(6, 1, 5);
    r.min_steps = 3;
    r.a_end = 2;
    r.a_sum = 3;
    r.a_max = 7;
    std::vector<int8_t> grid = {0, 10, 20, 30, 100, 0};
    std::vector<uint32_t> pot = {500, 400, 300, 200, 100, 0};
    std::vector<float> start = {1, 0, 0.5f, 0.5f}, delta = {1, 0, 1, 0}, fp = {0, 0}, ends(4);
    std::vector<uint32_t> out(8), res(8);
    need(rplgpu_rollout_host(&r, start.data(), delta.data(), 0, fp.data(), 1, grid.data(), pot.data(), 1, out.data(),
                             ends.data(), res.data()) == OK,
         "by hand: accepted");
    need(out[0] == 3 && out[1] == (RPLGPU_ROLLOUT_BLOCKED | RPLGPU_ROLLOUT_ADMISSIBLE) && out[2] == 60 && out[3] == 30 &&
             out[4] == 200 && out[5] == 200 && out[6] == 790 && out[7] == 0 && ends[2] == 3.5f,
         "by hand: the eight words");
    need(res[0] == 1 && res[1] == 0 && res[2] == 790 && res[4] == 1 && res[5] == 1 && res[7] == 0, "by hand: the result");
    need(rplgpu_rollout_host(&r, start.data(), delta.data(), 0, fp.data(), 0, grid.data(), pot.data(), 1, out.data(),
                             ends.data(), res.data()) == REFUSED &&
             rplgpu_rollout_host(&r, start.data(), delta.data(), 2, fp.data(), 1, grid.data(), pot.data(), 1, out.data(),
                                 ends.data(), res.data()) == REFUSED &&
             rplgpu_rollout_host(&r, nullptr, delta.data(), 0, fp.data(), 1, grid.data(), pot.data(), 1, out.data(),
                                 ends.data(), res.data()) == REFUSED,
         "by hand: refusals");
  }
  std::printf("by hand: done\n");

  // random calls at the sizes' edges, buffers of exactly the sizes the header names; values that are not finite too
  const uint32_t Ks[] = {1, 31, 32, 33, 101}, Ts[] = {1, 2, 33, 256}, Fs[] = {1, 2, 64};
  uint32_t calls = 0, blocked = 0, admissible = 0;
  for (uint32_t K : Ks)
    for (uint32_t T : Ts)
      for (uint32_t F : Fs)
        for (uint32_t per_step = 0; per_step < 2; ++per_step) {
          const uint32_t W = 37, H = 19;
          rplgpu_rollout_t r = spec_of(W, H, T);
          r.min_steps = (T + 1) / 2;
          r.unknown_value = rnd() % 101u;
          r.a_min = rnd() % 65536u;
          std::vector<int8_t> grid((size_t)W * H);
          for (auto &v : grid) v = (int8_t)((int)(rnd() % 120u) - 10);
          const bool has_pot = (rnd() & 1u) != 0;
          std::vector<uint32_t> pot(has_pot ? (size_t)W * H : 0);
          for (auto &v : pot) v = (rnd() & 7u) ? rnd() % 100000u : RPLGPU_NAV_UNREACHED;
          std::vector<float> start = {1.0f, 0.0f, 5.0f + 20.0f * unit(), 3.0f + 10.0f * unit()};
          std::vector<float> delta(4u * (size_t)K * (per_step ? T : 1u)), fp(2u * (size_t)F);
          for (size_t i = 0; i < delta.size(); i += 4) {
            const float th = (unit() - 0.5f) * 0.4f;
            delta[i] = std::cos(th);
            delta[i + 1] = std::sin(th);
            delta[i + 2] = unit() * 20.0f / (float)T;
            delta[i + 3] = 0.0f;
          }
          if (K > 2) delta[6] = std::numeric_limits<float>::infinity();
          if (K > 5) delta[4u * 5u] = std::numeric_limits<float>::quiet_NaN();
          for (auto &v : fp) v = unit() - 0.5f;
          std::vector<uint32_t> out(8u * (size_t)K), res(8);
          std::vector<float> ends(4u * (size_t)K);
          need(rplgpu_rollout_host(&r, start.data(), delta.data(), per_step, fp.data(), F, grid.data(),
                                   has_pot ? pot.data() : nullptr, K, out.data(), (rnd() & 1u) ? ends.data() : nullptr,
                                   res.data()) == OK,
               "random: accepted");
          uint32_t adm = 0;
          for (uint32_t k = 0; k < K; ++k) {
            need(out[8u * k] <= T, "random: n <= T");
            adm += (out[8u * k + 1u] & RPLGPU_ROLLOUT_ADMISSIBLE) ? 1u : 0u;
          }
          need(adm == res[0] && (res[7] == 1u) == (adm == 0u), "random: the admissible count");
          ++calls;
          blocked += res[5];
          admissible += res[0];
        }
  need(blocked > 0 && admissible > 0, "random: both kinds of candidate seen");
  std::printf("random: %u calls, %u candidates blocked, %u admissible\n", calls, blocked, admissible);

  // the deltas
  {
    std::vector<double> v = {0.5, -0.25, 0.0, 1.0, 0.0, 1.5707963267948966};
    std::vector<float> out(8);
    need(rplgpu_rollout_deltas(v.data(), 2, 1.0, out.data()) == OK && out[0] == 1.0f && out[1] == 0.0f &&
             out[2] == 0.5f && out[3] == -0.25f && out[5] == 1.0f && std::fabs(out[6] - 0.63661977f) < 1e-6f,
         "deltas: w = 0 and a quarter turn");
    need(rplgpu_rollout_deltas(v.data(), 0, 1.0, out.data()) == REFUSED &&
             rplgpu_rollout_deltas(nullptr, 2, 1.0, out.data()) == REFUSED,
         "deltas: refusals");
  }
  std::printf("deltas: done\n");
  std::printf(failures ? "%d FAILURES\n" : "all parts passed\n", failures);
  return failures ? 1 : 0;
}
