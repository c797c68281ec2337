// tools/dev/mppi_rules_asan.cpp — the rules of E28 (csrc/rplgpu_mppi_rules.cpp: the two host twins, the softmax table,
// the default, the check and the scratch size) under the host sanitizers, a stand-alone program: every buffer is a
// heap block of exactly the size the header names, so a byte written or read beside one is reported.  Host code only;
// two source files, no other object, no hipcc, no device, no LD_PRELOAD.  From the repository root, with
// C = rplidar_ros2_driver_amd/csrc (one command line):
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_mppi_rules.cpp tools/dev/mppi_rules_asan.cpp -o /tmp/mppi_rules_asan
//   /tmp/mppi_rules_asan
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

// one update over exact-size blocks; odd: entries that are not finite, the half turn, scores at the limits
void update_once(uint32_t K, uint32_t T, uint32_t per_step, uint32_t N, uint32_t shift, bool with_nominal, bool odd,
                 bool in_place) {
  rplgpu_mppi_t m;
  rplgpu_default_mppi(&m);
  m.steps = T;
  m.delta_per_step = per_step;
  m.table_len = N;
  m.shift = shift;
  const uint32_t T_e = per_step ? T : 1u;
  std::vector<uint32_t> out(8u * (size_t)K), rres(8, 0u), weights(K), sums(8u * (size_t)T_e), result(8);
  std::vector<float> delta(4u * (size_t)K * T_e), nominal(4u * (size_t)T_e, 0.25f), nout(4u * (size_t)T_e);
  std::vector<uint16_t> table(N);
  need(rplgpu_mppi_table(50.0, shift > 20 ? 20 : shift, N, table.data()) == OK, "table");
  for (uint32_t k = 0; k < K; ++k) {
    uint32_t *o = &out[8u * (size_t)k];
    for (int i = 0; i < 8; ++i) o[i] = rnd();
    o[1] = (rnd() & 3u) ? RPLGPU_ROLLOUT_ADMISSIBLE : RPLGPU_ROLLOUT_BLOCKED;
    o[7] = odd ? (rnd() & 0x3FFFFu) : 0u;
    if (odd && k == 0) o[6] = o[7] = 0xFFFFFFFFu;
  }
  rres[2] = odd ? rnd() : 0u;
  rres[7] = K == 3 ? 1u : 0u;
  for (size_t i = 0; i < delta.size(); i += 4) {
    const float th = unit() - 0.5f;
    delta[i] = std::cos(th);
    delta[i + 1] = std::sin(th);
    delta[i + 2] = unit() - 0.3f;
    delta[i + 3] = 0.2f * unit() - 0.1f;
    if (odd && (rnd() & 7u) == 0u) delta[i + (rnd() & 3u)] = std::numeric_limits<float>::quiet_NaN();
    if (odd && (rnd() & 7u) == 0u) delta[i + 2] = std::numeric_limits<float>::infinity();
    if (odd && (rnd() & 7u) == 0u) delta[i] = -1.0f;
    if (odd && (rnd() & 7u) == 0u) delta[i + 3] = 3.0e38f;
  }
  float *no = in_place ? nominal.data() : nout.data();
  need(rplgpu_mppi_update_host(&m, out.data(), rres.data(), delta.data(), table.data(),
                               with_nominal || in_place ? nominal.data() : nullptr, K, weights.data(), sums.data(), no,
                               result.data()) == OK, "update accepted");
  uint32_t n_w = 0;
  for (uint32_t k = 0; k < K; ++k) n_w += weights[k] != 0u ? 1u : 0u;
  need(result[0] == n_w, "result word 0 counts the weights");
  need(((result[7] & RPLGPU_MPPI_NO_WEIGHT) != 0u) == (n_w == 0u), "NO_WEIGHT");
  need(((result[7] & RPLGPU_MPPI_OFF_RANGE) != 0u) == (result[6] != 0u), "OFF_RANGE");
  if (!odd) need(result[6] == 0u, "every entry in range");
}

}  // namespace

int main() {
  rplgpu_mppi_t m;
  rplgpu_default_mppi(&m);
  rplgpu_default_mppi(nullptr);
  need(rplgpu_mppi_check(&m) == OK && rplgpu_mppi_check(nullptr) == REFUSED, "default and check");
  m.shift = 50;
  need(rplgpu_mppi_check(&m) == REFUSED, "shift 50");
  need(rplgpu_mppi_scratch_words(1, 2048, 56) == 8u * 8u + 12u * 64u * 56u && rplgpu_mppi_scratch_words(0, 1, 1) == 0 &&
           rplgpu_mppi_scratch_words(1, 1, 257) == 0 && rplgpu_mppi_scratch_words(65535, 1u << 20, 1) == 0,
       "scratch words");
  std::printf("default, check, scratch size\n");

  for (uint32_t N : {1u, 2u, 777u, 65536u}) {
    std::vector<uint16_t> t(N);
    need(rplgpu_mppi_table(3.0, N > 2 ? 1 : 49, N, t.data()) == OK && t[0] == 65535u, "table entry 0");
    for (uint32_t i = 1; i < N; ++i) need(t[i] <= t[i - 1], "table monotone");
  }
  need(rplgpu_mppi_table(0.0, 0, 4, nullptr) == REFUSED, "table refusals");
  std::printf("rplgpu_mppi_table\n");

  // the answer by hand
  {
    rplgpu_default_mppi(&m);
    m.steps = 1;
    m.table_len = 2;
    std::vector<uint32_t> out(16, 0u), rres(8, 0u), w(2), sums(8), res(8);
    out[1] = out[9] = RPLGPU_ROLLOUT_ADMISSIBLE;
    out[6] = 10;
    out[14] = 11;
    rres[2] = 10;
    std::vector<float> delta = {0, 1, 1, 0, 0, -1, 2, 0}, nout(4);
    std::vector<uint16_t> table = {3, 1};
    need(rplgpu_mppi_update_host(&m, out.data(), rres.data(), delta.data(), table.data(), nullptr, 2, w.data(),
                                 sums.data(), nout.data(), res.data()) == OK, "by hand accepted");
    need(w[0] == 3 && w[1] == 1 && sums[0] == 4 && sums[2] == (1u << 21) && sums[4] == 5120 && sums[6] == 0, "sums");
    need(nout[0] == 0.6f && nout[1] == 0.8f && nout[2] == 1.25f && nout[3] == 0.0f, "new delta (0.6, 0.8, 1.25, 0)");
    std::printf("the answer by hand\n");
  }

  for (uint32_t K : {1u, 3u, 31u, 101u})
    for (uint32_t T : {1u, 2u, 33u, 256u})
      for (uint32_t per_step = 0; per_step < 2; ++per_step)
        for (uint32_t odd = 0; odd < 2; ++odd) {
          update_once(K, T, per_step, 1 + (rnd() % 300u), odd ? 30 : 0, true, odd != 0, false);
          update_once(K, T, per_step, 65536, 49, false, odd != 0, false);
          update_once(K, T, per_step, 1, 0, true, odd != 0, true);
        }
  std::printf("rplgpu_mppi_update_host: K 1 .. 101, T 1 .. 256, both delta modes, NaN / Inf / half-turn entries\n");

  for (uint32_t K : {1u, 7u, 65u})
    for (uint32_t T : {1u, 5u, 256u})
      for (uint32_t T_n : {1u, 5u, 256u})
        for (uint32_t shift : {0u, 1u, 256u})
          for (uint32_t keep = 0; keep < 2; ++keep) {
            std::vector<float> nominal(4u * (size_t)T_n), noise(4u * (size_t)K * T), out(4u * (size_t)K * T);
            for (float &v : nominal) v = unit();
            for (float &v : noise) v = (rnd() & 31u) ? unit() : std::numeric_limits<float>::quiet_NaN();
            need(rplgpu_mppi_spread_host(nominal.data(), T_n, noise.data(), K, T, shift, keep, out.data()) == OK,
                 "spread accepted");
            if (keep) need(std::memcmp(out.data(), &nominal[4u * (shift < T_n - 1u ? shift : T_n - 1u)], 16) == 0, "keep_first");
            need(rplgpu_mppi_spread_host(nominal.data(), T_n, noise.data(), K, T, shift, keep, noise.data()) == OK &&
                     std::memcmp(out.data(), noise.data(), 4u * out.size()) == 0, "spread in place");
          }
  float one[4] = {1, 0, 0, 0};
  need(rplgpu_mppi_spread_host(one, 1, one, 1, 1, 257, 0, one) == REFUSED &&
           rplgpu_mppi_spread_host(nullptr, 1, one, 1, 1, 0, 0, one) == REFUSED, "spread refusals");
  std::printf("rplgpu_mppi_spread_host\n");

  std::printf(failures ? "%d FAILURES\n" : "all parts passed\n", failures);
  return failures ? 1 : 0;
}
