// tools/dev/plan_rules_asan.cpp — the rules of the planner stages under the host sanitizers, a stand-alone program in
// four parts: E26 (csrc/rplgpu_nav_rules.cpp: the field's and the path's host twins, the default, the check, the
// default rounds, the scratch size), E27 (csrc/rplgpu_rollout_rules.cpp: the host twin, the deltas of constant
// velocities, the default, the check, the scratch size), E28 (csrc/rplgpu_mppi_rules.cpp: the two host twins, the
// softmax table, the default, the check, the scratch size) and E29 (csrc/rplgpu_frontier_rules.cpp: the host twin, the
// default, the check, the scratch size).  Every buffer is a heap block of exactly the size the header names, so a byte
// written or read beside one is reported.  Host code only; five source files, no other object, no hipcc, no device,
// nothing preloaded.  From the repository root, with C = rplidar_ros2_driver_amd/csrc (one command line):
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//           -I include -I $C $C/rplgpu_nav_rules.cpp $C/rplgpu_rollout_rules.cpp $C/rplgpu_mppi_rules.cpp
//           $C/rplgpu_frontier_rules.cpp tools/dev/plan_rules_asan.cpp -o /tmp/plan_rules_asan
//   /tmp/plan_rules_asan
//
// prints its steps, one "E2x ...: passed" line per part, and exits 0; a call refused that should have been accepted,
// or a known answer missed, makes it exit 1.  tests/test_plan_cpp.py builds the same five files without a sanitizer.
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

uint32_t rng_state;  // (every part starts from the same seed)
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

// ---- E26 ------------------------------------------------------------------------------------------------------------
rplgpu_nav_field_t nav_spec(uint32_t w, uint32_t h) {
  rplgpu_nav_field_t f;
  rplgpu_default_nav_field(&f);
  f.width = w;
  f.height = h;
  f.rounds = rplgpu_nav_field_default_rounds(w, h);
  return f;
}

void nav_part() {
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
      rplgpu_nav_field_t f = nav_spec(w, h);
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
    rplgpu_nav_field_t f = nav_spec(40, 40);
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
    rplgpu_nav_field_t f = nav_spec(3, 3);
    std::vector<int8_t> grid(9, 0);
    std::vector<uint32_t> goal = {4}, pot(9);
    need(rplgpu_nav_field_host(&f, grid.data(), goal.data(), 1, pot.data(), nullptr) == OK, "known accepted");
    need(pot[0] == 350 && pot[1] == 250 && pot[2] == 350 && pot[3] == 250 && pot[4] == 0 && pot[8] == 350, "250 and 350");
    rplgpu_nav_field_t g2 = nav_spec(2, 2);
    std::vector<int8_t> gap = {0, 100, 100, 0};
    std::vector<uint32_t> goal2 = {3}, pot2(4);
    need(rplgpu_nav_field_host(&g2, gap.data(), goal2.data(), 1, pot2.data(), nullptr) == OK &&
             pot2[0] == RPLGPU_NAV_UNREACHED && pot2[3] == 0,
         "no corner cutting");
    std::printf("known answers\n");
  }
}

// ---- E27 ------------------------------------------------------------------------------------------------------------
rplgpu_rollout_t rollout_spec(uint32_t w, uint32_t h, uint32_t T) {
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

void rollout_part() {
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
    rplgpu_rollout_t r = rollout_spec(6, 1, 5);
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
          rplgpu_rollout_t r = rollout_spec(W, H, T);
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
}

// ---- E28 ------------------------------------------------------------------------------------------------------------
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

void mppi_part() {
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
}

// ---- E29 ------------------------------------------------------------------------------------------------------------
rplgpu_frontiers_t frontier_spec(uint32_t w, uint32_t h, uint32_t min_size) {
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
  const rplgpu_frontiers_t f = frontier_spec(w, h, 1u + rnd() % 3u);
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
  const rplgpu_frontiers_t f = frontier_spec(6, 5, 2);
  need(rplgpu_frontiers_host(&f, grid.data(), pot.data(), 16, labels.data(), rows.data(), 2, goal.data(),
                             n_goal.data(), result.data()) == OK, "the answer by hand accepted");
  static const uint32_t want[16] = {0, 6, 2, 2, 0, 1, 3, 11, 1, 6, 0, 1, 0, 3, 2, 0};
  static const uint32_t want_rows[16] = {1, 3, 6, 0, 1, 0, 11, 1, 17, 3, 14, 0, 9, 0, 44, 22};
  need(std::memcmp(result.data(), want, 64) == 0 && std::memcmp(rows.data(), want_rows, 64) == 0, "the answer by hand");
  need(goal[0] == 1 && n_goal[0] == 1 && labels[8] == 1 && labels[29] == 17 && labels[0] == RPLGPU_FRONTIER_NO_LABEL,
       "its labels and goal");
}

void refusals() {
  rplgpu_frontiers_t f = frontier_spec(4, 4, 1);
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
  f = frontier_spec(4, 4, 1);
  need(rplgpu_frontiers_host(&f, grid.data(), nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, result.data()) == OK &&
       result[0] == (RPLGPU_FRONTIER_NONE | RPLGPU_FRONTIER_NO_KEPT), "no free cell");
  need(rplgpu_frontiers_scratch_words(&f, 1, 1) == 16u + 4u + 32u + 8u && rplgpu_frontiers_scratch_words(&f, 0, 1) == 0 &&
       rplgpu_frontiers_scratch_words(&f, 1, 0) == 0 && rplgpu_frontiers_scratch_words(nullptr, 1, 1) == 0, "the scratch size");
  f = frontier_spec(4096, 4096, 1);
  need(rplgpu_frontiers_scratch_words(&f, 2048, 1) != 0 && rplgpu_frontiers_scratch_words(&f, 2049, 1) == 0, "G x tiles");
}

void frontier_part() {
  hand();
  std::printf("the answer by hand\n");
  refusals();
  std::printf("the refusals, the check, the scratch size\n");
  static const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {64, 64}, {65, 65}, {131, 70}, {4096, 3}, {3, 4096}};
  for (const auto &s : shapes)
    for (int round = 0; round < 4; ++round)
      random_once(s[0], s[1], (round & 1) != 0, round < 2 ? s[0] * s[1] : 3u, round == 3 ? 0u : 5u);
  std::printf("32 random maps\n");
}

}  // namespace

int main() {
  const struct {
    const char *name;
    void (*run)();
  } parts[] = {{"E26 nav rules", nav_part},
               {"E27 rollout rules", rollout_part},
               {"E28 mppi rules", mppi_part},
               {"E29 frontier rules", frontier_part}};
  for (const auto &p : parts) {
    rng_state = 2463534242u;
    const int before = failures;
    p.run();
    std::printf("%s: %s\n", p.name, failures == before ? "passed" : "FAILED");
  }
  if (failures) {
    std::printf("%d wrong\n", failures);
    return 1;
  }
  std::printf("all parts passed\n");
  return 0;
}
