// rplgpu_rollout_rules.cpp — the rules of E27, candidate motions rolled out of a pose and scored
// (include/rplgpu_msg.h), in plain C++: the default, the check, the scratch size, the deltas of constant velocities
// and the host twin, one candidate after the other ("the definition a reader can run").  No handle, no stream, no HIP
// header; built like rplgpu_nav_rules.cpp (-ffp-contract=off: no product below fuses with a sum).  The doors that
// call these are in rplgpu_rollout_stages.hip; tools/dev/plan_rules_asan.cpp drives this file under the
// host sanitizers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace {

struct Pose {
  float c, s, x, y;
};

float canon(float v) {
  if (v != v) {
    const uint32_t q = 0x7FC00000u;
    std::memcpy(&v, &q, 4);
  }
  return v;
}

// E16's MOVE
Pose moved(const Pose &p, const float *d) {
  const float dc = d[0], ds = d[1], dx = d[2], dy = d[3];
  Pose o;
  o.c = canon(p.c * dc - p.s * ds);
  o.s = canon(p.s * dc + p.c * ds);
  o.x = canon((p.c * dx - p.s * dy) + p.x);
  o.y = canon((p.s * dx + p.c * dy) + p.y);
  return o;
}

// E11's CELL; false: the position has none
bool cell_of(const rplgpu_rollout_t *r, float x, float y, int *cx, int *cy) {
  const float fu = std::floor((x - r->origin_x) / r->resolution);
  const float fv = std::floor((y - r->origin_y) / r->resolution);
  if (!(std::fabs(fu) < 1048576.0f && std::fabs(fv) < 1048576.0f)) return false;
  *cx = (int)fu;
  *cy = (int)fv;
  return true;
}

bool inside(const rplgpu_rollout_t *r, int cx, int cy) {
  return cx >= 0 && cy >= 0 && (uint32_t)cx < r->width && (uint32_t)cy < r->height;
}

}  // namespace

extern "C" {

void rplgpu_default_rollout(rplgpu_rollout_t *r) {
  if (!r) return;
  r->origin_x = -25.6f;
  r->origin_y = -25.6f;
  r->resolution = 0.05f;
  r->width = 1024;
  r->height = 1024;
  r->lethal = 99;
  r->unknown_value = 100;
  r->steps = 32;
  r->min_steps = 32;
  r->a_end = 1;
  r->a_min = 0;
  r->a_sum = 1;
  r->a_max = 0;
}

int32_t rplgpu_rollout_check(const rplgpu_rollout_t *r) {
  if (!r) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(r->origin_x) || !std::isfinite(r->origin_y) || !std::isfinite(r->resolution) ||
      !(r->resolution > 0.0f))
    return RPLGPU_ERR_INVALID_ARG;
  if (r->width == 0 || r->width > RPLGPU_MAX_OCC_DIM || r->height == 0 || r->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (r->lethal == 0 || r->lethal > 100u || r->unknown_value > 100u) return RPLGPU_ERR_INVALID_ARG;
  if (r->steps == 0 || r->steps > RPLGPU_ROLLOUT_MAX_STEPS || r->min_steps == 0 || r->min_steps > r->steps)
    return RPLGPU_ERR_INVALID_ARG;
  if (r->a_end > RPLGPU_ROLLOUT_MAX_WEIGHT || r->a_min > RPLGPU_ROLLOUT_MAX_WEIGHT ||
      r->a_sum > RPLGPU_ROLLOUT_MAX_WEIGHT || r->a_max > RPLGPU_ROLLOUT_MAX_WEIGHT)
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_rollout_scratch_words(uint32_t G, uint32_t K) {
  if (G == 0 || G > 65535u || K == 0 || K > RPLGPU_MAX_POSES) return 0;
  const uint64_t tiles = (uint64_t)((K + RPLGPU_ROLLOUT_TILE - 1u) / RPLGPU_ROLLOUT_TILE) * G;
  return tiles > RPLGPU_ROLLOUT_MAX_TILES ? 0 : 8ull * tiles;
}

int32_t rplgpu_rollout_deltas(const double *vxyw, uint32_t K, double dt, float *delta_out) {
  if (!vxyw || !delta_out || K == 0 || K > RPLGPU_MAX_POSES) return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t k = 0; k < K; ++k) {
    const double vx = vxyw[3u * (size_t)k], vy = vxyw[3u * (size_t)k + 1u], w = vxyw[3u * (size_t)k + 2u];
    const double th = w * dt;
    double dc = 1.0, ds = 0.0, dx = vx * dt, dy = vy * dt;
    if (w != 0.0) {
      dc = std::cos(th);
      ds = std::sin(th);
      if (!(std::fabs(th) < 1e-9)) {
        dx = (vx * ds - vy * (1.0 - dc)) / w;
        dy = (vx * (1.0 - dc) + vy * ds) / w;
      }
    }
    float *d = delta_out + 4u * (size_t)k;
    d[0] = (float)dc;
    d[1] = (float)ds;
    d[2] = (float)dx;
    d[3] = (float)dy;
  }
  return RPLGPU_OK;
}

int32_t rplgpu_rollout_host(const rplgpu_rollout_t *r, const float *start, const float *delta,
                            uint32_t delta_per_step, const float *footprint, uint32_t F, const int8_t *grid,
                            const uint32_t *potential, uint32_t K, uint32_t *out, float *end_poses,
                            uint32_t result[8]) {
  if (rplgpu_rollout_check(r) != RPLGPU_OK || !start || !delta || !footprint || !grid || !out || !result)
    return RPLGPU_ERR_INVALID_ARG;
  if (K == 0 || K > RPLGPU_MAX_POSES || (uint64_t)K * r->steps > (1ull << 24) || F == 0 ||
      F > RPLGPU_ROLLOUT_MAX_FOOTPRINT || delta_per_step > 1u)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t T = r->steps;
  uint32_t admissible = 0, best_k = RPLGPU_ROLLOUT_NONE, ties = 0, n_blocked = 0, n_range = 0;
  uint64_t best = ~0ull;
  for (uint32_t k = 0; k < K; ++k) {
    Pose p{start[0], start[1], start[2], start[3]};
    float end_pose[4];
    std::memcpy(end_pose, start, 16);  // (bit for bit when n = 0)
    uint32_t n = 0, flags = 0, cost_sum = 0, cost_max = 0;
    uint32_t d_end = potential ? RPLGPU_NAV_UNREACHED : 0u, d_min = d_end;
    for (uint32_t t = 1; t <= T; ++t) {
      p = moved(p, delta + 4u * (delta_per_step ? (size_t)k * T + (t - 1u) : (size_t)k));
      bool blocked = false, off_range = false;
      uint32_t m = 0;
      for (uint32_t i = 0; i < F; ++i) {
        const float fx = footprint[2u * i], fy = footprint[2u * i + 1u];
        const float rx = (p.c * fx - p.s * fy) + p.x;
        const float ry = (p.s * fx + p.c * fy) + p.y;
        int cx, cy;
        if (!cell_of(r, rx, ry, &cx, &cy)) {
          blocked = off_range = true;
          continue;
        }
        if (!inside(r, cx, cy)) {
          blocked = true;
          continue;
        }
        const int v = grid[(size_t)cy * r->width + (size_t)cx];
        const uint32_t value = v >= 0 ? (uint32_t)v : r->unknown_value;
        if (value >= r->lethal) blocked = true;
        m = std::max(m, value);
      }
      if (blocked) {
        flags |= RPLGPU_ROLLOUT_BLOCKED | (off_range ? RPLGPU_ROLLOUT_CELL_RANGE : 0u);
        break;
      }
      n = t;
      cost_sum += m;
      cost_max = std::max(cost_max, m);
      if (potential) {
        int cx, cy;
        d_end = cell_of(r, p.x, p.y, &cx, &cy) && inside(r, cx, cy) ? potential[(size_t)cy * r->width + (size_t)cx]
                                                                      : RPLGPU_NAV_UNREACHED;
        d_min = std::min(d_min, d_end);
      }
      std::memcpy(end_pose, &p, 16);
    }
    if (potential && d_end == RPLGPU_NAV_UNREACHED) flags |= RPLGPU_ROLLOUT_END_UNREACHED;
    uint64_t score = ~0ull;
    if (n >= r->min_steps && !(flags & RPLGPU_ROLLOUT_END_UNREACHED)) {
      flags |= RPLGPU_ROLLOUT_ADMISSIBLE;
      score = (uint64_t)r->a_end * d_end + (uint64_t)r->a_min * d_min + (uint64_t)r->a_sum * cost_sum +
              (uint64_t)r->a_max * cost_max;
      ++admissible;
      if (score < best) {
        best = score;
        best_k = k;
        ties = 1;
      } else if (score == best) {
        ++ties;
      }
    }
    n_blocked += (flags & RPLGPU_ROLLOUT_BLOCKED) ? 1u : 0u;
    n_range += (flags & RPLGPU_ROLLOUT_CELL_RANGE) ? 1u : 0u;
    const uint32_t words[8] = {n, flags, cost_sum, cost_max, d_end, d_min, (uint32_t)score, (uint32_t)(score >> 32)};
    std::memcpy(out + 8u * (size_t)k, words, sizeof(words));
    if (end_poses) std::memcpy(end_poses + 4u * (size_t)k, end_pose, 16);
  }
  const uint32_t words[8] = {admissible, best_k,  (uint32_t)best, (uint32_t)(best >> 32),
                             ties,       n_blocked, n_range,      admissible ? 0u : 1u};
  std::memcpy(result, words, sizeof(words));
  return RPLGPU_OK;
}

}  // extern "C"
