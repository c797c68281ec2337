// rplgpu_mppi_rules.cpp — the rules of E28, rolled-out candidates weighed and blended into new controls
// (include/rplgpu_msg.h), in plain C++: the default, the check, the scratch size, the softmax table and the two host
// twins, one candidate after the other ("the definition a reader can run").  No handle, no stream, no HIP header; built
// like rplgpu_rollout_rules.cpp (-ffp-contract=off: no product below fuses with a sum).  The doors that call these are
// in rplgpu_mppi_stages.hip; tools/dev/plan_rules_asan.cpp drives this file under the host sanitizers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rpl_mppi.hpp"
#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace {

float canon(float v) {
  if (v != v) {
    const uint32_t q = 0x7FC00000u;
    std::memcpy(&v, &q, 4);
  }
  return v;
}

// the header's QUANTISATION; false: not in range
bool quant(const float *d, float xy_scale, int32_t *H, int32_t *X, int32_t *Y) {
  const float one_c = 1.0f + d[0];
  const float h = d[1] / one_c;
  const float th = h * 1048576.0f, tx = d[2] * xy_scale, ty = d[3] * xy_scale;
  if (!(std::fabs(th) < 8388608.0f && std::fabs(tx) < 8388608.0f && std::fabs(ty) < 8388608.0f)) return false;
  *H = (int32_t)std::rint(th);
  *X = (int32_t)std::rint(tx);
  *Y = (int32_t)std::rint(ty);
  return true;
}

void put64(uint32_t *w, uint64_t v) {
  w[0] = (uint32_t)v;
  w[1] = (uint32_t)(v >> 32);
}

}  // namespace

extern "C" {

void rplgpu_default_mppi(rplgpu_mppi_t *m) {
  if (!m) return;
  m->xy_scale = 1024.0f;
  m->shift = 0;
  m->table_len = 1024;
  m->steps = 32;
  m->delta_per_step = 1;
}

int32_t rplgpu_mppi_check(const rplgpu_mppi_t *m) {
  if (!m) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(m->xy_scale) || !(m->xy_scale > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (m->shift > RPLGPU_MPPI_MAX_SHIFT || m->table_len == 0 || m->table_len > RPLGPU_MPPI_MAX_TABLE)
    return RPLGPU_ERR_INVALID_ARG;
  if (m->steps == 0 || m->steps > RPLGPU_ROLLOUT_MAX_STEPS || m->delta_per_step > 1u) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_mppi_scratch_words(uint32_t G, uint32_t K, uint32_t T_e) {
  rpl::MppiLayout l;
  return rpl::mppi_layout(G, K, T_e, &l) ? l.words : 0;
}

int32_t rplgpu_mppi_table(double lambda, uint32_t shift, uint32_t N, uint16_t *out) {
  if (!out || !std::isfinite(lambda) || !(lambda > 0.0) || shift > RPLGPU_MPPI_MAX_SHIFT || N == 0 ||
      N > RPLGPU_MPPI_MAX_TABLE)
    return RPLGPU_ERR_INVALID_ARG;
  const double unit = std::ldexp(1.0, (int)shift);
  for (uint32_t i = 0; i < N; ++i) out[i] = (uint16_t)std::floor(65535.0 * std::exp(-((double)i * unit) / lambda) + 0.5);
  out[0] = 65535u;
  return RPLGPU_OK;
}

int32_t rplgpu_mppi_update_host(const rplgpu_mppi_t *m, const uint32_t *out, const uint32_t rollout_result[8],
                                const float *delta, const uint16_t *table, const float *nominal, uint32_t K,
                                uint32_t *weights, uint32_t *sums, float *nominal_out, uint32_t result[8]) {
  if (rplgpu_mppi_check(m) != RPLGPU_OK || !out || !rollout_result || !delta || !table || !weights || !sums ||
      !nominal_out || !result)
    return RPLGPU_ERR_INVALID_ARG;
  if (K == 0 || K > RPLGPU_MAX_POSES || (uint64_t)K * m->steps > (1ull << 24)) return RPLGPU_ERR_INVALID_ARG;
  const uint32_t T_e = m->delta_per_step ? m->steps : 1u, N = m->table_len;
  const uint64_t best = (uint64_t)rollout_result[2] | ((uint64_t)rollout_result[3] << 32);
  const bool none = (rollout_result[7] & 1u) != 0;
  uint32_t n_weighted = 0, n_clamped = 0, n_off = 0, flags = 0;
  uint64_t sum_w = 0, sum_w2 = 0;
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t *o = out + 8u * (size_t)k;
    uint32_t w = 0;
    if ((o[1] & RPLGPU_ROLLOUT_ADMISSIBLE) && !none) {
      const uint64_t s = (uint64_t)o[6] | ((uint64_t)o[7] << 32);
      const uint64_t d = s < best ? 0ull : s - best;
      uint64_t i = d >> m->shift;
      if (i > (uint64_t)(N - 1u)) {
        i = N - 1u;
        ++n_clamped;
      }
      w = table[i];
    }
    weights[k] = w;
    n_weighted += w != 0 ? 1u : 0u;
    sum_w += w;
    sum_w2 += (uint64_t)w * w;
  }
  for (uint32_t t = 0; t < T_e; ++t) {
    int64_t W = 0, sH = 0, sX = 0, sY = 0;
    for (uint32_t k = 0; k < K; ++k) {
      const int64_t w = weights[k];
      if (w == 0) continue;
      int32_t H, X, Y;
      if (!quant(delta + 4u * ((size_t)k * T_e + t), m->xy_scale, &H, &X, &Y)) {
        ++n_off;
        continue;
      }
      W += w;
      sH += w * H;
      sX += w * X;
      sY += w * Y;
    }
    uint32_t *so = sums + 8u * (size_t)t;
    put64(so, (uint64_t)W);
    put64(so + 2, (uint64_t)sH);
    put64(so + 4, (uint64_t)sX);
    put64(so + 6, (uint64_t)sY);
    float nd[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    if (W > 0) {
      const double dW = (double)W;
      const double hb = ((double)sH / dW) * (1.0 / 1048576.0);
      const double hh = hb * hb;
      const double den = 1.0 + hh;
      const double sc = (double)m->xy_scale;
      nd[0] = (float)((1.0 - hh) / den);
      nd[1] = (float)((hb + hb) / den);
      nd[2] = (float)(((double)sX / dW) / sc);
      nd[3] = (float)(((double)sY / dW) / sc);
    } else {
      if (nominal) std::memcpy(nd, nominal + 4u * (size_t)t, 16);  // (before the store: nominal_out may be nominal)
      flags |= RPLGPU_MPPI_EMPTY_STEP;
    }
    std::memmove(nominal_out + 4u * (size_t)t, nd, 16);
  }
  flags |= (n_weighted == 0 ? RPLGPU_MPPI_NO_WEIGHT : 0u) | (n_off != 0 ? RPLGPU_MPPI_OFF_RANGE : 0u);
  const uint32_t words[8] = {n_weighted,         n_clamped, (uint32_t)sum_w, (uint32_t)(sum_w >> 32), (uint32_t)sum_w2,
                             (uint32_t)(sum_w2 >> 32), n_off,     flags};
  std::memcpy(result, words, sizeof(words));
  return RPLGPU_OK;
}

int32_t rplgpu_mppi_spread_host(const float *nominal, uint32_t T_n, const float *noise, uint32_t K, uint32_t T,
                                uint32_t shift, uint32_t keep_first, float *out) {
  if (!nominal || !noise || !out || K == 0 || K > RPLGPU_MAX_POSES || T == 0 || T > RPLGPU_ROLLOUT_MAX_STEPS ||
      T_n == 0 || T_n > RPLGPU_ROLLOUT_MAX_STEPS || (uint64_t)K * T > (1ull << 24) ||
      shift > RPLGPU_MPPI_MAX_SPREAD_SHIFT)
    return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t k = 0; k < K; ++k) {
    for (uint32_t t = 0; t < T; ++t) {
      const float *p = nominal + 4u * (size_t)std::min(t + shift, T_n - 1u);
      const size_t e = 4u * ((size_t)k * T + t);
      float o[4];
      if (keep_first && k == 0) {
        std::memcpy(o, p, 16);
      } else {
        const float c = p[0], s = p[1], x = p[2], y = p[3];
        const float dc = noise[e], ds = noise[e + 1], dx = noise[e + 2], dy = noise[e + 3];
        o[0] = canon(c * dc - s * ds);
        o[1] = canon(s * dc + c * ds);
        o[2] = canon((c * dx - s * dy) + x);
        o[3] = canon((s * dx + c * dy) + y);
      }
      std::memcpy(out + e, o, 16);
    }
  }
  return RPLGPU_OK;
}

}  // extern "C"
