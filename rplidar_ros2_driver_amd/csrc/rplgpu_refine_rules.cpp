// rplgpu_refine_rules.cpp — the rules of E25, poses refined below a cell by Gauss-Newton on the interpolated field
// (include/rplgpu_msg.h), in plain C++: the defaults, the check, the scratch size, the host twins of the sums and of
// the step that the device tests are held against, and the covariance.  No handle, no stream, no HIP header; built
// like rplgpu_pose_rules.cpp, with -ffp-contract=off: what is written as one operation here is one rounding.  The
// doors that call these are in rplgpu_refine_stages.hip; tools/dev/refine_rules_asan.cpp drives this file alone under
// the host sanitizers.
#include <cmath>
#include <cstring>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace {

typedef unsigned __int128 u128;
typedef __int128 i128;

// the nine numbers of STEP, before the damping
struct Normal {
  double a11, a12, a22, a13, a23, a33, g1, g2, g3;
};

double d64s(const uint32_t *w) { return (double)(int64_t)(((uint64_t)w[1] << 32) | w[0]); }
double d64u(const uint32_t *w) { return (double)(((uint64_t)w[1] << 32) | w[0]); }
double d96(const uint32_t *w, bool is_signed) {
  const double top = is_signed ? (double)(int32_t)w[2] : (double)w[2];
  return (top * 4294967296.0 + (double)w[1]) * 4294967296.0 + (double)w[0];
}

Normal normal_of(const uint32_t *s) {
  const double k16 = 1.0 / 65536.0, k20 = 1.0 / 1048576.0, k24 = 1.0 / 16777216.0, k28 = 1.0 / 268435456.0;
  Normal n;
  n.a11 = d64u(s + 0) * k16;
  n.a12 = d64s(s + 2) * k16;
  n.a22 = d64u(s + 4) * k16;
  n.a13 = d96(s + 12, true) * k20;
  n.a23 = d96(s + 15, true) * k20;
  n.a33 = d96(s + 18, false) * k24;
  n.g1 = d64s(s + 6) * k24;
  n.g2 = d64s(s + 8) * k24;
  n.g3 = d96(s + 21, true) * k28;
  return n;
}

struct Cofactors {
  double c11, c12, c13, c22, c23, c33, det;
};
Cofactors cofactors_of(const Normal &n) {
  Cofactors c;
  c.c11 = n.a22 * n.a33 - n.a23 * n.a23;
  c.c12 = n.a13 * n.a23 - n.a12 * n.a33;
  c.c13 = n.a12 * n.a23 - n.a13 * n.a22;
  c.c22 = n.a11 * n.a33 - n.a13 * n.a13;
  c.c23 = n.a12 * n.a13 - n.a11 * n.a23;
  c.c33 = n.a11 * n.a22 - n.a12 * n.a12;
  c.det = (n.a11 * c.c11 + n.a12 * c.c12) + n.a13 * c.c13;
  return c;
}

void put64(uint32_t *w, uint64_t v) {
  w[0] = (uint32_t)v;
  w[1] = (uint32_t)(v >> 32);
}
void put96(uint32_t *w, u128 v) {
  w[0] = (uint32_t)v;
  w[1] = (uint32_t)(v >> 32);
  w[2] = (uint32_t)(v >> 64);
}

float canonical(float v) {
  if (v != v) {
    const uint32_t qnan = 0x7FC00000u;
    std::memcpy(&v, &qnan, 4);
  }
  return v;
}

int field_at(const int8_t *field, const rplgpu_pose_refine_t *r, int ix, int iy) {
  if (ix < 0 || iy < 0 || (uint32_t)ix >= r->width || (uint32_t)iy >= r->height) return 0;
  const int v = field[(size_t)iy * r->width + (size_t)ix];
  return v > 0 ? v : 0;
}

}  // namespace

extern "C" {

void rplgpu_default_pose_refine(rplgpu_pose_refine_t *r) {
  if (!r) return;
  r->origin_x = -25.6f;
  r->origin_y = -25.6f;
  r->resolution = 0.05f;
  r->width = 1024;
  r->height = 1024;
  r->target = 127;
  r->damping = 0.0f;
  r->max_step_cells = 2.0f;
  r->max_rot = 0.1f;
  r->min_points = 16;
}

int32_t rplgpu_pose_refine_check(const rplgpu_pose_refine_t *r) {
  if (!r) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(r->origin_x) || !std::isfinite(r->origin_y) || !std::isfinite(r->resolution) ||
      !std::isfinite(r->damping) || !std::isfinite(r->max_step_cells) || !std::isfinite(r->max_rot))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(r->resolution > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (r->width == 0 || r->width > RPLGPU_MAX_OCC_DIM || r->height == 0 || r->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (r->target == 0 || r->target > 127u) return RPLGPU_ERR_INVALID_ARG;
  if (!(r->damping >= 0.0f) || !(r->max_step_cells > 0.0f) || !(r->max_rot > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (r->min_points < 3u) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_refine_scratch_words(uint32_t G, uint32_t P) {
  if (G == 0 || P == 0 || P > RPLGPU_MAX_POSES) return 0;
  return 2ull * RPLGPU_REFINE_PLANES * (uint64_t)G * P;
}

int32_t rplgpu_refine_sums_host(const float *x, const float *y, uint32_t n, const float *poses, uint32_t P,
                                const int8_t *field, const rplgpu_pose_refine_t *r, uint32_t *sums_out,
                                uint32_t result[8], uint32_t *status) {
  if (rplgpu_pose_refine_check(r) != RPLGPU_OK || !poses || !field || !sums_out || (n != 0 && (!x || !y)) ||
      P == 0 || P > RPLGPU_MAX_POSES || n > (1u << 24))
    return RPLGPU_ERR_INVALID_ARG;
  uint32_t finite = 0, st = 0, best_q = 0;
  uint64_t best_v = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (std::isfinite(x[i]) && std::isfinite(y[i])) ++finite;
  const float lim_h = 268435456.0f, lim_l = 8192.0f;
  const int64_t target = (int64_t)r->target * 65536;
  for (uint32_t q = 0; q < P; ++q) {
    const float c = poses[4u * (size_t)q], s = poses[4u * (size_t)q + 1u];
    const float tx = poses[4u * (size_t)q + 2u], ty = poses[4u * (size_t)q + 3u];
    uint64_t sxx = 0, syy = 0, sv = 0;
    int64_t sxy = 0, sxe = 0, sye = 0;
    i128 sxt = 0, syt = 0, ste = 0;
    u128 stt = 0, see = 0;
    uint32_t cnt = 0, dropped = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (!(std::isfinite(x[i]) && std::isfinite(y[i]))) continue;
      const float ax = c * x[i] - s * y[i];
      const float ay = s * x[i] + c * y[i];
      const float rx = ax + tx, ry = ay + ty;
      const float hu = ((rx - r->origin_x) / r->resolution) * 256.0f - 128.0f;
      const float hv = ((ry - r->origin_y) / r->resolution) * 256.0f - 128.0f;
      const float lx = ax / r->resolution, ly = ay / r->resolution;
      if (!(std::fabs(hu) < lim_h && std::fabs(hv) < lim_h && std::fabs(lx) < lim_l && std::fabs(ly) < lim_l)) {
        ++dropped;
        continue;
      }
      const int U = (int)std::floor(hu), V_ = (int)std::floor(hv);
      const int i0 = U >> 8, j0 = V_ >> 8, a = U & 255, b = V_ & 255;
      const int64_t Lx = (int64_t)std::rint(lx * 16.0f), Ly = (int64_t)std::rint(ly * 16.0f);
      const int m00 = field_at(field, r, i0, j0), m10 = field_at(field, r, i0 + 1, j0);
      const int m01 = field_at(field, r, i0, j0 + 1), m11 = field_at(field, r, i0 + 1, j0 + 1);
      const int64_t V = (int64_t)(256 - a) * (256 - b) * m00 + (int64_t)a * (256 - b) * m10 +
                        (int64_t)(256 - a) * b * m01 + (int64_t)a * b * m11;
      const int64_t Gx = (int64_t)(256 - b) * (m10 - m00) + (int64_t)b * (m11 - m01);
      const int64_t Gy = (int64_t)(256 - a) * (m01 - m00) + (int64_t)a * (m11 - m10);
      const int64_t Gt = Gy * Lx - Gx * Ly;
      const int64_t E = target - V;
      sxx += (uint64_t)(Gx * Gx);
      sxy += Gx * Gy;
      syy += (uint64_t)(Gy * Gy);
      sxe += Gx * E;
      sye += Gy * E;
      sv += (uint64_t)V;
      sxt += (i128)Gx * Gt;
      syt += (i128)Gy * Gt;
      stt += (u128)((i128)Gt * Gt);
      ste += (i128)Gt * E;
      see += (u128)((i128)E * E);
      ++cnt;
    }
    uint32_t *w = sums_out + 32u * (size_t)q;
    put64(w + 0, sxx);
    put64(w + 2, (uint64_t)sxy);
    put64(w + 4, syy);
    put64(w + 6, (uint64_t)sxe);
    put64(w + 8, (uint64_t)sye);
    put64(w + 10, sv);
    put96(w + 12, (u128)sxt);
    put96(w + 15, (u128)syt);
    put96(w + 18, stt);
    put96(w + 21, (u128)ste);
    put96(w + 24, see);
    w[27] = cnt;
    w[28] = dropped;
    w[29] = w[30] = w[31] = 0;
    if (dropped) st |= RPLGPU_SCAN_CELL_RANGE;
    if (sv > best_v) {
      best_v = sv;
      best_q = q;
    }
  }
  if (result) {
    result[0] = result[1] = result[2] = result[3] = 0;
    result[4] = best_q;
    result[5] = (uint32_t)best_v;
    result[6] = (uint32_t)(best_v >> 32);
    result[7] = finite;
  }
  if (status) *status = st;
  return RPLGPU_OK;
}

int32_t rplgpu_refine_step_host(const uint32_t sums[32], const rplgpu_pose_refine_t *r, const float pose[4],
                                float pose_out[4], uint32_t step[4]) {
  if (rplgpu_pose_refine_check(r) != RPLGPU_OK || !sums || !pose || !pose_out) return RPLGPU_ERR_INVALID_ARG;
  uint32_t flags = 0;
  double dx = 0.0, dy = 0.0, dt = 0.0;
  if (sums[27] < r->min_points) {
    flags = RPLGPU_REFINE_FEW;
  } else {
    Normal n = normal_of(sums);
    const double damping = (double)r->damping;
    n.a11 = n.a11 + damping * n.a11;
    n.a22 = n.a22 + damping * n.a22;
    n.a33 = n.a33 + damping * n.a33;
    const Cofactors c = cofactors_of(n);
    if (!(c.det > 0.0) || !std::isfinite(c.det)) {
      flags = RPLGPU_REFINE_SINGULAR;
    } else {
      dx = ((c.c11 * n.g1 + c.c12 * n.g2) + c.c13 * n.g3) / c.det;
      dy = ((c.c12 * n.g1 + c.c22 * n.g2) + c.c23 * n.g3) / c.det;
      dt = ((c.c13 * n.g1 + c.c23 * n.g2) + c.c33 * n.g3) / c.det;
      flags = std::isfinite(dx) && std::isfinite(dy) && std::isfinite(dt) ? RPLGPU_REFINE_STEPPED
                                                                            : RPLGPU_REFINE_SINGULAR;
    }
  }
  float out[4] = {pose[0], pose[1], pose[2], pose[3]};
  float mx = 0.0f, my = 0.0f, mt = 0.0f;
  if (flags & RPLGPU_REFINE_STEPPED) {
    const double ms = (double)r->max_step_cells, mr = (double)r->max_rot;
    if (dx > ms) { dx = ms; flags |= RPLGPU_REFINE_CLAMP_X; }
    if (dx < -ms) { dx = -ms; flags |= RPLGPU_REFINE_CLAMP_X; }
    if (dy > ms) { dy = ms; flags |= RPLGPU_REFINE_CLAMP_Y; }
    if (dy < -ms) { dy = -ms; flags |= RPLGPU_REFINE_CLAMP_Y; }
    if (dt > mr) { dt = mr; flags |= RPLGPU_REFINE_CLAMP_T; }
    if (dt < -mr) { dt = -mr; flags |= RPLGPU_REFINE_CLAMP_T; }
    const double h = 0.5 * dt;
    const double hh = h * h;
    const double den = 1.0 + hh;
    const double dc = (1.0 - hh) / den;
    const double ds = (h + h) / den;
    const float fc = (float)dc, fs = (float)ds;
    mx = (float)(dx * (double)r->resolution);
    my = (float)(dy * (double)r->resolution);
    mt = (float)dt;
    out[0] = canonical(pose[0] * fc - pose[1] * fs);
    out[1] = canonical(pose[1] * fc + pose[0] * fs);
    out[2] = canonical(pose[2] + mx);
    out[3] = canonical(pose[3] + my);
  }
  std::memcpy(pose_out, out, 16);
  if (step) {
    std::memcpy(step + 0, &mx, 4);
    std::memcpy(step + 1, &my, 4);
    std::memcpy(step + 2, &mt, 4);
    step[3] = flags;
  }
  return (int32_t)flags;
}

int32_t rplgpu_refine_covariance(const uint32_t sums[32], const rplgpu_pose_refine_t *r, double cov9[9]) {
  if (rplgpu_pose_refine_check(r) != RPLGPU_OK || !sums || !cov9) return RPLGPU_ERR_INVALID_ARG;
  const Normal n = normal_of(sums);
  const Cofactors c = cofactors_of(n);
  if (!(c.det > 0.0) || !std::isfinite(c.det)) {
    for (int k = 0; k < 9; ++k) cov9[k] = 0.0;
    return RPLGPU_ERR_INVALID_ARG;
  }
  const double res = (double)r->resolution;
  const double inv[9] = {c.c11 / c.det, c.c12 / c.det, c.c13 / c.det, c.c12 / c.det, c.c22 / c.det,
                         c.c23 / c.det, c.c13 / c.det, c.c23 / c.det, c.c33 / c.det};
  const double sc[3] = {res, res, 1.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) cov9[3 * i + j] = sc[i] * inv[3 * i + j] * sc[j];
  return RPLGPU_OK;
}

}  // extern "C"
