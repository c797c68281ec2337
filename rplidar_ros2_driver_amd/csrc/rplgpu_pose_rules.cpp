// rplgpu_pose_rules.cpp — the rules of the pose-list stages E15 - E23 (include/rplgpu_msg.h) in plain C++: every
// rplgpu_default_* and rplgpu_*_check, the small tables and conversions, and the eight host twins that the device
// tests are held against.  No handle, no stream, no HIP header: integer and float32 arithmetic whose every rounding is
// part of the contract, so this unit is built with -ffp-contract=off -fno-fast-math like every other (the twins'
// comments rely on it).  The doors that call these checks are in rplgpu_pose_stages.hip; tools/dev/pose_rules_asan.cpp
// drives this file alone under the host sanitizers.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_rules.hpp"

// ---- what more than one stage uses ----------------------------------------------------------------------------------

// the grid of E15, E19, E22 and E23: finite origin and resolution, resolution > 0, 1 .. RPLGPU_MAX_OCC_DIM cells a side
static bool grid_spec_ok(float origin_x, float origin_y, float resolution, uint32_t width, uint32_t height) {
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y) || !std::isfinite(resolution)) return false;
  if (!(resolution > 0.0f)) return false;
  return width != 0 && width <= RPLGPU_MAX_OCC_DIM && height != 0 && height <= RPLGPU_MAX_OCC_DIM;
}

// the bins of E20 and E21: nx, ny in 1 .. 65536, T in 1 .. RPLGPU_MAX_HEADING_BINS, at most RPLGPU_MAX_POSE_BINS bins
static bool bin_dims_ok(uint32_t nx, uint32_t ny, uint32_t T) {
  if (nx == 0 || nx > 65536u || ny == 0 || ny > 65536u) return false;
  if (T == 0 || T > RPLGPU_MAX_HEADING_BINS) return false;
  return (uint64_t)nx * ny * T <= (uint64_t)RPLGPU_MAX_POSE_BINS;
}

// a (c, s) pair composed with another on the right, and a vector turned by one: float32, each of the four products
// rounded, then the difference and the sum (-ffp-contract=off)
static void rotate(const float r[2], const float n[2], float a[2]) {
  const float p0 = r[0] * n[0], p1 = r[1] * n[1], p2 = r[1] * n[0], p3 = r[0] * n[1];
  a[0] = p0 - p1;
  a[1] = p2 + p3;
}

// a NaN among the four floats of a list entry is stored as 0x7FC00000; true when there was one
static bool canonical_nans(float v[4]) {
  const uint32_t qnan = 0x7FC00000u;
  bool any = false;
  for (int k = 0; k < 4; ++k) {
    if (v[k] != v[k]) {
      std::memcpy(&v[k], &qnan, 4);
      any = true;
    }
  }
  return any;
}

// E17's quantisation of (c, s), for E17, E20 and E21: one float32 product each, the range test, one
// round-to-nearest-even (the default rounding mode); q is (0, 0) for a pair out of range (es_quantise_cs of
// rpl_moments.hpp)
static bool quantise_cs(const float *cs, int32_t q[2]) {
  const float tc = cs[0] * 1048576.0f, ts = cs[1] * 1048576.0f;
  q[0] = q[1] = 0;
  if (!(std::fabs(tc) < 8388608.0f && std::fabs(ts) < 8388608.0f)) return false;
  q[0] = (int32_t)std::rint(tc);
  q[1] = (int32_t)std::rint(ts);
  return true;
}

// E15's RESULT rule on P final weights: the top weight, its first index, how many equal it, how many are zero, the
// "samples in" word, weight 0 and the 64-bit sum
static void score_result(const uint32_t *weights, uint32_t P, uint32_t samples_in, uint32_t result[8]) {
  uint32_t top = 0, at = 0, same = 0, dead = 0;
  uint64_t sum = 0;
  for (uint32_t q = 0; q < P; ++q) {
    const uint32_t w = weights[q];
    if (w > top) {
      top = w;
      at = q;
    }
    dead += w == 0u ? 1u : 0u;
    sum += w;
  }
  for (uint32_t q = 0; q < P; ++q) same += weights[q] == top ? 1u : 0u;
  const uint32_t words[8] = {top, at, same, dead, samples_in, weights[0], (uint32_t)sum, (uint32_t)(sum >> 32)};
  std::memcpy(result, words, 32);
}

extern "C" {

// ---- E15: a list of arbitrary poses weighed against a likelihood field ----------------------------------------------

void rplgpu_default_pose_score(rplgpu_pose_score_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->resolution = 0.05f;
  s->width = 1024;
  s->height = 1024;
}

int32_t rplgpu_pose_score_check(const rplgpu_pose_score_t *s) {
  if (!s || !grid_spec_ok(s->origin_x, s->origin_y, s->resolution, s->width, s->height)) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

int32_t rplgpu_pose_list(const double *xyt, uint32_t n, float *poses_out) {
  if (n > RPLGPU_MAX_POSES || (n && (!xyt || !poses_out))) return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t q = 0; q < n; ++q) {
    const double th = xyt[3u * q + 2u];
    poses_out[4u * q] = th == 0.0 ? 1.0f : (float)std::cos(th);
    poses_out[4u * q + 1u] = th == 0.0 ? 0.0f : (float)std::sin(th);  // (+0 for theta = -0 too)
    poses_out[4u * q + 2u] = (float)xyt[3u * q];
    poses_out[4u * q + 3u] = (float)xyt[3u * q + 1u];
  }
  return RPLGPU_OK;
}

// ---- E16: a weighted pose list resampled and moved ------------------------------------------------------------------

// E16's move: the delta composed on the right, the translation turned and then added; a NaN that the move makes is
// stored as 0x7FC00000
static void resample_move(const float *pose, const float *d, float *out) {
  float heading[2], shift[2];
  rotate(pose, d, heading);
  rotate(pose, d + 2, shift);
  float v[4] = {heading[0], heading[1], shift[0] + pose[2], shift[1] + pose[3]};
  canonical_nans(v);
  std::memcpy(out, v, 16);
}

int32_t rplgpu_resample_host(const uint32_t *weights, uint32_t P, uint32_t M, uint32_t u, const float *poses,
                             const float *delta, uint32_t n_delta, float *poses_out, uint32_t *ancestors_out,
                             uint32_t result[8]) {
  if (!weights || !poses || !poses_out || !result || P == 0 || P > RPLGPU_MAX_POSES || M == 0 ||
      M > RPLGPU_MAX_POSES || (delta && n_delta != 1u && n_delta != M) ||
      rpl::ranges_overlap(poses, 16ull * P, poses_out, 16ull * M))
    return RPLGPU_ERR_INVALID_ARG;
  uint64_t S = 0, sq = 0;
  uint32_t carry = 0, nz = 0;
  for (uint32_t i = 0; i < P; ++i) {
    const uint64_t w = weights[i], w2 = w * w;
    S += w;
    sq += w2;
    carry += sq < w2 ? 1u : 0u;
    nz += w != 0 ? 1u : 0u;
  }
  const uint64_t q = S / M, rho = S % M;
  const uint64_t r = (uint64_t)u * (S >> 32) + (((uint64_t)u * (S & 0xffffffffull)) >> 32);
  uint32_t i = 0, distinct = 0, last = 0xFFFFFFFFu;
  uint64_t C = weights[0];  // C[i], inclusive
  for (uint32_t j = 0; j < M; ++j) {
    uint32_t a;
    if (S == 0) {
      a = j % P;
    } else {
      const uint64_t t = (uint64_t)j * q + ((uint64_t)j * rho + r) / M;  // < S: the walk ends inside the list
      while (C <= t) C += weights[++i];
      a = i;
    }
    if (a != last) ++distinct;  // (a is non-decreasing)
    last = a;
    if (delta)
      resample_move(poses + 4u * (size_t)a, delta + (n_delta == 1u ? 0u : 4u * (size_t)j), poses_out + 4u * (size_t)j);
    else
      std::memcpy(poses_out + 4u * (size_t)j, poses + 4u * (size_t)a, 16);
    if (ancestors_out) ancestors_out[j] = a;
  }
  result[0] = (uint32_t)S;
  result[1] = (uint32_t)(S >> 32);
  result[2] = (uint32_t)sq;
  result[3] = (uint32_t)(sq >> 32);
  result[4] = carry;
  result[5] = nz;
  result[6] = S == 0 ? std::min(M, P) : distinct;
  result[7] = S == 0 ? 1u : 0u;
  return RPLGPU_OK;
}

// ---- E17: a weighted pose list reduced to a pose estimate -----------------------------------------------------------

void rplgpu_default_pose_estimate(rplgpu_pose_estimate_t *s) {
  if (!s) return;
  s->xy_scale = 1024.0f;
  s->gate_r2 = 512ull * 512ull;
  s->gate_dot = 15ll << 36;
}

int32_t rplgpu_pose_estimate_check(const rplgpu_pose_estimate_t *s) {
  if (!s || !std::isfinite(s->xy_scale) || !(s->xy_scale > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

// E17's quantisation of one pose entry to X, Y, C, S: x and y by quantise_cs's rule at xy_scale, (c, s) by quantise_cs
static bool estimate_quantise(const float *pose, float xy_scale, int32_t q[4]) {
  const float tx = pose[2] * xy_scale, ty = pose[3] * xy_scale;
  if (!(std::fabs(tx) < 8388608.0f && std::fabs(ty) < 8388608.0f) || !quantise_cs(pose, q + 2)) return false;
  q[0] = (int32_t)std::rint(tx);
  q[1] = (int32_t)std::rint(ty);
  return true;
}

// E17's sums on the host, for E17 and E21: two sets of eight 128-bit sums and two counts (set 0: every pose added, set
// 1: those the caller says)
namespace {
struct EstimateSums {
  __int128 sum[2][8] = {};
  uint32_t count[2][2] = {{0, 0}, {0, 0}};
  // q: the X, Y, C, S of a pose that estimate_quantise admits
  void add(const int32_t q[4], uint32_t weight, bool in_set1) {
    const int64_t X = q[0], Y = q[1], C = q[2], S = q[3];
    const __int128 w = weight;
    const __int128 term[8] = {w, w * X, w * Y, w * C, w * S, w * (X * X), w * (X * Y), w * (Y * Y)};
    for (int k = 0; k < (in_set1 ? 2 : 1); ++k) {
      for (int m = 0; m < 8; ++m) sum[k][m] += term[m];
      count[k][0] += 1u;
      count[k][1] += weight != 0 ? 1u : 0u;
    }
  }
  // result words 2 - 5 and 8 - 71; bit k of what it returns: W of set k is zero
  uint32_t write(uint32_t *result) const {
    for (int k = 0; k < 2; ++k) {
      result[2 + 2 * k] = count[k][0];
      result[3 + 2 * k] = count[k][1];
      for (int m = 0; m < 8; ++m) {
        const unsigned __int128 v = (unsigned __int128)sum[k][m];
        for (int j = 0; j < 4; ++j) result[8 + 32 * k + 4 * m + j] = (uint32_t)(v >> (32 * j));
      }
    }
    return (sum[0][0] == 0 ? 1u : 0u) | (sum[1][0] == 0 ? 2u : 0u);
  }
};
}  // namespace

int32_t rplgpu_estimate_host(const float *poses, uint32_t P, const uint32_t *weights,
                             const rplgpu_pose_estimate_t *s, uint32_t center, uint32_t result[72]) {
  if (!poses || !result || rplgpu_pose_estimate_check(s) != RPLGPU_OK || P == 0 || P > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t qc = std::min(center, P - 1u);
  int32_t c[4] = {0, 0, 0, 0};
  const bool c_in = estimate_quantise(poses + 4u * (size_t)qc, s->xy_scale, c);
  EstimateSums sums;
  for (uint32_t i = 0; i < P; ++i) {
    int32_t q[4];
    if (!estimate_quantise(poses + 4u * (size_t)i, s->xy_scale, q)) continue;
    const int64_t dX = (int64_t)q[0] - c[0], dY = (int64_t)q[1] - c[1];
    const bool gate = c_in && (uint64_t)(dX * dX + dY * dY) <= s->gate_r2 &&
                      (int64_t)q[2] * c[2] + (int64_t)q[3] * c[3] >= s->gate_dot;
    sums.add(q, weights ? weights[i] : 1u, gate);
  }
  const uint32_t empty = sums.write(result);
  result[0] = (c_in ? 0u : 1u) | (result[2] != P ? 2u : 0u) | empty << 2;
  result[1] = qc;
  result[6] = result[7] = 0u;
  return RPLGPU_OK;
}

int32_t rplgpu_estimate_pose(const uint32_t result[72], float xy_scale, uint32_t set, double out[8]) {
  if (!result || !out || set > 1u || !std::isfinite(xy_scale) || !(xy_scale > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  double v[8];  // each sum rounded to fp64 once
  for (int m = 0; m < 8; ++m) {
    unsigned __int128 u = 0;
    for (int j = 3; j >= 0; --j) u = (u << 32) | result[8 + 32 * set + 4 * m + j];
    v[m] = (double)(__int128)u;
  }
  if (v[0] == 0.0) return RPLGPU_ERR_INVALID_ARG;  // (W < 2^52 is exact, so this is W == 0)
  const double scale = (double)xy_scale, scale2 = scale * scale;  // (24 x 24 bits: exact)
  const double mx = v[1] / v[0] / scale, my = v[2] / v[0] / scale;
  out[0] = mx;
  out[1] = my;
  out[2] = std::atan2(v[4], v[3]);
  out[3] = v[5] / v[0] / scale2 - mx * mx;
  out[4] = v[6] / v[0] / scale2 - mx * my;
  out[5] = v[7] / v[0] / scale2 - my * my;
  out[6] = std::hypot(v[3], v[4]) / (v[0] * 1048576.0);
  out[7] = v[0];
  return RPLGPU_OK;
}

// ---- E18: a pose list's motion noise --------------------------------------------------------------------------------

void rplgpu_default_motion_noise(rplgpu_motion_noise_t *s) {
  if (!s) return;
  s->seed = 0;
  s->step = 0;
  s->first = 0;
  s->reserved = 0;
}

static void philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
  }
  std::memcpy(out, c, 16);
}

int32_t rplgpu_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) return RPLGPU_ERR_INVALID_ARG;
  philox4x32(ctr, key, out);
  return RPLGPU_OK;
}

// E18's integer normal of one draw: the eight 16-bit halves of the block, minus their mean
static int32_t motion_draw(const rplgpu_motion_noise_t *s, uint32_t g, uint32_t j, uint32_t i) {
  const uint32_t ctr[4] = {s->first + j, (g << 2) | i, (uint32_t)s->step, (uint32_t)(s->step >> 32)};
  const uint32_t key[2] = {(uint32_t)s->seed, (uint32_t)(s->seed >> 32)};
  uint32_t w[4];
  philox4x32(ctr, key, w);
  int32_t z = -262140;
  for (int k = 0; k < 4; ++k) z += (int32_t)(w[k] & 0xFFFFu) + (int32_t)(w[k] >> 16);
  return z;
}

// E18's noise rotation by 2 atan(Z k): float32, every operation rounded once (-ffp-contract=off); the composition
// r o n is rotate()
static void motion_noise(int32_t z, float k, float n[2]) {
  const float t = (float)z * k, q = t * t, den = 1.0f + q;
  n[0] = (1.0f - q) / den;
  n[1] = (t + t) / den;
}

int32_t rplgpu_sample_motion_host(const float odom[8], uint32_t group, uint32_t M, const rplgpu_motion_noise_t *s,
                                  float *delta_out, uint32_t result[8]) {
  if (!odom || !s || !delta_out || !result || group > 65534u || M == 0 || M > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const float r1[2] = {odom[0], odom[1]}, r2[2] = {odom[3], odom[4]};
  const float trans = odom[2], k1 = odom[5], kt = odom[6], k2 = odom[7];
  uint32_t nans = 0, zmax = 0;
  int64_t sum = 0;
  uint64_t squares = 0;
  for (uint32_t j = 0; j < M; ++j) {
    int32_t z[3];
    for (uint32_t i = 0; i < 3; ++i) {
      z[i] = motion_draw(s, group, j, i);
      zmax = std::max(zmax, (uint32_t)std::abs(z[i]));
      sum += z[i];
      squares += (uint64_t)((int64_t)z[i] * z[i]);
    }
    float n1[2], n2[2], a[2], b[2], d[2];
    motion_noise(z[0], k1, n1);
    motion_noise(z[2], k2, n2);
    rotate(r1, n1, a);
    rotate(r2, n2, b);
    rotate(a, b, d);
    const float noise = (float)z[1] * kt;
    const float tr = trans + noise;
    float v[4] = {d[0], d[1], a[0] * tr, a[1] * tr};
    nans += canonical_nans(v) ? 1u : 0u;
    std::memcpy(delta_out + 4u * (size_t)j, v, 16);
  }
  result[0] = nans;
  result[1] = zmax;
  result[2] = (uint32_t)(uint64_t)sum;
  result[3] = (uint32_t)((uint64_t)sum >> 32);
  result[4] = (uint32_t)squares;
  result[5] = (uint32_t)(squares >> 32);
  result[6] = 0u;
  result[7] = nans ? 1u : 0u;
  return RPLGPU_OK;
}

int32_t rplgpu_motion_odometry(double dx, double dy, double dtheta, const double alpha[4], float out[8]) {
  if (!alpha || !out) return RPLGPU_ERR_INVALID_ARG;
  const double pi = 3.14159265358979323846;
  const double trans = std::sqrt(dx * dx + dy * dy);
  const double rot1 = trans >= 0.01 ? std::atan2(dy, dx) : 0.0;
  const double d = dtheta - rot1;
  const double rot2 = std::atan2(std::sin(d), std::cos(d));
  const double f1 = std::min(std::fabs(rot1), pi - std::fabs(rot1));
  const double f2 = std::min(std::fabs(rot2), pi - std::fabs(rot2));
  const double v1 = alpha[0] * f1 * f1 + alpha[1] * trans * trans;
  const double vt = alpha[2] * trans * trans + alpha[3] * (f1 * f1 + f2 * f2);
  const double v2 = alpha[0] * f2 * f2 + alpha[1] * trans * trans;
  const double sigma_z = std::sqrt(2863311530.0);
  out[0] = (float)std::cos(rot1);
  out[1] = (float)std::sin(rot1);
  out[2] = (float)trans;
  out[3] = (float)std::cos(rot2);
  out[4] = (float)std::sin(rot2);
  out[5] = (float)(std::sqrt(v1) / (2.0 * sigma_z));
  out[6] = (float)(std::sqrt(vt) / sigma_z);
  out[7] = (float)(std::sqrt(v2) / (2.0 * sigma_z));
  return RPLGPU_OK;
}

// ---- E19: a pose list seeded over a grid's free cells ---------------------------------------------------------------

void rplgpu_default_pose_seed(rplgpu_pose_seed_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->resolution = 0.05f;
  s->width = 1024;
  s->height = 1024;
  s->free_lo = 0;
  s->free_hi = 0;
  s->flags = 0;
}

int32_t rplgpu_pose_seed_check(const rplgpu_pose_seed_t *s) {
  if (!s || !grid_spec_ok(s->origin_x, s->origin_y, s->resolution, s->width, s->height)) return RPLGPU_ERR_INVALID_ARG;
  if (s->free_lo < -128 || s->free_lo > 127 || s->free_hi < -128 || s->free_hi > 127 || s->free_lo > s->free_hi)
    return RPLGPU_ERR_INVALID_ARG;
  if (s->flags > 1u) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

int32_t rplgpu_seed_headings(uint32_t H, float *cs) {
  if (!cs || H == 0 || H > 65536u) return RPLGPU_ERR_INVALID_ARG;
  const double two_pi = 6.283185307179586476925286766559;
  for (uint32_t k = 0; k < H; ++k) {
    const double a = two_pi * (double)k / (double)H;
    cs[2u * k] = k == 0 ? 1.0f : (float)std::cos(a);
    cs[2u * k + 1u] = k == 0 ? 0.0f : (float)std::sin(a);
  }
  return RPLGPU_OK;
}

// the E11 cell rule on the host, for E19, E22 and E23: float32, every operation rounded once (-ffp-contract=off)
static bool host_cell(float x, float y, float origin_x, float origin_y, float resolution, int32_t *cx, int32_t *cy) {
  const float du = x - origin_x, dv = y - origin_y;
  const float u = du / resolution, v = dv / resolution;
  const float fu = std::floor(u), fv = std::floor(v);
  if (!(std::fabs(fu) < 1048576.0f && std::fabs(fv) < 1048576.0f)) return false;
  *cx = (int32_t)fu;
  *cy = (int32_t)fv;
  return true;
}

int32_t rplgpu_seed_poses_host(const rplgpu_pose_seed_t *s, const int8_t *grid, const float *headings, uint32_t H,
                               uint32_t group, uint32_t M, const rplgpu_motion_noise_t *noise, float *poses_out,
                               uint32_t *cells_out, uint32_t result[8]) {
  if (rplgpu_pose_seed_check(s) != RPLGPU_OK || !grid || !headings || !noise || !poses_out || !result ||
      group > 65534u || H == 0 || H > 65536u || M == 0 || M > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t cells = s->width * s->height;
  auto is_free = [&](uint32_t i) { return grid[i] >= s->free_lo && grid[i] <= s->free_hi; };
  uint32_t F = 0;
  for (uint32_t i = 0; i < cells; ++i) F += is_free(i) ? 1u : 0u;
  const bool none = F == 0;
  if (none) F = cells;
  // the draws first, then ONE walk over the cells in index order hands every draw its cell: the outputs sorted by r
  std::vector<uint32_t> words(4u * (size_t)M), order(M), cell(M);
  const uint32_t key[2] = {(uint32_t)noise->seed, (uint32_t)(noise->seed >> 32)};
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t ctr[4] = {noise->first + j, (group << 2) | 3u, (uint32_t)noise->step,
                             (uint32_t)(noise->step >> 32)};
    philox4x32(ctr, key, &words[4u * (size_t)j]);
    order[j] = j;
  }
  auto rank = [&](uint32_t j) { return (uint32_t)(((uint64_t)words[4u * (size_t)j] * F) >> 32); };
  if (none) {
    for (uint32_t j = 0; j < M; ++j) cell[j] = rank(j);
  } else {
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rank(a) < rank(b); });
    uint32_t seen = 0, q = 0;  // free cells in front of cell i; outputs served
    for (uint32_t i = 0; i < cells && q < M; ++i) {
      if (!is_free(i)) continue;
      while (q < M && rank(order[q]) == seen) cell[order[q++]] = i;
      ++seen;
    }
  }
  uint32_t off = 0, lo = 0xFFFFFFFFu, hi = 0;
  const bool centres = (s->flags & 1u) != 0;
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t *p = &words[4u * (size_t)j];
    const uint32_t k = (uint32_t)(((uint64_t)p[1] * H) >> 32);
    const uint32_t cy = cell[j] / s->width, cx = cell[j] - cy * s->width;
    const float fx = centres ? 0.5f : ((float)(p[2] >> 24) + 0.5f) * (1.0f / 256.0f);
    const float fy = centres ? 0.5f : ((float)(p[3] >> 24) + 0.5f) * (1.0f / 256.0f);
    const float ux = (float)cx + fx, uy = (float)cy + fy;
    const float mx = ux * s->resolution, my = uy * s->resolution;
    const float x = s->origin_x + mx, y = s->origin_y + my;
    int32_t bx = 0, by = 0;
    if (!(host_cell(x, y, s->origin_x, s->origin_y, s->resolution, &bx, &by) && bx == (int32_t)cx && by == (int32_t)cy))
      ++off;
    lo = std::min(lo, cell[j]);
    hi = std::max(hi, cell[j]);
    std::memcpy(poses_out + 4u * (size_t)j, headings + 2u * (size_t)k, 8);  // bit for bit
    poses_out[4u * (size_t)j + 2u] = x;
    poses_out[4u * (size_t)j + 3u] = y;
    if (cells_out) cells_out[j] = cell[j];
  }
  result[0] = F;
  result[1] = off;
  result[2] = lo;
  result[3] = hi;
  result[4] = result[5] = result[6] = 0u;
  result[7] = (none ? 1u : 0u) | (off ? 2u : 0u);
  return RPLGPU_OK;
}

// ---- E20: a pose list's occupied bins and the KLD sample count ------------------------------------------------------

void rplgpu_default_pose_bins(rplgpu_pose_bins_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->inv_size = 2.0f;
  s->nx = 103;
  s->ny = 103;
  s->flags = 0;
}

int32_t rplgpu_pose_bins_check(const rplgpu_pose_bins_t *s, uint32_t T) {
  if (!s || !std::isfinite(s->origin_x) || !std::isfinite(s->origin_y) || !std::isfinite(s->inv_size))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(s->inv_size > 0.0f) || !bin_dims_ok(s->nx, s->ny, T) || s->flags > 1u) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_bin_map_words(uint32_t nx, uint32_t ny, uint32_t T) {
  if (!bin_dims_ok(nx, ny, T)) return 0;
  const uint64_t words = rpl::bin_map_words(nx * ny * T);  // (checked: at most RPLGPU_MAX_POSE_BINS bins)
  return (words + 1u) & ~(uint64_t)1u;
}

// E20's quantisation of (c, s): false for an entry that is out of range or quantises to (0, 0) (bn_quantise of
// rpl_bins.hip)
static bool bins_quantise(const float *cs, int32_t q[2]) { return quantise_cs(cs, q) && (q[0] != 0 || q[1] != 0); }
static uint32_t bins_half(const int32_t a[2]) { return (a[1] > 0 || (a[1] == 0 && a[0] > 0)) ? 0u : 1u; }
// a <= b in the angular order, both in range and not (0, 0)
static bool bins_le(const int32_t a[2], const int32_t b[2]) {
  const uint32_t ha = bins_half(a), hb = bins_half(b);
  if (ha != hb) return ha < hb;
  return (int64_t)a[0] * b[1] - (int64_t)a[1] * b[0] >= 0;
}

int32_t rplgpu_heading_edges_check(const float *cs, uint32_t T) {
  if (!cs || T == 0 || T > RPLGPU_MAX_HEADING_BINS) return RPLGPU_ERR_INVALID_ARG;
  int32_t prev[2], cur[2];
  if (!bins_quantise(cs, prev) || prev[0] != 1048576 || prev[1] != 0) return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t k = 1; k < T; ++k) {
    if (!bins_quantise(cs + 2u * (size_t)k, cur)) return RPLGPU_ERR_INVALID_ARG;
    if (bins_le(cur, prev)) return RPLGPU_ERR_INVALID_ARG;  // not strictly behind its predecessor
    prev[0] = cur[0];
    prev[1] = cur[1];
  }
  return RPLGPU_OK;
}

int32_t rplgpu_bin_poses_host(const rplgpu_pose_bins_t *s, const float *poses, uint32_t P, const uint32_t *weights,
                              const float *edges, uint32_t T, uint32_t *map, uint32_t *bins_out,
                              uint32_t result[8]) {
  if (rplgpu_pose_bins_check(s, T) != RPLGPU_OK || !poses || !edges || !map || !result || P == 0 ||
      P > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t nb = s->nx * s->ny * T, words = rpl::bin_map_words(nb);
  const bool keep = (s->flags & 1u) != 0;
  if (!keep) std::memset(map, 0, 4u * (size_t)words);
  std::vector<int32_t> eq(2u * (size_t)T);
  std::vector<unsigned char> e_ok(T);
  for (uint32_t k = 0; k < T; ++k) e_ok[k] = bins_quantise(edges + 2u * (size_t)k, &eq[2u * (size_t)k]) ? 1 : 0;
  uint32_t K = 0, counted = 0, outside = 0, skipped = 0, lo_bin = 0xFFFFFFFFu, hi_bin = 0;
  for (uint32_t i = 0; i < P; ++i) {
    const float *p = poses + 4u * (size_t)i;
    uint32_t b = 0xFFFFFFFFu;
    if (weights && weights[i] == 0u) {
      ++skipped;  // (whether or not it is in range)
    } else {
      const float dx = p[2] - s->origin_x, dy = p[3] - s->origin_y;
      const float fx = dx * s->inv_size, fy = dy * s->inv_size;  // (-ffp-contract=off: the difference rounded first)
      const bool x_in = fx >= 0.0f && fx < (float)s->nx;
      const bool y_in = fy >= 0.0f && fy < (float)s->ny;
      int32_t h[2];
      const bool h_in = bins_quantise(p, h);
      if (x_in && y_in && h_in) {
        const uint32_t bx = (uint32_t)std::floor(fx), by = (uint32_t)std::floor(fy);
        uint32_t lo = 0, hi = T;
        while (hi - lo > 1u) {
          const uint32_t mid = (lo + hi) >> 1;
          if (e_ok[mid] && bins_le(&eq[2u * (size_t)mid], h))
            lo = mid;
          else
            hi = mid;
        }
        b = (lo * s->ny + by) * s->nx + bx;
        ++counted;
        lo_bin = std::min(lo_bin, b);
        hi_bin = std::max(hi_bin, b);
        const uint32_t bit = 1u << (b & 31u);
        if (!(map[b >> 5] & bit)) ++K;  // a bit this call turns from 0 to 1
        map[b >> 5] |= bit;
      } else {
        ++outside;
      }
    }
    if (bins_out) bins_out[i] = b;
  }
  result[0] = K;
  result[1] = counted;
  result[2] = outside;
  result[3] = skipped;
  result[4] = lo_bin;
  result[5] = hi_bin;
  result[6] = 0u;
  result[7] = (counted == 0 ? 1u : 0u) | (outside != 0 ? 2u : 0u) | (keep ? 4u : 0u);
  return RPLGPU_OK;
}

uint32_t rplgpu_kld_samples(uint32_t k, double epsilon, double z, uint32_t m_min, uint32_t m_max) {
  if (k <= 1u) return m_max;
  const double b = 2.0 / (9.0 * ((double)k - 1.0));
  const double x = 1.0 - b + std::sqrt(b) * z;
  const double n = std::ceil(((double)k - 1.0) / (2.0 * epsilon) * x * x * x);
  if (!(n >= (double)m_min)) return m_min;  // (NaN too)
  if (n > (double)m_max) return m_max;
  return (uint32_t)n;
}

// ---- E21: a binned pose list clustered, the heaviest cluster summed -------------------------------------------------

void rplgpu_default_pose_clusters(rplgpu_pose_clusters_t *s) {
  if (!s) return;
  s->nx = 103;
  s->ny = 103;
  s->xy_scale = 1024.0f;
  s->flags = 1;
}

int32_t rplgpu_pose_clusters_check(const rplgpu_pose_clusters_t *s, uint32_t T) {
  if (!s || !bin_dims_ok(s->nx, s->ny, T)) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(s->xy_scale) || !(s->xy_scale > 0.0f) || s->flags > 1u) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

int32_t rplgpu_cluster_poses_host(const rplgpu_pose_clusters_t *s, const float *poses, uint32_t P,
                                  const uint32_t *weights, uint32_t T, const uint32_t *map, const uint32_t *bins,
                                  uint32_t *labels_out, uint32_t *clusters_out, uint32_t cluster_cap,
                                  uint32_t result[80]) {
  if (rplgpu_pose_clusters_check(s, T) != RPLGPU_OK || !poses || !map || !bins || !result || P == 0 ||
      P > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t nx = s->nx, ny = s->ny, nb = nx * ny * T, none = 0xFFFFFFFFu;
  const bool wrap = (s->flags & 1u) != 0;
  auto occupied = [&](uint32_t b) { return b < nb && ((map[b >> 5] >> (b & 31u)) & 1u) != 0; };
  // the occupied bins in ascending id; a bin's place in that list is found by bisection
  std::vector<uint32_t> ids;
  for (uint32_t b = 0; b < nb; ++b)
    if (occupied(b)) ids.push_back(b);
  const uint32_t K = (uint32_t)ids.size();
  std::memset(result, 0, 4u * RPLGPU_CLUSTER_WORDS);
  result[1] = result[72] = none;
  result[7] = K;
  if (K > RPLGPU_MAX_POSES) {  // the BOUND rule
    result[0] = 32u;
    if (labels_out)
      for (uint32_t i = 0; i < P; ++i) labels_out[i] = none;
    return RPLGPU_OK;
  }
  auto place = [&](uint32_t b) { return (uint32_t)(std::lower_bound(ids.begin(), ids.end(), b) - ids.begin()); };
  // a flood fill from every occupied bin not yet reached, in ascending id: the bin it starts from is the label, and
  // the clusters are met in ascending label order
  std::vector<uint32_t> cluster_of(K, none), label, stack;
  for (uint32_t k0 = 0; k0 < K; ++k0) {
    if (cluster_of[k0] != none) continue;
    const uint32_t c = (uint32_t)label.size();
    label.push_back(ids[k0]);
    cluster_of[k0] = c;
    stack.push_back(ids[k0]);
    while (!stack.empty()) {
      const uint32_t b = stack.back();
      stack.pop_back();
      const int64_t bx = b % nx, by = (b / nx) % ny, kt = b / nx / ny;
      for (int dk = -1; dk <= 1; ++dk) {
        int64_t k = kt + dk;
        if (wrap) k = (k + T) % T;
        if (k < 0 || k >= (int64_t)T) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          for (int dx = -1; dx <= 1; ++dx) {
            const int64_t x = bx + dx, y = by + dy;
            if (x < 0 || x >= (int64_t)nx || y < 0 || y >= (int64_t)ny) continue;  // no wrap in x or y
            const uint32_t q = (uint32_t)((k * ny + y) * nx + x);
            if (q == b || !occupied(q)) continue;
            const uint32_t at = place(q);
            if (cluster_of[at] != none) continue;
            cluster_of[at] = c;
            stack.push_back(q);
          }
        }
      }
    }
  }
  const uint32_t nc = (uint32_t)label.size();
  // the poses: labels, the clusters' weights and counts
  std::vector<uint64_t> W(nc, 0);
  std::vector<uint32_t> count(nc, 0), pose_cluster(P, none);
  uint32_t stray = 0, unlabelled = 0, flags = 0;
  for (uint32_t i = 0; i < P; ++i) {
    uint32_t lab = none;
    if (bins[i] == none) {
      ++unlabelled;
    } else if (!occupied(bins[i])) {
      ++stray;
      flags |= 16u;
    } else {
      const uint32_t c = cluster_of[place(bins[i])];
      lab = label[c];
      int32_t q[4];
      if (estimate_quantise(poses + 4u * (size_t)i, s->xy_scale, q)) {
        pose_cluster[i] = c;
        W[c] += weights ? weights[i] : 1u;
        count[c] += 1u;
      } else {
        flags |= 2u;
      }
    }
    if (labels_out) labels_out[i] = lab;
  }
  // BEST and SECOND: the largest W, ties to the smaller label (the clusters are in ascending label order)
  uint32_t best = none, second = none;
  for (uint32_t c = 0; c < nc; ++c)
    if (best == none || W[c] > W[best]) best = c;
  for (uint32_t c = 0; c < nc; ++c)
    if (c != best && (second == none || W[c] > W[second])) second = c;
  if (clusters_out) {
    for (uint32_t c = 0; c < nc && c < cluster_cap; ++c) {
      clusters_out[4u * c] = label[c];
      clusters_out[4u * c + 1u] = count[c];
      clusters_out[4u * c + 2u] = (uint32_t)W[c];
      clusters_out[4u * c + 3u] = (uint32_t)(W[c] >> 32);
    }
  }
  EstimateSums sums;
  for (uint32_t i = 0; i < P; ++i) {
    if (pose_cluster[i] == none) continue;
    int32_t q[4] = {0, 0, 0, 0};
    estimate_quantise(poses + 4u * (size_t)i, s->xy_scale, q);  // (admitted above)
    sums.add(q, weights ? weights[i] : 1u, pose_cluster[i] == best);
  }
  result[0] = (nc == 0 ? 1u : 0u) | flags | sums.write(result) << 2;
  result[1] = best != none ? label[best] : none;
  result[6] = nc;
  if (second != none) {
    result[72] = label[second];
    result[73] = count[second];
    result[74] = (uint32_t)W[second];
    result[75] = (uint32_t)(W[second] >> 32);
  }
  result[76] = stray;
  result[77] = unlabelled;
  return RPLGPU_OK;
}

// ---- E22: a beam fan cast from every pose of a list into a grid -----------------------------------------------------

void rplgpu_default_range_cast(rplgpu_range_cast_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->resolution = 0.05f;
  s->width = 1024;
  s->height = 1024;
  s->max_steps = 240;
  s->hit_lo = 100;
  s->unknown_stops = 1;
  s->table_half = 40;
}

int32_t rplgpu_range_cast_check(const rplgpu_range_cast_t *s) {
  if (!s || !grid_spec_ok(s->origin_x, s->origin_y, s->resolution, s->width, s->height)) return RPLGPU_ERR_INVALID_ARG;
  if (s->max_steps == 0 || s->max_steps > RPLGPU_MAX_OCC_STEPS) return RPLGPU_ERR_INVALID_ARG;
  if (s->hit_lo < 1 || s->hit_lo > 127 || s->unknown_stops > 1u || s->table_half > RPLGPU_MAX_CAST_TABLE_HALF)
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

double rplgpu_cast_range_m(uint32_t word, float resolution) {
  if (word == RPLGPU_CAST_DROPPED) return std::nan("");
  if ((word >> 28) == RPLGPU_CAST_NONE) return HUGE_VAL;
  return std::sqrt((double)(word & 0x0FFFFFFFu)) * (double)resolution;
}

// one ray by the header's rule; *n_out: the visit at which it stopped (0 for a dropped ray)
static uint32_t cast_ray(const rplgpu_range_cast_t *s, const float *pose, const float *beam, const int8_t *grid,
                         uint32_t *n_out) {
  const float tx = pose[2], ty = pose[3];
  float dir[2];
  rotate(pose, beam, dir);
  const float rm = (float)s->max_steps * s->resolution;
  const float mx = dir[0] * rm, my = dir[1] * rm;
  const float ex = tx + mx, ey = ty + my;
  int32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  *n_out = 0;
  if (!host_cell(tx, ty, s->origin_x, s->origin_y, s->resolution, &x0, &y0) ||
      !host_cell(ex, ey, s->origin_x, s->origin_y, s->resolution, &x1, &y1))
    return RPLGPU_CAST_DROPPED;
  const int32_t ax = std::abs(x1 - x0), ay = std::abs(y1 - y0);
  const int32_t stepx = (x1 > x0) - (x1 < x0), stepy = (y1 > y0) - (y1 < y0);
  int32_t err = ax - ay, x = x0, y = y0;
  uint32_t n = 0, kind;
  for (;;) {
    if (x < 0 || y < 0 || x >= (int32_t)s->width || y >= (int32_t)s->height) {
      kind = RPLGPU_CAST_LEFT;
      break;
    }
    const int32_t v = grid[(size_t)y * s->width + (size_t)x];
    if (v >= s->hit_lo) {
      kind = RPLGPU_CAST_HIT;
      break;
    }
    if (v < 0 && s->unknown_stops) {
      kind = RPLGPU_CAST_UNKNOWN;
      break;
    }
    if ((x == x1 && y == y1) || n == s->max_steps) {
      kind = RPLGPU_CAST_NONE;
      break;
    }
    const int32_t e2 = 2 * err;
    if (e2 > -ay) {
      err -= ay;
      x += stepx;
    }
    if (e2 < ax) {
      err += ax;
      y += stepy;
    }
    ++n;
  }
  *n_out = n;
  const int32_t dx = x - x0, dy = y - y0;
  return (uint32_t)(dx * dx + dy * dy) | (kind << 28);
}

// the table term of one range word against the measured range z (not NaN), the header's WEIGHT rule
static uint32_t cast_term(const rplgpu_range_cast_t *s, uint32_t word, float z, const uint8_t *table) {
  const int32_t K = (int32_t)s->table_half;
  const float mz = z / s->resolution;
  const float de = (word >> 28) == RPLGPU_CAST_NONE ? HUGE_VALF : std::sqrt((float)(word & 0x0FFFFFFFu));
  if (mz == HUGE_VALF && de == HUGE_VALF) return table[2 * K + 1];
  const float d = mz - de;
  const float cl = std::max(-(float)K, std::min((float)K, std::floor(d)));
  return table[K + (int32_t)cl];
}

int32_t rplgpu_cast_ranges_host(const rplgpu_range_cast_t *s, const float *poses, uint32_t P, const float *beams,
                                uint32_t A, const int8_t *grid, const float *measured, uint32_t meas_count,
                                uint32_t meas_first, uint32_t meas_step, const uint8_t *table, uint32_t *ranges_out,
                                uint32_t *weights_out, uint32_t result[8], uint32_t cast[8]) {
  if (rplgpu_range_cast_check(s) != RPLGPU_OK || !poses || !beams || !grid || !cast || (!ranges_out && !measured) ||
      P == 0 || P > RPLGPU_MAX_POSES || A == 0 || A > RPLGPU_MAX_MERGE_BEAMS ||
      (uint64_t)P * A > RPLGPU_MAX_CAST_RAYS)
    return RPLGPU_ERR_INVALID_ARG;
  if (measured && (!table || !weights_out || !result ||
                   (uint64_t)meas_first + (uint64_t)(A - 1u) * meas_step >= meas_count))
    return RPLGPU_ERR_INVALID_ARG;
  uint32_t counts[5] = {0, 0, 0, 0, 0}, far_hit = 0, beams_in = 0;
  uint64_t steps = 0;
  for (uint32_t q = 0; q < P; ++q) {
    uint32_t w = 0;
    for (uint32_t a = 0; a < A; ++a) {
      uint32_t n = 0;
      const uint32_t word = cast_ray(s, poses + 4u * (size_t)q, beams + 2u * (size_t)a, grid, &n);
      steps += n;
      if (word == RPLGPU_CAST_DROPPED) {
        ++counts[4];
      } else {
        ++counts[word >> 28];
        if ((word >> 28) == RPLGPU_CAST_HIT) far_hit = std::max(far_hit, word & 0x0FFFFFFFu);
      }
      if (ranges_out) ranges_out[(size_t)q * A + a] = word;
      if (measured && word != RPLGPU_CAST_DROPPED) {
        const float z = measured[meas_first + (size_t)a * meas_step];
        if (!std::isnan(z)) w += cast_term(s, word, z, table);
      }
    }
    if (measured) weights_out[q] = w;
  }
  if (measured) {
    for (uint32_t a = 0; a < A; ++a) beams_in += std::isnan(measured[meas_first + (size_t)a * meas_step]) ? 0u : 1u;
    score_result(weights_out, P, beams_in, result);
  }
  for (uint32_t i = 0; i < 5; ++i) cast[i] = counts[i];
  cast[5] = far_hit;
  cast[6] = (uint32_t)steps;
  cast[7] = (uint32_t)(steps >> 32);
  return RPLGPU_OK;
}

// ---- E23: the beams a pose list disagrees with are left out of the weights ------------------------------------------

void rplgpu_default_beam_agree(rplgpu_beam_agree_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->resolution = 0.05f;
  s->width = 1024;
  s->height = 1024;
  s->agree_lo = 1;
  s->keep_num = 3;
  s->keep_den = 10;
  s->err_num = 9;
  s->err_den = 10;
}

int32_t rplgpu_beam_agree_check(const rplgpu_beam_agree_t *s) {
  if (!s || !grid_spec_ok(s->origin_x, s->origin_y, s->resolution, s->width, s->height)) return RPLGPU_ERR_INVALID_ARG;
  if (s->agree_lo < 1 || s->agree_lo > 127) return RPLGPU_ERR_INVALID_ARG;
  if (s->keep_den == 0 || s->keep_den > RPLGPU_AGREE_MAX_DEN || s->keep_num > s->keep_den) return RPLGPU_ERR_INVALID_ARG;
  if (s->err_den == 0 || s->err_den > RPLGPU_AGREE_MAX_DEN || s->err_num > RPLGPU_AGREE_MAX_DEN)
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

// E23's three comparisons, for the host twin (the kernels of rpl_agree.hip spell the same expressions)
static bool agree_kept(const rplgpu_beam_agree_t *s, uint32_t count, uint32_t P) {
  return (uint64_t)count * s->keep_den > (uint64_t)s->keep_num * P;
}
static bool agree_falls_back(const rplgpu_beam_agree_t *s, uint32_t F, uint32_t K) {
  return F > 0 && (uint64_t)(F - K) * s->err_den >= (uint64_t)s->err_num * F;
}

// E15's field value of the point (x, y) at one pose: the point turned, then the translation added, each rounded;
// *no_cell is set for a position without a cell
static uint32_t agree_look_host(const rplgpu_beam_agree_t *s, const int8_t *field, const float *pose, float x, float y,
                                bool *no_cell) {
  const float point[2] = {x, y};
  float turned[2];
  rotate(pose, point, turned);
  const float rx = turned[0] + pose[2], ry = turned[1] + pose[3];
  int32_t cx = 0, cy = 0;
  if (!host_cell(rx, ry, s->origin_x, s->origin_y, s->resolution, &cx, &cy)) {
    *no_cell = true;
    return 0u;
  }
  if (cx < 0 || cy < 0 || (uint32_t)cx >= s->width || (uint32_t)cy >= s->height) return 0u;
  const int v = field[(size_t)cy * s->width + (size_t)cx];
  return (uint32_t)std::max(v, 0);
}

int32_t rplgpu_beam_agree_points_host(const float *x, const float *y, const uint32_t *slot, const uint32_t *index,
                                      uint32_t n_points, uint32_t n_scans, uint32_t n_stride, const float *poses,
                                      uint32_t P, const int8_t *field, const rplgpu_beam_agree_t *s,
                                      uint32_t *counts_out, uint32_t *mask_out, uint32_t *weights_out,
                                      uint32_t result[8], uint32_t agree[8], uint32_t *status) {
  if (rplgpu_beam_agree_check(s) != RPLGPU_OK || !poses || !field || !counts_out || !mask_out || !weights_out ||
      !result || !agree || (n_points && (!x || !y || !slot || !index)) || P == 0 || P > RPLGPU_MAX_POSES ||
      n_scans == 0 || n_stride == 0 || (uint64_t)n_scans * n_stride > (1ull << 24))
    return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t k = 0; k < n_points; ++k) {
    if (slot[k] >= n_scans || index[k] >= n_stride) return RPLGPU_ERR_INVALID_ARG;
  }
  const uint32_t mask_words = (n_stride + 31u) / 32u;
  std::fill(counts_out, counts_out + (size_t)n_scans * n_stride, 0u);
  std::fill(mask_out, mask_out + (size_t)n_scans * mask_words, 0u);
  std::vector<uint64_t> w(P, 0u);
  std::vector<uint32_t> finite;  // the points that are finite
  bool no_cell = false;
  // first all look-ups: E15's sums and the counts
  uint32_t hi = 0, lo = 0xFFFFFFFFu;
  uint64_t total = 0;
  for (uint32_t k = 0; k < n_points; ++k) {
    if (!(std::fabs(x[k]) < HUGE_VALF && std::fabs(y[k]) < HUGE_VALF)) continue;
    finite.push_back(k);
    uint32_t count = 0;
    for (uint32_t q = 0; q < P; ++q) {
      const uint32_t f = agree_look_host(s, field, poses + 4u * (size_t)q, x[k], y[k], &no_cell);
      w[q] += f;
      count += f >= (uint32_t)s->agree_lo ? 1u : 0u;
    }
    counts_out[(size_t)slot[k] * n_stride + index[k]] = count;
    hi = std::max(hi, count);
    lo = std::min(lo, count);
    total += count;
  }
  // the rule's mask, whether or not the group falls back
  const uint32_t F = (uint32_t)finite.size();
  uint32_t K = 0;
  for (uint32_t k : finite) {
    if (!agree_kept(s, counts_out[(size_t)slot[k] * n_stride + index[k]], P)) continue;
    mask_out[(size_t)slot[k] * mask_words + (index[k] >> 5)] |= 1u << (index[k] & 31u);
    ++K;
  }
  const bool back = agree_falls_back(s, F, K);
  if (!back) {  // the skipped samples leave the weights again
    for (uint32_t k : finite) {
      if ((mask_out[(size_t)slot[k] * mask_words + (index[k] >> 5)] >> (index[k] & 31u)) & 1u) continue;
      for (uint32_t q = 0; q < P; ++q) w[q] -= agree_look_host(s, field, poses + 4u * (size_t)q, x[k], y[k], &no_cell);
    }
  }
  // E15's result words from the final weights
  for (uint32_t q = 0; q < P; ++q) weights_out[q] = (uint32_t)w[q];  // (n_scans * n_stride <= 2^24: no sum wraps)
  score_result(weights_out, P, F, result);
  const uint32_t agr[8] = {F, K, back ? 1u : 0u, back ? F : K, hi, F ? lo : 0u, (uint32_t)total, (uint32_t)(total >> 32)};
  std::memcpy(agree, agr, 32);
  if (status) *status = no_cell ? RPLGPU_SCAN_CELL_RANGE : 0u;
  return RPLGPU_OK;
}

}  // extern "C"
