// rpl_motion.hip — E18: a pose list's motion noise drawn on the device, include/rplgpu_msg.h,
// rplgpu_sample_motion_dev: per group one odometry increment (two unit vectors, a translation, three noise scales)
// becomes M deltas in E16's n_delta = M layout.  The generator is counter based (Philox4x32-10): output j of group g
// depends on (seed, step, first + j, g) alone, so no state lives on the device and no order matters.
//
// Two launches, no workgroup waits on another, every loop bounded by a constant, no index that comes from data:
//   k_motion_prepare   zeroes the eight result words of every group;
//   k_motion_sample    grid (tiles of 1024 outputs, G), one output per thread: three Philox blocks (rot1, trans, rot2),
//                      each reduced to the integer normal Z (the eight 16-bit halves minus 262140); the float32 steps
//                      of the header, each rounded once (this unit is built with -ffp-contract=off; `/` is the IEEE
//                      divide); one 16-byte store.  The statistics of a tile fit 32 bits — |sum Z| < 2^30, and Z^2
//                      (below 2^37) travels as its low 16 bits and the rest, both sums below 2^32 — so the wave sums
//                      are the 32-bit row shifts of rpl_device.hpp, sixteen per value through LDS, and thread 0 adds
//                      the tile to the group's words with integer atomics.  The result words are only 4-byte aligned:
//                      a 64-bit sum is two 32-bit atomic adds, the high one with the carry the low one's return value
//                      shows.  The number of carries is floor((the sum of all low parts) / 2^32) whatever the order,
//                      so the words have one answer.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_philox.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef float mo_f32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kMoTile = kBlock;  // outputs per tile: one per thread
constexpr int32_t kMoZBias = 262140;  // 4 * 65535: the mean of the eight halves

// Philox4x32-10 (rpl_philox.hpp) on the counter (c0, c1, c2, c3) under the key (k0, k1), reduced to Z
__device__ __forceinline__ int32_t mo_draw(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                           uint32_t k1) {
  const Philox4 p = philox4x32_10(c0, c1, c2, c3, k0, k1);
  const uint32_t halves = (p.w0 & 0xFFFFu) + (p.w0 >> 16) + (p.w1 & 0xFFFFu) + (p.w1 >> 16) + (p.w2 & 0xFFFFu) +
                          (p.w2 >> 16) + (p.w3 & 0xFFFFu) + (p.w3 >> 16);
  return (int32_t)halves - kMoZBias;
}

struct MoRot {
  float c, s;
};
// the rotation by 2 atan(t), t = Z * k: a unit vector without a cosine
__device__ __forceinline__ MoRot mo_noise(int32_t z, float k) {
  const float t = (float)z * k, q = t * t, den = 1.0f + q;
  MoRot n;
  n.c = (1.0f - q) / den;
  n.s = (t + t) / den;
  return n;
}
// r o n: each product rounded, then the difference or sum
__device__ __forceinline__ MoRot mo_compose(MoRot r, MoRot n) {
  const float p0 = r.c * n.c, p1 = r.s * n.s, p2 = r.s * n.c, p3 = r.c * n.s;
  MoRot a;
  a.c = p0 - p1;
  a.s = p2 + p3;
  return a;
}
__device__ __forceinline__ float mo_canon(float v, bool *nan) {
  const bool is = v != v;
  *nan = *nan || is;
  return is ? __uint_as_float(0x7FC00000u) : v;
}

// a 64-bit value added to two 4-byte aligned words: the carry out of the low word is what its atomic returns
__device__ __forceinline__ void mo_add64(uint32_t *at, u64 v) {
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  const uint32_t old = atomicAdd(at, lo);
  const uint32_t up = hi + ((uint32_t)(old + lo) < old ? 1u : 0u);
  if (up) atomicAdd(at + 1, up);
}

__global__ __launch_bounds__(kBlock) void k_motion_prepare(uint32_t *__restrict__ result, uint32_t words) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < words) result[i] = 0u;
}

__global__ __launch_bounds__(kBlock) void k_motion_sample(const float *__restrict__ odom, uint32_t odom_per_group,
                                                          uint32_t M, uint32_t seed_lo, uint32_t seed_hi,
                                                          uint32_t step_lo, uint32_t step_hi, uint32_t first,
                                                          float *__restrict__ delta, u64 delta_stride,
                                                          uint32_t *__restrict__ result) {
  __shared__ uint32_t s_part[5][kWaves];
  const uint32_t g = blockIdx.y;
  const uint32_t j = blockIdx.x * kMoTile + threadIdx.x;
  const bool live = j < M;
  const mo_f32x4 *od = reinterpret_cast<const mo_f32x4 *>(odom + 8u * (size_t)(odom_per_group ? g : 0u));
  const mo_f32x4 o0 = od[0], o1 = od[1];  // (c1, s1, trans, c2), (s2, k1, kt, k2)
  const uint32_t c0 = first + j;          // (mod 2^32)
  const int32_t z0 = mo_draw(c0, g << 2, step_lo, step_hi, seed_lo, seed_hi);
  const int32_t z1 = mo_draw(c0, g << 2 | 1u, step_lo, step_hi, seed_lo, seed_hi);
  const int32_t z2 = mo_draw(c0, g << 2 | 2u, step_lo, step_hi, seed_lo, seed_hi);
  MoRot r1, r2;
  r1.c = o0.x;
  r1.s = o0.y;
  r2.c = o0.w;
  r2.s = o1.x;
  const MoRot a = mo_compose(r1, mo_noise(z0, o1.y));
  const MoRot b = mo_compose(r2, mo_noise(z2, o1.w));
  const float noise = (float)z1 * o1.z;
  const float tr = o0.z + noise;
  const MoRot d = mo_compose(a, b);
  bool nan = false;
  mo_f32x4 out;
  out.x = mo_canon(d.c, &nan);
  out.y = mo_canon(d.s, &nan);
  out.z = mo_canon(a.c * tr, &nan);
  out.w = mo_canon(a.s * tr, &nan);
  if (live) reinterpret_cast<mo_f32x4 *>(delta + (size_t)g * delta_stride)[j] = out;  // j < M <= delta_stride / 4
  // the tile's statistics, a thread without an output adding nothing
  const u64 w0 = (u64)((i64)z0 * z0), w1 = (u64)((i64)z1 * z1), w2 = (u64)((i64)z2 * z2);
  const uint32_t v_nan = live && nan ? 1u : 0u;
  const uint32_t v_max = live ? (uint32_t)max(max(abs(z0), abs(z1)), abs(z2)) : 0u;
  const uint32_t v_sum = live ? (uint32_t)(z0 + z1 + z2) : 0u;  // (two's complement)
  const uint32_t v_lo = live ? (uint32_t)(w0 & 0xFFFFu) + (uint32_t)(w1 & 0xFFFFu) + (uint32_t)(w2 & 0xFFFFu) : 0u;
  const uint32_t v_hi = live ? (uint32_t)(w0 >> 16) + (uint32_t)(w1 >> 16) + (uint32_t)(w2 >> 16) : 0u;
  const uint32_t t_nan = wave_incl_scan_fast(v_nan), t_max = wave_max_lane63(v_max);
  const uint32_t t_sum = wave_incl_scan_fast(v_sum), t_lo = wave_incl_scan_fast(v_lo);
  const uint32_t t_hi = wave_incl_scan_fast(v_hi);
  if (lane_id() == 63u) {
    s_part[0][wave_id()] = t_nan;
    s_part[1][wave_id()] = t_max;
    s_part[2][wave_id()] = t_sum;
    s_part[3][wave_id()] = t_lo;
    s_part[4][wave_id()] = t_hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t n = 0u, m = 0u, sum = 0u, lo = 0u, hi = 0u;
    for (int k = 0; k < kWaves; ++k) {
      n += s_part[0][k];
      m = max(m, s_part[1][k]);
      sum += s_part[2][k];
      lo += s_part[3][k];
      hi += s_part[4][k];
    }
    uint32_t *res = result + 8u * (size_t)g;
    if (n) {
      atomicAdd(res + 0, n);
      atomicOr(res + 7, 1u);
    }
    atomicMax(res + 1, m);
    mo_add64(res + 2, (u64)(i64)(int32_t)sum);  // |sum Z| of a tile < 2^30: the sign extends
    mo_add64(res + 4, (u64)lo + ((u64)hi << 16));
  }
}

}  // namespace

hipError_t launch_motion(hipStream_t s, const float *odom, uint32_t odom_per_group, uint32_t G, uint32_t M,
                         unsigned long long seed, unsigned long long step, uint32_t first, float *delta,
                         unsigned long long delta_stride, uint32_t *result) {
  if (G == 0 || G > 65535u || M == 0 || M > RPLGPU_MAX_POSES || delta_stride < 4ull * M || (delta_stride & 3u))
    return hipErrorInvalidValue;
  const uint32_t words = 8u * G;
  hipLaunchKernelGGL(k_motion_prepare, dim3((words + kBlock - 1u) / kBlock), dim3(kBlock), 0, s, result, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_motion_sample, dim3((M + kMoTile - 1u) / kMoTile, G), dim3(kBlock), 0, s, odom,
                     odom_per_group, M, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step,
                     (uint32_t)(step >> 32), first, delta, delta_stride, result);
  return hipGetLastError();
}

}  // namespace rpl
