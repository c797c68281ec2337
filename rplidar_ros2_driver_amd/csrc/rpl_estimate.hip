// rpl_estimate.hip — E17: a weighted pose list reduced to the sums of a pose estimate, include/rplgpu_msg.h,
// rplgpu_estimate_poses_dev: E15's weights and the list they weigh (or E16's list, every weight 1) become the integer
// moments a mean pose and its covariance are formed from.  Every pose entry is quantised by one float32 product and
// one round-to-nearest-even; from there on everything is integers, so no order of summation matters.
//
// Two launches, 1024 poses per tile, no workgroup waits on another, no atomic and no loop bounded by a word from memory:
//   k_estimate_tiles   one pose per thread (one 16-byte load, one 4-byte load); every thread quantises the centre pose
//                      itself (a broadcast load).  Per set (0: in range, 1: in the gate) eleven 64-bit limbs:
//                        W, wX, wY, wC, wS                       below 2^55 per pose, 2^61 per wave;
//                        w * (m mod 2^23) and w * floor(m / 2^23) for m = XX, XY, YY (|m| <= 2^46): the same bounds,
//                      so a wave's sum of a limb never leaves 64 bits and nothing carries.  Wave sums by row shifts,
//                      sixteen wave sums per limb in LDS, then thread m < 16 forms sum m of the tile in 128 bits
//                      (low limb + 2^23 * high limb for the second moments) and thread 16 the four counts;
//   k_estimate_finish  one workgroup per group, wave m owns sum m: lane l adds the tiles l, l + 64, ... (at most 16
//                      rounds) in 128 bits with the carry by hand, the wave reduces the two halves by shuffles and lane 0
//                      stores the four words; wave 0 adds the counts as well; thread 0 writes words 0 - 7.
// The scratch of a group (uint32 words; T tiles): 17 planes of T entries of 4 words, 68 T in all.  Plane m < 16,
// entry t: sum m = 8 k + j of tile t (set k, sum j in the header's order), 128-bit two's complement, low to high.
// Plane 16, entry t: the tile's counts (in range, in range with w != 0, in the gate, in the gate with w != 0).
// A plane is read by consecutive lanes at consecutive entries.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef __int128 i128;
typedef float es_f32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kEsTile = kBlock;   // poses per tile: one per thread
constexpr uint32_t kEsSums = 16u;      // two sets of eight
constexpr uint32_t kEsPlanes = 17u;    // the sums and the counts
constexpr uint32_t kEsLimbs = 11u;     // 64-bit limbs per set inside a tile
constexpr float kEsCsScale = 1048576.0f;
constexpr float kEsLimit = 8388608.0f;
static_assert(RPLGPU_MAX_POSES / kEsTile <= (uint32_t)kBlock, "a lane of the finish kernel adds at most 16 tiles");
static_assert(kEsSums == (uint32_t)kWaves, "one wave of the finish kernel per sum");
static_assert(RPLGPU_ESTIMATE_WORDS == 8u + 4u * kEsSums, "the result's layout");

__host__ __device__ inline uint32_t es_tiles(uint32_t P) { return (P + kEsTile - 1u) / kEsTile; }
__host__ __device__ inline u64 es_group_words(uint32_t T) { return 4ull * kEsPlanes * T; }

struct EsPose {
  int32_t X, Y, C, S;
  bool in;
};

// one float32 product and one round-to-nearest-even per entry (this unit is built with -ffp-contract=off)
__device__ __forceinline__ EsPose es_quantise(es_f32x4 v, float xy_scale) {
  const float tc = v.x * kEsCsScale, ts = v.y * kEsCsScale, tx = v.z * xy_scale, ty = v.w * xy_scale;
  EsPose q;
  q.in = fabsf(tx) < kEsLimit && fabsf(ty) < kEsLimit && fabsf(tc) < kEsLimit && fabsf(ts) < kEsLimit;  // NaN: false
  q.X = q.in ? (int32_t)rintf(tx) : 0;
  q.Y = q.in ? (int32_t)rintf(ty) : 0;
  q.C = q.in ? (int32_t)rintf(tc) : 0;
  q.S = q.in ? (int32_t)rintf(ts) : 0;
  return q;
}

// the sum of a 64-bit value over the wave, valid in lane 63: the row shifts and row broadcasts of wave_incl_scan_fast
// on both halves (a lane without a source adds 0)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ i64 es_dpp_add(i64 v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u64)v, CTRL, ROWMASK, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((u64)v >> 32), CTRL, ROWMASK, 0xF, false);
  return (i64)((u64)v + (((u64)hi << 32) | lo));
}
__device__ __forceinline__ i64 es_wave_sum_lane63(i64 v) {
  v = es_dpp_add<0x111, 0xF>(v);  // row_shr:1
  v = es_dpp_add<0x112, 0xF>(v);  // row_shr:2
  v = es_dpp_add<0x114, 0xF>(v);  // row_shr:4
  v = es_dpp_add<0x118, 0xF>(v);  // row_shr:8
  v = es_dpp_add<0x142, 0xA>(v);  // row_bcast:15 -> rows 1,3
  v = es_dpp_add<0x143, 0xC>(v);  // row_bcast:31 -> rows 2,3
  return v;
}

__device__ __forceinline__ void es_store128(uint32_t *at, i128 v) {
  u64 *p = reinterpret_cast<u64 *>(at);  // (the scratch is 8-byte aligned and an entry has 16 bytes)
  p[0] = (u64)v;
  p[1] = (u64)((unsigned __int128)v >> 64);
}

__global__ __launch_bounds__(kBlock) void k_estimate_tiles(const float *__restrict__ poses, u64 pose_stride,
                                                           uint32_t poses_per_group,
                                                           const uint32_t *__restrict__ weights, u64 weight_stride,
                                                           uint32_t P, float xy_scale, u64 gate_r2, i64 gate_dot,
                                                           const uint32_t *__restrict__ center, u64 center_stride,
                                                           uint32_t *__restrict__ scratch) {
  __shared__ i64 s_limb[2u * kEsLimbs][kWaves];
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t tile = blockIdx.x, g = blockIdx.y;
  const uint32_t T = es_tiles(P);
  const es_f32x4 *src =
      reinterpret_cast<const es_f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
  const uint32_t qc = min(center ? center[(size_t)g * center_stride] : 0u, P - 1u);  // clamped before it is used
  const EsPose c = es_quantise(src[qc], xy_scale);
  const uint32_t i = tile * kEsTile + threadIdx.x;
  const bool live = i < P;
  const es_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const EsPose q = es_quantise(live ? src[i] : zero, xy_scale);
  const uint32_t w = live ? (weights ? weights[(size_t)g * weight_stride + i] : 1u) : 0u;
  const bool in0 = live && q.in;
  const i64 dX = (i64)q.X - c.X, dY = (i64)q.Y - c.Y;
  const u64 r2 = (u64)(dX * dX + dY * dY);
  const i64 dot = (i64)q.C * c.C + (i64)q.S * c.S;
  const bool in1 = in0 && c.in && r2 <= gate_r2 && dot >= gate_dot;
  const i64 w0 = in0 ? (i64)w : 0ll;
  const i64 xx = (i64)q.X * q.X, xy = (i64)q.X * q.Y, yy = (i64)q.Y * q.Y;
  i64 l[2u * kEsLimbs];
  l[0] = w0;
  l[1] = w0 * q.X;
  l[2] = w0 * q.Y;
  l[3] = w0 * q.C;
  l[4] = w0 * q.S;
  l[5] = w0 * (xx & 0x7FFFFFll);
  l[6] = w0 * (xx >> 23);
  l[7] = w0 * (xy & 0x7FFFFFll);
  l[8] = w0 * (xy >> 23);  // (an arithmetic shift: floor, so that low + 2^23 * high is xy for either sign)
  l[9] = w0 * (yy & 0x7FFFFFll);
  l[10] = w0 * (yy >> 23);
#pragma unroll
  for (uint32_t k = 0; k < kEsLimbs; ++k) l[kEsLimbs + k] = in1 ? l[k] : 0ll;
#pragma unroll
  for (uint32_t k = 0; k < 2u * kEsLimbs; ++k) {
    const i64 sum = es_wave_sum_lane63(l[k]);
    if (lane_id() == 63u) s_limb[k][wave_id()] = sum;
  }
  // the four counts of a wave are at most 64 each: one byte each
  const uint32_t alive = w != 0u ? 1u : 0u;
  const uint32_t cnt = wave_incl_scan_fast((in0 ? 1u | alive << 8 : 0u) | (in1 ? 1u << 16 | alive << 24 : 0u));
  if (lane_id() == 63u) s_cnt[wave_id()] = cnt;
  __syncthreads();
  uint32_t *grp = scratch + (size_t)g * es_group_words(T);
  if (threadIdx.x < kEsSums) {
    const uint32_t set = threadIdx.x >> 3, j = threadIdx.x & 7u;
    const uint32_t a = set * kEsLimbs + (j < 5u ? j : 5u + 2u * (j - 5u));
    i128 low = 0, high = 0;
    for (int k = 0; k < kWaves; ++k) {
      low += s_limb[a][k];
      if (j >= 5u) high += s_limb[a + 1u][k];
    }
    es_store128(grp + 4u * ((size_t)threadIdx.x * T + tile), low + high * (i128)8388608);
  } else if (threadIdx.x == kEsSums) {
    uint32_t n[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < kWaves; ++k) {
      const uint32_t v = s_cnt[k];
      n[0] += v & 0xFFu;
      n[1] += (v >> 8) & 0xFFu;
      n[2] += (v >> 16) & 0xFFu;
      n[3] += v >> 24;
    }
    u64 *rec = reinterpret_cast<u64 *>(grp + 4u * ((size_t)kEsSums * T + tile));
    rec[0] = (u64)n[0] | (u64)n[1] << 32;
    rec[1] = (u64)n[2] | (u64)n[3] << 32;
  }
}

__global__ __launch_bounds__(kBlock) void k_estimate_finish(const float *__restrict__ poses, u64 pose_stride,
                                                            uint32_t poses_per_group, uint32_t P, float xy_scale,
                                                            const uint32_t *__restrict__ center, u64 center_stride,
                                                            const uint32_t *__restrict__ scratch,
                                                            uint32_t *__restrict__ result) {
  __shared__ uint32_t s_cnt[4];
  __shared__ uint32_t s_empty[2];
  const uint32_t g = blockIdx.x, m = wave_id();
  const uint32_t T = es_tiles(P);
  const uint32_t *grp = scratch + (size_t)g * es_group_words(T);
  uint32_t *res = result + (size_t)RPLGPU_ESTIMATE_WORDS * g;
  u64 lo = 0ull, hi = 0ull;
  for (uint32_t t = lane_id(); t < T; t += 64u) {  // at most 16 rounds: T <= 1024
    const u64 *rec = reinterpret_cast<const u64 *>(grp + 4u * ((size_t)m * T + t));
    const u64 a = rec[0];
    lo += a;
    hi += rec[1] + (lo < a ? 1ull : 0ull);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const u64 olo = __shfl_xor(lo, d, 64), ohi = __shfl_xor(hi, d, 64);
    lo += olo;
    hi += ohi + (lo < olo ? 1ull : 0ull);  // (both lanes of a pair see the same carry)
  }
  if (lane_id() == 0u) {
    uint32_t *out = res + 8u + 4u * m;
    out[0] = (uint32_t)lo;
    out[1] = (uint32_t)(lo >> 32);
    out[2] = (uint32_t)hi;
    out[3] = (uint32_t)(hi >> 32);
    if ((m & 7u) == 0u) s_empty[m >> 3] = (lo | hi) == 0ull ? 1u : 0u;  // W of set 0 and of set 1
  }
  if (m == 0u) {  // (wave-uniform) the counts: at most 2^20 each
    uint32_t n0 = 0u, n1 = 0u, n2 = 0u, n3 = 0u;
    for (uint32_t t = lane_id(); t < T; t += 64u) {
      const uint32_t *rec = grp + 4u * ((size_t)kEsSums * T + t);
      n0 += rec[0];
      n1 += rec[1];
      n2 += rec[2];
      n3 += rec[3];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      n0 += __shfl_xor(n0, d, 64);
      n1 += __shfl_xor(n1, d, 64);
      n2 += __shfl_xor(n2, d, 64);
      n3 += __shfl_xor(n3, d, 64);
    }
    if (lane_id() == 0u) {
      s_cnt[0] = n0;
      s_cnt[1] = n1;
      s_cnt[2] = n2;
      s_cnt[3] = n3;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const es_f32x4 *src =
        reinterpret_cast<const es_f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
    const uint32_t qc = min(center ? center[(size_t)g * center_stride] : 0u, P - 1u);
    const EsPose c = es_quantise(src[qc], xy_scale);
    res[0] = (c.in ? 0u : 1u) | (s_cnt[0] != P ? 2u : 0u) | (s_empty[0] ? 4u : 0u) | (s_empty[1] ? 8u : 0u);
    res[1] = qc;
    res[2] = s_cnt[0];
    res[3] = s_cnt[1];
    res[4] = s_cnt[2];
    res[5] = s_cnt[3];
    res[6] = 0u;
    res[7] = 0u;
  }
}

}  // namespace

unsigned long long estimate_scratch_words(uint32_t G, uint32_t P) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES) return 0ull;
  return (u64)G * es_group_words(es_tiles(P));
}

hipError_t launch_estimate(hipStream_t s, const float *poses, unsigned long long pose_stride,
                           uint32_t poses_per_group, const uint32_t *weights, unsigned long long weight_stride,
                           uint32_t G, uint32_t P, float xy_scale, unsigned long long gate_r2, long long gate_dot,
                           const uint32_t *center, unsigned long long center_stride, uint32_t *result,
                           uint32_t *scratch) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || pose_stride < 4ull * P ||
      (weights && weight_stride < P))
    return hipErrorInvalidValue;
  const uint32_t T = es_tiles(P);
  hipLaunchKernelGGL(k_estimate_tiles, dim3(T, G), dim3(kBlock), 0, s, poses, pose_stride, poses_per_group, weights,
                     weight_stride, P, xy_scale, gate_r2, gate_dot, center, center_stride, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_estimate_finish, dim3(G), dim3(kBlock), 0, s, poses, pose_stride, poses_per_group, P,
                     xy_scale, center, center_stride, scratch, result);
  return hipGetLastError();
}

}  // namespace rpl
