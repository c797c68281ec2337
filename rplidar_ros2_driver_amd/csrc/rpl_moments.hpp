// rpl_moments.hpp — E17's integer moments, what rpl_estimate.hip (E17), rpl_clusters.hip (E21) and rpl_bins.hip (E20,
// the (c, s) half of the quantisation) share: a pose entry is quantised by one float32 product and one
// round-to-nearest-even; from there on everything is integers, so no order of summation matters.
//
// A tile is 1024 poses, one per thread.  Per set (0: the poses that count, 1: the caller's choice among them) eleven
// 64-bit limbs:
//   W, wX, wY, wC, wS                       below 2^55 per pose, 2^61 per wave;
//   w * (m mod 2^23) and w * floor(m / 2^23) for m = XX, XY, YY (|m| <= 2^46): the same bounds,
// so a wave's sum of a limb never leaves 64 bits and nothing carries.
//   es_tile_sums   wave sums by row shifts, sixteen wave sums per limb in LDS, then thread m < 16 forms sum m of the
//                  tile in 128 bits (low limb + 2^23 * high limb for the second moments) and thread 16 the four counts;
//   es_finish_sums one workgroup per group, wave m owns sum m: lane l adds the tiles l, l + 64, ... (at most 16 rounds)
//                  in 128 bits with the carry by hand, the wave reduces the two halves by shuffles and lane 0 stores
//                  the four words; wave 0 adds the counts as well.
// The planes of a group (uint32 words; T tiles): 17 planes of T entries of 4 words, 68 T in all.  Plane m < 16,
// entry t: sum m = 8 k + j of tile t (set k, sum j in the header's order), 128-bit two's complement, low to high.
// Plane 16, entry t: the tile's counts (set 0, set 0 with w != 0, set 1, set 1 with w != 0).  A plane is read by
// consecutive lanes at consecutive entries.
// A unit that includes this is built with -ffp-contract=off: every float32 operation rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rpl_device.hpp"
#include "rplgpu_msg.h"

namespace rpl {

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
static_assert(RPLGPU_MAX_POSES / kEsTile <= (uint32_t)kBlock, "a lane of the finish body adds at most 16 tiles");
static_assert(kEsSums == (uint32_t)kWaves, "one wave of the finish body per sum");
static_assert(RPLGPU_ESTIMATE_WORDS == 8u + 4u * kEsSums, "the result's layout");

__host__ __device__ inline uint32_t es_tiles(uint32_t P) { return (P + kEsTile - 1u) / kEsTile; }
__host__ __device__ inline u64 es_group_words(uint32_t T) { return 4ull * kEsPlanes * T; }

// one entry of (c, s): one float32 product, the range test (false for NaN), one round-to-nearest-even
__device__ __forceinline__ bool es_quantise_cs(float c, float s, int32_t *C, int32_t *S) {
  const float tc = c * kEsCsScale, ts = s * kEsCsScale;
  const bool in = fabsf(tc) < kEsLimit && fabsf(ts) < kEsLimit;
  *C = in ? (int32_t)rintf(tc) : 0;
  *S = in ? (int32_t)rintf(ts) : 0;
  return in;
}

struct EsPose {
  int32_t X, Y, C, S;
  bool in;
};

// one float32 product and one round-to-nearest-even per entry
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
  u64 *p = reinterpret_cast<u64 *>(at);  // (the planes are 8-byte aligned and an entry has 16 bytes)
  p[0] = (u64)v;
  p[1] = (u64)((unsigned __int128)v >> 64);
}

// The thread's pose q with weight w (0 for a thread without a pose) added to tile `tile` of the group's planes: into
// set 0 when in0, into set 1 as well when in1 (in1 implies in0).  The whole workgroup calls it; it holds a barrier.
__device__ __forceinline__ void es_tile_sums(const EsPose &q, uint32_t w, bool in0, bool in1, uint32_t tile,
                                             uint32_t T, uint32_t *planes) {
  __shared__ i64 s_limb[2u * kEsLimbs][kWaves];
  __shared__ uint32_t s_cnt[kWaves];
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
  if (threadIdx.x < kEsSums) {
    const uint32_t set = threadIdx.x >> 3, j = threadIdx.x & 7u;
    const uint32_t a = set * kEsLimbs + (j < 5u ? j : 5u + 2u * (j - 5u));
    i128 low = 0, high = 0;
    for (int k = 0; k < kWaves; ++k) {
      low += s_limb[a][k];
      if (j >= 5u) high += s_limb[a + 1u][k];
    }
    es_store128(planes + 4u * ((size_t)threadIdx.x * T + tile), low + high * (i128)8388608);
  } else if (threadIdx.x == kEsSums) {
    uint32_t n[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < kWaves; ++k) {
      const uint32_t v = s_cnt[k];
      n[0] += v & 0xFFu;
      n[1] += (v >> 8) & 0xFFu;
      n[2] += (v >> 16) & 0xFFu;
      n[3] += v >> 24;
    }
    u64 *rec = reinterpret_cast<u64 *>(planes + 4u * ((size_t)kEsSums * T + tile));
    rec[0] = (u64)n[0] | (u64)n[1] << 32;
    rec[1] = (u64)n[2] | (u64)n[3] << 32;
  }
}

// The group's planes added up over its T tiles: result words 8 - 71 written to res, the four counts left in s_cnt[4]
// and "W of set 0 / set 1 is zero" in s_empty[2] (LDS of the caller, valid in every thread behind the barrier this
// ends with) for the caller's own words.
__device__ __forceinline__ void es_finish_sums(const uint32_t *planes, uint32_t T, uint32_t *res, uint32_t *s_cnt,
                                               uint32_t *s_empty) {
  const uint32_t m = wave_id();
  u64 lo = 0ull, hi = 0ull;
  for (uint32_t t = lane_id(); t < T; t += 64u) {  // at most 16 rounds: T <= 1024
    const u64 *rec = reinterpret_cast<const u64 *>(planes + 4u * ((size_t)m * T + t));
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
      const uint32_t *rec = planes + 4u * ((size_t)kEsSums * T + t);
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
}

}  // namespace rpl
