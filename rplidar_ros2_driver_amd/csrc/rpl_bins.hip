// rpl_bins.hip — E20: a pose list's occupied bins counted on the device, include/rplgpu_msg.h, rplgpu_bin_poses_dev:
// per group the P poses (c, s, x, y) of E15 / E16 / E17's layout are binned in (x, y, heading) by fixed float32 and
// integer rules and marked in the group's bit map; eight result words give K (the bits turned from 0 to 1), the poses
// counted, out of range and skipped, and the range of the bin ids.
//
// Two launches, no workgroup waits on another, every loop bounded by a constant, every index that comes from data
// clamped into its array:
//   k_bins_start   grid (blocks of 8192 map words, G): the map words cleared with 8-byte stores (one block per group
//                  and nothing cleared under KEEP); block 0 of a group starts its eight result words.
//   k_bins_mark    grid (tiles of 1024 poses, G), one pose per thread, one 16-byte load.  Each workgroup quantises the
//                  edge table into LDS once (an edge that is out of range or (0, 0) is stored as (0, 0): never <=
//                  anything); the heading bin is the header's bisection, 10 steps, `mid` clamped into the table.
//                  THE MARKS: the list that matters most, a converged one, puts every pose into the same few map
//                  words, and one word takes about 88 returning atomics per microsecond.  So
//                    (1) the lanes of a wave that hit the same word are merged before anything leaves the wave: take
//                        the first pending lane's word, OR the bits of the lanes that share it (six DPP steps), hand
//                        the union to that lane and retire them — one round for a converged list.  The rounds stop
//                        at 8, not at the 64 a wave could need: a lane still pending then marks alone, which only
//                        happens on a list spread over many words, where there is little to merge and (2) still
//                        holds the atomics down (measured: 2^20 spread poses 0.201 ms for 0.227 ms with 64 rounds,
//                        16384 poses 0.019 ms for 0.026 ms, the converged and the one-bin list unchanged);
//                    (2) the lanes that hold a union then read their word at device scope (a relaxed agent-scope
//                        load: L2, never a stale L1 line) and skip the atomic when every bit is already there — a
//                        stale read only costs an atomic, never the count;
//                    (3) K is the popcount of bits & ~old over the values the RETURNING atomic ORs gave back: each bit
//                        goes 0 -> 1 exactly once and exactly one atomic sees it, in any order, and a bit that KEEP
//                        found set is nobody's.
//                  A tile's statistics are wave reductions through LDS and thread 0's integer atomics, as E18 / E19.
// The quantisation of (c, s) is E17's (rpl_moments.hpp, es_quantise_cs).  This unit is built with -ffp-contract=off:
// every float32 operation rounds once.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_moments.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

constexpr uint32_t kBnTile = kBlock;          // poses per tile: one per thread
constexpr uint32_t kBnClearWords = 8192u;     // map words per block of k_bins_start: four pairs per thread
constexpr uint32_t kBnMergeRounds = 8u;       // merge rounds per wave; a lane still pending after them marks alone
static_assert(RPLGPU_MAX_HEADING_BINS == (uint32_t)kBlock, "one edge per thread");
static_assert(kBnClearWords == 8u * kBlock, "four 8-byte stores per thread");

// E17's rule for one entry of (c, s); false as well for an entry that quantises to (0, 0)
__device__ __forceinline__ bool bn_quantise(float c, float s, int32_t *C, int32_t *S) {
  return es_quantise_cs(c, s, C, S) && (*C != 0 || *S != 0);
}

__device__ __forceinline__ uint32_t bn_half(int32_t C, int32_t S) { return (S > 0 || (S == 0 && C > 0)) ? 0u : 1u; }

// edge e <= heading h in the angular order; (0, 0) stands for an edge that is never <= anything
__device__ __forceinline__ bool bn_le(int2 e, int32_t C, int32_t S) {
  if (e.x == 0 && e.y == 0) return false;
  const uint32_t he = bn_half(e.x, e.y), hh = bn_half(C, S);
  if (he != hh) return he < hh;
  return (i64)e.x * S - (i64)e.y * C >= 0;
}

// the OR over the wave, valid in lane 63 (a lane without a source keeps its own value), then broadcast
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t bn_dpp_or(uint32_t v) {
  return v | (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWMASK, 0xF, false);
}
__device__ __forceinline__ uint32_t bn_wave_or(uint32_t v) {
  v = bn_dpp_or<0x111, 0xF>(v);  // row_shr:1
  v = bn_dpp_or<0x112, 0xF>(v);  // row_shr:2
  v = bn_dpp_or<0x114, 0xF>(v);  // row_shr:4
  v = bn_dpp_or<0x118, 0xF>(v);  // row_shr:8
  v = bn_dpp_or<0x142, 0xA>(v);  // row_bcast:15 -> rows 1,3
  v = bn_dpp_or<0x143, 0xC>(v);  // row_bcast:31 -> rows 2,3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ __launch_bounds__(kBlock) void k_bins_start(uint32_t *__restrict__ map, u64 map_stride, uint32_t words,
                                                       uint32_t keep, uint32_t *__restrict__ result) {
  const uint32_t g = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x < 8u)
    result[8u * (size_t)g + threadIdx.x] = threadIdx.x == 4u ? 0xFFFFFFFFu : threadIdx.x == 7u ? 1u | keep << 2 : 0u;
  if (keep) return;
  uint32_t *grp = map + (size_t)g * map_stride;  // 8-byte aligned: d_map is and map_stride is even
#pragma unroll
  for (uint32_t i = 0; i < 4u; ++i) {
    const uint32_t w = blockIdx.x * kBnClearWords + 2u * (i * kBlock + threadIdx.x);  // below 2^21 + 8192
    if (w + 1u < words)
      *reinterpret_cast<uint2 *>(grp + w) = make_uint2(0u, 0u);
    else if (w < words)
      grp[w] = 0u;  // the last word of an odd count: the word behind it is not the map's
  }
}

__global__ __launch_bounds__(kBlock) void k_bins_mark(
    float origin_x, float origin_y, float inv_size, uint32_t nx, uint32_t ny, const float *__restrict__ poses,
    u64 pose_stride, uint32_t poses_per_group, const uint32_t *__restrict__ weights, u64 weight_stride, uint32_t P,
    const float2 *__restrict__ edges, uint32_t T, uint32_t *__restrict__ map, u64 map_stride,
    uint32_t *__restrict__ bins_out, u64 bin_stride, uint32_t *__restrict__ result) {
  __shared__ int2 s_edge[RPLGPU_MAX_HEADING_BINS];
  __shared__ uint32_t s_part[4][kWaves];
  const uint32_t g = blockIdx.y;
  const uint32_t i = blockIdx.x * kBnTile + threadIdx.x;
  const bool live = i < P;
  if (threadIdx.x < T) {
    const float2 e = edges[threadIdx.x];
    int2 q;
    bn_quantise(e.x, e.y, &q.x, &q.y);  // (0, 0) when out of range
    s_edge[threadIdx.x] = q;
  }
  const es_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const es_f32x4 v =
      live ? reinterpret_cast<const es_f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride)[i] : zero;
  const uint32_t w = live ? (weights ? weights[(size_t)g * weight_stride + i] : 1u) : 0u;
  __syncthreads();
  // the position bin
  const float dx = v.z - origin_x, dy = v.w - origin_y;
  const float fx = dx * inv_size, fy = dy * inv_size;
  const bool pos_in = fx >= 0.0f && fx < (float)nx && fy >= 0.0f && fy < (float)ny;  // NaN: false
  const uint32_t bx = pos_in ? (uint32_t)floorf(fx) : 0u, by = pos_in ? (uint32_t)floorf(fy) : 0u;
  // the heading bin
  int32_t C, S;
  const bool head_in = bn_quantise(v.x, v.y, &C, &S);
  uint32_t lo = 0u, hi = T;
#pragma unroll
  for (uint32_t step = 0; step < 10u; ++step) {
    if (hi - lo > 1u) {
      const uint32_t mid = min((lo + hi) >> 1, T - 1u);
      if (bn_le(s_edge[mid], C, S))
        lo = mid;
      else
        hi = mid;
    }
  }
  const uint32_t nb = nx * ny * T, words = bin_map_words(nb);
  const bool skipped = live && w == 0u;
  const bool counted = live && !skipped && pos_in && head_in;
  const bool outside = live && !skipped && !counted;
  const uint32_t b = min((lo * ny + min(by, ny - 1u)) * nx + min(bx, nx - 1u), nb - 1u);
  if (live && bins_out) bins_out[(size_t)g * bin_stride + i] = counted ? b : 0xFFFFFFFFu;  // i < P <= bin_stride
  // (1) the lanes of the wave that hit the same map word hand their bits to the first of them
  const uint32_t word = min(b >> 5, words - 1u), bit = 1u << (b & 31u);
  u64 pending = __ballot(counted);
  uint32_t mine = 0u;
  for (uint32_t round = 0; round < kBnMergeRounds && pending; ++round) {
    const int first = __ffsll((i64)pending) - 1;
    const uint32_t fw = (uint32_t)__builtin_amdgcn_readlane((int)word, first);
    const bool same = counted && word == fw;
    const uint32_t all = bn_wave_or(same ? bit : 0u);
    if ((int)lane_id() == first) mine = all;
    pending &= ~__ballot(same);
  }
  if ((pending >> lane_id()) & 1ull) mine = bit;  // past the bound a lane marks alone
  // (2), (3)
  uint32_t fresh = 0u;
  if (mine) {
    uint32_t *at = map + (size_t)g * map_stride + word;
    const uint32_t seen = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((seen & mine) != mine) fresh = (uint32_t)__popc(mine & ~atomicOr(at, mine));
  }
  // the tile's statistics; the three counts of a wave are at most 64 each: one byte each
  const uint32_t cnt = wave_incl_scan_fast((counted ? 1u : 0u) | (outside ? 1u << 8 : 0u) | (skipped ? 1u << 16 : 0u));
  const uint32_t t_new = wave_incl_scan_fast(fresh);  // at most 64 * 32
  const uint32_t t_min = wave_min_lane63(counted ? b : 0xFFFFFFFFu);
  const uint32_t t_max = wave_max_lane63(counted ? b : 0u);
  if (lane_id() == 63u) {
    s_part[0][wave_id()] = cnt;
    s_part[1][wave_id()] = t_new;
    s_part[2][wave_id()] = t_min;
    s_part[3][wave_id()] = t_max;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t n_in = 0u, n_out = 0u, n_skip = 0u, k = 0u, bmin = 0xFFFFFFFFu, bmax = 0u;
    for (int q = 0; q < kWaves; ++q) {
      const uint32_t c = s_part[0][q];
      n_in += c & 0xFFu;
      n_out += (c >> 8) & 0xFFu;
      n_skip += (c >> 16) & 0xFFu;
      k += s_part[1][q];
      bmin = min(bmin, s_part[2][q]);
      bmax = max(bmax, s_part[3][q]);
    }
    // the words every tile of the group shares: minimum, maximum and flag are read first (device scope) and left
    // alone when they already say it — a stale read only costs an atomic
    uint32_t *res = result + 8u * (size_t)g;
    if (k) atomicAdd(res + 0, k);
    if (n_in) {
      atomicAdd(res + 1, n_in);
      if (bmin < __hip_atomic_load(res + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(res + 4, bmin);
      if (bmax > __hip_atomic_load(res + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(res + 5, bmax);
      if (__hip_atomic_load(res + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u) atomicAnd(res + 7, ~1u);
    }
    if (n_out) {
      atomicAdd(res + 2, n_out);
      if (!(__hip_atomic_load(res + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2u)) atomicOr(res + 7, 2u);
    }
    if (n_skip) atomicAdd(res + 3, n_skip);
  }
}

}  // namespace

hipError_t launch_bins(hipStream_t s, const BinsK &k, const float *poses, unsigned long long pose_stride,
                       uint32_t poses_per_group, const uint32_t *weights, unsigned long long weight_stride,
                       uint32_t G, uint32_t P, const float *edges, uint32_t T, uint32_t *map,
                       unsigned long long map_stride, uint32_t *bins_out, unsigned long long bin_stride,
                       uint32_t *result) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || T == 0 || T > RPLGPU_MAX_HEADING_BINS ||
      k.nx == 0 || k.nx > 65536u || k.ny == 0 || k.ny > 65536u ||
      (u64)k.nx * k.ny * T > (u64)RPLGPU_MAX_POSE_BINS)
    return hipErrorInvalidValue;
  const uint32_t words = bin_map_words(k.nx * k.ny * T);
  if (pose_stride < 4ull * P || (pose_stride & 3u) || (weights && weight_stride < P) || map_stride < words ||
      (map_stride & 1u) || (bins_out && bin_stride < P))
    return hipErrorInvalidValue;
  const uint32_t clear_blocks = k.keep ? 1u : (words + kBnClearWords - 1u) / kBnClearWords;
  hipLaunchKernelGGL(k_bins_start, dim3(clear_blocks, G), dim3(kBlock), 0, s, map, map_stride, words, k.keep, result);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bins_mark, dim3((P + kBnTile - 1u) / kBnTile, G), dim3(kBlock), 0, s, k.origin_x, k.origin_y,
                     k.inv_size, k.nx, k.ny, poses, pose_stride, poses_per_group, weights, weight_stride, P,
                     reinterpret_cast<const float2 *>(edges), T, map, map_stride, bins_out, bin_stride, result);
  return hipGetLastError();
}

}  // namespace rpl
