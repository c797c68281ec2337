// rpl_wide.hip — E24: a group of scans matched to a likelihood field over a window of up to 256 cells a side by
// bound and refine, include/rplgpu_msg.h, rplgpu_match_wide_dev and rplgpu_pool_field_dev.  The answer is E13's
// (rpl_match.hip) over the wide window; what is scored finely is only the blocks of 8 x 8 shifts whose upper bound,
// read from the pooled field, can still win.
//
//   k_pool_field    P, the 8 x 8 sliding maximum of the clipped field (rows, then columns, in LDS tiles);
//   k_wide_prepare  zeroes every group's bounds volume, result and work words and the head of its scratch;
//   k_wide_bound    k_match_score's shape with shifts of 8 cells and P in place of the field: threads own blocks;
//   k_wide_seed     the greatest bound (seed A) and the block of (0, 0, 0) (seed B) as a two-entry list;
//   k_wide_refine   E13's score for every candidate of the listed blocks of one rotation, one wave per block;
//   k_wide_list     b0 from the seeds' scores, the blocks with U >= b0 counted and, below the cap, listed by rotation;
//   k_wide_best     E13's tie rule over the listed blocks' candidates (the seeds' when the list is above the cap).
//
// k_wide_refine runs twice with the same fixed grid, over the seeds and over the list: the list's length stays on the
// device.  The front end (a sample to its cell, runs of equal cells to one weighted list entry) is k_match_score's:
// rpl_front.hpp's scan_front and front_cell_pass, here with the wide bias and the reach of a block below the window.
//
// A group's scratch, in words (rplgpu_wide_match_scratch_words): [0, 8) counters, [8, 144) the list's first entry per
// rotation, [144, 272) the seeds' 2 x 64 scores, [272, 272 + cap) the list, then 64 score words per list entry.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_front.hpp"
#include "rpl_wide.hpp"

namespace rpl {
namespace {

constexpr int kS = (int)RPLGPU_WIDE_MATCH_BLOCK;
constexpr int kCellBias = 320;  // cell + kCellBias > 0 for every listed cell: an entry is never 0
constexpr int kMaxOwn = 5;      // blocks a thread owns when a rotation has more than kBlock (65 * 65 / 1024)
static_assert(kS == 8, "a block is one wave of candidates: lane = 8 * (j in the block) + (i in the block)");
static_assert(((2u * RPLGPU_MAX_WIDE_SHIFT + kS) / kS) * ((2u * RPLGPU_MAX_WIDE_SHIFT + kS) / kS) <=
                  (uint32_t)kMaxOwn * kBlock, "a rotation's blocks do not fit the registers of a workgroup");
// -(256 + 7) .. 4096 + 255, biased, per axis
static_assert(RPLGPU_MAX_OCC_DIM + RPLGPU_MAX_WIDE_SHIFT + kCellBias <= (1u << kCellBits), "cell bits");
static_assert(RPLGPU_MAX_WIDE_SHIFT + kS - 1 < (uint32_t)kCellBias, "cell bias");

// the scratch of one group, in words
constexpr uint32_t kHdrListed = 0, kHdrSeeds = 1, kHdrSeedAt = 2, kHdrUnproven = 4;
constexpr uint32_t kRotAt = 8, kSeedScoresAt = 144, kListAt = 272;
static_assert(kRotAt + 2u * RPLGPU_MAX_MATCH_ROT + 2u <= kSeedScoresAt, "the first entry per rotation, and the end");

// P(x, y): 0 where P is not defined
__device__ __forceinline__ uint32_t pooled_look(const int8_t *__restrict__ pooled, int x, int y, uint32_t Wp,
                                                uint32_t Hp) {
  const int ax = x + (kS - 1), ay = y + (kS - 1);
  if ((uint32_t)ax >= Wp || (uint32_t)ay >= Hp) return 0u;
  const int v = pooled[(uint32_t)ay * Wp + (uint32_t)ax];
  return (uint32_t)max(v, 0);
}

// ---- the pooled field -------------------------------------------------------------------------------------------------
constexpr int kPoolTile = 32, kPoolIn = kPoolTile + kS - 1, kPoolThreads = 256;

__global__ __launch_bounds__(kPoolThreads) void k_pool_field(const int8_t *__restrict__ field,
                                                             unsigned long long field_stride, uint32_t W, uint32_t H,
                                                             int8_t *__restrict__ pooled,
                                                             unsigned long long pooled_stride) {
  __shared__ int8_t s_in[kPoolIn][kPoolIn + 1];
  __shared__ int8_t s_row[kPoolIn][kPoolTile];
  const int8_t *fld = field + (size_t)blockIdx.z * field_stride;
  int8_t *out = pooled + (size_t)blockIdx.z * pooled_stride;
  const uint32_t Wp = W + (uint32_t)kS - 1u, Hp = H + (uint32_t)kS - 1u;
  const int px0 = (int)blockIdx.x * kPoolTile, py0 = (int)blockIdx.y * kPoolTile;  // the tile's corner in P's grid
  for (int t = (int)threadIdx.x; t < kPoolIn * kPoolIn; t += kPoolThreads) {
    const int ly = t / kPoolIn, lx = t - ly * kPoolIn;
    s_in[ly][lx] = (int8_t)field_look(fld, px0 - (kS - 1) + lx, py0 - (kS - 1) + ly, W, H);
  }
  __syncthreads();
  for (int t = (int)threadIdx.x; t < kPoolIn * kPoolTile; t += kPoolThreads) {
    const int ly = t / kPoolTile, lx = t - ly * kPoolTile;
    int v = 0;
#pragma unroll
    for (int a = 0; a < kS; ++a) v = max(v, (int)s_in[ly][lx + a]);
    s_row[ly][lx] = (int8_t)v;
  }
  __syncthreads();
  for (int t = (int)threadIdx.x; t < kPoolTile * kPoolTile; t += kPoolThreads) {
    const int ly = t / kPoolTile, lx = t - ly * kPoolTile;
    int v = 0;
#pragma unroll
    for (int b = 0; b < kS; ++b) v = max(v, (int)s_row[ly + b][lx]);
    const uint32_t ax = (uint32_t)(px0 + lx), ay = (uint32_t)(py0 + ly);
    if (ax < Wp && ay < Hp) out[(size_t)ay * Wp + ax] = (int8_t)v;
  }
}

// ---- prepare ------------------------------------------------------------------------------------------------------------
constexpr uint32_t kPrepThreads = 256;

__global__ __launch_bounds__(kPrepThreads) void k_wide_prepare(uint32_t *__restrict__ bounds,
                                                               unsigned long long bounds_stride, uint32_t volume,
                                                               uint32_t blocks_per_group, uint32_t *__restrict__ scratch,
                                                               unsigned long long scratch_stride,
                                                               uint32_t *__restrict__ best, uint32_t *__restrict__ work) {
  const uint32_t g = blockIdx.x / blocks_per_group;
  const uint32_t b = blockIdx.x - g * blocks_per_group;
  const uint32_t w = b * kPrepThreads + threadIdx.x;
  if (w < volume) bounds[(size_t)g * bounds_stride + w] = 0u;
  if (b != 0) return;
  if (threadIdx.x < 8u) {
    best[8u * g + threadIdx.x] = 0u;
    work[8u * g + threadIdx.x] = 0u;
  }
  for (uint32_t t = threadIdx.x; t < kListAt; t += kPrepThreads) scratch[(size_t)g * scratch_stride + t] = 0u;
}

// ---- bound --------------------------------------------------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_wide_bound(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan, uint32_t group,
    KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, const float *__restrict__ pivot, WideK wk,
    MatchRot rot, const int8_t *__restrict__ pooled, unsigned long long pooled_stride, uint32_t field_per_group,
    uint32_t *__restrict__ bounds, unsigned long long bounds_stride, uint32_t *__restrict__ best,
    uint32_t *__restrict__ status) {
  __shared__ uint32_t s_list[kFrontList];
  __shared__ uint32_t s_sum[kBlock];
  __shared__ uint32_t s_cnt[2];  // the list's length, by the pass's parity: a reset never meets a late reader
  const MatchK &k = wk.k;
  const uint32_t sc = blockIdx.x;
  const uint32_t kk = blockIdx.y;  // k + K
  const uint32_t g = sc / group;
  const uint32_t n_in = n_per_scan[sc];
  const uint32_t n = scan_len(n_in, n_stride);
  const bool first_of_scan = kk == 0u && blockIdx.z == 0u;
  if (threadIdx.x == 0 && status && first_of_scan && n_in > n) atomicOr(&status[g], RPLGPU_SCAN_OUT_TRUNCATED);
  if (blockIdx.z * kFrontList >= n) return;  // (block-uniform)
  const ScanFront f = scan_front(nodes, n_stride, sc, n, p, T, keepmask, mask_stride, motion, pose2d);
  const CellRot cr = cell_rot(rot, kk, pivot, g);
  const int8_t *pl = pooled + (size_t)(field_per_group ? g : 0u) * pooled_stride;
  const uint32_t Wp = k.width + (uint32_t)kS - 1u, Hp = k.height + (uint32_t)kS - 1u;
  // the blocks of this thread: position c = bj * nbx + bi in the rotation, copy `slice` of `slices`
  const uint32_t nbx = wk.nbx, nb = nbx * wk.nby;
  const uint32_t per = min((nb + 63u) & ~63u, (uint32_t)kBlock);  // threads of one copy of the rotation's blocks
  const uint32_t slices = nb <= (uint32_t)kBlock ? (uint32_t)kBlock / per : 1u;
  const uint32_t slice = threadIdx.x / per, c0 = threadIdx.x - slice * per;
  int di[kMaxOwn], dj[kMaxOwn];
  bool own[kMaxOwn];
  uint32_t acc[kMaxOwn];
#pragma unroll
  for (int r = 0; r < kMaxOwn; ++r) {
    const uint32_t c = c0 + (uint32_t)r * kBlock;
    own[r] = slice < slices && c < nb && (r == 0 || nb > (uint32_t)kBlock);
    di[r] = (int)(c % nbx) * kS - (int)k.tx;
    dj[r] = (int)(c / nbx) * kS - (int)k.ty;
    acc[r] = 0u;
  }
  const bool wide = nb > (uint32_t)kBlock;  // (block-uniform)
  uint32_t finite = 0u;
  bool cell_range = false;
  uint32_t pass = 0u;
  for (uint32_t base = blockIdx.z * kFrontList; base < n; base += gridDim.z * kFrontList) {
    uint32_t *cnt_at = &s_cnt[pass++ & 1u];
    // (a cell up to kS - 1 below the window is still in the reach of a block's look-up into P, and that look-up
    // covers the look-ups of the block's candidates into the field)
    front_cell_pass<FAST, kCellBias, kS - 1>(f, base, p, k, cr, s_list, cnt_at, &finite, &cell_range);
    const uint32_t cnt = *cnt_at;  // <= kFrontList
    if (!wide) {
      if (own[0]) {
#pragma unroll 4
        for (uint32_t e = slice; e < cnt; e += slices) {
          const uint32_t w = s_list[e];
          const int cx = (int)(w & kCellMask) - kCellBias, cy = (int)((w >> kCellBits) & kCellMask) - kCellBias;
          acc[0] += ((w >> (2u * kCellBits)) + 1u) * pooled_look(pl, cx + di[0], cy + dj[0], Wp, Hp);
        }
      }
    } else {
      for (uint32_t e = 0; e < cnt; ++e) {
        const uint32_t w = s_list[e];
        const int cx = (int)(w & kCellMask) - kCellBias, cy = (int)((w >> kCellBits) & kCellMask) - kCellBias;
        const uint32_t wt = (w >> (2u * kCellBits)) + 1u;
#pragma unroll
        for (int r = 0; r < kMaxOwn; ++r)
          if (own[r]) acc[r] += wt * pooled_look(pl, cx + di[r], cy + dj[r], Wp, Hp);
      }
    }
  }
  if (status && __any(cell_range) && lane_id() == 0) atomicOr(&status[g], RPLGPU_SCAN_CELL_RANGE);
  if (kk == 0u) {  // word 4, the group's finite points: once per sample, by the workgroups of the first rotation
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) finite += __shfl_xor(finite, d, 64);
    if (lane_id() == 0 && finite) atomicAdd(&best[8u * g + 4u], finite);
  }
  uint32_t *vol = bounds + (size_t)g * bounds_stride + (size_t)kk * nb;
  if (wide) {
#pragma unroll
    for (int r = 0; r < kMaxOwn; ++r)
      if (own[r] && acc[r]) atomicAdd(&vol[c0 + (uint32_t)r * kBlock], acc[r]);
    return;
  }
  __syncthreads();
  s_sum[threadIdx.x] = own[0] ? acc[0] : 0u;  // copy `slice` at [slice * per, slice * per + per)
  __syncthreads();
  if (threadIdx.x < nb) {
    uint32_t sum = 0u;
    for (uint32_t s = 0; s < slices; ++s) sum += s_sum[s * per + threadIdx.x];
    if (sum) atomicAdd(&vol[threadIdx.x], sum);
  }
}

// ---- reductions over a workgroup of kBlock threads ----------------------------------------------------------------------
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long *s_tmp) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  __syncthreads();  // (the last reduction's readers are done with s_tmp)
  if (lane_id() == 0) s_tmp[wave_id()] = v;
  __syncthreads();
  v = s_tmp[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) v = s_tmp[w] > v ? s_tmp[w] : v;
  return v;
}

__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, unsigned long long *s_tmp) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if (lane_id() == 0) s_tmp[wave_id()] = v;
  __syncthreads();
  uint32_t sum = 0u;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) sum += (uint32_t)s_tmp[w];
  return sum;
}

// ---- the seeds ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_wide_seed(const uint32_t *__restrict__ bounds,
                                                      unsigned long long bounds_stride, WideK wk,
                                                      uint32_t *__restrict__ scratch,
                                                      unsigned long long scratch_stride, uint32_t *__restrict__ work) {
  __shared__ unsigned long long s_tmp[kWaves];
  const uint32_t g = blockIdx.x;
  const uint32_t *U = bounds + (size_t)g * bounds_stride;
  const uint32_t nb = wk.nbx * wk.nby, blocks = nb * (2u * wk.k.rot + 1u);
  // the greatest (U, ~flat index): among equal bounds the lowest index
  unsigned long long key = 0ull;
  for (uint32_t v = threadIdx.x; v < blocks; v += kBlock) {
    const unsigned long long cand = ((unsigned long long)U[v] << 32) | (uint32_t)~v;
    key = cand > key ? cand : key;
  }
  key = block_max_u64(key, s_tmp);
  if (threadIdx.x != 0) return;
  const uint32_t seed_a = ~(uint32_t)key;
  const uint32_t seed_b = (wk.k.rot * wk.nby + wk.k.ty / (uint32_t)kS) * wk.nbx + wk.k.tx / (uint32_t)kS;
  uint32_t *sg = scratch + (size_t)g * scratch_stride;
  sg[kHdrSeeds] = seed_a == seed_b ? 1u : 2u;
  sg[kHdrSeedAt] = seed_a;
  sg[kHdrSeedAt + 1u] = seed_b;
  work[8u * g + 0u] = blocks;
  work[8u * g + 1u] = (uint32_t)(key >> 32);
  work[8u * g + 2u] = seed_a;
  work[8u * g + 5u] = wk.max_blocks;
}

// the candidate `lane` of block v: false when it lies outside the window
__device__ __forceinline__ bool wide_candidate(const WideK &wk, uint32_t v, uint32_t lane, int *kr, int *j, int *i) {
  const uint32_t nb = wk.nbx * wk.nby, kk = v / nb, c = v - kk * nb;
  *kr = (int)kk - (int)wk.k.rot;
  *i = (int)(c % wk.nbx) * kS - (int)wk.k.tx + (int)(lane & 7u);
  *j = (int)(c / wk.nbx) * kS - (int)wk.k.ty + (int)(lane >> 3);
  return *i <= (int)wk.k.tx && *j <= (int)wk.k.ty;
}

// ---- refine ---------------------------------------------------------------------------------------------------------------
// seeds != 0: the entries are the group's one or two seeds and their scores go to the seeds' 128 words; else the
// entries are the list's of this rotation.  Entry e's candidate `lane` has its score at 64 e + lane.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_wide_refine(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan, uint32_t group,
    KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, const float *__restrict__ pivot, WideK wk,
    MatchRot rot, const int8_t *__restrict__ field, unsigned long long field_stride, uint32_t field_per_group,
    uint32_t *__restrict__ scratch, unsigned long long scratch_stride, uint32_t seeds) {
  __shared__ uint32_t s_list[kFrontList];
  __shared__ uint32_t s_cnt[2];
  const MatchK &k = wk.k;
  const uint32_t sc = blockIdx.x;
  const uint32_t kk = blockIdx.y;  // k + K
  const uint32_t g = sc / group;
  const uint32_t n = scan_len(n_per_scan[sc], n_stride);
  if (blockIdx.z * kFrontList >= n) return;  // (block-uniform)
  uint32_t *sg = scratch + (size_t)g * scratch_stride;
  const uint32_t nb = wk.nbx * wk.nby;
  // the entries [e0, e1) of this workgroup's rotation (block-uniform)
  uint32_t e0, e1;
  const uint32_t *list;
  uint32_t *scores;
  if (seeds) {
    const uint32_t ns = min(sg[kHdrSeeds], 2u);
    list = sg + kHdrSeedAt;
    scores = sg + kSeedScoresAt;
    e0 = 0u;
    e1 = ns;
    bool mine = false;
    for (uint32_t e = 0; e < ns; ++e) mine = mine || list[e] / nb == kk;
    if (!mine) return;
  } else {
    const uint32_t listed = min(sg[kHdrListed], wk.max_blocks);
    list = sg + kListAt;
    scores = sg + kListAt + wk.max_blocks;
    e0 = min(sg[kRotAt + kk], listed);
    e1 = min(sg[kRotAt + kk + 1u], listed);
    if (e0 >= e1) return;
  }
  const ScanFront f = scan_front(nodes, n_stride, sc, n, p, T, keepmask, mask_stride, motion, pose2d);
  const CellRot cr = cell_rot(rot, kk, pivot, g);
  const int8_t *fld = field + (size_t)(field_per_group ? g : 0u) * field_stride;
  const uint32_t W = k.width, H = k.height;
  uint32_t finite = 0u;  // (the bound kernel has counted them)
  bool cell_range = false;
  uint32_t pass = 0u;
  for (uint32_t base = blockIdx.z * kFrontList; base < n; base += gridDim.z * kFrontList) {
    uint32_t *cnt_at = &s_cnt[pass++ & 1u];
    // (a cell up to kS - 1 below the window is still in the reach of a block's look-up into P, and that look-up
    // covers the look-ups of the block's candidates into the field)
    front_cell_pass<FAST, kCellBias, kS - 1>(f, base, p, k, cr, s_list, cnt_at, &finite, &cell_range);
    const uint32_t cnt = *cnt_at;  // <= kFrontList
    for (uint32_t e = e0 + wave_id(); e < e1; e += (uint32_t)kWaves) {  // one wave per block of 64 candidates
      const uint32_t v = list[e];
      if (v / nb != kk) continue;  // (a seed of another rotation; wave-uniform)
      int kr, j, i;
      if (!wide_candidate(wk, v, lane_id(), &kr, &j, &i)) continue;  // the last block of an axis is partial
      uint32_t acc = 0u;
#pragma unroll 4
      for (uint32_t q = 0; q < cnt; ++q) {
        const uint32_t w = s_list[q];
        const int cx = (int)(w & kCellMask) - kCellBias, cy = (int)((w >> kCellBits) & kCellMask) - kCellBias;
        acc += ((w >> (2u * kCellBits)) + 1u) * field_look(fld, cx + i, cy + j, W, H);
      }
      if (acc) atomicAdd(&scores[(size_t)e * 64u + lane_id()], acc);
    }
  }
}

// ---- the list ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_wide_list(const uint32_t *__restrict__ bounds,
                                                      unsigned long long bounds_stride, WideK wk,
                                                      uint32_t *__restrict__ scratch,
                                                      unsigned long long scratch_stride, uint32_t *__restrict__ work) {
  __shared__ unsigned long long s_tmp[kWaves];
  __shared__ uint32_t s_cnt[2u * RPLGPU_MAX_MATCH_ROT + 2u];  // per rotation: the count, then the next free place
  __shared__ uint32_t s_n;
  const uint32_t g = blockIdx.x;
  const uint32_t *U = bounds + (size_t)g * bounds_stride;
  uint32_t *sg = scratch + (size_t)g * scratch_stride;
  const uint32_t rots = 2u * wk.k.rot + 1u, nb = wk.nbx * wk.nby, blocks = nb * rots, cap = wk.max_blocks;
  // b0: the greatest score over the in-window candidates of the seeds
  const uint32_t ns = min(sg[kHdrSeeds], 2u);
  unsigned long long mine = 0ull;
  if (threadIdx.x < 64u * ns) {
    int kr, j, i;
    if (wide_candidate(wk, sg[kHdrSeedAt + threadIdx.x / 64u], threadIdx.x & 63u, &kr, &j, &i))
      mine = sg[kSeedScoresAt + threadIdx.x];
  }
  const uint32_t b0 = (uint32_t)block_max_u64(mine, s_tmp);
  for (uint32_t t = threadIdx.x; t < rots + 1u; t += kBlock) s_cnt[t] = 0u;
  __syncthreads();
  for (uint32_t v = threadIdx.x; v < blocks; v += kBlock)
    if (U[v] >= b0) atomicAdd(&s_cnt[v / nb], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {  // counts to first places (at most 129 of them), the total behind the last
    uint32_t at = 0u;
    for (uint32_t r = 0; r < rots; ++r) {
      const uint32_t c = s_cnt[r];
      s_cnt[r] = at;
      at += c;
    }
    s_cnt[rots] = at;
    s_n = at;
  }
  __syncthreads();
  const uint32_t n = s_n;
  const bool proven = n <= cap;
  if (threadIdx.x == 0) {
    work[8u * g + 3u] = b0;
    work[8u * g + 4u] = n;
    sg[kHdrListed] = proven ? n : 0u;
    sg[kHdrUnproven] = proven ? 0u : 1u;
  }
  // the first entry of every rotation, and the end; all 0 when nothing is listed
  for (uint32_t t = threadIdx.x; t < rots + 1u; t += kBlock) sg[kRotAt + t] = proven ? s_cnt[t] : 0u;
  if (!proven) return;  // (block-uniform) nothing beyond the seeds is scored, and nothing beyond the cap is written
  __syncthreads();      // (the first places are in the scratch before they start to move)
  for (uint32_t v = threadIdx.x; v < blocks; v += kBlock)
    if (U[v] >= b0) {
      const uint32_t at = atomicAdd(&s_cnt[v / nb], 1u);
      if (at < cap) sg[kListAt + at] = v;
    }
  uint32_t *scores = sg + kListAt + cap;
  for (size_t w = threadIdx.x; w < (size_t)n * 64u; w += kBlock) scores[w] = 0u;
}

// ---- the best ---------------------------------------------------------------------------------------------------------------
// The tie rule as one number, smaller is better: i*i + j*j (18 bits), |k| (7), k > 0 (1), j + Ty (10), i > 0 (1).
// With i*i + j*j and j equal two candidates differ in the sign of i alone, so one bit orders i.
__device__ __forceinline__ unsigned long long wide_penalty(int kr, int j, int i, uint32_t ty) {
  return ((unsigned long long)(uint32_t)(i * i + j * j) << 19) | ((unsigned long long)(uint32_t)abs(kr) << 12) |
         ((kr > 0 ? 1ull : 0ull) << 11) | ((unsigned long long)(uint32_t)(j + (int)ty) << 1) | (i > 0 ? 1ull : 0ull);
}

__global__ __launch_bounds__(kBlock) void k_wide_best(WideK wk, const uint32_t *__restrict__ scratch,
                                                      unsigned long long scratch_stride, uint32_t *__restrict__ best) {
  __shared__ unsigned long long s_tmp[kWaves];
  const uint32_t g = blockIdx.x;
  const uint32_t *sg = scratch + (size_t)g * scratch_stride;
  const uint32_t ns = min(sg[kHdrSeeds], 2u);
  const bool unproven = sg[kHdrUnproven] != 0u;
  const uint32_t entries = unproven ? ns : min(sg[kHdrListed], wk.max_blocks);
  const uint32_t *list = unproven ? sg + kHdrSeedAt : sg + kListAt;
  const uint32_t *scores = unproven ? sg + kSeedScoresAt : sg + kListAt + wk.max_blocks;
  const size_t total = (size_t)entries * 64u;
  // first pass: the best score
  unsigned long long mine = 0ull;
  for (size_t w = threadIdx.x; w < total; w += kBlock) {
    int kr, j, i;
    if (!wide_candidate(wk, list[w >> 6], (uint32_t)w & 63u, &kr, &j, &i)) continue;
    const unsigned long long sc = scores[w];
    mine = sc > mine ? sc : mine;
  }
  const uint32_t top = (uint32_t)block_max_u64(mine, s_tmp);
  // second pass: how many candidates have it, and which of them the tie rule picks
  uint32_t eq = 0u;
  unsigned long long pen = ~0ull;
  int bk = 0, bj = 0, bi = 0;
  for (size_t w = threadIdx.x; w < total; w += kBlock) {
    int kr, j, i;
    if (!wide_candidate(wk, list[w >> 6], (uint32_t)w & 63u, &kr, &j, &i)) continue;
    if (scores[w] != top) continue;
    ++eq;
    const unsigned long long q = wide_penalty(kr, j, i, wk.k.ty);
    if (q < pen) {
      pen = q;
      bk = kr;
      bj = j;
      bi = i;
    }
  }
  const unsigned long long least = ~block_max_u64(~pen, s_tmp);
  if (pen == least && pen != ~0ull) {  // (penalties are distinct: one thread)
    best[8u * g + 0u] = top;
    best[8u * g + 1u] = (uint32_t)bk;
    best[8u * g + 2u] = (uint32_t)bj;
    best[8u * g + 3u] = (uint32_t)bi;
  }
  const uint32_t sum = block_sum_u32(eq, s_tmp);
  if (threadIdx.x == 0) {
    // (0, 0, 0) is a candidate of seed B, the last seed
    const uint32_t lane0 = (wk.k.ty % (uint32_t)kS) * (uint32_t)kS + wk.k.tx % (uint32_t)kS;
    best[8u * g + 5u] = ns ? sg[kSeedScoresAt + (ns - 1u) * 64u + lane0] : 0u;
    best[8u * g + 6u] = sum;
    best[8u * g + 7u] = unproven ? RPLGPU_WIDE_MATCH_UNPROVEN : 0u;
  }
}

bool wide_args_ok(const WideK &wk) {
  const MatchK &k = wk.k;
  const uint32_t s = RPLGPU_WIDE_MATCH_BLOCK;
  return k.width != 0 && k.height != 0 && k.width <= RPLGPU_MAX_OCC_DIM && k.height <= RPLGPU_MAX_OCC_DIM &&
         k.tx <= RPLGPU_MAX_WIDE_SHIFT && k.ty <= RPLGPU_MAX_WIDE_SHIFT && k.rot <= RPLGPU_MAX_MATCH_ROT &&
         wk.nbx == (2u * k.tx + s) / s && wk.nby == (2u * k.ty + s) / s && wk.max_blocks != 0 &&
         wk.max_blocks <= RPLGPU_MAX_WIDE_BLOCKS;
}

}  // namespace

uint32_t wide_blocks(const WideK &wk) { return (2u * wk.k.rot + 1u) * wk.nby * wk.nbx; }
unsigned long long wide_scratch_words(const WideK &wk) { return (unsigned long long)kListAt + 65ull * wk.max_blocks; }

hipError_t launch_pool_field(hipStream_t s, const int8_t *field, unsigned long long field_stride, uint32_t F,
                             uint32_t width, uint32_t height, int8_t *pooled, unsigned long long pooled_stride) {
  if (F == 0) return hipSuccess;
  const uint32_t Wp = width + RPLGPU_WIDE_MATCH_BLOCK - 1u, Hp = height + RPLGPU_WIDE_MATCH_BLOCK - 1u;
  if (width == 0 || height == 0 || width > RPLGPU_MAX_OCC_DIM || height > RPLGPU_MAX_OCC_DIM || F > 65535u ||
      field_stride < (unsigned long long)width * height || pooled_stride < (unsigned long long)Wp * Hp)
    return hipErrorInvalidValue;
  const dim3 grid((Wp + kPoolTile - 1u) / kPoolTile, (Hp + kPoolTile - 1u) / kPoolTile, F);
  hipLaunchKernelGGL(k_pool_field, grid, dim3(kPoolThreads), 0, s, field, field_stride, width, height, pooled,
                     pooled_stride);
  return hipGetLastError();
}

hipError_t launch_wide_prepare(hipStream_t s, uint32_t *bounds, unsigned long long bounds_stride, uint32_t G,
                               const WideK &wk, uint32_t *scratch, uint32_t *best, uint32_t *work) {
  if (G == 0) return hipSuccess;
  if (!wide_args_ok(wk) || bounds_stride < wide_blocks(wk)) return hipErrorInvalidValue;
  const uint64_t bpg = ((uint64_t)wide_blocks(wk) + kPrepThreads - 1u) / kPrepThreads;
  if ((uint64_t)G * bpg > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wide_prepare, dim3((uint32_t)(G * bpg)), dim3(kPrepThreads), 0, s, bounds, bounds_stride,
                     wide_blocks(wk), (uint32_t)bpg, scratch, wide_scratch_words(wk), best, work);
  return hipGetLastError();
}

namespace {
dim3 wide_scan_grid(uint32_t B, uint32_t n_stride, const WideK &wk) {
  // slices of a scan's passes, as launch_match_score
  const uint32_t passes = (min(n_stride, kMaxN) + kFrontList - 1u) / kFrontList;
  return dim3(B, 2u * wk.k.rot + 1u, min(passes, 8u));
}
}  // namespace

hipError_t launch_wide_bound(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                             uint32_t B, uint32_t group, const KParams &p, const Tables &T, const uint32_t *keepmask,
                             uint32_t mask_stride, const float *motion, const float *pose2d, const float *pivot,
                             const WideK &wk, const MatchRot &rot, const int8_t *pooled,
                             unsigned long long pooled_stride, uint32_t field_per_group, uint32_t *bounds,
                             unsigned long long bounds_stride, uint32_t *best, uint32_t *status) {
  if (B == 0) return hipSuccess;
  const unsigned long long pcells = (unsigned long long)(wk.k.width + RPLGPU_WIDE_MATCH_BLOCK - 1u) *
                                    (wk.k.height + RPLGPU_WIDE_MATCH_BLOCK - 1u);
  if (group == 0 || !wide_args_ok(wk) || pooled_stride < pcells || bounds_stride < wide_blocks(wk))
    return hipErrorInvalidValue;
  const dim3 grid = wide_scan_grid(B, n_stride, wk);
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_wide_bound<true>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, pivot, wk, rot, pooled, pooled_stride,
                       field_per_group, bounds, bounds_stride, best, status);
  else
    hipLaunchKernelGGL(k_wide_bound<false>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, pivot, wk, rot, pooled, pooled_stride,
                       field_per_group, bounds, bounds_stride, best, status);
  return hipGetLastError();
}

hipError_t launch_wide_seed(hipStream_t s, const uint32_t *bounds, unsigned long long bounds_stride, uint32_t G,
                            const WideK &wk, uint32_t *scratch, uint32_t *work) {
  if (G == 0) return hipSuccess;
  if (!wide_args_ok(wk) || bounds_stride < wide_blocks(wk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wide_seed, dim3(G), dim3(kBlock), 0, s, bounds, bounds_stride, wk, scratch,
                     wide_scratch_words(wk), work);
  return hipGetLastError();
}

hipError_t launch_wide_refine(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                              uint32_t B, uint32_t group, const KParams &p, const Tables &T, const uint32_t *keepmask,
                              uint32_t mask_stride, const float *motion, const float *pose2d, const float *pivot,
                              const WideK &wk, const MatchRot &rot, const int8_t *field,
                              unsigned long long field_stride, uint32_t field_per_group, uint32_t *scratch,
                              uint32_t seeds) {
  if (B == 0) return hipSuccess;
  if (group == 0 || !wide_args_ok(wk) || field_stride < (unsigned long long)wk.k.width * wk.k.height)
    return hipErrorInvalidValue;
  const dim3 grid = wide_scan_grid(B, n_stride, wk);
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_wide_refine<true>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, pivot, wk, rot, field, field_stride,
                       field_per_group, scratch, wide_scratch_words(wk), seeds);
  else
    hipLaunchKernelGGL(k_wide_refine<false>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, pivot, wk, rot, field, field_stride,
                       field_per_group, scratch, wide_scratch_words(wk), seeds);
  return hipGetLastError();
}

hipError_t launch_wide_list(hipStream_t s, const uint32_t *bounds, unsigned long long bounds_stride, uint32_t G,
                            const WideK &wk, uint32_t *scratch, uint32_t *work) {
  if (G == 0) return hipSuccess;
  if (!wide_args_ok(wk) || bounds_stride < wide_blocks(wk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wide_list, dim3(G), dim3(kBlock), 0, s, bounds, bounds_stride, wk, scratch,
                     wide_scratch_words(wk), work);
  return hipGetLastError();
}

hipError_t launch_wide_best(hipStream_t s, uint32_t G, const WideK &wk, const uint32_t *scratch, uint32_t *best) {
  if (G == 0) return hipSuccess;
  if (!wide_args_ok(wk)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wide_best, dim3(G), dim3(kBlock), 0, s, wk, scratch, wide_scratch_words(wk), best);
  return hipGetLastError();
}

}  // namespace rpl
