// rpl_match.hip — E13: correlative scan matching of a group of scans (the sensors of one time step) against a
// likelihood field, include/rplgpu_msg.h, rplgpu_match_scans_dev: the group's points are laid over the field at
// every pose of a search window (2K+1 rotations about a pivot x (2Ty+1) x (2Tx+1) whole-cell shifts), the field
// values under them are added up per pose and the best pose is kept.
//
// The score volume is the call's own scratch, three launches and nothing on the handle:
//   k_match_prepare  zeroes every group's volume and its eight result words;
//   k_match_score    adds the field values under the points into the volume;
//   k_match_best     reduces a group's volume to its eight result words.
//
// k_match_score: one 1024-thread workgroup per (scan, rotation, slice of the scan's 2048-sample passes), the
// front end of rpl_front.hpp (scan_front, front_cell_pass: two nodes per bounds-checked buffer_load_dwordx4, E1 / E5
// keep bits, the (cos, sin) table, rpl_xf.hpp's sample_xy), so a point lands where E8, E9 and E11 put it, bit for
// bit.  Per 2048 samples (the first two steps are front_cell_pass, the look-up is rpl_grid.hpp's field_look):
//   * a sample becomes a CELL: the E11 cell of its rotated position.  A cell farther than the window from the
//     grid scores nothing at any shift and is dropped; the others fit 13 bits per axis.
//   * consecutive samples of a wave half that land in one cell (a wall's neighbours) become ONE list entry with
//     a weight of up to 64: the run lengths come from two ballots, no scan.  The entries are compacted into an
//     LDS list (one atomic per wave).
//   * then the threads own candidates, not points: the (j, i) shifts are laid out flat, i fastest, over
//     consecutive threads, so a wave's look-ups of one entry are consecutive bytes of one or two field rows.  A
//     window of up to 1024 candidates is repeated over the workgroup as often as it fits and each copy walks its
//     share of the list; a larger one gives every thread up to kMaxOwn candidates in registers.
//   * the copies are added up through LDS and leave with one no-return atomic add per candidate.
// All integers behind the cell rule: the volume depends on no order.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_front.hpp"

namespace rpl {
namespace {

constexpr int kCellBias = 64;  // cell + kCellBias >= 32 for every listed cell: an entry is never 0
constexpr int kMaxOwn = 5;     // candidates a thread owns when the window is above kBlock (65 * 65 / 1024)
static_assert((2u * RPLGPU_MAX_MATCH_SHIFT + 1u) * (2u * RPLGPU_MAX_MATCH_SHIFT + 1u) <= (uint32_t)kMaxOwn * kBlock,
              "the window does not fit the registers of a workgroup");
// -32 .. 4096 + 31, biased, per axis
static_assert(RPLGPU_MAX_OCC_DIM + RPLGPU_MAX_MATCH_SHIFT + kCellBias <= (1u << kCellBits), "cell bits");
static_assert(RPLGPU_MAX_MATCH_SHIFT <= (uint32_t)kCellBias / 2u, "cell bias");

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_match_score(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan, uint32_t group,
    KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, const float *__restrict__ pivot, MatchK k,
    MatchRot rot, const int8_t *__restrict__ field, unsigned long long field_stride, uint32_t field_per_group,
    uint32_t *__restrict__ scores, unsigned long long score_stride, uint32_t *__restrict__ best,
    uint32_t *__restrict__ status) {
  __shared__ uint32_t s_list[kFrontList];
  __shared__ uint32_t s_sum[kBlock];
  __shared__ uint32_t s_cnt[2];  // the list's length, by the pass's parity: a reset never meets a late reader
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
  const int8_t *fld = field + (size_t)(field_per_group ? g : 0u) * field_stride;
  const uint32_t W = k.width, H = k.height;
  // the candidates of this thread: window position c = (j + Ty) * nx + (i + Tx), copy `slice` of `slices`
  const uint32_t nx = 2u * k.tx + 1u, nc = nx * (2u * k.ty + 1u);
  const uint32_t per = min((nc + 63u) & ~63u, (uint32_t)kBlock);  // threads of one copy of the window
  const uint32_t slices = nc <= (uint32_t)kBlock ? (uint32_t)kBlock / per : 1u;
  const uint32_t slice = threadIdx.x / per, c0 = threadIdx.x - slice * per;
  int di[kMaxOwn], dj[kMaxOwn];
  bool own[kMaxOwn];
  uint32_t acc[kMaxOwn];
#pragma unroll
  for (int r = 0; r < kMaxOwn; ++r) {
    const uint32_t c = c0 + (uint32_t)r * kBlock;
    own[r] = slice < slices && c < nc && (r == 0 || nc > (uint32_t)kBlock);
    di[r] = (int)(c % nx) - (int)k.tx;
    dj[r] = (int)(c / nx) - (int)k.ty;
    acc[r] = 0u;
  }
  const bool wide = nc > (uint32_t)kBlock;  // (block-uniform)
  uint32_t finite = 0u;
  bool cell_range = false;
  uint32_t pass = 0u;
  for (uint32_t base = blockIdx.z * kFrontList; base < n; base += gridDim.z * kFrontList) {
    uint32_t *cnt_at = &s_cnt[pass++ & 1u];
    front_cell_pass<FAST, kCellBias, 0>(f, base, p, k, cr, s_list, cnt_at, &finite, &cell_range);
    const uint32_t cnt = *cnt_at;  // <= kFrontList
    if (!wide) {
      if (own[0]) {
#pragma unroll 4
        for (uint32_t e = slice; e < cnt; e += slices) {
          const uint32_t w = s_list[e];
          const int cx = (int)(w & kCellMask) - kCellBias, cy = (int)((w >> kCellBits) & kCellMask) - kCellBias;
          acc[0] += ((w >> (2u * kCellBits)) + 1u) * field_look(fld, cx + di[0], cy + dj[0], W, H);
        }
      }
    } else {
      for (uint32_t e = 0; e < cnt; ++e) {
        const uint32_t w = s_list[e];
        const int cx = (int)(w & kCellMask) - kCellBias, cy = (int)((w >> kCellBits) & kCellMask) - kCellBias;
        const uint32_t wt = (w >> (2u * kCellBits)) + 1u;
#pragma unroll
        for (int r = 0; r < kMaxOwn; ++r)
          if (own[r]) acc[r] += wt * field_look(fld, cx + di[r], cy + dj[r], W, H);
      }
    }
  }
  if (status && __any(cell_range) && lane_id() == 0) atomicOr(&status[g], RPLGPU_SCAN_CELL_RANGE);
  if (kk == 0u) {  // word 4, the group's finite points: once per sample, by the workgroups of the first rotation
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) finite += __shfl_xor(finite, d, 64);
    if (lane_id() == 0 && finite) atomicAdd(&best[8u * g + 4u], finite);
  }
  uint32_t *vol = scores + (size_t)g * score_stride + (size_t)kk * nc;
  if (wide) {
#pragma unroll
    for (int r = 0; r < kMaxOwn; ++r)
      if (own[r] && acc[r]) atomicAdd(&vol[c0 + (uint32_t)r * kBlock], acc[r]);
    return;
  }
  __syncthreads();
  s_sum[threadIdx.x] = own[0] ? acc[0] : 0u;  // copy `slice` at [slice * per, slice * per + per)
  __syncthreads();
  if (threadIdx.x < nc) {
    uint32_t sum = 0u;
    for (uint32_t s = 0; s < slices; ++s) sum += s_sum[s * per + threadIdx.x];
    if (sum) atomicAdd(&vol[threadIdx.x], sum);
  }
}

constexpr uint32_t kPrepThreads = 256;

__global__ __launch_bounds__(kPrepThreads) void k_match_prepare(uint32_t *__restrict__ scores,
                                                                unsigned long long score_stride, uint32_t volume,
                                                                uint32_t blocks_per_group,
                                                                uint32_t *__restrict__ best) {
  const uint32_t g = blockIdx.x / blocks_per_group;
  const uint32_t b = blockIdx.x - g * blocks_per_group;
  const uint32_t w = b * kPrepThreads + threadIdx.x;
  if (w < volume) scores[(size_t)g * score_stride + w] = 0u;
  if (b == 0 && threadIdx.x < 8u) best[8u * g + threadIdx.x] = 0u;
}

// The tie rule as one number, smaller is better: i*i + j*j (12 bits), |k| (7), k > 0 (1), j + Ty (7), i > 0 (1).
// With i*i + j*j and j equal two candidates differ in the sign of i alone, so one bit orders i.
__device__ __forceinline__ uint32_t match_penalty(int kr, int j, int i, uint32_t ty) {
  return ((uint32_t)(i * i + j * j) << 16) | ((uint32_t)abs(kr) << 9) | ((kr > 0 ? 1u : 0u) << 8) |
         ((uint32_t)(j + (int)ty) << 1) | (i > 0 ? 1u : 0u);
}

__global__ __launch_bounds__(kBlock) void k_match_best(const uint32_t *__restrict__ scores,
                                                       unsigned long long score_stride, MatchK k,
                                                       uint32_t *__restrict__ best) {
  __shared__ unsigned long long s_key[kWaves];
  __shared__ uint32_t s_eq[kWaves];
  const uint32_t g = blockIdx.x;
  const uint32_t *vol = scores + (size_t)g * score_stride;
  const uint32_t nx = 2u * k.tx + 1u, ny = 2u * k.ty + 1u, nc = nx * ny, volume = nc * (2u * k.rot + 1u);
  // the largest (score, ~penalty): the score in the high word, the tie rule below it
  unsigned long long key = 0ull;
  for (uint32_t v = threadIdx.x; v < volume; v += kBlock) {
    const uint32_t kk = v / nc, c = v - kk * nc;
    const int kr = (int)kk - (int)k.rot, j = (int)(c / nx) - (int)k.ty, i = (int)(c % nx) - (int)k.tx;
    const unsigned long long cand = ((unsigned long long)vol[v] << 32) | (uint32_t)~match_penalty(kr, j, i, k.ty);
    key = cand > key ? cand : key;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d, 64);
    key = o > key ? o : key;
  }
  if (lane_id() == 0) s_key[wave_id()] = key;
  __syncthreads();
  key = s_key[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) key = s_key[w] > key ? s_key[w] : key;
  const uint32_t top = (uint32_t)(key >> 32);
  // second pass: how many candidates have the best score, and which one carries the key
  uint32_t eq = 0u;
  for (uint32_t v = threadIdx.x; v < volume; v += kBlock) {
    if (vol[v] != top) continue;
    ++eq;
    const uint32_t kk = v / nc, c = v - kk * nc;
    const int kr = (int)kk - (int)k.rot, j = (int)(c / nx) - (int)k.ty, i = (int)(c % nx) - (int)k.tx;
    if ((uint32_t)~match_penalty(kr, j, i, k.ty) == (uint32_t)key) {  // (penalties are distinct: one thread)
      best[8u * g + 0u] = top;
      best[8u * g + 1u] = (uint32_t)kr;
      best[8u * g + 2u] = (uint32_t)j;
      best[8u * g + 3u] = (uint32_t)i;
      best[8u * g + 7u] = 0u;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) eq += __shfl_xor(eq, d, 64);
  if (lane_id() == 0) s_eq[wave_id()] = eq;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0u;
    for (int w = 0; w < kWaves; ++w) sum += s_eq[w];
    best[8u * g + 5u] = vol[(size_t)k.rot * nc + (size_t)k.ty * nx + k.tx];
    best[8u * g + 6u] = sum;
  }
}

// blocks of kPrepThreads words per group, or 0 when G groups do not fit a 1-D grid
uint32_t match_blocks_per_group(uint32_t G, uint32_t volume) {
  const uint64_t bpg = ((uint64_t)volume + kPrepThreads - 1u) / kPrepThreads;
  return (uint64_t)G * bpg > 0x7FFFFFFFull ? 0u : (uint32_t)bpg;
}

bool match_args_ok(const MatchK &k) {
  return k.width != 0 && k.height != 0 && k.width <= RPLGPU_MAX_OCC_DIM && k.height <= RPLGPU_MAX_OCC_DIM &&
         k.tx <= RPLGPU_MAX_MATCH_SHIFT && k.ty <= RPLGPU_MAX_MATCH_SHIFT && k.rot <= RPLGPU_MAX_MATCH_ROT;
}

}  // namespace

uint32_t match_volume(const MatchK &k) { return (2u * k.rot + 1u) * (2u * k.ty + 1u) * (2u * k.tx + 1u); }

hipError_t launch_match_prepare(hipStream_t s, uint32_t *scores, unsigned long long score_stride, uint32_t G,
                                const MatchK &k, uint32_t *best) {
  if (G == 0) return hipSuccess;
  if (!match_args_ok(k) || score_stride < match_volume(k)) return hipErrorInvalidValue;
  const uint32_t bpg = match_blocks_per_group(G, match_volume(k));
  if (!bpg) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_match_prepare, dim3(G * bpg), dim3(kPrepThreads), 0, s, scores, score_stride,
                     match_volume(k), bpg, best);
  return hipGetLastError();
}

hipError_t launch_match_score(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                              uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                              const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                              const float *pose2d, const float *pivot, const MatchK &k, const MatchRot &rot,
                              const int8_t *field, unsigned long long field_stride, uint32_t field_per_group,
                              uint32_t *scores, unsigned long long score_stride, uint32_t *best,
                              uint32_t *status) {
  if (B == 0) return hipSuccess;
  if (group == 0 || !match_args_ok(k) || field_stride < (unsigned long long)k.width * k.height ||
      score_stride < match_volume(k))
    return hipErrorInvalidValue;
  // slices of a scan's passes: enough workgroups for a time step of a few scans, and at most 8 x the atomics
  const uint32_t passes = (min(n_stride, kMaxN) + kFrontList - 1u) / kFrontList;
  const dim3 grid(B, 2u * k.rot + 1u, min(passes, 8u));
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_match_score<true>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, pivot, k, rot, field, field_stride,
                       field_per_group, scores, score_stride, best, status);
  else
    hipLaunchKernelGGL(k_match_score<false>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, pivot, k, rot, field, field_stride,
                       field_per_group, scores, score_stride, best, status);
  return hipGetLastError();
}

hipError_t launch_match_best(hipStream_t s, const uint32_t *scores, unsigned long long score_stride, uint32_t G,
                             const MatchK &k, uint32_t *best) {
  if (G == 0) return hipSuccess;
  if (!match_args_ok(k) || score_stride < match_volume(k)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_match_best, dim3(G), dim3(kBlock), 0, s, scores, score_stride, k, best);
  return hipGetLastError();
}

}  // namespace rpl
