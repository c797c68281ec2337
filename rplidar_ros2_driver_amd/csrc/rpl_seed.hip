// rpl_seed.hip — E19: a pose list seeded over a grid's free cells on the device, include/rplgpu_msg.h,
// rplgpu_seed_poses_dev: per group M poses (c, s, x, y) in E15 / E16's layout, each in the r-th free cell of the
// group's grid, r and the rest from one Philox4x32-10 block (rpl_philox.hpp) keyed as E18 with draw index 3.
//
// The free cells are never compacted into a list of indices (64 MB for the largest grid).  The scratch of one grid
// holds instead, for B = ceil(cells / 4096) index blocks of 4096 cells:
//   mask    64 B 64-bit words   bit i of word w: cell 64 w + i is free (cells at and beyond width * height: 0)
//   prefix  B words             the free cells in front of the block (k_seed_index leaves the block's own count here)
//   head    2 words             F after the substitution, and 1 when no cell was free
//   wcnt    64 B 16-bit words   the free cells of the block in front of the mask word (at most 4032)
// — 161 B + 2 words, about 1.3 bits per cell.
//
// Three launches, no workgroup waits on another, every loop bounded by a constant, every index that comes from
// scratch data clamped into its array:
//   k_seed_index   grid (B, G_f), a thread per 32-bit word of four cells (a word is read iff its first byte is a
//                  cell: grid_stride is a multiple of 4, so the word lies inside the group's stride; bytes behind the
//                  last cell are masked out).  Sixteen lanes OR their nibbles into a mask word; the first wave scans
//                  the 64 popcounts.
//   k_seed_scan    grid (G), one workgroup per group: the eight result words set to their start values (0, word 2
//                  to 0xFFFFFFFF for the minimum); workgroups g < G_f also form the exclusive prefix of their
//                  grid's <= 4096 block counts, four per thread, and write the head.
//   k_seed_emit    grid (tiles of 1024 outputs, G), one output per thread: Philox, r = hi(p0 * F), then the largest
//                  block with prefix <= r (12 steps), the largest mask word with wcnt <= the rest (6 steps) and the
//                  n-th set bit by popcounts of halves (6 steps) — an empty block or word has the prefix of its
//                  successor and is never the LARGEST such index while r < F; with F substituted the cell is r and
//                  nothing is read.  Then the float32 steps of the header, each rounded once (this unit is built
//                  with -ffp-contract=off; `/` is the IEEE divide), the E11 cell rule (rpl_grid.hpp) on the result, one 16-byte
//                  store.  A tile's statistics are wave reductions through LDS and thread 0's integer atomics.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_grid.hpp"
#include "rpl_launch.hpp"
#include "rpl_philox.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef unsigned long long u64;
typedef uint32_t sd_u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kSdTile = kBlock;          // outputs per tile: one per thread
constexpr uint32_t kSdBlockCells = 4096u;     // cells per index block: four per thread
constexpr uint32_t kSdBlockWords = 64u;       // mask words per index block
constexpr uint32_t kSdMaxBlocks = RPLGPU_MAX_OCC_DIM * RPLGPU_MAX_OCC_DIM / kSdBlockCells;
static_assert(kSdBlockCells == 4u * kBlock && kSdMaxBlocks == 4u * kBlock, "four cells and four blocks per thread");

struct SeedScratch {
  u64 *mask;
  uint32_t *prefix, *head;
  uint16_t *wcnt;
};
__host__ __device__ inline uint32_t sd_blocks(uint32_t cells) { return (cells + kSdBlockCells - 1u) / kSdBlockCells; }
__host__ __device__ inline u64 sd_grid_words(uint32_t blocks) { return ((u64)blocks * 161u + 2u + 1u) & ~1ull; }
__device__ __forceinline__ SeedScratch sd_scratch(uint32_t *scratch, uint32_t blocks, uint32_t gf) {
  uint32_t *base = scratch + sd_grid_words(blocks) * gf;
  SeedScratch s;
  s.mask = reinterpret_cast<u64 *>(base);
  s.prefix = base + 128u * (size_t)blocks;
  s.head = s.prefix + blocks;
  s.wcnt = reinterpret_cast<uint16_t *>(s.head + 2);
  return s;
}

__global__ __launch_bounds__(kBlock) void k_seed_index(const int8_t *__restrict__ grid, u64 grid_stride,
                                                       uint32_t cells, uint32_t blocks, int32_t free_lo,
                                                       int32_t free_hi, uint32_t *__restrict__ scratch) {
  __shared__ u64 s_mask[kSdBlockWords];
  const uint32_t b = blockIdx.x, gf = blockIdx.y;
  const uint32_t first = b * kSdBlockCells + 4u * threadIdx.x;  // the thread's first cell, below 2^24 + 4096
  uint32_t nib = 0u;
  if (first < cells) {
    const uint32_t word = reinterpret_cast<const uint32_t *>(grid + (size_t)gf * grid_stride)[first >> 2];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
      const int32_t v = (int32_t)(int8_t)(word >> (8u * i));
      if (first + i < cells && v >= free_lo && v <= free_hi) nib |= 1u << i;
    }
  }
  // sixteen lanes make one mask word: lanes 0 .. 7 of the sixteen its low half, 8 .. 15 its high half
  const uint32_t sub = lane_id() & 15u;
  uint32_t lo = sub < 8u ? nib << (4u * sub) : 0u, hi = sub < 8u ? 0u : nib << (4u * (sub - 8u));
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, d, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, d, 64);
  }
  if (sub == 0u) s_mask[threadIdx.x >> 4] = (u64)lo | (u64)hi << 32;
  __syncthreads();
  if (threadIdx.x < kSdBlockWords) {
    const SeedScratch s = sd_scratch(scratch, blocks, gf);
    const u64 m = s_mask[threadIdx.x];
    const uint32_t c = (uint32_t)__popcll(m);
    const uint32_t incl = wave_incl_scan_fast(c);
    const size_t w = (size_t)b * kSdBlockWords + threadIdx.x;  // every block has all 64 words
    s.mask[w] = m;
    s.wcnt[w] = (uint16_t)(incl - c);
    if (threadIdx.x == kSdBlockWords - 1u) s.prefix[b] = incl;  // the block's count, until k_seed_scan
  }
}

__global__ __launch_bounds__(kBlock) void k_seed_scan(uint32_t cells, uint32_t blocks, uint32_t n_grids,
                                                      uint32_t *__restrict__ scratch, uint32_t *__restrict__ result) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  const uint32_t g = blockIdx.x;
  if (threadIdx.x < 8u) result[8u * (size_t)g + threadIdx.x] = threadIdx.x == 2u ? 0xFFFFFFFFu : 0u;
  if (g >= n_grids) return;  // (the whole workgroup)
  const SeedScratch s = sd_scratch(scratch, blocks, g);
  uint32_t c[4], sum = 0u;
#pragma unroll
  for (uint32_t i = 0; i < 4u; ++i) {
    const uint32_t b = 4u * threadIdx.x + i;
    c[i] = b < blocks ? s.prefix[b] : 0u;
    sum += c[i];
  }
  uint32_t total;
  uint32_t run = block_excl_scan(sum, s_tmp, &total);
#pragma unroll
  for (uint32_t i = 0; i < 4u; ++i) {
    const uint32_t b = 4u * threadIdx.x + i;
    if (b < blocks) s.prefix[b] = run;
    run += c[i];
  }
  if (threadIdx.x == 0) {
    s.head[0] = total ? total : cells;
    s.head[1] = total ? 0u : 1u;
  }
}

__global__ __launch_bounds__(kBlock) void k_seed_emit(
    float origin_x, float origin_y, float resolution, uint32_t width, uint32_t cells, uint32_t blocks,
    uint32_t centres, uint32_t grid_per_group, const uint2 *__restrict__ headings, uint32_t H, uint32_t M,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi, uint32_t first,
    const uint32_t *__restrict__ scratch, float *__restrict__ poses_out, u64 out_stride,
    uint32_t *__restrict__ cells_out, u64 cell_stride, uint32_t *__restrict__ result) {
  __shared__ uint32_t s_part[3][kWaves];
  const uint32_t g = blockIdx.y;
  const uint32_t j = blockIdx.x * kSdTile + threadIdx.x;
  const bool live = j < M;
  const SeedScratch s = sd_scratch(const_cast<uint32_t *>(scratch), blocks, grid_per_group ? g : 0u);
  const Philox4 p = philox4x32_10(first + j, g << 2 | 3u, step_lo, step_hi, seed_lo, seed_hi);  // (first + j mod 2^32)
  const uint32_t p0 = p.w0, p1 = p.w1, p2 = p.w2, p3 = p.w3;
  const uint32_t F = min(max(s.head[0], 1u), cells), none = s.head[1] & 1u;
  const uint32_t r = __umulhi(p0, F);  // below F
  uint32_t cell = r;
  if (!none) {
    uint32_t b = 0u;
#pragma unroll
    for (uint32_t step = kSdMaxBlocks >> 1; step; step >>= 1) {
      const uint32_t t = b + step;
      if (t < blocks && s.prefix[t] <= r) b = t;
    }
    const uint32_t rb = r - min(s.prefix[b], r);
    const uint16_t *wc = s.wcnt + (size_t)b * kSdBlockWords;
    uint32_t w = 0u;
#pragma unroll
    for (uint32_t step = kSdBlockWords >> 1; step; step >>= 1) {
      const uint32_t t = w + step;  // below 64
      if ((uint32_t)wc[t] <= rb) w = t;
    }
    uint32_t n = rb - min((uint32_t)wc[w], rb);
    const u64 m = s.mask[(size_t)b * kSdBlockWords + w];
    uint32_t pos = 0u;
#pragma unroll
    for (uint32_t half = 32u; half; half >>= 1) {
      const uint32_t c = (uint32_t)__popcll((m >> pos) & ((1ull << half) - 1ull));
      if (n >= c) {
        n -= c;
        pos += half;
      }
    }
    cell = min((b * kSdBlockWords + w) * 64u + min(pos, 63u), cells - 1u);
  }
  const uint32_t k = __umulhi(p1, H);  // below H
  const uint2 cs = headings[k];
  const uint32_t cy = cell / width, cx = cell - cy * width;
  const float fx = centres ? 0.5f : ((float)(p2 >> 24) + 0.5f) * (1.0f / 256.0f);
  const float fy = centres ? 0.5f : ((float)(p3 >> 24) + 0.5f) * (1.0f / 256.0f);
  const float ux = (float)cx + fx, uy = (float)cy + fy;
  const float mx = ux * resolution, my = uy * resolution;
  const float x = origin_x + mx, y = origin_y + my;
  int bx = 0, by = 0;
  const bool has = grid_cell(x, y, origin_x, origin_y, resolution, &bx, &by);
  const bool off = !(has && bx == (int)cx && by == (int)cy);
  if (live) {
    sd_u32x4 out;
    out.x = cs.x;
    out.y = cs.y;
    out.z = __float_as_uint(x);
    out.w = __float_as_uint(y);
    reinterpret_cast<sd_u32x4 *>(poses_out + (size_t)g * out_stride)[j] = out;  // j < M <= out_stride / 4
    if (cells_out) cells_out[(size_t)g * cell_stride + j] = cell;               // j < M <= cell_stride
  }
  // the tile's statistics, a thread without an output adding nothing
  const uint32_t t_off = wave_incl_scan_fast(live && off ? 1u : 0u);
  const uint32_t t_min = wave_min_lane63(live ? cell : 0xFFFFFFFFu);
  const uint32_t t_max = wave_max_lane63(live ? cell : 0u);
  if (lane_id() == 63u) {
    s_part[0][wave_id()] = t_off;
    s_part[1][wave_id()] = t_min;
    s_part[2][wave_id()] = t_max;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // (output 0 of the tile is live: the grid has no empty tile)
    uint32_t n = 0u, lo = 0xFFFFFFFFu, hi = 0u;
    for (int q = 0; q < kWaves; ++q) {
      n += s_part[0][q];
      lo = min(lo, s_part[1][q]);
      hi = max(hi, s_part[2][q]);
    }
    uint32_t *res = result + 8u * (size_t)g;
    atomicMax(res + 0, F);
    if (n) atomicAdd(res + 1, n);
    atomicMin(res + 2, lo);
    atomicMax(res + 3, hi);
    const uint32_t flags = none | (n ? 2u : 0u);
    if (flags) atomicOr(res + 7, flags);
  }
}

}  // namespace

unsigned long long seed_scratch_words(uint32_t n_grids, uint32_t width, uint32_t height) {
  if (n_grids == 0 || n_grids > 65535u || width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 ||
      height > RPLGPU_MAX_OCC_DIM)
    return 0;
  return sd_grid_words(sd_blocks(width * height)) * n_grids;
}

hipError_t launch_seed(hipStream_t s, const SeedK &k, const int8_t *grid, unsigned long long grid_stride,
                       uint32_t grid_per_group, const float *headings, uint32_t H, uint32_t G, uint32_t M,
                       unsigned long long seed, unsigned long long step, uint32_t first, float *poses_out,
                       unsigned long long out_stride, uint32_t *cells_out, unsigned long long cell_stride,
                       uint32_t *result, uint32_t *scratch) {
  if (G == 0 || G > 65535u || M == 0 || M > RPLGPU_MAX_POSES || H == 0 || H > 65536u || k.width == 0 ||
      k.width > RPLGPU_MAX_OCC_DIM || k.height == 0 || k.height > RPLGPU_MAX_OCC_DIM)
    return hipErrorInvalidValue;
  const uint32_t cells = k.width * k.height, blocks = sd_blocks(cells), n_grids = grid_per_group ? G : 1u;
  if (grid_stride < cells || (grid_stride & 3u) || out_stride < 4ull * M || (out_stride & 3u) ||
      (cells_out && cell_stride < M))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_seed_index, dim3(blocks, n_grids), dim3(kBlock), 0, s, grid, grid_stride, cells, blocks,
                     k.free_lo, k.free_hi, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_seed_scan, dim3(G), dim3(kBlock), 0, s, cells, blocks, n_grids, scratch, result);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_seed_emit, dim3((M + kSdTile - 1u) / kSdTile, G), dim3(kBlock), 0, s, k.origin_x, k.origin_y,
                     k.resolution, k.width, cells, blocks, k.centres, grid_per_group,
                     reinterpret_cast<const uint2 *>(headings), H, M, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)step, (uint32_t)(step >> 32), first, scratch, poses_out, out_stride, cells_out,
                     cell_stride, result);
  return hipGetLastError();
}

}  // namespace rpl
