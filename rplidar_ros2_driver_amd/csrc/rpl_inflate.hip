// rpl_inflate.hip — E12: the costmap inflation layer over the grids E11 wrote (include/rplgpu_msg.h,
// rplgpu_inflate_grids_dev): every cell takes table[D2], D2 the squared cell distance to the nearest lethal
// cell (>= 100) of its grid within rc cells, combined with its own byte.  An exact gather, no atomics on
// the grid, one launch:
//
// k_inflate: one 256-thread workgroup per 64 x 64 output tile per grid (tiles x G flattened into
// blockIdx.x).
//   * STAGE  the (64 + 2 rc)^2 input window becomes a lethal BITMASK in LDS, 192 bits per window row (bit b
//     of a row is column tile_x0 - 64 + b; rc <= 64).  The window is read in aligned 32-bit words of the
//     grid's flat byte array (a row of an odd-width grid starts at any byte); a lethal byte is rare, so the
//     bits are ORed in one by one.  Cells outside the grid set nothing.
//   * EMPTY  a window without a lethal bit (one __syncthreads_or) skips the two passes: its cost is 0.
//   * ROWS   per window row and output column, hx = the distance |dx| <= rc to the nearest lethal bit of
//     that row from the three 64-bit mask words (clz / ffs, no scan), 255 for none; a u8 in LDS, four
//     columns per thread and store.
//   * COLS   per output word (four cells of a tile row, lanes along x): D2 = min over |dy| <= rc of
//     hx^2 + dy^2, rows y, y -+ 1, y -+ 2, ... and out once dy^2 >= the largest of the four minima.  The
//     four hx bytes are one LDS word (W a multiple of 4) or two and a v_alignbyte (any other W, where the
//     output words of a row start at any of its bytes).
//   * STORE  cost = table[D2] (the table staged in LDS), combined with the input bytes by the header's
//     rule, one 32-bit store per word; a word that the tile holds only part of (the tile's left and right
//     edge in an odd-width grid, the last word of a grid) is stored byte by byte, so the bytes behind a grid
//     and the neighbour tile's cells are never written.  Counts: a wave reduction, an LDS add per wave, one
//     global atomic per workgroup and counter.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"

namespace rpl {
namespace {

constexpr uint32_t kInfThreads = 256;
constexpr uint32_t kTile = 64;
constexpr uint32_t kMaxRc = RPLGPU_MAX_INFLATION_CELLS;
static_assert(kMaxRc <= kTile, "a mask row holds one tile width of halo on either side");
constexpr uint32_t kWinMax = kTile + 2u * kMaxRc;  // window rows (and bits per mask row)
constexpr uint32_t kMaskWords = kWinMax / 32u;     // 32-bit words per mask row
constexpr uint32_t kNone = 255u;                   // hx of a row without a lethal bit within rc
constexpr uint32_t kTableMax = kMaxRc * kMaxRc + 1u;

// hx of output column c (0 .. 63) of a mask row m0 | m1 | m2 (bit i of mk: column 64 k + i - 64)
__device__ __forceinline__ uint32_t inflate_hx(unsigned long long m0, unsigned long long m1,
                                               unsigned long long m2, uint32_t c, uint32_t rc) {
  uint32_t dl = kNone, dr = kNone;
  const unsigned long long lo = m1 & (~0ull >> (63u - c));  // columns <= c of this tile
  if (lo) dl = c - (63u - (uint32_t)__clzll((long long)lo));
  else if (m0) dl = c + 1u + (uint32_t)__clzll((long long)m0);
  const unsigned long long hi = m1 & (~0ull << c);           // columns >= c
  if (hi) dr = (uint32_t)__ffsll((unsigned long long)hi) - 1u - c;
  else if (m2) dr = 63u - c + (uint32_t)__ffsll((unsigned long long)m2);
  const uint32_t d = min(dl, dr);
  return d <= rc ? d : kNone;
}

// the header's per-cell rule: input byte v (as int8), cost 0 .. 100
__device__ __forceinline__ uint32_t inflate_combine(uint32_t vb, uint32_t cost, uint32_t inflate_unknown) {
  const int v = (int)(int8_t)vb;
  if (v >= 100) return 100u;
  if (v >= 0) return max((uint32_t)v, cost);
  return (inflate_unknown ? cost > 0u : cost >= 99u) ? cost : 0xFFu;
}

// ALIGNED: width is a multiple of 4 — every tile row starts on a word of the grid
template <bool ALIGNED>
__global__ __launch_bounds__(kInfThreads) void k_inflate(
    const uint8_t *__restrict__ in, unsigned long long in_stride, uint8_t *__restrict__ out,
    unsigned long long out_stride, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t tiles_per_grid,
    const uint8_t *__restrict__ table, uint32_t rc, uint32_t inflate_unknown, uint32_t *__restrict__ cells) {
  constexpr uint32_t kPitch = ALIGNED ? kTile : kTile + 8u;  // bytes per hx row; 4 pad bytes on either side
  constexpr uint32_t kPad = ALIGNED ? 0u : 4u;
  constexpr uint32_t kRowWords = ALIGNED ? kTile / 4u : kTile / 4u + 1u;  // output words a tile row touches
  __shared__ uint32_t s_mask[kWinMax * kMaskWords];
  __shared__ uint32_t s_hx[kWinMax * kPitch / 4u];
  __shared__ uint32_t s_table[(kTableMax + 3u) / 4u];
  __shared__ uint32_t s_cnt[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t g = blockIdx.x / tiles_per_grid;
  const uint32_t t = blockIdx.x - g * tiles_per_grid;
  const uint32_t tile_y = t / tiles_x;
  const int tx0 = (int)((t - tile_y * tiles_x) * kTile), ty0 = (int)(tile_y * kTile);
  const uint32_t win = kTile + 2u * rc;  // window rows
  const uint8_t *gin = in + (size_t)g * in_stride;
  const uint32_t *gin32 = reinterpret_cast<const uint32_t *>(gin);

  for (uint32_t j = tid; j < win * kMaskWords; j += kInfThreads) s_mask[j] = 0u;
  if (tid < 4u) s_cnt[tid] = 0u;
  __syncthreads();

  // STAGE: window columns [xa, xb) of the grid, rows ty0 - rc + r
  const int xa = max(0, tx0 - (int)rc), xb = min((int)W, tx0 + (int)kTile + (int)rc);
  const uint32_t row_words = (uint32_t)(xb - xa + 3) / 4u + 1u;  // aligned words a window row can touch
  const uint32_t ls = row_words <= 16u ? 4u : (row_words <= 32u ? 5u : 6u);  // lanes per row: 16 / 32 / 64
  const uint32_t k = tid & ((1u << ls) - 1u);
  int found = 0;
  for (uint32_t r = tid >> ls; r < win; r += kInfThreads >> ls) {
    const int y = ty0 - (int)rc + (int)r;
    if (y < 0 || y >= (int)H) continue;
    const uint32_t f0 = (uint32_t)y * W + (uint32_t)xa, f1 = (uint32_t)y * W + (uint32_t)xb;  // < 2^24
    const uint32_t w = (f0 >> 2) + k;
    if (4u * w >= f1) continue;
    const uint32_t v = gin32[w];
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
      const uint32_t f = 4u * w + e;
      if ((int)(int8_t)((v >> (8u * e)) & 0xFFu) < 100 || f < f0 || f >= f1) continue;
      const uint32_t b = f - (uint32_t)y * W + kTile - (uint32_t)tx0;  // column - (tx0 - 64), 0 .. 191
      atomicOr(&s_mask[r * kMaskWords + (b >> 5)], 1u << (b & 31u));
      found = 1;
    }
  }
  const bool any = __syncthreads_or(found) != 0;  // (also: the mask is complete)

  if (any) {
    const uint32_t n_table = rc * rc + 1u;  // whole words as words, the tail byte by byte: nothing is read
    for (uint32_t j = tid; j < n_table / 4u; j += kInfThreads)  // behind the table's last byte
      s_table[j] = reinterpret_cast<const uint32_t *>(table)[j];
    if (tid < (n_table & 3u))
      reinterpret_cast<uint8_t *>(s_table)[(n_table & ~3u) + tid] = table[(n_table & ~3u) + tid];
    // ROWS: item = (window row, four output columns)
    for (uint32_t i = tid; i < win * (kTile / 4u); i += kInfThreads) {
      const uint32_t r = i / (kTile / 4u), q = i % (kTile / 4u);
      const uint32_t *m = &s_mask[r * kMaskWords];
      const unsigned long long m0 = m[0] | ((unsigned long long)m[1] << 32),
                               m1 = m[2] | ((unsigned long long)m[3] << 32),
                               m2 = m[4] | ((unsigned long long)m[5] << 32);
      uint32_t hx4 = 0xFFFFFFFFu;
      if (m0 | m1 | m2) {
        hx4 = 0u;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) hx4 |= inflate_hx(m0, m1, m2, 4u * q + e, rc) << (8u * e);
      }
      s_hx[(r * kPitch + kPad) / 4u + q] = hx4;
      if (!ALIGNED) {
        if (q == 0u) s_hx[r * kPitch / 4u] = 0xFFFFFFFFu;
        if (q == kTile / 4u - 1u) s_hx[(r * kPitch + kPad + kTile) / 4u] = 0xFFFFFFFFu;
      }
    }
    __syncthreads();
  }

  // COLS + STORE: item = (tile row, output word of that row)
  uint8_t *gout = out + (size_t)g * out_stride;
  const uint32_t span = min(kTile, W - (uint32_t)tx0);  // tile columns inside the grid
  const uint32_t rc2 = rc * rc;
  const uint8_t *tab8 = reinterpret_cast<const uint8_t *>(s_table);
  uint32_t c_hi = 0u, c_lo = 0u;  // counts, 16 bits each: (== 100, == 99), (1 .. 98, -1); a wave adds <= 1280
  for (uint32_t i = tid; i < kTile * kRowWords; i += kInfThreads) {
    const uint32_t ty = i / kRowWords, j = i % kRowWords;
    const uint32_t y = (uint32_t)ty0 + ty;
    if (y >= H) continue;
    const uint32_t f0 = y * W + (uint32_t)tx0;
    const uint32_t a = ALIGNED ? 0u : (f0 & 3u);
    const uint32_t w = (f0 >> 2) + j;
    const int xr0 = (int)(4u * j) - (int)a;  // tile column of the word's first byte, -3 .. 64
    uint32_t valid = 0u;                     // byte mask of the word's cells that are this tile's
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (xr0 + e >= 0 && xr0 + e < (int)span) valid |= 0xFFu << (8 * e);
    if (!valid) continue;
    const uint32_t vin = gin32[w];
    uint32_t best[4];  // D2 so far; 0 for a cell that is not this tile's, so that it never keeps the walk going
#pragma unroll
    for (int e = 0; e < 4; ++e) best[e] = ((valid >> (8 * e)) & 1u) ? 0xFFFFFFu : 0u;
    if (any) {
      const uint32_t o = kPad + 4u * j - a;  // byte offset of the four hx in a row, >= 1 when not aligned
      const uint32_t lo_w = o >> 2, sh = o & 3u;
      const uint32_t rr = ty + rc;
      auto row4 = [&](uint32_t r) -> uint32_t {
        const uint32_t *p = &s_hx[r * kPitch / 4u + lo_w];
        if (ALIGNED) return p[0];
        return __builtin_amdgcn_alignbyte(p[1], p[0], sh);
      };
      auto take = [&](uint32_t h4, uint32_t dd) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t hx = (h4 >> (8 * e)) & 0xFFu;
          best[e] = min(best[e], hx * hx + dd);
        }
      };
      take(row4(rr), 0u);
      for (uint32_t d = 1; d <= rc; ++d) {
        const uint32_t dd = d * d;
        if (dd >= max(max(best[0], best[1]), max(best[2], best[3]))) break;
        take(row4(rr - d), dd);
        take(row4(rr + d), dd);
      }
    }
    uint32_t res = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((valid >> (8 * e)) & 1u)) continue;
      const uint32_t cost = (any && best[e] <= rc2) ? (uint32_t)tab8[best[e]] : 0u;
      const uint32_t rv = inflate_combine((vin >> (8 * e)) & 0xFFu, cost, inflate_unknown);
      res |= rv << (8 * e);
      c_hi += (rv == 100u ? 1u : 0u) + (rv == 99u ? 1u << 16 : 0u);
      c_lo += (rv >= 1u && rv <= 98u ? 1u : 0u) + (rv == 0xFFu ? 1u << 16 : 0u);
    }
    if (valid == 0xFFFFFFFFu) {
      reinterpret_cast<uint32_t *>(gout)[w] = res;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((valid >> (8 * e)) & 1u) gout[4u * (size_t)w + e] = (uint8_t)(res >> (8 * e));
    }
  }
  if (!cells) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    c_hi += __shfl_xor(c_hi, d, 64);
    c_lo += __shfl_xor(c_lo, d, 64);
  }
  if (lane_id() == 0) {
    if (c_hi & 0xFFFFu) atomicAdd(&s_cnt[0], c_hi & 0xFFFFu);
    if (c_hi >> 16) atomicAdd(&s_cnt[1], c_hi >> 16);
    if (c_lo & 0xFFFFu) atomicAdd(&s_cnt[2], c_lo & 0xFFFFu);
    if (c_lo >> 16) atomicAdd(&s_cnt[3], c_lo >> 16);
  }
  __syncthreads();
  if (tid < 4u && s_cnt[tid]) atomicAdd(&cells[4u * g + tid], s_cnt[tid]);
}

}  // namespace

hipError_t launch_inflate(hipStream_t s, const int8_t *in, unsigned long long in_stride, int8_t *out,
                          unsigned long long out_stride, uint32_t G, uint32_t width, uint32_t height,
                          const uint8_t *table, uint32_t rc, uint32_t inflate_unknown, uint32_t *cells) {
  if (G == 0 || width == 0 || height == 0 || width > RPLGPU_MAX_OCC_DIM || height > RPLGPU_MAX_OCC_DIM ||
      rc > kMaxRc || in_stride < (unsigned long long)width * height || (in_stride & 3u) ||
      out_stride < (unsigned long long)width * height || (out_stride & 3u))
    return hipErrorInvalidValue;
  const uint32_t tiles_x = (width + kTile - 1u) / kTile, tiles_y = (height + kTile - 1u) / kTile;
  const uint32_t tiles = tiles_x * tiles_y;
  if ((uint64_t)G * tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (width & 3u)
    hipLaunchKernelGGL(k_inflate<false>, dim3(G * tiles), dim3(kInfThreads), 0, s, (const uint8_t *)in, in_stride,
                       (uint8_t *)out, out_stride, width, height, tiles_x, tiles, table, rc, inflate_unknown, cells);
  else
    hipLaunchKernelGGL(k_inflate<true>, dim3(G * tiles), dim3(kInfThreads), 0, s, (const uint8_t *)in, in_stride,
                       (uint8_t *)out, out_stride, width, height, tiles_x, tiles, table, rc, inflate_unknown, cells);
  return hipGetLastError();
}

}  // namespace rpl
