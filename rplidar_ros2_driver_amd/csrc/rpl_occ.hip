// rpl_occ.hip — E11: one ray-cast occupancy grid per group of scans (the sensors of one time step),
// include/rplgpu_msg.h, rplgpu_occupancy_grid_dev: every beam is traced from ITS sensor through the grid,
// the cells it passes are cleared, the cell it ends in is marked (the costmap obstacle layer's mark-and-clear).
//
// The output is its own scratch, three launches and nothing on the handle:
//   k_occ_prepare  zeroes the width * height bytes of every group's grid;
//   k_occ_walk     ORs 0x01 (cleared) / 0x02 (marked) into the cells' bytes;
//   k_occ_finish   maps a byte with 0x02 to 100, one with 0x01 to 0, any other to d_prev or -1, and counts.
//
// k_occ_walk: one 1024-thread workgroup per scan, the front end of rpl_front.hpp WRITTEN OUT (two nodes per
// bounds-checked buffer_load_dwordx4, E1 / E5 keep bits, the (cos, sin) table, rpl_xf.hpp's sample_xy), so a
// point lands where E8 and E9 put it, bit for bit.  It is the one kernel of E9 - E25 that does not call that
// header: through scan_len / scan_front / scan_pair / wave_slot the compiler's code had the same instruction
// count and resources but another order of a few scalar instructions, and the clean-rings walk of
// tools/dev/occbench.py measured 0.1 - 0.2 % above this form after five more alternating pairs
// (profiles/r31/scan_front_r31.txt).  A change to the front end in rpl_front.hpp has
// to be repeated here; tests/test_gpu_occ.py holds this copy to the oracle.  Behind it, per 2048 samples:
//   * a sample becomes a RAY: one word, the end cell relative to the sensor cell (the sensor cell is the
//     scan's; the spec bounds |delta| by raytrace_max / resolution <= 8192) and the whole / cut / mark bits.
//     A ray equal to its predecessor's is dropped (consecutive samples of a wall end in the same cell; the
//     result is a set), the others are compacted into an LDS queue (ballot, one atomic per wave).
//   * the rays of a scan differ in length by an order of magnitude.  The walk is ONE loop of one Bresenham
//     step per iteration; a lane whose ray is done pulls the next one off the queue (an LDS counter) in the
//     same iteration, so the lanes of a wave sit at different rays and none idles through the wave's longest.
//     An iteration in which some lane pulls costs the wave that pull; rays are 100 - 800 steps long.
//   * every ray of a scan passes the cells next to its sensor: clears go to a kWin x kWin bit window around
//     the sensor cell in LDS — test the bit first (a broadcast read), ds_or only when it is not set yet, so
//     the hot cells cost a read — and the window is flushed once per scan, four cells per 32-bit atomic OR.
//     Only clears beyond the window and the marks (one per ray) are global atomics (no return value).
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_msg.hpp"
#include "rpl_ray.hpp"  // the cell rule and the ray word, shared with rpl_map.hip
#include "rpl_xf.hpp"

namespace rpl {
namespace {

typedef uint32_t oc_u32x4 __attribute__((ext_vector_type(4)));
constexpr int kWin = 640;                    // window side in cells: 50 KB of bits
constexpr int kWinWords = kWin / 32;         // words per window row
constexpr uint32_t kQueue = 2u * kBlock;     // rays per pass: two samples per thread
constexpr uint32_t kClearBit = 1u, kMarkBit = 2u;

struct OccWalk {
  uint32_t *s_win;   // kWin rows of kWinWords words: the cleared bits around the sensor
  uint32_t *words;   // the group's grid as words
  int wx0, wy0;      // grid cell of the window's corner
  uint32_t W, H;
};
__device__ __forceinline__ void occ_or_byte(const OccWalk &o, int cx, int cy, uint32_t bit) {
  const uint32_t idx = (uint32_t)cy * o.W + (uint32_t)cx;
  atomicOr(&o.words[idx >> 2], bit << ((idx & 3u) * 8u));
}
__device__ __forceinline__ void occ_clear(const OccWalk &o, int cx, int cy) {
  if ((uint32_t)cx >= o.W || (uint32_t)cy >= o.H) return;
  const uint32_t wx = (uint32_t)(cx - o.wx0), wy = (uint32_t)(cy - o.wy0);
  if (wx < (uint32_t)kWin && wy < (uint32_t)kWin) {
    uint32_t *w = &o.s_win[wy * kWinWords + (wx >> 5)];
    const uint32_t m = 1u << (wx & 31u);
    if (!(*(volatile uint32_t *)w & m)) atomicOr(w, m);
  } else {
    occ_or_byte(o, cx, cy, kClearBit);
  }
}
__device__ __forceinline__ void occ_end(const OccWalk &o, int cx, int cy, uint32_t ray) {
  if (ray & kRayCut) {
    occ_clear(o, cx, cy);
  } else if ((ray & kRayMark) && (uint32_t)cx < o.W && (uint32_t)cy < o.H) {
    occ_or_byte(o, cx, cy, kMarkBit);
  }
}

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_occ_walk(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan,
    uint32_t group, KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, OccK k, uint8_t *__restrict__ grid,
    unsigned long long grid_stride, uint32_t *__restrict__ status) {
  __shared__ uint32_t s_win[kWin * kWinWords];
  __shared__ uint32_t s_q[kQueue];
  __shared__ uint32_t s_cnt, s_head;
  const uint32_t sc = blockIdx.x;
  const uint32_t g = sc / group;
  for (uint32_t j = threadIdx.x; j < (uint32_t)(kWin * kWinWords); j += kBlock) s_win[j] = 0u;
  const uint32_t n_in = n_per_scan[sc];
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(n_in, min(n_stride, kMaxN)));
  if (threadIdx.x == 0 && status && n_in > n) atomicOr(&status[g], RPLGPU_SCAN_OUT_TRUNCATED);
  const ScanSide sd = scan_side(sc, keepmask, mask_stride, motion, pose2d, T.scan_t0);
  const float2 *cs = p.inverted ? T.cs_inv : T.cs;
  const uint32_t q_min16 = p.clip_enable ? (min(p.q_min, 256u) << 16) : 0u;
  const uint2 *scan = nodes + (size_t)sc * n_stride;
  // bounds-checked over the scan's n * 8 bytes: a node beyond it reads as zero (and i < n drops it)
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void *)scan, 0, (int)(n * 8u), 0x00020000);
  int x0 = 0, y0 = 0;
  const bool sensor_ok = grid_cell(sd.xf.tx, sd.xf.ty, k.origin_x, k.origin_y, k.resolution, &x0, &y0);
  OccWalk o;
  o.s_win = s_win;
  o.words = reinterpret_cast<uint32_t *>(grid + (size_t)g * grid_stride);
  o.wx0 = x0 - kWin / 2;
  o.wy0 = y0 - kWin / 2;
  o.W = k.width;
  o.H = k.height;
  bool cell_range = false;
  for (uint32_t base = 0; base < n; base += kQueue) {
    if (threadIdx.x == 0) {
      s_cnt = 0u;
      s_head = 0u;
    }
    __syncthreads();  // (also: the window is clear, the last pass's walkers are done with the queue)
    const uint32_t pr = base / 2u + threadIdx.x;
    if (2u * pr < n) {  // (the active lanes of a wave are its first ones: a lane's predecessor is active)
      const oc_u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(pr * 16u), 0, 0);
      const uint32_t i0 = 2u * pr, i1 = i0 + 1u;
      bool k0 = i0 < n && (__builtin_amdgcn_alignbit(t.y, t.x, 16) - p.d_lo) <= p.d_span &&
                (t.y & 0x00FF0000u) >= q_min16;  // E1
      bool k1 = i1 < n && (__builtin_amdgcn_alignbit(t.w, t.z, 16) - p.d_lo) <= p.d_span &&
                (t.w & 0x00FF0000u) >= q_min16;
      if (sd.ror_bits) {  // E1 AND E5 (launch_ror_mask); both samples sit in one word (i0 is even)
        const uint32_t w = sd.ror_bits[i0 >> 5];
        k0 = k0 && ((w >> (i0 & 31u)) & 1u);
        k1 = k1 && ((w >> (i1 & 31u)) & 1u);
      }
      const uint32_t r0 = occ_ray<FAST>(t.x, t.y, i0, k0, cs, sd.xf, k, sensor_ok, x0, y0, &cell_range);
      const uint32_t r1 = occ_ray<FAST>(t.z, t.w, i1, k1, cs, sd.xf, k, sensor_ok, x0, y0, &cell_range);
      const uint32_t before = __shfl_up(r1, 1, 64);  // the ray of sample i0 - 1
      const bool p0 = r0 && !(lane_id() != 0 && r0 == before), p1 = r1 && r1 != r0;
      // one LDS atomic per wave: the wave's rays stay together in the queue, in sample order
      const unsigned long long m0 = __ballot(p0), m1 = __ballot(p1);
      const unsigned long long below = (1ull << lane_id()) - 1ull;
      uint32_t at = 0u;
      if (lane_id() == 0) at = atomicAdd(&s_cnt, (uint32_t)(__popcll(m0) + __popcll(m1)));
      at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at) + (uint32_t)(__popcll(m0 & below) + __popcll(m1 & below));
      if (p0) s_q[at] = r0;
      if (p1) s_q[at + (p0 ? 1u : 0u)] = r1;
    }
    __syncthreads();
    const uint32_t cnt = s_cnt;
    // One Bresenham step per iteration, and a lane without a ray pulls the next one in the same iteration:
    // the lanes of a wave are at different rays, so a wave's loop count is its share of the pass's cell
    // visits, not its longest ray.  A lane leaves when it has no ray and the queue is empty.
    bool busy = false;
    uint32_t ray = 0u;
    int x = 0, y = 0, x1 = 0, y1 = 0, ax = 0, ay = 0, stepx = 0, stepy = 0, err = 0, left = 0;
    for (;;) {
      if (!busy) {
        const uint32_t qi = atomicAdd(&s_head, 1u);
        if (qi >= cnt) break;
        ray = s_q[qi];
        const int ddx = (int)(ray & 0x7FFFu) - kRayBias, ddy = (int)((ray >> 15) & 0x7FFFu) - kRayBias;
        x1 = x0 + ddx;
        y1 = y0 + ddy;
        ax = abs(ddx);
        ay = abs(ddy);
        stepx = ddx > 0 ? 1 : (ddx < 0 ? -1 : 0);
        stepy = ddy > 0 ? 1 : (ddy < 0 ? -1 : 0);
        err = ax - ay;
        x = x0;
        y = y0;
        left = ax + ay;  // (every step moves at least one axis towards the end cell: this bounds the walk)
        busy = true;
      }
      if (x == x1 && y == y1) {
        occ_end(o, x, y, ray);
        busy = false;
      } else if (--left < 0) {
        busy = false;  // (not reachable)
      } else {
        occ_clear(o, x, y);
        const int e2 = 2 * err;
        if (e2 > -ay) {
          err -= ay;
          x += stepx;
        }
        if (e2 < ax) {
          err += ax;
          y += stepy;
        }
      }
    }
    __syncthreads();  // nobody pulls any more: the counters may be reset
  }
  if (status && __any(cell_range) && lane_id() == 0) atomicOr(&status[g], RPLGPU_SCAN_CELL_RANGE);
  // the window, four cells per atomic: a nibble of a window word is four consecutive cells of one row
  for (uint32_t j = threadIdx.x; j < (uint32_t)(kWin * kWinWords); j += kBlock) {
    const uint32_t w = s_win[j];
    if (!w) continue;
    const int cy = o.wy0 + (int)(j / kWinWords);
    if ((uint32_t)cy >= o.H) continue;
    const int cxw = o.wx0 + 32 * (int)(j % kWinWords);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t b = (w >> (4 * q)) & 0xFu;
      if (!b) continue;
      const int cx = cxw + 4 * q;
      uint32_t v = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (((b >> e) & 1u) && (uint32_t)(cx + e) < o.W) v |= kClearBit << (8 * e);
      if (!v) continue;
      // (cx may be up to 3 below 0: those bytes of v are zero, and so is whatever would leave the grid)
      const long long idx = (long long)cy * (long long)o.W + (long long)cx;
      const long long wi = idx >> 2;
      const uint32_t sh = (uint32_t)(idx & 3) * 8u;
      const uint32_t lo = v << sh, hi = sh ? v >> (32u - sh) : 0u;
      if (lo) atomicOr(&o.words[wi], lo);
      if (hi) atomicOr(&o.words[wi + 1], hi);
    }
  }
}

constexpr uint32_t kCellThreads = 256;

// byte mask of the bytes of word `w` (of a group's words) that are cells: all but the tail of the last word
__device__ __forceinline__ uint32_t occ_cell_mask(uint32_t w, uint32_t n_cells) {
  const uint32_t left = n_cells - 4u * w;  // >= 1
  return left >= 4u ? 0xFFFFFFFFu : (1u << (8u * left)) - 1u;
}

__global__ __launch_bounds__(kCellThreads) void k_occ_prepare(uint8_t *__restrict__ grid,
                                                              unsigned long long grid_stride, uint32_t n_cells,
                                                              uint32_t blocks_per_group) {
  const uint32_t g = blockIdx.x / blocks_per_group;
  const uint32_t w = (blockIdx.x - g * blocks_per_group) * kCellThreads + threadIdx.x;
  if (4u * w >= n_cells) return;
  uint32_t *words = reinterpret_cast<uint32_t *>(grid + (size_t)g * grid_stride);
  const uint32_t m = occ_cell_mask(w, n_cells);
  words[w] = m == 0xFFFFFFFFu ? 0u : (words[w] & ~m);
}

__global__ __launch_bounds__(kCellThreads) void k_occ_finish(uint8_t *__restrict__ grid,
                                                             unsigned long long grid_stride, uint32_t n_cells,
                                                             uint32_t blocks_per_group,
                                                             const int8_t *__restrict__ prev,
                                                             uint32_t *__restrict__ cells) {
  const uint32_t g = blockIdx.x / blocks_per_group;
  const uint32_t w = (blockIdx.x - g * blocks_per_group) * kCellThreads + threadIdx.x;
  uint32_t c = 0u;  // counts of 0 / 100 / -1, 10 bits each (a wave adds at most 256)
  if (4u * w < n_cells) {
    uint32_t *words = reinterpret_cast<uint32_t *>(grid + (size_t)g * grid_stride);
    const int8_t *pv = prev ? prev + (size_t)g * grid_stride + 4u * (size_t)w : nullptr;
    const uint32_t m = occ_cell_mask(w, n_cells);
    const uint32_t in = words[w];
    uint32_t out = in & ~m;
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      if (!((m >> (8u * e)) & 0xFFu)) continue;
      const uint32_t b = (in >> (8u * e)) & 0xFFu;
      uint32_t r;
      if (b & kMarkBit) r = 100u;
      else if (b & kClearBit) r = 0u;
      else r = pv ? (uint32_t)(uint8_t)pv[e] : 0xFFu;
      out |= r << (8u * e);
      c += (r == 0u ? 1u : 0u) + (r == 100u ? 1u << 10 : 0u) + (r == 0xFFu ? 1u << 20 : 0u);
    }
    words[w] = out;
  }
  if (!cells) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
  if (lane_id() == 0 && c) {
    if (c & 0x3FFu) atomicAdd(&cells[3u * g], c & 0x3FFu);
    if ((c >> 10) & 0x3FFu) atomicAdd(&cells[3u * g + 1u], (c >> 10) & 0x3FFu);
    if ((c >> 20) & 0x3FFu) atomicAdd(&cells[3u * g + 2u], (c >> 20) & 0x3FFu);
  }
}

constexpr uint32_t kMsgThreads = 256;
constexpr uint32_t kChunk = 16384;  // dwords per workgroup and step

// The prefix carries every scalar and the data length word (the same for all G messages); a message
// differs from the next only by its two stamps and its cells.
__global__ __launch_bounds__(kMsgThreads) void k_msg_occupancy(
    const uint8_t *__restrict__ grid, unsigned long long grid_stride, uint32_t n_cells,
    const rplgpu_stamp_t *__restrict__ stamps, rplmsg::Prefix P, uint8_t *__restrict__ msgs,
    uint32_t msg_stride, uint32_t *__restrict__ msg_len, uint32_t *__restrict__ status) {
  const uint32_t b = blockIdx.y;
  const uint64_t total = (uint64_t)P.len + n_cells;
  const bool fits = total <= msg_stride;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    msg_len[b] = fits ? (uint32_t)total : 0u;
    if (status && !fits) atomicOr(&status[b], RPLGPU_SCAN_OUT_TRUNCATED);
  }
  if (!fits) return;
  uint8_t *msg8 = msgs + (size_t)b * msg_stride;
  uint32_t *msg = reinterpret_cast<uint32_t *>(msg8);
  const uint8_t *src8 = grid + (size_t)b * grid_stride;
  if (blockIdx.x == 0) {
    for (uint32_t i = threadIdx.x; i < P.len / 4; i += kMsgThreads) msg[i] = P.words[i];
    __syncthreads();  // the stamp patches overwrite template words
    if (threadIdx.x == 0) {
      msg[P.stamp_off / 4] = (uint32_t)stamps[b].sec;
      msg[P.stamp_off / 4 + 1] = stamps[b].nanosec;
      msg[P.a_off / 4] = (uint32_t)stamps[b].sec;  // info.map_load_time
      msg[P.a_off / 4 + 1] = stamps[b].nanosec;
      for (uint32_t i = n_cells & ~3u; i < n_cells; ++i) msg8[P.len + i] = src8[i];  // the tail bytes
    }
  }
  const uint32_t *src = reinterpret_cast<const uint32_t *>(src8);
  uint32_t *out = msg + P.len / 4;
  const uint32_t nw = n_cells / 4u;
  for (uint32_t first = blockIdx.x * kChunk; first < nw; first += gridDim.x * kChunk) {
    const uint32_t last = min(first + kChunk, nw);
    for (uint32_t j = first + threadIdx.x; j < last; j += kMsgThreads) out[j] = src[j];
  }
}

// blocks of kCellThreads words per group, or 0 when G groups do not fit a 1-D grid
uint32_t occ_blocks_per_group(uint32_t G, uint32_t n_cells) {
  const uint64_t bpg = ((uint64_t)(n_cells + 3u) / 4u + kCellThreads - 1u) / kCellThreads;
  return (uint64_t)G * bpg > 0x7FFFFFFFull ? 0u : (uint32_t)bpg;
}

}  // namespace

hipError_t launch_occ_prepare(hipStream_t s, int8_t *grid, unsigned long long grid_stride, uint32_t G,
                              const OccK &k) {
  if (G == 0) return hipSuccess;
  const uint32_t n_cells = k.width * k.height;
  const uint32_t bpg = occ_blocks_per_group(G, n_cells);
  if (!bpg) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_occ_prepare, dim3(G * bpg), dim3(kCellThreads), 0, s, (uint8_t *)grid, grid_stride,
                     n_cells, bpg);
  return hipGetLastError();
}

hipError_t launch_occ_walk(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                           uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                           const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                           const float *pose2d, const OccK &k, int8_t *grid, unsigned long long grid_stride,
                           uint32_t *status) {
  if (B == 0) return hipSuccess;
  if (group == 0 || k.width == 0 || k.height == 0 || k.width > RPLGPU_MAX_OCC_DIM ||
      k.height > RPLGPU_MAX_OCC_DIM || grid_stride < (unsigned long long)k.width * k.height || (grid_stride & 3u))
    return hipErrorInvalidValue;
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_occ_walk<true>, dim3(B), dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride,
                       n_per_scan, group, p, T, keepmask, mask_stride, motion, pose2d, k, (uint8_t *)grid,
                       grid_stride, status);
  else
    hipLaunchKernelGGL(k_occ_walk<false>, dim3(B), dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride,
                       n_per_scan, group, p, T, keepmask, mask_stride, motion, pose2d, k, (uint8_t *)grid,
                       grid_stride, status);
  return hipGetLastError();
}

hipError_t launch_occ_finish(hipStream_t s, int8_t *grid, unsigned long long grid_stride, uint32_t G,
                             const OccK &k, const int8_t *prev, uint32_t *cells) {
  if (G == 0) return hipSuccess;
  const uint32_t n_cells = k.width * k.height;
  const uint32_t bpg = occ_blocks_per_group(G, n_cells);
  if (!bpg) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_occ_finish, dim3(G * bpg), dim3(kCellThreads), 0, s, (uint8_t *)grid, grid_stride,
                     n_cells, bpg, prev, cells);
  return hipGetLastError();
}

hipError_t launch_msg_occupancy(hipStream_t s, const int8_t *grid, unsigned long long grid_stride,
                                uint32_t n_cells, uint32_t G, const rplgpu_stamp_t *stamps,
                                const rplmsg::Prefix &P, uint8_t *msgs, uint32_t msg_stride, uint32_t *msg_len,
                                uint32_t *status) {
  if (G == 0) return hipSuccess;
  const uint32_t gx = min((n_cells / 4u + kChunk - 1) / kChunk, 64u);
  for (uint32_t b0 = 0; b0 < G; b0 += 65535u) {  // gridDim.y limit
    const uint32_t nb = min(G - b0, 65535u);
    hipLaunchKernelGGL(k_msg_occupancy, dim3(gx ? gx : 1, nb), dim3(kMsgThreads), 0, s,
                       (const uint8_t *)grid + (size_t)b0 * grid_stride, grid_stride, n_cells, stamps + b0, P,
                       msgs + (size_t)b0 * msg_stride, msg_stride, msg_len + b0,
                       status ? status + b0 : nullptr);
  }
  return hipGetLastError();
}

}  // namespace rpl
