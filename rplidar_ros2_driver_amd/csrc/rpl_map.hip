// rpl_map.hip — E14: a persistent hit / miss count map that many time steps vote on, the cell rule that turns
// the counts into the int8 grid E12 and E13 take, and E13's result applied to the poses on the device
// (include/rplgpu_msg.h: rplgpu_map_update_dev, rplgpu_map_grid_dev, rplgpu_apply_match_dev).
//
//   k_map_walk     adds every ray of every scan into the ONE count map (two uint32 per cell: misses, hits);
//   k_map_grid     one pass over the cells: counts -> 100 / 0 / percentage / prev-or--1, four cells per thread;
//   k_apply_match  one thread per scan: the group's (k, j, i) composed in front of the scan's pose.
//
// k_map_walk is k_occ_walk (rpl_occ.hip) with counts in the place of bits: one 1024-thread workgroup per scan,
// the same scan set-up and pair load (rpl_front.hpp's scan_front, scan_pair) and ray word (rpl_ray.hpp), 2048 samples
// per pass, the same one-step-per-iteration Bresenham over an LDS ray queue.  The wave compaction alone is written out
// here (see the pass).  What differs, because a count cannot "test the bit and skip":
//   * equal consecutive rays are not dropped but become ONE queue entry with a weight of up to 64 (the two
//     ballots of rpl_match.hip); the ray word is full, so the weights have a byte queue of their own;
//   * the window around the sensor holds 16-bit counters, two per LDS word (a scan has at most 32768 samples
//     and a ray visits a cell once: no counter carries into its neighbour), added to with no-return LDS adds
//     and flushed once per scan with no-return global adds of the non-zero counters;
//   * the sensor cell, which every walked ray of length > 0 clears exactly once, is counted in registers (one
//     LDS add per wave and pass) and its walk step is taken when the ray is pulled, without a visit;
//   * misses beyond the window and all hits are no-return global adds of the weight.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_front.hpp"
#include "rpl_ray.hpp"

namespace rpl {
namespace {

constexpr int kMapWin = 176;                  // window side in cells: 176 * 176 * 2 B = 61952 B of counters
constexpr int kMapWinWords = kMapWin / 2;     // words per window row
constexpr uint32_t kQueue = kFrontList;       // rays per pass: two samples per thread
static_assert(kMapWin % 2 == 0, "two counters per word");
static_assert(kMaxN <= 32768u, "a 16-bit window counter holds a scan's samples");

struct MapWalk {
  uint32_t *s_win;   // kMapWin rows of kMapWinWords words: the miss counters around the sensor
  uint32_t *counts;  // the map: misses at 2 * cell, hits at 2 * cell + 1
  int wx0, wy0;      // grid cell of the window's corner
  uint32_t W, H;
};
__device__ __forceinline__ void map_miss(const MapWalk &o, int cx, int cy, uint32_t w) {
  if ((uint32_t)cx >= o.W || (uint32_t)cy >= o.H) return;
  const uint32_t wx = (uint32_t)(cx - o.wx0), wy = (uint32_t)(cy - o.wy0);
  if (wx < (uint32_t)kMapWin && wy < (uint32_t)kMapWin) {
    atomicAdd(&o.s_win[wy * kMapWinWords + (wx >> 1)], w << (16u * (wx & 1u)));
  } else {
    atomicAdd(&o.counts[2u * ((uint32_t)cy * o.W + (uint32_t)cx)], w);
  }
}
__device__ __forceinline__ void map_end(const MapWalk &o, int cx, int cy, uint32_t ray, uint32_t w) {
  if (ray & kRayCut) {
    map_miss(o, cx, cy, w);
  } else if ((ray & kRayMark) && (uint32_t)cx < o.W && (uint32_t)cy < o.H) {
    atomicAdd(&o.counts[2u * ((uint32_t)cy * o.W + (uint32_t)cx) + 1u], w);
  }
}

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_map_walk(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan,
    uint32_t group, KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, OccK k, uint32_t *__restrict__ counts,
    uint32_t *__restrict__ status) {
  __shared__ uint32_t s_win[kMapWin * kMapWinWords];
  __shared__ uint32_t s_q[kQueue];
  __shared__ uint8_t s_wt[kQueue];
  __shared__ uint32_t s_cnt, s_head, s_sensor;
  const uint32_t sc = blockIdx.x;
  const uint32_t g = sc / group;
  for (uint32_t j = threadIdx.x; j < (uint32_t)(kMapWin * kMapWinWords); j += kBlock) s_win[j] = 0u;
  if (threadIdx.x == 0) s_sensor = 0u;
  const uint32_t n_in = n_per_scan[sc];
  const uint32_t n = scan_len(n_in, n_stride);
  if (threadIdx.x == 0 && status && n_in > n) atomicOr(&status[g], RPLGPU_SCAN_OUT_TRUNCATED);
  const ScanFront f = scan_front(nodes, n_stride, sc, n, p, T, keepmask, mask_stride, motion, pose2d);
  int x0 = 0, y0 = 0;
  const bool sensor_ok = grid_cell(f.sd.xf.tx, f.sd.xf.ty, k.origin_x, k.origin_y, k.resolution, &x0, &y0);
  MapWalk o;
  o.s_win = s_win;
  o.counts = counts;
  o.wx0 = x0 - kMapWin / 2;
  o.wy0 = y0 - kMapWin / 2;
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
    uint32_t own = 0u;  // this lane's share of the sensor cell's misses
    uint32_t at = 0u;
    bool h0 = false, h1 = false;
    uint32_t r0 = 0u, r1 = 0u, wt0 = 0u, wt1 = 0u;
    unsigned long long m0 = 0ull, m1 = 0ull;
    if (2u * pr < n) {  // (the active lanes of a wave are its first ones: a lane's predecessor is active)
      const ScanPair s = scan_pair(f, p, pr);
      r0 = occ_ray<FAST>(s.t.x, s.t.y, s.i0, s.k0, f.cs, f.sd.xf, k, sensor_ok, x0, y0, &cell_range);
      r1 = occ_ray<FAST>(s.t.z, s.t.w, s.i1, s.k1, f.cs, f.sd.xf, k, sensor_ok, x0, y0, &cell_range);
      // A sample continues a run when it has the ray of the sample before it; sample 0 of lanes 0 and 32 never
      // does, so a run holds at most 64 samples.  Every sample with a ray is in exactly one run: the weights of a
      // pass add up to its rays.
      const uint32_t before = __shfl_up(r1, 1, 64);  // the ray of sample i0 - 1
      const bool e0 = r0 && (lane_id() & 31u) != 0u && r0 == before, e1 = r1 && r1 == r0;
      h0 = r0 && !e0;
      h1 = r1 && !e1;
      m0 = __ballot(h0);
      m1 = __ballot(h1);
      const unsigned long long c_first = __ballot(e0), c_both = c_first & __ballot(e1);
      const uint32_t behind = run_behind(lane_id(), c_both, c_first);
      wt0 = e1 ? 2u + behind : 1u;
      wt1 = 1u + behind;
      // the sensor cell: every entry whose end cell is another one clears it once per sample of the run
      constexpr uint32_t kAtSensor = ((uint32_t)kRayBias << 15) | (uint32_t)kRayBias;
      own = (h0 && (r0 & 0x3FFFFFFFu) != kAtSensor ? wt0 : 0u) + (h1 && (r1 & 0x3FFFFFFFu) != kAtSensor ? wt1 : 0u);
    }
    // (outside the branch: a shuffle must not read a lane that is switched off)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) own += __shfl_xor(own, d, 64);
    // one LDS atomic per wave: the wave's rays stay together in the queue, in sample order (rpl_front.hpp's wave_slot
    // written out: its two ballots stand in the branch above, in front of the reduction, and lane 0's two atomics go
    // together; with wave_slot here the clean-rings walk measured 0.5 % slower)
    if (2u * pr < n) {  // (the same lanes as above: lane 0 is one of them)
      const unsigned long long below = (1ull << lane_id()) - 1ull;
      if (lane_id() == 0) {
        at = atomicAdd(&s_cnt, (uint32_t)(__popcll(m0) + __popcll(m1)));
        if (own) atomicAdd(&s_sensor, own);
      }
      at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at) + (uint32_t)(__popcll(m0 & below) + __popcll(m1 & below));
      if (h0) {
        s_q[at] = r0;
        s_wt[at] = (uint8_t)wt0;
      }
      if (h1) {
        s_q[at + (h0 ? 1u : 0u)] = r1;
        s_wt[at + (h0 ? 1u : 0u)] = (uint8_t)wt1;
      }
    }
    __syncthreads();
    const uint32_t cnt = s_cnt;  // <= kQueue: two entries per thread at the most
    // One Bresenham step per iteration, and a lane without a ray pulls the next one in the same iteration (and
    // takes its first step, off the sensor cell, there and then): the lanes of a wave are at different rays, so a
    // wave's loop count is its share of the pass's cell visits, not its longest ray.
    bool busy = false;
    uint32_t ray = 0u, w = 0u;
    int x = 0, y = 0, x1 = 0, y1 = 0, ax = 0, ay = 0, stepx = 0, stepy = 0, err = 0, left = 0;
    for (;;) {
      if (!busy) {
        const uint32_t qi = atomicAdd(&s_head, 1u);
        if (qi >= cnt) break;
        ray = s_q[qi];
        w = s_wt[qi];
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
        if (ddx != 0 || ddy != 0) {  // the sensor cell is counted: step off it
          const int e2 = 2 * err;
          if (e2 > -ay) {
            err -= ay;
            x += stepx;
          }
          if (e2 < ax) {
            err += ax;
            y += stepy;
          }
          --left;
        }
      }
      if (x == x1 && y == y1) {
        map_end(o, x, y, ray, w);
        busy = false;
      } else if (--left < 0) {
        busy = false;  // (not reachable)
      } else {
        map_miss(o, x, y, w);
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
  if (threadIdx.x == 0 && s_sensor && (uint32_t)x0 < o.W && (uint32_t)y0 < o.H)
    atomicAdd(&counts[2u * ((uint32_t)y0 * o.W + (uint32_t)x0)], s_sensor);
  // the window: the two counters of a word are two consecutive cells of one row
  for (uint32_t j = threadIdx.x; j < (uint32_t)(kMapWin * kMapWinWords); j += kBlock) {
    const uint32_t v = s_win[j];
    if (!v) continue;
    const int cy = o.wy0 + (int)(j / kMapWinWords);
    if ((uint32_t)cy >= o.H) continue;
    const int cx = o.wx0 + 2 * (int)(j % kMapWinWords);
    const uint32_t lo = v & 0xFFFFu, hi = v >> 16;
    if (lo && (uint32_t)cx < o.W) atomicAdd(&counts[2u * ((uint32_t)cy * o.W + (uint32_t)cx)], lo);
    if (hi && (uint32_t)(cx + 1) < o.W) atomicAdd(&counts[2u * ((uint32_t)cy * o.W + (uint32_t)(cx + 1))], hi);
  }
}

constexpr uint32_t kCellThreads = 256;

// byte mask of the bytes of word `w` that are cells: all but the tail of the last word
__device__ __forceinline__ uint32_t map_cell_mask(uint32_t w, uint32_t n_cells) {
  const uint32_t left = n_cells - 4u * w;  // >= 1
  return left >= 4u ? 0xFFFFFFFFu : (1u << (8u * left)) - 1u;
}

struct MapRule {  // a checked rplgpu_map_rule_t
  uint32_t min_observations, occupied_percent, mode;
};

__global__ __launch_bounds__(kCellThreads) void k_map_grid(const uint2 *__restrict__ counts, uint32_t n_cells,
                                                           MapRule rule, const int8_t *__restrict__ prev,
                                                           uint8_t *__restrict__ grid, uint32_t *__restrict__ cells) {
  const uint32_t w = blockIdx.x * kCellThreads + threadIdx.x;
  uint32_t c_lo = 0u, c_hi = 0u;  // counts of -1 | 0 and of 100 | other, 16 bits each (a wave adds at most 256)
  if (4u * w < n_cells) {
    uint32_t *words = reinterpret_cast<uint32_t *>(grid);
    const uint32_t m = map_cell_mask(w, n_cells);
    uint32_t out = m == 0xFFFFFFFFu ? 0u : (words[w] & ~m);
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      if (!((m >> (8u * e)) & 0xFFu)) continue;
      const uint2 hm = counts[4u * w + e];  // (misses, hits)
      const unsigned long long h = hm.y, n = (unsigned long long)hm.x + hm.y;
      uint32_t r;
      if (n < rule.min_observations) r = prev ? (uint32_t)(uint8_t)prev[4u * (size_t)w + e] : 0xFFu;
      else if (rule.mode == 0u) r = (h > 0ull && 100ull * h >= (unsigned long long)rule.occupied_percent * n) ? 100u : 0u;
      else r = (uint32_t)((200ull * h + n) / (2ull * n));
      out |= r << (8u * e);
      c_lo += (r == 0xFFu ? 1u : 0u) + (r == 0u ? 1u << 16 : 0u);
      c_hi += (r == 100u ? 1u : 0u) + (r != 0xFFu && r != 0u && r != 100u ? 1u << 16 : 0u);
    }
    words[w] = out;
  }
  if (!cells) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    c_lo += __shfl_xor(c_lo, d, 64);
    c_hi += __shfl_xor(c_hi, d, 64);
  }
  if (lane_id() == 0) {
    if (c_lo & 0xFFFFu) atomicAdd(&cells[0], c_lo & 0xFFFFu);
    if (c_lo >> 16) atomicAdd(&cells[1], c_lo >> 16);
    if (c_hi & 0xFFFFu) atomicAdd(&cells[2], c_hi & 0xFFFFu);
    if (c_hi >> 16) atomicAdd(&cells[3], c_hi >> 16);
  }
}

constexpr uint32_t kApplyThreads = 256;

__global__ __launch_bounds__(kApplyThreads) void k_apply_match(const uint32_t *__restrict__ best, MatchK k,
                                                               MatchRot rot, const float *__restrict__ pivot,
                                                               const float *pose_in, uint32_t B, uint32_t group,
                                                               uint32_t flags, float *pose_out,
                                                               float *__restrict__ pivot_out) {
  const uint32_t sc = blockIdx.x * kApplyThreads + threadIdx.x;
  if (sc >= B) return;
  const uint32_t g = sc / group;
  const uint32_t *bw = best + 8u * (size_t)g;
  const int kr = (int)bw[1], j = (int)bw[2], i = (int)bw[3];
  const int K = (int)k.rot;
  bool keep = kr < -K || kr > K;  // (a caller's error: no table index leaves the table)
  if ((flags & 1u) && (bw[6] != 1u || bw[0] == 0u)) keep = true;
  const float px = pivot ? pivot[2u * g] : 0.0f, py = pivot ? pivot[2u * g + 1u] : 0.0f;
  float r00 = 1.0f, r01 = 0.0f, tx = 0.0f, r10 = 0.0f, r11 = 1.0f, ty = 0.0f;
  if (pose_in) {
    const float *q = pose_in + 6u * (size_t)sc;
    r00 = q[0]; r01 = q[1]; tx = q[2]; r10 = q[3]; r11 = q[4]; ty = q[5];
  }
  float opx = px, opy = py;
  if (!keep) {
    const uint32_t kk = (uint32_t)(kr + K);
    const float c = rot.cs[2u * kk], s = rot.cs[2u * kk + 1u];
    const float dx = (float)i * k.resolution, dy = (float)j * k.resolution;
    const float n00 = c * r00 - s * r10, n01 = c * r01 - s * r11;
    const float n10 = s * r00 + c * r10, n11 = s * r01 + c * r11;
    const float qx = tx - px, qy = ty - py;
    const float ntx = ((c * qx - s * qy) + px) + dx;
    const float nty = ((s * qx + c * qy) + py) + dy;
    r00 = n00; r01 = n01; r10 = n10; r11 = n11; tx = ntx; ty = nty;
    opx = px + dx;
    opy = py + dy;
  }
  float *q = pose_out + 6u * (size_t)sc;
  q[0] = r00; q[1] = r01; q[2] = tx; q[3] = r10; q[4] = r11; q[5] = ty;
  if (pivot_out && sc == g * group) {
    pivot_out[2u * g] = opx;
    pivot_out[2u * g + 1u] = opy;
  }
}

}  // namespace

hipError_t launch_map_walk(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                           uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                           const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                           const float *pose2d, const OccK &k, uint32_t *counts, uint32_t *status) {
  if (B == 0) return hipSuccess;
  if (group == 0 || k.width == 0 || k.height == 0 || k.width > RPLGPU_MAX_OCC_DIM ||
      k.height > RPLGPU_MAX_OCC_DIM || !counts)
    return hipErrorInvalidValue;
  // (a 1-D grid takes 2^31 - 1 workgroups: no batch is split, as in launch_occ_walk)
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_map_walk<true>, dim3(B), dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, counts, status);
  else
    hipLaunchKernelGGL(k_map_walk<false>, dim3(B), dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, counts, status);
  return hipGetLastError();
}

hipError_t launch_map_grid(hipStream_t s, const uint32_t *counts, uint32_t width, uint32_t height,
                           uint32_t min_observations, uint32_t occupied_percent, uint32_t mode, const int8_t *prev,
                           int8_t *grid, uint32_t *cells) {
  if (width == 0 || height == 0 || width > RPLGPU_MAX_OCC_DIM || height > RPLGPU_MAX_OCC_DIM || !counts || !grid ||
      min_observations == 0 || occupied_percent > 100u || mode > 1u)
    return hipErrorInvalidValue;
  const uint32_t n_cells = width * height;
  const uint32_t blocks = ((n_cells + 3u) / 4u + kCellThreads - 1u) / kCellThreads;
  hipLaunchKernelGGL(k_map_grid, dim3(blocks), dim3(kCellThreads), 0, s, (const uint2 *)counts, n_cells,
                     MapRule{min_observations, occupied_percent, mode}, prev, (uint8_t *)grid, cells);
  return hipGetLastError();
}

hipError_t launch_apply_match(hipStream_t s, const uint32_t *best, const MatchK &k, const MatchRot &rot,
                              const float *pivot, const float *pose_in, uint32_t B, uint32_t group, uint32_t flags,
                              float *pose_out, float *pivot_out) {
  if (B == 0) return hipSuccess;
  if (group == 0 || !best || !pose_out || k.rot > RPLGPU_MAX_MATCH_ROT) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_apply_match, dim3((B + kApplyThreads - 1u) / kApplyThreads), dim3(kApplyThreads), 0, s, best,
                     k, rot, pivot, pose_in, B, group, flags, pose_out, pivot_out);
  return hipGetLastError();
}

}  // namespace rpl
