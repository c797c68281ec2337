// rpl_cast.hip — E22: a beam fan cast from every pose of a list into a grid, include/rplgpu_msg.h,
// rplgpu_cast_ranges_dev: per group the P poses (c, s, tx, ty) of E15 / E16 / E19's layout each send A rays, one per
// entry (cb, sb) of the beam table, through the group's int8 grid by E11's all-integer Bresenham rule to the first cell
// that stops them; a ray's range word is D2 | kind << 28.  With a measured scan the word is compared with the beam's
// measured range through the caller's byte table and the terms are summed into E15's weights.
//
// Two launches of this unit (E15's k_pose_prepare in front and k_pose_best behind them when weights are asked for), no
// workgroup waits on another, every loop bounded by N = max_steps or a constant, every index that comes from data
// tested or clamped before use:
//   k_cast_start   grid (G): the eight cast words of a group zeroed; with a measured scan result word 4 = the beams
//                  whose z is not NaN (k_pose_prepare has zeroed the eight result words and the P weights).
//   k_cast         grid (tiles of 256 rays, G), one ray per thread, ray r = q * A + a: neighbouring lanes take
//                  neighbouring beams of one pose, so their first steps read the same grid lines and the range words
//                  leave as one coalesced store.  The set-up is one 16-byte pose load, one 8-byte beam load, the two
//                  float32 compositions of the header and two cell rules (four IEEE divides); the walk reads one grid
//                  byte per visit.  A tile's 256 rays belong to at most 256 consecutive poses: their terms are added
//                  in LDS and leave as at most one integer atomic per pose and tile.  The counts are ballots and wave
//                  reductions into LDS, then seven integer atomics per workgroup: order-free sums and one max; the
//                  64-bit sum of n is a 32-bit add whose returned value tells the one adder that wrapped the low word
//                  to carry into the high word.
// This unit is built with -ffp-contract=off: every float32 operation rounds once.  The cell rule is E11's, rpl_grid.hpp's
// grid_cell with this stage's spec.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_grid.hpp"
#include "rpl_launch.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef float ca_f32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kCaBlock = 256u;  // rays per tile: one per thread
constexpr uint32_t kCaWaves = kCaBlock / 64u;
static_assert((uint64_t)kCaBlock * RPLGPU_MAX_OCC_STEPS < (1ull << 32), "a tile's sum of n fits one word");
static_assert(255ull * RPLGPU_MAX_MERGE_BEAMS < (1ull << 32), "a weight fits one word");

__global__ __launch_bounds__(kCaBlock) void k_cast_start(const float *__restrict__ measured,
                                                         unsigned long long meas_stride, uint32_t meas_first,
                                                         uint32_t meas_step, uint32_t A,
                                                         uint32_t *__restrict__ result, uint32_t *__restrict__ cast) {
  __shared__ uint32_t s_n[kCaWaves];
  const uint32_t g = blockIdx.x;
  if (threadIdx.x < 8u) cast[8u * g + threadIdx.x] = 0u;
  if (!measured) return;  // (the same in every thread)
  uint32_t n = 0u;
  for (uint32_t a = threadIdx.x; a < A; a += kCaBlock) {
    const float z = measured[(size_t)g * meas_stride + meas_first + (size_t)a * meas_step];
    n += z != z ? 0u : 1u;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
  if (lane_id() == 0) s_n[wave_id()] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0u;
    for (uint32_t w = 0; w < kCaWaves; ++w) sum += s_n[w];
    result[8u * g + 4u] = sum;
  }
}

__global__ __launch_bounds__(kCaBlock) void k_cast(
    const CastK k, const float *__restrict__ poses, unsigned long long pose_stride, uint32_t poses_per_group,
    uint32_t P, const float2 *__restrict__ beams, uint32_t A, const int8_t *__restrict__ grid,
    unsigned long long grid_stride, uint32_t grid_per_group, const float *__restrict__ measured,
    unsigned long long meas_stride, uint32_t meas_first, uint32_t meas_step, const uint8_t *__restrict__ table,
    uint32_t *__restrict__ ranges, unsigned long long range_stride, uint32_t *__restrict__ weights,
    unsigned long long weight_stride, uint32_t *__restrict__ cast) {
  __shared__ uint32_t s_w[kCaBlock];  // the terms of pose q_first + i of this tile
  __shared__ uint32_t s_cnt[8];       // the tile's share of the eight cast words (6: the sum of n, one word)
  const uint32_t g = blockIdx.y;
  const uint32_t rays = P * A;  // <= 2^28 (host-checked)
  const uint32_t r_first = blockIdx.x * kCaBlock, r = r_first + threadIdx.x;
  const bool live = r < rays;
  const uint32_t q_first = r_first / A;
  s_w[threadIdx.x] = 0u;
  if (threadIdx.x < 8u) s_cnt[threadIdx.x] = 0u;
  __syncthreads();

  uint32_t word = RPLGPU_CAST_DROPPED, n = 0u;
  if (live) {
    const uint32_t q = min(r / A, P - 1u), a = r - q * A;
    const float *pl = poses + (poses_per_group ? (size_t)g * pose_stride : (size_t)0);
    const ca_f32x4 pose = *reinterpret_cast<const ca_f32x4 *>(pl + 4u * (size_t)q);
    const float2 b = beams[a];
    const float c = pose.x, s = pose.y, tx = pose.z, ty = pose.w;
    const float dc = c * b.x - s * b.y, ds = s * b.x + c * b.y;  // (each product rounded, then the difference or sum)
    const float rm = (float)k.max_steps * k.resolution;
    const float ex = tx + dc * rm, ey = ty + ds * rm;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    if (grid_cell(tx, ty, k.origin_x, k.origin_y, k.resolution, &x0, &y0) &&
        grid_cell(ex, ey, k.origin_x, k.origin_y, k.resolution, &x1, &y1)) {
      const int8_t *gr = grid + (grid_per_group ? (size_t)g * grid_stride : (size_t)0);
      const int ax = abs(x1 - x0), ay = abs(y1 - y0);
      const int stepx = (x1 > x0) - (x1 < x0), stepy = (y1 > y0) - (y1 < y0);
      int err = ax - ay, x = x0, y = y0;
      uint32_t kind = RPLGPU_CAST_NONE;
      for (n = 0u; n <= k.max_steps; ++n) {  // (the rule's n == N test leaves first: the bound of the loop twice)
        if ((uint32_t)x >= k.width || (uint32_t)y >= k.height) {
          kind = RPLGPU_CAST_LEFT;
          break;
        }
        const int v = gr[(uint32_t)y * k.width + (uint32_t)x];
        if (v >= k.hit_lo) {
          kind = RPLGPU_CAST_HIT;
          break;
        }
        if (v < 0 && k.unknown_stops) {
          kind = RPLGPU_CAST_UNKNOWN;
          break;
        }
        if ((x == x1 && y == y1) || n == k.max_steps) break;
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
      n = min(n, k.max_steps);
      const int dx = x - x0, dy = y - y0;  // |dx|, |dy| <= n <= 8192
      const uint32_t d2 = (uint32_t)(dx * dx + dy * dy);
      word = d2 | (kind << 28);
    }
    if (ranges) ranges[(size_t)g * range_stride + r] = word;
    if (measured && word != RPLGPU_CAST_DROPPED) {
      const float z = measured[(size_t)g * meas_stride + meas_first + (size_t)a * meas_step];
      if (!(z != z)) {
        const uint32_t K = k.table_half;
        const float inf = __builtin_huge_valf();
        const float mz = z / k.resolution;
        const float de = (word >> 28) == RPLGPU_CAST_NONE ? inf : sqrtf((float)(word & 0x0FFFFFFFu));
        uint32_t idx = 2u * K + 1u;
        if (!(mz == inf && de == inf)) {
          const float d = mz - de;
          const float cl = fmaxf(-(float)K, fminf((float)K, floorf(d)));
          idx = (uint32_t)min(max((int)K + (int)cl, 0), (int)(2u * K));
        }
        const uint32_t t = table[idx];
        if (t) atomicAdd(&s_w[min(q - q_first, kCaBlock - 1u)], t);
      }
    }
  }

  // the tile's counts: a ray is of exactly one of five classes
  const bool dropped = word == RPLGPU_CAST_DROPPED;
  const uint32_t kind = word >> 28;
  uint32_t hit_d2 = live && !dropped && kind == RPLGPU_CAST_HIT ? (word & 0x0FFFFFFFu) : 0u;
  uint32_t steps = live ? n : 0u;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    hit_d2 = max(hit_d2, (uint32_t)__shfl_xor(hit_d2, d, 64));
    steps += __shfl_xor(steps, d, 64);
  }
#pragma unroll
  for (uint32_t cls = 0; cls < 5u; ++cls) {
    const bool mine = live && (cls == 4u ? dropped : (!dropped && kind == cls));
    const uint32_t cnt = (uint32_t)__popcll(__ballot(mine));
    if (lane_id() == 0 && cnt) atomicAdd(&s_cnt[cls], cnt);
  }
  if (lane_id() == 0) {
    if (hit_d2) atomicMax(&s_cnt[5], hit_d2);
    if (steps) atomicAdd(&s_cnt[6], steps);
  }
  __syncthreads();
  if (measured) {
    const uint32_t q = q_first + threadIdx.x, w = s_w[threadIdx.x];
    if (q < P && w) atomicAdd(&weights[(size_t)g * weight_stride + q], w);
  }
  if (threadIdx.x < 7u) {
    const uint32_t v = s_cnt[threadIdx.x];
    uint32_t *out = cast + 8u * (size_t)g;
    if (v) {
      if (threadIdx.x < 5u) {
        atomicAdd(&out[threadIdx.x], v);
      } else if (threadIdx.x == 5u) {
        atomicMax(&out[5], v);
      } else {
        const uint32_t old = atomicAdd(&out[6], v);
        if (old + v < old) atomicAdd(&out[7], 1u);  // this add wrapped the low word
      }
    }
  }
}

}  // namespace

hipError_t launch_cast(hipStream_t s, const CastK &k, const float *poses, unsigned long long pose_stride,
                       uint32_t poses_per_group, uint32_t G, uint32_t P, const float *beams, uint32_t A,
                       const int8_t *grid, unsigned long long grid_stride, uint32_t grid_per_group,
                       const float *measured, unsigned long long meas_stride, uint32_t meas_first, uint32_t meas_step,
                       const uint8_t *table, uint32_t *ranges, unsigned long long range_stride, uint32_t *weights,
                       unsigned long long weight_stride, uint32_t *result, uint32_t *cast) {
  const unsigned long long rays = (unsigned long long)P * A;
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || A == 0 || A > RPLGPU_MAX_MERGE_BEAMS ||
      rays > RPLGPU_MAX_CAST_RAYS || k.width == 0 || k.height == 0 || k.width > RPLGPU_MAX_OCC_DIM ||
      k.height > RPLGPU_MAX_OCC_DIM || k.max_steps == 0 || k.max_steps > RPLGPU_MAX_OCC_STEPS ||
      k.table_half > RPLGPU_MAX_CAST_TABLE_HALF || !poses || !beams || !grid || !cast || (!ranges && !measured) ||
      pose_stride < 4ull * P || (pose_stride & 3u) || grid_stride < (unsigned long long)k.width * k.height ||
      (ranges && range_stride < rays))
    return hipErrorInvalidValue;
  if (measured && (!table || !weights || !result || weight_stride < P ||
                   meas_first + (unsigned long long)(A - 1u) * meas_step >= meas_stride))
    return hipErrorInvalidValue;
  if (measured) {
    const hipError_t e = launch_pose_prepare(s, weights, weight_stride, G, P, result);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cast_start, dim3(G), dim3(kCaBlock), 0, s, measured, meas_stride, meas_first, meas_step, A,
                     result, cast);
  const dim3 tiles((uint32_t)((rays + kCaBlock - 1u) / kCaBlock), G);
  hipLaunchKernelGGL(k_cast, tiles, dim3(kCaBlock), 0, s, k, poses, pose_stride, poses_per_group, P,
                     (const float2 *)beams, A, grid, grid_stride, grid_per_group, measured, meas_stride, meas_first,
                     meas_step, table, ranges, range_stride, weights, weight_stride, cast);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (measured) e = launch_pose_best(s, weights, weight_stride, G, P, result);
  return e;
}

}  // namespace rpl
