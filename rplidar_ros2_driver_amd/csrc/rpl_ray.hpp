// rpl_ray.hpp — what the ray walkers share behind rpl_xf.hpp's front end: E11 (rpl_occ.hip) and E14
// (rpl_map.hip) turn a sample into the same RAY word by the same float32 operations, and E13 (rpl_match.hip) and
// E14 turn runs of equal consecutive samples into one entry with a weight by the same two ballots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rpl_grid.hpp"
#include "rpl_launch.hpp"
#include "rpl_xf.hpp"

namespace rpl {

constexpr int kRayBias = 16384;              // |end cell - sensor cell| < kRayBias (host-checked spec: <= 8195)
constexpr uint32_t kRayCut = 1u << 30, kRayMark = 1u << 31;

// One sample to its ray word, or 0: no ray (not kept, ignored by the range rules, or dropped).
template <bool FAST>
__device__ __forceinline__ uint32_t occ_ray(uint32_t lo, uint32_t hi, uint32_t i, bool kept,
                                            const float2 *__restrict__ cs, const ScanXf &xf, const OccK &k,
                                            bool sensor_ok, int x0, int y0, bool *cell_range) {
  if (!kept) return 0u;
  const f2 xy = sample_xy<FAST>(lo, hi, i, cs, xf);
  const float sx = xf.tx, sy = xf.ty;
  const float dx = xy.x - sx, dy = xy.y - sy;
  const float d = sqrtf(dx * dx + dy * dy);
  if (!(d < __builtin_huge_valf()) || d < k.range_min) return 0u;  // (not finite: NaN fails the compare)
  float ex = xy.x, ey = xy.y;
  uint32_t bits = d <= k.obstacle_max ? kRayMark : 0u;
  if (!(d <= k.raytrace_max)) {
    const float t = k.raytrace_max / d;
    ex = sx + dx * t;
    ey = sy + dy * t;
    bits = kRayCut;
  }
  int x1, y1;
  if (!sensor_ok || !grid_cell(ex, ey, k.origin_x, k.origin_y, k.resolution, &x1, &y1)) {
    *cell_range = true;
    return 0u;
  }
  const int ddx = x1 - x0, ddy = y1 - y0;
  if (abs(ddx) >= kRayBias || abs(ddy) >= kRayBias) {  // (not reachable with a checked spec)
    *cell_range = true;
    return 0u;
  }
  return bits | ((uint32_t)(ddy + kRayBias) << 15) | (uint32_t)(ddx + kRayBias);
}

// Samples that continue a run, counted from sample 0 of lane L + 1: `both` has a lane's bit when its two
// samples continue, `first` when its sample 0 does.
__device__ __forceinline__ uint32_t run_behind(uint32_t L, unsigned long long both, unsigned long long first) {
  if (L >= 63u) return 0u;
  const unsigned long long stop = (~both >> (L + 1u)) | (~0ull << (63u - L));
  const uint32_t n = (uint32_t)__builtin_ctzll(stop);
  const uint32_t at = L + 1u + n;
  return 2u * n + (at < 64u ? (uint32_t)((first >> at) & 1ull) : 0u);
}

}  // namespace rpl
