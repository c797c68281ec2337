// rpl_estimate.hip — E17: a weighted pose list reduced to the sums of a pose estimate, include/rplgpu_msg.h,
// rplgpu_estimate_poses_dev: E15's weights and the list they weigh (or E16's list, every weight 1) become the integer
// moments a mean pose and its covariance are formed from.  Every pose entry is quantised by one float32 product and
// one round-to-nearest-even; from there on everything is integers, so no order of summation matters.
//
// Two launches, 1024 poses per tile, no workgroup waits on another, no atomic and no loop bounded by a word from memory;
// the limbs, the wave sums, the 128-bit adds and the layout of the scratch are rpl_moments.hpp's, shared with E21:
//   k_estimate_tiles   one pose per thread (one 16-byte load, one 4-byte load); every thread quantises the centre pose
//                      itself (a broadcast load) and tests the gate; es_tile_sums adds the tile (set 0: in range, set 1:
//                      in the gate);
//   k_estimate_finish  one workgroup per group: es_finish_sums writes words 8 - 71, thread 0 writes words 0 - 7.
// The scratch of a group: rpl_moments.hpp's 17 planes of T tiles, 68 T words.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_moments.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

__global__ __launch_bounds__(kBlock) void k_estimate_tiles(const float *__restrict__ poses, u64 pose_stride,
                                                           uint32_t poses_per_group,
                                                           const uint32_t *__restrict__ weights, u64 weight_stride,
                                                           uint32_t P, float xy_scale, u64 gate_r2, i64 gate_dot,
                                                           const uint32_t *__restrict__ center, u64 center_stride,
                                                           uint32_t *__restrict__ scratch) {
  const uint32_t tile = blockIdx.x, g = blockIdx.y;
  const uint32_t T = es_tiles(P);
  const es_f32x4 *src =
      reinterpret_cast<const es_f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
  const uint32_t qc = min(center ? center[(size_t)g * center_stride] : 0u, P - 1u);  // clamped before it is used
  const EsPose c = es_quantise(src[qc], xy_scale);
  const uint32_t i = tile * kEsTile + threadIdx.x;
  const bool live = i < P;
  const es_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const EsPose q = es_quantise(live ? src[i] : zero, xy_scale);
  const uint32_t w = live ? (weights ? weights[(size_t)g * weight_stride + i] : 1u) : 0u;
  const bool in0 = live && q.in;
  const i64 dX = (i64)q.X - c.X, dY = (i64)q.Y - c.Y;
  const u64 r2 = (u64)(dX * dX + dY * dY);
  const i64 dot = (i64)q.C * c.C + (i64)q.S * c.S;
  const bool in1 = in0 && c.in && r2 <= gate_r2 && dot >= gate_dot;
  es_tile_sums(q, w, in0, in1, tile, T, scratch + (size_t)g * es_group_words(T));
}

__global__ __launch_bounds__(kBlock) void k_estimate_finish(const float *__restrict__ poses, u64 pose_stride,
                                                            uint32_t poses_per_group, uint32_t P, float xy_scale,
                                                            const uint32_t *__restrict__ center, u64 center_stride,
                                                            const uint32_t *__restrict__ scratch,
                                                            uint32_t *__restrict__ result) {
  __shared__ uint32_t s_cnt[4];
  __shared__ uint32_t s_empty[2];
  const uint32_t g = blockIdx.x;
  const uint32_t T = es_tiles(P);
  const uint32_t *grp = scratch + (size_t)g * es_group_words(T);
  uint32_t *res = result + (size_t)RPLGPU_ESTIMATE_WORDS * g;
  es_finish_sums(grp, T, res, s_cnt, s_empty);
  if (threadIdx.x == 0) {
    const es_f32x4 *src =
        reinterpret_cast<const es_f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
    const uint32_t qc = min(center ? center[(size_t)g * center_stride] : 0u, P - 1u);
    const EsPose c = es_quantise(src[qc], xy_scale);
    res[0] = (c.in ? 0u : 1u) | (s_cnt[0] != P ? 2u : 0u) | (s_empty[0] ? 4u : 0u) | (s_empty[1] ? 8u : 0u);
    res[1] = qc;
    res[2] = s_cnt[0];
    res[3] = s_cnt[1];
    res[4] = s_cnt[2];
    res[5] = s_cnt[3];
    res[6] = 0u;
    res[7] = 0u;
  }
}

}  // namespace

unsigned long long estimate_scratch_words(uint32_t G, uint32_t P) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES) return 0ull;
  return (u64)G * es_group_words(es_tiles(P));
}

hipError_t launch_estimate(hipStream_t s, const float *poses, unsigned long long pose_stride,
                           uint32_t poses_per_group, const uint32_t *weights, unsigned long long weight_stride,
                           uint32_t G, uint32_t P, float xy_scale, unsigned long long gate_r2, long long gate_dot,
                           const uint32_t *center, unsigned long long center_stride, uint32_t *result,
                           uint32_t *scratch) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || pose_stride < 4ull * P ||
      (weights && weight_stride < P))
    return hipErrorInvalidValue;
  const uint32_t T = es_tiles(P);
  hipLaunchKernelGGL(k_estimate_tiles, dim3(T, G), dim3(kBlock), 0, s, poses, pose_stride, poses_per_group, weights,
                     weight_stride, P, xy_scale, gate_r2, gate_dot, center, center_stride, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_estimate_finish, dim3(G), dim3(kBlock), 0, s, poses, pose_stride, poses_per_group, P,
                     xy_scale, center, center_stride, scratch, result);
  return hipGetLastError();
}

}  // namespace rpl
