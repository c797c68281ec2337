// rpl_pose.hip — E15: a list of arbitrary poses weighed against a likelihood field, include/rplgpu_msg.h,
// rplgpu_score_poses_dev: the points of a group of scans (the sensors of one time step, in the base frame) are laid
// over the field at every pose (c, s, tx, ty) of a caller-made list, the field values under them are added up per
// pose and the list is reduced to eight result words.  The particle filter's sensor update (AMCL's form): poses
// that sit on no lattice, so every look-up has a rotation, a translation and a cell rule of its own.
//
// The weights are the call's own scratch and result, three launches and nothing on the handle:
//   k_pose_prepare  zeroes every group's P weights and its eight result words;
//   k_pose_score    adds the field values under the points into the weights;
//   k_pose_best     reduces a group's weights to its eight result words.
//
// k_pose_score: one 1024-thread workgroup per (scan, tile of 1024 poses, slice of the scan's 2048-sample passes),
// the front end of rpl_front.hpp (scan_front, front_point_pass: two nodes per bounds-checked buffer_load_dwordx4,
// E1 / E5 keep bits, the (cos, sin) table, rpl_xf.hpp's sample_xy), so a point lands where E8, E9, E11 and E13 put
// it, bit for bit.  Per 2048 samples:
//   * the finite points are compacted into an LDS list of float2 (front_point_pass: one atomic per wave);
//   * then a thread owns ONE pose in registers and walks the list: every lane of a wave reads the same LDS
//     address, a broadcast, two points per 128-bit read.  A list of up to 1024 poses is rounded up to whole waves
//     and repeated over the workgroup as often as it fits; each copy walks its share of the point pairs;
//   * the copies are added up through LDS and leave with one no-return atomic add per non-zero pose.
// All integers behind the cell rule: the weights depend on no order.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_front.hpp"

namespace rpl {
namespace {

static_assert(kFrontList * sizeof(float2) == 16384, "the point list is 16 KiB");

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_pose_score(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan, uint32_t group,
    KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, PoseK k, const float *__restrict__ poses,
    uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group, const int8_t *__restrict__ field,
    unsigned long long field_stride, uint32_t field_per_group, uint32_t *__restrict__ weights,
    unsigned long long weight_stride, uint32_t *__restrict__ result, uint32_t *__restrict__ status) {
  __shared__ f32x4 s_pts[kFrontList / 2u];  // two points (x0, y0, x1, y1) per element
  __shared__ uint32_t s_sum[kBlock];
  __shared__ uint32_t s_cnt[2];  // the list's length, by the pass's parity: a reset never meets a late reader
  const uint32_t sc = blockIdx.x;
  const uint32_t tile = blockIdx.y;
  const uint32_t g = sc / group;
  const uint32_t n_in = n_per_scan[sc];
  const uint32_t n = scan_len(n_in, n_stride);
  const bool first_of_scan = tile == 0u && blockIdx.z == 0u;
  if (threadIdx.x == 0 && status && first_of_scan && n_in > n) atomicOr(&status[g], RPLGPU_SCAN_OUT_TRUNCATED);
  if (blockIdx.z * kFrontList >= n) return;  // (block-uniform)
  const ScanFront f = scan_front(nodes, n_stride, sc, n, p, T, keepmask, mask_stride, motion, pose2d);
  const OccK ck{k.origin_x, k.origin_y, k.resolution, k.width, k.height, 0.0f, 0.0f, 0.0f};  // (the cell rule's part)
  const int8_t *fld = field + (size_t)(field_per_group ? g : 0u) * field_stride;
  const PoseLane l = pose_lane(tile, P, poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
  uint32_t acc = 0u;
  uint32_t finite = 0u;
  bool cell_range = false;
  uint32_t pass = 0u;
  float2 *pts = reinterpret_cast<float2 *>(s_pts);
  for (uint32_t base = blockIdx.z * kFrontList; base < n; base += gridDim.z * kFrontList) {
    uint32_t *cnt_at = &s_cnt[pass++ & 1u];
    if (threadIdx.x == 0) *cnt_at = 0u;
    __syncthreads();  // (also: the last pass's readers are done with the list)
    front_point_pass<FAST>(f, base, p, cnt_at, pts, nullptr, nullptr, nullptr, &finite);
    __syncthreads();
    const uint32_t cnt = *cnt_at;  // <= kFrontList
    if (l.own) {
      // copy `slice` walks the point pairs slice, slice + slices, ...: pair e holds points 2e and 2e + 1 < kFrontList
#pragma unroll 2
      for (uint32_t e = l.slice; 2u * e < cnt; e += l.slices) {
        const f32x4 v = s_pts[e];
        acc += pose_look(v.x, v.y, l.c, l.s, l.tx, l.ty, ck, fld, &cell_range);
        if (2u * e + 1u < cnt) acc += pose_look(v.z, v.w, l.c, l.s, l.tx, l.ty, ck, fld, &cell_range);
      }
    }
  }
  if (status && __any(cell_range) && lane_id() == 0) atomicOr(&status[g], RPLGPU_SCAN_CELL_RANGE);
  if (tile == 0u) {  // word 4, the group's finite points: once per sample, by the workgroups of the first tile
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) finite += __shfl_xor(finite, d, 64);
    if (lane_id() == 0 && finite) atomicAdd(&result[8u * g + 4u], finite);
  }
  __syncthreads();
  s_sum[threadIdx.x] = acc;  // copy `slice` at [slice * per, slice * per + per); 0 where a thread owns no pose
  __syncthreads();
  if (threadIdx.x < l.per && tile * kPoseTile + threadIdx.x < P) {
    uint32_t sum = 0u;
    for (uint32_t s = 0; s < l.slices; ++s) sum += s_sum[s * l.per + threadIdx.x];  // slices * per <= kBlock
    if (sum) atomicAdd(&weights[(size_t)g * weight_stride + tile * kPoseTile + threadIdx.x], sum);
  }
}

constexpr uint32_t kPrepThreads = 256;

__global__ __launch_bounds__(kPrepThreads) void k_pose_prepare(uint32_t *__restrict__ weights,
                                                               unsigned long long weight_stride, uint32_t P,
                                                               uint32_t blocks_per_group,
                                                               uint32_t *__restrict__ result) {
  const uint32_t g = blockIdx.x / blocks_per_group;
  const uint32_t b = blockIdx.x - g * blocks_per_group;
  const uint32_t w = b * kPrepThreads + threadIdx.x;
  if (w < P) weights[(size_t)g * weight_stride + w] = 0u;
  if (b == 0 && threadIdx.x < 8u) result[8u * g + threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kBlock) void k_pose_best(const uint32_t *__restrict__ weights,
                                                      unsigned long long weight_stride, uint32_t P,
                                                      uint32_t *__restrict__ result) {
  __shared__ unsigned long long s_key[kWaves];
  __shared__ unsigned long long s_total[kWaves];
  __shared__ uint32_t s_zero[kWaves];
  __shared__ uint32_t s_eq[kWaves];
  const uint32_t g = blockIdx.x;
  const uint32_t *wt = weights + (size_t)g * weight_stride;
  // the largest (weight, ~q): the weight in the high word, so the smallest q wins a tie
  unsigned long long key = 0ull, total = 0ull;
  uint32_t zero = 0u;
  for (uint32_t v = threadIdx.x; v < P; v += kBlock) {
    const uint32_t w = wt[v];
    const unsigned long long cand = ((unsigned long long)w << 32) | (uint32_t)~v;
    key = cand > key ? cand : key;
    zero += w == 0u ? 1u : 0u;
    total += w;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d, 64);
    key = o > key ? o : key;
    zero += __shfl_xor(zero, d, 64);
    total += __shfl_xor(total, d, 64);
  }
  if (lane_id() == 0) {
    s_key[wave_id()] = key;
    s_zero[wave_id()] = zero;
    s_total[wave_id()] = total;
  }
  __syncthreads();
  key = s_key[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) key = s_key[w] > key ? s_key[w] : key;
  const uint32_t top = (uint32_t)(key >> 32);
  uint32_t eq = 0u;  // second pass: how many poses have the best weight
  for (uint32_t v = threadIdx.x; v < P; v += kBlock) eq += wt[v] == top ? 1u : 0u;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) eq += __shfl_xor(eq, d, 64);
  if (lane_id() == 0) s_eq[wave_id()] = eq;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t n_eq = 0u, n_zero = 0u;
    unsigned long long sum = 0ull;
    for (int w = 0; w < kWaves; ++w) {
      n_eq += s_eq[w];
      n_zero += s_zero[w];
      sum += s_total[w];
    }
    result[8u * g + 0u] = top;
    result[8u * g + 1u] = ~(uint32_t)key;
    result[8u * g + 2u] = n_eq;
    result[8u * g + 3u] = n_zero;
    result[8u * g + 5u] = wt[0];  // (word 4 is k_pose_score's)
    result[8u * g + 6u] = (uint32_t)sum;
    result[8u * g + 7u] = (uint32_t)(sum >> 32);
  }
}

// blocks of kPrepThreads words per group, or 0 when G groups do not fit a 1-D grid
uint32_t pose_blocks_per_group(uint32_t G, uint32_t P) {
  const uint64_t bpg = ((uint64_t)P + kPrepThreads - 1u) / kPrepThreads;
  return (uint64_t)G * bpg > 0x7FFFFFFFull ? 0u : (uint32_t)bpg;
}

bool pose_args_ok(const PoseK &k, uint32_t P) {
  return k.width != 0 && k.height != 0 && k.width <= RPLGPU_MAX_OCC_DIM && k.height <= RPLGPU_MAX_OCC_DIM &&
         P != 0 && P <= RPLGPU_MAX_POSES;
}

}  // namespace

hipError_t launch_pose_prepare(hipStream_t s, uint32_t *weights, unsigned long long weight_stride, uint32_t G,
                               uint32_t P, uint32_t *result) {
  if (G == 0) return hipSuccess;
  if (P == 0 || P > RPLGPU_MAX_POSES || weight_stride < P) return hipErrorInvalidValue;
  const uint32_t bpg = pose_blocks_per_group(G, P);
  if (!bpg) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pose_prepare, dim3(G * bpg), dim3(kPrepThreads), 0, s, weights, weight_stride, P, bpg,
                     result);
  return hipGetLastError();
}

hipError_t launch_pose_score(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                             uint32_t B, uint32_t group, const KParams &p, const Tables &T,
                             const uint32_t *keepmask, uint32_t mask_stride, const float *motion,
                             const float *pose2d, const PoseK &k, const float *poses, uint32_t P,
                             unsigned long long pose_stride, uint32_t poses_per_group, const int8_t *field,
                             unsigned long long field_stride, uint32_t field_per_group, uint32_t *weights,
                             unsigned long long weight_stride, uint32_t *result, uint32_t *status) {
  if (B == 0) return hipSuccess;
  if (group == 0 || !pose_args_ok(k, P) || field_stride < (unsigned long long)k.width * k.height ||
      pose_stride < 4ull * P || (pose_stride & 3u) || weight_stride < P)
    return hipErrorInvalidValue;
  // slices of a scan's passes: enough workgroups for a time step of a few scans, and at most 8 x the atomics
  const uint32_t passes = (min(n_stride, kMaxN) + kFrontList - 1u) / kFrontList;
  const dim3 grid(B, (P + kPoseTile - 1u) / kPoseTile, min(passes, 8u));
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_pose_score<true>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride,
                       poses_per_group, field, field_stride, field_per_group, weights, weight_stride, result,
                       status);
  else
    hipLaunchKernelGGL(k_pose_score<false>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride,
                       poses_per_group, field, field_stride, field_per_group, weights, weight_stride, result,
                       status);
  return hipGetLastError();
}

hipError_t launch_pose_best(hipStream_t s, const uint32_t *weights, unsigned long long weight_stride, uint32_t G,
                            uint32_t P, uint32_t *result) {
  if (G == 0) return hipSuccess;
  if (P == 0 || P > RPLGPU_MAX_POSES || weight_stride < P) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pose_best, dim3(G), dim3(kBlock), 0, s, weights, weight_stride, P, result);
  return hipGetLastError();
}

}  // namespace rpl
