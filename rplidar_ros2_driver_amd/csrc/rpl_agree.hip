// rpl_agree.hip — E23: the beams a pose list disagrees with are left out of the weights, include/rplgpu_msg.h,
// rplgpu_score_poses_agree_dev (AMCL's beam skip of the likelihood_field_prob model).
//
// The decision needs every sample's count over the WHOLE list before any sample can be left out, so there are two
// passes over look-ups — but E15 is not paid twice: the first pass makes the count AND the full E15 sum from one
// field load, the second takes off only what the skipped samples added (usually a few percent of the points).  The
// weights are unsigned and no final value is negative, so the subtraction is exact in any order.
//   k_agree_prepare  zeroes weights, result, counts, mask and agree words (the smallest count starts at ~0);
//   k_agree_count    E15's grid and walk (one workgroup per scan x tile of 1024 poses x slice of passes, the front end
//                    of rpl_front.hpp, a thread owns one pose and walks the LDS point list by broadcast): per point
//                    acc += f, one ballot of f >= agree_lo per wave popcounted into an LDS counter of the list entry;
//                    at the end of a pass the non-zero counters leave with one no-return atomic add each; the first
//                    tile's workgroups store the finite bits and add result word 4;
//   k_agree_decide   a thread per sample: the rule bit from count and P, a ballot makes the mask words (finite AND
//                    kept), wave reductions and integer atomics make F, K, the largest, smallest and summed count;
//   k_agree_flag     a thread per group: agree words 2, 3 and 5;
//   k_agree_apply    count's grid: nothing for a group that fell back, else only the skipped samples are listed and
//                    their sums are subtracted per pose.
// launch_pose_best (rpl_pose.hip) then makes the result words from the final weights.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rpl_agree.hpp"
#include "rpl_front.hpp"

namespace rpl {
namespace {

static_assert(kFrontList * sizeof(float2) == 16384, "the point list is 16 KiB");

constexpr uint32_t kPrepThreads = 256;
constexpr uint32_t kPrepBlocks = 2048;

// every output word of the call: G x P weights, 8 G result words, B x n_stride counts, B x mask_words mask words,
// 8 G agree words (word 5, the smallest count, starts at ~0 for the atomic min)
__global__ __launch_bounds__(kPrepThreads) void k_agree_prepare(
    uint32_t *__restrict__ weights, unsigned long long weight_stride, uint32_t G, uint32_t P,
    uint32_t *__restrict__ result, uint32_t *__restrict__ counts, unsigned long long count_stride, uint32_t B,
    uint32_t n_stride, uint32_t *__restrict__ mask, unsigned long long mask_words_stride, uint32_t mask_words,
    uint32_t *__restrict__ agree) {
  const unsigned long long t0 = (unsigned long long)blockIdx.x * kPrepThreads + threadIdx.x;
  const unsigned long long step = (unsigned long long)gridDim.x * kPrepThreads;
  for (unsigned long long v = t0; v < (unsigned long long)G * P; v += step) {
    const unsigned long long g = v / P;
    weights[g * weight_stride + (v - g * P)] = 0u;
  }
  for (unsigned long long v = t0; v < (unsigned long long)B * n_stride; v += step) {
    const unsigned long long sc = v / n_stride;
    counts[sc * count_stride + (v - sc * n_stride)] = 0u;
  }
  for (unsigned long long v = t0; v < (unsigned long long)B * mask_words; v += step) {
    const unsigned long long sc = v / mask_words;
    mask[sc * mask_words_stride + (v - sc * mask_words)] = 0u;
  }
  for (unsigned long long v = t0; v < 8ull * G; v += step) {
    result[v] = 0u;
    agree[v] = (v & 7u) == 5u ? 0xFFFFFFFFu : 0u;
  }
}

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_agree_count(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan, uint32_t group,
    KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, AgreeK k, const float *__restrict__ poses,
    uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group, const int8_t *__restrict__ field,
    unsigned long long field_stride, uint32_t field_per_group, uint32_t *__restrict__ weights,
    unsigned long long weight_stride, uint32_t *__restrict__ result, uint32_t *__restrict__ status,
    uint32_t *__restrict__ counts, unsigned long long count_stride, uint32_t *__restrict__ mask,
    unsigned long long mask_words_stride) {
  __shared__ f32x4 s_pts[kFrontList / 2u];  // two points (x0, y0, x1, y1) per element
  __shared__ uint32_t s_idx[kFrontList];       // the sample index of every list entry
  __shared__ uint32_t s_agree[kFrontList];     // the poses of this tile that agree with it
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
  uint32_t *cnt_row = counts + (size_t)sc * count_stride;
  uint32_t *fin_row = tile == 0u ? mask + (size_t)sc * mask_words_stride : nullptr;
  uint32_t acc = 0u;
  uint32_t finite = 0u;
  bool cell_range = false;
  uint32_t pass = 0u;
  float2 *pts = reinterpret_cast<float2 *>(s_pts);
  // a thread zeroes and flushes the same two counters, t and t + kBlock: no barrier between a flush and the reset
  s_agree[threadIdx.x] = 0u;
  s_agree[threadIdx.x + kBlock] = 0u;
  for (uint32_t base = blockIdx.z * kFrontList; base < n; base += gridDim.z * kFrontList) {
    uint32_t *cnt_at = &s_cnt[pass++ & 1u];
    if (threadIdx.x == 0) *cnt_at = 0u;
    __syncthreads();  // (also: the last pass's readers are done with the list, its flush with the indices)
    front_point_pass<FAST>(f, base, p, cnt_at, pts, s_idx, fin_row, nullptr, &finite);
    __syncthreads();
    const uint32_t cnt = *cnt_at;  // <= kFrontList
    if (l.slice < l.slices) {      // (wave-uniform: the ballots below see whole waves)
      // copy `slice` walks the point pairs slice, slice + slices, ...: pair e holds points 2e and 2e + 1 < kFrontList
      // (not unrolled: the ballots are convergent operations)
      for (uint32_t e = l.slice; 2u * e < cnt; e += l.slices) {
        const f32x4 v = s_pts[e];
        uint32_t f0 = 0u, f1 = 0u;
        if (l.own) {
          f0 = pose_look(v.x, v.y, l.c, l.s, l.tx, l.ty, ck, fld, &cell_range);
          if (2u * e + 1u < cnt) f1 = pose_look(v.z, v.w, l.c, l.s, l.tx, l.ty, ck, fld, &cell_range);
        }
        acc += f0 + f1;
        // a lane without a pose has f = 0 < agree_lo; so has the missing second point of the last pair
        const unsigned long long m0 = __ballot(l.own && f0 >= k.agree_lo);
        const unsigned long long m1 = __ballot(l.own && f1 >= k.agree_lo);
        if (lane_id() == 0) {
          if (m0) atomicAdd(&s_agree[2u * e], (uint32_t)__popcll(m0));
          if (m1) atomicAdd(&s_agree[2u * e + 1u], (uint32_t)__popcll(m1));
        }
      }
    }
    __syncthreads();
    // the pass's counters leave: entry j < cnt <= kFrontList has sample s_idx[j] < n <= n_stride <= count_stride
#pragma unroll
    for (uint32_t j = threadIdx.x; j < kFrontList; j += kBlock) {
      const uint32_t c = s_agree[j];
      if (j < cnt && c) {
        atomicAdd(&cnt_row[s_idx[j]], c);
        s_agree[j] = 0u;
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

constexpr uint32_t kDecideThreads = 256;

// grid (B, ceil(n_stride / 256)): thread i of scan sc
__global__ __launch_bounds__(kDecideThreads) void k_agree_decide(
    uint32_t n_stride, uint32_t group, uint32_t P, uint32_t keep_num, uint32_t keep_den,
    const uint32_t *__restrict__ counts, unsigned long long count_stride, uint32_t *__restrict__ mask,
    unsigned long long mask_words_stride, uint32_t *__restrict__ agree) {
  const uint32_t sc = blockIdx.x;
  const uint32_t g = sc / group;
  const uint32_t i = blockIdx.y * kDecideThreads + threadIdx.x;  // (a wave: 64 samples from a multiple of 64)
  uint32_t *row = mask + (size_t)sc * mask_words_stride;
  uint32_t c = 0u;
  bool fin = false;
  if (i < n_stride) {
    c = counts[(size_t)sc * count_stride + i];
    fin = (row[i >> 5] >> (i & 31u)) & 1u;  // the finite bit, k_agree_count's
  }
  const bool kept = fin && (unsigned long long)c * keep_den > (unsigned long long)keep_num * P;
  const unsigned long long mf = __ballot(fin), mk = __ballot(kept);
  // the wave's two mask words: finite AND kept (the loads above are done: the ballot needed them)
  const uint32_t w0 = (i - lane_id()) >> 5;
  if (lane_id() == 0 && w0 * 32u < n_stride) row[w0] = (uint32_t)mk;
  if (lane_id() == 32 && (w0 + 1u) * 32u < n_stride) row[w0 + 1u] = (uint32_t)(mk >> 32);
  uint32_t hi = c, lo = fin ? c : 0xFFFFFFFFu, sum = c;  // sum <= 64 x 2^20
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    hi = max(hi, (uint32_t)__shfl_xor(hi, d, 64));
    lo = min(lo, (uint32_t)__shfl_xor(lo, d, 64));
    sum += __shfl_xor(sum, d, 64);
  }
  if (lane_id() == 0 && (mf || sum)) {
    uint32_t *out = agree + 8u * (size_t)g;
    if (mf) {
      atomicAdd(&out[0], (uint32_t)__popcll(mf));
      atomicMin(&out[5], lo);
    }
    if (mk) atomicAdd(&out[1], (uint32_t)__popcll(mk));
    if (sum) {
      atomicMax(&out[4], hi);
      const uint32_t old = atomicAdd(&out[6], sum);  // 64 bits in two words: the carry by the returned value
      if (old + sum < old) atomicAdd(&out[7], 1u);
    }
  }
}

__global__ __launch_bounds__(kDecideThreads) void k_agree_flag(uint32_t G, uint32_t err_num, uint32_t err_den,
                                                               uint32_t *__restrict__ agree) {
  const uint32_t g = blockIdx.x * kDecideThreads + threadIdx.x;
  if (g >= G) return;
  uint32_t *out = agree + 8u * (size_t)g;
  const uint32_t F = out[0], K = out[1];
  const bool back = F > 0u && (unsigned long long)(F - K) * err_den >= (unsigned long long)err_num * F;
  out[2] = back ? 1u : 0u;
  out[3] = back ? F : K;
  if (F == 0u) out[5] = 0u;
}

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_agree_apply(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan, uint32_t group,
    KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, AgreeK k, const float *__restrict__ poses,
    uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group, const int8_t *__restrict__ field,
    unsigned long long field_stride, uint32_t field_per_group, uint32_t *__restrict__ weights,
    unsigned long long weight_stride, const uint32_t *__restrict__ mask, unsigned long long mask_words_stride,
    const uint32_t *__restrict__ agree) {
  __shared__ f32x4 s_pts[kFrontList / 2u];
  __shared__ uint32_t s_sum[kBlock];
  __shared__ uint32_t s_cnt[2];
  const uint32_t sc = blockIdx.x;
  const uint32_t tile = blockIdx.y;
  const uint32_t g = sc / group;
  if (agree[8u * (size_t)g + 2u]) return;  // (block-uniform) the group fell back: every finite sample stays in
  const uint32_t n = scan_len(n_per_scan[sc], n_stride);
  if (blockIdx.z * kFrontList >= n) return;  // (block-uniform)
  const ScanFront f = scan_front(nodes, n_stride, sc, n, p, T, keepmask, mask_stride, motion, pose2d);
  const OccK ck{k.origin_x, k.origin_y, k.resolution, k.width, k.height, 0.0f, 0.0f, 0.0f};
  const int8_t *fld = field + (size_t)(field_per_group ? g : 0u) * field_stride;
  const PoseLane l = pose_lane(tile, P, poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
  const uint32_t *rule_row = mask + (size_t)sc * mask_words_stride;
  uint32_t acc = 0u;
  uint32_t finite = 0u;
  bool cell_range = false;  // (the count pass has reported it)
  uint32_t pass = 0u;
  float2 *pts = reinterpret_cast<float2 *>(s_pts);
  for (uint32_t base = blockIdx.z * kFrontList; base < n; base += gridDim.z * kFrontList) {
    uint32_t *cnt_at = &s_cnt[pass++ & 1u];
    if (threadIdx.x == 0) *cnt_at = 0u;
    __syncthreads();
    front_point_pass<FAST>(f, base, p, cnt_at, pts, nullptr, nullptr, rule_row, &finite);
    __syncthreads();
    const uint32_t cnt = *cnt_at;  // the skipped samples of the pass: usually none
    if (l.own) {
#pragma unroll 2
      for (uint32_t e = l.slice; 2u * e < cnt; e += l.slices) {
        const f32x4 v = s_pts[e];
        acc += pose_look(v.x, v.y, l.c, l.s, l.tx, l.ty, ck, fld, &cell_range);
        if (2u * e + 1u < cnt) acc += pose_look(v.z, v.w, l.c, l.s, l.tx, l.ty, ck, fld, &cell_range);
      }
    }
  }
  if (!__syncthreads_or(acc != 0u)) return;  // nothing to take off
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < l.per && tile * kPoseTile + threadIdx.x < P) {
    uint32_t sum = 0u;
    for (uint32_t s = 0; s < l.slices; ++s) sum += s_sum[s * l.per + threadIdx.x];
    // what the count pass added for these samples at this pose: the weight holds at least that
    if (sum) atomicSub(&weights[(size_t)g * weight_stride + tile * kPoseTile + threadIdx.x], sum);
  }
}

bool agree_args_ok(const AgreeK &k, uint32_t P) {
  return k.width != 0 && k.height != 0 && k.width <= RPLGPU_MAX_OCC_DIM && k.height <= RPLGPU_MAX_OCC_DIM &&
         P != 0 && P <= RPLGPU_MAX_POSES && k.agree_lo >= 1u && k.agree_lo <= 127u && k.keep_den != 0 &&
         k.keep_den <= RPLGPU_AGREE_MAX_DEN && k.keep_num <= k.keep_den && k.err_den != 0 &&
         k.err_den <= RPLGPU_AGREE_MAX_DEN && k.err_num <= RPLGPU_AGREE_MAX_DEN;
}

}  // namespace

hipError_t launch_agree(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan, uint32_t B,
                        uint32_t group, uint32_t G, const KParams &p, const Tables &T, const uint32_t *keepmask,
                        uint32_t mask_stride, const float *motion, const float *pose2d, const AgreeK &k,
                        const float *poses, uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group,
                        const int8_t *field, unsigned long long field_stride, uint32_t field_per_group,
                        uint32_t *weights, unsigned long long weight_stride, uint32_t *result, uint32_t *status,
                        uint32_t *counts, unsigned long long count_stride, uint32_t *mask,
                        unsigned long long mask_words_stride, uint32_t *agree) {
  if (B == 0) return hipSuccess;
  const uint32_t mask_words = (n_stride + 31u) / 32u;
  if (group == 0 || G == 0 || (unsigned long long)G * group < B || (unsigned long long)(G - 1u) * group >= B ||
      !agree_args_ok(k, P) || field_stride < (unsigned long long)k.width * k.height || pose_stride < 4ull * P ||
      (pose_stride & 3u) || weight_stride < P || n_stride == 0 || n_stride > kMaxN ||
      count_stride < n_stride || mask_words_stride < mask_words)
    return hipErrorInvalidValue;
  const unsigned long long words = std::max<unsigned long long>((unsigned long long)G * P, (unsigned long long)B * n_stride);
  const uint32_t prep = (uint32_t)std::min<unsigned long long>((words + kPrepThreads - 1u) / kPrepThreads, kPrepBlocks);
  hipLaunchKernelGGL(k_agree_prepare, dim3(prep), dim3(kPrepThreads), 0, s, weights, weight_stride, G, P, result,
                     counts, count_stride, B, n_stride, mask, mask_words_stride, mask_words, agree);
  // slices of a scan's passes, as launch_pose_score
  const uint32_t passes = (n_stride + kFrontList - 1u) / kFrontList;
  const dim3 grid(B, (P + kPoseTile - 1u) / kPoseTile, std::min(passes, 8u));
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_agree_count<true>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride, poses_per_group,
                       field, field_stride, field_per_group, weights, weight_stride, result, status, counts,
                       count_stride, mask, mask_words_stride);
  else
    hipLaunchKernelGGL(k_agree_count<false>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride, poses_per_group,
                       field, field_stride, field_per_group, weights, weight_stride, result, status, counts,
                       count_stride, mask, mask_words_stride);
  hipLaunchKernelGGL(k_agree_decide, dim3(B, (n_stride + kDecideThreads - 1u) / kDecideThreads),
                     dim3(kDecideThreads), 0, s, n_stride, group, P, k.keep_num, k.keep_den, counts, count_stride,
                     mask, mask_words_stride, agree);
  hipLaunchKernelGGL(k_agree_flag, dim3((G + kDecideThreads - 1u) / kDecideThreads), dim3(kDecideThreads), 0, s, G,
                     k.err_num, k.err_den, agree);
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_agree_apply<true>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride, poses_per_group,
                       field, field_stride, field_per_group, weights, weight_stride, mask, mask_words_stride, agree);
  else
    hipLaunchKernelGGL(k_agree_apply<false>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride, poses_per_group,
                       field, field_stride, field_per_group, weights, weight_stride, mask, mask_words_stride, agree);
  return hipGetLastError();
}

}  // namespace rpl
