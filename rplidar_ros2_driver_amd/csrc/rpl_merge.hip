// rpl_merge.hip — E9: the scans of a group (the sensors of one time step) merged into ONE LaserScan in
// the common frame (include/rplgpu_msg.h, rplgpu_merge_scans_dev).
//
// k_merge_scans: one 1024-thread workgroup per scan.  The scan is opened by rpl_front.hpp (scan_front, scan_pair:
// two consecutive samples per buffer_load_dwordx4, the E1 / E5 keep bits), a kept sample runs E2 with the
// (cos, sin) table, then E6 + the planar pose through rpl_xf.hpp's sample_xy — the front end of E8, so a
// point lands where rplgpu_cloud_fused_voxel_dev puts it, bit for bit.  The beam comes from
// the exact side tests of the spec (merge_bin), the reduction is a 64-bit min over
//   key = r2 bits << 32 | slot in group << 15 | sample index
// in LDS (ds_min_u64: r2 >= 0, so its bits order like the value; ties go to the first point in
// acquisition order), and one pass flushes the beams the scan hit into its group's key row with a
// global 64-bit atomic min.  k_merge_finish turns the key rows into ranges / intensities (the winner's
// quality byte is read back by its index), counts the hit beams and resets the rows for the next launch.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_front.hpp"
#include "rpl_msg.hpp"

namespace rpl {
namespace {

constexpr unsigned long long kEmptyBeam = ~0ull;

// cross_k(p) >= 0: the products of two float32 values are exact in fp64 and the difference is rounded
// once, so the sign is exact (-ffp-contract=off keeps the three operations apart)
__device__ __forceinline__ bool on_left(float2 e, float x, float y) {
  const double a = (double)e.x * (double)y;
  const double b = (double)e.y * (double)x;
  return a - b >= 0.0;
}

// The beam of the spec: the smallest k in [0, count) with cross_k >= 0 && cross_k+1 < 0, or -1.
// monotone (host-checked: every step e_k -> e_k+1 and every quarter [qb[q], qb[q+1]] turns by an angle
// in (0, pi)): inside a quarter the sign sequence is 1 .. 1 0 .. 0, so the quarter holds a transition
// iff its first edge says 1 and its last 0 — and then exactly one.  The first such quarter therefore
// holds the smallest k (on a full circle the wrap sliver lies in quarter 0 AND quarter 3: quarter 0
// wins, as the rule says), a point in no quarter has no beam, and a bisection with the invariant
// sign(lo) = 1, sign(hi) = 0 finds the transition in at most log2(count / 4) + 1 steps.  The atan2f
// guess only seeds the bisection (two tests; right nearly always): a wrong guess costs steps, never
// the bin.  Not monotone (inc below ~1e-7 rad, where rounding the edges to float can turn a step
// backwards): the documented fallback, a linear walk over every edge.
__device__ __forceinline__ int merge_bin(float x, float y, const MergeK &mk) {
  if (!mk.monotone) {
    bool s = on_left(mk.edges[0], x, y);
    for (uint32_t k = 0; k < mk.count; ++k) {
      const bool s1 = on_left(mk.edges[k + 1], x, y);
      if (s && !s1) return (int)k;
      s = s1;
    }
    return -1;
  }
  bool s = on_left(mk.qe[0], x, y);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (mk.qb[q] == mk.qb[q + 1]) continue;  // (empty quarter: same edge, same sign)
    const bool s1 = on_left(mk.qe[q + 1], x, y);
    if (s && !s1) {
      uint32_t lo = mk.qb[q], hi = mk.qb[q + 1];
      float rel = atan2f(y, x) - mk.a0;
      if (rel < 0.0f) rel += 6.2831855f;
      if (rel < 0.0f) rel += 6.2831855f;
      const float t = rel * mk.rinc;
      const uint32_t g = (t >= 0.0f && t < 16777216.0f) ? (uint32_t)t : 0u;
      if (g > lo && g < hi) {
        if (on_left(mk.edges[g], x, y)) lo = g; else hi = g;
      }
      if (g + 1u > lo && g + 1u < hi) {
        if (on_left(mk.edges[g + 1u], x, y)) lo = g + 1u; else hi = g + 1u;
      }
      while (hi - lo > 1u) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (on_left(mk.edges[m], x, y)) lo = m; else hi = m;
      }
      return (int)lo;
    }
    s = s1;
  }
  return -1;
}

template <bool FAST>
__device__ __forceinline__ void merge_sample(uint32_t lo, uint32_t hi, uint32_t i, bool kept,
                                             const float2 *__restrict__ cs, const ScanXf &xf,
                                             const MergeK &mk, unsigned long long slot_bits,
                                             unsigned long long *s_key) {
  if (!kept) return;
  const f2 xy = sample_xy<FAST>(lo, hi, i, cs, xf);  // E2, E6 + pose (rpl_xf.hpp)
  const float r2 = xy.x * xy.x + xy.y * xy.y;
  const float r = sqrtf(r2);
  if (!(r >= mk.range_min && r <= mk.range_max)) return;
  const int k = merge_bin(xy.x, xy.y, mk);
  if (k < 0) return;
  atomicMin(&s_key[k], ((unsigned long long)__float_as_uint(r2) << 32) | slot_bits | i);
}

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_merge_scans(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan,
    uint32_t group, KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, MergeK mk,
    unsigned long long *__restrict__ keys, uint32_t *__restrict__ status) {
  __shared__ unsigned long long s_key[kMergeMaxBeams];
  const uint32_t sc = blockIdx.x;
  const uint32_t g = sc / group, slot = sc - g * group;
  for (uint32_t j = threadIdx.x; j < mk.count; j += kBlock) s_key[j] = kEmptyBeam;
  const uint32_t n_in = n_per_scan[sc];
  const uint32_t n = scan_len(n_in, n_stride);
  if (threadIdx.x == 0 && status && n_in > n) atomicOr(&status[g], RPLGPU_SCAN_OUT_TRUNCATED);
  const ScanFront f = scan_front(nodes, n_stride, sc, n, p, T, keepmask, mask_stride, motion, pose2d);
  const unsigned long long slot_bits = (unsigned long long)slot << 15;
  __syncthreads();
  for (uint32_t pr = threadIdx.x; 2u * pr < n; pr += kBlock) {
    const ScanPair s = scan_pair(f, p, pr);
    merge_sample<FAST>(s.t.x, s.t.y, s.i0, s.k0, f.cs, f.sd.xf, mk, slot_bits, s_key);
    merge_sample<FAST>(s.t.z, s.t.w, s.i1, s.k1, f.cs, f.sd.xf, mk, slot_bits, s_key);
  }
  __syncthreads();
  unsigned long long *row = keys + (size_t)g * mk.count;
  for (uint32_t j = threadIdx.x; j < mk.count; j += kBlock) {
    const unsigned long long k = s_key[j];
    if (k != kEmptyBeam) atomicMin(&row[j], k);
  }
}

constexpr uint32_t kFinishThreads = 256;

__global__ __launch_bounds__(kFinishThreads) void k_merge_finish(
    unsigned long long *__restrict__ keys, uint32_t count, uint32_t blocks_per_row,
    const uint2 *__restrict__ nodes, uint32_t n_stride, uint32_t group, int is_new_protocol,
    float *__restrict__ ranges, float *__restrict__ intens, uint32_t *__restrict__ beams_hit) {
  const uint32_t g = blockIdx.x / blocks_per_row;
  const uint32_t j = (blockIdx.x - g * blocks_per_row) * kFinishThreads + threadIdx.x;
  bool hit = false;
  if (j < count) {
    const size_t o = (size_t)g * count + j;
    const unsigned long long k = keys[o];
    float r = __builtin_inff(), in = 0.0f;  // an empty beam, as publish_scan fills it (:640-641)
    if (k != kEmptyBeam) {
      hit = true;
      r = sqrtf(__uint_as_float((uint32_t)(k >> 32)));
      const uint32_t slot = (uint32_t)(k >> 15) & ((1u << kMergeSlotBits) - 1u);
      const uint32_t i = (uint32_t)k & 0x7FFFu;
      const uint2 nd = nodes[((size_t)g * group + slot) * n_stride + i];
      in = nd_intensity(nd_quality(nd), is_new_protocol);
      keys[o] = kEmptyBeam;  // the row is clean for the next launch
    }
    ranges[o] = r;
    intens[o] = in;
  }
  const unsigned long long b = __ballot(hit);
  if (lane_id() == 0 && b) atomicAdd(&beams_hit[g], (uint32_t)__popcll(b));
}

constexpr uint32_t kMsgThreads = 256;
constexpr uint32_t kChunk = 16384;  // dwords per workgroup

// The prefix carries every scalar and the ranges length word (the same for all G messages); a message
// differs from the next only by its stamp and its arrays.
__global__ __launch_bounds__(kMsgThreads) void k_msg_merged(
    const float *__restrict__ ranges, const float *__restrict__ intens, uint32_t count,
    const rplgpu_stamp_t *__restrict__ stamps, rplmsg::Prefix P, uint8_t *__restrict__ msgs,
    uint32_t msg_stride, uint32_t *__restrict__ msg_len, uint32_t *__restrict__ status) {
  const uint32_t b = blockIdx.y;
  const uint64_t total = (uint64_t)P.len + 8ull * count + 4ull;
  const bool fits = total <= msg_stride;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    msg_len[b] = fits ? (uint32_t)total : 0u;
    if (status && !fits) atomicOr(&status[b], RPLGPU_SCAN_OUT_TRUNCATED);
  }
  if (!fits) return;
  uint32_t *msg = reinterpret_cast<uint32_t *>(msgs + (size_t)b * msg_stride);
  if (blockIdx.x == 0) {
    for (uint32_t i = threadIdx.x; i < P.len / 4; i += kMsgThreads) msg[i] = P.words[i];
    __syncthreads();  // the stamp patch overwrites template words
    if (threadIdx.x == 0) {
      msg[P.stamp_off / 4] = (uint32_t)stamps[b].sec;
      msg[P.stamp_off / 4 + 1] = stamps[b].nanosec;
      msg[P.len / 4 + count] = count;  // intensities length word, right after ranges
    }
  }
  const float *r = ranges + (size_t)b * count;
  const float *q = intens + (size_t)b * count;
  uint32_t *out = msg + P.len / 4;
  for (uint32_t first = blockIdx.x * kChunk; first < 2u * count; first += gridDim.x * kChunk) {
    const uint32_t last = min(first + kChunk, 2u * count);
    for (uint32_t j = first + threadIdx.x; j < last; j += kMsgThreads) {
      if (j < count)
        out[j] = __float_as_uint(r[j]);
      else
        out[j + 1] = __float_as_uint(q[j - count]);
    }
  }
}

}  // namespace

hipError_t launch_merge_scans(hipStream_t s, const void *nodes, uint32_t n_stride,
                              const uint32_t *n_per_scan, uint32_t B, uint32_t group, const KParams &p,
                              const Tables &T, const uint32_t *keepmask, uint32_t mask_stride,
                              const float *motion, const float *pose2d, const MergeK &mk,
                              unsigned long long *keys, uint32_t *status) {
  if (B == 0) return hipSuccess;
  if (group == 0 || group > (1u << kMergeSlotBits) || mk.count == 0 || mk.count > kMergeMaxBeams)
    return hipErrorInvalidValue;
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_merge_scans<true>, dim3(B), dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride,
                       n_per_scan, group, p, T, keepmask, mask_stride, motion, pose2d, mk, keys, status);
  else
    hipLaunchKernelGGL(k_merge_scans<false>, dim3(B), dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride,
                       n_per_scan, group, p, T, keepmask, mask_stride, motion, pose2d, mk, keys, status);
  return hipGetLastError();
}

hipError_t launch_merge_finish(hipStream_t s, unsigned long long *keys, uint32_t G, uint32_t count,
                               const void *nodes, uint32_t n_stride, uint32_t group, int is_new_protocol,
                               float *ranges, float *intens, uint32_t *beams_hit) {
  if (G == 0) return hipSuccess;
  const uint32_t per_row = (count + kFinishThreads - 1u) / kFinishThreads;
  hipLaunchKernelGGL(k_merge_finish, dim3(G * per_row), dim3(kFinishThreads), 0, s, keys, count, per_row,
                     (const uint2 *)nodes, n_stride, group, is_new_protocol, ranges, intens, beams_hit);
  return hipGetLastError();
}

hipError_t launch_msg_merged(hipStream_t s, const float *ranges, const float *intens, uint32_t count,
                             uint32_t G, const rplgpu_stamp_t *stamps, const rplmsg::Prefix &P,
                             uint8_t *msgs, uint32_t msg_stride, uint32_t *msg_len, uint32_t *status) {
  if (G == 0) return hipSuccess;
  const uint32_t gx = min((2u * count + kChunk - 1) / kChunk, 4u);
  for (uint32_t b0 = 0; b0 < G; b0 += 65535u) {  // gridDim.y limit
    const uint32_t nb = min(G - b0, 65535u);
    hipLaunchKernelGGL(k_msg_merged, dim3(gx ? gx : 1, nb), dim3(kMsgThreads), 0, s,
                       ranges + (size_t)b0 * count, intens + (size_t)b0 * count, count, stamps + b0, P,
                       msgs + (size_t)b0 * msg_stride, msg_stride, msg_len + b0,
                       status ? status + b0 : nullptr);
  }
  return hipGetLastError();
}

}  // namespace rpl
