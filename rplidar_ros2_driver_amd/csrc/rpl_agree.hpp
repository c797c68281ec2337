// rpl_agree.hpp — E23 (include/rplgpu_msg.h, rplgpu_score_poses_agree_dev): the launchers of rpl_agree.hip and the
// front end its two walking kernels share.
//
// The front end is k_pose_score's (rpl_pose.hip), operation for operation: two nodes per bounds-checked
// buffer_load_dwordx4, the E1 / E5 keep bits, the (cos, sin) table, rpl_xf.hpp's sample_xy, the finite test and the
// compaction into an LDS list with one atomic per wave — so a point lands where E15 puts it, bit for bit.  What it
// adds: the sample index kept beside every list entry, the finite bits of a wave's 128 samples stored as four mask
// words, and a second keep test against the rule's mask (the apply pass lists only the skipped samples).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_grid.hpp"
#include "rpl_xf.hpp"

namespace rpl {

struct AgreeK {  // a checked rplgpu_beam_agree_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  uint32_t agree_lo;
  uint32_t keep_num, keep_den, err_num, err_den;
};

// E23, five kernels on the stream between the scan prologue and launch_pose_best: prepare (every output word
// zeroed, the smallest count started at ~0), count (E15's sums and the per-sample counts from one field load, the
// finite bits, result word 4), decide (the rule bit per sample ANDed into the mask, F, K, the largest, smallest and
// summed count), flag (agree words 2, 3 and 5), apply (the skipped samples' sums taken off the weights again, unless
// the group fell back).  counts: count_stride >= n_stride words per scan; mask: mask_words_stride >=
// ceil(n_stride / 32) words per scan; agree: eight words per group.
hipError_t launch_agree(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan, uint32_t B,
                        uint32_t group, uint32_t G, const KParams &p, const Tables &T, const uint32_t *keepmask,
                        uint32_t mask_stride, const float *motion, const float *pose2d, const AgreeK &k,
                        const float *poses, uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group,
                        const int8_t *field, unsigned long long field_stride, uint32_t field_per_group,
                        uint32_t *weights, unsigned long long weight_stride, uint32_t *result, uint32_t *status,
                        uint32_t *counts, unsigned long long count_stride, uint32_t *mask,
                        unsigned long long mask_words_stride, uint32_t *agree);

#if defined(__HIPCC__)
typedef uint32_t ag_u32x4 __attribute__((ext_vector_type(4)));
typedef float ag_f32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kAgList = 2u * kBlock;  // points per pass: two samples per thread
constexpr uint32_t kAgTile = kBlock;       // poses per workgroup: one per thread

// the 16 low bits of x moved to the even bit positions
__device__ __forceinline__ uint32_t agree_spread16(uint32_t x) {
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  return (x | (x << 1)) & 0x55555555u;
}

// E15's field value under the cell of (c*x - s*y + tx, s*x + c*y + ty), rpl_pose.hip's pose_look
__device__ __forceinline__ uint32_t agree_look(float x, float y, float c, float s, float tx, float ty, const OccK &k,
                                               const int8_t *__restrict__ field, bool *cell_range) {
  const float rx = (c * x - s * y) + tx;
  const float ry = (s * x + c * y) + ty;
  int cx, cy;
  if (!grid_cell(rx, ry, k.origin_x, k.origin_y, k.resolution, &cx, &cy)) {
    *cell_range = true;
    return 0u;
  }
  if ((uint32_t)cx >= k.width || (uint32_t)cy >= k.height) return 0u;
  const int v = field[(uint32_t)cy * k.width + (uint32_t)cx];
  return (uint32_t)max(v, 0);
}

// One pass of one workgroup: the samples [base, base + kAgList) of a scan of n samples behind `rsrc` (bounds-checked
// over n * 8 bytes), two per thread, through E1 / E5 / E2 / E6 / the mount pose and the finite test into the LDS list
// pts[0 .. *cnt_at), a wave's points together and in sample order.  *cnt_at is 0 on entry (reset before the barrier
// in front of this call); the caller puts a barrier behind it.
//   idx      (optional, LDS)   the sample index of every list entry
//   fin_row  (optional, global) the scan's mask row: the finite bits of the wave's 128 samples are stored as whole
//            words (a word belongs to one wave of one workgroup; words without a sample below n are left alone)
//   rule_row (optional, global) the scan's mask row after the decision: only the finite samples whose bit is 0 are
//            listed (the skipped ones)
//   *finite  the thread's finite samples are added
template <bool FAST>
__device__ __forceinline__ void agree_front_pass(const __amdgpu_buffer_rsrc_t rsrc, uint32_t n, uint32_t base,
                                                 const KParams &p, uint32_t q_min16, const float2 *__restrict__ cs,
                                                 const ScanSide &sd, uint32_t *cnt_at, float2 *pts, uint32_t *idx,
                                                 uint32_t *__restrict__ fin_row,
                                                 const uint32_t *__restrict__ rule_row, uint32_t *finite) {
  const uint32_t pr = base / 2u + threadIdx.x;
  if (2u * pr < n) {  // (the active lanes of a wave are its first ones)
    const ag_u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(pr * 16u), 0, 0);
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
    f2 a = {0.0f, 0.0f}, b = {0.0f, 0.0f};
    if (k0) {
      a = sample_xy<FAST>(t.x, t.y, i0, cs, sd.xf);
      k0 = fabsf(a.x) < __builtin_huge_valf() && fabsf(a.y) < __builtin_huge_valf();
    }
    if (k1) {
      b = sample_xy<FAST>(t.z, t.w, i1, cs, sd.xf);
      k1 = fabsf(b.x) < __builtin_huge_valf() && fabsf(b.y) < __builtin_huge_valf();
    }
    *finite += (k0 ? 1u : 0u) + (k1 ? 1u : 0u);
    if (fin_row) {  // (workgroup-uniform) lane w of the wave's first four stores word w of its 128 samples
      const unsigned long long f0 = __ballot(k0), f1 = __ballot(k1);
      const uint32_t w = lane_id() & 3u;
      const uint32_t word = agree_spread16((uint32_t)(f0 >> (16u * w)) & 0xFFFFu) |
                            (agree_spread16((uint32_t)(f1 >> (16u * w)) & 0xFFFFu) << 1);
      const uint32_t at_word = (i0 - 2u * lane_id()) / 32u + w;  // (i0 - 2 lane: the wave's first sample, a multiple of 128)
      if (lane_id() < 4u && at_word * 32u < n) fin_row[at_word] = word;  // < ceil(n / 32) <= the row's words
    }
    if (rule_row) {  // (workgroup-uniform) i1 <= n - 1 or dropped: the word lies inside the row
      const uint32_t w = rule_row[i0 >> 5];
      k0 = k0 && !((w >> (i0 & 31u)) & 1u);
      k1 = k1 && !((w >> (i1 & 31u)) & 1u);
    }
    // one LDS atomic per wave: the wave's points stay together in the list, in sample order
    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
    const unsigned long long below = (1ull << lane_id()) - 1ull;
    uint32_t at = 0u;
    if (lane_id() == 0) at = atomicAdd(cnt_at, (uint32_t)(__popcll(m0) + __popcll(m1)));
    at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at) + (uint32_t)(__popcll(m0 & below) + __popcll(m1 & below));
    if (k0) {  // at + 1 <= the wave's share: < kAgList
      pts[at] = make_float2(a.x, a.y);
      if (idx) idx[at] = i0;
    }
    if (k1) {
      pts[at + (k0 ? 1u : 0u)] = make_float2(b.x, b.y);
      if (idx) idx[at + (k0 ? 1u : 0u)] = i1;
    }
  }
}
#endif  // __HIPCC__

}  // namespace rpl
