// rpl_front.hpp — the scan front end that the streaming stages from E9 on share, one copy of each step: E9
// (rpl_merge.hip), E13 (rpl_match.hip), E14 (rpl_map.hip), E15 (rpl_pose.hip), E23 (rpl_agree.hip), E24 (rpl_wide.hip)
// and E25 (rpl_refine.hip) open a scan through this file, so a point lands where E8, E9 and E11 put it, bit for bit,
// because it is the same code.  E11's k_occ_walk (rpl_occ.hip) holds the same steps written out, for a measured reason
// that its header gives: a change here has to be repeated there.
//   scan_len          the clamped length of a scan;
//   scan_front        what a workgroup knows about its scan: that length, the bounds-checked buffer resource, the E1
//                     quality bound, the (cos, sin) table, rpl_xf.hpp's ScanSide;
//   scan_pair         two nodes per buffer_load_dwordx4 and their E1 (AND E5) keep bits;
//   wave_slot         a lane's place in an LDS list: two ballots, one atomic per wave (k_map_walk writes its own out);
//   front_point_pass  2048 samples to an LDS list of finite points (E15, E23, E25);
//   front_cell_pass   2048 samples to an LDS list of weighted cells (E13, E24);
//   pose_lane         the pose of a thread of a 1024-pose tile (E15, E23, E25).
// The field look-ups behind the lists are rpl_grid.hpp's.  rpl_voxel.hip, rpl_ror.hip, rpl_laserscan.hip and
// rpl_kernels.hip stream their samples in loops of another kind and do not come through here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_grid.hpp"
#include "rpl_ray.hpp"  // run_behind
#include "rpl_xf.hpp"

namespace rpl {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kFrontList = 2u * kBlock;  // samples, and so list entries at the most, per pass: two per thread
constexpr uint32_t kPoseTile = kBlock;        // poses per workgroup: one per thread

// ---- the scan set-up ------------------------------------------------------------------------------------------------
struct ScanFront {
  __amdgpu_buffer_rsrc_t rsrc;  // bounds-checked over the scan's n * 8 bytes: a node beyond it reads as zero
  uint32_t n;                   // the samples taken: scan_len of the scan, and what rsrc is bounds-checked over
  uint32_t q_min16;             // the E1 quality bound at the quality byte's place in a node's high dword
  const float2 *cs;
  ScanSide sd;
};
// the samples a kernel takes of a scan: n_in clamped to the stride and to kMaxN (wave-uniform).  Apart from scan_front,
// so that a workgroup with nothing to do (a slice of passes beyond n, a rotation without a listed block) can leave
// before the loads of the scan's side are issued, as every kernel here did before it called this file.
__device__ __forceinline__ uint32_t scan_len(uint32_t n_in, uint32_t n_stride) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)min(n_in, min(n_stride, kMaxN)));
}
// n MUST be scan_len(n_per_scan[sc], n_stride): it becomes f.n, the bound of every `i < f.n` test, and n * 8 bytes is
// the size the buffer resource checks the loads against; nothing else ties the two together.
__device__ __forceinline__ ScanFront scan_front(const uint2 *__restrict__ nodes, uint32_t n_stride, uint32_t sc,
                                                uint32_t n, const KParams &p, const Tables &T,
                                                const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
                                                const float *__restrict__ motion, const float *__restrict__ pose2d) {
  ScanFront f;
  f.n = n;
  f.sd = scan_side(sc, keepmask, mask_stride, motion, pose2d, T.scan_t0);
  f.cs = p.inverted ? T.cs_inv : T.cs;
  f.q_min16 = p.clip_enable ? (min(p.q_min, 256u) << 16) : 0u;
  f.rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(nodes + (size_t)sc * n_stride), 0, (int)(n * 8u), 0x00020000);
  return f;
}

// ---- the pair load and the keep bits --------------------------------------------------------------------------------
// Pair pr (2 pr < n): the samples i0 = 2 pr and i1 = i0 + 1 as the four dwords of one load, and whether E1, ANDed with
// E5 where the scan has keep bits (launch_ror_mask), keeps them.  i1 = n reads as zero and is dropped.
struct ScanPair {
  u32x4 t;  // (lo, hi) of i0, (lo, hi) of i1
  uint32_t i0, i1;
  bool k0, k1;
};
__device__ __forceinline__ ScanPair scan_pair(const ScanFront &f, const KParams &p, uint32_t pr) {
  ScanPair s;
  s.t = __builtin_amdgcn_raw_buffer_load_b128(f.rsrc, (int)(pr * 16u), 0, 0);
  s.i0 = 2u * pr;
  s.i1 = s.i0 + 1u;
  s.k0 = s.i0 < f.n && (__builtin_amdgcn_alignbit(s.t.y, s.t.x, 16) - p.d_lo) <= p.d_span &&
         (s.t.y & 0x00FF0000u) >= f.q_min16;  // E1
  s.k1 = s.i1 < f.n && (__builtin_amdgcn_alignbit(s.t.w, s.t.z, 16) - p.d_lo) <= p.d_span &&
         (s.t.w & 0x00FF0000u) >= f.q_min16;
  if (f.sd.ror_bits) {  // E1 AND E5; both samples sit in one word (i0 is even)
    const uint32_t w = f.sd.ror_bits[s.i0 >> 5];
    s.k0 = s.k0 && ((w >> (s.i0 & 31u)) & 1u);
    s.k1 = s.k1 && ((w >> (s.i1 & 31u)) & 1u);
  }
  return s;
}

// ---- the wave compaction --------------------------------------------------------------------------------------------
// The list place of a lane's first listed sample (its second one follows it): one LDS atomic per wave, so the wave's
// entries stay together in the list, in sample order.  Lane 0 is among the callers (the active lanes of a wave are
// its first ones).
__device__ __forceinline__ uint32_t wave_slot(bool h0, bool h1, uint32_t *cnt_at) {
  const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1);
  const unsigned long long below = (1ull << lane_id()) - 1ull;
  uint32_t at = 0u;
  if (lane_id() == 0) at = atomicAdd(cnt_at, (uint32_t)(__popcll(m0) + __popcll(m1)));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)at) + (uint32_t)(__popcll(m0 & below) + __popcll(m1 & below));
}

// ---- the point-list pass --------------------------------------------------------------------------------------------
// the 16 low bits of x moved to the even bit positions
__device__ __forceinline__ uint32_t spread16(uint32_t x) {
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  return (x | (x << 1)) & 0x55555555u;
}

// One pass of one workgroup: the samples [base, base + kFrontList) of the scan, two per thread, through E1 / E5 / E2 /
// E6 / the mount pose and the finite test into the LDS list pts[0 .. *cnt_at), a wave's points together and in sample
// order.  *cnt_at is 0 on entry (reset before the barrier in front of this call); the caller puts a barrier behind it.
//   idx      (optional, LDS)   the sample index of every list entry
//   fin_row  (optional, global) the scan's mask row: the finite bits of the wave's 128 samples are stored as whole
//            words (a word belongs to one wave of one workgroup; words without a sample below n are left alone)
//   rule_row (optional, global) the scan's mask row after E23's decision: only the finite samples whose bit is 0 are
//            listed (the skipped ones)
//   *finite  the thread's finite samples are added
template <bool FAST>
__device__ __forceinline__ void front_point_pass(const ScanFront &f, uint32_t base, const KParams &p, uint32_t *cnt_at,
                                                 float2 *pts, uint32_t *idx, uint32_t *__restrict__ fin_row,
                                                 const uint32_t *__restrict__ rule_row, uint32_t *finite) {
  const uint32_t n = f.n;
  const uint32_t pr = base / 2u + threadIdx.x;
  if (2u * pr < n) {  // (the active lanes of a wave are its first ones)
    const ScanPair s = scan_pair(f, p, pr);
    const uint32_t i0 = s.i0, i1 = s.i1;
    bool k0 = s.k0, k1 = s.k1;
    f2 a = {0.0f, 0.0f}, b = {0.0f, 0.0f};
    if (k0) {
      a = sample_xy<FAST>(s.t.x, s.t.y, i0, f.cs, f.sd.xf);
      k0 = fabsf(a.x) < __builtin_huge_valf() && fabsf(a.y) < __builtin_huge_valf();
    }
    if (k1) {
      b = sample_xy<FAST>(s.t.z, s.t.w, i1, f.cs, f.sd.xf);
      k1 = fabsf(b.x) < __builtin_huge_valf() && fabsf(b.y) < __builtin_huge_valf();
    }
    *finite += (k0 ? 1u : 0u) + (k1 ? 1u : 0u);
    if (fin_row) {  // (workgroup-uniform) lane w of the wave's first four stores word w of its 128 samples
      const unsigned long long f0 = __ballot(k0), f1 = __ballot(k1);
      const uint32_t w = lane_id() & 3u;
      const uint32_t word = spread16((uint32_t)(f0 >> (16u * w)) & 0xFFFFu) |
                            (spread16((uint32_t)(f1 >> (16u * w)) & 0xFFFFu) << 1);
      const uint32_t at_word = (i0 - 2u * lane_id()) / 32u + w;  // (i0 - 2 lane: the wave's first sample, a multiple of 128)
      if (lane_id() < 4u && at_word * 32u < n) fin_row[at_word] = word;  // < ceil(n / 32) <= the row's words
    }
    if (rule_row) {  // (workgroup-uniform) i1 <= n - 1 or dropped: the word lies inside the row
      const uint32_t w = rule_row[i0 >> 5];
      k0 = k0 && !((w >> (i0 & 31u)) & 1u);
      k1 = k1 && !((w >> (i1 & 31u)) & 1u);
    }
    const uint32_t at = wave_slot(k0, k1, cnt_at);
    if (k0) {  // at + 1 <= the wave's share: < kFrontList
      pts[at] = make_float2(a.x, a.y);
      if (idx) idx[at] = i0;
    }
    if (k1) {
      pts[at + (k0 ? 1u : 0u)] = make_float2(b.x, b.y);
      if (idx) idx[at + (k0 ? 1u : 0u)] = i1;
    }
  }
}

// ---- the cell-list pass ---------------------------------------------------------------------------------------------
constexpr uint32_t kCellBits = 13;  // a listed cell per axis, biased
constexpr uint32_t kCellMask = (1u << kCellBits) - 1u;

// the rotation (c, s) about the pivot (px, py) that a workgroup of E13 or E24 lays its scan over the field at
struct CellRot {
  float c, s, px, py;
};
__device__ __forceinline__ CellRot cell_rot(const MatchRot &rot, uint32_t kk, const float *__restrict__ pivot,
                                            uint32_t g) {
  return CellRot{rot.cs[2u * kk], rot.cs[2u * kk + 1u], pivot ? pivot[2u * g] : 0.0f,
                 pivot ? pivot[2u * g + 1u] : 0.0f};
}

// One sample to its list word (the cell of its rotated position, biased by BIAS per axis, weight field 0), or 0: not
// kept, not finite, without a cell, or out of every candidate's reach: farther than the window from the grid, or more
// than BELOW cells farther on the low side.  BIAS > the reach on the low side, so a listed word is never 0.  (r by
// value, four floats: by reference k_match_score and k_wide_bound come out with two or three more spilled SGPRs.)
template <bool FAST, int BIAS, int BELOW>
__device__ __forceinline__ uint32_t cell_word(uint32_t lo, uint32_t hi, uint32_t i, bool kept, const ScanFront &f,
                                              const MatchK &k, const CellRot r, uint32_t *finite, bool *cell_range) {
  if (!kept) return 0u;
  const f2 xy = sample_xy<FAST>(lo, hi, i, f.cs, f.sd.xf);
  if (!(fabsf(xy.x) < __builtin_huge_valf() && fabsf(xy.y) < __builtin_huge_valf())) return 0u;
  *finite += 1u;
  const float qx = xy.x - r.px, qy = xy.y - r.py;
  const float rx = (r.c * qx - r.s * qy) + r.px;
  const float ry = (r.s * qx + r.c * qy) + r.py;
  int cx, cy;
  if (!grid_cell(rx, ry, k.origin_x, k.origin_y, k.resolution, &cx, &cy)) {
    *cell_range = true;
    return 0u;
  }
  if (cx < -(int)k.tx - BELOW || cx >= (int)(k.width + k.tx) || cy < -(int)k.ty - BELOW ||
      cy >= (int)(k.height + k.ty))
    return 0u;
  return ((uint32_t)(cy + BIAS) << kCellBits) | (uint32_t)(cx + BIAS);
}

// One pass of one workgroup, called by all of its threads: the samples [base, base + kFrontList) of the scan, two per
// thread, into the LDS list s_list[0 .. *cnt_at), complete on return.  Consecutive samples of a wave half that land in
// one cell (a wall's neighbours) become ONE entry: the cell word, above its 2 * kCellBits bits the run's length - 1.
template <bool FAST, int BIAS, int BELOW>
__device__ __forceinline__ void front_cell_pass(const ScanFront &f, uint32_t base, const KParams &p, const MatchK &k,
                                                const CellRot &r, uint32_t *s_list, uint32_t *cnt_at, uint32_t *finite,
                                                bool *cell_range) {
  if (threadIdx.x == 0) *cnt_at = 0u;
  __syncthreads();  // (also: the last pass's readers are done with the list)
  const uint32_t pr = base / 2u + threadIdx.x;
  if (2u * pr < f.n) {  // (the active lanes of a wave are its first ones: a lane's predecessor is active)
    const ScanPair s = scan_pair(f, p, pr);
    const uint32_t w0 = cell_word<FAST, BIAS, BELOW>(s.t.x, s.t.y, s.i0, s.k0, f, k, r, finite, cell_range);
    const uint32_t w1 = cell_word<FAST, BIAS, BELOW>(s.t.z, s.t.w, s.i1, s.k1, f, k, r, finite, cell_range);
    // A sample continues a run when it has the cell of the sample before it; sample 0 of lanes 0 and 32 never
    // does, so a run holds at most 64 samples and its weight - 1 fits the six bits above the cell.
    const uint32_t before = __shfl_up(w1, 1, 64);  // the word of sample i0 - 1
    const bool e0 = w0 && (lane_id() & 31u) != 0u && w0 == before, e1 = w1 && w1 == w0;
    const bool h0 = w0 && !e0, h1 = w1 && !e1;
    const unsigned long long c_first = __ballot(e0), c_both = c_first & __ballot(e1);
    const uint32_t behind = run_behind(lane_id(), c_both, c_first);
    const uint32_t wt0 = e1 ? 2u + behind : 1u, wt1 = 1u + behind;
    const uint32_t at = wave_slot(h0, h1, cnt_at);
    if (h0) s_list[at] = w0 | ((wt0 - 1u) << (2u * kCellBits));
    if (h1) s_list[at + (h0 ? 1u : 0u)] = w1 | ((wt1 - 1u) << (2u * kCellBits));
  }
  __syncthreads();
}

// ---- the thread-to-pose layout --------------------------------------------------------------------------------------
// The pose of a thread: a list of up to kPoseTile poses is rounded up to whole waves and repeated over the workgroup
// as often as it fits; copy `slice` of `slices` walks every slices-th pair of the point list.
struct PoseLane {
  uint32_t per, slices, slice, q;
  bool own;
  float c, s, tx, ty;
};
__device__ __forceinline__ PoseLane pose_lane(uint32_t tile, uint32_t P, const float *__restrict__ list) {
  PoseLane l;
  l.per = min((P + 63u) & ~63u, kPoseTile);  // threads of one copy of the list
  l.slices = P <= kPoseTile ? kPoseTile / l.per : 1u;
  l.slice = threadIdx.x / l.per;  // (wave-uniform: per is whole waves)
  l.q = tile * kPoseTile + (threadIdx.x - l.slice * l.per);
  l.own = l.slice < l.slices && l.q < P;
  l.c = l.s = l.tx = l.ty = 0.0f;
  if (l.own) {  // a thread without a pose loads nothing and adds nothing
    const f32x4 v = *reinterpret_cast<const f32x4 *>(list + 4u * (size_t)l.q);
    l.c = v.x; l.s = v.y; l.tx = v.z; l.ty = v.w;
  }
  return l;
}

}  // namespace rpl
