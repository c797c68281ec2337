// rpl_refine.hip — E25: poses refined below a cell by Gauss-Newton on the bilinearly interpolated field,
// include/rplgpu_msg.h, rplgpu_refine_poses_dev (Hector's matcher; Cartographer's last stage).
//
//   k_refine_prepare  zeroes the scratch planes and the eight result words of every group;
//   k_refine_sums     E23's grid and walk (one workgroup per scan x tile of 1024 poses x slice of passes; the front
//                     end is scan_front, front_point_pass and pose_lane of rpl_front.hpp; a thread owns one pose and
//                     walks the LDS point list by broadcast): per point four field bytes, V, Gx, Gy, Gt, E and the eleven sums in
//                     registers; at the end the copies of a short list are added in LDS, limb by limb, and every
//                     32-bit limb leaves with one 64-bit no-return atomic add onto its own plane of the scratch, so
//                     no carry crosses an atomic and the planes depend on no order;
//   k_refine_finish   a thread per pose: the carries run through the planes once, 32 words stored;
//   k_refine_best     a workgroup per group: result words 4 - 6;
//   k_refine_step     a thread per pose: the fp64 step of the header through __dmul_rn / __dadd_rn / __ddiv_rn (nothing
//                     can fuse), the float32 move, result words 0 - 3;
//   k_match_poses, k_compose_poses  the joints to E13 / E24 and to E11 / E14, a thread per group / per scan.
// A workgroup walks at most two passes of 2048 samples (launch_refine_sums' grid), so a thread adds at most 4096
// points: the sums whose terms stay below 2^48 are plain 64-bit in registers; S Gt^2 and S Gt E carry a third limb.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rpl_front.hpp"
#include "rpl_refine.hpp"

namespace rpl {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr uint32_t kPlanes = RPLGPU_REFINE_PLANES;
constexpr uint32_t kMaxZ = 8u;  // slices of a scan's passes
static_assert((kMaxN + kFrontList - 1u) / kFrontList <= 2u * kMaxZ,
              "a workgroup walks at most two passes: 4096 points");
static_assert(RPLGPU_REFINE_WORDS == 32u && kPlanes == 29u, "the layout of the header's table");

// a thread's sums (the header's table; the limbs are made at the end)
struct RefineAcc {
  u64 sxx, syy, sv, see;
  i64 sxy, sxe, sye, sxt, syt;
  u64 stt_lo, ste_lo;
  uint32_t stt_hi;
  int32_t ste_hi;
  uint32_t n, dropped;
};

// one point at one pose, the header's PER POINT rule
__device__ __forceinline__ void refine_point(float x, float y, const PoseLane &l, const RefineK &k,
                                             const int8_t *__restrict__ field, RefineAcc &a) {
  const float ax = l.c * x - l.s * y;
  const float ay = l.s * x + l.c * y;
  const float rx = ax + l.tx, ry = ay + l.ty;
  const float hu = ((rx - k.origin_x) / k.resolution) * 256.0f - 128.0f;
  const float hv = ((ry - k.origin_y) / k.resolution) * 256.0f - 128.0f;
  const float lx = ax / k.resolution, ly = ay / k.resolution;
  if (!(fabsf(hu) < 268435456.0f && fabsf(hv) < 268435456.0f && fabsf(lx) < 8192.0f && fabsf(ly) < 8192.0f)) {
    ++a.dropped;
    return;
  }
  const int U = (int)floorf(hu), V_ = (int)floorf(hv);
  const int i0 = U >> 8, j0 = V_ >> 8, fa = U & 255, fb = V_ & 255;  // |i0|, |j0| <= 2^20: i0 + 1 does not wrap
  const int Lx = (int)rintf(lx * 16.0f), Ly = (int)rintf(ly * 16.0f);
  // m(ix, iy): 0 outside the grid and for a negative byte
  const uint32_t W = k.width, H = k.height;
  const int m00 = (int)field_look(field, i0, j0, W, H), m10 = (int)field_look(field, i0 + 1, j0, W, H);
  const int m01 = (int)field_look(field, i0, j0 + 1, W, H), m11 = (int)field_look(field, i0 + 1, j0 + 1, W, H);
  const int na = 256 - fa, nb = 256 - fb;
  const int V = na * nb * m00 + fa * nb * m10 + na * fb * m01 + fa * fb * m11;  // <= 127 * 65536
  const int Gx = nb * (m10 - m00) + fb * (m11 - m01);
  const int Gy = na * (m01 - m00) + fa * (m11 - m10);
  const i64 Gt = (i64)Gy * Lx - (i64)Gx * Ly;
  const int E = (int)(k.target * 65536u) - V;
  a.sxx += (u64)(uint32_t)(Gx * Gx);
  a.sxy += (i64)(Gx * Gy);
  a.syy += (u64)(uint32_t)(Gy * Gy);
  a.sxe += (i64)Gx * E;
  a.sye += (i64)Gy * E;
  a.sv += (u64)(uint32_t)V;
  a.sxt += (i64)Gx * Gt;
  a.syt += (i64)Gy * Gt;
  a.see += (u64)((i64)E * E);
  const u64 g = (u64)(Gt < 0 ? -Gt : Gt);  // < 2^33: the square has up to 66 bits
  const u64 sq = g * g;
  a.stt_lo += sq;
  a.stt_hi += (uint32_t)__umul64hi(g, g) + (a.stt_lo < sq ? 1u : 0u);
  const i64 te = Gt * (i64)E;  // < 2^56
  a.ste_lo += (u64)te;
  a.ste_hi += (int32_t)(te >> 63) + (a.ste_lo < (u64)te ? 1 : 0);
  ++a.n;
}

constexpr uint32_t kPrepThreads = 256;
constexpr uint32_t kPrepBlocks = 2048;

__global__ __launch_bounds__(kPrepThreads) void k_refine_prepare(u64 planes, u64 *__restrict__ scratch, uint32_t G,
                                                                 uint32_t *__restrict__ result) {
  const u64 t0 = (u64)blockIdx.x * kPrepThreads + threadIdx.x;
  const u64 step = (u64)gridDim.x * kPrepThreads;
  for (u64 v = t0; v < planes; v += step) scratch[v] = 0ull;
  for (u64 v = t0; v < 8ull * G; v += step) result[v] = 0u;
}

template <bool FAST>
__global__ __launch_bounds__(kBlock) void k_refine_sums(
    const uint2 *__restrict__ nodes, uint32_t n_stride, const uint32_t *__restrict__ n_per_scan, uint32_t group,
    KParams p, Tables T, const uint32_t *__restrict__ keepmask, uint32_t mask_stride,
    const float *__restrict__ motion, const float *__restrict__ pose2d, RefineK k, const float *__restrict__ poses,
    uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group, const int8_t *__restrict__ field,
    unsigned long long field_stride, uint32_t field_per_group, u64 *__restrict__ scratch,
    uint32_t *__restrict__ result, uint32_t *__restrict__ status) {
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
  const int8_t *fld = field + (size_t)(field_per_group ? g : 0u) * field_stride;
  const PoseLane l = pose_lane(tile, P, poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
  RefineAcc a = {};
  uint32_t finite = 0u;
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
      for (uint32_t e = l.slice; 2u * e < cnt; e += l.slices) {
        const f32x4 v = s_pts[e];
        refine_point(v.x, v.y, l, k, fld, a);
        if (2u * e + 1u < cnt) refine_point(v.z, v.w, l, k, fld, a);
      }
    }
  }
  if (status && __any(a.dropped != 0u) && lane_id() == 0) atomicOr(&status[g], RPLGPU_SCAN_CELL_RANGE);
  if (tile == 0u) {  // word 7, the group's finite points: once per sample, by the workgroups of the first tile
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) finite += __shfl_xor(finite, d, 64);
    if (lane_id() == 0 && finite) atomicAdd(&result[8u * g + 7u], finite);
  }
  // the limbs, in the order of the header's words; a 64-bit sum of signed terms is its two's complement, and the
  // third limb of the three that stayed in 64 bits is their sign
  const uint32_t limb[kPlanes] = {
      (uint32_t)a.sxx, (uint32_t)(a.sxx >> 32), (uint32_t)a.sxy, (uint32_t)((u64)a.sxy >> 32),
      (uint32_t)a.syy, (uint32_t)(a.syy >> 32), (uint32_t)a.sxe, (uint32_t)((u64)a.sxe >> 32),
      (uint32_t)a.sye, (uint32_t)((u64)a.sye >> 32), (uint32_t)a.sv, (uint32_t)(a.sv >> 32),
      (uint32_t)a.sxt, (uint32_t)((u64)a.sxt >> 32), (uint32_t)(a.sxt >> 63),
      (uint32_t)a.syt, (uint32_t)((u64)a.syt >> 32), (uint32_t)(a.syt >> 63),
      (uint32_t)a.stt_lo, (uint32_t)(a.stt_lo >> 32), a.stt_hi,
      (uint32_t)a.ste_lo, (uint32_t)(a.ste_lo >> 32), (uint32_t)a.ste_hi,
      (uint32_t)a.see, (uint32_t)(a.see >> 32), 0u,
      a.n, a.dropped};
  // plane j of the group: P 64-bit words; the copies of a short list are added here first, one limb at a time
  u64 *plane = scratch + (size_t)g * kPlanes * P;
  const bool writer = threadIdx.x < l.per && tile * kPoseTile + threadIdx.x < P;
#pragma unroll
  for (uint32_t j = 0; j < kPlanes; ++j) {
    __syncthreads();
    s_sum[threadIdx.x] = limb[j];  // copy `slice` at [slice * per, slice * per + per); 0 where a thread owns no pose
    __syncthreads();
    if (writer) {
      u64 sum = 0ull;
      for (uint32_t s = 0; s < l.slices; ++s) sum += s_sum[s * l.per + threadIdx.x];  // slices * per <= kBlock
      if (sum) atomicAdd(&plane[(size_t)j * P + tile * kPoseTile + threadIdx.x], sum);  // q < P: inside the plane
    }
  }
}

constexpr uint32_t kPoseThreads = 256;

// grid (ceil(P / 256), G): the planes of pose q into its 32 words
__global__ __launch_bounds__(kPoseThreads) void k_refine_finish(uint32_t P, const u64 *__restrict__ scratch,
                                                                uint32_t *__restrict__ sums,
                                                                unsigned long long sums_stride) {
  const uint32_t q = blockIdx.x * kPoseThreads + threadIdx.x;
  const uint32_t g = blockIdx.y;
  if (q >= P) return;
  const u64 *plane = scratch + (size_t)g * kPlanes * P + q;
  uint32_t w[32];
  // the widths of the header's table: six values of two limbs, five of three, two of one; the carry out of a
  // value's last limb is dropped (the sum modulo 2^64 or 2^96 is its two's complement)
  uint32_t j = 0;
#pragma unroll
  for (uint32_t v = 0; v < 13u; ++v) {
    const uint32_t width = v < 6u ? 2u : v < 11u ? 3u : 1u;
    u64 carry = 0ull;
#pragma unroll
    for (uint32_t i = 0; i < width; ++i, ++j) {
      const u64 t = plane[(size_t)j * P] + carry;  // a plane holds < 2^32 limbs below 2^32, the carry is below 2^32
      w[j] = (uint32_t)t;
      carry = t >> 32;
    }
  }
  w[29] = w[30] = w[31] = 0u;
  u32x4 *out = reinterpret_cast<u32x4 *>(sums + (size_t)g * sums_stride + 32u * (size_t)q);
#pragma unroll
  for (uint32_t i = 0; i < 8u; ++i) out[i] = u32x4{w[4u * i], w[4u * i + 1u], w[4u * i + 2u], w[4u * i + 3u]};
}

// grid G: the smallest q with the greatest S V (words 10 - 11 of a pose's sums)
__global__ __launch_bounds__(kPoseThreads) void k_refine_best(uint32_t P, const uint32_t *__restrict__ sums,
                                                              unsigned long long sums_stride,
                                                              uint32_t *__restrict__ result) {
  __shared__ u64 s_v[kPoseThreads];
  __shared__ uint32_t s_q[kPoseThreads];
  const uint32_t g = blockIdx.x;
  const uint32_t *row = sums + (size_t)g * sums_stride;
  u64 best = 0ull;
  uint32_t at = 0xFFFFFFFFu;
  for (uint32_t q = threadIdx.x; q < P; q += kPoseThreads) {  // ascending q: the first of equals stays
    const u64 v = ((u64)row[32u * (size_t)q + 11u] << 32) | row[32u * (size_t)q + 10u];
    if (at == 0xFFFFFFFFu || v > best) {
      best = v;
      at = q;
    }
  }
  s_v[threadIdx.x] = best;
  s_q[threadIdx.x] = at;
  __syncthreads();
  for (uint32_t d = kPoseThreads / 2u; d > 0u; d >>= 1) {
    if (threadIdx.x < d) {
      const u64 ov = s_v[threadIdx.x + d];
      const uint32_t oq = s_q[threadIdx.x + d];
      if (ov > s_v[threadIdx.x] || (ov == s_v[threadIdx.x] && oq < s_q[threadIdx.x])) {
        s_v[threadIdx.x] = ov;
        s_q[threadIdx.x] = oq;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {  // (P >= 1: thread 0 has seen pose 0)
    result[8u * (size_t)g + 4u] = s_q[0];
    result[8u * (size_t)g + 5u] = (uint32_t)s_v[0];
    result[8u * (size_t)g + 6u] = (uint32_t)(s_v[0] >> 32);
  }
}

__global__ __launch_bounds__(kPoseThreads) void k_refine_zero4(uint32_t G, uint32_t *__restrict__ result) {
  const uint32_t v = blockIdx.x * kPoseThreads + threadIdx.x;
  if (v < 4u * G) result[8u * (size_t)(v >> 2) + (v & 3u)] = 0u;
}

__device__ __forceinline__ double rf_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double rf_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double rf_sub(double a, double b) { return __dadd_rn(a, -b); }
__device__ __forceinline__ bool rf_finite(double v) { return fabs(v) < __builtin_huge_val(); }
__device__ __forceinline__ double rf_d64s(uint32_t w0, uint32_t w1) { return __ll2double_rn((i64)(((u64)w1 << 32) | w0)); }
__device__ __forceinline__ double rf_d64u(uint32_t w0, uint32_t w1) { return __ull2double_rn(((u64)w1 << 32) | w0); }
__device__ __forceinline__ double rf_d96(uint32_t w0, uint32_t w1, uint32_t w2, bool is_signed) {
  const double top = is_signed ? (double)(int32_t)w2 : (double)w2;
  return rf_add(rf_mul(rf_add(rf_mul(top, 4294967296.0), (double)w1), 4294967296.0), (double)w0);
}
__device__ __forceinline__ uint32_t rf_canon(float v) { return v != v ? 0x7FC00000u : __float_as_uint(v); }

// grid (ceil(P / 256), G): the header's STEP, operation for operation (rplgpu_refine_step_host is the same sequence)
__global__ __launch_bounds__(kPoseThreads) void k_refine_step(
    const uint32_t *__restrict__ sums, unsigned long long sums_stride, RefineK k, const float *poses,
    unsigned long long pose_stride, uint32_t poses_per_group, uint32_t P, float *poses_out,
    unsigned long long out_stride, uint32_t *__restrict__ step, unsigned long long step_stride,
    uint32_t *__restrict__ result) {
  const uint32_t q = blockIdx.x * kPoseThreads + threadIdx.x;
  const uint32_t g = blockIdx.y;
  uint32_t flags = 0u;
  if (q < P) {
    const u32x4 *in = reinterpret_cast<const u32x4 *>(sums + (size_t)g * sums_stride + 32u * (size_t)q);
    uint32_t w[28];
#pragma unroll
    for (uint32_t i = 0; i < 7u; ++i) {
      const u32x4 v = in[i];
      w[4u * i] = v.x; w[4u * i + 1u] = v.y; w[4u * i + 2u] = v.z; w[4u * i + 3u] = v.w;
    }
    const u32x4 pose =
        *reinterpret_cast<const u32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride + 4u * (size_t)q);
    double dx = 0.0, dy = 0.0, dt = 0.0;
    if (w[27] < k.min_points) {
      flags = RPLGPU_REFINE_FEW;
    } else {
      const double k16 = 1.0 / 65536.0, k20 = 1.0 / 1048576.0, k24 = 1.0 / 16777216.0, k28 = 1.0 / 268435456.0;
      double a11 = rf_mul(rf_d64u(w[0], w[1]), k16);
      const double a12 = rf_mul(rf_d64s(w[2], w[3]), k16);
      double a22 = rf_mul(rf_d64u(w[4], w[5]), k16);
      const double a13 = rf_mul(rf_d96(w[12], w[13], w[14], true), k20);
      const double a23 = rf_mul(rf_d96(w[15], w[16], w[17], true), k20);
      double a33 = rf_mul(rf_d96(w[18], w[19], w[20], false), k24);
      const double g1 = rf_mul(rf_d64s(w[6], w[7]), k24);
      const double g2 = rf_mul(rf_d64s(w[8], w[9]), k24);
      const double g3 = rf_mul(rf_d96(w[21], w[22], w[23], true), k28);
      const double damping = (double)k.damping;
      a11 = rf_add(a11, rf_mul(damping, a11));
      a22 = rf_add(a22, rf_mul(damping, a22));
      a33 = rf_add(a33, rf_mul(damping, a33));
      const double c11 = rf_sub(rf_mul(a22, a33), rf_mul(a23, a23));
      const double c12 = rf_sub(rf_mul(a13, a23), rf_mul(a12, a33));
      const double c13 = rf_sub(rf_mul(a12, a23), rf_mul(a13, a22));
      const double c22 = rf_sub(rf_mul(a11, a33), rf_mul(a13, a13));
      const double c23 = rf_sub(rf_mul(a12, a13), rf_mul(a11, a23));
      const double c33 = rf_sub(rf_mul(a11, a22), rf_mul(a12, a12));
      const double det = rf_add(rf_add(rf_mul(a11, c11), rf_mul(a12, c12)), rf_mul(a13, c13));
      if (!(det > 0.0) || !rf_finite(det)) {
        flags = RPLGPU_REFINE_SINGULAR;
      } else {
        dx = __ddiv_rn(rf_add(rf_add(rf_mul(c11, g1), rf_mul(c12, g2)), rf_mul(c13, g3)), det);
        dy = __ddiv_rn(rf_add(rf_add(rf_mul(c12, g1), rf_mul(c22, g2)), rf_mul(c23, g3)), det);
        dt = __ddiv_rn(rf_add(rf_add(rf_mul(c13, g1), rf_mul(c23, g2)), rf_mul(c33, g3)), det);
        flags = rf_finite(dx) && rf_finite(dy) && rf_finite(dt) ? RPLGPU_REFINE_STEPPED : RPLGPU_REFINE_SINGULAR;
      }
    }
    u32x4 out = pose;
    float mx = 0.0f, my = 0.0f, mt = 0.0f;
    if (flags & RPLGPU_REFINE_STEPPED) {
      const double ms = (double)k.max_step_cells, mr = (double)k.max_rot;
      if (dx > ms) { dx = ms; flags |= RPLGPU_REFINE_CLAMP_X; }
      if (dx < -ms) { dx = -ms; flags |= RPLGPU_REFINE_CLAMP_X; }
      if (dy > ms) { dy = ms; flags |= RPLGPU_REFINE_CLAMP_Y; }
      if (dy < -ms) { dy = -ms; flags |= RPLGPU_REFINE_CLAMP_Y; }
      if (dt > mr) { dt = mr; flags |= RPLGPU_REFINE_CLAMP_T; }
      if (dt < -mr) { dt = -mr; flags |= RPLGPU_REFINE_CLAMP_T; }
      const double h = rf_mul(0.5, dt);
      const double hh = rf_mul(h, h);
      const double den = rf_add(1.0, hh);
      const double dc = __ddiv_rn(rf_sub(1.0, hh), den);
      const double ds = __ddiv_rn(rf_add(h, h), den);
      const float fc = __double2float_rn(dc), fs = __double2float_rn(ds);
      mx = __double2float_rn(rf_mul(dx, (double)k.resolution));
      my = __double2float_rn(rf_mul(dy, (double)k.resolution));
      mt = __double2float_rn(dt);
      const float c = __uint_as_float(pose.x), s = __uint_as_float(pose.y);
      out.x = rf_canon(__fsub_rn(__fmul_rn(c, fc), __fmul_rn(s, fs)));
      out.y = rf_canon(__fadd_rn(__fmul_rn(s, fc), __fmul_rn(c, fs)));
      out.z = rf_canon(__fadd_rn(__uint_as_float(pose.z), mx));
      out.w = rf_canon(__fadd_rn(__uint_as_float(pose.w), my));
    }
    // q < P: inside the group's 4 P floats of out_stride, 4 P words of step_stride
    *reinterpret_cast<u32x4 *>(poses_out + (size_t)g * out_stride + 4u * (size_t)q) = out;
    if (step)
      *reinterpret_cast<u32x4 *>(step + (size_t)g * step_stride + 4u * (size_t)q) =
          u32x4{__float_as_uint(mx), __float_as_uint(my), __float_as_uint(mt), flags};
  }
  // result words 0 - 3: one popcount per wave (a thread without a pose has no flag)
  const u64 b0 = __ballot(flags & RPLGPU_REFINE_STEPPED), b1 = __ballot(flags & RPLGPU_REFINE_FEW);
  const u64 b2 = __ballot(flags & RPLGPU_REFINE_SINGULAR);
  const u64 b3 = __ballot(flags & (RPLGPU_REFINE_CLAMP_X | RPLGPU_REFINE_CLAMP_Y | RPLGPU_REFINE_CLAMP_T));
  if (lane_id() == 0) {
    uint32_t *out = result + 8u * (size_t)g;
    if (b0) atomicAdd(&out[0], (uint32_t)__popcll(b0));
    if (b1) atomicAdd(&out[1], (uint32_t)__popcll(b1));
    if (b2) atomicAdd(&out[2], (uint32_t)__popcll(b2));
    if (b3) atomicAdd(&out[3], (uint32_t)__popcll(b3));
  }
}

// a thread per group: E13's correction of the base prior, the header's order of operations
__global__ __launch_bounds__(kPoseThreads) void k_match_poses(const uint32_t *__restrict__ best, MatchK k, MatchRot rot,
                                                              const float *__restrict__ pivot,
                                                              const float *__restrict__ prior, uint32_t G,
                                                              float *__restrict__ poses_out,
                                                              unsigned long long out_stride) {
  const uint32_t g = blockIdx.x * kPoseThreads + threadIdx.x;
  if (g >= G) return;
  const uint32_t *bw = best + 8u * (size_t)g;
  const int kr = (int)bw[1], j = (int)bw[2], i = (int)bw[3];
  const int K = (int)k.rot;
  const float px = pivot ? pivot[2u * (size_t)g] : 0.0f, py = pivot ? pivot[2u * (size_t)g + 1u] : 0.0f;
  u32x4 out = {__float_as_uint(1.0f), 0u, __float_as_uint(px), __float_as_uint(py)};
  if (prior) out = *reinterpret_cast<const u32x4 *>(prior + 4u * (size_t)g);
  if (kr >= -K && kr <= K) {  // (else a caller's error: the prior is kept, no table index leaves the table)
    const uint32_t kk = (uint32_t)(kr + K);
    const float c = rot.cs[2u * kk], s = rot.cs[2u * kk + 1u];
    const float c0 = __uint_as_float(out.x), s0 = __uint_as_float(out.y);
    const float qx = __uint_as_float(out.z) - px, qy = __uint_as_float(out.w) - py;
    out.x = __float_as_uint(c * c0 - s * s0);
    out.y = __float_as_uint(s * c0 + c * s0);
    out.z = __float_as_uint(((c * qx - s * qy) + px) + (float)i * k.resolution);
    out.w = __float_as_uint(((s * qx + c * qy) + py) + (float)j * k.resolution);
  }
  *reinterpret_cast<u32x4 *>(poses_out + (size_t)g * out_stride) = out;
}

// a thread per scan: pose q_g of the group's list composed in front of the scan's mount pose
__global__ __launch_bounds__(kPoseThreads) void k_compose_poses(const float *__restrict__ poses,
                                                                unsigned long long pose_stride,
                                                                uint32_t poses_per_group, uint32_t P,
                                                                const uint32_t *__restrict__ result, uint32_t q,
                                                                const float *pose_in, uint32_t B, uint32_t group,
                                                                float *pose_out) {
  const uint32_t sc = blockIdx.x * kPoseThreads + threadIdx.x;
  if (sc >= B) return;
  const uint32_t g = sc / group;
  const uint32_t qg = result ? result[8u * (size_t)g + 4u] : q;
  float r00 = 1.0f, r01 = 0.0f, tx = 0.0f, r10 = 0.0f, r11 = 1.0f, ty = 0.0f;
  if (pose_in) {
    const float *m = pose_in + 6u * (size_t)sc;
    r00 = m[0]; r01 = m[1]; tx = m[2]; r10 = m[3]; r11 = m[4]; ty = m[5];
  }
  if (qg < P) {  // (else the mount pose is copied: no index leaves the list)
    const f32x4 v =
        *reinterpret_cast<const f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride + 4u * (size_t)qg);
    const float c = v.x, s = v.y;
    const float n00 = c * r00 - s * r10, n01 = c * r01 - s * r11;
    const float n10 = s * r00 + c * r10, n11 = s * r01 + c * r11;
    const float ntx = (c * tx - s * ty) + v.z;
    const float nty = (s * tx + c * ty) + v.w;
    r00 = n00; r01 = n01; r10 = n10; r11 = n11; tx = ntx; ty = nty;
  }
  float *o = pose_out + 6u * (size_t)sc;
  o[0] = r00; o[1] = r01; o[2] = tx; o[3] = r10; o[4] = r11; o[5] = ty;
}

bool refine_args_ok(const RefineK &k, uint32_t P) {
  return k.width != 0 && k.height != 0 && k.width <= RPLGPU_MAX_OCC_DIM && k.height <= RPLGPU_MAX_OCC_DIM && P != 0 &&
         P <= RPLGPU_MAX_POSES && k.target >= 1u && k.target <= 127u;
}

}  // namespace

hipError_t launch_refine_prepare(hipStream_t s, uint32_t G, uint32_t P, uint32_t *scratch, uint32_t *result) {
  if (G == 0 || P == 0 || P > RPLGPU_MAX_POSES || !scratch || !result) return hipErrorInvalidValue;
  const u64 planes = (u64)kPlanes * G * P;
  const uint32_t blocks = (uint32_t)std::min<u64>((planes + kPrepThreads - 1u) / kPrepThreads, kPrepBlocks);
  hipLaunchKernelGGL(k_refine_prepare, dim3(blocks), dim3(kPrepThreads), 0, s, planes, (u64 *)scratch, G, result);
  return hipGetLastError();
}

hipError_t launch_refine_sums(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                              uint32_t B, uint32_t group, const KParams &p, const Tables &T, const uint32_t *keepmask,
                              uint32_t mask_stride, const float *motion, const float *pose2d, const RefineK &k,
                              const float *poses, uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group,
                              const int8_t *field, unsigned long long field_stride, uint32_t field_per_group,
                              uint32_t *scratch, uint32_t *result, uint32_t *status) {
  if (B == 0) return hipSuccess;
  if (group == 0 || !refine_args_ok(k, P) || field_stride < (unsigned long long)k.width * k.height ||
      pose_stride < 4ull * P || (pose_stride & 3u) || n_stride == 0 || n_stride > kMaxN || !scratch || !result)
    return hipErrorInvalidValue;
  // slices of a scan's passes, as launch_pose_score: at most two passes a workgroup
  const uint32_t passes = (n_stride + kFrontList - 1u) / kFrontList;
  const dim3 grid(B, (P + kPoseTile - 1u) / kPoseTile, std::min(passes, kMaxZ));
  if (p.fast_d4000)
    hipLaunchKernelGGL(k_refine_sums<true>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride, poses_per_group,
                       field, field_stride, field_per_group, (u64 *)scratch, result, status);
  else
    hipLaunchKernelGGL(k_refine_sums<false>, grid, dim3(kBlock), 0, s, (const uint2 *)nodes, n_stride, n_per_scan,
                       group, p, T, keepmask, mask_stride, motion, pose2d, k, poses, P, pose_stride, poses_per_group,
                       field, field_stride, field_per_group, (u64 *)scratch, result, status);
  return hipGetLastError();
}

hipError_t launch_refine_finish(hipStream_t s, uint32_t G, uint32_t P, const uint32_t *scratch, uint32_t *sums,
                                unsigned long long sums_stride, uint32_t *result) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || sums_stride < 32ull * P || (sums_stride & 3u) ||
      !scratch || !sums || !result)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_refine_finish, dim3((P + kPoseThreads - 1u) / kPoseThreads, G), dim3(kPoseThreads), 0, s, P,
                     (const u64 *)scratch, sums, sums_stride);
  hipLaunchKernelGGL(k_refine_best, dim3(G), dim3(kPoseThreads), 0, s, P, sums, sums_stride, result);
  return hipGetLastError();
}

hipError_t launch_refine_step(hipStream_t s, const uint32_t *sums, unsigned long long sums_stride, const RefineK &k,
                              const float *poses, unsigned long long pose_stride, uint32_t poses_per_group, uint32_t G,
                              uint32_t P, float *poses_out, unsigned long long out_stride, uint32_t *step,
                              unsigned long long step_stride, uint32_t *result, bool zero_result) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || sums_stride < 32ull * P || (sums_stride & 3u) ||
      pose_stride < 4ull * P || (pose_stride & 3u) || out_stride < 4ull * P || (out_stride & 3u) ||
      (step && (step_stride < 4ull * P || (step_stride & 3u))) || !sums || !poses || !poses_out || !result)
    return hipErrorInvalidValue;
  if (zero_result)
    hipLaunchKernelGGL(k_refine_zero4, dim3((4u * G + kPoseThreads - 1u) / kPoseThreads), dim3(kPoseThreads), 0, s, G,
                       result);
  hipLaunchKernelGGL(k_refine_step, dim3((P + kPoseThreads - 1u) / kPoseThreads, G), dim3(kPoseThreads), 0, s, sums,
                     sums_stride, k, poses, pose_stride, poses_per_group, P, poses_out, out_stride, step, step_stride,
                     result);
  return hipGetLastError();
}

hipError_t launch_match_poses(hipStream_t s, const uint32_t *best, const MatchK &k, const MatchRot &rot,
                              const float *pivot, const float *prior, uint32_t G, float *poses_out,
                              unsigned long long out_stride) {
  if (G == 0 || !best || !poses_out || out_stride < 4u || (out_stride & 3u) || k.rot > RPLGPU_MAX_MATCH_ROT)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_match_poses, dim3((G + kPoseThreads - 1u) / kPoseThreads), dim3(kPoseThreads), 0, s, best, k,
                     rot, pivot, prior, G, poses_out, out_stride);
  return hipGetLastError();
}

hipError_t launch_compose_poses(hipStream_t s, const float *poses, unsigned long long pose_stride,
                                uint32_t poses_per_group, uint32_t P, const uint32_t *result, uint32_t q,
                                const float *pose_in, uint32_t B, uint32_t group, float *pose_out) {
  if (B == 0) return hipSuccess;
  if (group == 0 || !poses || !pose_out || P == 0 || P > RPLGPU_MAX_POSES || pose_stride < 4ull * P ||
      (pose_stride & 3u))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_compose_poses, dim3((B + kPoseThreads - 1u) / kPoseThreads), dim3(kPoseThreads), 0, s, poses,
                     pose_stride, poses_per_group, P, result, q, pose_in, B, group, pose_out);
  return hipGetLastError();
}

}  // namespace rpl
