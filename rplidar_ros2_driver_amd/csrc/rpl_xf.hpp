// rpl_xf.hpp — the per-sample front end that E8 (rpl_voxel.hip), E9 (rpl_merge.hip) and E11 (rpl_occ.hip) share: where a
// point of one scan of a group goes between polar->XY and the common frame (E6 de-skew, planar pose),
// and what of the scan the streaming code needs besides its nodes (the E5 keep bits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rpl {

typedef float f2 __attribute__((ext_vector_type(2)));

// E8 (include/rplgpu_msg.h): what happens to a point between polar->XY and the grid when a GROUP
// of scans shares one grid — the scan's motion during its acquisition (E6 de-skew, same
// operations in the same order as k_cloud) and its sensor's planar pose.  All zeros / identity
// reproduce x, y bit for bit.
struct ScanXf {
  float vx, vy, wz, dt;             // planar twist of the sensor and time between samples
  float t0;                         // time of the first sample relative to the fused instant
  uint32_t has_t0;                  // (0: no offsets set — tau = i * dt, bit for bit as without them)
  float r00, r01, tx, r10, r11, ty;  // [R | t] of the sensor in the common frame (2-D)
};
__device__ __forceinline__ f2 apply_xf(f2 xy, uint32_t sample_index, const ScanXf &m) {
  float tau = (float)sample_index * m.dt;
  if (m.has_t0) tau = m.t0 + tau;  // (scan-uniform)
  const float a = m.wz * tau, a2 = a * a;
  float ts = a2 * (1.0f / 120.0f);
  ts = ts + (-1.0f / 6.0f);
  ts = a2 * ts;
  ts = ts + 1.0f;
  const float sn = a * ts;
  float tc = a2 * (-1.0f / 720.0f);
  tc = tc + (1.0f / 24.0f);
  tc = a2 * tc;
  tc = tc + (-0.5f);
  tc = a2 * tc;
  const float cn = tc + 1.0f;
  const float x1 = (cn * xy.x - sn * xy.y) + m.vx * tau;
  const float y1 = (sn * xy.x + cn * xy.y) + m.vy * tau;
  f2 o;
  o.x = (m.r00 * x1 + m.r01 * y1) + m.tx;
  o.y = (m.r10 * x1 + m.r11 * y1) + m.ty;
  return o;
}

// a / 4000 as mul + 2 FMA: the form rpl_voxel.hip's div_by proves bit-identical to the IEEE divide
// on the device (k_validate_div) before KParams::fast_d4000 is set
__device__ __forceinline__ float xf_div4000(float a) {
  const float q = a * 0.00025f;
  const float e = fmaf(-q, 4000.0f, a);
  return fmaf(e, 0.00025f, q);
}

// One packed node (lo, hi: its two dwords) to its point in the common frame, as E9 and E11 stream it:
// E2 with the (cos, sin) table `cs`, then E6 + the planar pose.  FAST: the validated divide by 4000.
template <bool FAST>
__device__ __forceinline__ f2 sample_xy(uint32_t lo, uint32_t hi, uint32_t i, const float2 *__restrict__ cs,
                                        const ScanXf &xf) {
  const uint32_t d = __builtin_amdgcn_alignbit(hi, lo, 16);
  const float df = __uint2float_rn(d);
  const float dm = FAST ? xf_div4000(df) : df / 4000.0f;  // :590
  const float2 c = cs[lo & 0xFFFFu];
  f2 xy = {c.x * dm, c.y * dm};                            // E2
  return apply_xf(xy, i, xf);                              // E6 + pose, as E8
}

// What of one scan the streaming code needs besides its nodes: the E5 keep bits and the E8 transform.
struct ScanSide {
  const uint32_t *ror_bits;
  ScanXf xf;
};
__device__ __forceinline__ ScanSide scan_side(uint32_t sc, const uint32_t *__restrict__ keepmask,
                                              uint32_t mask_stride, const float *__restrict__ motion,
                                              const float *__restrict__ pose2d,
                                              const float *__restrict__ scan_t0) {
  ScanSide s;
  s.ror_bits = keepmask ? keepmask + (size_t)sc * mask_stride : nullptr;
  s.xf = ScanXf{0.f, 0.f, 0.f, 0.f, 0.f, 0u, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  if (motion) {
    s.xf.vx = motion[4 * sc]; s.xf.vy = motion[4 * sc + 1]; s.xf.wz = motion[4 * sc + 2]; s.xf.dt = motion[4 * sc + 3];
    if (scan_t0) { s.xf.t0 = scan_t0[sc]; s.xf.has_t0 = 1u; }
  }
  if (pose2d) {
    s.xf.r00 = pose2d[6 * sc]; s.xf.r01 = pose2d[6 * sc + 1]; s.xf.tx = pose2d[6 * sc + 2];
    s.xf.r10 = pose2d[6 * sc + 3]; s.xf.r11 = pose2d[6 * sc + 4]; s.xf.ty = pose2d[6 * sc + 5];
  }
  return s;
}
}  // namespace rpl
