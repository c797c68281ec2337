// rpl_mppi.hip — E28: rolled-out candidates weighed and blended into new controls, include/rplgpu_msg.h,
// rplgpu_mppi_update_dev and rplgpu_mppi_spread_dev.  The update is a K-long fold for each of T_e steps over K T_e
// entries of 16 bytes that lie [k][t]; everything that is summed is an integer, so no order shows.
//
// Three launches, no workgroup waits for another, no loop is bounded by a word from memory:
//   k_mppi_weights  a thread per candidate: three words of E27's output, two of its result and one table gather make
//                   w; the one writer of d_weights.  A record per workgroup: how many w != 0, how many clamped, sum w,
//                   sum w^2.
//   k_mppi_sums     lanes step-fastest (tw = the power of two at or above T_e, 256 / tw rows of candidates), so a wave
//                   reads one contiguous run of entries; a lane folds RPLGPU_MPPI_PER_LANE candidates of its step into
//                   four int64 sums and a count in registers, the rows fold by wave shuffles (tw < 64) and LDS atomics,
//                   row 0 writes the workgroup's record of twelve words per step into the scratch.  At G = 1, K 2048,
//                   T 56 that is 64 workgroups of 32 candidates; at T_e = 256, 256 of 8.
//   k_mppi_close    a workgroup per group, laid out the same way over (step, record): folds the sums records, writes
//                   the eight words of a step and the step's new delta (E25's fp64 lines), folds the weight records
//                   into the result words.
// k_mppi_spread is one launch, a thread per (candidate, step).
#include <hip/hip_runtime.h>

#include "rpl_mppi.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef uint32_t mp_u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kMpWRecord = 8u, kMpSRecord = 12u;

struct MpAcc {  // a step's sums over a set of candidates, two's complement
  u64 w, h, x, y;
  uint32_t off;  // entries not in range
};

// tw <= 32: the lanes of a wave that hold the same step (lane & (tw - 1)) fold into the lanes below tw
__device__ __forceinline__ void mp_wave_fold(MpAcc &a, uint32_t tw) {
  for (uint32_t d = 32u; d >= tw && d != 0u; d >>= 1) {  // at most 6 rounds, uniform over the wave
    a.w += __shfl_xor(a.w, (int)d, 64);
    a.h += __shfl_xor(a.h, (int)d, 64);
    a.x += __shfl_xor(a.x, (int)d, 64);
    a.y += __shfl_xor(a.y, (int)d, 64);
    a.off += __shfl_xor(a.off, (int)d, 64);
  }
}

// every lane's sums into s_acc[5 t ..]: shuffles first where a wave holds a step more than once.  The caller has
// zeroed s_acc and synchronised; it synchronises again before it reads.
__device__ __forceinline__ void mp_block_fold(MpAcc a, uint32_t tw, uint32_t t, u64 *s_acc) {
  bool lead = true;
  if (tw < 64u) {
    mp_wave_fold(a, tw);
    lead = (threadIdx.x & 63u) < tw;
  }
  if (lead && (a.w | a.off) != 0u) {  // (w = 0: h, x and y are 0 too)
    atomicAdd(&s_acc[5u * t], a.w);
    atomicAdd(&s_acc[5u * t + 1u], a.h);
    atomicAdd(&s_acc[5u * t + 2u], a.x);
    atomicAdd(&s_acc[5u * t + 3u], a.y);
    atomicAdd(&s_acc[5u * t + 4u], (u64)a.off);
  }
}

// grid (ceil(K / 256), G)
__global__ __launch_bounds__(kMpBlock) void k_mppi_weights(const MppiK k, const uint32_t *__restrict__ out,
                                                           u64 out_stride, const uint32_t *__restrict__ ro_result,
                                                           const uint16_t *__restrict__ table, uint32_t K,
                                                           uint32_t *__restrict__ weights, u64 weight_stride,
                                                           uint32_t *__restrict__ scratch) {
  __shared__ u64 s_sum[2];
  __shared__ uint32_t s_cnt[2];
  const uint32_t tid = threadIdx.x, g = blockIdx.y, kk = blockIdx.x * kMpBlock + tid;
  if (tid < 2u) {
    s_sum[tid] = 0ull;
    s_cnt[tid] = 0u;
  }
  __syncthreads();
  uint32_t w = 0u, clamped = 0u;
  if (kk < K) {
    const uint32_t *res = ro_result + 8u * (size_t)g;
    const mp_u32x4 *o = reinterpret_cast<const mp_u32x4 *>(out + (size_t)g * out_stride) + 2u * (size_t)kk;
    const mp_u32x4 lo = o[0], hi = o[1];
    if ((lo.y & RPLGPU_ROLLOUT_ADMISSIBLE) && !(res[7] & 1u)) {
      const u64 s = (u64)hi.z | ((u64)hi.w << 32), m = (u64)res[2] | ((u64)res[3] << 32);
      const u64 d = s < m ? 0ull : s - m;
      u64 i = d >> k.shift;
      if (i > (u64)(k.table_len - 1u)) {
        i = k.table_len - 1u;
        clamped = 1u;
      }
      w = table[i];  // i < table_len
    }
    weights[(size_t)g * weight_stride + kk] = w;  // kk < K <= the stride
  }
  u64 sw = w, sw2 = (u64)w * w;
  uint32_t cnt = (w != 0u ? 1u : 0u) | (clamped << 16);  // (at most 64 of each in a wave)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sw += __shfl_xor(sw, d, 64);
    sw2 += __shfl_xor(sw2, d, 64);
    cnt += __shfl_xor(cnt, d, 64);
  }
  if ((tid & 63u) == 0u) {
    atomicAdd(&s_sum[0], sw);
    atomicAdd(&s_sum[1], sw2);
    atomicAdd(&s_cnt[0], cnt & 0xFFFFu);
    atomicAdd(&s_cnt[1], cnt >> 16);
  }
  __syncthreads();
  if (tid == 0u) {
    mp_u32x4 a, b;
    a.x = s_cnt[0];
    a.y = s_cnt[1];
    a.z = (uint32_t)s_sum[0];
    a.w = (uint32_t)(s_sum[0] >> 32);
    b.x = (uint32_t)s_sum[1];
    b.y = (uint32_t)(s_sum[1] >> 32);
    b.z = b.w = 0u;
    mp_u32x4 *rec = reinterpret_cast<mp_u32x4 *>(scratch + kMpWRecord * ((size_t)g * gridDim.x + blockIdx.x));
    rec[0] = a;  // (the scratch is 16-byte aligned, a record is 32 bytes)
    rec[1] = b;
  }
}

// the header's QUANTISATION; false: not in range
__device__ __forceinline__ bool mp_quant(float4 d, float xy_scale, int32_t *H, int32_t *X, int32_t *Y) {
  const float h = __fdiv_rn(d.y, __fadd_rn(1.0f, d.x));
  const float th = __fmul_rn(h, 1048576.0f), tx = __fmul_rn(d.z, xy_scale), ty = __fmul_rn(d.w, xy_scale);
  if (!(fabsf(th) < 8388608.0f && fabsf(tx) < 8388608.0f && fabsf(ty) < 8388608.0f)) return false;
  *H = (int32_t)rintf(th);
  *X = (int32_t)rintf(tx);
  *Y = (int32_t)rintf(ty);
  return true;
}

// grid (chunks, G); tw_log: log2 of the lanes of steps
__global__ __launch_bounds__(kMpBlock) void k_mppi_sums(const MppiK k, uint32_t tw_log,
                                                        const float *__restrict__ delta, u64 delta_stride,
                                                        uint32_t delta_per_group, uint32_t K,
                                                        const uint32_t *__restrict__ weights, u64 weight_stride,
                                                        uint32_t *__restrict__ scratch_sums) {
  __shared__ u64 s_acc[5u * kMpBlock];
  const uint32_t tid = threadIdx.x, g = blockIdx.y, chunk = blockIdx.x;
  const uint32_t tw = 1u << tw_log, rows = kMpBlock >> tw_log, t = tid & (tw - 1u), r = tid >> tw_log;
  const uint32_t T_e = k.steps_e;
  for (uint32_t i = tid; i < 5u * tw; i += kMpBlock) s_acc[i] = 0ull;
  __syncthreads();
  const float4 *dl = reinterpret_cast<const float4 *>(delta + (size_t)(delta_per_group ? g : 0u) * delta_stride);
  const uint32_t *wg = weights + (size_t)g * weight_stride;
  const uint32_t k0 = chunk * rows * RPLGPU_MPPI_PER_LANE + r;
  MpAcc a{0ull, 0ull, 0ull, 0ull, 0u};
#pragma unroll
  for (uint32_t j = 0; j < RPLGPU_MPPI_PER_LANE; ++j) {
    const uint32_t kk = k0 + j * rows;
    if (kk >= K || t >= T_e) continue;
    const uint32_t w = wg[kk];
    if (w == 0u) continue;
    const float4 d = dl[(size_t)kk * T_e + t];  // < K T_e <= the stride / 4
    int32_t H, X, Y;
    if (!mp_quant(d, k.xy_scale, &H, &X, &Y)) {
      ++a.off;
      continue;
    }
    a.w += w;
    a.h += (u64)((i64)w * H);
    a.x += (u64)((i64)w * X);
    a.y += (u64)((i64)w * Y);
  }
  mp_block_fold(a, tw, t, s_acc);
  __syncthreads();
  if (tid < T_e && tid < tw) {  // row 0: t = tid
    const u64 *v = s_acc + 5u * tid;
    mp_u32x4 q0, q1, q2;
    q0.x = (uint32_t)v[0]; q0.y = (uint32_t)(v[0] >> 32); q0.z = (uint32_t)v[1]; q0.w = (uint32_t)(v[1] >> 32);
    q1.x = (uint32_t)v[2]; q1.y = (uint32_t)(v[2] >> 32); q1.z = (uint32_t)v[3]; q1.w = (uint32_t)(v[3] >> 32);
    q2.x = (uint32_t)v[4]; q2.y = q2.z = q2.w = 0u;
    mp_u32x4 *rec = reinterpret_cast<mp_u32x4 *>(
        scratch_sums + kMpSRecord * (((size_t)g * gridDim.x + chunk) * T_e + tid));  // 48 bytes a record
    rec[0] = q0;
    rec[1] = q1;
    rec[2] = q2;
  }
}

__device__ __forceinline__ double mp_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double mp_add(double a, double b) { return __dadd_rn(a, b); }

// grid (G)
__global__ __launch_bounds__(kMpBlock) void k_mppi_close(const MppiK k, uint32_t tw_log, uint32_t chunks,
                                                         uint32_t w_blocks, const uint32_t *__restrict__ scratch_w,
                                                         const uint32_t *__restrict__ scratch_sums,
                                                         const float *nominal, u64 nominal_stride,
                                                         uint32_t nominal_per_group, uint32_t *__restrict__ sums,
                                                         u64 sums_stride, float *nominal_out, u64 nominal_out_stride,
                                                         uint32_t *__restrict__ result) {
  __shared__ u64 s_acc[5u * kMpBlock];
  __shared__ u64 s_sum[2];
  __shared__ uint32_t s_cnt[4];  // w != 0, clamped, entries off range, a step without weight
  const uint32_t tid = threadIdx.x, g = blockIdx.x;
  const uint32_t tw = 1u << tw_log, rows = kMpBlock >> tw_log, t = tid & (tw - 1u), r = tid >> tw_log;
  const uint32_t T_e = k.steps_e;
  for (uint32_t i = tid; i < 5u * tw; i += kMpBlock) s_acc[i] = 0ull;
  if (tid < 2u) s_sum[tid] = 0ull;
  if (tid < 4u) s_cnt[tid] = 0u;
  __syncthreads();
  // the sums records: [chunk][step], twelve words each
  MpAcc a{0ull, 0ull, 0ull, 0ull, 0u};
  if (t < T_e) {
    const mp_u32x4 *recs = reinterpret_cast<const mp_u32x4 *>(scratch_sums + kMpSRecord * (size_t)g * chunks * T_e);
    for (uint32_t c = r; c < chunks; c += rows) {  // chunks: an argument of the launch
      const mp_u32x4 *rec = recs + 3u * ((size_t)c * T_e + t);
      const mp_u32x4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
      a.w += (u64)q0.x | ((u64)q0.y << 32);
      a.h += (u64)q0.z | ((u64)q0.w << 32);
      a.x += (u64)q1.x | ((u64)q1.y << 32);
      a.y += (u64)q1.z | ((u64)q1.w << 32);
      a.off += q2.x;
    }
  }
  mp_block_fold(a, tw, t, s_acc);
  // the weight records
  {
    const mp_u32x4 *recs = reinterpret_cast<const mp_u32x4 *>(scratch_w + kMpWRecord * (size_t)g * w_blocks);
    u64 sw = 0ull, sw2 = 0ull;
    uint32_t cnt = 0u, clamped = 0u;
    for (uint32_t i = tid; i < w_blocks; i += kMpBlock) {  // at most 16 rounds
      const mp_u32x4 q0 = recs[2u * (size_t)i], q1 = recs[2u * (size_t)i + 1u];
      cnt += q0.x;
      clamped += q0.y;
      sw += (u64)q0.z | ((u64)q0.w << 32);
      sw2 += (u64)q1.x | ((u64)q1.y << 32);
    }
    if (tid < w_blocks) {
      atomicAdd(&s_sum[0], sw);
      atomicAdd(&s_sum[1], sw2);
      atomicAdd(&s_cnt[0], cnt);
      atomicAdd(&s_cnt[1], clamped);
    }
  }
  __syncthreads();
  if (tid < T_e && tid < tw) {  // row 0: the finish of step tid
    const u64 *v = s_acc + 5u * tid;
    const u64 W = v[0];
    mp_u32x4 q0, q1;
    q0.x = (uint32_t)v[0]; q0.y = (uint32_t)(v[0] >> 32); q0.z = (uint32_t)v[1]; q0.w = (uint32_t)(v[1] >> 32);
    q1.x = (uint32_t)v[2]; q1.y = (uint32_t)(v[2] >> 32); q1.z = (uint32_t)v[3]; q1.w = (uint32_t)(v[3] >> 32);
    mp_u32x4 *so = reinterpret_cast<mp_u32x4 *>(sums + (size_t)g * sums_stride) + 2u * (size_t)tid;
    so[0] = q0;
    so[1] = q1;
    mp_u32x4 nd;
    if (W != 0ull) {
      const double dW = __ull2double_rn(W);
      const double hb = mp_mul(__ddiv_rn(__ll2double_rn((i64)v[1]), dW), 1.0 / 1048576.0);
      const double hh = mp_mul(hb, hb);
      const double den = mp_add(1.0, hh);
      const double dc = __ddiv_rn(mp_add(1.0, -hh), den);
      const double ds = __ddiv_rn(mp_add(hb, hb), den);
      const double sc = (double)k.xy_scale;
      const double dx = __ddiv_rn(__ddiv_rn(__ll2double_rn((i64)v[2]), dW), sc);
      const double dy = __ddiv_rn(__ddiv_rn(__ll2double_rn((i64)v[3]), dW), sc);
      nd.x = __float_as_uint(__double2float_rn(dc));
      nd.y = __float_as_uint(__double2float_rn(ds));
      nd.z = __float_as_uint(__double2float_rn(dx));
      nd.w = __float_as_uint(__double2float_rn(dy));
    } else {
      nd.x = 0x3F800000u;
      nd.y = nd.z = nd.w = 0u;
      if (nominal)  // read before the store below: nominal_out may be nominal
        nd = reinterpret_cast<const mp_u32x4 *>(nominal + (size_t)(nominal_per_group ? g : 0u) * nominal_stride)[tid];
      atomicOr(&s_cnt[3], 1u);
    }
    reinterpret_cast<mp_u32x4 *>(nominal_out + (size_t)g * nominal_out_stride)[tid] = nd;
    if (v[4] != 0ull) atomicAdd(&s_cnt[2], (uint32_t)v[4]);
  }
  __syncthreads();
  if (tid == 0u) {
    uint32_t *res = result + 8u * (size_t)g;
    res[0] = s_cnt[0];
    res[1] = s_cnt[1];
    res[2] = (uint32_t)s_sum[0];
    res[3] = (uint32_t)(s_sum[0] >> 32);
    res[4] = (uint32_t)s_sum[1];
    res[5] = (uint32_t)(s_sum[1] >> 32);
    res[6] = s_cnt[2];
    res[7] = (s_cnt[0] == 0u ? RPLGPU_MPPI_NO_WEIGHT : 0u) | (s_cnt[2] != 0u ? RPLGPU_MPPI_OFF_RANGE : 0u) |
             (s_cnt[3] != 0u ? RPLGPU_MPPI_EMPTY_STEP : 0u);
  }
}

__device__ __forceinline__ uint32_t mp_canon(float v) { return v != v ? 0x7FC00000u : __float_as_uint(v); }

// grid (ceil(K T / 256), G): a thread per (candidate, step); in place when out is noise
__global__ __launch_bounds__(kMpBlock) void k_mppi_spread(const float *__restrict__ nominal, u64 nominal_stride,
                                                          uint32_t nominal_per_group, uint32_t T_n, const float *noise,
                                                          u64 noise_stride, uint32_t noise_per_group, uint32_t n,
                                                          uint32_t T, uint32_t shift, uint32_t keep_first, float *out,
                                                          u64 out_stride) {
  const uint32_t e = blockIdx.x * kMpBlock + threadIdx.x, g = blockIdx.y;
  if (e >= n) return;  // n = K T <= 2^24
  const uint32_t t = e % T;
  const uint32_t idx = min(t + shift, T_n - 1u);
  const mp_u32x4 pb =
      reinterpret_cast<const mp_u32x4 *>(nominal + (size_t)(nominal_per_group ? g : 0u) * nominal_stride)[idx];
  const float4 d = reinterpret_cast<const float4 *>(noise + (size_t)(noise_per_group ? g : 0u) * noise_stride)[e];
  mp_u32x4 o = pb;
  if (!(keep_first && e < T)) {  // E16's MOVE with the nominal delta as the pose
    const float c = __uint_as_float(pb.x), s = __uint_as_float(pb.y), x = __uint_as_float(pb.z),
                y = __uint_as_float(pb.w);
    o.x = mp_canon(__fsub_rn(__fmul_rn(c, d.x), __fmul_rn(s, d.y)));
    o.y = mp_canon(__fadd_rn(__fmul_rn(s, d.x), __fmul_rn(c, d.y)));
    o.z = mp_canon(__fadd_rn(__fsub_rn(__fmul_rn(c, d.z), __fmul_rn(s, d.w)), x));
    o.w = mp_canon(__fadd_rn(__fadd_rn(__fmul_rn(s, d.z), __fmul_rn(c, d.w)), y));
  }
  reinterpret_cast<mp_u32x4 *>(out + (size_t)g * out_stride)[e] = o;  // e < K T <= the stride / 4
}

}  // namespace

hipError_t launch_mppi_update(hipStream_t s, const MppiK &k, const uint32_t *out, unsigned long long out_stride,
                              const uint32_t *rollout_result, const float *delta, unsigned long long delta_stride,
                              uint32_t delta_per_group, const uint16_t *table, const float *nominal,
                              unsigned long long nominal_stride, uint32_t nominal_per_group, uint32_t G, uint32_t K,
                              uint32_t *weights, unsigned long long weight_stride, uint32_t *sums,
                              unsigned long long sums_stride, float *nominal_out,
                              unsigned long long nominal_out_stride, uint32_t *result, uint32_t *scratch) {
  MppiLayout l;
  const uint32_t T_e = k.steps_e;
  if (!mppi_layout(G, K, T_e, &l) || k.table_len == 0 || k.table_len > RPLGPU_MPPI_MAX_TABLE ||
      k.shift > RPLGPU_MPPI_MAX_SHIFT || out_stride < 8ull * K || delta_stride < 4ull * K * T_e ||
      weight_stride < K || sums_stride < 8ull * T_e || nominal_out_stride < 4ull * T_e ||
      (nominal && nominal_stride < 4ull * T_e) || (reinterpret_cast<uintptr_t>(scratch) & 15u))
    return hipErrorInvalidValue;
  uint32_t *scratch_sums = scratch + l.w_words;
  hipLaunchKernelGGL(k_mppi_weights, dim3(l.w_blocks, G), dim3(kMpBlock), 0, s, k, out, out_stride, rollout_result,
                     table, K, weights, weight_stride, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mppi_sums, dim3(l.chunks, G), dim3(kMpBlock), 0, s, k, l.tw_log, delta, delta_stride,
                     delta_per_group, K, weights, weight_stride, scratch_sums);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mppi_close, dim3(G), dim3(kMpBlock), 0, s, k, l.tw_log, l.chunks, l.w_blocks, scratch,
                     scratch_sums, nominal, nominal_stride, nominal_per_group, sums, sums_stride, nominal_out,
                     nominal_out_stride, result);
  return hipGetLastError();
}

hipError_t launch_mppi_spread(hipStream_t s, const float *nominal, unsigned long long nominal_stride,
                              uint32_t nominal_per_group, uint32_t T_n, const float *noise,
                              unsigned long long noise_stride, uint32_t noise_per_group, uint32_t G, uint32_t K,
                              uint32_t T, uint32_t shift, uint32_t keep_first, float *out,
                              unsigned long long out_stride) {
  const u64 n = (u64)K * T;
  if (G == 0 || G > 65535u || K == 0 || K > RPLGPU_MAX_POSES || T == 0 || T > RPLGPU_ROLLOUT_MAX_STEPS || T_n == 0 ||
      T_n > RPLGPU_ROLLOUT_MAX_STEPS || n > (1ull << 24) || shift > RPLGPU_MPPI_MAX_SPREAD_SHIFT ||
      nominal_stride < 4ull * T_n || noise_stride < 4ull * n || out_stride < 4ull * n)
    return hipErrorInvalidValue;
  const uint32_t blocks = (uint32_t)((n + kMpBlock - 1u) / kMpBlock);
  if ((u64)blocks * G > RPLGPU_MPPI_MAX_BLOCKS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mppi_spread, dim3(blocks, G), dim3(kMpBlock), 0, s, nominal, nominal_stride, nominal_per_group,
                     T_n, noise, noise_stride, noise_per_group, (uint32_t)n, T, shift, keep_first, out, out_stride);
  return hipGetLastError();
}

}  // namespace rpl
