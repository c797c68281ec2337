// rpl_resample.hip — E16: a weighted pose list resampled and moved, include/rplgpu_msg.h,
// rplgpu_resample_poses_dev: E15's weights and the list they weigh become the list of the next time step.
// Systematic (low-variance) resampling in integers: with S the sum of the weights, C their inclusive running sum and
// r = floor(u S / 2^32) from the caller's one random word, output j descends from the smallest i with
// C[i] > t_j = floor((j S + r) / M); then the odometry increment is composed on the right, or the 16 bytes are copied.
//
// Three launches, 1024 poses per tile, no workgroup waits on another and no loop is bounded by a word from memory:
//   k_resample_tiles  per tile the 64-bit sum, the 96-bit sum of squares (64 bits + a carry count) and the number
//                     of weights that are not 0;
//   k_resample_scan   per group the exclusive scan of the tile sums, S, q = S / M, rho = S % M and r, and per tile
//                     the first output that descends from it, b[t] = J(base[t]): t_j is non-decreasing in j, so J is
//                     found by a bisection of 21 fixed steps over j in [0, M].  Result words 0 - 5 and 7;
//   k_resample_emit   per tile with outputs the inclusive 64-bit scan of its 1024 weights in LDS, then the workgroup
//                     walks the OUTPUTS b[t] + tid, + 1024, ...: one t_j, a bisection of 10 fixed steps over the LDS
//                     scan, one 16-byte load, the copy or the move, one 16-byte store and the ancestor word.
//                     Distinct ancestors: 1024 LDS flags set by plain stores, counted once, one atomic add per tile.
// The scratch of a group (uint32 words; T tiles): 16 header words | T records of 8 | T + 1 boundaries (padded to an
// even count).  Header: S, q, rho, r as 64-bit values, then the S = 0 flag.  Record: tile sum, squares low (both 64
// bit), carry count, non-zero count, then the tile's base (64 bit, written by the scan).
//
// S = 0: a[j] = j mod P has no tile structure, so the scan hands tile t the outputs [t * ceil(M / T), ...) and
// the emit kernel takes j mod P; word 6 is min(M, P) and comes from the scan.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef unsigned long long u64;
typedef uint32_t rs_u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kRsTile = kBlock;  // poses per tile: one per thread
constexpr uint32_t kRsHeader = 16u;   // words
constexpr uint32_t kRsRecord = 8u;    // words per tile
static_assert(kRsTile == 1024u, "the emit kernel's bisection has 10 steps");
static_assert(RPLGPU_MAX_POSES / kRsTile <= (uint32_t)kBlock, "one workgroup scans a group's tile sums");
static_assert(RPLGPU_MAX_POSES <= (1u << 20), "J's bisection has 21 steps");

__host__ __device__ inline uint32_t rs_tiles(uint32_t P) { return (P + kRsTile - 1u) / kRsTile; }
__host__ __device__ inline uint32_t rs_bounds_words(uint32_t T) { return (T + 2u) & ~1u; }  // T + 1, even
__host__ __device__ inline u64 rs_group_words(uint32_t T) {
  return (u64)kRsHeader + (u64)kRsRecord * T + rs_bounds_words(T);
}

// t_j = floor((j S + r) / M) with S = q M + rho: every term below 2^63
__device__ __forceinline__ u64 rs_t(uint32_t j, u64 q, u64 rho, u64 r, uint32_t M) {
  return (u64)j * q + ((u64)j * rho + r) / M;
}

// inclusive scan of one 64-bit value per thread over the workgroup; s_wave: kWaves words of LDS.  Two barriers.
__device__ __forceinline__ u64 rs_block_incl_scan(u64 v, u64 *s_wave) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(v, d, 64);
    if ((int)lane_id() >= d) v += o;
  }
  if (lane_id() == 63u) s_wave[wave_id()] = v;
  __syncthreads();
  u64 before = 0ull;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) before += (uint32_t)w < wave_id() ? s_wave[w] : 0ull;
  __syncthreads();  // (s_wave may be used again)
  return v + before;
}

__global__ __launch_bounds__(kBlock) void k_resample_tiles(const uint32_t *__restrict__ weights,
                                                           u64 weight_stride, uint32_t P,
                                                           uint32_t *__restrict__ scratch) {
  __shared__ u64 s_sum[kWaves];
  __shared__ u64 s_sq[kWaves];
  __shared__ uint32_t s_carry[kWaves];
  __shared__ uint32_t s_nz[kWaves];
  const uint32_t tile = blockIdx.x, g = blockIdx.y;
  const uint32_t T = rs_tiles(P);
  const uint32_t i = tile * kRsTile + threadIdx.x;
  const uint32_t w = i < P ? weights[(size_t)g * weight_stride + i] : 0u;
  u64 sum = w, sq = (u64)w * w;
  uint32_t carry = 0u, nz = w != 0u ? 1u : 0u;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sum += __shfl_xor(sum, d, 64);
    const u64 o = __shfl_xor(sq, d, 64);
    carry += __shfl_xor(carry, d, 64);
    sq += o;
    carry += sq < o ? 1u : 0u;  // (both lanes of a pair see the same wrap)
    nz += __shfl_xor(nz, d, 64);
  }
  if (lane_id() == 0) {
    s_sum[wave_id()] = sum;
    s_sq[wave_id()] = sq;
    s_carry[wave_id()] = carry;
    s_nz[wave_id()] = nz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t_sum = 0ull, t_sq = 0ull;
    uint32_t t_carry = 0u, t_nz = 0u;
    for (int k = 0; k < kWaves; ++k) {
      t_sum += s_sum[k];
      t_sq += s_sq[k];
      t_carry += s_carry[k] + (t_sq < s_sq[k] ? 1u : 0u);
      t_nz += s_nz[k];
    }
    uint32_t *rec = scratch + (size_t)g * rs_group_words(T) + kRsHeader + (size_t)kRsRecord * tile;
    *reinterpret_cast<u64 *>(rec) = t_sum;
    *reinterpret_cast<u64 *>(rec + 2) = t_sq;
    rec[4] = t_carry;
    rec[5] = t_nz;
  }
}

__global__ __launch_bounds__(kBlock) void k_resample_scan(uint32_t P, uint32_t M, const uint32_t *__restrict__ u_in,
                                                          uint32_t *__restrict__ scratch,
                                                          uint32_t *__restrict__ result) {
  __shared__ u64 s_wave[kWaves];
  __shared__ u64 s_sq[kWaves];
  __shared__ uint32_t s_carry[kWaves];
  __shared__ uint32_t s_nz[kWaves];
  __shared__ u64 s_head[4];  // S, q, rho, r
  const uint32_t g = blockIdx.x;
  const uint32_t T = rs_tiles(P);
  uint32_t *grp = scratch + (size_t)g * rs_group_words(T);
  uint32_t *rec = grp + kRsHeader + (size_t)kRsRecord * threadIdx.x;
  uint32_t *bounds = grp + kRsHeader + (size_t)kRsRecord * T;
  const bool own = threadIdx.x < T;
  const u64 mine = own ? *reinterpret_cast<const u64 *>(rec) : 0ull;
  u64 sq = own ? *reinterpret_cast<const u64 *>(rec + 2) : 0ull;
  uint32_t carry = own ? rec[4] : 0u, nz = own ? rec[5] : 0u;
  const u64 incl = rs_block_incl_scan(mine, s_wave);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = __shfl_xor(sq, d, 64);
    carry += __shfl_xor(carry, d, 64);
    sq += o;
    carry += sq < o ? 1u : 0u;
    nz += __shfl_xor(nz, d, 64);
  }
  if (lane_id() == 0) {
    s_sq[wave_id()] = sq;
    s_carry[wave_id()] = carry;
    s_nz[wave_id()] = nz;
  }
  if (threadIdx.x == kBlock - 1) s_head[0] = incl;  // S
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 S = s_head[0];
    const uint32_t u = u_in ? u_in[g] : 0u;
    const u64 q = S / M, rho = S % M;
    const u64 r = (u64)u * (S >> 32) + (((u64)u * (S & 0xffffffffull)) >> 32);  // floor(u S / 2^32) < S
    s_head[1] = q;
    s_head[2] = rho;
    s_head[3] = r;
    u64 t_sq = 0ull;
    uint32_t t_carry = 0u, t_nz = 0u;
    for (int k = 0; k < kWaves; ++k) {
      t_sq += s_sq[k];
      t_carry += s_carry[k] + (t_sq < s_sq[k] ? 1u : 0u);
      t_nz += s_nz[k];
    }
    u64 *head = reinterpret_cast<u64 *>(grp);
    head[0] = S;
    head[1] = q;
    head[2] = rho;
    head[3] = r;
    grp[8] = S == 0ull ? 1u : 0u;
    uint32_t *res = result + 8u * (size_t)g;
    res[0] = (uint32_t)S;
    res[1] = (uint32_t)(S >> 32);
    res[2] = (uint32_t)t_sq;
    res[3] = (uint32_t)(t_sq >> 32);
    res[4] = t_carry;
    res[5] = t_nz;
    res[6] = S == 0ull ? min(M, P) : 0u;  // (otherwise the emit kernel adds its tiles' distinct ancestors)
    res[7] = S == 0ull ? 1u : 0u;
    bounds[T] = M;
  }
  __syncthreads();
  if (!own) return;
  const u64 S = s_head[0], q = s_head[1], rho = s_head[2], r = s_head[3];
  const u64 base = incl - mine;
  *reinterpret_cast<u64 *>(rec + 6) = base;
  uint32_t first;
  if (S == 0ull) {
    const uint32_t chunk = (M + T - 1u) / T;
    first = (uint32_t)min((u64)threadIdx.x * chunk, (u64)M);
  } else {
    // J(base): the number of outputs with t_j < base = the smallest j in [0, M] whose t_j >= base
    uint32_t lo = 0u, hi = M;
#pragma unroll 1
    for (int step = 0; step < 21; ++step) {
      const uint32_t mid = (lo + hi) >> 1;
      const bool below = mid < hi && rs_t(mid, q, rho, r, M) < base;
      lo = below ? mid + 1u : lo;
      hi = below ? hi : mid;
    }
    first = lo;
  }
  bounds[threadIdx.x] = first;
}

template <bool MOVE>
__global__ __launch_bounds__(kBlock) void k_resample_emit(
    const uint32_t *__restrict__ weights, u64 weight_stride, const float *__restrict__ poses, u64 pose_stride,
    uint32_t poses_per_group, uint32_t P, uint32_t M, const float *__restrict__ delta, uint32_t n_delta,
    u64 delta_stride, uint32_t delta_per_group, float *__restrict__ out, u64 out_stride,
    uint32_t *__restrict__ ancestors, u64 anc_stride, const uint32_t *__restrict__ scratch,
    uint32_t *__restrict__ result) {
  __shared__ u64 s_c[kRsTile];         // base + the inclusive scan of the tile's weights
  __shared__ uint32_t s_used[kRsTile];  // 1: the pose has a descendant
  __shared__ u64 s_wave[kWaves];
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t tile = blockIdx.x, g = blockIdx.y;
  const uint32_t T = rs_tiles(P);
  const uint32_t *grp = scratch + (size_t)g * rs_group_words(T);
  const uint32_t *bounds = grp + kRsHeader + (size_t)kRsRecord * T;
  const uint32_t b1 = min(bounds[tile + 1u], M);  // (no output index leaves [0, M), whatever the scratch holds)
  const uint32_t b0 = min(bounds[tile], b1);
  if (b0 == b1) return;  // (block-uniform) no output descends from this tile
  const u64 *head = reinterpret_cast<const u64 *>(grp);
  const u64 q = head[1], rho = head[2], r = head[3];
  const bool dead = grp[8] != 0u;  // S = 0
  const rs_u32x4 *src =
      reinterpret_cast<const rs_u32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride);
  rs_u32x4 *dst = reinterpret_cast<rs_u32x4 *>(out + (size_t)g * out_stride);
  const rs_u32x4 *dl =
      MOVE ? reinterpret_cast<const rs_u32x4 *>(delta + (size_t)(delta_per_group ? g : 0u) * delta_stride) : nullptr;
  uint32_t *anc = ancestors ? ancestors + (size_t)g * anc_stride : nullptr;
  if (!dead) {
    const uint32_t i = tile * kRsTile + threadIdx.x;
    const u64 w = i < P ? weights[(size_t)g * weight_stride + i] : 0u;
    const u64 base = *reinterpret_cast<const u64 *>(grp + kRsHeader + (size_t)kRsRecord * tile + 6u);
    s_c[threadIdx.x] = base + rs_block_incl_scan(w, s_wave);
    s_used[threadIdx.x] = 0u;
    __syncthreads();
  }
  for (uint32_t j = b0 + threadIdx.x; j < b1; j += kRsTile) {  // at most 1024 rounds: b1 <= M <= 2^20
    uint32_t a;
    if (dead) {
      a = j % P;
    } else {
      const u64 t = rs_t(j, q, rho, r, M);
      uint32_t pos = 0u;  // the smallest k with s_c[k] > t; pos + step - 1 <= 1022
#pragma unroll
      for (uint32_t step = kRsTile / 2u; step > 0u; step >>= 1) pos += s_c[pos + step - 1u] <= t ? step : 0u;
      s_used[pos] = 1u;
      a = min(tile * kRsTile + pos, P - 1u);  // (a pose of the list, whatever the scratch holds)
    }
    rs_u32x4 v = src[a];
    if (MOVE) {
      const rs_u32x4 dv = dl[n_delta == 1u ? 0u : j];
      const float c = __uint_as_float(v.x), s = __uint_as_float(v.y), x = __uint_as_float(v.z),
                  y = __uint_as_float(v.w);
      const float dc = __uint_as_float(dv.x), ds = __uint_as_float(dv.y), dx = __uint_as_float(dv.z),
                  dy = __uint_as_float(dv.w);
      const float c2 = c * dc - s * ds;
      const float s2 = s * dc + c * ds;
      const float x2 = (c * dx - s * dy) + x;
      const float y2 = (s * dx + c * dy) + y;
      // a NaN that the move makes is stored as 0x7FC00000: which payload survives is the implementation's choice
      v.x = c2 != c2 ? 0x7FC00000u : __float_as_uint(c2);
      v.y = s2 != s2 ? 0x7FC00000u : __float_as_uint(s2);
      v.z = x2 != x2 ? 0x7FC00000u : __float_as_uint(x2);
      v.w = y2 != y2 ? 0x7FC00000u : __float_as_uint(y2);
    }
    dst[j] = v;
    if (anc) anc[j] = a;
  }
  if (dead) return;  // (block-uniform; word 6 is the scan kernel's)
  __syncthreads();
  uint32_t cnt = s_used[threadIdx.x];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if (lane_id() == 0) s_cnt[wave_id()] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0u;
    for (int k = 0; k < kWaves; ++k) total += s_cnt[k];
    atomicAdd(&result[8u * (size_t)g + 6u], total);
  }
}

}  // namespace

unsigned long long resample_scratch_words(uint32_t G, uint32_t P) {
  if (G == 0 || P == 0 || P > RPLGPU_MAX_POSES) return 0ull;
  return (u64)G * rs_group_words(rs_tiles(P));
}

hipError_t launch_resample(hipStream_t s, const uint32_t *weights, unsigned long long weight_stride,
                           const float *poses, unsigned long long pose_stride, uint32_t poses_per_group, uint32_t G,
                           uint32_t P, uint32_t M, const uint32_t *u, const float *delta, uint32_t n_delta,
                           unsigned long long delta_stride, uint32_t delta_per_group, float *out,
                           unsigned long long out_stride, uint32_t *ancestors, unsigned long long anc_stride,
                           uint32_t *result, uint32_t *scratch) {
  if (G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || M == 0 || M > RPLGPU_MAX_POSES ||
      weight_stride < P || pose_stride < 4ull * P || out_stride < 4ull * M || (ancestors && anc_stride < M) ||
      (delta && n_delta != 1u && n_delta != M) || (delta && delta_stride < 4ull * n_delta))
    return hipErrorInvalidValue;
  const uint32_t T = rs_tiles(P);
  hipLaunchKernelGGL(k_resample_tiles, dim3(T, G), dim3(kBlock), 0, s, weights, weight_stride, P, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_resample_scan, dim3(G), dim3(kBlock), 0, s, P, M, u, scratch, result);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (delta)
    hipLaunchKernelGGL(k_resample_emit<true>, dim3(T, G), dim3(kBlock), 0, s, weights, weight_stride, poses,
                       pose_stride, poses_per_group, P, M, delta, n_delta, delta_stride, delta_per_group, out,
                       out_stride, ancestors, anc_stride, scratch, result);
  else
    hipLaunchKernelGGL(k_resample_emit<false>, dim3(T, G), dim3(kBlock), 0, s, weights, weight_stride, poses,
                       pose_stride, poses_per_group, P, M, delta, n_delta, delta_stride, delta_per_group, out,
                       out_stride, ancestors, anc_stride, scratch, result);
  return hipGetLastError();
}

}  // namespace rpl
