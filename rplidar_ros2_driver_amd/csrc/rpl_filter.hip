// rpl_filter.hip — E10: the scan-shadow (veiling / mixed-pixel) filter and the speckle filter on
// LaserScan arrays that are already in HBM (include/rplgpu_msg.h, rplgpu_filter_laserscan_batch_dev).
//
// Both are neighbourhood rules over ranges[] with a bounded reach: a beam's fate depends on the beams
// within W (pair tests) + N (removal window) + L (run search) <= 192 places on either side.  So a
// workgroup of 512 threads takes a TILE of 2048 beams plus that halo into LDS and long scans split into
// several tiles; nothing limits the scan length.  Per tile, every step a strided pass over LDS:
//   load      s_r[t]  = input bits of beam (tile0 - H + t); beams that do not exist read +inf, and with
//             `circular` the index is taken modulo count (a scan shorter than the halo repeats)
//   detect    s_d[t]  = r if the beam has a shadow pair among its 2W neighbours, else +inf
//             (s, c per distance y come from a table built once per tile; the side tests are the
//             exact-sign fp64 form of the header, so no atan2 is evaluated)
//   remove    s_p[t]  = quiet NaN if min(s_d[t-N .. t+N]) < r, else the input bits
//   link      one ballot word per 64 beams: beams t and t+1 both finite after removal and within D
//   write     run length = ones below + ones above the beam in the link words (ctz / clz across the
//             word boundary, each side capped at min(L, count) - 1); shorter than L: quiet NaN
// The positions within W + N + L of the tile's edge see fewer neighbours than they have; by
// construction nothing computed there reaches the TILE beams the workgroup writes.
// -ffp-contract=off keeps r1 - r2 * c and the fp64 cross terms as separate roundings (the spec).
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"

namespace rpl {
namespace {

constexpr uint32_t kFThreads = 512;
constexpr uint32_t kFTile = 2048;
constexpr uint32_t kFMaxHalo = 3u * RPLGPU_MAX_FILTER_WINDOW;
constexpr uint32_t kFSpan = kFTile + 2u * kFMaxHalo;
constexpr uint32_t kFWords = (kFSpan + kFThreads - 1u) / kFThreads * kFThreads / 64u;
constexpr uint32_t kQuietNaN = 0x7FC00000u;  // what a removed beam holds
constexpr uint32_t kInfBits = 0x7F800000u;

__device__ __forceinline__ bool finite_bits(uint32_t u) { return (u & kInfBits) != kInfBits; }

// sin / cos of E6 (rpl_xf.hpp's apply_xf) at a: the same float32 operations in the same order
__device__ __forceinline__ float2 e6_sincos(float a) {
  const float a2 = a * a;
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
  return make_float2(sn, cn);
}

// theta = atan2(a, b) lies below min_angle or above max_angle: the sign of the fp64 cross product of
// float vectors is exact (exact products, one rounding)
__device__ __forceinline__ bool shadow_pair(float r1, float r2, float2 sc, const FilterK &k) {
  const float a = r2 * sc.x;
  const float rc = r2 * sc.y;
  const float b = r1 - rc;
  const double da = (double)a, db = (double)b;
  const double below = (double)k.cmin * da - (double)k.smin * db;
  const double above = (double)k.cmax * da - (double)k.smax * db;
  return below < 0.0 || above > 0.0;
}

__global__ __launch_bounds__(kFThreads) void k_filter_scans(
    const uint32_t *__restrict__ ranges, const uint32_t *__restrict__ intens, uint32_t n_stride,
    const uint32_t *__restrict__ beam_count, FilterK k, uint32_t *__restrict__ ranges_out,
    uint32_t *__restrict__ intens_out, uint32_t *__restrict__ removed) {
  __shared__ uint32_t s_r[kFSpan];
  __shared__ float s_d[kFSpan];
  __shared__ uint32_t s_p[kFSpan];
  __shared__ unsigned long long s_w[kFWords];
  __shared__ float2 s_sc[RPLGPU_MAX_FILTER_WINDOW];
  __shared__ uint32_t s_cnt[2];

  const uint32_t b = blockIdx.y;
  const uint32_t count = beam_count ? min(beam_count[b], n_stride) : k.count;  // never past the scan's slot
  const uint32_t tile0 = blockIdx.x * kFTile;
  if (tile0 >= count) return;  // (also: a scan of no beams writes nothing)
  const uint32_t tile_n = min(kFTile, count - tile0);
  const uint32_t tid = threadIdx.x;

  float inc = k.inc;
  if (k.inc_mode != kFilterIncGiven) {  // as publish_scan states it (:635 Mode A, :666-668 Mode B)
    const double den = (k.inc_mode == kFilterIncModeA) ? (double)count : (double)(count > 1u ? count - 1u : 1u);
    inc = (float)(kTwoPi / den);
  }
  // on a circle no window reaches half way round, so no beam meets itself
  const uint32_t half = (count - 1u) / 2u;
  const uint32_t W = k.shadow ? (k.circular ? min(k.W, half) : k.W) : 0u;
  const uint32_t N = k.shadow ? (k.circular ? min(k.N, half) : k.N) : 0u;
  const uint32_t L = k.speckle ? k.L : 0u;
  const uint32_t H = W + N + L;
  const uint32_t P = tile_n + 2u * H;
  const uint32_t *r_in = ranges + (size_t)b * n_stride;
  const uint32_t *i_in = intens + (size_t)b * n_stride;
  uint32_t *r_out = ranges_out + (size_t)b * n_stride;
  uint32_t *i_out = intens_out + (size_t)b * n_stride;

  if (tid < W) s_sc[tid] = e6_sincos((float)(tid + 1u) * inc);
  if (tid < 2u) s_cnt[tid] = 0u;
  for (uint32_t t = tid; t < P; t += kFThreads) {
    int g = (int)(tile0 + t) - (int)H;
    if (g < 0 || g >= (int)count) {
      if (k.circular) {
        g %= (int)count;
        if (g < 0) g += (int)count;
      } else {
        g = -1;
      }
    }
    s_r[t] = (g >= 0) ? r_in[g] : kInfBits;
  }
  for (uint32_t j = tid; j < tile_n; j += kFThreads) i_out[tile0 + j] = i_in[tile0 + j];  // bit copy
  __syncthreads();

  uint32_t n_shadow = 0, n_speckle = 0;
  const uint32_t *post = s_r;
  if (k.shadow) {
    for (uint32_t t = tid; t < P; t += kFThreads) {
      const uint32_t u1 = s_r[t];
      bool det = false;
      if (finite_bits(u1)) {
        const float r1 = __uint_as_float(u1);
        for (uint32_t y = 1; y <= W; ++y) {
          if (!((float)y * inc <= 0.5f)) break;  // (monotone in y)
          const float2 sc = s_sc[y - 1u];
          if (t >= y) {
            const uint32_t u2 = s_r[t - y];
            if (finite_bits(u2)) det = det || shadow_pair(r1, __uint_as_float(u2), sc, k);
          }
          if (t + y < P) {
            const uint32_t u2 = s_r[t + y];
            if (finite_bits(u2)) det = det || shadow_pair(r1, __uint_as_float(u2), sc, k);
          }
        }
      }
      s_d[t] = det ? __uint_as_float(u1) : __builtin_inff();
    }
    __syncthreads();
    for (uint32_t t = tid; t < P; t += kFThreads) {
      const uint32_t u = s_r[t];
      bool rm = false;
      if (finite_bits(u)) {
        const uint32_t lo = t >= N ? t - N : 0u, hi = min(t + N, P - 1u);
        float m = __builtin_inff();
        for (uint32_t q = lo; q <= hi; ++q) m = fminf(m, s_d[q]);  // the nearest detected beam in reach
        rm = m < __uint_as_float(u);                                // only farther beams go
      }
      s_p[t] = rm ? kQuietNaN : u;
      if (rm && t >= H && t < H + tile_n) ++n_shadow;
    }
    post = s_p;
    __syncthreads();
  }
  if (k.speckle) {
    for (uint32_t base = 0; base < P; base += kFThreads) {  // (whole waves: the ballot needs every lane)
      const uint32_t t = base + tid;
      bool link = false;
      if (t + 1u < P) {
        const uint32_t u0 = post[t], u1 = post[t + 1u];
        link = finite_bits(u0) && finite_bits(u1) &&
               fabsf(__uint_as_float(u1) - __uint_as_float(u0)) <= k.D;
      }
      const unsigned long long w = __builtin_amdgcn_ballot_w64(link);
      if (lane_id() == 0) s_w[t >> 6] = w;
    }
    __syncthreads();
  }
  const uint32_t cap = L ? min(L, count) - 1u : 0u;
  for (uint32_t j = tid; j < tile_n; j += kFThreads) {
    const uint32_t t = H + j;
    uint32_t u = post[t];
    if (k.speckle && finite_bits(u)) {
      const uint32_t wi = t >> 6, sh = t & 63u;
      const unsigned long long w0 = s_w[wi];
      // bit 0 = link t -> t+1, upwards; and bit 63 = link t-1 -> t, downwards.  s_w[wi + 1] may be a word
      // no ballot wrote (in bounds: kFWords covers the padded span); its bits are never counted, because
      // the link bit of position P - 1 is always 0 and lies at or below them, so ctz stops there
      const unsigned long long up = sh ? (w0 >> sh) | (s_w[wi + 1u] << (64u - sh)) : w0;
      const unsigned long long wb = wi ? s_w[wi - 1u] : 0ull;
      const unsigned long long dn = sh ? (w0 << (64u - sh)) | (wb >> sh) : wb;
      const uint32_t right = min(~up ? (uint32_t)__builtin_ctzll(~up) : 64u, cap);
      const uint32_t left = min(~dn ? (uint32_t)__builtin_clzll(~dn) : 64u, cap);
      // a run that closes the circle is seen from both sides: it has count beams
      if (min(left + right + 1u, count) < L) {
        u = kQuietNaN;
        ++n_speckle;
      }
    }
    r_out[tile0 + j] = u;
  }
  if (removed) {
    const uint32_t ws = wave_incl_scan_fast(n_shadow), wk = wave_incl_scan_fast(n_speckle);
    if (lane_id() == 63) {
      if (ws) atomicAdd(&s_cnt[0], ws);
      if (wk) atomicAdd(&s_cnt[1], wk);
    }
    __syncthreads();
    if (tid < 2u && s_cnt[tid]) atomicAdd(&removed[2u * b + tid], s_cnt[tid]);
  }
}

}  // namespace

hipError_t launch_filter_scans(hipStream_t s, const float *ranges, const float *intens, uint32_t n_stride,
                               const uint32_t *beam_count, uint32_t B, const FilterK &k, float *ranges_out,
                               float *intens_out, uint32_t *removed) {
  const uint32_t longest = beam_count ? n_stride : k.count;
  if (B == 0 || longest == 0) return hipSuccess;
  if (k.W > RPLGPU_MAX_FILTER_WINDOW || k.N > RPLGPU_MAX_FILTER_WINDOW || k.L > RPLGPU_MAX_FILTER_WINDOW ||
      (!beam_count && k.count > n_stride) || longest > (1u << 30))  // (beam indices are ints in the kernel)
    return hipErrorInvalidValue;
  // (tiles of the longest scan the layout admits: a tile beyond its scan's count returns at once)
  const uint32_t tiles = (longest + kFTile - 1u) / kFTile;
  for (uint32_t b0 = 0; b0 < B; b0 += 65535u) {  // gridDim.y limit
    const uint32_t nb = min(B - b0, 65535u);
    const size_t o = (size_t)b0 * n_stride;
    hipLaunchKernelGGL(k_filter_scans, dim3(tiles, nb), dim3(kFThreads), 0, s,
                       reinterpret_cast<const uint32_t *>(ranges) + o,
                       reinterpret_cast<const uint32_t *>(intens) + o, n_stride,
                       beam_count ? beam_count + b0 : nullptr, k, reinterpret_cast<uint32_t *>(ranges_out) + o,
                       reinterpret_cast<uint32_t *>(intens_out) + o, removed ? removed + 2u * (size_t)b0 : nullptr);
  }
  return hipGetLastError();
}

}  // namespace rpl
