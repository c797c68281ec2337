// rpl_rollout.hip — E27: candidate motions rolled out of a pose and scored, include/rplgpu_msg.h, rplgpu_rollout_dev.
// K candidates per group, each a chain of T compositions (E16's MOVE) that no prefix trick may reorder, and behind
// every pose F + 1 dependent gathers: the footprint's bytes of the costmap and the centre's word of E26's field.
//
// Two launches, no workgroup waits for another:
//   k_rollout_tiles  a workgroup of 256 threads takes a tile of 32 candidates of one group and walks T in chunks of 32
//                    steps.  Phase 1: a lane per candidate rolls the chunk and leaves its poses in LDS (per-step deltas
//                    are staged there first by all lanes: a candidate's are contiguous, a lane reading its own row would
//                    stride by 16 T bytes).  Phase 2: all lanes spread over (point, step, candidate), candidate
//                    fastest; a look-up folds into the pose's word by one LDS atomicMax (a value, 0x100 blocked,
//                    0x300 blocked off range), the centre's D is a plain store.  Phase 3: the candidate's lane scans
//                    the chunk's words in order for n, the sums and D.  25 KB of LDS: six workgroups a CU.
//                    Behind the last chunk the lane writes its eight words and the end pose, and wave 0 folds the
//                    tile's (score, k) minimum and counts into the tile's record.
//   k_rollout_close  a workgroup per group folds the records into the result words.
// Everything behind the cell rule is integers and every fold is a minimum or a sum: no order shows.
#include <hip/hip_runtime.h>

#include "rpl_grid.hpp"
#include "rpl_rollout.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef unsigned long long u64;
typedef uint32_t ro_u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kRoBlock = 256u;
constexpr uint32_t kRoTile = RPLGPU_ROLLOUT_TILE;  // candidates per workgroup
constexpr uint32_t kRoChunk = 32u;                 // steps per pass over the LDS
constexpr uint32_t kRoRow = kRoTile + 1u;          // poses per step in LDS (padded: the staging writes step-fastest)
constexpr uint32_t kRoBlockedWord = 0x100u, kRoRangeWord = 0x300u;  // above every value that does not block
constexpr uint32_t kRoRecord = 8u;
static_assert(kRoTile == 32u && kRoChunk == 32u, "the index arithmetic below shifts by 5");
static_assert(kRoTile <= 64u, "one wave folds a tile");

__device__ __forceinline__ float ro_canon(float v) { return v != v ? __uint_as_float(0x7FC00000u) : v; }

// E16's MOVE, operation for operation
__device__ __forceinline__ float4 ro_move(float4 p, float4 d) {
  const float c = p.x, s = p.y, x = p.z, y = p.w;
  const float c2 = c * d.x - s * d.y;
  const float s2 = s * d.x + c * d.y;
  const float x2 = (c * d.z - s * d.w) + x;
  const float y2 = (s * d.z + c * d.w) + y;
  return make_float4(ro_canon(c2), ro_canon(s2), ro_canon(x2), ro_canon(y2));
}

// the VALUE of the footprint point (fx, fy) at pose q, or one of the two blocked words
__device__ __forceinline__ uint32_t ro_point(const RolloutK &k, float4 q, float fx, float fy,
                                             const int8_t *__restrict__ grid) {
  const float rx = (q.x * fx - q.y * fy) + q.z;
  const float ry = (q.y * fx + q.x * fy) + q.w;
  int cx, cy;
  if (!grid_cell(rx, ry, k.origin_x, k.origin_y, k.resolution, &cx, &cy)) return kRoRangeWord;
  if ((uint32_t)cx >= k.width || (uint32_t)cy >= k.height) return kRoBlockedWord;
  const int v = grid[(uint32_t)cy * k.width + (uint32_t)cx];  // < width * height <= the grid's stride
  const uint32_t p = v >= 0 ? (uint32_t)v : k.unknown_value;
  return p >= k.lethal ? kRoBlockedWord : p;
}

// D at the centre of pose q
__device__ __forceinline__ uint32_t ro_centre(const RolloutK &k, float4 q, const uint32_t *__restrict__ potential) {
  int cx, cy;
  if (!grid_cell(q.z, q.w, k.origin_x, k.origin_y, k.resolution, &cx, &cy)) return RPLGPU_NAV_UNREACHED;
  if ((uint32_t)cx >= k.width || (uint32_t)cy >= k.height) return RPLGPU_NAV_UNREACHED;
  return potential[(uint32_t)cy * k.width + (uint32_t)cx];
}

struct RoCand {  // what a lane holds of its candidate while it walks T
  uint32_t n, flags, cost_sum, cost_max, d_end, d_min;
  ro_u32x4 end_pose;
};

__device__ __forceinline__ ro_u32x4 ro_bits(float4 p) {
  ro_u32x4 v;
  v.x = __float_as_uint(p.x);
  v.y = __float_as_uint(p.y);
  v.z = __float_as_uint(p.z);
  v.w = __float_as_uint(p.w);
  return v;
}

// one more pose of a candidate that is not blocked yet: word m (ro_point's fold), d its centre's D
__device__ __forceinline__ void ro_take(RoCand &c, uint32_t m, uint32_t d, float4 pose, bool has_potential) {
  if (m >= kRoBlockedWord) {
    c.flags |= RPLGPU_ROLLOUT_BLOCKED | (m == kRoRangeWord ? RPLGPU_ROLLOUT_CELL_RANGE : 0u);
    return;
  }
  ++c.n;
  c.cost_sum += m;
  c.cost_max = max(c.cost_max, m);
  if (has_potential) {
    c.d_end = d;
    c.d_min = min(c.d_min, d);
  }
  c.end_pose = ro_bits(pose);
}

struct RoBest {  // the fold of a set of candidates
  u64 score;
  uint32_t k, ties, admissible, blocked, range;
};

__device__ __forceinline__ RoBest ro_fold(const RoBest &a, const RoBest &b) {
  RoBest o;
  o.score = min(a.score, b.score);
  o.k = a.score == b.score ? min(a.k, b.k) : (a.score < b.score ? a.k : b.k);
  o.ties = (a.score == o.score ? a.ties : 0u) + (b.score == o.score ? b.ties : 0u);
  o.admissible = a.admissible + b.admissible;
  o.blocked = a.blocked + b.blocked;
  o.range = a.range + b.range;
  return o;
}

__device__ __forceinline__ RoBest ro_wave_fold(RoBest v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    RoBest o;
    o.score = __shfl_xor(v.score, d, 64);
    o.k = __shfl_xor(v.k, d, 64);
    o.ties = __shfl_xor(v.ties, d, 64);
    o.admissible = __shfl_xor(v.admissible, d, 64);
    o.blocked = __shfl_xor(v.blocked, d, 64);
    o.range = __shfl_xor(v.range, d, 64);
    v = ro_fold(v, o);
  }
  return v;
}

__device__ __forceinline__ RoBest ro_none() { return RoBest{~0ull, RPLGPU_ROLLOUT_NONE, 0u, 0u, 0u, 0u}; }

// the candidate's flags and score, its eight words and its end pose; -> its part of the fold
__device__ __forceinline__ RoBest ro_finish(const RolloutK &k, RoCand &c, bool has_potential, uint32_t kk,
                                            uint32_t *__restrict__ out_g, float *__restrict__ end_g) {
  if (has_potential && c.d_end == RPLGPU_NAV_UNREACHED) c.flags |= RPLGPU_ROLLOUT_END_UNREACHED;
  u64 score = ~0ull;
  if (c.n >= k.min_steps && !(c.flags & RPLGPU_ROLLOUT_END_UNREACHED)) {
    c.flags |= RPLGPU_ROLLOUT_ADMISSIBLE;
    score = (u64)k.a_end * c.d_end + (u64)k.a_min * c.d_min + (u64)k.a_sum * c.cost_sum + (u64)k.a_max * c.cost_max;
  }
  ro_u32x4 lo, hi;
  lo.x = c.n;
  lo.y = c.flags;
  lo.z = c.cost_sum;
  lo.w = c.cost_max;
  hi.x = c.d_end;
  hi.y = c.d_min;
  hi.z = (uint32_t)score;
  hi.w = (uint32_t)(score >> 32);
  ro_u32x4 *o = reinterpret_cast<ro_u32x4 *>(out_g) + 2u * (size_t)kk;
  o[0] = lo;
  o[1] = hi;
  if (end_g) reinterpret_cast<ro_u32x4 *>(end_g)[kk] = c.end_pose;
  const bool adm = (c.flags & RPLGPU_ROLLOUT_ADMISSIBLE) != 0u;
  return RoBest{score, adm ? kk : RPLGPU_ROLLOUT_NONE, adm ? 1u : 0u, adm ? 1u : 0u,
                (c.flags & RPLGPU_ROLLOUT_BLOCKED) ? 1u : 0u, (c.flags & RPLGPU_ROLLOUT_CELL_RANGE) ? 1u : 0u};
}

__device__ __forceinline__ void ro_store_record(uint32_t *__restrict__ rec, const RoBest &b) {
  ro_u32x4 lo, hi;
  lo.x = (uint32_t)b.score;
  lo.y = (uint32_t)(b.score >> 32);
  lo.z = b.k;
  lo.w = b.ties;
  hi.x = b.admissible;
  hi.y = b.blocked;
  hi.z = b.range;
  hi.w = 0u;
  reinterpret_cast<ro_u32x4 *>(rec)[0] = lo;  // (the scratch is 16-byte aligned, records are 32 bytes)
  reinterpret_cast<ro_u32x4 *>(rec)[1] = hi;
}

template <bool PER_STEP>
__global__ __launch_bounds__(kRoBlock) void k_rollout_tiles(
    const RolloutK k, const float *__restrict__ start, uint32_t start_per_group, const float *__restrict__ delta,
    u64 delta_stride, uint32_t delta_per_group, const float *__restrict__ footprint, uint32_t F,
    const int8_t *__restrict__ grid, u64 grid_stride, const uint32_t *__restrict__ potential, u64 potential_stride,
    uint32_t grid_per_group, uint32_t K, uint32_t *__restrict__ out, u64 out_stride, float *__restrict__ end_poses,
    u64 end_stride, uint32_t *__restrict__ scratch) {
  __shared__ float4 s_pose[kRoChunk * kRoRow];    // [step][candidate]
  __shared__ uint32_t s_m[kRoChunk * kRoTile];    // the fold of a pose's points
  __shared__ uint32_t s_d[kRoChunk * kRoTile];    // D at a pose's centre
  __shared__ float2 s_fp[RPLGPU_ROLLOUT_MAX_FOOTPRINT];
  const uint32_t tid = threadIdx.x, tile = blockIdx.x, g = blockIdx.y;
  const uint32_t k0 = tile * kRoTile;
  const uint32_t nv = min(kRoTile, K - k0);  // the tile's candidates
  const uint32_t T = k.steps;
  const size_t g_c = grid_per_group ? g : 0u;
  const int8_t *grid_g = grid + g_c * grid_stride;
  const bool has_potential = potential != nullptr;
  const uint32_t *pot_g = has_potential ? potential + g_c * potential_stride : nullptr;
  const float4 *dl = reinterpret_cast<const float4 *>(delta + (size_t)(delta_per_group ? g : 0u) * delta_stride);
  if (tid < F) s_fp[tid] = reinterpret_cast<const float2 *>(footprint)[tid];
  const bool own = tid < nv;
  const uint32_t kk = k0 + tid;
  float4 pose = make_float4(0.0f, 0.0f, 0.0f, 0.0f), dv = pose;
  if (own) {
    pose = reinterpret_cast<const float4 *>(start)[start_per_group ? g : 0u];
    if (!PER_STEP) dv = dl[kk];
  }
  RoCand c;
  c.n = c.flags = c.cost_sum = c.cost_max = 0u;
  c.d_end = c.d_min = has_potential ? RPLGPU_NAV_UNREACHED : 0u;
  c.end_pose = ro_bits(pose);  // (the start bit for bit while n = 0)
  const uint32_t n_looks = F + (has_potential ? 1u : 0u);
  for (uint32_t t0 = 0; t0 < T; t0 += kRoChunk) {  // at most 8 chunks
    const uint32_t cs = min(kRoChunk, T - t0);
    for (uint32_t i = tid; i < kRoChunk * kRoTile; i += kRoBlock) s_m[i] = 0u;
    if (PER_STEP) {
      // 32 lanes a candidate: its chunk's deltas are one run of 16 cs bytes
      const uint32_t st = tid & 31u;
      for (uint32_t cand = tid >> 5; cand < nv; cand += kRoBlock / 32u)
        if (st < cs) s_pose[st * kRoRow + cand] = dl[(size_t)(k0 + cand) * T + t0 + st];  // < K T <= the stride / 4
      __syncthreads();
    }
    // phase 1
    if (own) {
      for (uint32_t st = 0; st < cs; ++st) {
        if (PER_STEP) dv = s_pose[st * kRoRow + tid];
        pose = ro_move(pose, dv);
        s_pose[st * kRoRow + tid] = pose;
      }
    }
    __syncthreads();
    // phase 2
    for (uint32_t p = 0; p < n_looks; ++p) {
      const bool centre = p == F;
      const float2 fp = centre ? make_float2(0.0f, 0.0f) : s_fp[p];
      for (uint32_t i = tid; i < cs * kRoTile; i += kRoBlock) {
        const uint32_t cand = i & 31u, st = i >> 5;
        if (cand >= nv) continue;
        const float4 q = s_pose[st * kRoRow + cand];
        if (centre)
          s_d[i] = ro_centre(k, q, pot_g);
        else
          atomicMax(&s_m[i], ro_point(k, q, fp.x, fp.y, grid_g));
      }
    }
    __syncthreads();
    // phase 3
    if (own) {
      for (uint32_t st = 0; st < cs && !(c.flags & RPLGPU_ROLLOUT_BLOCKED); ++st)
        ro_take(c, s_m[st * kRoTile + tid], has_potential ? s_d[st * kRoTile + tid] : 0u, s_pose[st * kRoRow + tid],
                has_potential);
    }
    __syncthreads();  // (the next chunk writes all three again)
  }
  RoBest b = ro_none();
  if (own)
    b = ro_finish(k, c, has_potential, kk, out + (size_t)g * out_stride,
                  end_poses ? end_poses + (size_t)g * end_stride : nullptr);
  if (tid < 64u) {
    b = ro_wave_fold(b);
    if (tid == 0u) ro_store_record(scratch + kRoRecord * ((size_t)g * gridDim.x + tile), b);
  }
}

__global__ __launch_bounds__(kRoBlock) void k_rollout_close(uint32_t tiles, const uint32_t *__restrict__ scratch,
                                                            uint32_t *__restrict__ result) {
  __shared__ RoBest s_wave[kRoBlock / 64u];
  const uint32_t g = blockIdx.x;
  const uint32_t *recs = scratch + kRoRecord * (size_t)g * tiles;
  RoBest b = ro_none();
  for (uint32_t t = threadIdx.x; t < tiles; t += kRoBlock) {  // at most 128 rounds: tiles <= 2^20 / 32
    const ro_u32x4 lo = reinterpret_cast<const ro_u32x4 *>(recs)[2u * (size_t)t];
    const ro_u32x4 hi = reinterpret_cast<const ro_u32x4 *>(recs)[2u * (size_t)t + 1u];
    b = ro_fold(b, RoBest{(u64)lo.x | ((u64)lo.y << 32), lo.z, lo.w, hi.x, hi.y, hi.z});
  }
  b = ro_wave_fold(b);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x != 0u) return;
  for (uint32_t w = 1; w < kRoBlock / 64u; ++w) b = ro_fold(b, s_wave[w]);
  uint32_t *res = result + 8u * (size_t)g;
  res[0] = b.admissible;
  res[1] = b.k;
  res[2] = (uint32_t)b.score;
  res[3] = (uint32_t)(b.score >> 32);
  res[4] = b.ties;
  res[5] = b.blocked;
  res[6] = b.range;
  res[7] = b.admissible ? 0u : 1u;
}

}  // namespace

hipError_t launch_rollout(hipStream_t s, const RolloutK &k, const float *start, uint32_t start_per_group,
                          const float *delta, unsigned long long delta_stride, uint32_t delta_per_group,
                          uint32_t delta_per_step, const float *footprint, uint32_t F, const int8_t *grid,
                          unsigned long long grid_stride, const uint32_t *potential,
                          unsigned long long potential_stride, uint32_t grid_per_group, uint32_t G, uint32_t K,
                          uint32_t *out, unsigned long long out_stride, float *end_poses,
                          unsigned long long end_stride, uint32_t *result, uint32_t *scratch) {
  const u64 cells = (u64)k.width * k.height;
  if (G == 0 || G > 65535u || K == 0 || K > RPLGPU_MAX_POSES || k.steps == 0 || k.steps > RPLGPU_ROLLOUT_MAX_STEPS ||
      (u64)K * k.steps > (1ull << 24) || F == 0 || F > RPLGPU_ROLLOUT_MAX_FOOTPRINT || delta_per_step > 1u ||
      delta_stride < 4ull * K * (delta_per_step ? k.steps : 1u) || grid_stride < cells ||
      (potential && potential_stride < cells) || out_stride < 8ull * K || (end_poses && end_stride < 4ull * K) ||
      (reinterpret_cast<uintptr_t>(scratch) & 15u))
    return hipErrorInvalidValue;
  const uint32_t tiles = (K + kRoTile - 1u) / kRoTile;
  if ((u64)tiles * G > RPLGPU_ROLLOUT_MAX_TILES) return hipErrorInvalidValue;
  if (delta_per_step)
    hipLaunchKernelGGL(k_rollout_tiles<true>, dim3(tiles, G), dim3(kRoBlock), 0, s, k, start, start_per_group, delta,
                       delta_stride, delta_per_group, footprint, F, grid, grid_stride, potential, potential_stride,
                       grid_per_group, K, out, out_stride, end_poses, end_stride, scratch);
  else
    hipLaunchKernelGGL(k_rollout_tiles<false>, dim3(tiles, G), dim3(kRoBlock), 0, s, k, start, start_per_group, delta,
                       delta_stride, delta_per_group, footprint, F, grid, grid_stride, potential, potential_stride,
                       grid_per_group, K, out, out_stride, end_poses, end_stride, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rollout_close, dim3(G), dim3(kRoBlock), 0, s, tiles, scratch, result);
  return hipGetLastError();
}

}  // namespace rpl
