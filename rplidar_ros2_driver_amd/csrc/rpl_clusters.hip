// rpl_clusters.hip — E21: a binned pose list clustered on the device, include/rplgpu_msg.h, rplgpu_cluster_poses_dev:
// per group the occupied bins of E20's bit map are labelled by connected component (26 neighbours, the heading axis
// wrapping by flag), every pose is given its bin's label, every cluster its weight, and the heaviest cluster is reduced
// to E17's integer sums.
//
// Nine launches on the stream.  No workgroup waits on another; every loop carries a bound stated at the loop, and a loop
// that reaches it sets flag bit 5 and leaves; every index read from memory is clamped into its array.
//   k_cl_index    grid (blocks of 1024 map words, G): a word per thread, its popcount (bits at and beyond NB masked),
//                 the block's exclusive scan into wpre, the block's total into bbase.
//   k_cl_scan     grid (G): the <= 2048 block totals scanned (two per thread) into bbase; the header started, K stored.
//                 The RANK of an occupied bin b = bbase[w >> 10] + wpre[w] + popc(word & bits below b), w = b >> 5:
//                 monotone in the bin id.
//   k_cl_init     grid (blocks of 1024 bins, G), a thread per BIN (enumerated from the map, not from the poses): an
//                 occupied bin of rank r stores parent[r] = r, binid[r] = b and clears its table row.
//   k_cl_link     the same grid: an occupied bin tests its 13 FORWARD neighbours' bits (dk = +1 with any dx, dy — the
//                 wrap makes T - 1 -> 0 such a step; dk = 0 with dy = +1; dk = 0, dy = 0, dx = +1: every neighbour pair
//                 is forward for one of its two bins) and unites the ranks.  EVERY access to parent[] in this launch is
//                 a relaxed agent-scope atomic — load, min, compare-exchange — so no XCD works on a stale line.  The
//                 hook puts the larger ROOT under the smaller (a compare-exchange that only a root passes), so
//                 parent[x] <= x throughout, the trees never hold a cycle, and the final root of a component is its
//                 smallest rank = its smallest bin id whatever the timing.  A failed hook (the root was hooked by
//                 somebody else in between) goes on from the value the atomic returned: the pair only ever decreases.
//   k_cl_flatten  grid (blocks of 1024 ranks, G): root[r] = the end of r's walk, stored in an array of its own.  The
//                 walks of this launch still shorten parent[] as they pass (the atomic min of the find) while other
//                 threads walk it: every access to parent[] is again an agent-scope atomic, a pointer only moves to a
//                 smaller node of the same tree and no root changes any more, so every walk ends at the same root
//                 whatever it meets.  The roots flagged, their block-exclusive count into ordpre, block totals into
//                 rbase.
//   k_cl_weigh    grid (tiles of 1024 poses, G), a thread per pose: bin -> rank -> root -> label, the label written,
//                 the pose quantised by E17's rule; W (64-bit) and the count of the root's table row raised by integer
//                 atomics after the lanes of the wave that hit the same root were merged (eight rounds, as
//                 rpl_bins.hip; a lane still pending then adds alone) and the first root of every wave was merged
//                 once more across the workgroup's sixteen waves through LDS (a converged list sent 2 x 16 384
//                 atomics to ONE row without it, 0.20 ms of the call by a kernel trace); pord[i] = the root rank of a pose that
//                 contributes, 0xFFFFFFFF otherwise; strays, unlabelled entries and the flags added to the header.
//   k_cl_best     grid (G): rbase scanned (<= 1024 totals, one per thread) -> N_c; one sweep over the rank blocks that
//                 hold a root writes the table rows of the roots of ordinal < cap and finds BEST by (W descending,
//                 rank ascending), a second sweep finds SECOND among the others.
//   k_cl_tiles, k_cl_finish   E17's tile reduction and finish (rpl_moments.hpp's es_tile_sums and es_finish_sums, the
//                 bodies rpl_estimate.hip runs) with "pord[i] is BEST's root" in place of the gate; the finish kernel
//                 adds its own words 0 - 7 and 72 - 79.
// With K above kClMaxBins (a KEEP map ORed over several lists) k_cl_scan says so in the header and every later kernel
// does nothing but write the header's rule: labels 0xFFFFFFFF, word 0 = 32.
//
// THE SCRATCH of a group (uint32 words; every part of even length, so the 64-bit parts are 8-byte aligned), with
// words = ceil(NB / 32), NBLK = ceil(words / 1024), KC = min(NB, 2^20), RBLK = ceil(KC / 1024), TL = ceil(P / 1024):
//   hdr 16 | bbase even(NBLK) | rbase even(RBLK) | wpre even(words) | parent, root, binid, ordpre, tabN even(KC) each |
//   tabW 2 even(KC) | pord even(P) | E17's 68 TL
// rplgpu_cluster_scratch_words = G times that sum.  hdr: 0 K, 1 N_c, 2 flags (bits 1, 4, 5), 3 strays, 4 unlabelled,
// 5 BEST's root rank, 6 BEST's label, 7 SECOND's label, 8 its poses, 9, 10 its W, 11 K is above the bound.
// This unit is built with -ffp-contract=off: every float32 operation rounds once.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_moments.hpp"
#include "rpl_unionfind.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

constexpr uint32_t kClBlock = kBlock;            // map words per index block, bins per link block, poses per tile
constexpr uint32_t kClMaxBins = RPLGPU_MAX_POSES;  // occupied bins a call holds
constexpr uint32_t kClNone = 0xFFFFFFFFu;
constexpr uint32_t kClMergeRounds = 8u;
static_assert(RPLGPU_MAX_POSE_BINS / 32u / kClBlock <= 2u * kClBlock, "k_cl_scan takes two block totals per thread");
static_assert(kClMaxBins / kClBlock <= kClBlock, "k_cl_best takes one block total per thread");
static_assert(RPLGPU_CLUSTER_WORDS == RPLGPU_ESTIMATE_WORDS + 8u, "the result's layout");

enum { H_K = 0, H_NC, H_FLAGS, H_STRAY, H_UNLAB, H_BEST, H_BESTLABEL, H_SECLABEL, H_SECN, H_SECW0, H_SECW1, H_OVER,
       H_WORDS = 16 };

__host__ __device__ inline u64 cl_even(u64 v) { return (v + 1ull) & ~1ull; }

struct ClLayout {
  u64 bbase, rbase, wpre, parent, root, binid, ordpre, tabn, tabw, pord, est, total;
  uint32_t kc;
};
__host__ __device__ inline ClLayout cl_layout(uint32_t nb, uint32_t P) {
  ClLayout l;
  const uint32_t words = bin_map_words(nb);
  l.kc = nb < kClMaxBins ? nb : kClMaxBins;
  const u64 kc = cl_even(l.kc);
  l.bbase = H_WORDS;
  l.rbase = l.bbase + cl_even((words + kClBlock - 1u) / kClBlock);
  l.wpre = l.rbase + cl_even((l.kc + kClBlock - 1u) / kClBlock);
  l.parent = l.wpre + cl_even(words);
  l.root = l.parent + kc;
  l.binid = l.root + kc;
  l.ordpre = l.binid + kc;
  l.tabn = l.ordpre + kc;
  l.tabw = l.tabn + kc;
  l.pord = l.tabw + 2ull * kc;
  l.est = l.pord + cl_even(P);
  l.total = l.est + es_group_words(es_tiles(P));
  return l;
}

struct ClArgs {
  uint32_t nx, ny, T, nb, wrap, P;
  const uint32_t *map;
  u64 map_stride;
  uint32_t *scratch;
};

// word w of a group's map with the bits at and beyond NB masked
__device__ __forceinline__ uint32_t cl_word(const uint32_t *map, uint32_t w, uint32_t nb) {
  const uint32_t v = map[w];
  const uint32_t tail = nb & 31u;
  return (w == (nb >> 5) && tail) ? v & ((1u << tail) - 1u) : v;
}

// the rank of bin b (its bit need not be set: then the rank of the next occupied bin), clamped below kc
__device__ __forceinline__ uint32_t cl_rank(const uint32_t *map, const uint32_t *grp, const ClLayout &l, uint32_t b,
                                            uint32_t nb) {
  const uint32_t w = b >> 5;
  const uint32_t below = cl_word(map, w, nb) & ((1u << (b & 31u)) - 1u);
  const uint32_t r = grp[l.bbase + (w >> 10)] + grp[l.wpre + w] + (uint32_t)__popc(below);
  return min(r, l.kc - 1u);
}

__global__ __launch_bounds__(kBlock) void k_cl_index(ClArgs a) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  const uint32_t g = blockIdx.y;
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  const uint32_t *map = a.map + (size_t)g * a.map_stride;
  const uint32_t words = bin_map_words(a.nb);
  const uint32_t w = blockIdx.x * kClBlock + threadIdx.x;
  const uint32_t pc = w < words ? (uint32_t)__popc(cl_word(map, w, a.nb)) : 0u;
  uint32_t total;
  const uint32_t pre = block_excl_scan(pc, s_tmp, &total);
  if (w < words) grp[l.wpre + w] = pre;
  if (threadIdx.x == 0) grp[l.bbase + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_cl_scan(ClArgs a) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  const uint32_t g = blockIdx.x;
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  const uint32_t nblk = (bin_map_words(a.nb) + kClBlock - 1u) / kClBlock;  // <= 2048
  const uint32_t i0 = 2u * threadIdx.x, i1 = i0 + 1u;
  const uint32_t v0 = i0 < nblk ? grp[l.bbase + i0] : 0u, v1 = i1 < nblk ? grp[l.bbase + i1] : 0u;
  uint32_t K;
  const uint32_t pre = block_excl_scan(v0 + v1, s_tmp, &K);
  if (i0 < nblk) grp[l.bbase + i0] = pre;
  if (i1 < nblk) grp[l.bbase + i1] = pre + v0;
  if (threadIdx.x < (uint32_t)H_WORDS) {
    const uint32_t t = threadIdx.x;
    const uint32_t over = K > l.kc ? 1u : 0u;
    grp[t] = t == H_K ? K : t == H_OVER ? over : (t == H_BEST || t == H_BESTLABEL || t == H_SECLABEL) ? kClNone : 0u;
  }
}

__global__ __launch_bounds__(kBlock) void k_cl_init(ClArgs a) {
  const uint32_t g = blockIdx.y;
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  if (grp[H_OVER]) return;
  const uint32_t *map = a.map + (size_t)g * a.map_stride;
  const uint32_t b = blockIdx.x * kClBlock + threadIdx.x;
  if (b >= a.nb || !((cl_word(map, b >> 5, a.nb) >> (b & 31u)) & 1u)) return;
  const uint32_t r = cl_rank(map, grp, l, b, a.nb);
  grp[l.parent + r] = r;
  grp[l.binid + r] = b;
  grp[l.tabn + r] = 0u;
  reinterpret_cast<u64 *>(grp + l.tabw)[r] = 0ull;
}

// the union-find over the ranks (rpl_unionfind.hpp): values clamped below kc, walks bounded by K, bit 5 at the bound
__device__ __forceinline__ UfGlobal cl_uf(uint32_t K, uint32_t kc, uint32_t *hdr) {
  return UfGlobal{kc, K, hdr + H_FLAGS, 32u};
}

__global__ __launch_bounds__(kBlock) void k_cl_link(ClArgs a) {
  const uint32_t g = blockIdx.y;
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  if (grp[H_OVER]) return;
  const uint32_t *map = a.map + (size_t)g * a.map_stride;
  const uint32_t b = blockIdx.x * kClBlock + threadIdx.x;
  if (b >= a.nb || !((cl_word(map, b >> 5, a.nb) >> (b & 31u)) & 1u)) return;
  const uint32_t K = min(grp[H_K], l.kc);
  const uint32_t r = cl_rank(map, grp, l, b, a.nb);
  const uint32_t bx = b % a.nx, rest = b / a.nx, by = rest % a.ny, kt = rest / a.ny;
  uint32_t *parent = grp + l.parent;
#pragma unroll 1
  for (uint32_t n = 0; n < 13u; ++n) {  // the 13 forward neighbours: n = 0 .. 8 dk = 1; 9 .. 11 dy = 1; 12 dx = 1
    const int dk = n < 9u ? 1 : 0;
    const int dy = n < 9u ? (int)(n / 3u) - 1 : n < 12u ? 1 : 0;
    const int dx = n < 9u ? (int)(n % 3u) - 1 : n < 12u ? (int)n - 10 : 1;
    const int x = (int)bx + dx, y = (int)by + dy;
    if (x < 0 || x >= (int)a.nx || y < 0 || y >= (int)a.ny) continue;
    uint32_t k = kt + (uint32_t)dk;
    if (k == a.T) {
      if (!a.wrap) continue;
      k = 0u;
    }
    const uint32_t q = (k * a.ny + (uint32_t)y) * a.nx + (uint32_t)x;  // below NB
    if (q == b || !((cl_word(map, q >> 5, a.nb) >> (q & 31u)) & 1u)) continue;
    uf_unite(parent, r, cl_rank(map, grp, l, q, a.nb), cl_uf(K, l.kc, grp));
  }
}

__global__ __launch_bounds__(kBlock) void k_cl_flatten(ClArgs a) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  const uint32_t g = blockIdx.y;
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  if (grp[H_OVER]) return;  // (block-uniform)
  const uint32_t K = min(grp[H_K], l.kc);
  if (blockIdx.x * kClBlock >= K) return;  // (block-uniform)
  const uint32_t r = blockIdx.x * kClBlock + threadIdx.x;
  uint32_t is_root = 0u;
  if (r < K) {
    const uint32_t root = uf_find(grp + l.parent, r, cl_uf(K, l.kc, grp));
    grp[l.root + r] = root;
    is_root = root == r ? 1u : 0u;
  }
  uint32_t total;
  const uint32_t pre = block_excl_scan(is_root, s_tmp, &total);
  if (r < K) grp[l.ordpre + r] = pre;
  if (threadIdx.x == 0) grp[l.rbase + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_cl_weigh(ClArgs a, const float *__restrict__ poses, u64 pose_stride,
                                                     uint32_t poses_per_group, const uint32_t *__restrict__ weights,
                                                     u64 weight_stride, float xy_scale,
                                                     const uint32_t *__restrict__ bins, u64 bin_stride,
                                                     uint32_t *__restrict__ labels, u64 label_stride) {
  __shared__ uint32_t s_part[kWaves];
  __shared__ uint32_t s_root[kWaves], s_n[kWaves];
  __shared__ u64 s_w[kWaves];
  const uint32_t g = blockIdx.y;
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  const uint32_t *map = a.map + (size_t)g * a.map_stride;
  const uint32_t i = blockIdx.x * kClBlock + threadIdx.x;
  const bool live = i < a.P;
  const bool over = grp[H_OVER] != 0u;
  const uint32_t K = min(grp[H_K], l.kc);
  const uint32_t b = live ? bins[(size_t)g * bin_stride + i] : kClNone;
  const bool unlab = live && b == kClNone;
  bool labelled = false;
  if (live && !unlab && !over && b < a.nb) labelled = ((cl_word(map, b >> 5, a.nb) >> (b & 31u)) & 1u) != 0u;
  const bool stray = live && !unlab && !over && !labelled;
  uint32_t root = 0u, label = kClNone;
  if (labelled) {  // (K >= 1 here)
    const uint32_t r = min(cl_rank(map, grp, l, b, a.nb), K - 1u);
    root = min(grp[l.root + r], K - 1u);
    label = grp[l.binid + root];
  }
  if (live && labels) labels[(size_t)g * label_stride + i] = label;  // i < P <= label_stride
  const es_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const es_f32x4 v =
      labelled ? reinterpret_cast<const es_f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride)[i] : zero;
  const bool in = labelled && es_quantise(v, xy_scale).in;
  const uint32_t w = in ? (weights ? weights[(size_t)g * weight_stride + i] : 1u) : 0u;
  if (live) grp[l.pord + i] = in ? root : kClNone;
  // the lanes of the wave that hit the same root hand their weight and count to the first of them; what the FIRST
  // round gathers (the root of the wave's first contributing lane: on a converged list every lane's) is not added by
  // the wave but handed to the workgroup through LDS, where the waves that hold the same root are merged once more
  u64 pending = __ballot(in);
  u64 my_w = 0ull, wave_w = 0ull;
  uint32_t my_n = 0u, wave_n = 0u, wave_root = kClNone;  // (wave_*: the same in every lane)
  for (uint32_t round = 0; round < kClMergeRounds && pending; ++round) {
    const int first = __ffsll((i64)pending) - 1;
    const uint32_t fr = (uint32_t)__builtin_amdgcn_readlane((int)root, first);
    const bool same = in && root == fr;
    u64 sw = same ? (u64)w : 0ull;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sw += __shfl_xor(sw, d, 64);  // at most 64 * 2^32
    const u64 who = __ballot(same);
    if (round == 0u) {
      wave_root = fr;
      wave_w = sw;
      wave_n = (uint32_t)__popcll(who);
    } else if ((int)lane_id() == first) {
      my_w = sw;
      my_n = (uint32_t)__popcll(who);
    }
    pending &= ~who;
  }
  if ((pending >> lane_id()) & 1ull) {  // past the bound a lane adds alone
    my_w = w;
    my_n = 1u;
  }
  if (my_n) {
    atomicAdd(reinterpret_cast<u64 *>(grp + l.tabw) + root, my_w);
    atomicAdd(grp + l.tabn + root, my_n);
  }
  if (lane_id() == 0u) {
    s_root[wave_id()] = wave_root;
    s_w[wave_id()] = wave_w;
    s_n[wave_id()] = wave_n;
  }
  // the tile's counts; at most 64 each in a wave: one byte each
  const bool outr = labelled && !in;
  const uint32_t cnt = wave_incl_scan_fast((stray ? 1u : 0u) | (unlab ? 1u << 8 : 0u) | (outr ? 1u << 16 : 0u));
  if (lane_id() == 63u) s_part[wave_id()] = cnt;
  __syncthreads();
  if (threadIdx.x < (uint32_t)kWaves && s_root[threadIdx.x] != kClNone) {
    // wave q's first root: the first wave of the workgroup that holds it adds for all of them (at most 64 * 16 poses)
    const uint32_t q = threadIdx.x, r = min(s_root[q], l.kc - 1u);
    bool mine = true;
    for (uint32_t p = 0; p < q; ++p) mine = mine && s_root[p] != s_root[q];
    if (mine) {
      u64 sum_w = 0ull;
      uint32_t sum_n = 0u;
      for (uint32_t p = q; p < (uint32_t)kWaves; ++p) {
        if (s_root[p] == s_root[q]) {
          sum_w += s_w[p];
          sum_n += s_n[p];
        }
      }
      atomicAdd(reinterpret_cast<u64 *>(grp + l.tabw) + r, sum_w);
      atomicAdd(grp + l.tabn + r, sum_n);
    }
  }
  if (threadIdx.x == 0) {
    uint32_t n_stray = 0u, n_unlab = 0u, n_out = 0u;
    for (int q = 0; q < kWaves; ++q) {
      n_stray += s_part[q] & 0xFFu;
      n_unlab += (s_part[q] >> 8) & 0xFFu;
      n_out += (s_part[q] >> 16) & 0xFFu;
    }
    if (n_stray) atomicAdd(grp + H_STRAY, n_stray);
    if (n_unlab) atomicAdd(grp + H_UNLAB, n_unlab);
    const uint32_t f = (n_out ? 2u : 0u) | (n_stray ? 16u : 0u);
    if (f) atomicOr(grp + H_FLAGS, f);
  }
}

// (W descending, rank ascending); kClNone is no candidate
__device__ __forceinline__ bool cl_better(u64 w1, uint32_t r1, u64 w2, uint32_t r2) {
  if (r1 == kClNone) return false;
  if (r2 == kClNone) return true;
  return w1 > w2 || (w1 == w2 && r1 < r2);
}

// the best (W, rank) over the block; every thread gets it
__device__ __forceinline__ void cl_block_best(u64 *w, uint32_t *r, u64 *s_w, uint32_t *s_r) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const u64 ow = __shfl_xor(*w, d, 64);
    const uint32_t orank = __shfl_xor(*r, d, 64);
    if (cl_better(ow, orank, *w, *r)) {
      *w = ow;
      *r = orank;
    }
  }
  __syncthreads();  // (the arrays' earlier readers are done)
  if (lane_id() == 0u) {
    s_w[wave_id()] = *w;
    s_r[wave_id()] = *r;
  }
  __syncthreads();
  u64 bw = s_w[0];
  uint32_t br = s_r[0];
  for (int q = 1; q < kWaves; ++q) {
    if (cl_better(s_w[q], s_r[q], bw, br)) {
      bw = s_w[q];
      br = s_r[q];
    }
  }
  *w = bw;
  *r = br;
}

__global__ __launch_bounds__(kBlock) void k_cl_best(ClArgs a, uint32_t *__restrict__ clusters, u64 cluster_stride,
                                                    uint32_t cap) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  __shared__ uint32_t s_base[kClBlock], s_cnt[kClBlock];
  __shared__ u64 s_w[kWaves];
  __shared__ uint32_t s_r[kWaves];
  const uint32_t g = blockIdx.x;
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  if (grp[H_OVER]) return;  // (block-uniform)
  const uint32_t K = min(grp[H_K], l.kc);
  const uint32_t nblk = (K + kClBlock - 1u) / kClBlock;  // <= 1024
  uint32_t nc;
  const uint32_t roots_here = threadIdx.x < nblk ? grp[l.rbase + threadIdx.x] : 0u;  // of rank block threadIdx.x
  s_cnt[threadIdx.x] = roots_here;
  s_base[threadIdx.x] = block_excl_scan(roots_here, s_tmp, &nc);
  __syncthreads();
  const u64 *tabw = reinterpret_cast<const u64 *>(grp + l.tabw);
  u64 bw = 0ull;
  uint32_t br = kClNone;
  // a rank block without a root is passed over (a spread list: one component, 556 blocks, one root)
  for (uint32_t blk = 0; blk < nblk; ++blk) {  // at most 1024 rounds: K <= 2^20
    const uint32_t r = blk * kClBlock + threadIdx.x;
    if (s_cnt[blk] == 0u || r >= K || grp[l.root + r] != r) continue;
    const u64 w = tabw[r];
    if (cl_better(w, r, bw, br)) {
      bw = w;
      br = r;
    }
    const uint32_t ord = s_base[r >> 10] + grp[l.ordpre + r];
    if (clusters && ord < cap) {
      uint32_t *row = clusters + (size_t)g * cluster_stride + 4u * (size_t)ord;  // ord < cap, 4 cap <= cluster_stride
      row[0] = grp[l.binid + r];
      row[1] = grp[l.tabn + r];
      row[2] = (uint32_t)w;
      row[3] = (uint32_t)(w >> 32);
    }
  }
  cl_block_best(&bw, &br, s_w, s_r);
  u64 sw = 0ull;
  uint32_t sr = kClNone;
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    const uint32_t r = blk * kClBlock + threadIdx.x;
    if (s_cnt[blk] == 0u || r >= K || grp[l.root + r] != r || r == br) continue;
    const u64 w = tabw[r];
    if (cl_better(w, r, sw, sr)) {
      sw = w;
      sr = r;
    }
  }
  cl_block_best(&sw, &sr, s_w, s_r);
  if (threadIdx.x == 0) {
    grp[H_NC] = nc;
    grp[H_BEST] = br;
    grp[H_BESTLABEL] = br != kClNone ? grp[l.binid + br] : kClNone;
    grp[H_SECLABEL] = sr != kClNone ? grp[l.binid + sr] : kClNone;
    grp[H_SECN] = sr != kClNone ? grp[l.tabn + sr] : 0u;
    grp[H_SECW0] = (uint32_t)sw;
    grp[H_SECW1] = (uint32_t)(sw >> 32);
  }
}

// ---- E17's tile reduction and finish (rpl_moments.hpp) ----------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_cl_tiles(ClArgs a, const float *__restrict__ poses, u64 pose_stride,
                                                     uint32_t poses_per_group, const uint32_t *__restrict__ weights,
                                                     u64 weight_stride, float xy_scale) {
  const uint32_t tile = blockIdx.x, g = blockIdx.y;
  const uint32_t TL = es_tiles(a.P);
  const ClLayout l = cl_layout(a.nb, a.P);
  uint32_t *grp = a.scratch + (size_t)g * l.total;
  const uint32_t best = grp[H_BEST];
  const uint32_t i = tile * kClBlock + threadIdx.x;
  const bool live = i < a.P;
  const uint32_t ord = live ? grp[l.pord + i] : kClNone;
  const bool in0 = ord != kClNone;  // labelled and in range (k_cl_weigh)
  const bool in1 = in0 && ord == best;
  const es_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const es_f32x4 v =
      in0 ? reinterpret_cast<const es_f32x4 *>(poses + (size_t)(poses_per_group ? g : 0u) * pose_stride)[i] : zero;
  const EsPose q = es_quantise(v, xy_scale);
  const uint32_t w = in0 ? (weights ? weights[(size_t)g * weight_stride + i] : 1u) : 0u;
  es_tile_sums(q, w, in0, in1, tile, TL, grp + l.est);
}

__global__ __launch_bounds__(kBlock) void k_cl_finish(ClArgs a, uint32_t *__restrict__ result) {
  __shared__ uint32_t s_cnt[4];
  __shared__ uint32_t s_empty[2];
  const uint32_t g = blockIdx.x;
  const ClLayout l = cl_layout(a.nb, a.P);
  const uint32_t *grp = a.scratch + (size_t)g * l.total;
  uint32_t *res = result + (size_t)RPLGPU_CLUSTER_WORDS * g;
  es_finish_sums(grp + l.est, es_tiles(a.P), res, s_cnt, s_empty);
  if (threadIdx.x == 0) {
    const bool over = grp[H_OVER] != 0u;
    const uint32_t nc = grp[H_NC];
    res[0] = over ? 32u
                  : (nc == 0u ? 1u : 0u) | (grp[H_FLAGS] & 50u) | (s_empty[0] ? 4u : 0u) | (s_empty[1] ? 8u : 0u);
    res[1] = over ? kClNone : grp[H_BESTLABEL];
    res[2] = s_cnt[0];
    res[3] = s_cnt[1];
    res[4] = s_cnt[2];
    res[5] = s_cnt[3];
    res[6] = over ? 0u : nc;
    res[7] = grp[H_K];
    res[72] = over ? kClNone : grp[H_SECLABEL];
    res[73] = over ? 0u : grp[H_SECN];
    res[74] = over ? 0u : grp[H_SECW0];
    res[75] = over ? 0u : grp[H_SECW1];
    res[76] = over ? 0u : grp[H_STRAY];
    res[77] = over ? 0u : grp[H_UNLAB];
    res[78] = 0u;
    res[79] = 0u;
  }
}

bool cl_refused(uint32_t G, uint32_t P, uint32_t nx, uint32_t ny, uint32_t T) {
  return G == 0 || G > 65535u || P == 0 || P > RPLGPU_MAX_POSES || T == 0 || T > RPLGPU_MAX_HEADING_BINS || nx == 0 ||
         nx > 65536u || ny == 0 || ny > 65536u || (u64)nx * ny * T > (u64)RPLGPU_MAX_POSE_BINS;
}

}  // namespace

unsigned long long clusters_scratch_words(uint32_t G, uint32_t P, uint32_t nx, uint32_t ny, uint32_t T) {
  if (cl_refused(G, P, nx, ny, T)) return 0ull;
  return (u64)G * cl_layout(nx * ny * T, P).total;
}

hipError_t launch_clusters(hipStream_t s, const ClustersK &k, const float *poses, unsigned long long pose_stride,
                           uint32_t poses_per_group, const uint32_t *weights, unsigned long long weight_stride,
                           uint32_t G, uint32_t P, uint32_t T, const uint32_t *map, unsigned long long map_stride,
                           const uint32_t *bins, unsigned long long bin_stride, uint32_t *labels,
                           unsigned long long label_stride, uint32_t *clusters, unsigned long long cluster_stride,
                           uint32_t cluster_cap, uint32_t *result, uint32_t *scratch) {
  if (cl_refused(G, P, k.nx, k.ny, T)) return hipErrorInvalidValue;
  const uint32_t nb = k.nx * k.ny * T, words = bin_map_words(nb);
  if (pose_stride < 4ull * P || (pose_stride & 3u) || (weights && weight_stride < P) || map_stride < words ||
      bin_stride < P || (labels && label_stride < P) || (clusters && cluster_stride < 4ull * cluster_cap))
    return hipErrorInvalidValue;
  const ClLayout l = cl_layout(nb, P);
  const ClArgs a{k.nx, k.ny, T, nb, k.wrap, P, map, map_stride, scratch};
  const uint32_t word_blocks = (words + kClBlock - 1u) / kClBlock, bin_blocks = (nb + kClBlock - 1u) / kClBlock;
  const uint32_t rank_blocks = (l.kc + kClBlock - 1u) / kClBlock, tiles = es_tiles(P);
  hipError_t e;
#define RPL_CL_LAUNCH(kernel, grid, ...)                                        \
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, __VA_ARGS__);            \
  if ((e = hipGetLastError()) != hipSuccess) return e
  RPL_CL_LAUNCH(k_cl_index, dim3(word_blocks, G), a);
  RPL_CL_LAUNCH(k_cl_scan, dim3(G), a);
  RPL_CL_LAUNCH(k_cl_init, dim3(bin_blocks, G), a);
  RPL_CL_LAUNCH(k_cl_link, dim3(bin_blocks, G), a);
  RPL_CL_LAUNCH(k_cl_flatten, dim3(rank_blocks, G), a);
  RPL_CL_LAUNCH(k_cl_weigh, dim3(tiles, G), a, poses, pose_stride, poses_per_group, weights, weight_stride, k.xy_scale,
                bins, bin_stride, labels, label_stride);
  RPL_CL_LAUNCH(k_cl_best, dim3(G), a, clusters, cluster_stride, cluster_cap);
  RPL_CL_LAUNCH(k_cl_tiles, dim3(tiles, G), a, poses, pose_stride, poses_per_group, weights, weight_stride, k.xy_scale);
  RPL_CL_LAUNCH(k_cl_finish, dim3(G), a, result);
#undef RPL_CL_LAUNCH
  return hipSuccess;
}

}  // namespace rpl
