// rpl_frontier.hip — E29 (include/rplgpu_msg.h, rplgpu_frontiers_dev): a map's frontier cells found, grouped into
// 8-connected components and the next goal picked, on the device.  Integers only; the result depends on no order of
// execution.  Seven launches on one stream, nothing on the handle, no workgroup ever waits for another:
//   k_fr_init     grid (blocks of 1024 table rows, G): the header cleared, every table row emptied.
//   k_fr_tile     grid (tiles x G), 256 threads, a workgroup per 64 x 64 tile (E12's and E26's tiling): the tile's
//                 66 x 66 window of bytes classified into LDS, the frontier mask (64 rows of 64 bits) built from it
//                 (D is read at the cell itself only, so it is not staged).  A tile with no frontier bit writes its
//                 empty labels and leaves.  Otherwise the tile's own components are labelled IN LDS: the runs of
//                 every row come out of the mask with ffs / clz, a run is named by its first cell, and the runs of
//                 adjacent rows that touch (8-adjacency: the run widened by one bit each way) are united in an LDS
//                 union-find of E21's discipline (the larger root hooked under the smaller by compare-exchange).
//                 Every frontier cell then gets the GLOBAL cell index of its tile-local root into the parent plane,
//                 every other cell 0xFFFFFFFF.  A local root is the tile's smallest cell of the component, so
//                 parent[c] <= c from the start.
//   k_fr_seam     grid (tiles x G), 128 threads: the cells of a tile's last column test NE, E and SE, those of its
//                 last row SW, S and SE — every 8-adjacent pair that lies in two tiles is met from one of its cells,
//                 the pairs (63, 63)-(64, 64) and (64, 63)-(63, 64) of a four-tile corner included — and unite through
//                 the parent plane.  EVERY access to the parent plane in this launch and the next is a relaxed
//                 agent-scope atomic — load, min, compare-exchange — so no XCD works on a stale line.  The hook puts
//                 the larger ROOT under the smaller, so parent[x] <= x throughout, the trees never hold a cycle and
//                 the final root of a component is its smallest cell index whatever the timing.
//   k_fr_flatten  grid (blocks of 1024 cells, G): every frontier cell walks to its root and hangs itself under it
//                 (an atomic min: a pointer only moves to a smaller node of the same tree, and no root changes any
//                 more); the label written to d_labels_out; the roots flagged, their block-exclusive count into ord,
//                 the block totals into rbase.
//   k_fr_rank     grid (G): rbase scanned (<= 16 totals per thread) -> N; N above comp_cap sets the bound.
//   k_fr_sums     grid (tiles x G), 256 threads: the cells of a tile folded per root in an LDS table (1024 slots, eight
//                 probes; a cell that finds no slot sends alone), then one set of integer atomics per (tile, root)
//                 into the root's table row: n, sum cx, sum cy (64-bit adds) and the least key (a 64-bit min).
//   k_fr_close    grid (G), 1024 threads: the rows in rank (= label) order, min_size applied by a scan over blocks of
//                 1024 ranks, BEST by (cost, label), the result words and the goal.
// Every loop carries its bound; every index read from memory is clamped into its array; every store is a vector
// store or plain C++.  This unit is built with -ffp-contract=off, although there is no float in it.
#include <hip/hip_runtime.h>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_frontier.hpp"
#include "rpl_unionfind.hpp"
#include "rplgpu_msg.h"

namespace rpl {
namespace {

typedef unsigned long long fu64;

constexpr uint32_t kFrTile = RPLGPU_NAV_TILE;
constexpr uint32_t kFrWin = kFrTile + 2u;
constexpr uint32_t kFrTileCells = kFrTile * kFrTile;
constexpr uint32_t kFrTileBlock = 256u;
constexpr uint32_t kFrSeamBlock = 2u * kFrTile;
constexpr uint32_t kFrNone = RPLGPU_FRONTIER_NO_LABEL;
constexpr uint32_t kFrSlots = 1024u;
constexpr uint32_t kFrProbes = 8u;
static_assert(kFrTile == 64u, "a mask row is one 64-bit word");
static_assert(kFrRankBlock == (uint32_t)kBlock, "k_fr_flatten counts the roots of one workgroup's cells");
static_assert((uint64_t)RPLGPU_MAX_OCC_DIM * RPLGPU_MAX_OCC_DIM / kFrRankBlock <= 16u * kBlock,
              "k_fr_rank takes sixteen block totals per thread");
static_assert(RPLGPU_FRONTIER_MAX_COMPS / kBlock <= 1024u, "k_fr_close's stated bound");

enum { FH_F = 0, FH_N, FH_FLAGS, FH_OVER };

struct FrArgs {
  uint32_t width, height, lethal, comp_cap;
  FrLayout l;
  const int8_t *grid;
  fu64 grid_stride;
  const uint32_t *pot;
  fu64 pot_stride;
  uint32_t *scratch;
};

struct FrTileAt {
  uint32_t g, x0, y0;
};
__device__ __forceinline__ FrTileAt fr_tile_at(const FrArgs &a) {
  const uint32_t tiles = a.l.tiles_x * a.l.tiles_y;
  const uint32_t g = blockIdx.x / tiles, t = blockIdx.x % tiles;
  return FrTileAt{g, (t % a.l.tiles_x) * kFrTile, (t / a.l.tiles_x) * kFrTile};
}

// the two union-finds (rpl_unionfind.hpp).  The tile's own, in LDS: nodes are the tile's cells (the first cell of a
// run stands for the run).  Across tiles, on the parent plane: nodes are the grid's cells, as E21's are its ranks.
__device__ __forceinline__ UfLds fr_uf_lds(uint32_t *loop) { return UfLds{kFrTileCells, kFrTileCells, loop}; }
__device__ __forceinline__ UfGlobal fr_uf(uint32_t cells, uint32_t *hdr) {
  return UfGlobal{cells, cells, hdr + FH_FLAGS, RPLGPU_FRONTIER_LOOP};
}

// the bits [from, from + len) of a 64-bit word, len in 1 .. 64
__device__ __forceinline__ fu64 fr_bits(uint32_t from, uint32_t len) {
  return (len >= 64u ? ~0ull : ((1ull << len) - 1ull)) << from;
}
// the length of the run of set bits of m that begins at bit s (set)
__device__ __forceinline__ uint32_t fr_run_len(fu64 m, uint32_t s) {
  const fu64 rest = ~(m >> s);
  return rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
}
// the first bit of the run of m that holds bit q (set)
__device__ __forceinline__ uint32_t fr_run_start(fu64 m, uint32_t q) {
  const fu64 clear_below = ~m & ((1ull << q) - 1ull);
  return clear_below ? 64u - (uint32_t)__builtin_clzll(clear_below) : 0u;
}

__global__ __launch_bounds__(kBlock) void k_fr_init(FrArgs a) {
  const uint32_t g = blockIdx.y;
  uint32_t *grp = a.scratch + (size_t)g * a.l.total;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < kFrHdrWords) grp[i] = 0u;
  if (i >= a.comp_cap) return;
  uint32_t *row = grp + a.l.table + 8ull * i;
  reinterpret_cast<uint4 *>(row)[0] = make_uint4(0u, kFrNone, 0u, 0u);
  reinterpret_cast<uint4 *>(row)[1] = make_uint4(0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu);
}

__global__ __launch_bounds__(kFrTileBlock) void k_fr_tile(FrArgs a) {
  __shared__ uint8_t s_cls[kFrWin * kFrWin];  // 0 neither, 1 FREE, 2 UNKNOWN; outside the grid 0
  __shared__ uint32_t s_mask[2u * kFrTile];   // row r: the words 2 r (bits 0 - 31) and 2 r + 1
  __shared__ uint32_t s_par[kFrTileCells];
  __shared__ uint32_t s_count;
  const FrTileAt at = fr_tile_at(a);
  const int8_t *grid = a.grid + (size_t)at.g * a.grid_stride;
  const uint32_t *pot = a.pot ? a.pot + (size_t)at.g * a.pot_stride : nullptr;
  uint32_t *grp = a.scratch + (size_t)at.g * a.l.total;
  uint32_t *parent = grp + a.l.parent;
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < kFrWin * kFrWin; i += kFrTileBlock) {  // bound: 18 rounds
    const int x = (int)at.x0 + (int)(i % kFrWin) - 1, y = (int)at.y0 + (int)(i / kFrWin) - 1;
    uint32_t cls = 0u;
    if (x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height) {
      const int v = grid[(size_t)y * a.width + (size_t)x];
      cls = v < 0 ? 2u : (uint32_t)v < a.lethal ? 1u : 0u;
    }
    s_cls[i] = (uint8_t)cls;
  }
  if (tid < 2u * kFrTile) s_mask[tid] = 0u;
  if (tid == 0) s_count = 0u;
  __syncthreads();
  // the frontier bits: a thread takes a quarter of a row
  const uint32_t row = tid >> 2, quarter = tid & 3u;
  uint32_t bits = 0u;
  for (uint32_t j = 0; j < 16u; ++j) {
    const uint32_t lx = quarter * 16u + j, wi = (row + 1u) * kFrWin + lx + 1u;
    if (s_cls[wi] != 1u) continue;  // (FREE: the cell is inside the grid)
    if (s_cls[wi - 1u] != 2u && s_cls[wi + 1u] != 2u && s_cls[wi - kFrWin] != 2u && s_cls[wi + kFrWin] != 2u) continue;
    const uint32_t d = pot ? pot[(size_t)(at.y0 + row) * a.width + (at.x0 + lx)] : 0u;
    if (d != RPLGPU_NAV_UNREACHED) bits |= 1u << j;
  }
  if (bits) {
    atomicOr(&s_mask[2u * row + (quarter >> 1)], bits << ((quarter & 1u) * 16u));
    atomicAdd(&s_count, (uint32_t)__popc(bits));
  }
  for (uint32_t i = tid; i < kFrTileCells; i += kFrTileBlock) s_par[i] = i;  // bound: 16 rounds
  __syncthreads();
  const uint32_t count = s_count;
  if (count == 0u) {  // (block-uniform) the empty labels
    for (uint32_t i = tid; i < kFrTileCells; i += kFrTileBlock) {  // bound: 16 rounds
      const uint32_t x = at.x0 + (i & 63u), y = at.y0 + (i >> 6);
      if (x < a.width && y < a.height) parent[(size_t)y * a.width + x] = kFrNone;
    }
    return;
  }
  // the runs that begin in this thread's quarter, united with the runs of the next row they touch
  uint32_t loop = 0u;
  const fu64 m = (fu64)s_mask[2u * row] | ((fu64)s_mask[2u * row + 1u] << 32);
  const fu64 below = row + 1u < kFrTile ? (fu64)s_mask[2u * row + 2u] | ((fu64)s_mask[2u * row + 3u] << 32) : 0ull;
  fu64 starts = m & ~(m << 1) & fr_bits(quarter * 16u, 16u);
  for (uint32_t i = 0; starts && below && i < 8u; ++i) {  // bound: 8 runs begin in 16 bits
    const uint32_t s = (uint32_t)__builtin_ctzll(starts);
    starts &= starts - 1ull;
    const fu64 run = fr_bits(s, fr_run_len(m, s));
    fu64 touch = below & (run | (run << 1) | (run >> 1));
    for (uint32_t k = 0; touch && k < 33u; ++k) {  // bound: 33 runs of a row touch one run
      const uint32_t q = (uint32_t)__builtin_ctzll(touch);
      const uint32_t s2 = fr_run_start(below, q), end2 = q + fr_run_len(below, q);
      uf_unite(s_par, row * kFrTile + s, (row + 1u) * kFrTile + s2, fr_uf_lds(&loop));
      touch = end2 >= 64u ? 0ull : touch & ~((1ull << end2) - 1ull);
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < kFrTileCells; i += kFrTileBlock) {  // bound: 16 rounds
    const uint32_t lx = i & 63u, ly = i >> 6, x = at.x0 + lx, y = at.y0 + ly;
    if (x >= a.width || y >= a.height) continue;
    const fu64 mr = (fu64)s_mask[2u * ly] | ((fu64)s_mask[2u * ly + 1u] << 32);
    uint32_t label = kFrNone;
    if ((mr >> lx) & 1ull) {
      const uint32_t root = uf_find(s_par, ly * kFrTile + fr_run_start(mr, lx), fr_uf_lds(&loop));
      label = (at.y0 + (root >> 6)) * a.width + at.x0 + (root & 63u);  // a frontier cell: inside the grid
    }
    parent[(size_t)y * a.width + x] = label;
  }
  if (tid == 0) atomicAdd(grp + FH_F, count);
  if (loop) atomicOr(grp + FH_FLAGS, RPLGPU_FRONTIER_LOOP);
}

__global__ __launch_bounds__(kFrSeamBlock) void k_fr_seam(FrArgs a) {
  const FrTileAt at = fr_tile_at(a);
  uint32_t *grp = a.scratch + (size_t)at.g * a.l.total;
  uint32_t *parent = grp + a.l.parent;
  const uint32_t cells = (uint32_t)a.l.cells;
  const bool column = threadIdx.x < kFrTile;
  const uint32_t x = column ? at.x0 + kFrTile - 1u : at.x0 + threadIdx.x - kFrTile;
  const uint32_t y = column ? at.y0 + threadIdx.x : at.y0 + kFrTile - 1u;
  if (x >= a.width || y >= a.height) return;
  const uint32_t c = y * a.width + x;
  if (UfGlobal::load(parent + c) == kFrNone) return;
  for (int n = -1; n <= 1; ++n) {  // the last column: NE, E, SE; the last row: SW, S, SE
    const int nx = column ? (int)x + 1 : (int)x + n, ny = column ? (int)y + n : (int)y + 1;
    if (nx < 0 || ny < 0 || nx >= (int)a.width || ny >= (int)a.height) continue;
    const uint32_t q = (uint32_t)ny * a.width + (uint32_t)nx;  // below cells
    if (UfGlobal::load(parent + q) == kFrNone) continue;
    uf_unite(parent, c, q, fr_uf(cells, grp));
  }
}

__global__ __launch_bounds__(kBlock) void k_fr_flatten(FrArgs a, uint32_t *__restrict__ labels, fu64 label_stride) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  const uint32_t g = blockIdx.y;
  uint32_t *grp = a.scratch + (size_t)g * a.l.total;
  uint32_t *parent = grp + a.l.parent;
  const uint32_t cells = (uint32_t)a.l.cells;
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  uint32_t is_root = 0u;
  if (c < cells) {
    uint32_t label = kFrNone;
    if (UfGlobal::load(parent + c) != kFrNone) {
      label = uf_find(parent, c, fr_uf(cells, grp));
      atomicMin(parent + c, label);
      is_root = label == c ? 1u : 0u;
    }
    if (labels) labels[(size_t)g * label_stride + c] = label;
  }
  uint32_t total;
  const uint32_t pre = block_excl_scan(is_root, s_tmp, &total);
  if (is_root) grp[a.l.ord + c] = pre;
  if (threadIdx.x == 0) grp[a.l.rbase + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_fr_rank(FrArgs a) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  uint32_t *grp = a.scratch + (size_t)blockIdx.x * a.l.total;
  uint32_t *rbase = grp + a.l.rbase;
  const uint32_t per = (a.l.blocks + kBlock - 1u) / kBlock;  // <= 16
  const uint32_t i0 = threadIdx.x * per;
  uint32_t sum = 0u;
  for (uint32_t j = 0; j < per && j < 16u; ++j)  // bound: 16
    if (i0 + j < a.l.blocks) sum += rbase[i0 + j];
  uint32_t N;
  uint32_t run = block_excl_scan(sum, s_tmp, &N);
  for (uint32_t j = 0; j < per && j < 16u; ++j) {  // bound: 16
    if (i0 + j >= a.l.blocks) break;
    const uint32_t v = rbase[i0 + j];
    rbase[i0 + j] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    grp[FH_N] = N;
    grp[FH_OVER] = N > a.comp_cap ? 1u : 0u;
  }
}

// the table row of a root: its rank among the roots in ascending cell index, clamped below comp_cap
__device__ __forceinline__ uint32_t *fr_row(const FrArgs &a, uint32_t *grp, uint32_t root) {
  const uint32_t rank = grp[a.l.rbase + (root >> 10)] + grp[a.l.ord + root];
  return grp + a.l.table + 8ull * min(rank, a.comp_cap - 1u);
}
__device__ __forceinline__ void fr_send(uint32_t *row, uint32_t n, fu64 sx, fu64 sy, fu64 key) {
  atomicAdd(row, n);
  atomicAdd(reinterpret_cast<fu64 *>(row + 2), sx);
  atomicAdd(reinterpret_cast<fu64 *>(row + 4), sy);
  atomicMin(reinterpret_cast<fu64 *>(row + 6), key);
}

__global__ __launch_bounds__(kFrTileBlock) void k_fr_sums(FrArgs a) {
  __shared__ uint32_t s_root[kFrSlots], s_n[kFrSlots];
  __shared__ fu64 s_sx[kFrSlots], s_sy[kFrSlots], s_key[kFrSlots];
  const FrTileAt at = fr_tile_at(a);
  uint32_t *grp = a.scratch + (size_t)at.g * a.l.total;
  if (grp[FH_OVER]) return;  // (block-uniform)
  const uint32_t *parent = grp + a.l.parent;
  const uint32_t *pot = a.pot ? a.pot + (size_t)at.g * a.pot_stride : nullptr;
  const uint32_t cells = (uint32_t)a.l.cells;
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < kFrSlots; i += kFrTileBlock) {  // bound: 4 rounds
    s_root[i] = kFrNone;
    s_n[i] = 0u;
    s_sx[i] = 0ull;
    s_sy[i] = 0ull;
    s_key[i] = ~0ull;
  }
  __syncthreads();
  for (uint32_t i = tid; i < kFrTileCells; i += kFrTileBlock) {  // bound: 16 rounds
    const uint32_t x = at.x0 + (i & 63u), y = at.y0 + (i >> 6);
    if (x >= a.width || y >= a.height) continue;
    const uint32_t c = y * a.width + x;
    uint32_t root = parent[c];
    if (root == kFrNone) continue;
    root = min(root, cells - 1u);
    const fu64 key = ((fu64)(pot ? pot[c] : 0u) << 32) | c;
    if (root == c) fr_row(a, grp, root)[1] = root;  // (the one cell of the component that is its root)
    const uint32_t slot = (root * 2654435761u) >> 22;
    bool placed = false;
    for (uint32_t probe = 0; probe < kFrProbes && !placed; ++probe) {  // bound: kFrProbes
      const uint32_t at_slot = (slot + probe) & (kFrSlots - 1u);
      const uint32_t old = atomicCAS(&s_root[at_slot], kFrNone, root);
      if (old != kFrNone && old != root) continue;
      atomicAdd(&s_n[at_slot], 1u);
      atomicAdd(&s_sx[at_slot], (fu64)x);
      atomicAdd(&s_sy[at_slot], (fu64)y);
      atomicMin(&s_key[at_slot], key);
      placed = true;
    }
    if (!placed) fr_send(fr_row(a, grp, root), 1u, x, y, key);
  }
  __syncthreads();
  for (uint32_t i = tid; i < kFrSlots; i += kFrTileBlock) {  // bound: 4 rounds
    const uint32_t root = s_root[i];
    if (root != kFrNone) fr_send(fr_row(a, grp, root), s_n[i], s_sx[i], s_sy[i], s_key[i]);
  }
}

struct FrBest {
  long long cost;
  uint32_t label, rank;
};
__device__ __forceinline__ bool fr_better(const FrBest &p, const FrBest &q) {
  if (p.label == kFrNone) return false;
  return q.label == kFrNone || p.cost < q.cost || (p.cost == q.cost && p.label < q.label);
}

__global__ __launch_bounds__(kBlock) void k_fr_close(FrArgs a, uint32_t min_size, uint32_t dist_weight,
                                                    uint32_t size_weight, uint32_t *__restrict__ rows, fu64 row_stride,
                                                    uint32_t row_cap, uint32_t *__restrict__ goal, fu64 goal_stride,
                                                    uint32_t *__restrict__ n_goal, uint32_t *__restrict__ result) {
  __shared__ uint32_t s_tmp[kWaves + 1];
  __shared__ long long s_cost[kBlock];
  __shared__ uint32_t s_label[kBlock], s_rank[kBlock], s_drop[kBlock], s_max[kBlock];
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const uint32_t *grp = a.scratch + (size_t)g * a.l.total;
  const uint32_t *table = grp + a.l.table;
  const uint32_t F = grp[FH_F], N = grp[FH_N], over = grp[FH_OVER];
  uint32_t flags = grp[FH_FLAGS] & RPLGPU_FRONTIER_LOOP;
  const uint32_t n_rows = over ? 0u : min(N, a.comp_cap);
  uint32_t *out_rows = rows ? rows + (size_t)g * row_stride : nullptr;
  uint32_t kept = 0u, dropped = 0u, greatest = 0u;
  FrBest best{0, kFrNone, 0u};
  for (uint32_t base = 0, round = 0; base < n_rows && round < 1024u; base += kBlock, ++round) {  // bound: 1024 rounds
    const uint32_t r = base + tid;
    uint32_t is_kept = 0u;
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
    if (r < n_rows) {
      lo = reinterpret_cast<const uint4 *>(table + 8ull * r)[0];  // n, label, sum cx
      hi = reinterpret_cast<const uint4 *>(table + 8ull * r)[1];  // sum cy, the key (cell, Dmin)
      greatest = max(greatest, lo.x);
      if (lo.x >= min_size) {
        is_kept = 1u;
        const FrBest mine{(long long)dist_weight * (long long)hi.w - (long long)size_weight * (long long)lo.x, lo.y, r};
        if (fr_better(mine, best)) best = mine;
      } else {
        dropped += lo.x;
      }
    }
    uint32_t total;
    const uint32_t pos = kept + block_excl_scan(is_kept, s_tmp, &total);
    if (is_kept && out_rows && pos < row_cap) {
      const uint32_t row[8] = {lo.y, lo.x, lo.z, lo.w, hi.x, hi.y, hi.w, hi.z};
      for (uint32_t i = 0; i < 8u; ++i) out_rows[8ull * pos + i] = row[i];
    }
    kept += total;
    __syncthreads();
  }
  s_cost[tid] = best.cost;
  s_label[tid] = best.label;
  s_rank[tid] = best.rank;
  s_drop[tid] = dropped;
  s_max[tid] = greatest;
  __syncthreads();
  for (uint32_t half = kBlock / 2u; half > 0u; half >>= 1) {  // bound: 10 rounds
    if (tid < half) {
      const FrBest p{s_cost[tid], s_label[tid], s_rank[tid]}, q{s_cost[tid + half], s_label[tid + half], s_rank[tid + half]};
      if (fr_better(q, p)) {
        s_cost[tid] = q.cost;
        s_label[tid] = q.label;
        s_rank[tid] = q.rank;
      }
      s_drop[tid] += s_drop[tid + half];
      s_max[tid] = max(s_max[tid], s_max[tid + half]);
    }
    __syncthreads();
  }
  if (tid != 0) return;
  uint32_t w[16] = {0u, F, N, kept, s_drop[0], kFrNone, 0u, 0u, 0u, 0u, 0u, 0u, 0u, s_max[0], 0u, 0u};
  w[14] = out_rows ? min(kept, row_cap) : 0u;
  if (F == 0u) flags |= RPLGPU_FRONTIER_NONE;
  if (over) flags |= RPLGPU_FRONTIER_BOUND;
  const bool have = s_label[0] != kFrNone;
  if (have) {
    const uint32_t *row = table + 8ull * min(s_rank[0], a.comp_cap - 1u);
    w[5] = row[1];
    w[6] = row[0];
    w[7] = row[7];
    w[8] = row[6];
    w[9] = row[2];
    w[10] = row[3];
    w[11] = row[4];
    w[12] = row[5];
  } else {
    flags |= RPLGPU_FRONTIER_NO_KEPT;
  }
  w[0] = flags;
  for (uint32_t i = 0; i < 16u; ++i) result[16ull * g + i] = w[i];
  if (goal && n_goal) {
    if (have) goal[(size_t)g * goal_stride] = w[8];
    n_goal[g] = have ? 1u : 0u;
  }
}

}  // namespace

hipError_t launch_frontiers(hipStream_t s, const FrontierK &k, const int8_t *grid, unsigned long long grid_stride,
                            const uint32_t *potential, unsigned long long potential_stride, uint32_t G,
                            uint32_t comp_cap, uint32_t *labels, unsigned long long label_stride, uint32_t *rows,
                            unsigned long long row_stride, uint32_t row_cap, uint32_t *goal,
                            unsigned long long goal_stride, uint32_t *n_goal, uint32_t *result, uint32_t *scratch) {
  FrArgs a;
  if (!frontier_layout(k.width, k.height, G, comp_cap, &a.l)) return hipErrorInvalidValue;
  a.width = k.width;
  a.height = k.height;
  a.lethal = k.lethal;
  a.comp_cap = comp_cap;
  a.grid = grid;
  a.grid_stride = grid_stride;
  a.pot = potential;
  a.pot_stride = potential_stride;
  a.scratch = scratch;
  const uint32_t tiles = a.l.tiles_x * a.l.tiles_y * G;  // <= RPLGPU_NAV_MAX_TILES
  const uint32_t init_blocks = ((comp_cap > kFrHdrWords ? comp_cap : kFrHdrWords) + kBlock - 1u) / kBlock;
#define RPL_FR_LAUNCH(kernel, grid_dim, block_dim, ...)                   \
  hipLaunchKernelGGL(kernel, grid_dim, dim3(block_dim), 0, s, __VA_ARGS__); \
  if (hipError_t e = hipGetLastError()) return e
  RPL_FR_LAUNCH(k_fr_init, dim3(init_blocks, G), kBlock, a);
  RPL_FR_LAUNCH(k_fr_tile, dim3(tiles), kFrTileBlock, a);
  RPL_FR_LAUNCH(k_fr_seam, dim3(tiles), kFrSeamBlock, a);
  RPL_FR_LAUNCH(k_fr_flatten, dim3(a.l.blocks, G), kBlock, a, labels, label_stride);
  RPL_FR_LAUNCH(k_fr_rank, dim3(G), kBlock, a);
  RPL_FR_LAUNCH(k_fr_sums, dim3(tiles), kFrTileBlock, a);
  RPL_FR_LAUNCH(k_fr_close, dim3(G), kBlock, a, k.min_size, k.dist_weight, k.size_weight, rows, row_stride, row_cap,
                goal, goal_stride, n_goal, result);
#undef RPL_FR_LAUNCH
  return hipSuccess;
}

}  // namespace rpl
