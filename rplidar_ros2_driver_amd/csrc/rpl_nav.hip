// rpl_nav.hip — E26: the cost-to-goal field over a costmap and the paths down it (include/rplgpu_msg.h,
// rplgpu_nav_field_dev / rplgpu_nav_paths_dev).  The field is the least fixed point of a min-plus equation over
// integers, so any schedule of relaxations that only ever lowers a word to the length of a real path ends on it.
//
// k_nav_relax, the hot path: one 256-thread workgroup per 64 x 64 tile per grid (tiles x G flattened into
// blockIdx.x), one launch a ROUND.
//   * DIRTY  one thread reads the tile's word of this round's plane and clears it; a tile that is not dirty leaves.
//   * STAGE  the tile's D with a one-cell halo (66 x 66 words, pitch 67: a lane a row and a lane a column both walk
//     the banks without a conflict) and the cells' weights (66 x 66 uint16, 0 = impassable or outside) go to LDS;
//     then every cell's four diagonal permissions (the corner rule) are folded into its weight word's bits 11 - 14.
//   * RELAX  in LDS until a round of sweeps changes nothing (one __syncthreads_or a round): wave 0 sweeps left to
//     right (a lane a row), wave 1 right to left, wave 2 top to bottom (a lane a column), wave 3 bottom to top, all at
//     once on the same words; a step reads the three neighbours upstream and lowers the cell with an LDS atomic min,
//     so a value crosses the tile in one sweep and two waves meeting on a cell lose nothing.  (The other form that
//     was measured — a thread per 16-cell strip against all eight neighbours — lost by 2.5 x to 4.9 x and lives in
//     tools/dev/patches/nav_plain_sweeps_r33.diff.)
//   * STORE  the cells that changed; where one of them lies on the tile's border, the up to eight tiles that read
//     it are marked dirty in the NEXT round's plane.
// No workgroup ever waits for another and no fence crosses workgroups: D is updated in place, only a tile's owner
// writes its interior, and a halo word read old or new is the length of a real path either way — every value is
// always >= the answer; the owner of a changed border marks its neighbours for the next launch, so a field with no
// dirty tile is the fixed point.  Convergence is carried by launch boundaries only.
//
// k_nav_init / k_nav_goals / k_nav_close / k_nav_stats: the field filled and the planes cleared, the goals written
// and the tiles that read them marked, the dirty tiles counted (and the live plane moved to plane 0, where the next call starts),
// the reached cells and their greatest value.
// k_nav_paths: one thread a path, a dependent chain of neighbour reads — not the hot path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rpl_device.hpp"
#include "rplgpu_msg.h"
#include "rpl_rules.hpp"
#include "rpl_nav.hpp"

namespace rpl {
namespace {

constexpr uint32_t kNavThreads = 256;
constexpr int kT = (int)RPLGPU_NAV_TILE;
constexpr int kDP = kT + 3;   // pitch of a D row in LDS, words (odd)
constexpr int kWP = kT + 2;   // pitch of a weight row in LDS, uint16
constexpr uint32_t kNone = RPLGPU_NAV_UNREACHED;
constexpr uint32_t kWeightMask = 0x7FFu;
static_assert(RPLGPU_NAV_MAX_COST <= kWeightMask, "a weight and four permissions share a uint16");
static_assert((unsigned long long)RPLGPU_NAV_MAX_CAP + 7ull * RPLGPU_NAV_MAX_COST < (1ull << 32), "cap + a step overflows");
constexpr uint32_t kBit4 = 1u << 11, kBit5 = 1u << 12, kBit6 = 1u << 13, kBit7 = 1u << 14;  // steps 4 .. 7 allowed

__device__ __forceinline__ uint32_t nav_weight(const NavK &k, uint32_t byte) {
  return nav_byte_weight(k, (int)(int8_t)byte);
}

// the least of what the four straight (n4) and the permitted diagonal (n7) neighbours offer a cell of weight w
__device__ __forceinline__ uint32_t nav_offer(uint32_t n4, uint32_t n7, uint32_t w, uint32_t cap) {
  const uint32_t c4 = n4 <= cap ? n4 + 5u * w : kNone;  // (a reached word is <= cap <= 0xFFFF0000: no carry)
  const uint32_t c7 = n7 <= cap ? n7 + 7u * w : kNone;
  const uint32_t best = min(c4, c7);
  return best <= cap ? best : kNone;
}

__device__ __forceinline__ uint32_t lds_read(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one directional sweep of one wave: the lane's line starts at D word p and weight pw, a step along it is ds (dsw in
// the weights), the line beside it dl; bit_m / bit_p: the permissions of the steps to (-ds, -dl) and (-ds, +dl)
__device__ __forceinline__ int nav_sweep(uint32_t *sD, const uint16_t *sW, int p, int ds, int dl, int pw, int dsw,
                                         uint32_t bit_m, uint32_t bit_p, uint32_t cap) {
  int changed = 0;
  for (int i = 0; i < kT; ++i, p += ds, pw += dsw) {
    const uint32_t info = sW[pw], w = info & kWeightMask;
    const uint32_t n5 = lds_read(&sD[p - ds]), nm = lds_read(&sD[p - ds - dl]), np = lds_read(&sD[p - ds + dl]);
    const uint32_t own = lds_read(&sD[p]);
    const uint32_t n7 = min((info & bit_m) ? nm : kNone, (info & bit_p) ? np : kNone);
    const uint32_t best = w ? nav_offer(n5, n7, w, cap) : kNone;
    if (best < own) {
      atomicMin(&sD[p], best);
      changed = 1;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next step's reads stay behind this step's min)
  }
  return changed;
}

__global__ __launch_bounds__(kNavThreads) void k_nav_relax(NavK k, const uint8_t *__restrict__ grid,
                                                           unsigned long long grid_stride, uint32_t *potential,
                                                           unsigned long long potential_stride, uint32_t *flags,
                                                           uint32_t round, uint32_t *result) {
  __shared__ uint32_t sD[(kT + 2) * kDP];
  __shared__ uint16_t sW[(kT + 2) * kWP];
  __shared__ uint32_t s_mark[9];
  __shared__ uint32_t s_dirty;
  const uint32_t tid = threadIdx.x;
  const uint32_t tiles = k.tiles_x * k.tiles_y;
  const uint32_t g = blockIdx.x / tiles, t = blockIdx.x - g * tiles;
  uint32_t *plane = flags + ((size_t)g * 2u + (round & 1u)) * tiles;
  uint32_t *plane_next = flags + ((size_t)g * 2u + ((round + 1u) & 1u)) * tiles;

  // DIRTY (one reader: every thread of the workgroup takes the same way)
  if (tid == 0) {
    const uint32_t d = __hip_atomic_load(&plane[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_dirty = d;
    if (d) __hip_atomic_store(&plane[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid < 9u) s_mark[tid] = 0u;
  __syncthreads();
  if (!s_dirty) return;

  const uint32_t W = k.width, H = k.height;
  const uint32_t tile_y = t / k.tiles_x, tile_x = t - tile_y * k.tiles_x;
  const int x0 = (int)(tile_x * RPLGPU_NAV_TILE), y0 = (int)(tile_y * RPLGPU_NAV_TILE);
  const uint8_t *ggrid = grid + (size_t)g * grid_stride;
  uint32_t *gpot = potential + (size_t)g * potential_stride;
  const int lx = (int)(tid & 63u), ly0 = (int)(tid >> 6) * 16;

  // STAGE: the thread's 16 cells, then the 260 cells of the halo; a cell outside the grid is UNREACHED and impassable
  uint32_t orig[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t gx = (uint32_t)(x0 + lx), gy = (uint32_t)(y0 + ly0 + j);
    uint32_t d = kNone, w = 0u;
    if (gx < W && gy < H) {
      const uint32_t c = gy * W + gx;  // < 2^24
      d = gpot[c];
      w = nav_weight(k, ggrid[c]);
    }
    orig[j] = d;
    sD[(ly0 + j + 1) * kDP + lx + 1] = d;
    sW[(ly0 + j + 1) * kWP + lx + 1] = (uint16_t)w;
  }
  for (int i = (int)tid; i < 4 * kT + 4; i += (int)kNavThreads) {
    int hx, hy;
    if (i < kT + 2) { hx = i; hy = 0; }
    else if (i < 2 * (kT + 2)) { hx = i - (kT + 2); hy = kT + 1; }
    else if (i < 3 * kT + 4) { hx = 0; hy = i - 2 * (kT + 2) + 1; }
    else { hx = kT + 1; hy = i - (3 * kT + 4) + 1; }
    const int gx = x0 + hx - 1, gy = y0 + hy - 1;
    uint32_t d = kNone, w = 0u;
    if (gx >= 0 && gy >= 0 && (uint32_t)gx < W && (uint32_t)gy < H) {
      const uint32_t c = (uint32_t)gy * W + (uint32_t)gx;
      d = gpot[c];
      w = nav_weight(k, ggrid[c]);
    }
    sD[hy * kDP + hx] = d;
    sW[hy * kWP + hx] = (uint16_t)w;
  }
  __syncthreads();
  // the corner rule: a diagonal step needs both cells it passes between (a side cell outside the grid has weight 0,
  // and then so is the diagonal neighbour)
  uint32_t info[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int p = (ly0 + j + 1) * kWP + lx + 1;
    const uint32_t w = sW[p];
    const bool e = sW[p + 1] != 0, wst = sW[p - 1] != 0, s = sW[p + kWP] != 0, n = sW[p - kWP] != 0;
    info[j] = w ? (w | (e && s ? kBit4 : 0u) | (wst && s ? kBit5 : 0u) | (e && n ? kBit6 : 0u) | (wst && n ? kBit7 : 0u))
                : 0u;
  }
  __syncthreads();  // (every plain weight is read before the first word with permissions is written)
#pragma unroll
  for (int j = 0; j < 16; ++j) sW[(ly0 + j + 1) * kWP + lx + 1] = (uint16_t)info[j];
  __syncthreads();

  // RELAX: four sweeps at once, one wave each, until a round of them changes nothing
  const uint32_t cap = k.cap;
  const uint32_t wave = tid >> 6;
  const int l = (int)(tid & 63u);
  for (;;) {
    int changed;
    if (wave == 0u)       // left to right: lane = row l, upstream (-1, 0), (-1, -1) step 7, (-1, +1) step 5
      changed = nav_sweep(sD, sW, (l + 1) * kDP + 1, 1, kDP, (l + 1) * kWP + 1, 1, kBit7, kBit5, cap);
    else if (wave == 1u)  // right to left: upstream (+1, 0), (+1, +1) step 4, (+1, -1) step 6
      changed = nav_sweep(sD, sW, (l + 1) * kDP + kT, -1, -kDP, (l + 1) * kWP + kT, -1, kBit4, kBit6, cap);
    else if (wave == 2u)  // top to bottom: lane = column l, upstream (0, -1), (-1, -1) step 7, (+1, -1) step 6
      changed = nav_sweep(sD, sW, kDP + l + 1, kDP, 1, kWP + l + 1, kWP, kBit7, kBit6, cap);
    else                  // bottom to top: upstream (0, +1), (+1, +1) step 4, (-1, +1) step 5
      changed = nav_sweep(sD, sW, kT * kDP + l + 1, -kDP, -1, kT * kWP + l + 1, -kWP, kBit4, kBit5, cap);
    if (!__syncthreads_or(changed)) break;
  }

  // STORE: what changed, and whom a changed border cell concerns
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int y = ly0 + j;
    const uint32_t d = sD[(y + 1) * kDP + lx + 1];
    if (d == orig[j]) continue;  // (a cell outside the grid never changes: its weight is 0)
    gpot[(uint32_t)(y0 + y) * W + (uint32_t)(x0 + lx)] = d;
    const bool xl = lx == 0, xr = lx == kT - 1, yt = y == 0, yb = y == kT - 1;
    if (xl) s_mark[3] = 1u;
    if (xr) s_mark[5] = 1u;
    if (yt) s_mark[1] = 1u;
    if (yb) s_mark[7] = 1u;
    if (xl && yt) s_mark[0] = 1u;
    if (xr && yt) s_mark[2] = 1u;
    if (xl && yb) s_mark[6] = 1u;
    if (xr && yb) s_mark[8] = 1u;
  }
  __syncthreads();
  if (tid < 9u && tid != 4u && s_mark[tid]) {
    const int nx = (int)tile_x + (int)(tid % 3u) - 1, ny = (int)tile_y + (int)(tid / 3u) - 1;
    if (nx >= 0 && ny >= 0 && (uint32_t)nx < k.tiles_x && (uint32_t)ny < k.tiles_y)
      __hip_atomic_store(&plane_next[(uint32_t)ny * k.tiles_x + (uint32_t)nx], 1u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) {
    atomicAdd(&result[8u * g + 6u], 1u);
    atomicMax(&result[8u * g + 7u], round + 1u);  // (the rounds with a dirty tile are the first ones)
  }
}

// The workgroup's sum of one value a thread, for k_nav_goals and k_nav_close (local to this unit: written for whole
// waves of 64 and a word at *s_sum that one thread cleared in front of a barrier the workgroup has passed).  The
// waves' sums meet in *s_sum by one LDS atomic a wave that has something to add; every thread passes the barrier
// inside and reads the total behind it.
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *s_sum) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane_id() == 0 && v) atomicAdd(s_sum, v);
  __syncthreads();
  return *s_sum;
}

// blockIdx.y: the grid.  The field UNREACHED and both planes clear unless resumed; the result words zero.
__global__ __launch_bounds__(kNavThreads) void k_nav_init(uint32_t cells, uint32_t tiles, uint32_t *potential,
                                                          unsigned long long potential_stride, uint32_t *flags,
                                                          uint32_t resume, uint32_t *result) {
  const uint32_t g = blockIdx.y;
  const uint32_t i0 = blockIdx.x * kNavThreads + threadIdx.x, step = gridDim.x * kNavThreads;
  if (i0 < 8u) result[8u * g + i0] = 0u;
  if (resume) return;
  uint32_t *gpot = potential + (size_t)g * potential_stride;
  for (uint32_t i = i0; i < cells; i += step) gpot[i] = kNone;
  uint32_t *gflags = flags + (size_t)g * 2u * tiles;
  for (uint32_t i = i0; i < 2u * tiles; i += step) gflags[i] = 0u;
}

// one workgroup a grid
__global__ __launch_bounds__(kNavThreads) void k_nav_goals(uint32_t W, uint32_t cells, uint32_t tiles_x, uint32_t tiles,
                                                           const uint32_t *__restrict__ goals,
                                                           unsigned long long goal_stride,
                                                           const uint32_t *__restrict__ n_goals, uint32_t *potential,
                                                           unsigned long long potential_stride, uint32_t *flags,
                                                           uint32_t resume, uint32_t *result) {
  __shared__ uint32_t s_taken;
  const uint32_t g = blockIdx.x;
  if (threadIdx.x == 0) s_taken = 0u;
  __syncthreads();
  const uint32_t n = n_goals[g], n_read = min(n, (uint32_t)RPLGPU_NAV_MAX_GOALS);
  const uint32_t *gg = goals + (size_t)g * goal_stride;
  uint32_t *gpot = potential + (size_t)g * potential_stride;
  uint32_t *plane0 = flags + (size_t)g * 2u * tiles;
  uint32_t taken = 0;
  for (uint32_t i = threadIdx.x; i < n_read; i += kNavThreads) {
    const uint32_t c = gg[i];
    if (c >= cells) continue;
    ++taken;
    if (resume) continue;  // (the goals are in the field already)
    gpot[c] = 0u;
    // the goal's tile and every tile whose halo holds the goal: a goal is no CHANGED cell when its tile runs, so
    // nobody else would tell the tiles that read it across a border
    const uint32_t y = c / W, x = c - y * W;
    const uint32_t tiles_y = tiles / tiles_x;
    const uint32_t tx0 = (x ? x - 1u : 0u) / RPLGPU_NAV_TILE, tx1 = min((x + 1u) / RPLGPU_NAV_TILE, tiles_x - 1u);
    const uint32_t ty0 = (y ? y - 1u : 0u) / RPLGPU_NAV_TILE, ty1 = min((y + 1u) / RPLGPU_NAV_TILE, tiles_y - 1u);
    for (uint32_t ty = ty0; ty <= ty1; ++ty)
      for (uint32_t tx = tx0; tx <= tx1; ++tx) plane0[ty * tiles_x + tx] = 1u;
  }
  taken = block_sum(taken, &s_taken);
  if (threadIdx.x == 0) {
    result[8u * g + 2u] = taken;
    result[8u * g + 3u] = n - taken;
  }
}

// one workgroup a grid: the dirty tiles left after `rounds` rounds into words 0 and 1; the live plane becomes plane 0
__global__ __launch_bounds__(kNavThreads) void k_nav_close(uint32_t tiles, uint32_t *flags, uint32_t rounds,
                                                           uint32_t *result) {
  __shared__ uint32_t s_count;
  const uint32_t g = blockIdx.x;
  uint32_t *plane0 = flags + (size_t)g * 2u * tiles, *plane1 = plane0 + tiles;
  if (threadIdx.x == 0) s_count = 0u;
  __syncthreads();
  const bool live1 = (rounds & 1u) != 0u;
  uint32_t count = 0;
  for (uint32_t i = threadIdx.x; i < tiles; i += kNavThreads) {
    const uint32_t d = live1 ? plane1[i] : plane0[i];
    if (d) ++count;
    if (live1) {
      plane0[i] = d;
      plane1[i] = 0u;
    }
  }
  count = block_sum(count, &s_count);
  if (threadIdx.x == 0) {
    result[8u * g + 0u] = count;
    result[8u * g + 1u] = count ? RPLGPU_NAV_UNFINISHED : 0u;
  }
}

// blockIdx.y: the grid.  The reached cells and the greatest reached value into words 4 and 5.  The sum and the greatest
// value go through ONE butterfly loop and ONE barrier, written out here: with block_sum and a block-max of its kind
// beside it the kernel came out with 11 VGPRs for 8 (and 193 instructions for 190), so this call site keeps its copy.
__global__ __launch_bounds__(kNavThreads) void k_nav_stats(uint32_t cells, const uint32_t *__restrict__ potential,
                                                           unsigned long long potential_stride, uint32_t *result) {
  __shared__ uint32_t s_n, s_max;
  const uint32_t g = blockIdx.y;
  const uint32_t *gpot = potential + (size_t)g * potential_stride;
  if (threadIdx.x == 0) s_n = s_max = 0u;
  __syncthreads();
  uint32_t n = 0, hi = 0;
  for (uint32_t i = blockIdx.x * kNavThreads + threadIdx.x; i < cells; i += gridDim.x * kNavThreads) {
    const uint32_t d = gpot[i];
    if (d != kNone) {
      ++n;
      hi = max(hi, d);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    n += __shfl_xor(n, d, 64);
    hi = max(hi, (uint32_t)__shfl_xor(hi, d, 64));
  }
  if (lane_id() == 0 && n) {
    atomicAdd(&s_n, n);
    atomicMax(&s_max, hi);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_n) {
    atomicAdd(&result[8u * g + 4u], s_n);
    atomicMax(&result[8u * g + 5u], s_max);
  }
}

// blockIdx.y: the grid; one thread a path
__global__ __launch_bounds__(kNavThreads) void k_nav_paths(NavK k, const uint8_t *__restrict__ grid,
                                                           unsigned long long grid_stride,
                                                           const uint32_t *__restrict__ potential,
                                                           unsigned long long potential_stride,
                                                           const uint32_t *__restrict__ starts, uint32_t S,
                                                           uint32_t *paths, uint32_t max_len, uint32_t *info) {
  const uint32_t g = blockIdx.y, s = blockIdx.x * kNavThreads + threadIdx.x;
  if (s >= S) return;
  const int W = (int)k.width, H = (int)k.height;
  const uint32_t cells = k.width * k.height;
  const uint8_t *ggrid = grid + (size_t)g * grid_stride;
  const uint32_t *gpot = potential + (size_t)g * potential_stride;
  const size_t at = (size_t)g * S + s;
  uint32_t *path = paths + at * max_len;
  const uint32_t start = starts[at];
  uint32_t len = 0, flags = 0, d0 = kNone, last = start;
  if (start >= cells) {
    flags = RPLGPU_NAV_PATH_NO_START;
  } else if ((d0 = gpot[start]) == kNone) {
    flags = RPLGPU_NAV_PATH_UNREACHED;
  } else {
    uint32_t c = start, d = d0;
    for (;;) {
      path[len++] = c;
      last = c;
      if (d == 0u) {
        flags = RPLGPU_NAV_PATH_REACHED;
        break;
      }
      if (len == max_len) {
        flags = RPLGPU_NAV_PATH_TRUNCATED;
        break;
      }
      const int cy = (int)(c / k.width), cx = (int)(c - (uint32_t)cy * k.width);
      const uint32_t w = nav_weight(k, ggrid[c]);
      uint32_t next = kNone, dn_next = 0;
      if (w) {
        const bool in_e = cx + 1 < W, in_w = cx > 0, in_s = cy + 1 < H, in_n = cy > 0;
        const bool e = in_e && nav_weight(k, ggrid[c + 1u]) != 0u, wst = in_w && nav_weight(k, ggrid[c - 1u]) != 0u;
        const bool so = in_s && nav_weight(k, ggrid[c + k.width]) != 0u;
        const bool no = in_n && nav_weight(k, ggrid[c - k.width]) != 0u;
        const bool ok[8] = {in_e, in_w, in_s, in_n, e && so, wst && so, e && no, wst && no};
        const int dx[8] = {1, -1, 0, 0, 1, -1, 1, -1}, dy[8] = {0, 0, 1, -1, 1, 1, -1, -1};
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) {
          if (next != kNone || !ok[dir]) continue;
          const uint32_t n = (uint32_t)((cy + dy[dir]) * W + cx + dx[dir]);
          const uint32_t dn = gpot[n];
          // (dn <= d keeps the sum from wrapping: a word above d cannot satisfy the equality)
          if (dn != kNone && dn <= d && dn + (dir < 4 ? 5u : 7u) * w == d) {
            next = n;
            dn_next = dn;
          }
        }
      }
      if (next == kNone) {
        flags = RPLGPU_NAV_PATH_BROKEN;
        break;
      }
      c = next;
      d = dn_next;
    }
  }
  info[4u * at + 0u] = len;
  info[4u * at + 1u] = flags;
  info[4u * at + 2u] = d0;
  info[4u * at + 3u] = last;
}

uint32_t span_blocks(uint32_t items) {  // workgroups of a grid-stride launch over `items`
  return std::min<uint32_t>(std::max<uint32_t>((items + kNavThreads - 1u) / kNavThreads, 1u), 4096u);
}

}  // namespace

hipError_t launch_nav_init(hipStream_t s, const NavK &k, uint32_t G, uint32_t *potential,
                           unsigned long long potential_stride, uint32_t *flags, uint32_t resume, uint32_t *result) {
  const uint32_t cells = k.width * k.height, tiles = k.tiles_x * k.tiles_y;
  hipLaunchKernelGGL(k_nav_init, dim3(resume ? 1u : span_blocks(cells), G), dim3(kNavThreads), 0, s, cells, tiles,
                     potential, potential_stride, flags, resume, result);
  return hipGetLastError();
}

hipError_t launch_nav_goals(hipStream_t s, const NavK &k, uint32_t G, const uint32_t *goals,
                            unsigned long long goal_stride, const uint32_t *n_goals, uint32_t *potential,
                            unsigned long long potential_stride, uint32_t *flags, uint32_t resume, uint32_t *result) {
  hipLaunchKernelGGL(k_nav_goals, dim3(G), dim3(kNavThreads), 0, s, k.width, k.width * k.height, k.tiles_x,
                     k.tiles_x * k.tiles_y, goals, goal_stride, n_goals, potential, potential_stride, flags, resume,
                     result);
  return hipGetLastError();
}

hipError_t launch_nav_relax(hipStream_t s, const NavK &k, uint32_t G, const int8_t *grid,
                            unsigned long long grid_stride, uint32_t *potential, unsigned long long potential_stride,
                            uint32_t *flags, uint32_t round, uint32_t *result) {
  uint32_t tiles_x, tiles_y;
  if (!nav_tiles(k.width, k.height, G, &tiles_x, &tiles_y)) return hipErrorInvalidValue;  // (x 256 threads: below 2^32)
  hipLaunchKernelGGL(k_nav_relax, dim3(G * tiles_x * tiles_y), dim3(kNavThreads), 0, s, k, (const uint8_t *)grid,
                     grid_stride, potential, potential_stride, flags, round, result);
  return hipGetLastError();
}

hipError_t launch_nav_close(hipStream_t s, const NavK &k, uint32_t G, const uint32_t *potential,
                            unsigned long long potential_stride, uint32_t *flags, uint32_t rounds, uint32_t *result) {
  hipLaunchKernelGGL(k_nav_close, dim3(G), dim3(kNavThreads), 0, s, k.tiles_x * k.tiles_y, flags, rounds, result);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint32_t cells = k.width * k.height;
  hipLaunchKernelGGL(k_nav_stats, dim3(span_blocks(cells / 4u), G), dim3(kNavThreads), 0, s, cells, potential,
                     potential_stride, result);
  return hipGetLastError();
}

hipError_t launch_nav_paths(hipStream_t s, const NavK &k, uint32_t G, const int8_t *grid,
                            unsigned long long grid_stride, const uint32_t *potential,
                            unsigned long long potential_stride, const uint32_t *starts, uint32_t S, uint32_t *paths,
                            uint32_t max_len, uint32_t *info) {
  if (G == 0 || G > 65535u || S == 0 || max_len == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_nav_paths, dim3((S + kNavThreads - 1u) / kNavThreads, G), dim3(kNavThreads), 0, s, k,
                     (const uint8_t *)grid, grid_stride, potential, potential_stride, starts, S, paths, max_len, info);
  return hipGetLastError();
}

}  // namespace rpl
