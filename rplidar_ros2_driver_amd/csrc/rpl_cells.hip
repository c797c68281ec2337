// rpl_cells.hip — rplgpu_merge_cells_dev (include/rplgpu_comm.h): the gathered cell records of every rank
// -> ONE fused voxel grid per group, byte-identical to rplgpu_cloud_fused_voxel_dev over all the group's
// scans (the records hold exact integer sums; the rules are in rpl_cells.hpp, shared with the host twin).
//
// A rank's records of a group are sorted by key and unique, so the union needs no sort: a merge by
// co-rank.  One workgroup per group (grid-stride over the groups), two passes over its records:
//   1. record j of rank r is the LEADER of its key when no rank s < r holds that key (binary searches
//      over the lists of the ranks before it, which sit in L2).  A running block scan over the leader
//      flags, rank after rank, gives lp_r[j] = leaders among records 0 .. j - 1 of rank r, kept in the
//      handle's scratch at the record's own place in the gathered buffer (bit 31: leader), and the
//      group's cell count M = the sum of the ranks' leader counts.  The group reserves M points.
//   2. a leader's cell index = the number of distinct keys below its key = sum over the ranks s of the
//      leaders among the records of s below that key = sum_s lp_s[lower_bound_s(key)] (lp_r[j] for its
//      own rank); on the way it adds the equal-key records of the ranks after it (at most world - 1)
//      and writes the cell's point.
// No LDS staging of the lists: a group's size is bounded by the slots only.
#include <algorithm>

#include "rpl_device.hpp"
#include "rpl_launch.hpp"
#include "rpl_cells.hpp"

namespace rpl {

using cells::u64;
constexpr uint32_t kLeaderBit = 0x80000000u;

__global__ __launch_bounds__(kBlock) void k_merge_cells(
    const rplgpu_cell_t *__restrict__ all, u64 slot_cells, const uint32_t *__restrict__ meta_all,
    uint32_t meta_words, uint32_t world, uint32_t n_groups, double unit, float4 *__restrict__ arena,
    u64 capacity, u64 *__restrict__ cursor, u64 *__restrict__ group_start,
    uint32_t *__restrict__ n_points, uint32_t *__restrict__ status, uint32_t *__restrict__ lp) {
  __shared__ u64 s_first[cells::kMaxWorld];  // rank r's records of the group: all + s_first[r] ...
  __shared__ uint32_t s_n[cells::kMaxWorld];  // ... s_n[r] of them (a group fits 32 bits: lp words)
  __shared__ uint32_t s_lead[cells::kMaxWorld];  // leaders among them
  __shared__ uint32_t s_tmp[kWaves + 1];
  __shared__ u64 s_at;
  __shared__ uint32_t s_cut;
  for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    if (threadIdx.x == 0) s_cut = 0u;
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < world; r += kBlock) {
      const uint32_t *m = meta_all + (size_t)r * meta_words;
      u64 st, n;
      cells::group_extent(m, g, n_groups, slot_cells, &st, &n);
      s_first[r] = (u64)r * slot_cells + st;
      s_n[r] = (uint32_t)(n < 0x7FFFFFFFull ? n : 0x7FFFFFFFull);
      if (cells::group_cut(m, g)) atomicOr(&s_cut, 1u);
    }
    __syncthreads();
    // ---- pass 1: leaders and the per-rank leader prefixes ----
    uint32_t M = 0u;  // (block-uniform)
    for (uint32_t r = 0; r < world; ++r) {
      const rplgpu_cell_t *L = all + s_first[r];
      const uint32_t n = s_n[r];
      uint32_t carry = 0u;
      for (uint32_t base = 0; base < n; base += kBlock) {
        const uint32_t j = base + threadIdx.x;
        uint32_t lead = 0u;
        if (j < n) {
          const uint32_t key = L[j].key;
          lead = 1u;
          for (uint32_t s = 0; s < r; ++s) {
            const rplgpu_cell_t *S = all + s_first[s];
            const u64 p = cells::lower_bound(S, s_n[s], key);
            if (p < s_n[s] && S[p].key == key) { lead = 0u; break; }
          }
        }
        uint32_t tot;
        const uint32_t ex = block_excl_scan(lead, s_tmp, &tot);
        if (j < n) lp[s_first[r] + j] = (carry + ex) | (lead ? kLeaderBit : 0u);
        carry += tot;
        __syncthreads();  // (s_tmp is reused by the next scan)
      }
      if (threadIdx.x == 0) s_lead[r] = carry;
      M += carry;
    }
    if (threadIdx.x == 0) {
      const u64 at = atomicAdd(cursor, (u64)M);
      const u64 room = at >= capacity ? 0ull : capacity - at;
      const uint32_t kept = (uint32_t)(M < room ? M : room);
      group_start[g] = at;
      n_points[g] = kept;
      if (status) status[g] = (s_cut || kept < M) ? RPLGPU_SCAN_OUT_TRUNCATED : 0u;
      s_at = at;
    }
    __syncthreads();  // (also publishes pass 1's lp words to the whole workgroup)
    const u64 at = s_at;
    const u64 room = at >= capacity ? 0ull : capacity - at;
    // ---- pass 2: every leader sums its key and writes its cell ----
    for (uint32_t r = 0; r < world; ++r) {
      const rplgpu_cell_t *L = all + s_first[r];
      const uint32_t n = s_n[r];
      for (uint32_t j = threadIdx.x; j < n; j += kBlock) {
        const uint32_t w = lp[s_first[r] + j];
        if (!(w & kLeaderBit)) continue;
        const rplgpu_cell_t c = L[j];
        u64 idx = w & ~kLeaderBit;
        uint32_t cnt = c.count, isum = c.isum;
        double sx = c.sx, sy = c.sy;
        for (uint32_t s = 0; s < world; ++s) {
          if (s == r) continue;
          const rplgpu_cell_t *S = all + s_first[s];
          const uint32_t ns = s_n[s];
          const u64 p = cells::lower_bound(S, ns, c.key);
          idx += p < ns ? (lp[s_first[s] + p] & ~kLeaderBit) : s_lead[s];
          if (s > r && p < ns && S[p].key == c.key) {  // (ranks before r do not hold the key)
            const rplgpu_cell_t e = S[p];
            cnt += e.count;
            isum += e.isum;
            sx += e.sx;
            sy += e.sy;
          }
        }
        if (idx < room) {
          float v[4];
          cells::cell_point(cnt, isum, sx, sy, unit, v);
          arena[at + idx] = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
    __syncthreads();  // (the LDS tables are rewritten for the next group)
  }
}

hipError_t launch_merge_cells(hipStream_t s, const void *cells_all, unsigned long long slot_cells,
                              const uint32_t *meta_all, uint32_t meta_words, uint32_t world,
                              uint32_t n_groups, double unit, float *arena,
                              unsigned long long capacity, unsigned long long *cursor,
                              unsigned long long *group_start, uint32_t *n_points, uint32_t *status,
                              uint32_t *scratch, uint32_t n_cu) {
  if (n_groups == 0 || world == 0 || world > cells::kMaxWorld) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>(n_groups, 2u * (n_cu ? n_cu : 256u));
  hipLaunchKernelGGL(k_merge_cells, dim3(grid), dim3(kBlock), 0, s,
                     (const rplgpu_cell_t *)cells_all, slot_cells, meta_all, meta_words, world, n_groups,
                     unit, (float4 *)arena, capacity, cursor, group_start, n_points, status, scratch);
  return hipGetLastError();
}

}  // namespace rpl
