// rpl_unionfind.hpp — the lock-free union-find of E21 (rpl_clusters.hip: k_cl_link, k_cl_flatten) and E29
// (rpl_frontier.hip: k_fr_tile in LDS; k_fr_seam and k_fr_flatten on the parent plane).  Device code only.
//
// THE DISCIPLINE.  Nodes are 0 .. limit - 1 and parent[x] <= x always: a root is its own parent, and the only write
// that joins two trees is the HOOK, a compare-exchange that puts the larger ROOT under the smaller and that only a
// node which still is a root passes.  So the trees never hold a cycle, and the final root of a component is its
// smallest node whatever the timing.  Every access to parent[] is a relaxed atomic of the policy's scope (agent for
// global memory, so no XCD works on a stale line; workgroup for LDS), and every value read is clamped below `limit`.
//   find   parents strictly decrease, so a walk ends within `bound` steps; at the bound the policy's flag is raised
//          and the walk leaves where it stands.  With kShorten a node found two steps below its grandparent is hung
//          under it (atomicMin: a pointer only ever moves to a smaller node of the SAME tree — only roots are ever
//          hooked to another tree — so every node keeps reaching its tree's root and the later walks are short).
//   unite  at most 2 bound + 2 rounds: a round that does not end the loop replaces the larger of (a, b) by a smaller
//          value and never raises the other.  A failed hook (the root was hooked by somebody else in between, and
//          nothing was written) goes on from the value the atomic returned.
//
// A POLICY names what differs between the call sites:
//   static uint32_t load(const uint32_t *p)   the relaxed atomic load of its scope
//   static constexpr bool kShorten            whether find takes the grandparent step
//   uint32_t limit, bound                     values read are clamped below limit; the step bound
//   void overrun() const                      what a loop that reaches its bound does (a flag in a header, a local one)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rpl {

// parent[] in global memory, the flag a bit of a header word
struct UfGlobal {
  uint32_t limit, bound;
  uint32_t *flag_word;
  uint32_t flag_bit;
  static constexpr bool kShorten = true;
  static __device__ __forceinline__ uint32_t load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void overrun() const { atomicOr(flag_word, flag_bit); }
};

// parent[] in LDS, one workgroup's: walks are short (a tile), so no grandparent step; the flag is the thread's own
struct UfLds {
  uint32_t limit, bound;
  uint32_t *flag;
  static constexpr bool kShorten = false;
  static __device__ __forceinline__ uint32_t load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void overrun() const { *flag = 1u; }
};

template <class Policy>
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x, const Policy &pol) {
  for (uint32_t step = 0;; ++step) {  // bound: pol.bound steps (x strictly decreases)
    const uint32_t p = min(Policy::load(parent + x), pol.limit - 1u);
    if (p >= x) return x;  // (p == x: a root; p > x cannot be, and would end the walk as well)
    if (Policy::kShorten) {
      const uint32_t gp = min(Policy::load(parent + p), pol.limit - 1u);
      if (gp >= p) return p;
      if (step >= pol.bound) {
        pol.overrun();
        return x;
      }
      atomicMin(parent + x, gp);
      x = gp;
    } else {
      if (step >= pol.bound) {
        pol.overrun();
        return x;
      }
      x = p;
    }
  }
}

template <class Policy>
__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t a, uint32_t b, const Policy &pol) {
  for (uint32_t round = 0;; ++round) {  // bound: 2 pol.bound + 2 rounds
    a = uf_find(parent, a, pol);
    b = uf_find(parent, b, pol);
    if (a == b) return;
    if (round >= 2u * pol.bound + 2u) {
      pol.overrun();
      return;
    }
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = min(atomicCAS(parent + hi, hi, lo), pol.limit - 1u);
    if (old == hi) return;  // hi was still a root and now hangs under lo
    a = old;                // somebody hooked hi under old < hi in between: go on from there
    b = lo;
  }
}

}  // namespace rpl
