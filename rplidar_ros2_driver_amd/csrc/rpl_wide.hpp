// rpl_wide.hpp — E24: what rpl_wide.hip (the kernels) and rplgpu_wide_stages.hip (the doors) share.  The pooled field
// is a launch of its own; a match is seven launches on the stream and nothing on the handle: prepare zeroes the
// bounds volumes, the result and work words and the head of every group's scratch, bound adds the pooled values
// under the points into the bounds (and the finite points into result word 4), seed picks the two seeds, refine
// (seeds = 1) scores them, list finds b0, counts the blocks with U >= b0 and lists them when they fit the cap, refine
// (seeds = 0) scores the listed blocks, best applies E13's tie rule.  The two refine launches have the same fixed
// grid: the list's length never leaves the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rpl_launch.hpp"

namespace rpl {

struct WideK {  // a checked rplgpu_wide_match_t: k.tx, k.ty up to RPLGPU_MAX_WIDE_SHIFT
  MatchK k;
  uint32_t nbx, nby;  // blocks per axis, ceil((2T + 1) / RPLGPU_WIDE_MATCH_BLOCK)
  uint32_t max_blocks;
};
uint32_t wide_blocks(const WideK &wk);                   // the words of one group's bounds volume
unsigned long long wide_scratch_words(const WideK &wk);  // the words of one group's scratch
hipError_t launch_pool_field(hipStream_t s, const int8_t *field, unsigned long long field_stride, uint32_t F,
                             uint32_t width, uint32_t height, int8_t *pooled, unsigned long long pooled_stride);
hipError_t launch_wide_prepare(hipStream_t s, uint32_t *bounds, unsigned long long bounds_stride, uint32_t G,
                               const WideK &wk, uint32_t *scratch, uint32_t *best, uint32_t *work);
hipError_t launch_wide_bound(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                             uint32_t B, uint32_t group, const KParams &p, const Tables &T, const uint32_t *keepmask,
                             uint32_t mask_stride, const float *motion, const float *pose2d, const float *pivot,
                             const WideK &wk, const MatchRot &rot, const int8_t *pooled,
                             unsigned long long pooled_stride, uint32_t field_per_group, uint32_t *bounds,
                             unsigned long long bounds_stride, uint32_t *best, uint32_t *status);
hipError_t launch_wide_seed(hipStream_t s, const uint32_t *bounds, unsigned long long bounds_stride, uint32_t G,
                            const WideK &wk, uint32_t *scratch, uint32_t *work);
hipError_t launch_wide_refine(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                              uint32_t B, uint32_t group, const KParams &p, const Tables &T, const uint32_t *keepmask,
                              uint32_t mask_stride, const float *motion, const float *pose2d, const float *pivot,
                              const WideK &wk, const MatchRot &rot, const int8_t *field,
                              unsigned long long field_stride, uint32_t field_per_group, uint32_t *scratch,
                              uint32_t seeds);
hipError_t launch_wide_list(hipStream_t s, const uint32_t *bounds, unsigned long long bounds_stride, uint32_t G,
                            const WideK &wk, uint32_t *scratch, uint32_t *work);
hipError_t launch_wide_best(hipStream_t s, uint32_t G, const WideK &wk, const uint32_t *scratch, uint32_t *best);

}  // namespace rpl
