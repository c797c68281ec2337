// rpl_refine.hpp — E25 (include/rplgpu_msg.h, rplgpu_refine_poses_dev): what rpl_refine.hip (the kernels) and
// rplgpu_refine_stages.hip (the doors) share.  A round of sums is four launches on the stream and nothing on the
// handle: prepare zeroes the scratch planes and the result words, sums walks the points (the shared front end, rpl_front.hpp)
// and leaves through 64-bit integer atomics onto the planes, finish normalises the carries into the 32 words of a
// pose, best makes result words 4 - 6.  The step is one launch more; the two joining kernels are one launch each.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rpl_launch.hpp"

namespace rpl {

struct RefineK {  // a checked rplgpu_pose_refine_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  uint32_t target;
  float damping, max_step_cells, max_rot;
  uint32_t min_points;
};

// scratch: 2 * RPLGPU_REFINE_PLANES * G * P words, plane k of group g at 64-bit word (g * planes + k) * P + q
hipError_t launch_refine_prepare(hipStream_t s, uint32_t G, uint32_t P, uint32_t *scratch, uint32_t *result);
hipError_t launch_refine_sums(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
                              uint32_t B, uint32_t group, const KParams &p, const Tables &T, const uint32_t *keepmask,
                              uint32_t mask_stride, const float *motion, const float *pose2d, const RefineK &k,
                              const float *poses, uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group,
                              const int8_t *field, unsigned long long field_stride, uint32_t field_per_group,
                              uint32_t *scratch, uint32_t *result, uint32_t *status);
// finish and best: the planes into d_sums, then result words 4 - 6
hipError_t launch_refine_finish(hipStream_t s, uint32_t G, uint32_t P, const uint32_t *scratch, uint32_t *sums,
                                unsigned long long sums_stride, uint32_t *result);
// zero_result: result words 0 - 3 are zeroed on the stream first (the step called apart from the sums)
hipError_t launch_refine_step(hipStream_t s, const uint32_t *sums, unsigned long long sums_stride, const RefineK &k,
                              const float *poses, unsigned long long pose_stride, uint32_t poses_per_group, uint32_t G,
                              uint32_t P, float *poses_out, unsigned long long out_stride, uint32_t *step,
                              unsigned long long step_stride, uint32_t *result, bool zero_result);
hipError_t launch_match_poses(hipStream_t s, const uint32_t *best, const MatchK &k, const MatchRot &rot,
                              const float *pivot, const float *prior, uint32_t G, float *poses_out,
                              unsigned long long out_stride);
hipError_t launch_compose_poses(hipStream_t s, const float *poses, unsigned long long pose_stride,
                                uint32_t poses_per_group, uint32_t P, const uint32_t *result, uint32_t q,
                                const float *pose_in, uint32_t B, uint32_t group, float *pose_out);

}  // namespace rpl
