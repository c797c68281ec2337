// rpl_agree.hpp — E23 (include/rplgpu_msg.h, rplgpu_score_poses_agree_dev): the launcher of rpl_agree.hip.  The front
// end of its two walking kernels is rpl_front.hpp's front_point_pass, the one k_pose_score (rpl_pose.hip) calls, with
// its three options on: the sample index kept beside every list entry, the finite bits of a wave's 128 samples stored
// as four mask words, and a second keep test against the rule's mask (the apply pass lists only the skipped samples).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rpl_launch.hpp"

namespace rpl {

struct AgreeK {  // a checked rplgpu_beam_agree_t
  float origin_x, origin_y, resolution;
  uint32_t width, height;
  uint32_t agree_lo;
  uint32_t keep_num, keep_den, err_num, err_den;
};

// E23, five kernels on the stream between the scan prologue and launch_pose_best: prepare (every output word
// zeroed, the smallest count started at ~0), count (E15's sums and the per-sample counts from one field load, the
// finite bits, result word 4), decide (the rule bit per sample ANDed into the mask, F, K, the largest, smallest and
// summed count), flag (agree words 2, 3 and 5), apply (the skipped samples' sums taken off the weights again, unless
// the group fell back).  counts: count_stride >= n_stride words per scan; mask: mask_words_stride >=
// ceil(n_stride / 32) words per scan; agree: eight words per group.
hipError_t launch_agree(hipStream_t s, const void *nodes, uint32_t n_stride, const uint32_t *n_per_scan, uint32_t B,
                        uint32_t group, uint32_t G, const KParams &p, const Tables &T, const uint32_t *keepmask,
                        uint32_t mask_stride, const float *motion, const float *pose2d, const AgreeK &k,
                        const float *poses, uint32_t P, unsigned long long pose_stride, uint32_t poses_per_group,
                        const int8_t *field, unsigned long long field_stride, uint32_t field_per_group,
                        uint32_t *weights, unsigned long long weight_stride, uint32_t *result, uint32_t *status,
                        uint32_t *counts, unsigned long long count_stride, uint32_t *mask,
                        unsigned long long mask_words_stride, uint32_t *agree);

}  // namespace rpl
