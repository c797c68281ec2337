// rpl_mppi.hpp — E28 (include/rplgpu_msg.h, rplgpu_mppi_update_dev / rplgpu_mppi_spread_dev): what rpl_mppi.hip (the
// kernels), rplgpu_mppi_stages.hip (the doors) and rplgpu_mppi_rules.cpp (the rules, plain C++: this header names
// nothing of HIP unless a HIP unit includes it) share.  An update is three launches on one stream and nothing on the
// handle: weights (a thread per candidate, a record of eight words per workgroup), sums (lanes laid out step-fastest
// over the [k][t] entries, a lane folds RPLGPU_MPPI_PER_LANE candidates of its step in registers, a record of twelve
// words per workgroup and step) and close (a workgroup per group folds both kinds of record and does the finish).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif
#include <cstdint>

#include "rplgpu_msg.h"

namespace rpl {

constexpr uint32_t kMpBlock = 256u;

// how the sums launch and the close lay a workgroup over (step, candidate): tw lanes of steps (the power of two at or
// above T_e), kMpBlock / tw rows of candidates; a workgroup takes rows * RPLGPU_MPPI_PER_LANE candidates
struct MppiLayout {
  uint32_t tw_log, rows, per_block, chunks, w_blocks;
  uint64_t w_words, words;  // the weight records come first, then the sums records; both multiples of 4
};

// false: the shape is refused (K T_e above 2^24 included); *capacity says whether only a launch's size refuses it
inline bool mppi_layout(uint32_t G, uint32_t K, uint32_t T_e, MppiLayout *l, bool *capacity = nullptr) {
  if (capacity) *capacity = false;
  if (G == 0 || G > 65535u || K == 0 || K > RPLGPU_MAX_POSES || T_e == 0 || T_e > RPLGPU_ROLLOUT_MAX_STEPS ||
      (uint64_t)K * T_e > (1ull << 24))
    return false;
  uint32_t tw_log = 0;
  while ((1u << tw_log) < T_e) ++tw_log;  // <= 8
  l->tw_log = tw_log;
  l->rows = kMpBlock >> tw_log;
  l->per_block = l->rows * RPLGPU_MPPI_PER_LANE;
  l->chunks = (K + l->per_block - 1u) / l->per_block;
  l->w_blocks = (K + kMpBlock - 1u) / kMpBlock;
  if ((uint64_t)l->chunks * G > RPLGPU_MPPI_MAX_BLOCKS || (uint64_t)l->w_blocks * G > RPLGPU_MPPI_MAX_BLOCKS) {
    if (capacity) *capacity = true;
    return false;
  }
  l->w_words = 8ull * l->w_blocks * G;
  l->words = l->w_words + 12ull * l->chunks * T_e * G;
  return true;
}

#ifdef __HIP__
struct MppiK {  // a checked rplgpu_mppi_t
  float xy_scale;
  uint32_t shift, table_len, steps_e;  // steps_e: T_e
};

hipError_t launch_mppi_update(hipStream_t s, const MppiK &k, const uint32_t *out, unsigned long long out_stride,
                              const uint32_t *rollout_result, const float *delta, unsigned long long delta_stride,
                              uint32_t delta_per_group, const uint16_t *table, const float *nominal,
                              unsigned long long nominal_stride, uint32_t nominal_per_group, uint32_t G, uint32_t K,
                              uint32_t *weights, unsigned long long weight_stride, uint32_t *sums,
                              unsigned long long sums_stride, float *nominal_out,
                              unsigned long long nominal_out_stride, uint32_t *result, uint32_t *scratch);

hipError_t launch_mppi_spread(hipStream_t s, const float *nominal, unsigned long long nominal_stride,
                              uint32_t nominal_per_group, uint32_t T_n, const float *noise,
                              unsigned long long noise_stride, uint32_t noise_per_group, uint32_t G, uint32_t K,
                              uint32_t T, uint32_t shift, uint32_t keep_first, float *out,
                              unsigned long long out_stride);
#endif

}  // namespace rpl
