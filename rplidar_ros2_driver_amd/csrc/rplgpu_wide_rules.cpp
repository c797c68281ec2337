// rplgpu_wide_rules.cpp — the rules of E24, the wide-window scan matcher (include/rplgpu_msg.h), in plain C++: the
// defaults, the check, the sizes of the bounds volume and of the scratch, and the pooled field's host twin that the
// device test is held against.  No handle, no stream, no HIP header; built like rplgpu_pose_rules.cpp.  The doors that
// call these are in rplgpu_wide_stages.hip; tools/dev/wide_rules_asan.cpp drives this file alone under the host
// sanitizers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_rules.hpp"

extern "C" {

void rplgpu_default_wide_match(rplgpu_wide_match_t *m) {
  if (!m) return;
  m->origin_x = -25.6f;
  m->origin_y = -25.6f;
  m->resolution = 0.05f;
  m->width = 1024;
  m->height = 1024;
  m->shift_x = 64;
  m->shift_y = 64;
  m->rot_steps = 10;
  m->rot_step = (float)(0.25 * M_PI / 180.0);
  m->max_blocks = 1024;
}

// E13's check (rpl_rules.hpp's match_spec_check) with the wide shift limit, and the cap of the list
int32_t rplgpu_wide_match_check(const rplgpu_wide_match_t *m) {
  const int32_t rc = rpl::match_spec_check(m, RPLGPU_MAX_WIDE_SHIFT);
  if (rc != RPLGPU_OK) return rc;
  if (m->max_blocks == 0 || m->max_blocks > RPLGPU_MAX_WIDE_BLOCKS) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint32_t rplgpu_wide_match_blocks(const rplgpu_wide_match_t *m) {
  if (rplgpu_wide_match_check(m) != RPLGPU_OK) return 0;
  const uint32_t s = RPLGPU_WIDE_MATCH_BLOCK;
  const uint32_t nbx = (2u * m->shift_x + s) / s, nby = (2u * m->shift_y + s) / s;  // ceil((2T + 1) / s)
  return (2u * m->rot_steps + 1u) * nby * nbx;
}

uint64_t rplgpu_wide_match_scratch_words(const rplgpu_wide_match_t *m, uint32_t G) {
  if (rplgpu_wide_match_check(m) != RPLGPU_OK) return 0;
  return (uint64_t)G * (272ull + 65ull * m->max_blocks);
}

// rows, then columns: a sliding maximum of s cells each way over F = max(byte, 0), 0 outside the grid
int32_t rplgpu_pool_field_host(const int8_t *field, uint32_t width, uint32_t height, int8_t *pooled) {
  if (!field || !pooled) return RPLGPU_ERR_INVALID_ARG;
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t s = RPLGPU_WIDE_MATCH_BLOCK, Wp = width + s - 1u, Hp = height + s - 1u;
  std::vector<int8_t> rows((size_t)height * Wp);  // rows[y][px] = max over a of F(px - (s-1) + a, y)
  for (uint32_t y = 0; y < height; ++y)
    for (uint32_t px = 0; px < Wp; ++px) {
      int8_t best = 0;
      for (uint32_t a = 0; a < s; ++a) {
        const int64_t x = (int64_t)px - (int64_t)(s - 1u) + a;
        if (x >= 0 && x < (int64_t)width) best = std::max(best, field[(size_t)y * width + (size_t)x]);
      }
      rows[(size_t)y * Wp + px] = best;
    }
  for (uint32_t py = 0; py < Hp; ++py)
    for (uint32_t px = 0; px < Wp; ++px) {
      int8_t best = 0;
      for (uint32_t b = 0; b < s; ++b) {
        const int64_t y = (int64_t)py - (int64_t)(s - 1u) + b;
        if (y >= 0 && y < (int64_t)height) best = std::max(best, rows[(size_t)y * Wp + px]);
      }
      pooled[(size_t)py * Wp + px] = best;
    }
  return RPLGPU_OK;
}

}  // extern "C"
