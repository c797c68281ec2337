// rpl_rules.hpp — the small rules that the doors (rplgpu_pose_stages.hip, rplgpu_scan_stages.hip), the kernel
// launchers (rpl_launch.hpp) and the plain C++ rules units (rplgpu_pose_rules.cpp, rplgpu_wide_rules.cpp) share.  No
// HIP header and no attribute of one: a plain C++ compiler reads this file as it stands, given the include path of
// the two public C headers (every unit that includes this file is built with it).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace rpl {

// the words of a bit map of nb bins (nb <= RPLGPU_MAX_POSE_BINS), on the device and on the host, for E20 and E21
// (constexpr: callable from device code without an attribute)
constexpr uint32_t bin_map_words(uint32_t nb) { return (nb + 31u) >> 5; }

// the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool ranges_overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

// the RPLGPU_NAV_TILE-cell tiles of a width x height grid, a workgroup each in E26's rounds and E29's labelling;
// false: G grids of them are no launch (none, or above RPLGPU_NAV_MAX_TILES)
inline bool nav_tiles(uint32_t width, uint32_t height, uint64_t G, uint32_t *tiles_x, uint32_t *tiles_y) {
  *tiles_x = (width + RPLGPU_NAV_TILE - 1u) / RPLGPU_NAV_TILE;
  *tiles_y = (height + RPLGPU_NAV_TILE - 1u) / RPLGPU_NAV_TILE;
  const uint64_t all = G * *tiles_x * *tiles_y;  // (G below 2^32, a side at most RPLGPU_MAX_OCC_DIM: no carry)
  return all != 0 && all <= RPLGPU_NAV_MAX_TILES;
}

// E26's weight of a costmap byte v (as int8), 0: impassable; on the device and on the host, as bin_map_words.  Spec:
// the public rplgpu_nav_field_t or the kernels' copy of it, by reference (by value the fields cost k_nav_relax its
// instruction count: DESIGN.md, the planner stages' shared pieces)
template <class Spec>
constexpr uint32_t nav_byte_weight(const Spec &s, int v) {
  if (v < 0) return s.unknown_cost;
  if ((uint32_t)v >= s.lethal) return 0u;
  return s.neutral + s.factor * (uint32_t)v;
}

// the check of a match spec, E13's (rplgpu_scan_match_t) and E24's (rplgpu_wide_match_t, which adds its own
// max_blocks test): the two structs begin with the same fields and differ in the shift they allow
#define RPL_SAME_FIELD(f)                                                                                  \
  static_assert(offsetof(rplgpu_scan_match_t, f) == offsetof(rplgpu_wide_match_t, f) &&                     \
                    sizeof(rplgpu_scan_match_t::f) == sizeof(rplgpu_wide_match_t::f),                         \
                "rplgpu_scan_match_t and rplgpu_wide_match_t begin with the same fields: " #f)
RPL_SAME_FIELD(origin_x); RPL_SAME_FIELD(origin_y); RPL_SAME_FIELD(resolution); RPL_SAME_FIELD(width);
RPL_SAME_FIELD(height); RPL_SAME_FIELD(shift_x); RPL_SAME_FIELD(shift_y); RPL_SAME_FIELD(rot_steps);
RPL_SAME_FIELD(rot_step);
#undef RPL_SAME_FIELD
template <class Spec>
inline int32_t match_spec_check(const Spec *m, uint32_t max_shift) {
  if (!m) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(m->origin_x) || !std::isfinite(m->origin_y) || !std::isfinite(m->resolution) ||
      !std::isfinite(m->rot_step))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(m->resolution > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (m->width == 0 || m->width > RPLGPU_MAX_OCC_DIM || m->height == 0 || m->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (m->shift_x > max_shift || m->shift_y > max_shift || m->rot_steps > RPLGPU_MAX_MATCH_ROT)
    return RPLGPU_ERR_INVALID_ARG;
  if (m->rot_steps > 0 && (!(m->rot_step > 0.0f) || (double)m->rot_steps * (double)m->rot_step > M_PI / 2.0))
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

}  // namespace rpl
