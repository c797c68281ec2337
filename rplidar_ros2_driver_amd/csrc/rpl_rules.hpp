// rpl_rules.hpp — the two small rules that the pose-list doors (rplgpu_pose_stages.hip), the kernel launchers
// (rpl_launch.hpp) and the plain C++ rules unit (rplgpu_pose_rules.cpp) share.  No HIP header and no attribute of
// one: a plain C++ compiler reads this file as it stands.
#pragma once
#include <cstdint>

namespace rpl {

// the words of a bit map of nb bins (nb <= RPLGPU_MAX_POSE_BINS), on the device and on the host, for E20 and E21
// (constexpr: callable from device code without an attribute)
constexpr uint32_t bin_map_words(uint32_t nb) { return (nb + 31u) >> 5; }

// the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool ranges_overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace rpl
