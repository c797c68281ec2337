// rpl_philox.hpp — Philox4x32-10, the counter-based generator of E18 (rpl_motion.hip) and E19 (rpl_seed.hip), by the
// rule of include/rplgpu_msg.h (the E18 block): ten rounds on the counter (c0, c1, c2, c3) under the key (k0, k1), the
// key incremented before rounds 2 .. 10.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rpl {

constexpr uint32_t kPhiloxMul0 = 0xD2511F53u, kPhiloxMul1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxKey0 = 0x9E3779B9u, kPhiloxKey1 = 0xBB67AE85u;
constexpr int kPhiloxRounds = 10;

struct Philox4 {
  uint32_t w0, w1, w2, w3;  // the four output words
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < kPhiloxRounds; ++r) {
    if (r) {
      k0 += kPhiloxKey0;
      k1 += kPhiloxKey1;
    }
    const uint32_t h0 = __umulhi(kPhiloxMul0, c0), l0 = kPhiloxMul0 * c0;
    const uint32_t h1 = __umulhi(kPhiloxMul1, c2), l1 = kPhiloxMul1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
  }
  Philox4 out;
  out.w0 = c0;
  out.w1 = c1;
  out.w2 = c2;
  out.w3 = c3;
  return out;
}

}  // namespace rpl
