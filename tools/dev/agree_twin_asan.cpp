// tools/dev/agree_twin_asan.cpp — E23's host twin (rplgpu_beam_agree_points_host) and spec check under the host
// sanitizers, a stand-alone program: every buffer is a heap block of exactly the size the header names, so a word
// written or read beside one is reported.  Host code only; it makes no device call and needs no device.
//
//   cd rplidar_ros2_driver_amd/csrc && make          (the other units' objects)
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -I../../include -I. \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -c rplgpu_pose_stages.hip -o /tmp/pose_stages_san.o
//   /opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -I../../include -c ../../tools/dev/agree_twin_asan.cpp -o /tmp/agree_twin_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/agree_twin_main.o /tmp/pose_stages_san.o \
//         $(ls ../../build/obj/*.o | grep -v rplgpu_pose_stages) -ldl -o /tmp/agree_twin_asan
//   /tmp/agree_twin_asan        (prints "agree twin: ... ok" and exits 0)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"

namespace {

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}
float unit() { return (float)(rnd() >> 8) / 16777216.0f; }

template <class T>
T *block(size_t n) {
  return static_cast<T *>(std::malloc(n ? n * sizeof(T) : 1));
}

int run(uint32_t n_scans, uint32_t n_stride, uint32_t P, uint32_t W, uint32_t H, uint32_t err_num, bool odd_values) {
  rplgpu_beam_agree_t s;
  rplgpu_default_beam_agree(&s);
  s.origin_x = -1.0f;
  s.origin_y = -0.5f;
  s.resolution = 0.25f;
  s.width = W;
  s.height = H;
  s.agree_lo = 50;
  s.err_num = err_num;
  if (rplgpu_beam_agree_check(&s) != RPLGPU_OK) return 1;
  const uint32_t words = (n_stride + 31u) / 32u;
  // every second sample of every scan is a point, and always the last one of the stride
  std::vector<uint32_t> sl, ix;
  for (uint32_t b = 0; b < n_scans; ++b)
    for (uint32_t i = 0; i < n_stride; ++i)
      if ((i & 1u) == 0 || i + 1u == n_stride) {
        sl.push_back(b);
        ix.push_back(i);
      }
  const uint32_t m = (uint32_t)sl.size();
  float *x = block<float>(m), *y = block<float>(m), *poses = block<float>(4u * P);
  uint32_t *slot = block<uint32_t>(m), *index = block<uint32_t>(m);
  int8_t *field = block<int8_t>((size_t)W * H);
  uint32_t *counts = block<uint32_t>((size_t)n_scans * n_stride), *mask = block<uint32_t>((size_t)n_scans * words);
  uint32_t *weights = block<uint32_t>(P), *result = block<uint32_t>(8), *agree = block<uint32_t>(8);
  std::memcpy(slot, sl.data(), 4u * m);
  std::memcpy(index, ix.data(), 4u * m);
  for (uint32_t k = 0; k < m; ++k) {
    x[k] = -2.0f + unit() * (0.25f * W + 2.0f);
    y[k] = -1.5f + unit() * (0.25f * H + 2.0f);
  }
  for (size_t c = 0; c < (size_t)W * H; ++c) field[c] = (int8_t)(rnd() & 0xFFu);
  for (uint32_t q = 0; q < P; ++q) {
    const float th = unit() * 6.2831853f;
    poses[4u * q] = std::cos(th);
    poses[4u * q + 1u] = std::sin(th);
    poses[4u * q + 2u] = unit() - 0.5f;
    poses[4u * q + 3u] = unit() - 0.5f;
  }
  const bool odd = odd_values && m > 3 && P > 2;
  if (odd) {  // points and poses the rule defines without a cell
    x[1] = std::numeric_limits<float>::quiet_NaN();
    y[2] = std::numeric_limits<float>::infinity();
    x[3] = 3.0e38f;
    poses[2] = std::numeric_limits<float>::quiet_NaN();
    poses[4u * 1u + 3u] = -std::numeric_limits<float>::infinity();
    poses[4u * 2u + 2u] = 1.0e30f;
  }
  uint32_t status = 99;
  const int32_t rc = rplgpu_beam_agree_points_host(x, y, slot, index, m, n_scans, n_stride, poses, P, field, &s, counts,
                                                   mask, weights, result, agree, &status);
  int bad = rc != RPLGPU_OK;
  uint64_t total = 0;
  uint32_t bits = 0;
  for (size_t c = 0; c < (size_t)n_scans * n_stride; ++c) total += counts[c];
  for (size_t c = 0; c < (size_t)n_scans * words; ++c) bits += (uint32_t)__builtin_popcount(mask[c]);
  bad |= total != ((uint64_t)agree[6] | ((uint64_t)agree[7] << 32)) || bits != agree[1] || agree[0] != result[4] ||
         agree[1] > agree[0] || agree[3] != (agree[2] ? agree[0] : agree[1]) || (odd && status == 0);
  if (err_num == 0) bad |= agree[0] != 0 && agree[2] != 1;
  // the refusals write nothing and read nothing beside the blocks
  uint32_t far_slot = n_scans, keep = counts[0];
  bad |= rplgpu_beam_agree_points_host(x, y, &far_slot, index, 1, n_scans, n_stride, poses, P, field, &s, counts, mask,
                                       weights, result, agree, nullptr) != RPLGPU_ERR_INVALID_ARG;
  bad |= rplgpu_beam_agree_points_host(x, y, slot, index, m, n_scans, n_stride, poses, 0, field, &s, counts, mask,
                                       weights, result, agree, nullptr) != RPLGPU_ERR_INVALID_ARG;
  bad |= rplgpu_beam_agree_points_host(nullptr, nullptr, nullptr, nullptr, 0, n_scans, n_stride, poses, P, field,
                                       nullptr, counts, mask, weights, result, agree, nullptr) != RPLGPU_ERR_INVALID_ARG;
  bad |= counts[0] != keep;
  // no points at all: every output written, every word 0 but P zero weights
  bad |= rplgpu_beam_agree_points_host(nullptr, nullptr, nullptr, nullptr, 0, n_scans, n_stride, poses, P, field, &s,
                                       counts, mask, weights, result, agree, &status) != RPLGPU_OK;
  bad |= agree[0] != 0 || agree[2] != 0 || agree[5] != 0 || result[3] != P || status != 0;
  for (void *p : {(void *)x, (void *)y, (void *)poses, (void *)slot, (void *)index, (void *)field, (void *)counts,
                  (void *)mask, (void *)weights, (void *)result, (void *)agree})
    std::free(p);
  return bad;
}

}  // namespace

int main() {
  int bad = 0, runs = 0;
  for (uint32_t n_stride : {1u, 31u, 32u, 33u, 64u, 97u})
    for (uint32_t P : {1u, 3u, 64u})
      for (uint32_t err_num : {0u, 9u, 11u}) {
        bad |= run(1u + n_stride % 3u, n_stride, P, 13, 7, err_num, (runs & 1) != 0);
        ++runs;
      }
  bad |= run(2, 5, 4, 1, 1, 9, false);
  rplgpu_beam_agree_t s;
  rplgpu_default_beam_agree(&s);
  s.keep_den = 0;
  bad |= rplgpu_beam_agree_check(&s) != RPLGPU_ERR_INVALID_ARG || rplgpu_beam_agree_check(nullptr) != RPLGPU_ERR_INVALID_ARG;
  std::printf("agree twin: %d runs under the sanitizers, %s\n", runs + 1, bad ? "WRONG" : "ok");
  return bad ? 1 : 0;
}
