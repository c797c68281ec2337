// rplgpu_mppi_stages.hip — the extern "C" entry points of E28, rolled-out candidates weighed and blended into new
// controls (include/rplgpu_msg.h): rplgpu_mppi_update_dev, rplgpu_mppi_spread_dev and the host-buffer doors
// rplgpu_mppi_update and rplgpu_mppi_spread.
//
// Host side only: argument checks, the launches and the doors; the kernels are in rpl_mppi.hip, the spec's rules and
// the host twins in rplgpu_mppi_rules.cpp.  The handle and the doors' per-call buffer come from rpl_host.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_rules.hpp"
#include "rpl_mppi.hpp"

using namespace rpl::host;

namespace {

// K and the steps of an update, which the call and its door take alike
bool update_counts_ok(rplgpu_ctx *h, const char *fn, uint32_t K, uint32_t T) {
  return (K != 0 && K <= RPLGPU_MAX_POSES && (uint64_t)K * T <= (1ull << 24)) ||
         refuse(h, fn, "K must be in 1 .. RPLGPU_MAX_POSES with K * steps <= 2^24");
}

// K, T, T_n and the shift of a spread, likewise
bool spread_counts_ok(rplgpu_ctx *h, const char *fn, uint32_t K, uint32_t T, uint32_t T_n, uint32_t shift) {
  return (K != 0 && K <= RPLGPU_MAX_POSES && T != 0 && T <= RPLGPU_ROLLOUT_MAX_STEPS && T_n != 0 &&
          T_n <= RPLGPU_ROLLOUT_MAX_STEPS && (uint64_t)K * T <= (1ull << 24) &&
          shift <= RPLGPU_MPPI_MAX_SPREAD_SHIFT) ||
         refuse(h, fn, "K must be in 1 .. RPLGPU_MAX_POSES, T and T_n in 1 .. RPLGPU_ROLLOUT_MAX_STEPS with K * T <= "
                       "2^24, shift at most RPLGPU_MPPI_MAX_SPREAD_SHIFT");
}

}  // namespace

extern "C" {

int32_t rplgpu_mppi_update_dev(rplgpu_handle_t h, const rplgpu_mppi_t *m, const uint32_t *d_out, uint64_t out_stride,
                               const uint32_t *d_rollout_result, const float *d_delta, uint64_t delta_stride,
                               uint32_t delta_per_group, const uint16_t *d_table, const float *d_nominal,
                               uint64_t nominal_stride, uint32_t nominal_per_group, uint32_t G, uint32_t K,
                               uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_sums, uint64_t sums_stride,
                               float *d_nominal_out, uint64_t nominal_out_stride, uint32_t *d_result,
                               uint32_t *d_scratch) {
  const char *fn = "rplgpu_mppi_update_dev";
  const std::string at = std::string(fn) + ": ";
  if (!h || !m) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_mppi_check(m) != RPLGPU_OK) return refuse_spec(h, fn, "rplgpu_mppi_t");
  const PoseListDoor door{h, fn};
  const uint32_t T = m->steps, T_e = m->delta_per_step ? T : 1u;
  if (!door.groups(G) || !update_counts_ok(h, fn, K, T)) return RPLGPU_ERR_INVALID_ARG;
  if (!d_out || !d_rollout_result || !d_delta || !d_table || !d_weights || !d_sums || !d_nominal_out || !d_result ||
      !d_scratch || misaligned(d_out, 15u) || misaligned(d_delta, 15u) || misaligned(d_nominal, 15u) ||
      misaligned(d_sums, 15u) || misaligned(d_nominal_out, 15u) || misaligned(d_scratch, 15u) ||
      misaligned(d_table, 1u) || misaligned(d_rollout_result, 3u) || misaligned(d_weights, 3u) ||
      misaligned(d_result, 3u)) {
    h->err = at + "a required pointer is missing or a pointer is misaligned (16 bytes: d_out, d_delta, d_nominal, "
                  "d_sums, d_nominal_out, d_scratch; 2: d_table; 4: the others)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t n_delta = (uint64_t)K * T_e;
  if (out_stride < 8ull * K || (out_stride & 3u) || delta_stride < 4ull * n_delta || (delta_stride & 3u) ||
      (d_nominal && (nominal_stride < 4ull * T_e || (nominal_stride & 3u))) || weight_stride < K ||
      sums_stride < 8ull * T_e || (sums_stride & 3u) || nominal_out_stride < 4ull * T_e ||
      (nominal_out_stride & 3u)) {
    h->err = at + "out_stride >= 8 K, delta_stride >= 4 K T_e, nominal_stride and nominal_out_stride >= 4 T_e, "
                  "sums_stride >= 8 T_e (all multiples of 4) and weight_stride >= K are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  rpl::MppiLayout l;
  bool capacity = false;
  if (!rpl::mppi_layout(G, K, T_e, &l, &capacity)) {
    h->err = at + (capacity ? "a launch above RPLGPU_MPPI_MAX_BLOCKS workgroups"
                            : "G, K or the steps are out of range (see include/rplgpu_msg.h)");
    return capacity ? RPLGPU_ERR_CAPACITY : RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t last = G - 1u, noms = nominal_per_group ? last : 0ull;
  const bool in_place = d_nominal && d_nominal_out == d_nominal && nominal_out_stride == nominal_stride &&
                        (nominal_per_group || G == 1u);
  const Range ranges[] = {
      {d_out, 4ull * (last * out_stride + 8ull * K), false},
      {d_rollout_result, 32ull * G, false},
      {d_delta, 4ull * ((delta_per_group ? last * delta_stride : 0ull) + 4ull * n_delta), false},
      {d_table, 2ull * m->table_len, false},
      {d_nominal, d_nominal ? 4ull * (noms * nominal_stride + 4ull * T_e) : 0ull, false},
      {d_weights, 4ull * (last * weight_stride + K), true},
      {d_sums, 4ull * (last * sums_stride + 8ull * T_e), true},
      {d_nominal_out, 4ull * (last * nominal_out_stride + 4ull * T_e), true},
      {d_result, 32ull * G, true},
      {d_scratch, 4ull * l.words, true}};
  if (ranges_clash(ranges, in_place ? 4 : -1, 7)) {
    h->err = at + "an output overlaps an input or another output";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_out, "d_out", true}, {d_rollout_result, "d_rollout_result", true},
                           {d_delta, "d_delta", true}, {d_table, "d_table", true}, {d_weights, "d_weights", true},
                           {d_sums, "d_sums", true}, {d_nominal_out, "d_nominal_out", true},
                           {d_result, "d_result", true}, {d_scratch, "d_scratch", true},
                           {d_nominal, "d_nominal", false}}))
    return RPLGPU_ERR_INVALID_ARG;
  const rpl::MppiK k{m->xy_scale, m->shift, m->table_len, T_e};
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_mppi_update(h->stream, k, d_out, out_stride, d_rollout_result, d_delta, delta_stride,
                                     delta_per_group, d_table, d_nominal, nominal_stride, nominal_per_group, G, K,
                                     d_weights, weight_stride, d_sums, sums_stride, d_nominal_out, nominal_out_stride,
                                     d_result, d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_mppi_update(rplgpu_handle_t h, const rplgpu_mppi_t *m, const uint32_t *out,
                           const uint32_t rollout_result[8], const float *delta, const uint16_t *table,
                           const float *nominal, uint32_t K, uint32_t *weights, uint32_t *sums, float *nominal_out,
                           uint32_t result[8]) {
  const char *fn = "rplgpu_mppi_update";
  if (!h || !m || !out || !rollout_result || !delta || !table || !weights || !sums || !nominal_out || !result)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_mppi_check(m) != RPLGPU_OK) return refuse_spec(h, fn, "rplgpu_mppi_t");
  if (!update_counts_ok(h, fn, K, m->steps)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  const uint32_t T_e = m->delta_per_step ? m->steps : 1u;
  const size_t n_delta = (size_t)K * T_e;
  // out | rollout result | deltas | table | nominal | weights | sums | nominal out | result | scratch
  DoorBuffer buf(h, fn);
  const size_t o_out = buf.part(32u * (size_t)K), o_rres = buf.part(32), o_delta = buf.part(16u * n_delta);
  const size_t o_table = buf.part(2u * (size_t)m->table_len), o_nom = buf.part_if(nominal, 16u * (size_t)T_e);
  const size_t o_w = buf.part(4u * (size_t)K), o_sums = buf.part(32u * (size_t)T_e);
  const size_t o_nout = buf.part(16u * (size_t)T_e), o_res = buf.part(32);
  const size_t o_scr = buf.part(4u * (size_t)rplgpu_mppi_scratch_words(1, K, T_e));
  uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // every output is staged and filled behind the synchronise: a call that fails writes nothing (and nominal_out may
  // be nominal)
  std::vector<float> nout(4u * (size_t)T_e);
  std::vector<uint32_t> w_stage(K), sums_stage(8u * (size_t)T_e);
  const int32_t rc = buf.run([&]() -> int32_t {
    RPL_HIP(h, buf.put(o_out, out, 32u * (size_t)K));
    RPL_HIP(h, buf.put(o_rres, rollout_result, 32));
    RPL_HIP(h, buf.put(o_delta, delta, 16u * n_delta));
    RPL_HIP(h, buf.put(o_table, table, 2u * (size_t)m->table_len));
    RPL_HIP(h, buf.put(o_nom, nominal, 16u * (size_t)T_e));
    const int32_t irc = rplgpu_mppi_update_dev(
        h, m, buf.at<const uint32_t>(o_out), 8ull * K, buf.at<const uint32_t>(o_rres), buf.at<const float>(o_delta),
        4ull * n_delta, 0, buf.at<const uint16_t>(o_table), buf.at<const float>(o_nom), 4ull * T_e, 0, 1, K,
        buf.at<uint32_t>(o_w), K, buf.at<uint32_t>(o_sums), 8ull * T_e, buf.at<float>(o_nout), 4ull * T_e,
        buf.at<uint32_t>(o_res), buf.at<uint32_t>(o_scr));
    if (irc) return irc;
    RPL_HIP(h, buf.get(w_stage.data(), o_w, 4u * (size_t)K));
    RPL_HIP(h, buf.get(sums_stage.data(), o_sums, 32u * (size_t)T_e));
    RPL_HIP(h, buf.get(nout.data(), o_nout, 16u * (size_t)T_e));
    RPL_HIP(h, buf.get(words, o_res, 32));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
  if (rc) return rc;
  std::memcpy(weights, w_stage.data(), 4u * (size_t)K);
  std::memcpy(sums, sums_stage.data(), 32u * (size_t)T_e);
  std::memcpy(nominal_out, nout.data(), 16u * (size_t)T_e);
  std::memcpy(result, words, 32);
  return RPLGPU_OK;
}

int32_t rplgpu_mppi_spread_dev(rplgpu_handle_t h, const float *d_nominal, uint64_t nominal_stride,
                               uint32_t nominal_per_group, uint32_t T_n, const float *d_noise, uint64_t noise_stride,
                               uint32_t noise_per_group, uint32_t G, uint32_t K, uint32_t T, uint32_t shift,
                               uint32_t keep_first, float *d_out, uint64_t out_stride) {
  const char *fn = "rplgpu_mppi_spread_dev";
  const std::string at = std::string(fn) + ": ";
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  const PoseListDoor door{h, fn};
  if (!door.groups(G) || !spread_counts_ok(h, fn, K, T, T_n, shift)) return RPLGPU_ERR_INVALID_ARG;
  if (!d_nominal || !d_noise || !d_out || misaligned(d_nominal, 15u) || misaligned(d_noise, 15u) ||
      misaligned(d_out, 15u)) {
    h->err = at + "a pointer is missing or not 16-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t n = (uint64_t)K * T;
  if (nominal_stride < 4ull * T_n || (nominal_stride & 3u) || noise_stride < 4ull * n || (noise_stride & 3u) ||
      out_stride < 4ull * n || (out_stride & 3u)) {
    h->err = at + "nominal_stride >= 4 T_n, noise_stride and out_stride >= 4 K T (all multiples of 4) are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (((n + rpl::kMpBlock - 1u) / rpl::kMpBlock) * G > RPLGPU_MPPI_MAX_BLOCKS) {
    h->err = at + "a launch above RPLGPU_MPPI_MAX_BLOCKS workgroups";
    return RPLGPU_ERR_CAPACITY;
  }
  const uint64_t last = G - 1u;
  const bool in_place = (const float *)d_out == d_noise && out_stride == noise_stride && (noise_per_group || G == 1u);
  const Range ranges[] = {
      {d_nominal, 4ull * ((nominal_per_group ? last * nominal_stride : 0ull) + 4ull * T_n), false},
      {d_noise, 4ull * ((noise_per_group ? last * noise_stride : 0ull) + 4ull * n), false},
      {d_out, 4ull * (last * out_stride + 4ull * n), true}};
  if (ranges_clash(ranges, in_place ? 1 : -1, 2)) {
    h->err = at + "the output overlaps an input";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, {{d_nominal, "d_nominal", true}, {d_noise, "d_noise", true}, {d_out, "d_out", true}}))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_mppi_spread(h->stream, d_nominal, nominal_stride, nominal_per_group, T_n, d_noise,
                                     noise_stride, noise_per_group, G, K, T, shift, keep_first, d_out, out_stride));
  return RPLGPU_OK;
}

int32_t rplgpu_mppi_spread(rplgpu_handle_t h, const float *nominal, uint32_t T_n, const float *noise, uint32_t K,
                           uint32_t T, uint32_t shift, uint32_t keep_first, float *out) {
  const char *fn = "rplgpu_mppi_spread";
  if (!h || !nominal || !noise || !out) return RPLGPU_ERR_INVALID_ARG;
  if (!spread_counts_ok(h, fn, K, T, T_n, shift)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)K * T;
  DoorBuffer buf(h, fn);  // nominal | noise, spread in place
  const size_t o_nom = buf.part(16u * (size_t)T_n), o_noise = buf.part(16u * n);
  return buf.run([&]() -> int32_t {
    RPL_HIP(h, buf.put(o_nom, nominal, 16u * (size_t)T_n));
    RPL_HIP(h, buf.put(o_noise, noise, 16u * n));
    const int32_t irc = rplgpu_mppi_spread_dev(h, buf.at<const float>(o_nom), 4ull * T_n, 0, T_n,
                                               buf.at<const float>(o_noise), 4ull * n, 0, 1, K, T, shift, keep_first,
                                               buf.at<float>(o_noise), 4ull * n);
    if (irc) return irc;
    RPL_HIP(h, buf.get(out, o_noise, 16u * n));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  });
}

}  // extern "C"
