// rplgpu_api.hip — the extern "C" boundary declared in include/rplgpu.h, less the stages that
// have units of their own (rplgpu_scan_stages.hip, rplgpu_pose_stages.hip).
//
// Host side only: context/stream management, the host-evaluated lookup tables, the
// pinned staging used by the single-scan (host buffer) entry points, argument checking and
// the launch sizing of the batch, cloud / voxel, decode, message and exchange entry points.
// All arithmetic on samples happens in the kernel units (rpl_*.hip).  There is no CPU
// fallback: if no gfx950 device is usable, rplgpu_create fails.  What the three host units
// share (the handle, RPL_HIP, the helpers in rpl::host) is in rpl_host.hpp.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"
#include "rpl_host.hpp"
#include "rpl_msg.hpp"
#include "rpl_comm_layout.hpp"
#include "rpl_cells.hpp"

struct rplgpu_nccl_id_t {
  char internal[128];  // == ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES)
};

using namespace rpl::host;

namespace {

// Single-scan staging (rpl_host.hpp: nodes | tail | results | tail | flag): the flag word and the whole size.
constexpr size_t stage_flag_off(size_t max_n) { return stage_out_off(max_n) + round64(max_n * 16) + kTail; }
constexpr size_t stage_bytes(size_t max_n) { return stage_flag_off(max_n) + kTail; }

thread_local std::string g_create_err;

// dist_m exactly as src/rplidar_node.cpp:590 evaluates it (u32 -> f32 RNE, IEEE divide).
inline float host_dist_m(uint32_t d) { return static_cast<float>(d) / 4000.0f; }

// E1 keep mask as an interval of dist_mm_q2.  dist_m is monotone non-decreasing in d, so
//   {d : d != 0 && dist_m(d) >= range_min && dist_m(d) <= range_max} = [lo, hi]
// found by bisection with the very float expression the per-sample test would use.
// Returns false when the set is empty (also for NaN thresholds).
bool make_keep_interval(float range_min, float range_max, uint32_t *lo, uint32_t *hi) {
  const uint32_t dmax = 0xFFFFFFFFu;
  if (!(host_dist_m(dmax) >= range_min)) return false;  // also catches NaN
  if (!(host_dist_m(1u) <= range_max)) return false;
  uint32_t a = 1u, b = dmax;  // smallest d with dist_m(d) >= range_min
  while (a < b) {
    uint32_t m = a + (b - a) / 2;
    if (host_dist_m(m) >= range_min) b = m; else a = m + 1;
  }
  *lo = a;
  a = 1u, b = dmax;  // largest d with dist_m(d) <= range_max
  while (a < b) {
    uint32_t m = a + (b - a + 1) / 2;
    if (host_dist_m(m) <= range_max) a = m; else b = m - 1;
  }
  *hi = a;
  return *lo <= *hi;
}

// Which instance of k_cloud_voxel a batch launch uses: the one whose blocks may be aggregated in
// two classes pays off when scans make many short runs (range noise), and costs a clean batch
// 1.5-2.7 %.  RPLGPU_VOXEL_AGG_AUTO decides from THIS batch's own statistics: the queue entries per
// scan that the previous launch over the SAME batch (same device buffer, stride, scan count and
// group size) left in pinned memory behind it (read here without waiting: a stale or torn value
// only picks the other instance once — the results are the same either way).  A batch the handle
// has not launched before — another buffer or another shape — runs the plain instance; what an
// unrelated earlier batch looked like decides nothing (round 4: it did).  Round 6: the
// decision is kept per batch identity for the last eight identities, so that a caller alternating two
// staging buffers, or launching a batch in chunks (CloudExchange.step does), converges as well — the
// statistics always describe the previous launch and update THAT batch's entry.
bool voxel_split_for(rplgpu_ctx *c, const void *d_nodes, uint32_t n_stride, uint32_t B, uint32_t group) {
  group = std::max(1u, std::min(group, std::max(B, 1u)));
  const VoxelBatchId id{d_nodes, n_stride, B, group};
  const bool with_stats = c->h_vstats && (B + group - 1u) / group >= 64u;  // (launch_cloud_voxel's rule)
  auto find = [&](const VoxelBatchId &k) -> rplgpu_ctx::VoxelDecision * {
    for (auto &d : c->decisions)
      if (d.valid && d.id == k) return &d;
    return nullptr;
  };
  // the statistics in pinned memory describe the handle's PREVIOUS launch with statistics: they
  // update that batch's decision, whichever batch is launched now
  if (c->h_vstats && c->stats_valid) {
    const unsigned long long entries = __atomic_load_n(&c->h_vstats[0], __ATOMIC_RELAXED);
    const unsigned long long items = __atomic_load_n(&c->h_vstats[1], __ATOMIC_RELAXED);
    const uint32_t g = c->stats_group;
    if (items != 0 && entries <= items * g * 70000ull) {  // (sanity: a torn or stale pair)
      rplgpu_ctx::VoxelDecision *d = find(c->stats_id);
      if (!d) {
        d = &c->decisions[c->next_decision];
        c->next_decision = (c->next_decision + 1u) % (uint32_t)(sizeof(c->decisions) / sizeof(c->decisions[0]));
        d->id = c->stats_id;
        d->split = false;
        d->valid = true;
      }
      const unsigned long long avg = entries / (items * g);  // per scan, not per work item
      if (!d->split && avg > 6500ull) d->split = true;        // (a clean C3 scan: ~3300)
      else if (d->split && avg < 4000ull) d->split = false;   // (1 cm noise, two classes: ~6200)
    }
  }
  const rplgpu_ctx::VoxelDecision *mine = find(id);
  const bool split = mine ? mine->split : false;
  if (with_stats) {  // this launch's statistics will describe `id`
    c->stats_id = id;
    c->stats_valid = true;
    c->stats_group = group;
  }
  c->last_split = (c->force_split >= 0 ? c->force_split != 0 : split) ? 1 : 0;
  return c->last_split != 0;
}

// The reference's per-sample angle arithmetic, evaluated once per possible u16 input
// with the same operand types (float / double) and the same order of operations:
// src/rplidar_node.cpp:588-599 (conversion + wrap) and :646-651 (invert rule).
void build_tables(std::vector<float> &angle, std::vector<float> &angle_inv,
                  std::vector<float2> &cs, std::vector<float2> &cs_inv, std::vector<float> &inc,
                  std::vector<float> &rinc) {
  angle.resize(65536);
  angle_inv.resize(65536);
  cs.resize(65536);
  cs_inv.resize(65536);
  for (int q = 0; q < 65536; ++q) {
    uint16_t angle_z_q14 = (uint16_t)q;
    float angle_deg = angle_z_q14 * 90.0f / 16384.0f;
    float angle_rad = angle_deg * (M_PI / 180.0f);
    if (angle_rad < 0.0f) angle_rad += 2.0f * M_PI;
    if (angle_rad >= 2.0f * M_PI) angle_rad -= 2.0f * M_PI;
    float inv = (2.0f * M_PI) - angle_rad;
    if (inv >= 2.0f * M_PI) inv -= 2.0f * M_PI;
    angle[q] = angle_rad;
    angle_inv[q] = inv;
    cs[q] = make_float2((float)std::cos((double)angle_rad), (float)std::sin((double)angle_rad));
    cs_inv[q] = make_float2((float)std::cos((double)inv), (float)std::sin((double)inv));
  }
  // angle_increment of Mode A for every possible beam count, :635-636
  inc.resize(rpl::kMaxN + 1);
  inc[0] = 0.0f;
  for (uint32_t c = 1; c <= rpl::kMaxN; ++c)
    inc[c] = static_cast<float>((2.0 * M_PI) / static_cast<double>(c));
  // RN(1 / angle_increment) (IEEE fp32 divide) for the validated mul+2*FMA bin-index divide
  rinc.resize(rpl::kMaxN + 1);
  rinc[0] = 0.0f;
  for (uint32_t c = 1; c <= rpl::kMaxN; ++c) rinc[c] = 1.0f / inc[c];
}

template <class T>
int32_t upload(rplgpu_ctx *c, T **dst, const std::vector<T> &src) {
  RPL_HIP(c, hipMalloc((void **)dst, src.size() * sizeof(T)));
  RPL_HIP(c, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return RPLGPU_OK;
}

void comm_teardown(rplgpu_ctx *c);

void free_ctx(rplgpu_ctx *c) {
  if (!c) return;
  if (c->device >= 0) (void)hipSetDevice(c->device);
  comm_teardown(c);
  if (c->d_angle) (void)hipFree(c->d_angle);
  if (c->d_angle_inv) (void)hipFree(c->d_angle_inv);
  if (c->d_inc) (void)hipFree(c->d_inc);
  if (c->d_rinc) (void)hipFree(c->d_rinc);
  if (c->d_cs) (void)hipFree(c->d_cs);
  if (c->d_cs_inv) (void)hipFree(c->d_cs_inv);
  if (c->d_rcp) (void)hipFree(c->d_rcp);
  if (c->d_nodes) (void)hipFree(c->d_nodes);
  if (c->d_out) (void)hipFree(c->d_out);
  if (c->d_small) (void)hipFree(c->d_small);
  if (c->d_rormask) (void)hipFree(c->d_rormask);
  if (c->d_redo) (void)hipFree(c->d_redo);
  if (c->d_need_sort) (void)hipFree(c->d_need_sort);
  if (c->d_dec) (void)hipFree(c->d_dec);
  if (c->d_scans) (void)hipFree(c->d_scans);
  if (c->d_dec_todo) (void)hipFree(c->d_dec_todo);
  if (c->d_vstore) (void)hipFree(c->d_vstore);
  if (c->d_merge) (void)hipFree(c->d_merge);
  if (c->d_mkeys) (void)hipFree(c->d_mkeys);
  if (c->d_medges) (void)hipFree(c->d_medges);
  if (c->h_vstats) (void)hipHostFree(c->h_vstats);
  if (c->h_pin) (void)hipHostFree(c->h_pin);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

// Exhaustively compare the mul+2*FMA divide with the IEEE divide for divisor d on the
// device (about 2.4e9 operands, a few ms).  Returns RPLGPU_OK and sets *ok.
// (`rd`: the reciprocal the cheap divide is given — RN(1/d) for every caller but rplgpu_debug_validate_div)
int32_t count_div_mismatches(rplgpu_ctx *c, float d, float rd, uint32_t e_lo, uint32_t e_hi, uint32_t *count) {
  uint32_t zero = 0, bad = 1;
  RPL_HIP(c, hipMemcpyAsync(c->d_small + 8, &zero, 4, hipMemcpyHostToDevice, c->stream));
  RPL_HIP(c, rpl::launch_validate_div(c->stream, d, rd, e_lo, e_hi, c->d_small + 8));
  RPL_HIP(c, hipMemcpyAsync(&bad, c->d_small + 8, 4, hipMemcpyDeviceToHost, c->stream));
  RPL_HIP(c, hipStreamSynchronize(c->stream));
  *count = bad;
  return RPLGPU_OK;
}
int32_t validate_divisor(rplgpu_ctx *c, float d, uint32_t e_lo, uint32_t e_hi, bool *ok) {
  uint32_t bad = 1;
  if (int32_t rc = count_div_mismatches(c, d, 1.0f / d, e_lo, e_hi, &bad)) return rc;
  *ok = (bad == 0);
  return RPLGPU_OK;
}

// publish_scan on the handle's stream: Mode A (rpl_laserscan.hip) or Mode B.  The cheap
// bin-index divide of Mode A is used only after it was compared with the IEEE divide for
// every (beam count <= 32768, angle word, inverted or not) on this device, once per handle.
int32_t ensure_idx_checked(rplgpu_ctx *c);
int32_t run_laserscan(rplgpu_ctx *c, const void *d_nodes, uint32_t n_stride,
                      const uint32_t *d_n_per_scan, uint32_t B, const rplgpu_params_t &p,
                      float *d_ranges, float *d_intens, uint32_t *d_beam_count,
                      uint32_t n_given = 0xFFFFFFFFu) {
  const rpl::KParams kp = to_kparams(p);
  if (!p.scan_processing) {
    RPL_HIP(c, rpl::launch_laserscan_raw(c->stream, d_nodes, n_stride, d_n_per_scan, B, kp, d_ranges,
                                         d_intens, d_beam_count));
    return RPLGPU_OK;
  }
  if (int32_t vrc = ensure_idx_checked(c)) return vrc;
  RPL_HIP(c, rpl::launch_laserscan_a(c->stream, d_nodes, n_stride, d_n_per_scan, B, kp, tables_of(c),
                                     c->d_inc, c->d_rinc, use_fast_idx(c) && use_fast_d4000(c), d_ranges,
                                     d_intens, d_beam_count, n_given));
  return RPLGPU_OK;
}

// the bin-index divide of Mode A: validated once per handle (k_validate_idx, every beam count and
// angle word)
int32_t ensure_idx_checked(rplgpu_ctx *c) {
  if (!c->idx_checked) {
    uint32_t zero = 0, bad = 1;
    RPL_HIP(c, hipMemcpyAsync(c->d_small + 8, &zero, 4, hipMemcpyHostToDevice, c->stream));
    // every beam count a kernel can meet (n_stride may exceed max_samples_per_scan of the handle;
    // the kernels clamp to kMaxN), not just those up to max_n
    RPL_HIP(c, rpl::launch_validate_idx(c->stream, tables_of(c), c->d_inc, c->d_rinc, rpl::kMaxN,
                                        c->d_small + 8));
    RPL_HIP(c, hipMemcpyAsync(&bad, c->d_small + 8, 4, hipMemcpyDeviceToHost, c->stream));
    RPL_HIP(c, hipStreamSynchronize(c->stream));
    c->idx_ok = (bad == 0);
    c->idx_checked = true;
  }
  return RPLGPU_OK;
}

// nodes + their count to the device in ONE copy; *d_n = device address of the count word
int32_t upload_scan(rplgpu_ctx *c, const rplgpu_node_t *nodes, size_t n, const uint32_t **d_n) {
  std::memcpy(c->h_pin, nodes, n * 8);
  const uint32_t words[2] = {(uint32_t)n, 0u};  // count, status (cleared)
  std::memcpy(c->h_pin + n * 8, words, 8);
  RPL_HIP(c, hipMemcpyAsync(c->d_nodes, c->h_pin, n * 8 + 8, hipMemcpyHostToDevice, c->stream));
  *d_n = reinterpret_cast<const uint32_t *>(c->d_nodes + n * 8);
  return RPLGPU_OK;
}

// Zero-copy staging of one scan: the nodes and their count word are placed in the pinned buffer
// (a CPU copy of n * 8 bytes) and the kernels address that buffer directly.
// End of a zero-copy single-scan call: wait until the kernels queued on the stream are done and
// their writes to the pinned staging are visible.  hipStreamSynchronize costs ~15 us of wake-up
// latency on this stack; instead a one-lane kernel queued behind the work stores a sequence
// number into pinned memory (system-scope release) and the calling thread — the node's scan
// thread, which has nothing else to do until the scan is converted — polls it.  Falls back to
// the runtime's synchronisation after ~2 ms (that is also where errors surface).
int32_t wait_scan(rplgpu_ctx *c) {
  if (!c->spin_sync) {
    RPL_HIP(c, hipStreamSynchronize(c->stream));
    return RPLGPU_OK;
  }
  volatile uint32_t *flag = reinterpret_cast<volatile uint32_t *>(c->h_pin + c->flag_off);
  const uint32_t seq = ++c->scan_seq;
  RPL_HIP(c, rpl::launch_signal(c->stream, reinterpret_cast<uint32_t *>(c->d_pin + c->flag_off), seq));
  for (uint32_t spins = 0; spins < 400000u; ++spins) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return RPLGPU_OK;
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
  }
  RPL_HIP(c, hipStreamSynchronize(c->stream));
  return RPLGPU_OK;
}

struct ScanStage {
  const rplgpu_node_t *d_nodes;  // device view of the staged nodes
  const uint32_t *d_n;           // ... of the count word (status word right behind it)
  unsigned char *d_out;          // ... of the result area (16 B per sample + tail)
  unsigned char *h_out;          // host view of the result area
};
inline ScanStage stage_scan(rplgpu_ctx *c, const rplgpu_node_t *nodes, size_t n) {
  std::memcpy(c->h_pin, nodes, n * 8);
  const uint32_t words[2] = {(uint32_t)n, 0u};
  std::memcpy(c->h_pin + n * 8, words, 8);
  ScanStage s;
  s.d_nodes = reinterpret_cast<const rplgpu_node_t *>(c->d_pin);
  s.d_n = reinterpret_cast<const uint32_t *>(c->d_pin + n * 8);
  const size_t out_off = stage_out_off(c->max_n);
  s.d_out = c->d_pin + out_off;
  s.h_out = c->h_pin + out_off;
  return s;
}

}  // namespace

// ---- the helpers the stage units use as well (declared in rpl_host.hpp) ------------------------

namespace rpl {
namespace host {

rpl::KParams to_kparams(const rplgpu_params_t &p) {
  rpl::KParams k;
  k.is_new_protocol = p.is_new_protocol != 0;
  k.inverted = p.inverted != 0;
  k.scan_processing = p.scan_processing != 0;
  k.clip_enable = p.clip_enable != 0;
  k.q_min = p.q_min;
  k.range_min = p.range_min;
  k.range_max = p.range_max;
  k.voxel_leaf = p.voxel_leaf;
  k.ror_r2 = p.ror_radius * p.ror_radius;
  k.ror_k = p.ror_min_neighbors;
  // voxel fixed point: 2^-K = ulp(leaf), so L = leaf*2^K is the leaf's integer significand
  k.vox_scale = 1.0;
  k.vox_scale_f = 1.0f;
  k.vox_L = 1;
  k.vox_bias = 0;  // (round 3: offsets are summed as wrapping two's complement, no bias)
  k.inv_leaf = 1.0f;
  k.leaf_s = 1.0f;
  k.inv_leaf_s = 1.0f;
  k.fast_div = 0;
  k.fast_d4000 = 0;
  k.dbg = nullptr;
  k.cell_keys = nullptr;
  k.d_lo = 1u;  // :584 alone: dist_mm_q2 != 0
  k.d_span = 0xFFFFFFFEu;
  k.cell_range_safe = 0;
  if (k.clip_enable) {
    uint32_t lo, hi;
    if (make_keep_interval(p.range_min, p.range_max, &lo, &hi)) {
      k.d_lo = lo;
      k.d_span = hi - lo;
      if (p.voxel_leaf > 0.0f && host_dist_m(hi) / p.voxel_leaf < 32000.0f) k.cell_range_safe = 1;
    } else {
      k.d_span = 0u;
      k.q_min = 256u;  // no quality byte reaches 256: nothing is kept
    }
  }
  if (p.voxel_leaf > 0.0f && std::isfinite(p.voxel_leaf)) {
    int K = 23 - std::ilogb(p.voxel_leaf);
    k.vox_scale = std::ldexp(1.0, K);
    k.vox_scale_f = (float)k.vox_scale;
    k.vox_L = (int32_t)std::llround((double)p.voxel_leaf * k.vox_scale);
    k.inv_leaf = 1.0f / p.voxel_leaf;
    k.leaf_s = p.voxel_leaf * k.vox_scale_f;
    k.inv_leaf_s = k.inv_leaf / k.vox_scale_f;
  }
  return k;
}

rpl::Tables tables_of(rplgpu_ctx *c) {
  rpl::Tables t;
  t.angle = c->d_angle;
  t.angle_inv = c->d_angle_inv;
  t.cs = c->d_cs;
  t.cs_inv = c->d_cs_inv;
  t.rcp = c->d_rcp;
  t.work_ctr = c->d_small + 16;  // [16] next scan of k_cloud_voxel's queue (cleared per launch)
  t.n_cu = c->n_cu;
  t.voxel_store = c->d_vstore;
  t.voxel_store_wgs = c->vstore_wgs;
  t.voxel_store_recs = c->vstore_recs;
  t.voxel_stats = reinterpret_cast<unsigned long long *>(c->d_small + 24);  // [24..27]
  t.voxel_stats_host = c->h_vstats;
  t.voxel_split = c->force_split > 0 ? 1 : 0;  // (batch launches: voxel_split_for)
  t.scan_t0 = c->scan_t0;
  t.redo = c->d_redo;
  return t;
}

// A wrong pointer handed to a kernel is a GPU memory fault, and on this platform a fault ends
// the whole process (the node would die instead of falling back to its CPU loop, cf.
// src/rplidar_node.cpp:453-474).  So the batch entry points ask the runtime what a pointer is
// before launching: it has to be device (or managed / mapped host) memory reachable from the
// handle's device.  ~1 us per pointer against launches of >= tens of us.
bool device_readable(rplgpu_ctx *c, const void *ptr, const char *what) {
  if (!c->check_ptrs) return true;
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  const hipError_t e = hipPointerGetAttributes(&a, ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // unregistered host memory: not an error state worth keeping
    c->err = std::string(what) + " is not device-accessible memory";
    return false;
  }
  if (a.type == hipMemoryTypeDevice && a.device != c->device) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, c->device, a.device) != hipSuccess || !can) {
      c->err = std::string(what) + " lives on another device without peer access";
      return false;
    }
  }
  if (a.type == hipMemoryTypeUnregistered) {
    c->err = std::string(what) + " is plain host memory";
    return false;
  }
  return true;
}

int32_t check_batch(rplgpu_ctx *c, const void *nodes, uint32_t n_stride, const void *n_per_scan,
                    uint32_t B, bool own_buffers) {
  if (!c) return RPLGPU_ERR_INVALID_ARG;
  if (B == 0) return RPLGPU_OK;
  if (!nodes || !n_per_scan || n_stride == 0) {
    c->err = "null buffer or zero stride";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B > c->max_b) {
    c->err = "batch larger than max_batch given to rplgpu_create";
    return RPLGPU_ERR_CAPACITY;
  }
  if (!own_buffers && (!device_readable(c, nodes, "d_nodes") || !device_readable(c, n_per_scan, "d_n_per_scan")))
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

}  // namespace host
}  // namespace rpl

extern "C" {

int32_t rplgpu_abi_version(void) { return RPLGPU_ABI_VERSION; }

void rplgpu_default_params(rplgpu_params_t *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->scan_processing = 1;  // code default, src/rplidar_node.cpp:280
  p->range_min = 0.15f;    // :625
  p->range_max = 12.0f;    // cached_current_max_range_ initial value, include/rplidar_node.hpp
  p->voxel_leaf = 0.05f;
  p->ror_radius = 0.10f;
  p->ror_min_neighbors = 2;
}

void rplgpu_fill_meta(const rplgpu_params_t *p, uint32_t count, double scan_duration,
                      rplgpu_scan_meta_t *meta) {
  if (!meta) return;
  std::memset(meta, 0, sizeof(*meta));
  if (count == 0 || !p) return;  // :611-613 (and: no parameters, nothing to publish)
  meta->published = 1;
  meta->count = count;
  meta->angle_min = 0.0f;          // :623
  meta->angle_max = 2.0f * M_PI;   // :624
  meta->range_min = 0.15f;         // :625
  meta->range_max = p->range_max;  // :626
  meta->scan_time = scan_duration; // :627
  if (p->scan_processing) {        // :634-638
    size_t beam_count = count;
    meta->angle_increment = static_cast<float>((2.0 * M_PI) / static_cast<double>(beam_count));
    meta->time_increment = static_cast<float>(scan_duration / static_cast<double>(beam_count));
  } else {                         // :665-669
    size_t cnt = count;
    double denom = static_cast<double>(cnt > 1 ? cnt - 1 : 1);
    meta->angle_increment = static_cast<float>((2.0 * M_PI) / denom);
    meta->time_increment = static_cast<float>(scan_duration / denom);
  }
}

int32_t rplgpu_create(int32_t device_id, uint32_t max_samples_per_scan, uint32_t max_batch,
                      rplgpu_handle_t *out) {
  if (!out) return RPLGPU_ERR_INVALID_ARG;
  *out = nullptr;
  // (max_batch < 2^24: the ascend kernels' list of scans to sort packs a scan index into 24 bits)
  if (max_samples_per_scan == 0 || max_samples_per_scan > RPLGPU_MAX_SAMPLES_PER_SCAN ||
      max_batch == 0 || max_batch >= (1u << 24))
    return RPLGPU_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RPLGPU_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= ndev) return RPLGPU_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return RPLGPU_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RPLGPU_ERR_NO_DEVICE;  // CDNA4 only
  if (hipSetDevice(device_id) != hipSuccess) return RPLGPU_ERR_NO_DEVICE;

  rplgpu_ctx *c = new (std::nothrow) rplgpu_ctx();
  if (!c) return RPLGPU_ERR_HIP;
  c->device = device_id;
  c->max_n = max_samples_per_scan;
  c->max_b = max_batch;
  c->n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
  if (const char *e = std::getenv("RPLGPU_CHECK_POINTERS")) c->check_ptrs = std::atoi(e) != 0;
  auto fail = [&](int32_t code) {
    g_create_err = c->err;
    free_ctx(c);
    return code;
  };
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess)
    return fail(RPLGPU_ERR_HIP);
  c->stream = c->own_stream;

  std::vector<float> angle, angle_inv, inc, rinc;
  std::vector<float2> cs, cs_inv;
  build_tables(angle, angle_inv, cs, cs_inv, inc, rinc);
  // Sorting by q14 stands in for sorting by angle_rad (:607-609): require monotonicity.
  for (int q = 1; q < 65536; ++q) {
    if (!(angle[q] > angle[q - 1])) {
      c->err = "angle table not strictly increasing";
      return fail(RPLGPU_ERR_INVALID_ARG);
    }
  }
  // correctly rounded fp64 reciprocals of every possible per-cell sample count (IEEE divide)
  std::vector<double> rcp(rpl::kMaxN + 1);
  rcp[0] = 0.0;
  for (uint32_t k = 1; k <= rpl::kMaxN; ++k) rcp[k] = 1.0 / static_cast<double>(k);
  int32_t rc;
  if ((rc = upload(c, &c->d_rcp, rcp)) || (rc = upload(c, &c->d_angle, angle)) || (rc = upload(c, &c->d_angle_inv, angle_inv)) ||
      (rc = upload(c, &c->d_cs, cs)) || (rc = upload(c, &c->d_cs_inv, cs_inv)) ||
      (rc = upload(c, &c->d_inc, inc)) || (rc = upload(c, &c->d_rinc, rinc)))
    return fail(rc);

  const size_t n = c->max_n;
  // single-scan staging: the length word travels right behind the nodes and the result words
  // right behind the results, so that a call is one copy in and one copy out
  c->flag_off = stage_flag_off(n);  // (a cache line of its own, 64-byte aligned for every n)
  if (hipHostMalloc((void **)&c->h_pin, stage_bytes(n), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void **)&c->d_nodes, n * 8 + kTail) != hipSuccess ||
      hipMalloc((void **)&c->d_out, n * 16 + kTail) != hipSuccess ||
      hipMalloc((void **)&c->d_small, 128) != hipSuccess ||
      // per-call scratch of the batch entry points, sized once for max_batch (no allocation on
      // the per-call paths): ascend's "needs the sorting kernel" list and the E5 keep bits
      hipMalloc((void **)&c->d_need_sort, ((size_t)c->max_b + 1u) * 4u) != hipSuccess ||
      hipMalloc((void **)&c->d_rormask, (size_t)c->max_b * kMaskStride * 4u) != hipSuccess ||
      hipMalloc((void **)&c->d_redo, ((size_t)c->max_b + 4u) * 4u) != hipSuccess) {
    c->err = "staging allocation failed";
    return fail(RPLGPU_ERR_HIP);
  }
  c->need_sort_cap = c->max_b;
  // (the sort list starts, and is kept, empty between calls; the count of work items E5-inside listed is 0
  // until a launch of run_voxel says otherwise — rplgpu_debug_ror_listed reads it on any handle)
  if (hipMemset(c->d_need_sort, 0, 4) != hipSuccess || hipMemset(c->d_redo, 0, 4) != hipSuccess) {
    c->err = "staging allocation failed";
    return fail(RPLGPU_ERR_HIP);
  }
  // the voxel kernel's record stores (overflow of its LDS queue; 512 KiB per resident workgroup,
  // at most two workgroups per CU and never more than scans in a batch)
  c->vstore_wgs = std::min<uint32_t>(c->max_b, rpl::voxel_max_workgroups(c->n_cu));
  c->vstore_recs = (uint32_t)rpl::voxel_store_need(1u, rpl::kMaxN);
  // (x 2: every workgroup's record store is followed by its temporary cell area of the same size)
  if (hipMalloc(&c->d_vstore, (size_t)c->vstore_wgs * c->vstore_recs * 32u) != hipSuccess) {
    c->err = "record store allocation failed";
    return fail(RPLGPU_ERR_HIP);
  }
  // Single scans go through host memory the device can address: the kernels read the nodes from
  // the pinned staging and write their results into it over PCIe — one launch and one
  // synchronisation per call instead of DMA in + kernel + DMA out (RPLGPU_ZERO_COPY=0: the DMA
  // path of round 1, kept for comparison).
  if (hipHostMalloc((void **)&c->h_vstats, 16, hipHostMallocDefault) == hipSuccess) {
    c->h_vstats[0] = c->h_vstats[1] = 0ull;
  } else {
    c->h_vstats = nullptr;  // (no statistics: the plain instance is always used)
    (void)hipGetLastError();
  }
  if (hipHostGetDevicePointer((void **)&c->d_pin, c->h_pin, 0) != hipSuccess) c->d_pin = nullptr;
  if (const char *e = std::getenv("RPLGPU_ZERO_COPY")) c->zero_copy = std::atoi(e) != 0;
  if (!c->d_pin) c->zero_copy = false;
  if (const char *e = std::getenv("RPLGPU_SPIN_SYNC")) c->spin_sync = std::atoi(e) != 0;
  if (const char *e = std::getenv("RPLGPU_DEC_STAGE")) c->dec_stage = std::atoi(e) != 0;
  if (const char *e = std::getenv("RPLGPU_VOXEL_SPLIT")) c->force_split = std::atoi(e) != 0;  // developer aid
  if (const char *e = std::getenv("RPLGPU_ROR_FUSED")) c->ror_fused = std::atoi(e) != 0;  // 0: E5 as two kernels (tests / A-B runs)
  std::memset(c->h_pin + c->flag_off, 0, kTail);
  if (hipMemset(c->d_small, 0, 128) != hipSuccess) {  // incl. the voxel kernel's scan queue
    c->err = "staging clear failed";
    return fail(RPLGPU_ERR_HIP);
  }
  // dist_mm_q2 / 4000.0f: operands are the integer-valued floats 1 .. 2^32
  if (validate_divisor(c, 4000.0f, 127, 159, &c->div4000_ok) != RPLGPU_OK) return fail(RPLGPU_ERR_HIP);
  // the default leaf is validated here, so that the first cloud call does not have to stop the
  // stream for it (any other leaf is validated, once, by the first call that uses it)
  if (validate_divisor(c, 0.05f, 27, 167, &c->leaf_ok) != RPLGPU_OK) return fail(RPLGPU_ERR_HIP);
  c->leaf_checked = 0.05f;
  *out = c;
  return RPLGPU_OK;
}

int32_t rplgpu_destroy(rplgpu_handle_t h) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  free_ctx(h);
  return RPLGPU_OK;
}

const char *rplgpu_last_error(rplgpu_handle_t h) {
  if (!h) return g_create_err.c_str();
  return h->err.c_str();
}

int32_t rplgpu_set_stream(rplgpu_handle_t h, void *hip_stream) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  hipStream_t next = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  if (next != h->stream) {
    // work queued on the old stream shares the handle's scratch (scan queue, staging, masks)
    // with whatever is launched next: drain it before switching
    RPL_HIP(h, hipSetDevice(h->device));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
  }
  h->stream = next;
  return RPLGPU_OK;
}

int32_t rplgpu_set_cell_key_output(rplgpu_handle_t h, uint32_t *d_cell_keys) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (d_cell_keys && !device_readable(h, d_cell_keys, "d_cell_keys")) return RPLGPU_ERR_INVALID_ARG;
  h->cell_keys = d_cell_keys;
  return RPLGPU_OK;
}

int32_t rplgpu_set_scan_time_offsets_dev(rplgpu_handle_t h, const float *d_t0) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (d_t0 && !device_readable(h, d_t0, "d_t0")) return RPLGPU_ERR_INVALID_ARG;
  h->scan_t0 = d_t0;
  return RPLGPU_OK;
}

int32_t rplgpu_set_voxel_aggregation(rplgpu_handle_t h, int32_t mode) {
  if (!h || mode < RPLGPU_VOXEL_AGG_AUTO || mode > RPLGPU_VOXEL_AGG_TWO_CLASS) return RPLGPU_ERR_INVALID_ARG;
  h->force_split = mode == RPLGPU_VOXEL_AGG_AUTO ? -1 : (mode == RPLGPU_VOXEL_AGG_TWO_CLASS ? 1 : 0);
  return RPLGPU_OK;
}

// Developer aid (not part of rplgpu.h): device buffer of 16*B u64 receiving, per work item, the
// shader cycles k_cloud_voxel spent in its phases (slots 0-7: stream, ..., emit; 8-12: the
// streaming loop's sub-phases).
int32_t rplgpu_debug_set_cycle_buffer(rplgpu_handle_t h, void *d_buf) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  h->dbg = (unsigned long long *)d_buf;
  return RPLGPU_OK;
}
// Developer aid (tests): how many scans of the handle's last rplgpu_ascend_batch_dev /
// rplgpu_ascend_laserscan_batch_dev call failed the streaming kernel's order check and were sorted
// by k_ascend<true>.  Waits for the stream.
int32_t rplgpu_debug_ascend_sorted(rplgpu_handle_t h, uint32_t *count) {
  if (!h || !count) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  RPL_HIP(h, hipMemcpy(count, h->d_small + 28, 4, hipMemcpyDeviceToHost));
  return RPLGPU_OK;
}
// Developer aid (tests): the block-aggregation instance the handle's last voxel batch launch took
// (0 plain, 1 two-class) — what RPLGPU_VOXEL_AGG_AUTO decided for it.
// developer aid (tests): the single-scan staging layout a handle of this capacity gets — byte offsets of
// the result area and of the completion flag in the pinned buffer, and the buffer's size.  Host only.
int32_t rplgpu_debug_staging_layout(uint32_t max_samples_per_scan, uint64_t out[3]) {
  if (!out || max_samples_per_scan == 0 || max_samples_per_scan > RPLGPU_MAX_SAMPLES_PER_SCAN)
    return RPLGPU_ERR_INVALID_ARG;
  out[0] = stage_out_off(max_samples_per_scan);
  out[1] = stage_flag_off(max_samples_per_scan);
  out[2] = stage_bytes(max_samples_per_scan);
  return RPLGPU_OK;
}
int32_t rplgpu_debug_voxel_instance(rplgpu_handle_t h) { return h ? h->last_split : RPLGPU_ERR_INVALID_ARG; }
int32_t rplgpu_set_ror_mode(rplgpu_handle_t h, int32_t mode) {
  if (!h || (mode != RPLGPU_ROR_INSIDE && mode != RPLGPU_ROR_TWO_KERNELS)) return RPLGPU_ERR_INVALID_ARG;
  h->ror_fused = mode == RPLGPU_ROR_INSIDE ? 1 : 0;
  return RPLGPU_OK;
}
// (tests / tools: work items the last E5-inside launch left to the two kernels; waits for the stream)
int32_t rplgpu_debug_ror_listed(rplgpu_handle_t h, uint32_t *count) {
  if (!h || !count) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  RPL_HIP(h, hipMemcpy(count, h->d_redo, 4, hipMemcpyDeviceToHost));
  return RPLGPU_OK;
}
int32_t rplgpu_debug_fast_div(rplgpu_handle_t h) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return (h->div4000_ok ? 1 : 0) | (h->leaf_ok ? 2 : 0) | (h->idx_ok ? 4 : 0);
}
// Developer aid (tests): run the IEEE-divide kernel instances although validation passed.  `mask` has
// the bits of rplgpu_debug_fast_div (1: / 4000, 2: / leaf, 4: Mode A's bin index); while a bit is set,
// every launch site behaves as if that validation had failed.  Holds, across re-validations of the
// leaf, until cleared with mask = 0; rplgpu_debug_fast_div goes on returning what validation found.
int32_t rplgpu_debug_force_ieee_div(rplgpu_handle_t h, uint32_t mask) {
  if (!h || mask > 7u) return RPLGPU_ERR_INVALID_ARG;
  h->force_ieee = mask;
  return RPLGPU_OK;
}
// Developer aid (tests): k_validate_div for divisor `d` with a reciprocal of the caller's choice, over
// the operands of biased exponent e_lo .. e_hi — how many of the compared quotients differ from the
// IEEE divide (three forms are compared per operand; the count is a 32-bit word, so a range of more than
// 170 exponents can wrap it).  Waits for the stream.
int32_t rplgpu_debug_validate_div(rplgpu_handle_t h, float d, float rd, uint32_t e_lo, uint32_t e_hi,
                                  uint32_t *mismatches) {
  if (!h || !mismatches || e_lo > e_hi || e_hi > 254u) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  return count_div_mismatches(h, d, rd, e_lo, e_hi, mismatches);
}

int32_t rplgpu_synchronize(rplgpu_handle_t h) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  if (h->xstream) RPL_HIP(h, hipStreamSynchronize(h->xstream));
  return RPLGPU_OK;
}

// ---- device-resident batches ----------------------------------------------------

int32_t rplgpu_ascend_batch_dev(rplgpu_handle_t h, rplgpu_node_t *d_nodes, uint32_t n_stride,
                                const uint32_t *d_n_per_scan, uint32_t B, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_ascend(h->stream, d_nodes, n_stride, d_n_per_scan, B, d_status,
                                h->d_need_sort, false, h->d_small + 28));
  return RPLGPU_OK;
}

int32_t rplgpu_laserscan_batch_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                   uint32_t n_stride, const uint32_t *d_n_per_scan, uint32_t B,
                                   const rplgpu_params_t *p, float *d_ranges,
                                   float *d_intensities, uint32_t *d_beam_count) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !d_ranges || !d_intensities || !d_beam_count) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  return run_laserscan(h, d_nodes, n_stride, d_n_per_scan, B, *p, d_ranges, d_intensities,
                       d_beam_count);
}

// S1 -> S3 in one pass (see include/rplgpu.h): the LaserScan does not depend on the ascend step, so
// the binning kernel reads the raw nodes; the ascend kernels run behind it only when the caller
// wants the ascended nodes as well.
int32_t rplgpu_ascend_laserscan_batch_dev(rplgpu_handle_t h, rplgpu_node_t *d_nodes,
                                          uint32_t n_stride, const uint32_t *d_n_per_scan,
                                          uint32_t B, const rplgpu_params_t *p, float *d_ranges,
                                          float *d_intensities, uint32_t *d_beam_count,
                                          int32_t write_ascended, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !d_ranges || !d_intensities || !d_beam_count) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  rc = run_laserscan(h, d_nodes, n_stride, d_n_per_scan, B, *p, d_ranges, d_intensities,
                     d_beam_count);
  if (rc || !write_ascended) return rc;
  RPL_HIP(h, rpl::launch_ascend(h->stream, d_nodes, n_stride, d_n_per_scan, B, d_status,
                                h->d_need_sort, false, h->d_small + 28));
  return RPLGPU_OK;
}

// What a cloud entry point asks of prepare_cloud, and the plan it gets back.
struct CloudRequest {
  bool force_two_kernels = false;  // E5 as k_ror_mask + the masked kernel whatever the handle's mode
  bool defer_listed = false;       // see run_voxel (single-scan callers; d_status must be given then)
  bool own_buffers = false;        // the handle's own staging: no pointer check
  uint32_t group = 1;              // scans per work item (E8)
  bool cells = false;              // the arena holds cell records (rplgpu_cloud_fused_cells_dev)
};
struct CloudPlan {
  rpl::KParams kp;
  rpl::Tables T;
  const uint32_t *mask = nullptr;  // E5 as the two kernels: the keep bits (k_ror_mask is queued)
  bool ror_inside = false;         // E5 inside the voxel kernel: no mask, see run_voxel
};

// E5 runs inside the voxel kernel unless the caller forces the two kernels, when the handle's mode says so
// (rplgpu_set_ror_mode) and the ROR instance exists for the launch: voxel grid, validated divides, not
// the instrumented build
static bool ror_runs_inside(const rplgpu_ctx *h, const CloudRequest &req, const rplgpu_params_t &p,
                            const rpl::KParams &kp) {
  return !req.force_two_kernels && h->ror_fused && p.voxel_enable && kp.fast_div && !kp.dbg;
}

// parameter checks, divisor validation, the E5 path (with the mask of the two kernels queued) and the
// voxel kernel instance, shared by the cloud entry points (`plan`: a fresh CloudPlan)
static int32_t prepare_cloud(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                             const uint32_t *d_n_per_scan, uint32_t B, const rplgpu_params_t *p,
                             const CloudRequest &req, CloudPlan *plan) {
  if (p->ror_enable && !(p->ror_radius > 0.0f && p->ror_radius <= 1.0e6f)) {
    h->err = "ror_radius must be in (0, 1e6] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (p->voxel_enable && !(p->voxel_leaf >= 1e-6f && p->voxel_leaf <= 1024.0f)) {
    h->err = "voxel_leaf must be in [1e-6, 1024] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  plan->kp = to_kparams(*p);
  rpl::KParams &kp = plan->kp;
  if (p->voxel_enable) {
    // the cheap divides are used only for divisors proven bit-identical on this device
    if (h->leaf_checked != p->voxel_leaf) {
      int32_t vrc = validate_divisor(h, p->voxel_leaf, 27, 167, &h->leaf_ok);  // 2^-100..2^40
      if (vrc) return vrc;
      h->leaf_checked = p->voxel_leaf;
    }
    kp.fast_div = (use_fast_d4000(h) && use_fast_leaf(h)) ? 1 : 0;
  }
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  kp.dbg = h->dbg;
  kp.cell_keys = h->cell_keys;
  plan->T = tables_of(h);
  if (p->ror_enable) {  // E5 before E4: per-sample keep bits, then the cloud kernels apply them
    plan->ror_inside = ror_runs_inside(h, req, *p, kp);
    if (!plan->ror_inside) {
      RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, plan->T,
                                      h->d_rormask, kMaskStride));
      plan->mask = h->d_rormask;
    }
  }
  if (req.cells) {  // the record holds the key (no cell-key words); the instrumented instance has no cell form
    kp.cell_keys = nullptr;
    kp.dbg = nullptr;
  }
  if (p->voxel_enable) {
    plan->T.voxel_split = voxel_split_for(h, d_nodes, n_stride, B, req.group) ? 1 : 0;
    // (the cell form lives in the instances other than the plain one, csrc/rpl_voxel.hip voxel_reduce:
    // without E5 inside, the records come from the two-class instance, whose results are the same)
    if (req.cells && !plan->ror_inside) plan->T.voxel_split = 1;
  }
  return RPLGPU_OK;
}

// The voxel launch(es) of a plan; `v` describes input and output, the plan supplies E5.
// E5 + E4 of a launch in ONE pass over the scans (round 6): the voxel kernel's ROR instance
// settles a sample by its index neighbours while it streams the scan and resolves the few that stay
// open itself (csrc/rpl_voxel.hip: voxel_stream HASROR, ror_resolve).  A work item with more open
// samples than that (clutter: hundreds of isolated returns) is put on a list instead, and the two
// kernels of rounds 1-5 — k_ror_mask, then the voxel kernel with the mask — run over the LISTED
// items behind it: two launches that find an empty list on ring-like data and end at once.
// (`defer_listed`: the two launches over the list are left to the caller, who looks at the status word
// first — the single-scan entry points wait for their one scan anyway and redo it only if it carries
// rpl::kRorListedBit.)
static int32_t run_voxel(rplgpu_handle_t h, const CloudPlan &plan, rpl::VoxelLaunch v,
                         bool defer_listed = false) {
  if (v.arena) RPL_HIP(h, hipMemsetAsync(v.arena_cursor, 0, 8, h->stream));  // (the call resets *d_cursor)
  v.keepmask = plan.mask;  // (none with E5 inside)
  v.mask_stride = kMaskStride;
  if (plan.ror_inside) {
    RPL_HIP(h, hipMemsetAsync(h->d_redo, 0, 4, h->stream));
    v.ror = rpl::RorMode::kInside;
  }
  RPL_HIP(h, rpl::launch_cloud_voxel(h->stream, v, plan.kp, plan.T));
  if (!plan.ror_inside || defer_listed) return RPLGPU_OK;
  RPL_HIP(h, rpl::launch_ror_mask(h->stream, v.nodes, v.n_stride, v.n_per_scan, v.B, plan.kp, plan.T,
                                  h->d_rormask, kMaskStride, true, std::max(1u, std::min(v.group, v.B))));
  v.keepmask = h->d_rormask;
  v.ror = rpl::RorMode::kListed;
  RPL_HIP(h, rpl::launch_cloud_voxel(h->stream, v, plan.kp, plan.T));
  return RPLGPU_OK;
}

static int32_t cloud_arena_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, const rplgpu_params_t *p,
                               float *d_arena, uint64_t arena_capacity, uint64_t *d_cursor,
                               uint64_t *d_scan_start, uint32_t *d_n_points, uint32_t *d_status,
                               bool xyi) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !d_arena || !d_cursor || !d_scan_start || !d_n_points) return RPLGPU_ERR_INVALID_ARG;
  if (!p->voxel_enable) {
    h->err = "rplgpu_cloud_arena_dev needs voxel_enable";
    return RPLGPU_ERR_INVALID_ARG;
  }
  CloudPlan plan;
  if ((rc = prepare_cloud(h, d_nodes, n_stride, d_n_per_scan, B, p, CloudRequest{}, &plan))) return rc;
  rpl::VoxelLaunch v{d_nodes, n_stride, d_n_per_scan, B};
  v.arena = d_arena;
  v.arena_capacity = arena_capacity;
  v.arena_cursor = d_cursor;
  v.scan_start = d_scan_start;
  v.form = xyi ? rpl::ArenaForm::kXyi : rpl::ArenaForm::kXyzi;
  v.n_points = d_n_points;
  v.status = d_status;
  return run_voxel(h, plan, v);
}

int32_t rplgpu_cloud_arena_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, const rplgpu_params_t *p,
                               float *d_arena, uint64_t arena_capacity, uint64_t *d_cursor,
                               uint64_t *d_scan_start, uint32_t *d_n_points, uint32_t *d_status) {
  return cloud_arena_impl(h, d_nodes, n_stride, d_n_per_scan, B, p, d_arena, arena_capacity, d_cursor,
                          d_scan_start, d_n_points, d_status, false);
}

int32_t rplgpu_cloud_arena_xyi_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                   uint32_t n_stride, const uint32_t *d_n_per_scan, uint32_t B,
                                   const rplgpu_params_t *p, float *d_slot, uint64_t slot_points,
                                   uint64_t *d_cursor, uint64_t *d_scan_start, uint32_t *d_n_points,
                                   uint32_t *d_status) {
  return cloud_arena_impl(h, d_nodes, n_stride, d_n_per_scan, B, p, d_slot, slot_points, d_cursor,
                          d_scan_start, d_n_points, d_status, true);
}

// E8 (rplgpu_cloud_fused_voxel_dev) and its cell-record form (rplgpu_cloud_fused_cells_dev, include/rplgpu_comm.h):
// `cells` = the arena holds rplgpu_cell_t records, capacity in records
static int32_t fused_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                          const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                          const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                          float *d_arena, uint64_t arena_capacity, uint64_t *d_cursor,
                          uint64_t *d_group_start, uint32_t *d_n_points, uint32_t *d_status,
                          bool cells) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !d_arena || !d_cursor || !d_group_start || !d_n_points || group == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (!p->voxel_enable) {
    h->err = cells ? "rplgpu_cloud_fused_cells_dev needs voxel_enable" : "rplgpu_cloud_fused_voxel_dev needs voxel_enable";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((d_motion && !device_readable(h, d_motion, "d_motion")) ||
      (d_pose2d && !device_readable(h, d_pose2d, "d_pose2d")))
    return RPLGPU_ERR_INVALID_ARG;
  if (h->scan_t0 && !d_motion) {
    h->err = "rplgpu_cloud_fused_voxel_dev: scan time offsets are set (rplgpu_set_scan_time_offsets_dev) but d_motion is NULL";
    return RPLGPU_ERR_INVALID_ARG;
  }
  // Every sample of a group can end a run record: the record stores grow (only ever grow, and
  // only here — the first call with a larger group pays one reallocation) to group x stride.
  group = std::min(group, B);  // "all sensors in one grid" may be asked for with any group >= B
  const uint64_t need = rpl::voxel_store_need(group, n_stride);
  if (need > h->vstore_recs) {
    if (need > (1ull << 24)) {
      h->err = "rplgpu_cloud_fused_voxel_dev: group x n_stride above 2^24 samples";
      return RPLGPU_ERR_CAPACITY;
    }
    RPL_HIP(h, hipSetDevice(h->device));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    void *bigger = nullptr;
    if (hipMalloc(&bigger, (size_t)h->vstore_wgs * need * 32u) != hipSuccess) {
      h->err = "record store allocation failed";
      (void)hipGetLastError();
      return RPLGPU_ERR_HIP;
    }
    (void)hipFree(h->d_vstore);
    h->d_vstore = bigger;
    h->vstore_recs = (uint32_t)need;
  }
  CloudRequest req;
  req.group = group;
  req.cells = cells;
  CloudPlan plan;
  if ((rc = prepare_cloud(h, d_nodes, n_stride, d_n_per_scan, B, p, req, &plan))) return rc;
  rpl::VoxelLaunch v{d_nodes, n_stride, d_n_per_scan, B};
  v.group = group;
  v.motion = d_motion;
  v.pose2d = d_pose2d;
  v.arena = d_arena;
  v.arena_capacity = arena_capacity;
  v.arena_cursor = d_cursor;
  v.scan_start = d_group_start;
  v.form = cells ? rpl::ArenaForm::kCells : rpl::ArenaForm::kXyzi;
  v.n_points = d_n_points;
  v.status = d_status;
  return run_voxel(h, plan, v);
}

int32_t rplgpu_cloud_fused_voxel_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                     uint32_t n_stride, const uint32_t *d_n_per_scan, uint32_t B,
                                     uint32_t group, const rplgpu_params_t *p,
                                     const float *d_motion, const float *d_pose2d, float *d_arena,
                                     uint64_t arena_capacity, uint64_t *d_cursor,
                                     uint64_t *d_group_start, uint32_t *d_n_points,
                                     uint32_t *d_status) {
  return fused_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, d_arena,
                    arena_capacity, d_cursor, d_group_start, d_n_points, d_status, false);
}

int32_t rplgpu_cloud_fused_cells_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                     uint32_t n_stride, const uint32_t *d_n_per_scan, uint32_t B,
                                     uint32_t group, const rplgpu_params_t *p,
                                     const float *d_motion, const float *d_pose2d,
                                     rplgpu_cell_t *d_cells, uint64_t cells_capacity,
                                     uint64_t *d_cursor, uint64_t *d_group_start,
                                     uint32_t *d_n_cells, uint32_t *d_status) {
  return fused_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d,
                    reinterpret_cast<float *>(d_cells), cells_capacity, d_cursor, d_group_start, d_n_cells,
                    d_status, true);
}

// (`req`: how rplgpu_scan_to_cloud drives this over the handle's own staging; the batch entry point: defaults)
static int32_t cloud_batch_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                const uint32_t *d_n_per_scan, uint32_t B, const rplgpu_params_t *p,
                                float *d_xyzi, uint32_t out_stride, uint32_t *d_n_points,
                                uint32_t *d_status, const CloudRequest &req) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B, req.own_buffers);
  if (rc) return rc;
  if (!p || !d_xyzi || !d_n_points || out_stride == 0) return RPLGPU_ERR_INVALID_ARG;
  CloudPlan plan;
  if ((rc = prepare_cloud(h, d_nodes, n_stride, d_n_per_scan, B, p, req, &plan))) return rc;
  if (!p->voxel_enable) {
    RPL_HIP(h, rpl::launch_cloud(h->stream, d_nodes, n_stride, d_n_per_scan, B, plan.kp, plan.T, plan.mask,
                                 kMaskStride, d_xyzi, out_stride, d_n_points, d_status));
    return RPLGPU_OK;
  }
  rpl::VoxelLaunch v{d_nodes, n_stride, d_n_per_scan, B};
  v.xyzi = d_xyzi;
  v.out_stride = out_stride;
  v.n_points = d_n_points;
  v.status = d_status;
  return run_voxel(h, plan, v, req.defer_listed && d_status);
}

int32_t rplgpu_cloud_batch_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, const rplgpu_params_t *p,
                               float *d_xyzi, uint32_t out_stride, uint32_t *d_n_points,
                               uint32_t *d_status) {
  return cloud_batch_impl(h, d_nodes, n_stride, d_n_per_scan, B, p, d_xyzi, out_stride, d_n_points, d_status,
                          CloudRequest{});
}

int32_t rplgpu_pack_clouds_dev(rplgpu_handle_t h, const float *d_xyzi, uint32_t out_stride,
                               const uint32_t *d_n_points, uint32_t B, float *d_packed,
                               uint64_t *d_offsets) {
  if (!h || !d_offsets) return RPLGPU_ERR_INVALID_ARG;
  if (B && (!d_xyzi || !d_n_points || !d_packed)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_pack(h->stream, d_xyzi, out_stride, d_n_points, B, d_packed, d_offsets));
  return RPLGPU_OK;
}

// ---- single scan, host buffers ----------------------------------------------------

int32_t rplgpu_ascend(rplgpu_handle_t h, rplgpu_node_t *nodes, size_t n, uint32_t *sl_result) {
  if (!h || (!nodes && n)) return RPLGPU_ERR_INVALID_ARG;
  if (n > h->max_n) return RPLGPU_ERR_CAPACITY;
  if (n == 0) {  // 0 == count -> SL_RESULT_OPERATION_FAIL (src/sdk/src/sl_lidar_driver.cpp:151)
    if (sl_result) *sl_result = 0x80008001u;
    return RPLGPU_OK;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  if (h->zero_copy) {  // in place in the pinned staging: one launch pair, one synchronisation
    const ScanStage st = stage_scan(h, nodes, n);
    uint32_t *d_status = const_cast<uint32_t *>(st.d_n) + 1;
    RPL_HIP(h, rpl::launch_ascend(h->stream, const_cast<rplgpu_node_t *>(st.d_nodes), (uint32_t)n,
                                  st.d_n, 1, d_status, h->d_small + 20, /*defer_sort=*/true));
    if (int32_t wrc = wait_scan(h)) return wrc;
    uint32_t stw;
    std::memcpy(&stw, h->h_pin + n * 8 + 4, 4);
    if (stw & rpl::kAscendUnsorted) {  // (rare: the filled angles do not ascend) the sorting kernel after all
      RPL_HIP(h, rpl::launch_ascend_sort(h->stream, const_cast<rplgpu_node_t *>(st.d_nodes), (uint32_t)n,
                                         st.d_n, 1, d_status, h->d_small + 20));
      if (int32_t wrc = wait_scan(h)) return wrc;
      std::memcpy(&stw, h->h_pin + n * 8 + 4, 4);
    }
    const bool all_invalid = (stw & RPLGPU_SCAN_ALL_INVALID) != 0;
    if (!all_invalid) std::memcpy(nodes, h->h_pin, n * 8);
    if (sl_result) *sl_result = all_invalid ? 0x80008001u : 0u;
    return RPLGPU_OK;
  }
  const uint32_t *d_n;
  if (int32_t rc = upload_scan(h, nodes, n, &d_n)) return rc;
  uint32_t *d_status = const_cast<uint32_t *>(d_n) + 1;  // travels back with the nodes
  RPL_HIP(h, rpl::launch_ascend(h->stream, h->d_nodes, (uint32_t)n, d_n, 1, d_status,
                                h->d_small + 20));
  RPL_HIP(h, hipMemcpyAsync(h->h_pin, h->d_nodes, n * 8 + 8, hipMemcpyDeviceToHost, h->stream));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  uint32_t st;
  std::memcpy(&st, h->h_pin + n * 8 + 4, 4);
  const bool all_invalid = (st & RPLGPU_SCAN_ALL_INVALID) != 0;
  if (!all_invalid) std::memcpy(nodes, h->h_pin, n * 8);
  if (sl_result) *sl_result = all_invalid ? 0x80008001u : 0u;
  return RPLGPU_OK;
}

int32_t rplgpu_scan_to_laserscan(rplgpu_handle_t h, const rplgpu_node_t *nodes, size_t n,
                                 const rplgpu_params_t *p, double scan_duration, float *ranges,
                                 float *intensities, rplgpu_scan_meta_t *meta) {
  if (!h || !p || !meta || (n && (!nodes || !ranges || !intensities))) return RPLGPU_ERR_INVALID_ARG;
  if (n > h->max_n) return RPLGPU_ERR_CAPACITY;
  std::memset(meta, 0, sizeof(*meta));
  if (n == 0) return RPLGPU_OK;  // :561-563
  RPL_HIP(h, hipSetDevice(h->device));
  if (h->zero_copy) {
    const ScanStage st = stage_scan(h, nodes, n);
    float *d_r = reinterpret_cast<float *>(st.d_out);
    float *d_i = d_r + n;
    uint32_t *d_count = reinterpret_cast<uint32_t *>(d_i + n);
    if (int32_t lrc = run_laserscan(h, st.d_nodes, (uint32_t)n, st.d_n, 1, *p, d_r, d_i, d_count, (uint32_t)n))
      return lrc;
    if (int32_t wrc = wait_scan(h)) return wrc;
    uint32_t count;
    std::memcpy(&count, st.h_out + n * 8, 4);
    rplgpu_fill_meta(p, count, scan_duration, meta);
    if (count) {
      std::memcpy(ranges, st.h_out, (size_t)count * 4);
      std::memcpy(intensities, st.h_out + n * 4, (size_t)count * 4);
    }
    return RPLGPU_OK;
  }
  unsigned char *h_out = stage_out(h);
  const uint32_t *d_n;
  if (int32_t rc = upload_scan(h, nodes, n, &d_n)) return rc;
  float *d_r = reinterpret_cast<float *>(h->d_out);
  float *d_i = d_r + n;
  uint32_t *d_count = reinterpret_cast<uint32_t *>(d_i + n);  // travels back with the arrays
  if (int32_t lrc = run_laserscan(h, h->d_nodes, (uint32_t)n, d_n, 1, *p, d_r, d_i, d_count))
    return lrc;
  RPL_HIP(h, hipMemcpyAsync(h_out, h->d_out, n * 8 + 4, hipMemcpyDeviceToHost, h->stream));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  uint32_t count;
  std::memcpy(&count, h_out + n * 8, 4);
  rplgpu_fill_meta(p, count, scan_duration, meta);
  if (count) {
    std::memcpy(ranges, h_out, (size_t)count * 4);
    std::memcpy(intensities, h_out + n * 4, (size_t)count * 4);
  }
  return RPLGPU_OK;
}

int32_t rplgpu_scan_to_cloud(rplgpu_handle_t h, const rplgpu_node_t *nodes, size_t n,
                             const rplgpu_params_t *p, float *xyzi, uint32_t *n_points,
                             uint32_t *status) {
  if (!h || !p || !n_points || (n && (!nodes || !xyzi))) return RPLGPU_ERR_INVALID_ARG;
  if (n > h->max_n) return RPLGPU_ERR_CAPACITY;
  *n_points = 0;
  if (status) *status = 0;
  if (n == 0) return RPLGPU_OK;
  unsigned char *h_out = stage_out(h);
  uint32_t w[2];  // n_points, status: they travel behind the points
  RPL_HIP(h, hipSetDevice(h->device));
  if (h->zero_copy) {
    const ScanStage st = stage_scan(h, nodes, n);
    uint32_t *d_words = reinterpret_cast<uint32_t *>(st.d_out + n * 16);
    const rplgpu_node_t *d_in = st.d_nodes;
    const uint32_t *d_in_n = st.d_n;
    if (p->ror_enable) {
      // E5 reads a scan many times: it wants it in HBM.  The staged nodes and their count word
      // are brought over by a kernel of the same stream (not the copy engine), the results go
      // straight to the pinned staging as in the plain case.
      RPL_HIP(h, rpl::launch_stage_in(h->stream, st.d_nodes, h->d_nodes, (uint32_t)n + 1u));
      d_in = reinterpret_cast<const rplgpu_node_t *>(h->d_nodes);
      d_in_n = reinterpret_cast<const uint32_t *>(h->d_nodes + n * 8);
    }
    // (E5 + E4: the voxel kernel applies E5 itself, round 6; a scan it cannot settle comes back with the
    // internal "listed" status and is redone by the two kernels — this call waits for its scan anyway)
    // (Only for dense scans: below ~8 k samples per revolution the index neighbours of a sample are mostly
    // farther away than r — 360 samples at 10 m are 17 cm apart — the kernel gives the scan up at once and
    // the call would pay for both paths: 87 against 59 us at 360 samples, 61 against 73 us at 32 000.)
    CloudRequest req;
    req.own_buffers = true;
    req.force_two_kernels = n < 8192u;
    req.defer_listed = true;
    for (int pass = 0; pass < 2; ++pass) {  // (the second one: the two kernels, which list nothing)
      if (int32_t rc = cloud_batch_impl(h, d_in, (uint32_t)n, d_in_n, 1, p, reinterpret_cast<float *>(st.d_out),
                                        (uint32_t)n, d_words, d_words + 1, req))
        return rc;
      if (int32_t wrc = wait_scan(h)) return wrc;
      std::memcpy(w, h_out + n * 16, 8);
      if (!(w[1] & rpl::kRorListedBit)) break;
      req.force_two_kernels = true;
      req.defer_listed = false;
    }
  } else {
    // (E5 follows the handle's mode at every size here: rplgpu_cloud_batch_dev with B = 1)
    const uint32_t *d_n;
    if (int32_t urc = upload_scan(h, nodes, n, &d_n)) return urc;
    uint32_t *d_words = reinterpret_cast<uint32_t *>(h->d_out + n * 16);
    int32_t rc = rplgpu_cloud_batch_dev(h, reinterpret_cast<const rplgpu_node_t *>(h->d_nodes),
                                        (uint32_t)n, d_n, 1, p, reinterpret_cast<float *>(h->d_out),
                                        (uint32_t)n, d_words, d_words + 1);
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(h_out, h->d_out, n * 16 + 8, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(w, h_out + n * 16, 8);
  }
  *n_points = w[0];
  if (status) *status = w[1];
  std::memcpy(xyzi, h_out, (size_t)w[0] * 16);
  return (w[1] & (RPLGPU_SCAN_CELL_RANGE | RPLGPU_SCAN_TABLE_FULL)) ? RPLGPU_ERR_SCAN_OVERFLOW : RPLGPU_OK;
}

// ---- decode stage ------------------------------------------

size_t rplgpu_frame_size(uint8_t ans_type) {
  switch (ans_type) {  // packed wire structs, src/sdk/include/sl_lidar_cmd.h:189-286
    case RPLGPU_ANS_MEASUREMENT: return 5;
    case RPLGPU_ANS_CAPSULED: return 84;
    case RPLGPU_ANS_HQ: return 781;
    case RPLGPU_ANS_CAPSULED_ULTRA: return 132;
    case RPLGPU_ANS_DENSE_CAPSULED: return 84;
    case RPLGPU_ANS_ULTRA_DENSE_CAPSULED: return 170;
    default: return 0;
  }
}

size_t rplgpu_nodes_per_frame(uint8_t ans_type) {
  switch (ans_type) {
    case RPLGPU_ANS_MEASUREMENT: return 1;
    case RPLGPU_ANS_CAPSULED: return 32;
    case RPLGPU_ANS_HQ: return 96;
    case RPLGPU_ANS_CAPSULED_ULTRA: return 96;
    case RPLGPU_ANS_DENSE_CAPSULED: return 40;
    case RPLGPU_ANS_ULTRA_DENSE_CAPSULED: return 64;
    default: return 0;
  }
}

uint32_t rplgpu_decode_max_frames(uint8_t ans_type) {
  return rplgpu_frame_size(ans_type) ? rpl::decode_max_frames(ans_type) : 0u;
}
uint32_t rplgpu_decode_staged_frames(uint8_t ans_type) {
  return rplgpu_frame_size(ans_type) ? rpl::decode_staged_frames(ans_type) : 0u;
}

// Framing = what the first two switch cases of every onData loop decide
// (handler_capsules.cpp:107-135 and siblings, handler_hqnode.cpp:99-113,
// handler_normalnode.cpp:88-112): a frame starts at a byte accepted in position 0 whose
// successor is accepted in position 1; rejected bytes are dropped one at a time (a byte
// rejected in position 1 is dropped together with the pending position-0 byte's claim, it is
// not reconsidered as a start).  Sequential by nature, a few ns per byte, so it runs on the
// host; the GPU gets (offset, gap) per frame.
size_t rplgpu_frame_stream(uint8_t ans_type, const uint8_t *bytes, size_t nbytes,
                           uint32_t *frame_off, uint8_t *gap, size_t cap) {
  const size_t S = rplgpu_frame_size(ans_type);
  if (!S || (!bytes && nbytes)) return 0;
  const bool hq = ans_type == RPLGPU_ANS_HQ, legacy = ans_type == RPLGPU_ANS_MEASUREMENT;
  size_t found = 0, i = 0;
  uint8_t dirty = 0;
  while (i < nbytes) {
    const uint8_t b0 = bytes[i];
    const bool start_ok = hq ? (b0 == 0xA5u) : legacy ? ((((b0 >> 1) ^ b0) & 1u) != 0u)
                                                      : ((b0 >> 4) == 0xAu);
    if (!start_ok) {
      dirty = 1;
      ++i;
      continue;
    }
    if (!hq) {
      if (i + 1 >= nbytes) break;  // the second byte has not arrived yet
      const uint8_t b1 = bytes[i + 1];
      const bool second_ok = legacy ? ((b1 & 1u) != 0u) : ((b1 >> 4) == 0x5u);
      if (!second_ok) {
        dirty = 1;
        i += 2;  // both bytes are consumed
        continue;
      }
    }
    if (i + S > nbytes) break;  // incomplete trailing frame stays in the reference's cache
    if (found < cap) {
      if (frame_off) frame_off[found] = (uint32_t)i;
      if (gap) gap[found] = dirty;
    }
    ++found;
    dirty = 0;
    i += S;
  }
  return found;
}

// the part of a decode call every decode door takes from its caller as it is: the streams and the carried state
static rpl::DecodeLaunch decode_input(uint8_t ans_type, uint32_t sample_duration_us, const uint8_t *d_bytes,
                                      uint64_t stream_stride, const uint32_t *d_frame_off,
                                      const uint8_t *d_gap, const uint32_t *d_n_frames, uint32_t max_frames,
                                      uint32_t B, const int32_t *d_state_in, int32_t *d_state_out) {
  rpl::DecodeLaunch d;
  d.ans = ans_type;
  d.bytes = d_bytes;
  d.stream_stride = stream_stride;
  d.frame_off = d_frame_off;
  d.gap = d_gap;
  d.n_frames = d_n_frames;
  d.max_frames = max_frames;
  d.B = B;
  d.sample_duration_us = sample_duration_us;
  d.state_in = d_state_in;
  d.state_out = d_state_out;
  return d;
}

int32_t rplgpu_decode_batch_dev(rplgpu_handle_t h, uint8_t ans_type, uint32_t sample_duration_us,
                                const uint8_t *d_bytes, uint64_t stream_stride,
                                const uint32_t *d_frame_off, const uint8_t *d_gap,
                                const uint32_t *d_n_frames, uint32_t max_frames, uint32_t B,
                                const int32_t *d_state_in, int32_t *d_state_out,
                                rplgpu_node_t *d_nodes, uint32_t node_stride, uint32_t *d_n_nodes,
                                uint32_t *d_reset_at, uint32_t reset_stride, uint32_t *d_n_reset,
                                uint32_t *d_n_errors, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (!rplgpu_frame_size(ans_type)) return RPLGPU_ERR_INVALID_ARG;
  // the dense / ultra-dense discard threshold divides by 1000000 / sample_duration_us
  // (handler_capsules.cpp:750, :971): zero or > 1 s would divide by zero in the reference too
  if (sample_duration_us == 0 || sample_duration_us > 1000000u) return RPLGPU_ERR_INVALID_ARG;
  if (B && (!d_bytes || !d_n_frames || !d_nodes || !d_n_nodes)) return RPLGPU_ERR_INVALID_ARG;
  if (d_gap && !d_frame_off) return RPLGPU_ERR_INVALID_ARG;
  if (max_frames > rpl::decode_max_frames(ans_type)) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  if (B && (!device_readable(h, d_bytes, "d_bytes") || !device_readable(h, d_n_frames, "d_n_frames") ||
            (d_frame_off && !device_readable(h, d_frame_off, "d_frame_off"))))
    return RPLGPU_ERR_INVALID_ARG;
  uint32_t *stage_todo = nullptr;
  if (d_frame_off && h->dec_stage && max_frames <= rpl::decode_staged_frames(ans_type)) {
    if (h->dec_todo_cap < B) {  // (grows when a larger call arrives, never shrinks)
      RPL_HIP(h, hipStreamSynchronize(h->stream));
      if (h->d_dec_todo) (void)hipFree(h->d_dec_todo);
      h->d_dec_todo = nullptr;
      h->dec_todo_cap = 0;
      RPL_HIP(h, hipMalloc((void **)&h->d_dec_todo, (size_t)B * sizeof(uint32_t)));
      h->dec_todo_cap = B;
    }
    stage_todo = h->d_dec_todo;
  }
  rpl::DecodeLaunch d = decode_input(ans_type, sample_duration_us, d_bytes, stream_stride, d_frame_off,
                                     d_gap, d_n_frames, max_frames, B, d_state_in, d_state_out);
  d.nodes = d_nodes;
  d.node_stride = node_stride;
  d.n_nodes = d_n_nodes;
  d.reset_at = d_reset_at;
  d.reset_stride = reset_stride;
  d.n_reset = d_n_reset;
  d.n_errors = d_n_errors;
  d.status = d_status;
  d.staged_ok = h->dec_stage;
  d.stage_todo = stage_todo;
  RPL_HIP(h, rpl::launch_decode(h->stream, d));
  return RPLGPU_OK;
}

static int32_t decode_scans_impl(rplgpu_handle_t h, uint8_t ans_type, uint32_t sample_duration_us,
                                const uint8_t *d_bytes, uint64_t stream_stride,
                                const uint32_t *d_frame_off, const uint8_t *d_gap,
                                const uint32_t *d_n_frames, uint32_t max_frames, uint32_t B,
                                const int32_t *d_state_in, int32_t *d_state_out,
                                uint32_t max_count, rplgpu_node_t *d_batch, uint32_t n_stride,
                                uint32_t scan_cap, uint32_t *d_n_per_scan, uint32_t *d_n_scans,
                                uint32_t *d_n_errors, uint32_t *d_status,
                                const rplgpu_node_t *d_carry_in, const uint32_t *d_carry_len_in,
                                rplgpu_node_t *d_carry_out, uint32_t *d_carry_len_out,
                                uint32_t carry_stride) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  const bool carry = d_carry_out != nullptr;
  if (carry) {
    if (!d_carry_len_out || carry_stride == 0 || (d_carry_in == nullptr) != (d_carry_len_in == nullptr) ||
        d_carry_in == d_carry_out)
      return RPLGPU_ERR_INVALID_ARG;
  }
  const size_t npf = rplgpu_nodes_per_frame(ans_type);
  if (!npf || max_count == 0 || scan_cap == 0 || n_stride == 0) return RPLGPU_ERR_INVALID_ARG;
  if (sample_duration_us == 0 || sample_duration_us > 1000000u) return RPLGPU_ERR_INVALID_ARG;
  if (B && (!d_bytes || !d_n_frames || !d_batch || !d_n_per_scan || !d_n_scans || !d_status))
    return RPLGPU_ERR_INVALID_ARG;
  if (d_gap && !d_frame_off) return RPLGPU_ERR_INVALID_ARG;
  if (max_frames == 0 || max_frames > rpl::decode_max_frames(ans_type)) return RPLGPU_ERR_CAPACITY;
  if ((uint64_t)max_frames * npf > 0x7FFFFFFFull || (uint64_t)B * scan_cap > 0xFFFFFFFFull)
    return RPLGPU_ERR_CAPACITY;
  if (scan_cap > 65535u) return RPLGPU_ERR_CAPACITY;  // (a grid dimension of k_assemble)
  if (B == 0) return RPLGPU_OK;
  RPL_HIP(h, hipSetDevice(h->device));
  if (!device_readable(h, d_bytes, "d_bytes") || !device_readable(h, d_n_frames, "d_n_frames") ||
      (d_frame_off && !device_readable(h, d_frame_off, "d_frame_off")) ||
      !device_readable(h, d_batch, "d_batch") || !device_readable(h, d_n_per_scan, "d_n_per_scan") ||
      !device_readable(h, d_n_scans, "d_n_scans") || !device_readable(h, d_status, "d_status") ||
      (d_n_errors && !device_readable(h, d_n_errors, "d_n_errors")) ||
      (d_state_in && !device_readable(h, d_state_in, "d_state_in")) ||
      (d_state_out && !device_readable(h, d_state_out, "d_state_out")))
    return RPLGPU_ERR_INVALID_ARG;
  // scratch kept in the handle (grows when a larger call arrives, never shrinks): the decoded
  // node streams, the decoder's sync-node and reset lists, three counters per stream
  const uint32_t node_stride = (uint32_t)((size_t)max_frames * npf);
  const uint32_t sync_stride = rpl::decode_sync_stride();
  const uint32_t reset_stride = std::min<uint32_t>(max_frames, 2048u);  // a frame requests at most one reset
  auto up256 = [](size_t v) { return (v + 255) & ~size_t(255); };
  const size_t sz_nodes = up256((size_t)B * node_stride * 8), sz_sync = up256((size_t)B * sync_stride * 4);
  const size_t sz_rst = up256((size_t)B * reset_stride * 4), sz_cnt = up256((size_t)B * 4);
  const size_t need = sz_nodes + sz_sync + sz_rst + 5 * sz_cnt;
  if (h->scans_cap < need) {
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    if (h->d_scans) (void)hipFree(h->d_scans);
    h->d_scans = nullptr;
    h->scans_cap = 0;
    RPL_HIP(h, hipMalloc((void **)&h->d_scans, need));
    h->scans_cap = need;
  }
  unsigned char *p = h->d_scans;
  rplgpu_node_t *t_nodes = reinterpret_cast<rplgpu_node_t *>(p);
  uint32_t *t_sync = reinterpret_cast<uint32_t *>(p + sz_nodes);
  uint32_t *t_rst = reinterpret_cast<uint32_t *>(p + sz_nodes + sz_sync);
  uint32_t *t_nn = reinterpret_cast<uint32_t *>(p + sz_nodes + sz_sync + sz_rst);
  uint32_t *t_nr = t_nn + sz_cnt / 4, *t_ns = t_nr + sz_cnt / 4, *t_todo = t_ns + sz_cnt / 4;
  uint32_t *t_stage_todo = t_todo + sz_cnt / 4;  // (the staged decoder's own list, see launch_decode)
  // express / ultra / dense: the fused decoder knows the scan boundaries from the capsule headers
  // and writes the nodes of completed scans straight into their batch slots; a stream with more
  // sync nodes / reset requests than its tables hold raises t_todo[b] and takes the general path
  // below (decode to the node stream, then assemble), which skips every stream already done.
  rpl::DecodeLaunch d = decode_input(ans_type, sample_duration_us, d_bytes, stream_stride, d_frame_off,
                                     d_gap, d_n_frames, max_frames, B, d_state_in, d_state_out);
  d.nodes = t_nodes;
  d.node_stride = node_stride;
  d.n_nodes = t_nn;
  d.reset_at = t_rst;
  d.reset_stride = reset_stride;
  d.n_reset = t_nr;
  d.sync_at = t_sync;
  d.sync_stride = sync_stride;
  d.n_sync = t_ns;
  d.n_errors = d_n_errors;
  d.status = d_status;
  d.max_count = max_count;
  d.batch = d_batch;
  d.n_stride = n_stride;
  d.scan_cap = scan_cap;
  d.n_per_scan = d_n_per_scan;
  d.n_scans = d_n_scans;
  d.todo = t_todo;
  d.staged_ok = h->dec_stage;
  d.stage_todo = d_frame_off ? t_stage_todo : nullptr;
  // (with a carried scan every stream takes the general path: the fused decoder neither decodes
  // the nodes in front of a call's first sync node nor those behind its last)
  if (!carry && rpl::decode_fusable(ans_type)) {
    RPL_HIP(h, rpl::launch_decode_fused(h->stream, d));
    d.only = t_todo;
  }
  RPL_HIP(h, rpl::launch_decode(h->stream, d));
  const uint32_t *only = d.only;
  RPL_HIP(h, rpl::launch_assemble(h->stream, t_nodes, node_stride, t_nn, t_sync, sync_stride, t_ns,
                                  t_rst, reset_stride, t_nr, B, max_count, d_batch, n_stride,
                                  scan_cap, d_n_per_scan, d_n_scans, d_status, only, d_carry_in,
                                  d_carry_out, d_carry_len_in, d_carry_len_out, carry_stride));
  return RPLGPU_OK;
}

int32_t rplgpu_decode_scans_dev(rplgpu_handle_t h, uint8_t ans_type, uint32_t sample_duration_us,
                                const uint8_t *d_bytes, uint64_t stream_stride,
                                const uint32_t *d_frame_off, const uint8_t *d_gap,
                                const uint32_t *d_n_frames, uint32_t max_frames, uint32_t B,
                                const int32_t *d_state_in, int32_t *d_state_out,
                                uint32_t max_count, rplgpu_node_t *d_batch, uint32_t n_stride,
                                uint32_t scan_cap, uint32_t *d_n_per_scan, uint32_t *d_n_scans,
                                uint32_t *d_n_errors, uint32_t *d_status) {
  return decode_scans_impl(h, ans_type, sample_duration_us, d_bytes, stream_stride, d_frame_off, d_gap,
                           d_n_frames, max_frames, B, d_state_in, d_state_out, max_count, d_batch,
                           n_stride, scan_cap, d_n_per_scan, d_n_scans, d_n_errors, d_status, nullptr,
                           nullptr, nullptr, nullptr, 0u);
}

int32_t rplgpu_decode_scans_carry_dev(rplgpu_handle_t h, uint8_t ans_type,
                                      uint32_t sample_duration_us, const uint8_t *d_bytes,
                                      uint64_t stream_stride, const uint32_t *d_frame_off,
                                      const uint8_t *d_gap, const uint32_t *d_n_frames,
                                      uint32_t max_frames, uint32_t B, const int32_t *d_state_in,
                                      int32_t *d_state_out, uint32_t max_count,
                                      rplgpu_node_t *d_batch, uint32_t n_stride, uint32_t scan_cap,
                                      uint32_t *d_n_per_scan, uint32_t *d_n_scans,
                                      uint32_t *d_n_errors, uint32_t *d_status,
                                      const rplgpu_node_t *d_carry_in, const uint32_t *d_carry_len_in,
                                      rplgpu_node_t *d_carry_out, uint32_t *d_carry_len_out,
                                      uint32_t carry_stride) {
  if (!d_carry_out) return RPLGPU_ERR_INVALID_ARG;
  if (h && B) {
    if (!device_readable(h, d_carry_out, "d_carry_out") ||
        !device_readable(h, d_carry_len_out, "d_carry_len_out") ||
        (d_carry_in && (!device_readable(h, d_carry_in, "d_carry_in") ||
                        !device_readable(h, d_carry_len_in, "d_carry_len_in"))))
      return RPLGPU_ERR_INVALID_ARG;
  }
  return decode_scans_impl(h, ans_type, sample_duration_us, d_bytes, stream_stride, d_frame_off, d_gap,
                           d_n_frames, max_frames, B, d_state_in, d_state_out, max_count, d_batch,
                           n_stride, scan_cap, d_n_per_scan, d_n_scans, d_n_errors, d_status,
                           d_carry_in, d_carry_len_in, d_carry_out, d_carry_len_out, carry_stride);
}

int32_t rplgpu_segment_batch_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                 uint32_t node_stride, const uint32_t *d_n_nodes,
                                 const uint32_t *d_reset_at, uint32_t reset_stride,
                                 const uint32_t *d_n_reset, uint32_t B, uint32_t max_count,
                                 rplgpu_node_t *d_out_nodes, uint32_t out_stride,
                                 uint32_t *d_scan_off, uint32_t scan_cap, uint32_t *d_n_scans,
                                 uint32_t *d_status) {
  if (!h || max_count == 0) return RPLGPU_ERR_INVALID_ARG;
  if (B && (!d_nodes || !d_n_nodes || !d_out_nodes || !d_scan_off || !d_n_scans))
    return RPLGPU_ERR_INVALID_ARG;
  if ((d_reset_at == nullptr) != (d_n_reset == nullptr)) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_segment(h->stream, d_nodes, node_stride, d_n_nodes, d_reset_at,
                                 reset_stride, d_n_reset, B, max_count, d_out_nodes, out_stride,
                                 d_scan_off, scan_cap, d_n_scans, d_status));
  return RPLGPU_OK;
}

int32_t rplgpu_scans_to_batch_dev(rplgpu_handle_t h, const rplgpu_node_t *d_seg_nodes,
                                  uint32_t seg_stride, const uint32_t *d_scan_off,
                                  uint32_t scan_cap, const uint32_t *d_n_scans, uint32_t B,
                                  uint32_t *d_scan_base, rplgpu_node_t *d_batch, uint32_t n_stride,
                                  uint32_t max_scans, uint32_t *d_n_per_scan) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (B && (!d_seg_nodes || !d_scan_off || !d_n_scans || !d_scan_base || !d_batch || !d_n_per_scan))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_scans_to_batch(h->stream, d_seg_nodes, seg_stride, d_scan_off, scan_cap,
                                        d_n_scans, B, d_scan_base, d_batch, n_stride, max_scans,
                                        d_n_per_scan));
  return RPLGPU_OK;
}

int32_t rplgpu_decode_stream(rplgpu_handle_t h, uint8_t ans_type, uint32_t sample_duration_us,
                             const uint8_t *bytes, size_t nbytes, int32_t state[4],
                             rplgpu_node_t *nodes, size_t cap, size_t *n_nodes,
                             uint32_t *reset_at, size_t reset_cap, size_t *n_reset,
                             uint32_t *n_errors) {
  if (!h || !n_nodes || (nbytes && !bytes) || (cap && !nodes)) return RPLGPU_ERR_INVALID_ARG;
  const size_t S = rplgpu_frame_size(ans_type), npf = rplgpu_nodes_per_frame(ans_type);
  if (!S) return RPLGPU_ERR_INVALID_ARG;
  *n_nodes = 0;
  if (n_reset) *n_reset = 0;
  if (n_errors) *n_errors = 0;
  if (nbytes >= 0xFFFFFFFFull) return RPLGPU_ERR_CAPACITY;
  const size_t max_f = nbytes / S;
  std::vector<uint32_t> off(max_f ? max_f : 1);
  std::vector<uint8_t> gap(max_f ? max_f : 1);
  const size_t nf = rplgpu_frame_stream(ans_type, bytes, nbytes, off.data(), gap.data(), max_f);
  if (nf == 0) return RPLGPU_OK;
  RPL_HIP(h, hipSetDevice(h->device));
  const bool caps = ans_type != RPLGPU_ANS_MEASUREMENT && ans_type != RPLGPU_ANS_HQ;
  const size_t piece = std::min<size_t>(nf, rpl::decode_max_frames(ans_type));
  // device staging kept in the handle (grown when a longer recording arrives, never shrunk):
  // every sub-buffer starts on a 16-byte boundary (the decoder stores nodes as 8-byte words)
  const size_t node_cap = piece * npf, rcap = piece + 1;
  const size_t sz_bytes = up16(nbytes), sz_off = up16(piece * 4), sz_gap = up16(piece);
  const size_t sz_nodes = up16(node_cap * 8), sz_rst = up16(rcap * 4), sz_small = 128;
  const size_t need = sz_bytes + sz_off + sz_gap + sz_nodes + sz_rst + sz_small;
  if (h->dec_cap < need) {
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    if (h->d_dec) (void)hipFree(h->d_dec);
    h->d_dec = nullptr;
    h->dec_cap = 0;
    RPL_HIP(h, hipMalloc((void **)&h->d_dec, need));
    h->dec_cap = need;
  }
  unsigned char *d = h->d_dec;
  unsigned char *d_b = d, *d_off = d_b + sz_bytes, *d_gap = d_off + sz_off;
  unsigned char *d_nodes = d_gap + sz_gap, *d_rst = d_nodes + sz_nodes, *d_small = d_rst + sz_rst;
  // d_small (u32): [0] n_frames [1] n_nodes [2] n_reset [3] n_err [4] status
  //                [8..11] state in, [12..15] state out
  int32_t rc = RPLGPU_OK;
  auto fail = [&](hipError_t e, const char *what) {
    h->err = std::string(what) + ": " + hipGetErrorString(e);
    rc = RPLGPU_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipMemcpyAsync(d_b, bytes, nbytes, hipMemcpyHostToDevice, h->stream)) != hipSuccess) fail(e, "copy bytes");
  int32_t st[4] = {state ? state[0] : 0, state ? state[1] : 0, 0, 0};
  size_t done_nodes = 0, done_resets = 0, errs = 0;
  std::vector<uint32_t> rst_host(rcap);
  // pieces of at most `piece` frames; a capsule piece after the first starts one frame early
  // (flags bit 0: that frame only serves as the predecessor of the next one)
  for (size_t first = 0; first < nf && !rc;) {
    const bool overlap = caps && first > 0;
    const size_t lo = overlap ? first - 1 : first;
    const size_t cnt = std::min(piece, nf - lo);
    uint32_t small[32] = {0};
    small[0] = (uint32_t)cnt;
    small[8] = (uint32_t)st[0];
    small[9] = (uint32_t)st[1];
    small[10] = overlap ? 1u : 0u;
    if ((e = hipMemcpyAsync(d_off, off.data() + lo, cnt * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) fail(e, "copy offsets");
    if (!rc && (e = hipMemcpyAsync(d_gap, gap.data() + lo, cnt, hipMemcpyHostToDevice, h->stream)) != hipSuccess) fail(e, "copy gaps");
    if (!rc && (e = hipMemcpyAsync(d_small, small, sz_small, hipMemcpyHostToDevice, h->stream)) != hipSuccess) fail(e, "copy small");
    if (rc) break;
    uint32_t *ds = reinterpret_cast<uint32_t *>(d_small);
    rc = rplgpu_decode_batch_dev(h, ans_type, sample_duration_us, d_b, 0,
                                 reinterpret_cast<uint32_t *>(d_off), d_gap, ds, (uint32_t)cnt, 1,
                                 reinterpret_cast<int32_t *>(ds + 8), reinterpret_cast<int32_t *>(ds + 12),
                                 reinterpret_cast<rplgpu_node_t *>(d_nodes), (uint32_t)node_cap, ds + 1,
                                 reinterpret_cast<uint32_t *>(d_rst), (uint32_t)rcap, ds + 2, ds + 3, ds + 4);
    if (rc) break;
    if ((e = hipMemcpyAsync(small, d_small, sz_small, hipMemcpyDeviceToHost, h->stream)) != hipSuccess) { fail(e, "copy back"); break; }
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) { fail(e, "sync"); break; }
    const size_t got = small[1], nr = small[2];
    errs += small[3];
    st[0] = (int32_t)small[12];
    st[1] = (int32_t)small[13];
    if (got && done_nodes < cap) {
      const size_t ncopy = std::min(got, cap - done_nodes);
      if ((e = hipMemcpy(nodes + done_nodes, d_nodes, ncopy * 8, hipMemcpyDeviceToHost)) != hipSuccess) { fail(e, "copy nodes"); break; }
    }
    if (nr) {
      if ((e = hipMemcpy(rst_host.data(), d_rst, nr * 4, hipMemcpyDeviceToHost)) != hipSuccess) { fail(e, "copy resets"); break; }
      for (size_t i = 0; i < nr; ++i) {
        if (reset_at && done_resets < reset_cap) reset_at[done_resets] = (uint32_t)(rst_host[i] + done_nodes);
        ++done_resets;
      }
    }
    done_nodes += got;
    first = lo + cnt;
  }
  if (rc) return rc;
  *n_nodes = done_nodes;
  if (n_reset) *n_reset = done_resets;
  if (n_errors) *n_errors = (uint32_t)errs;
  if (state) {
    state[0] = st[0];
    state[1] = st[1];
    state[2] = 0;
    state[3] = 0;
  }
  return RPLGPU_OK;
}

// ---- serialised messages (include/rplgpu_msg.h) ------------------

int32_t rplgpu_msg_laserscan_layout(size_t frame_id_len, uint32_t count,
                                    rplgpu_laserscan_layout_t *out) {
  if (!out || frame_id_len > (1u << 20) || count > (1u << 27)) return RPLGPU_ERR_INVALID_ARG;
  rplgpu_scan_meta_t m{};
  m.count = count;
  rplmsg::Writer w(nullptr, 0);
  std::string fid(frame_id_len, 'x');
  rplmsg::write_laserscan(w, fid.data(), frame_id_len, rplgpu_stamp_t{0, 0}, m, out);
  return RPLGPU_OK;
}

int32_t rplgpu_msg_cloud_layout(size_t frame_id_len, uint32_t n_points,
                                rplgpu_cloud_layout_t *out) {
  if (!out || frame_id_len > (1u << 20) || n_points > (1u << 27)) return RPLGPU_ERR_INVALID_ARG;
  rplmsg::Writer w(nullptr, 0);
  std::string fid(frame_id_len, 'x');
  rplmsg::write_cloud(w, fid.data(), frame_id_len, rplgpu_stamp_t{0, 0}, n_points, out);
  return RPLGPU_OK;
}

int32_t rplgpu_msg_laserscan_header(const char *frame_id, rplgpu_stamp_t stamp,
                                    const rplgpu_scan_meta_t *meta, uint8_t *msg, size_t cap,
                                    rplgpu_laserscan_layout_t *layout) {
  if (!frame_id || !meta || !msg) return RPLGPU_ERR_INVALID_ARG;
  const size_t fl = std::strlen(frame_id);
  rplgpu_laserscan_layout_t L;
  if (int32_t rc = rplgpu_msg_laserscan_layout(fl, meta->count, &L)) return rc;
  if (layout) *layout = L;
  if (L.total_len > cap) return RPLGPU_ERR_CAPACITY;
  rplmsg::Writer w(msg, cap);
  rplmsg::write_laserscan(w, frame_id, fl, stamp, *meta, &L);
  return RPLGPU_OK;
}

int32_t rplgpu_msg_cloud_header(const char *frame_id, rplgpu_stamp_t stamp, uint32_t n_points,
                                uint8_t *msg, size_t cap, rplgpu_cloud_layout_t *layout) {
  if (!frame_id || !msg) return RPLGPU_ERR_INVALID_ARG;
  const size_t fl = std::strlen(frame_id);
  rplgpu_cloud_layout_t L;
  if (int32_t rc = rplgpu_msg_cloud_layout(fl, n_points, &L)) return rc;
  if (layout) *layout = L;
  if (L.total_len > cap) return RPLGPU_ERR_CAPACITY;
  rplmsg::Writer w(msg, cap);
  rplmsg::write_cloud(w, frame_id, fl, stamp, n_points, &L);
  return RPLGPU_OK;
}

int32_t rplgpu_host_alloc(rplgpu_handle_t h, size_t bytes, void **out) {
  if (!h || !out || bytes == 0) return RPLGPU_ERR_INVALID_ARG;
  *out = nullptr;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, hipHostMalloc(out, bytes, hipHostMallocDefault));
  void *dev = nullptr;
  if (hipHostGetDevicePointer(&dev, *out, 0) == hipSuccess && dev)
    h->pinned.push_back({static_cast<unsigned char *>(*out), static_cast<unsigned char *>(dev), bytes});
  return RPLGPU_OK;
}

int32_t rplgpu_host_free(rplgpu_handle_t h, void *p) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (!p) return RPLGPU_OK;
  RPL_HIP(h, hipSetDevice(h->device));
  for (size_t i = 0; i < h->pinned.size(); ++i)
    if (h->pinned[i].host == p) {
      h->pinned.erase(h->pinned.begin() + (long)i);
      break;
    }
  RPL_HIP(h, hipHostFree(p));
  return RPLGPU_OK;
}

static int32_t make_prefix(rplgpu_handle_t h, const char *frame_id, bool cloud,
                           const rplgpu_params_t *p, rplmsg::Prefix *P);

// device view of [p, p + bytes) when it lies inside a buffer from rplgpu_host_alloc, else null
static unsigned char *pinned_device_view(rplgpu_handle_t h, const void *p, size_t bytes) {
  const unsigned char *q = static_cast<const unsigned char *>(p);
  for (const auto &b : h->pinned)
    if (q >= b.host && q + bytes <= b.host + b.bytes) return b.dev + (q - b.host);
  return nullptr;
}

int32_t rplgpu_scan_to_laserscan_msg(rplgpu_handle_t h, const rplgpu_node_t *nodes, size_t n,
                                     const rplgpu_params_t *p, double scan_duration,
                                     const char *frame_id, rplgpu_stamp_t stamp, uint8_t *msg,
                                     size_t cap, size_t *msg_len, rplgpu_scan_meta_t *meta) {
  if (!h || !p || !meta || !frame_id || !msg || !msg_len || (n && !nodes))
    return RPLGPU_ERR_INVALID_ARG;
  if (n > h->max_n) return RPLGPU_ERR_CAPACITY;
  std::memset(meta, 0, sizeof(*meta));
  *msg_len = 0;
  if (n == 0) return RPLGPU_OK;  // :561-563
  rplgpu_laserscan_layout_t L;
  if (int32_t rc = rplgpu_msg_laserscan_layout(std::strlen(frame_id), (uint32_t)n, &L)) return rc;
  if (L.total_len > cap) {
    h->err = "message buffer smaller than the worst case (count == n)";
    return RPLGPU_ERR_CAPACITY;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  if (unsigned char *d_msg = h->zero_copy ? pinned_device_view(h, msg, cap) : nullptr) {
    // The message buffer is device-addressable (rplgpu_host_alloc): the kernels read the staged
    // nodes and WRITE THE SERIALISED MESSAGE IN PLACE — prefix, scalars, both arrays — over
    // PCIe: two launches, one synchronisation, no DMA, no host pass over the arrays.
    rplmsg::Prefix P;
    if (int32_t rc = make_prefix(h, frame_id, false, p, &P)) return rc;
    const ScanStage st = stage_scan(h, nodes, n);
    // per-scan inputs / outputs of the message kernel travel in the staging tail:
    // [count][status] after the nodes (stage_scan), then stamp (8 B), duration (8 B), msg_len, status
    unsigned char *tail_h = h->h_pin + n * 8 + 16, *tail_d = h->d_pin + n * 8 + 16;
    std::memcpy(tail_h, &stamp, 8);
    std::memcpy(tail_h + 8, &scan_duration, 8);
    const uint32_t zeros[2] = {0u, 0u};
    std::memcpy(tail_h + 16, zeros, 8);
    float *d_r = reinterpret_cast<float *>(h->d_out);  // the arrays themselves stay in HBM
    float *d_i = d_r + n;
    uint32_t *d_count = reinterpret_cast<uint32_t *>(st.d_out);  // host-visible
    if (p->scan_processing) {
      // Mode A on the validated fast path: ONE kernel bins the scan and writes the message
      // around and into its arrays (the arrays never exist outside the message)
      if (int32_t vrc = ensure_idx_checked(h)) return vrc;
      if (use_fast_idx(h) && use_fast_d4000(h) && (reinterpret_cast<uintptr_t>(d_msg) & 3u) == 0u) {
        rpl::LsMsgOut mo;
        mo.P = P;
        mo.msg = reinterpret_cast<uint32_t *>(d_msg);
        mo.msg_len = reinterpret_cast<uint32_t *>(tail_d + 16);
        mo.sec = stamp.sec;
        mo.nanosec = stamp.nanosec;
        mo.scan_duration = scan_duration;
        RPL_HIP(h, rpl::launch_laserscan_a(h->stream, st.d_nodes, (uint32_t)n, st.d_n, 1, to_kparams(*p),
                                           tables_of(h), h->d_inc, h->d_rinc, true, d_r, d_i, d_count,
                                           (uint32_t)n, &mo));
        if (int32_t wrc = wait_scan(h)) return wrc;
        uint32_t count, len;
        std::memcpy(&count, st.h_out, 4);
        std::memcpy(&len, tail_h + 16, 4);
        rplgpu_fill_meta(p, count, scan_duration, meta);
        *msg_len = count ? len : 0;
        return RPLGPU_OK;
      }
    }
    if (int32_t lrc = run_laserscan(h, st.d_nodes, (uint32_t)n, st.d_n, 1, *p, d_r, d_i, d_count, (uint32_t)n))
      return lrc;
    const uint32_t stride = (uint32_t)std::min<size_t>(cap, 0xFFFFFFFCu) & ~3u;
    RPL_HIP(h, rpl::launch_msg_laserscan(h->stream, d_r, d_i, (uint32_t)n, d_count, 1,
                                         p->scan_processing != 0,
                                         reinterpret_cast<const rplgpu_stamp_t *>(tail_d),
                                         reinterpret_cast<const double *>(tail_d + 8), P, d_msg, stride,
                                         reinterpret_cast<uint32_t *>(tail_d + 16),
                                         reinterpret_cast<uint32_t *>(tail_d + 20)));
    if (int32_t wrc = wait_scan(h)) return wrc;
    uint32_t count, len;
    std::memcpy(&count, st.h_out, 4);
    std::memcpy(&len, tail_h + 16, 4);
    rplgpu_fill_meta(p, count, scan_duration, meta);
    *msg_len = count ? len : 0;
    return RPLGPU_OK;
  }
  uint32_t *h_small = reinterpret_cast<uint32_t *>(stage_out(h));  // pinned scratch word
  const uint32_t *d_n;
  if (int32_t rc = upload_scan(h, nodes, n, &d_n)) return rc;
  float *d_r = reinterpret_cast<float *>(h->d_out);
  float *d_i = d_r + n;
  uint32_t *d_count = reinterpret_cast<uint32_t *>(d_i + n);
  if (int32_t lrc = run_laserscan(h, h->d_nodes, (uint32_t)n, d_n, 1, *p, d_r, d_i, d_count))
    return lrc;
  RPL_HIP(h, hipMemcpyAsync(h_small, d_count, 4, hipMemcpyDeviceToHost, h->stream));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  const uint32_t count = h_small[0];
  rplgpu_fill_meta(p, count, scan_duration, meta);
  if (count == 0) return RPLGPU_OK;  // :611-613: nothing is published
  if (int32_t rc = rplgpu_msg_laserscan_header(frame_id, stamp, meta, msg, cap, &L)) return rc;
  // the two arrays go by DMA to their final place inside the serialised message
  RPL_HIP(h, hipMemcpyAsync(msg + L.ranges_off, d_r, (size_t)count * 4, hipMemcpyDeviceToHost,
                            h->stream));
  RPL_HIP(h, hipMemcpyAsync(msg + L.intensities_off, d_i, (size_t)count * 4,
                            hipMemcpyDeviceToHost, h->stream));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  *msg_len = L.total_len;
  return RPLGPU_OK;
}

int32_t rplgpu_scan_to_cloud_msg(rplgpu_handle_t h, const rplgpu_node_t *nodes, size_t n,
                                 const rplgpu_params_t *p, const char *frame_id,
                                 rplgpu_stamp_t stamp, uint8_t *msg, size_t cap, size_t *msg_len,
                                 uint32_t *n_points, uint32_t *status) {
  if (!h || !p || !frame_id || !msg || !msg_len || !n_points || (n && !nodes))
    return RPLGPU_ERR_INVALID_ARG;
  if (n > h->max_n) return RPLGPU_ERR_CAPACITY;
  *n_points = 0;
  *msg_len = 0;
  if (status) *status = 0;
  rplgpu_cloud_layout_t L;
  if (int32_t rc = rplgpu_msg_cloud_layout(std::strlen(frame_id), (uint32_t)n, &L)) return rc;
  if (L.total_len > cap) {
    h->err = "message buffer smaller than the worst case (n points)";
    return RPLGPU_ERR_CAPACITY;
  }
  // The cloud itself comes through rplgpu_scan_to_cloud (zero-copy staging, completion flag): it
  // lands at its final offset inside the message — the data offset does not depend on the number
  // of points — and the CDR framing around it is written once that number is known.
  uint32_t np = 0, st = 0;
  int32_t crc = RPLGPU_OK;
  if (n) {
    crc = rplgpu_scan_to_cloud(h, nodes, n, p, reinterpret_cast<float *>(msg + L.data_off), &np, &st);
    if (crc != RPLGPU_OK && crc != RPLGPU_ERR_SCAN_OVERFLOW) return crc;
  }
  if (int32_t rc = rplgpu_msg_cloud_header(frame_id, stamp, np, msg, cap, &L)) return rc;
  *n_points = np;
  *msg_len = L.total_len;
  if (status) *status = st;
  return crc;
}

static int32_t make_prefix(rplgpu_handle_t h, const char *frame_id, bool cloud,
                           const rplgpu_params_t *p, rplmsg::Prefix *P) {
  const size_t fl = std::strlen(frame_id);
  if (fl > rplmsg::kMaxFrameId) {
    h->err = "frame_id longer than 255 bytes";
    return RPLGPU_ERR_INVALID_ARG;
  }
  std::memset(P, 0, sizeof(*P));
  rplmsg::Writer w(reinterpret_cast<uint8_t *>(P->words), sizeof(P->words));
  P->stamp_off = 4;
  if (cloud) {
    rplgpu_cloud_layout_t L;
    rplmsg::write_cloud(w, frame_id, fl, rplgpu_stamp_t{0, 0}, 0, &L);
    P->len = L.data_off;
    P->a_off = L.width_off;
    P->b_off = L.row_step_off;
    P->c_off = L.data_len_off;
  } else {
    rplgpu_scan_meta_t m;
    rplgpu_fill_meta(p, 1, 0.0, &m);  // angle_min/max, range_min/max: the per-publisher constants
    m.count = 0;
    rplgpu_laserscan_layout_t L;
    rplmsg::write_laserscan(w, frame_id, fl, rplgpu_stamp_t{0, 0}, m, &L);
    P->len = L.ranges_off;
    P->a_off = L.scalars_off;
    P->b_off = L.ranges_len_off;
  }
  if (P->len > sizeof(P->words) || (P->len & 3u)) {
    h->err = "message prefix does not fit the device template";
    return RPLGPU_ERR_INVALID_ARG;
  }
  return RPLGPU_OK;
}

int32_t rplgpu_laserscan_msgs_dev(rplgpu_handle_t h, const float *d_ranges,
                                  const float *d_intensities, uint32_t n_stride,
                                  const uint32_t *d_beam_count, uint32_t B,
                                  const rplgpu_params_t *p, const char *frame_id,
                                  const rplgpu_stamp_t *d_stamps, const double *d_scan_duration,
                                  uint8_t *d_msgs, uint32_t msg_stride, uint32_t *d_msg_len,
                                  uint32_t *d_status) {
  if (!h || !p || !frame_id) return RPLGPU_ERR_INVALID_ARG;
  if (B == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_beam_count || !d_stamps || !d_scan_duration || !d_msgs ||
      !d_msg_len || n_stride == 0 || (msg_stride & 3u))
    return RPLGPU_ERR_INVALID_ARG;
  rplmsg::Prefix P;
  if (int32_t rc = make_prefix(h, frame_id, false, p, &P)) return rc;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_msg_laserscan(h->stream, d_ranges, d_intensities, n_stride, d_beam_count,
                                       B, p->scan_processing != 0, d_stamps, d_scan_duration, P,
                                       d_msgs, msg_stride, d_msg_len, d_status));
  return RPLGPU_OK;
}

int32_t rplgpu_cloud_msgs_dev(rplgpu_handle_t h, const float *d_xyzi, uint32_t out_stride,
                              const uint64_t *d_scan_start, const uint32_t *d_n_points,
                              uint32_t B, const char *frame_id, const rplgpu_stamp_t *d_stamps,
                              uint8_t *d_msgs, uint32_t msg_stride, uint32_t *d_msg_len,
                              uint32_t *d_status) {
  if (!h || !frame_id) return RPLGPU_ERR_INVALID_ARG;
  if (B == 0) return RPLGPU_OK;
  if (!d_xyzi || !d_n_points || !d_stamps || !d_msgs || !d_msg_len || (msg_stride & 3u) ||
      (!d_scan_start && out_stride == 0))
    return RPLGPU_ERR_INVALID_ARG;
  rplmsg::Prefix P;
  if (int32_t rc = make_prefix(h, frame_id, true, nullptr, &P)) return rc;
  RPL_HIP(h, hipSetDevice(h->device));
  // a scan never yields more points than it has samples
  const uint32_t max_points = d_scan_start ? h->max_n : std::min(out_stride, h->max_n);
  RPL_HIP(h, rpl::launch_msg_cloud(h->stream, d_xyzi, out_stride, max_points,
                                   reinterpret_cast<const unsigned long long *>(d_scan_start),
                                   d_n_points, B, d_stamps, P, d_msgs, msg_stride, d_msg_len,
                                   d_status));
  return RPLGPU_OK;
}

int32_t rplgpu_transform_clouds_dev(rplgpu_handle_t h, float *d_xyzi, uint32_t out_stride,
                                    const uint64_t *d_scan_start, const uint32_t *d_n_points,
                                    uint32_t B, const float *d_pose) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (B == 0) return RPLGPU_OK;
  if (!d_xyzi || !d_n_points || !d_pose || (!d_scan_start && out_stride == 0))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  const uint32_t max_points = d_scan_start ? h->max_n : std::min(out_stride, h->max_n);
  RPL_HIP(h, rpl::launch_transform_clouds(
                 h->stream, d_xyzi, out_stride, max_points,
                 reinterpret_cast<const unsigned long long *>(d_scan_start), d_n_points, B, d_pose));
  return RPLGPU_OK;
}

int32_t rplgpu_fused_cloud_msg_dev(rplgpu_handle_t h, const float *d_arena,
                                   const uint64_t *d_total_points, uint64_t arena_capacity,
                                   const char *frame_id, rplgpu_stamp_t stamp, uint8_t *d_msg,
                                   uint64_t msg_capacity, uint64_t *d_msg_len, uint32_t *d_status) {
  if (!h || !frame_id || !d_arena || !d_total_points || !d_msg || !d_msg_len)
    return RPLGPU_ERR_INVALID_ARG;
  rplmsg::Prefix P;
  if (int32_t rc = make_prefix(h, frame_id, true, nullptr, &P)) return rc;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_msg_fused(h->stream, d_arena,
                                   reinterpret_cast<const unsigned long long *>(d_total_points),
                                   arena_capacity, stamp, P, d_msg, msg_capacity,
                                   reinterpret_cast<unsigned long long *>(d_msg_len), d_status));
  return RPLGPU_OK;
}

int32_t rplgpu_laserscan_to_cloud_batch_dev(rplgpu_handle_t h, const float *d_ranges,
                                            const float *d_intensities, uint32_t n_stride,
                                            const uint32_t *d_beam_count, uint32_t B,
                                            const rplgpu_params_t *p, float *d_xyzi,
                                            uint32_t out_stride, uint32_t *d_n_points,
                                            uint32_t *d_status) {
  if (!h || !p) return RPLGPU_ERR_INVALID_ARG;
  if (B == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_beam_count || !d_xyzi || !d_n_points || n_stride == 0 ||
      out_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (B > h->max_b) return RPLGPU_ERR_CAPACITY;
  if (!device_readable(h, d_ranges, "d_ranges") || !device_readable(h, d_intensities, "d_intensities") ||
      !device_readable(h, d_beam_count, "d_beam_count") || !device_readable(h, d_xyzi, "d_xyzi"))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_laserscan_to_cloud(h->stream, d_ranges, d_intensities, n_stride,
                                            d_beam_count, B, to_kparams(*p), d_xyzi, out_stride,
                                            d_n_points, d_status));
  return RPLGPU_OK;
}

int32_t rplgpu_laserscan_to_cloud(rplgpu_handle_t h, const float *ranges,
                                  const float *intensities, uint32_t count,
                                  const rplgpu_params_t *p, float *xyzi, uint32_t *n_points) {
  if (!h || !p || !n_points || (count && (!ranges || !intensities || !xyzi)))
    return RPLGPU_ERR_INVALID_ARG;
  if (count > h->max_n) return RPLGPU_ERR_CAPACITY;
  *n_points = 0;
  if (count == 0) return RPLGPU_OK;
  RPL_HIP(h, hipSetDevice(h->device));
  // staging: ranges | intensities | count word go in with one copy (d_nodes holds 8 B per sample)
  const size_t n = count;
  std::memcpy(h->h_pin, ranges, n * 4);
  std::memcpy(h->h_pin + n * 4, intensities, n * 4);
  const uint32_t words[2] = {count, 0u};
  std::memcpy(h->h_pin + n * 8, words, 8);
  RPL_HIP(h, hipMemcpyAsync(h->d_nodes, h->h_pin, n * 8 + 8, hipMemcpyHostToDevice, h->stream));
  const float *d_r = reinterpret_cast<const float *>(h->d_nodes);
  const uint32_t *d_cnt = reinterpret_cast<const uint32_t *>(h->d_nodes + n * 8);
  uint32_t *d_np = reinterpret_cast<uint32_t *>(h->d_out + n * 16);  // travels back with the points
  RPL_HIP(h, rpl::launch_laserscan_to_cloud(h->stream, d_r, d_r + n, count, d_cnt, 1,
                                            to_kparams(*p), reinterpret_cast<float *>(h->d_out),
                                            count, d_np, nullptr));
  unsigned char *h_out = stage_out(h);
  RPL_HIP(h, hipMemcpyAsync(h_out, h->d_out, n * 16 + 4, hipMemcpyDeviceToHost, h->stream));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  uint32_t np;
  std::memcpy(&np, h_out + n * 16, 4);
  *n_points = np;
  std::memcpy(xyzi, h_out, (size_t)np * 16);
  return RPLGPU_OK;
}

int32_t rplgpu_cloud_deskew_batch_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                      uint32_t n_stride, const uint32_t *d_n_per_scan, uint32_t B,
                                      const rplgpu_params_t *p, const float *d_motion,
                                      float *d_xyzi, uint32_t out_stride, uint32_t *d_n_points,
                                      uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !d_motion || !d_xyzi || !d_n_points || out_stride == 0) return RPLGPU_ERR_INVALID_ARG;
  if (p->voxel_enable) {
    h->err = "de-skew works on the plain cloud (voxel_enable = 0)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  CloudPlan plan;
  if ((rc = prepare_cloud(h, d_nodes, n_stride, d_n_per_scan, B, p, CloudRequest{}, &plan))) return rc;
  RPL_HIP(h, rpl::launch_cloud(h->stream, d_nodes, n_stride, d_n_per_scan, B, plan.kp, plan.T, plan.mask,
                               kMaskStride, d_xyzi, out_stride, d_n_points, d_status, d_motion));
  return RPLGPU_OK;
}

}  // extern "C"

// ---- multi-GPU exchange (include/rplgpu_comm.h) ------------------------------------------
// RCCL is loaded at run time: a node that never exchanges clouds does not need it, and a host
// process that already has an RCCL mapped (PyTorch ships its own) keeps exactly that one.
namespace {

struct RcclApi {
  void *lib = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, rplgpu_nccl_id_t, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*CommCount)(void *, int *) = nullptr;
  int (*CommUserRank)(void *, int *) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  bool ok = false;
};

RcclApi &rccl() {
  static RcclApi api = [] {
    RcclApi a;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char *n : names) {
      a.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (a.lib) break;
    }
    if (!a.lib) return a;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(a.lib, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(a.lib, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(a.lib, "ncclCommCount"));
    a.CommUserRank = reinterpret_cast<decltype(a.CommUserRank)>(dlsym(a.lib, "ncclCommUserRank"));
    a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(a.lib, "ncclAllGather"));
    a.Send = reinterpret_cast<decltype(a.Send)>(dlsym(a.lib, "ncclSend"));
    a.Recv = reinterpret_cast<decltype(a.Recv)>(dlsym(a.lib, "ncclRecv"));
    a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(dlsym(a.lib, "ncclGroupStart"));
    a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(dlsym(a.lib, "ncclGroupEnd"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllGather && a.GroupStart &&
           a.GroupEnd;
    return a;
  }();
  return api;
}

constexpr int kNcclUint32 = 3, kNcclFloat32 = 7;  // ncclDataType_t (rccl.h)

#define RPL_NCCL(ctx, call)                                                                     \
  do {                                                                                          \
    int r_ = (call);                                                                            \
    if (r_ != 0) {                                                                              \
      (ctx)->err = std::string(#call) + ": " +                                                 \
                   (rccl().GetErrorString ? rccl().GetErrorString(r_) : "RCCL error");          \
      return RPLGPU_ERR_HIP;                                                                    \
    }                                                                                           \
  } while (0)

void comm_teardown(rplgpu_ctx *c) {
  if (c->comm && rccl().ok) {
    if (c->xstream) (void)hipStreamSynchronize(c->xstream);
    (void)rccl().CommDestroy(c->comm);
  }
  c->comm = nullptr;
  c->comm_world = 0;
  if (c->ev_main) (void)hipEventDestroy(c->ev_main);
  for (auto &e : c->ev_x) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  if (c->xstream) (void)hipStreamDestroy(c->xstream);
  c->ev_main = nullptr;
  c->xstream = nullptr;
  c->n_exchanges = 0;
}

}  // namespace

extern "C" {

int32_t rplgpu_comm_unique_id(uint8_t id[RPLGPU_COMM_ID_BYTES]) {
  if (!id) return RPLGPU_ERR_INVALID_ARG;
  if (!rccl().ok) return RPLGPU_ERR_NO_DEVICE;
  static_assert(sizeof(rplgpu_nccl_id_t) == RPLGPU_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  return rccl().GetUniqueId(id) == 0 ? RPLGPU_OK : RPLGPU_ERR_HIP;
}

int32_t rplgpu_comm_size(rplgpu_handle_t h, int32_t *world, int32_t *rank) {
  if (!h || !world) return RPLGPU_ERR_INVALID_ARG;
  *world = 0;
  if (rank) *rank = -1;
  if (!h->comm) return RPLGPU_OK;  // no communicator: 0 ranks
  if (!rccl().ok || !rccl().CommCount) return RPLGPU_ERR_NO_DEVICE;
  int n = 0, r = -1;
  RPL_NCCL(h, rccl().CommCount(h->comm, &n));  // what RCCL itself says, not what was asked for
  if (rank && rccl().CommUserRank) RPL_NCCL(h, rccl().CommUserRank(h->comm, &r));
  *world = n;
  if (rank) *rank = r;
  return RPLGPU_OK;
}

int32_t rplgpu_comm_init(rplgpu_handle_t h, int32_t rank, int32_t world,
                         const uint8_t id[RPLGPU_COMM_ID_BYTES]) {
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return RPLGPU_ERR_INVALID_ARG;
  if (!rccl().ok) {
    h->err = "RCCL (librccl.so) could not be loaded";
    return RPLGPU_ERR_NO_DEVICE;
  }
  if (h->comm) {
    h->err = "communicator already initialised (rplgpu_comm_destroy first)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // (every failure below releases what was created so far: a retry starts from nothing)
  auto init = [&]() -> int32_t {
    RPL_HIP(h, hipStreamCreateWithFlags(&h->xstream, hipStreamNonBlocking));
    RPL_HIP(h, hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    for (auto &e : h->ev_x) RPL_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    rplgpu_nccl_id_t uid;
    std::memcpy(&uid, id, sizeof(uid));
    RPL_NCCL(h, rccl().CommInitRank(&h->comm, world, uid, rank));
    return RPLGPU_OK;
  };
  const int32_t rc = init();
  if (rc != RPLGPU_OK) {
    h->comm = nullptr;  // (not a communicator teardown can destroy)
    comm_teardown(h);
    return rc;
  }
  h->comm_rank = rank;
  h->comm_world = world;
  return RPLGPU_OK;
}

int32_t rplgpu_comm_destroy(rplgpu_handle_t h) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  (void)hipSetDevice(h->device);
  comm_teardown(h);
  return RPLGPU_OK;
}

uint32_t rplgpu_cloud_meta_words(uint32_t max_scans) { return 4u + 3u * max_scans; }

int32_t rplgpu_pack_cloud_meta_dev(rplgpu_handle_t h, const uint64_t *d_cursor,
                                   const uint64_t *d_scan_start, const uint32_t *d_n_points,
                                   uint32_t B, uint64_t slot_points, uint32_t max_scans,
                                   uint32_t *d_meta) {
  if (!h || !d_cursor || !d_meta || (B && (!d_scan_start || !d_n_points)) || B > max_scans)
    return RPLGPU_ERR_INVALID_ARG;
  if (!device_readable(h, d_cursor, "d_cursor") || !device_readable(h, d_meta, "d_meta"))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_pack_meta(h->stream, reinterpret_cast<const unsigned long long *>(d_cursor),
                                   reinterpret_cast<const unsigned long long *>(d_scan_start),
                                   d_n_points, B, slot_points, max_scans, d_meta));
  return RPLGPU_OK;
}

namespace {
int32_t allgather_slots(rplgpu_handle_t h, const float *d_points_local, uint64_t slot_points,
                        uint32_t point_floats, const uint32_t *d_meta_local, uint32_t meta_words,
                        float *d_points_all, uint32_t *d_meta_all);
}
int32_t rplgpu_allgather_clouds_dev(rplgpu_handle_t h, const float *d_points_local,
                                    uint64_t slot_points, const uint32_t *d_meta_local,
                                    uint32_t meta_words, float *d_points_all,
                                    uint32_t *d_meta_all) {
  return allgather_slots(h, d_points_local, slot_points, 4u, d_meta_local, meta_words, d_points_all,
                         d_meta_all);
}
int32_t rplgpu_allgather_clouds_xyi_dev(rplgpu_handle_t h, const float *d_slot_local,
                                        uint64_t slot_points, const uint32_t *d_meta_local,
                                        uint32_t meta_words, float *d_slots_all,
                                        uint32_t *d_meta_all) {
  return allgather_slots(h, d_slot_local, slot_points, 3u, d_meta_local, meta_words, d_slots_all,
                         d_meta_all);
}
namespace {
int32_t allgather_slots(rplgpu_handle_t h, const float *d_points_local, uint64_t slot_points,
                        uint32_t point_floats, const uint32_t *d_meta_local, uint32_t meta_words,
                        float *d_points_all, uint32_t *d_meta_all) {
  if (!h || !d_points_local || !d_meta_local || !d_points_all || !d_meta_all || meta_words == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (!h->comm) {
    h->err = "rplgpu_comm_init has not been called";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, d_points_local, "d_points_local") ||
      !device_readable(h, d_points_all, "d_points_all") ||
      !device_readable(h, d_meta_local, "d_meta_local") ||
      !device_readable(h, d_meta_all, "d_meta_all"))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  // the exchange stream picks up after everything queued on the main stream so far
  RPL_HIP(h, hipEventRecord(h->ev_main, h->stream));
  RPL_HIP(h, hipStreamWaitEvent(h->xstream, h->ev_main, 0));
  RPL_NCCL(h, rccl().GroupStart());
  int r1 = rccl().AllGather(d_meta_local, d_meta_all, meta_words, kNcclUint32, h->comm, h->xstream);
  int r2 = slot_points ? rccl().AllGather(d_points_local, d_points_all,
                                          (size_t)slot_points * point_floats, kNcclFloat32, h->comm,
                                          h->xstream)
                       : 0;
  const int r3 = rccl().GroupEnd();
  // the ring event is recorded whatever RCCL said, so that a later fence waits for what was
  // really queued on the exchange stream and never for an event of an older exchange
  RPL_HIP(h, hipEventRecord(h->ev_x[h->n_exchanges & 3u], h->xstream));
  ++h->n_exchanges;
  RPL_NCCL(h, r1);
  RPL_NCCL(h, r2);
  RPL_NCCL(h, r3);
  return RPLGPU_OK;
}
}  // namespace

namespace {
// grouped ncclSend / ncclRecv of slots of `slot_floats` 32-bit words (points or cell records) and META
// blocks to `root` (rplgpu_gather_clouds_dev, rplgpu_gather_cells_dev)
int32_t gather_slots(rplgpu_handle_t h, int32_t root, const float *d_points_local, size_t slot_floats,
                     const uint32_t *d_meta_local, uint32_t meta_words, float *d_points_all,
                     uint32_t *d_meta_all);
}  // namespace

int32_t rplgpu_gather_clouds_dev(rplgpu_handle_t h, int32_t root, const float *d_points_local,
                                 uint64_t slot_points, uint32_t point_floats,
                                 const uint32_t *d_meta_local, uint32_t meta_words,
                                 float *d_points_all, uint32_t *d_meta_all) {
  if (!h || !d_points_local || !d_meta_local || meta_words == 0 || (point_floats != 3u && point_floats != 4u))
    return RPLGPU_ERR_INVALID_ARG;
  return gather_slots(h, root, d_points_local, (size_t)slot_points * point_floats, d_meta_local,
                      meta_words, d_points_all, d_meta_all);
}

int32_t rplgpu_gather_cells_dev(rplgpu_handle_t h, int32_t root, const rplgpu_cell_t *d_cells_local,
                                uint64_t slot_cells, const uint32_t *d_meta_local,
                                uint32_t meta_words, rplgpu_cell_t *d_cells_all,
                                uint32_t *d_meta_all) {
  if (!h || !d_cells_local || !d_meta_local || meta_words == 0) return RPLGPU_ERR_INVALID_ARG;
  constexpr size_t kWords = sizeof(rplgpu_cell_t) / 4u;
  return gather_slots(h, root, reinterpret_cast<const float *>(d_cells_local), (size_t)slot_cells * kWords,
                      d_meta_local, meta_words, reinterpret_cast<float *>(d_cells_all), d_meta_all);
}

namespace {
int32_t gather_slots(rplgpu_handle_t h, int32_t root, const float *d_points_local, size_t slot_floats,
                     const uint32_t *d_meta_local, uint32_t meta_words, float *d_points_all,
                     uint32_t *d_meta_all) {
  if (!h->comm) {
    h->err = "rplgpu_comm_init has not been called";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (root < 0 || root >= h->comm_world) return RPLGPU_ERR_INVALID_ARG;
  if (!rccl().Send || !rccl().Recv) {
    h->err = "this RCCL has no ncclSend / ncclRecv";
    return RPLGPU_ERR_NO_DEVICE;
  }
  const bool is_root = h->comm_rank == root;
  if (is_root && (!d_points_all || !d_meta_all)) return RPLGPU_ERR_INVALID_ARG;
  if (!device_readable(h, d_points_local, "d_points_local") ||
      !device_readable(h, d_meta_local, "d_meta_local") ||
      (is_root && (!device_readable(h, d_points_all, "d_points_all") ||
                   !device_readable(h, d_meta_all, "d_meta_all"))))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, hipEventRecord(h->ev_main, h->stream));
  RPL_HIP(h, hipStreamWaitEvent(h->xstream, h->ev_main, 0));
  int rs = 0;
  hipError_t hs = hipSuccess;
  const int g0 = rccl().GroupStart();
  if (is_root) {
    for (int r = 0; r < h->comm_world && rs == 0; ++r) {
      if (r == root) continue;
      rs = rccl().Recv(d_meta_all + (size_t)r * meta_words, meta_words, kNcclUint32, r, h->comm, h->xstream);
      if (rs == 0 && slot_floats)
        rs = rccl().Recv(d_points_all + (size_t)r * slot_floats, slot_floats, kNcclFloat32, r, h->comm,
                         h->xstream);
    }
  } else {
    rs = rccl().Send(d_meta_local, meta_words, kNcclUint32, root, h->comm, h->xstream);
    if (rs == 0 && slot_floats)
      rs = rccl().Send(d_points_local, slot_floats, kNcclFloat32, root, h->comm, h->xstream);
  }
  const int g1 = rccl().GroupEnd();
  if (is_root) {  // the root's own slot and META block (in place: nothing to move)
    float *own = d_points_all + (size_t)root * slot_floats;
    uint32_t *own_meta = d_meta_all + (size_t)root * meta_words;
    if (own != d_points_local && slot_floats)
      hs = hipMemcpyAsync(own, d_points_local, slot_floats * 4u, hipMemcpyDeviceToDevice, h->xstream);
    if (hs == hipSuccess && own_meta != d_meta_local)
      hs = hipMemcpyAsync(own_meta, d_meta_local, (size_t)meta_words * 4u, hipMemcpyDeviceToDevice,
                          h->xstream);
  }
  // (as in the all-gather: the ring event is recorded whatever happened above)
  RPL_HIP(h, hipEventRecord(h->ev_x[h->n_exchanges & 3u], h->xstream));
  ++h->n_exchanges;
  RPL_NCCL(h, g0);
  RPL_NCCL(h, rs);
  RPL_NCCL(h, g1);
  RPL_HIP(h, hs);
  return RPLGPU_OK;
}
}  // namespace

int32_t rplgpu_comm_fence_lag(rplgpu_handle_t h, uint32_t lag) {
  if (!h || lag > 3u) return RPLGPU_ERR_INVALID_ARG;
  if (!h->comm || h->n_exchanges <= lag) return RPLGPU_OK;  // no such exchange: nothing to wait for
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, hipStreamWaitEvent(h->stream, h->ev_x[(h->n_exchanges - 1u - lag) & 3u], 0));
  return RPLGPU_OK;
}

int32_t rplgpu_comm_fence(rplgpu_handle_t h) { return rplgpu_comm_fence_lag(h, 0u); }

int32_t rplgpu_unpack_gathered_dev(rplgpu_handle_t h, const float *d_points_all,
                                   uint64_t slot_points, const uint32_t *d_meta_all,
                                   uint32_t meta_words, uint32_t world, uint32_t max_scans,
                                   float *d_packed, uint64_t *d_total,
                                   uint64_t *d_scan_start_all, uint32_t *d_n_points_all,
                                   uint32_t *d_status) {
  if (!h || !d_points_all || !d_meta_all || !d_packed || !d_total || !d_scan_start_all ||
      !d_n_points_all || world == 0 || world > 4096 || meta_words < rplgpu_cloud_meta_words(max_scans))
    return RPLGPU_ERR_INVALID_ARG;
  if (!device_readable(h, d_points_all, "d_points_all") || !device_readable(h, d_meta_all, "d_meta_all") ||
      !device_readable(h, d_packed, "d_packed"))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_unpack_gathered(
                 h->stream, d_points_all, slot_points, d_meta_all, meta_words, world, max_scans, d_packed,
                 reinterpret_cast<unsigned long long *>(d_total),
                 reinterpret_cast<unsigned long long *>(d_scan_start_all), d_n_points_all, d_status,
                 h->n_cu, false));
  return RPLGPU_OK;
}

int32_t rplgpu_unpack_gathered_xyi_dev(rplgpu_handle_t h, const float *d_slots_all,
                                       uint64_t slot_points, const uint32_t *d_meta_all,
                                       uint32_t meta_words, uint32_t world, uint32_t max_scans,
                                       float *d_packed, uint64_t *d_total,
                                       uint64_t *d_scan_start_all, uint32_t *d_n_points_all,
                                       uint32_t *d_status) {
  if (!h || !d_slots_all || !d_meta_all || !d_packed || !d_total || !d_scan_start_all ||
      !d_n_points_all || world == 0 || world > 4096 || meta_words < rplgpu_cloud_meta_words(max_scans))
    return RPLGPU_ERR_INVALID_ARG;
  if (!device_readable(h, d_slots_all, "d_slots_all") || !device_readable(h, d_meta_all, "d_meta_all") ||
      !device_readable(h, d_packed, "d_packed"))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_unpack_gathered(
                 h->stream, d_slots_all, slot_points, d_meta_all, meta_words, world, max_scans, d_packed,
                 reinterpret_cast<unsigned long long *>(d_total),
                 reinterpret_cast<unsigned long long *>(d_scan_start_all), d_n_points_all, d_status,
                 h->n_cu, true));
  return RPLGPU_OK;
}

int32_t rplgpu_pack_cloud_xyi_dev(rplgpu_handle_t h, const float *d_arena, const uint64_t *d_cursor,
                                  uint64_t slot_points, float *d_slot) {
  if (!h || !d_arena || !d_cursor || !d_slot) return RPLGPU_ERR_INVALID_ARG;
  if (!device_readable(h, d_arena, "d_arena") || !device_readable(h, d_cursor, "d_cursor") ||
      !device_readable(h, d_slot, "d_slot"))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_pack_xyi(h->stream, d_arena,
                                  reinterpret_cast<const unsigned long long *>(d_cursor), slot_points,
                                  d_slot, h->n_cu));
  return RPLGPU_OK;
}

// argument checks shared by rplgpu_merge_cells_dev and its host twin
static bool merge_args_ok(const void *cells_all, const uint32_t *meta_all, uint32_t meta_words,
                          uint32_t world, uint32_t n_groups, const rplgpu_params_t *p, const float *arena,
                          const uint64_t *cursor, const uint64_t *group_start, const uint32_t *n_points) {
  return cells_all && meta_all && p && arena && cursor && group_start && n_points && world >= 1u &&
         world <= rpl::cells::kMaxWorld && n_groups <= (1u << 24) &&
         meta_words >= rplgpu_cloud_meta_words(n_groups) && p->voxel_leaf >= 1e-6f &&
         p->voxel_leaf <= 1024.0f;
}

int32_t rplgpu_merge_cells_dev(rplgpu_handle_t h, const rplgpu_cell_t *d_cells_all,
                               uint64_t slot_cells, const uint32_t *d_meta_all, uint32_t meta_words,
                               uint32_t world, uint32_t n_groups, const rplgpu_params_t *p,
                               float *d_arena, uint64_t arena_capacity, uint64_t *d_cursor,
                               uint64_t *d_group_start, uint32_t *d_n_points, uint32_t *d_status) {
  if (!h || !merge_args_ok(d_cells_all, d_meta_all, meta_words, world, n_groups, p, d_arena, d_cursor,
                           d_group_start, d_n_points))
    return RPLGPU_ERR_INVALID_ARG;
  if (!device_readable(h, d_cells_all, "d_cells_all") || !device_readable(h, d_meta_all, "d_meta_all") ||
      !device_readable(h, d_arena, "d_arena") || !device_readable(h, d_cursor, "d_cursor"))
    return RPLGPU_ERR_INVALID_ARG;
  // a group's records of all ranks are indexed by 31 bits (the leader prefixes), and the scratch
  // holds one word per record of the gathered buffer
  if (slot_cells > (0x7FFFFFFFull / world)) {
    h->err = "rplgpu_merge_cells_dev: world x slot_cells above 2^31 records";
    return RPLGPU_ERR_CAPACITY;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t need = (size_t)world * slot_cells;
  if (need > h->merge_cap) {  // grows (only ever grows) on the first call with larger slots
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    void *bigger = nullptr;
    if (hipMalloc(&bigger, need * 4u) != hipSuccess) {
      h->err = "merge scratch allocation failed";
      (void)hipGetLastError();
      return RPLGPU_ERR_HIP;
    }
    if (h->d_merge) (void)hipFree(h->d_merge);
    h->d_merge = static_cast<uint32_t *>(bigger);
    h->merge_cap = need;
  }
  const double unit = 1.0 / to_kparams(*p).vox_scale;
  RPL_HIP(h, hipMemsetAsync(d_cursor, 0, 8, h->stream));
  RPL_HIP(h, rpl::launch_merge_cells(h->stream, d_cells_all, slot_cells, d_meta_all, meta_words, world,
                                     n_groups, unit, d_arena, arena_capacity,
                                     reinterpret_cast<unsigned long long *>(d_cursor),
                                     reinterpret_cast<unsigned long long *>(d_group_start), d_n_points,
                                     d_status, h->d_merge, h->n_cu));
  return RPLGPU_OK;
}

/* Host twins of the layout kernels: the same rules (rpl_comm_layout.hpp), plain loops, no device —
 * what a world-size-2 test over a CPU transport (gloo) drives. */
int32_t rplgpu_pack_cloud_meta_host(uint64_t cursor, const uint64_t *scan_start,
                                    const uint32_t *n_points, uint32_t B, uint64_t slot_points,
                                    uint32_t max_scans, uint32_t *meta) {
  if (!meta || (B && (!scan_start || !n_points)) || B > max_scans) return RPLGPU_ERR_INVALID_ARG;
  rpl::layout::meta_head(cursor, B, slot_points, meta);
  for (uint32_t t = 0; t < max_scans; ++t)
    rpl::layout::meta_scan(t, B, reinterpret_cast<const unsigned long long *>(scan_start), n_points,
                           slot_points, meta);
  return RPLGPU_OK;
}

int32_t rplgpu_pack_cloud_xyi_host(const float *arena, uint64_t cursor, uint64_t slot_points,
                                   float *slot) {
  if (!arena || !slot) return RPLGPU_ERR_INVALID_ARG;
  const uint64_t n = cursor < slot_points ? cursor : slot_points;
  for (uint64_t i = 0; i < n; ++i) {
    slot[3 * i] = arena[4 * i];
    slot[3 * i + 1] = arena[4 * i + 1];
    slot[3 * i + 2] = arena[4 * i + 3];
  }
  return RPLGPU_OK;
}

int32_t rplgpu_unpack_gathered_host(const float *points_all, uint64_t slot_points,
                                    uint32_t point_floats, const uint32_t *meta_all,
                                    uint32_t meta_words, uint32_t world, uint32_t max_scans,
                                    float *packed, uint64_t *total, uint64_t *scan_start_all,
                                    uint32_t *n_points_all, uint32_t *status) {
  if (!points_all || !meta_all || !packed || !total || !scan_start_all || !n_points_all ||
      world == 0 || world > 4096 || (point_floats != 3u && point_floats != 4u) ||
      meta_words < rplgpu_cloud_meta_words(max_scans))
    return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t r = 0; r < world; ++r) {
    unsigned long long off, mine, all;
    rpl::layout::rank_extent(meta_all, meta_words, world, slot_points, r, &off, &mine, &all);
    const uint32_t *m = meta_all + (size_t)r * meta_words;
    if (r == 0) *total = all;
    if (status) status[r] = (m[3] & 1u) ? RPLGPU_SCAN_OUT_TRUNCATED : 0u;
    for (uint32_t s = 0; s < max_scans; ++s) {
      unsigned long long st;
      rpl::layout::scan_row(m, s, max_scans, off, &st, &n_points_all[(size_t)r * max_scans + s]);
      scan_start_all[(size_t)r * max_scans + s] = st;
    }
    const float *src = points_all + (size_t)r * slot_points * point_floats;
    float *dst = packed + 4u * off;
    for (unsigned long long i = 0; i < mine; ++i) {
      if (point_floats == 3u) {
        dst[4 * i] = src[3 * i]; dst[4 * i + 1] = src[3 * i + 1]; dst[4 * i + 2] = 0.0f; dst[4 * i + 3] = src[3 * i + 2];
      } else {
        std::memcpy(dst + 4 * i, src + 4 * i, 16);
      }
    }
  }
  return RPLGPU_OK;
}

int32_t rplgpu_merge_cells_host(const rplgpu_cell_t *cells_all, uint64_t slot_cells,
                                const uint32_t *meta_all, uint32_t meta_words, uint32_t world,
                                uint32_t n_groups, const rplgpu_params_t *p, float *arena,
                                uint64_t arena_capacity, uint64_t *cursor, uint64_t *group_start,
                                uint32_t *n_points, uint32_t *status) {
  if (!merge_args_ok(cells_all, meta_all, meta_words, world, n_groups, p, arena, cursor, group_start,
                     n_points) ||
      slot_cells > (0x7FFFFFFFull / world))
    return RPLGPU_ERR_INVALID_ARG;
  const double unit = 1.0 / to_kparams(*p).vox_scale;
  std::vector<unsigned long long> first(world), n(world), at(world);
  unsigned long long total = 0ull;
  for (uint32_t g = 0; g < n_groups; ++g) {
    bool cut = false;
    for (uint32_t r = 0; r < world; ++r) {
      const uint32_t *m = meta_all + (size_t)r * meta_words;
      unsigned long long st;
      rpl::cells::group_extent(m, g, n_groups, slot_cells, &st, &n[r]);
      first[r] = (unsigned long long)r * slot_cells + st;
      at[r] = 0ull;
      cut = cut || rpl::cells::group_cut(m, g);
    }
    // k-way merge of the ranks' sorted lists: the smallest key left, summed over every rank holding it
    const unsigned long long start = total;
    unsigned long long cells = 0ull;
    while (true) {
      uint32_t key = 0xFFFFFFFFu;
      bool any = false;
      for (uint32_t r = 0; r < world; ++r)
        if (at[r] < n[r] && (!any || cells_all[first[r] + at[r]].key < key)) {
          key = cells_all[first[r] + at[r]].key;
          any = true;
        }
      if (!any) break;
      uint32_t cnt = 0u, isum = 0u;
      double sx = 0.0, sy = 0.0;
      for (uint32_t r = 0; r < world; ++r) {
        if (at[r] < n[r] && cells_all[first[r] + at[r]].key == key) {
          const rplgpu_cell_t &c = cells_all[first[r] + at[r]++];
          cnt += c.count;
          isum += c.isum;
          sx += c.sx;
          sy += c.sy;
        }
      }
      const unsigned long long o = start + cells++;
      if (o < arena_capacity) rpl::cells::cell_point(cnt, isum, sx, sy, unit, arena + 4u * o);
    }
    const unsigned long long room = start >= arena_capacity ? 0ull : arena_capacity - start;
    const uint32_t kept = (uint32_t)std::min(cells, room);
    group_start[g] = start;
    n_points[g] = kept;
    if (status) status[g] = (cut || kept < cells) ? RPLGPU_SCAN_OUT_TRUNCATED : 0u;
    total += cells;
  }
  *cursor = total;
  return RPLGPU_OK;
}

}  // extern "C"
