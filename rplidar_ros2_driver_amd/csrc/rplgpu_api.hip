// rplgpu_api.hip — the extern "C" boundary declared in include/rplgpu.h.
//
// Host side only: context/stream management, the host-evaluated lookup tables, the
// pinned staging used by the single-scan (host buffer) entry points, and argument
// checking.  All arithmetic on samples happens in rpl_kernels.hip.  There is no CPU
// fallback: if no gfx950 device is usable, rplgpu_create fails.
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
#include "rpl_msg.hpp"
#include "rpl_comm_layout.hpp"
#include "rpl_cells.hpp"

// which batch the voxel queue statistics in pinned memory describe (voxel_split_for)
struct VoxelBatchId {
  const void *nodes = nullptr;
  uint32_t n_stride = 0, B = 0, group = 0;
  bool operator==(const VoxelBatchId &o) const {
    return nodes == o.nodes && n_stride == o.n_stride && B == o.B && group == o.group;
  }
};

struct rplgpu_ctx {
  int device = -1;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  uint32_t max_n = 0, max_b = 0;
  // tables
  float *d_angle = nullptr, *d_angle_inv = nullptr, *d_inc = nullptr, *d_rinc = nullptr;
  float2 *d_cs = nullptr, *d_cs_inv = nullptr;
  double *d_rcp = nullptr;
  // single-scan staging
  unsigned char *h_pin = nullptr;  // pinned: nodes | out (16 B / sample) | 2 x u32
  unsigned char *d_pin = nullptr;  // the same memory as the device sees it (zero-copy single scans)
  bool zero_copy = true;           // single-scan entry points: kernels read / write h_pin directly
  bool spin_sync = true;           // ... and complete through a flag in pinned memory (wait_scan)
  size_t flag_off = 0;             // offset of that flag in h_pin
  uint32_t scan_seq = 0;
  struct Pinned { unsigned char *host, *dev; size_t bytes; };
  std::vector<Pinned> pinned;      // buffers handed out by rplgpu_host_alloc (device-addressable)
  unsigned char *d_nodes = nullptr, *d_out = nullptr;
  uint32_t *d_rormask = nullptr;  // E5 keep bits, max_b scans x kMaskStride words
  uint32_t *d_redo = nullptr;     // E5 inside the voxel kernel: [0] work items left to the two-kernel path, [4 ...] which
  int32_t ror_fused = 1;          // RPLGPU_ROR_FUSED=0: always the two kernels (tests / A-B runs)
  uint32_t *d_need_sort = nullptr;  // ascend: [0] how many scans the sorting kernel must redo, [1..] which (B + 1 words)
  uint32_t need_sort_cap = 0;
  uint32_t *d_small = nullptr;  // [0]=n, [1]=count, [2]=status, [8]=divide-validation mismatches, [16] voxel work
                                // counter, [20..21] single-scan ascend list, [24..27] voxel queue statistics
  // fast-divide validation cache (see k_validate_div)
  bool div4000_ok = false;
  float leaf_checked = 0.0f;
  bool leaf_ok = false;
  bool idx_checked = false, idx_ok = false;  // Mode A bin-index divide, see k_validate_idx
  // rplgpu_debug_force_ieee_div (tests): bits of rplgpu_debug_fast_div to treat as "validation failed".
  // Kept apart from the *_ok flags: they go on recording what the validators found.
  uint32_t force_ieee = 0;
  unsigned long long *dbg = nullptr;  // developer aid: per-block phase cycle counters
  uint32_t *cell_keys = nullptr;      // optional cell-key output of the voxel kernel (rplgpu_set_cell_key_output)
  const float *scan_t0 = nullptr;     // optional per-scan time offsets of E6 (rplgpu_set_scan_time_offsets_dev)
  // k_cloud_voxel's queue statistics of the previous launch, copied to pinned memory behind every
  // launch (no synchronisation): they choose the kernel instance of the NEXT launch (voxel_split)
  unsigned long long *h_vstats = nullptr;
  uint32_t stats_group = 1;           // scans per work item of the launch the statistics come from
  bool stats_valid = false;           // ... and which batch that launch was over (voxel_split_for)
  VoxelBatchId stats_id;
  // the decision per batch identity, for the last few identities (a caller that alternates two staging
  // buffers, or launches a batch in chunks — rplgpu's own exchange pipeline does — has several alive)
  struct VoxelDecision { VoxelBatchId id; bool split = false; bool valid = false; };
  VoxelDecision decisions[8];
  uint32_t next_decision = 0;
  int32_t last_split = 0;             // the instance the last batch launch took (rplgpu_debug_voxel_instance)
  uint32_t n_cu = 0;                  // compute units of `device`
  void *d_vstore = nullptr;           // k_cloud_voxel record stores (one per resident workgroup)
  int32_t force_split = -1;           // RPLGPU_VOXEL_SPLIT: -1 follow the statistics, 0 / 1 forced
  bool dec_stage = true;              // RPLGPU_DEC_STAGE=0: the plain decoder only (tests / A-B runs)
  uint32_t vstore_wgs = 0;
  uint32_t vstore_recs = 0;           // records per workgroup (grows with the largest E8 group seen)
  uint32_t *d_merge = nullptr;        // rplgpu_merge_cells_dev scratch (world x slot_cells words, grown on demand)
  size_t merge_cap = 0;               // (words)
  // rplgpu_merge_scans_dev (E9): key rows (G x count u64, all ~0 between launches) and the edge table of
  // the last spec (e_0 .. e_count), both grown on demand
  unsigned long long *d_mkeys = nullptr;
  size_t mkeys_cap = 0;               // (keys)
  bool mkeys_clean = true;            // false from the merge launch until its finishing launch is queued
  float2 *d_medges = nullptr;
  size_t medges_cap = 0;              // (edges)
  bool mspec_valid = false;           // d_medges / mspec_k hold the table of mspec
  rplgpu_scan_merge_t mspec;
  rpl::MergeK mspec_k;
  unsigned char *d_dec = nullptr;     // rplgpu_decode_stream staging (grown on demand, kept)
  size_t dec_cap = 0;
  unsigned char *d_scans = nullptr;   // rplgpu_decode_scans_dev scratch (node streams, sync lists)
  size_t scans_cap = 0;
  uint32_t *d_dec_todo = nullptr;     // rplgpu_decode_batch_dev with frame offsets: streams the staged decoder leaves to the plain one
  size_t dec_todo_cap = 0;            // (words)
  bool check_ptrs = true;             // batch entry points verify that buffers are device memory
  // multi-GPU exchange (include/rplgpu_comm.h)
  void *comm = nullptr;               // ncclComm_t
  int32_t comm_rank = 0, comm_world = 0;
  hipStream_t xstream = nullptr;      // exchange stream
  hipEvent_t ev_main = nullptr, ev_x[4] = {nullptr, nullptr, nullptr, nullptr};  // ring of exchange-done events
  uint32_t n_exchanges = 0;
  std::string err;
};

struct rplgpu_nccl_id_t {
  char internal[128];  // == ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES)
};

namespace {

constexpr uint32_t kMaskStride = rpl::kMaxN / 32u;  // keep-mask words per scan
constexpr size_t kTail = 64;  // bytes behind a staging region for the words that travel with it

// Single-scan staging (pinned, one allocation): nodes | tail | results (16 B / sample) | tail | flag.
// Both regions are rounded up to 64 bytes, so that for EVERY capacity the result area (it receives
// 16-byte stores) and the flag word's cache line start on a 64-byte boundary.
constexpr size_t round64(size_t v) { return (v + 63u) & ~(size_t)63u; }
constexpr size_t stage_out_off(size_t max_n) { return round64(max_n * 8) + kTail; }
constexpr size_t stage_flag_off(size_t max_n) { return stage_out_off(max_n) + round64(max_n * 16) + kTail; }
constexpr size_t stage_bytes(size_t max_n) { return stage_flag_off(max_n) + kTail; }

thread_local std::string g_create_err;

#define RPL_HIP(ctx, call)                                                              \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
      return RPLGPU_ERR_HIP;                                                            \
    }                                                                                   \
  } while (0)

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
                    uint32_t B, bool own_buffers = false) {  // (the handle's own staging: no pointer check)
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

// What the launch sites consult: the validators' verdicts, less what rplgpu_debug_force_ieee_div refuses.
inline bool use_fast_d4000(const rplgpu_ctx *c) { return c->div4000_ok && !(c->force_ieee & 1u); }
inline bool use_fast_leaf(const rplgpu_ctx *c) { return c->leaf_ok && !(c->force_ieee & 2u); }
inline bool use_fast_idx(const rplgpu_ctx *c) { return c->idx_ok && !(c->force_ieee & 4u); }

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

// Single-scan staging (pinned host side): nodes | length word ... results | result words.
inline unsigned char *stage_out(const rplgpu_ctx *c) { return c->h_pin + stage_out_off(c->max_n); }

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

// ---- E9: one merged LaserScan per group of scans (include/rplgpu_msg.h) ---------------------------

int32_t rplgpu_scan_merge_edges(const rplgpu_scan_merge_t *m, float *edges, float *inc) {
  if (!m) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(m->angle_min) || !std::isfinite(m->angle_max) || !std::isfinite(m->range_min) ||
      !std::isfinite(m->range_max) || !std::isfinite(m->scan_time))
    return RPLGPU_ERR_INVALID_ARG;
  if (m->count == 0 || m->count > RPLGPU_MAX_MERGE_BEAMS) return RPLGPU_ERR_INVALID_ARG;
  const double span = (double)m->angle_max - (double)m->angle_min;
  const float f_inc = (float)(span / (double)m->count);
  if (!(f_inc > 0.0f) || f_inc > (float)(M_PI / 2)) return RPLGPU_ERR_INVALID_ARG;
  if (span > 2.0 * M_PI * (1.0 + 0x1p-20)) return RPLGPU_ERR_INVALID_ARG;
  if (!(0.0f <= m->range_min && m->range_min < m->range_max)) return RPLGPU_ERR_INVALID_ARG;
  if (edges)
    for (uint32_t k = 0; k <= m->count; ++k) {
      const double phi = (double)m->angle_min + (double)k * (double)f_inc;
      edges[2 * k] = (float)std::cos(phi);
      edges[2 * k + 1] = (float)std::sin(phi);
    }
  if (inc) *inc = f_inc;
  return RPLGPU_OK;
}

namespace {

// e_a -> e_b turns by an angle in (0, pi): the exact sign of the fp64 cross product of float vectors
bool turns_left(float2 a, float2 b) { return (double)a.x * (double)b.y - (double)a.y * (double)b.x > 0.0; }

// the edge table of spec `m` on the device and the kernel's view of it (cached per spec)
int32_t merge_spec_upload(rplgpu_ctx *c, const rplgpu_scan_merge_t &m, rpl::MergeK *out) {
  if (c->mspec_valid && std::memcmp(&c->mspec, &m, sizeof(m)) == 0) {
    *out = c->mspec_k;
    return RPLGPU_OK;
  }
  std::vector<float2> e(m.count + 1u);
  float inc = 0.0f;
  if (rplgpu_scan_merge_edges(&m, reinterpret_cast<float *>(e.data()), &inc) != RPLGPU_OK) {
    c->err = "rplgpu_scan_merge_t: invalid spec (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  // the table in use may still be read by queued launches
  RPL_HIP(c, hipStreamSynchronize(c->stream));
  c->mspec_valid = false;
  if (e.size() > c->medges_cap) {
    if (c->d_medges) (void)hipFree(c->d_medges);
    c->d_medges = nullptr;
    c->medges_cap = 0;
    RPL_HIP(c, hipMalloc((void **)&c->d_medges, e.size() * sizeof(float2)));
    c->medges_cap = e.size();
  }
  RPL_HIP(c, hipMemcpy(c->d_medges, e.data(), e.size() * sizeof(float2), hipMemcpyHostToDevice));
  rpl::MergeK k;
  k.edges = c->d_medges;
  k.count = m.count;
  bool mono = true;
  for (uint32_t i = 0; i < m.count && mono; ++i) mono = turns_left(e[i], e[i + 1]);
  for (int q = 0; q < 5; ++q) {
    k.qb[q] = (uint32_t)((uint64_t)q * m.count / 4u);
    k.qe[q] = e[k.qb[q]];
  }
  for (int q = 0; q < 4 && mono; ++q)
    if (k.qb[q] != k.qb[q + 1]) mono = turns_left(k.qe[q], k.qe[q + 1]);
  k.monotone = mono ? 1u : 0u;
  double a0 = std::fmod((double)m.angle_min, 2.0 * M_PI);
  if (a0 < 0.0) a0 += 2.0 * M_PI;
  k.a0 = (float)a0;
  k.rinc = 1.0f / inc;
  k.range_min = m.range_min;
  k.range_max = m.range_max;
  c->mspec = m;
  c->mspec_k = k;
  c->mspec_valid = true;
  *out = k;
  return RPLGPU_OK;
}

}  // namespace

int32_t rplgpu_merge_scans_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                               const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                               const rplgpu_scan_merge_t *m, float *d_ranges, float *d_intensities,
                               uint32_t *d_beams_hit, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !m || !d_ranges || !d_intensities || !d_beams_hit || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_merge_edges(m, nullptr, nullptr) != RPLGPU_OK) {
    h->err = "rplgpu_merge_scans_dev: invalid rplgpu_scan_merge_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if ((d_motion && !device_readable(h, d_motion, "d_motion")) ||
      (d_pose2d && !device_readable(h, d_pose2d, "d_pose2d")) ||
      !device_readable(h, d_ranges, "d_ranges") || !device_readable(h, d_intensities, "d_intensities") ||
      !device_readable(h, d_beams_hit, "d_beams_hit") || (d_status && !device_readable(h, d_status, "d_status")))
    return RPLGPU_ERR_INVALID_ARG;
  if (h->scan_t0 && !d_motion) {
    h->err = "rplgpu_merge_scans_dev: scan time offsets are set (rplgpu_set_scan_time_offsets_dev) but d_motion is NULL";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (p->ror_enable && !(p->ror_radius > 0.0f && p->ror_radius <= 1.0e6f)) {
    h->err = "ror_radius must be in (0, 1e6] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  group = std::min(group, B);  // as E8: "all sensors in one scan" may be asked for with any group >= B
  if ((uint64_t)group * std::min(n_stride, rpl::kMaxN) > (1ull << 24) || group > (1u << rpl::kMergeSlotBits)) {
    h->err = "rplgpu_merge_scans_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_CAPACITY;
  }
  const uint32_t G = (B + group - 1u) / group;
  RPL_HIP(h, hipSetDevice(h->device));
  rpl::MergeK mk;
  if ((rc = merge_spec_upload(h, *m, &mk))) return rc;
  const size_t need = (size_t)G * m->count;
  if (need > h->mkeys_cap) {  // (only ever grows; fresh rows are empty)
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    if (h->d_mkeys) (void)hipFree(h->d_mkeys);
    h->d_mkeys = nullptr;
    h->mkeys_cap = 0;
    if (hipMalloc((void **)&h->d_mkeys, need * sizeof(unsigned long long)) != hipSuccess) {
      h->err = "merge key rows allocation failed";
      (void)hipGetLastError();
      return RPLGPU_ERR_HIP;
    }
    h->mkeys_cap = need;
    h->mkeys_clean = false;
  }
  if (!h->mkeys_clean)  // a new allocation, or a call that failed between the two launches
    RPL_HIP(h, hipMemsetAsync(h->d_mkeys, 0xFF, h->mkeys_cap * sizeof(unsigned long long), h->stream));
  rpl::KParams kp = to_kparams(*p);
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  const rpl::Tables T = tables_of(h);
  const uint32_t *mask = nullptr;
  if (p->ror_enable) {  // E1 AND E5 keep bits, the mask E8's two-kernel path applies
    RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, T, h->d_rormask,
                                    kMaskStride));
    mask = h->d_rormask;
  }
  RPL_HIP(h, hipMemsetAsync(d_beams_hit, 0, (size_t)G * 4u, h->stream));
  if (d_status) RPL_HIP(h, hipMemsetAsync(d_status, 0, (size_t)G * 4u, h->stream));
  h->mkeys_clean = false;
  RPL_HIP(h, rpl::launch_merge_scans(h->stream, d_nodes, n_stride, d_n_per_scan, B, group, kp, T, mask,
                                     kMaskStride, d_motion, d_pose2d, mk, h->d_mkeys, d_status));
  RPL_HIP(h, rpl::launch_merge_finish(h->stream, h->d_mkeys, G, m->count, d_nodes, n_stride, group,
                                      p->is_new_protocol, d_ranges, d_intensities, d_beams_hit));
  h->mkeys_clean = true;
  return RPLGPU_OK;
}

int32_t rplgpu_merged_laserscan_msgs_dev(rplgpu_handle_t h, const float *d_ranges,
                                         const float *d_intensities, uint32_t G,
                                         const rplgpu_scan_merge_t *m, const char *frame_id,
                                         const rplgpu_stamp_t *d_stamps, uint8_t *d_msgs,
                                         uint32_t msg_stride, uint32_t *d_msg_len, uint32_t *d_status) {
  if (!h || !m || !frame_id) return RPLGPU_ERR_INVALID_ARG;
  float inc = 0.0f;
  if (rplgpu_scan_merge_edges(m, nullptr, &inc) != RPLGPU_OK) {
    h->err = "rplgpu_merged_laserscan_msgs_dev: invalid rplgpu_scan_merge_t";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_stamps || !d_msgs || !d_msg_len || (msg_stride & 3u))
    return RPLGPU_ERR_INVALID_ARG;
  const size_t fl = std::strlen(frame_id);
  if (fl > rplmsg::kMaxFrameId) {
    h->err = "frame_id longer than 255 bytes";
    return RPLGPU_ERR_INVALID_ARG;
  }
  rplgpu_scan_meta_t meta;
  std::memset(&meta, 0, sizeof(meta));
  meta.angle_min = m->angle_min;
  meta.angle_max = m->angle_max;
  meta.angle_increment = inc;
  meta.time_increment = 0.0f;  // every point is already moved to the fused instant
  meta.scan_time = m->scan_time;
  meta.range_min = m->range_min;
  meta.range_max = m->range_max;
  meta.count = m->count;
  meta.published = 1;
  rplmsg::Prefix P;
  std::memset(&P, 0, sizeof(P));
  rplmsg::Writer w(reinterpret_cast<uint8_t *>(P.words), sizeof(P.words));
  rplgpu_laserscan_layout_t L;
  rplmsg::write_laserscan(w, frame_id, fl, rplgpu_stamp_t{0, 0}, meta, &L);
  P.stamp_off = 4;
  P.len = L.ranges_off;  // every scalar and the ranges length word come with the template
  P.a_off = L.scalars_off;
  P.b_off = L.ranges_len_off;
  if (P.len > sizeof(P.words) || (P.len & 3u)) {
    h->err = "message prefix does not fit the device template";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_msg_merged(h->stream, d_ranges, d_intensities, m->count, G, d_stamps, P, d_msgs,
                                    msg_stride, d_msg_len, d_status));
  return RPLGPU_OK;
}

// ---- E10: scan-shadow and speckle filters on LaserScan arrays (include/rplgpu_msg.h) ---------------

void rplgpu_default_scan_filter(rplgpu_scan_filter_t *f) {
  if (!f) return;
  f->shadow_enable = 1;
  f->shadow_min_angle = (float)(10.0 * M_PI / 180.0);
  f->shadow_max_angle = (float)(170.0 * M_PI / 180.0);
  f->shadow_window = 2;
  f->shadow_neighbors = 1;
  f->speckle_enable = 1;
  f->speckle_max_range_difference = 0.05f;
  f->speckle_min_run = 4;
  f->circular = 1;
}

int32_t rplgpu_scan_filter_check(const rplgpu_scan_filter_t *f, float dirs[4]) {
  if (!f) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(f->shadow_min_angle) || !std::isfinite(f->shadow_max_angle) ||
      !std::isfinite(f->speckle_max_range_difference))
    return RPLGPU_ERR_INVALID_ARG;
  const double lo = (double)f->shadow_min_angle, hi = (double)f->shadow_max_angle;
  if (!(0.0 < lo && lo < M_PI / 2 && M_PI / 2 < hi && hi < M_PI)) return RPLGPU_ERR_INVALID_ARG;
  if (f->shadow_window < 1u || f->shadow_window > RPLGPU_MAX_FILTER_WINDOW ||
      f->shadow_neighbors > RPLGPU_MAX_FILTER_WINDOW || f->speckle_min_run < 1u ||
      f->speckle_min_run > RPLGPU_MAX_FILTER_WINDOW || !(f->speckle_max_range_difference >= 0.0f))
    return RPLGPU_ERR_INVALID_ARG;
  if (dirs) {
    dirs[0] = (float)std::cos(lo);
    dirs[1] = (float)std::sin(lo);
    dirs[2] = (float)std::cos(hi);
    dirs[3] = (float)std::sin(hi);
  }
  return RPLGPU_OK;
}

namespace {

int32_t filter_kernel_args(rplgpu_ctx *c, const rplgpu_scan_filter_t *f, rpl::FilterK *k) {
  float dirs[4];
  if (rplgpu_scan_filter_check(f, dirs) != RPLGPU_OK) {
    c->err = "invalid rplgpu_scan_filter_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  std::memset(k, 0, sizeof(*k));
  k->shadow = f->shadow_enable ? 1u : 0u;
  k->speckle = f->speckle_enable ? 1u : 0u;
  k->circular = f->circular ? 1u : 0u;
  k->W = f->shadow_window;
  k->N = f->shadow_neighbors;
  k->L = f->speckle_min_run;
  k->D = f->speckle_max_range_difference;
  k->cmin = dirs[0];
  k->smin = dirs[1];
  k->cmax = dirs[2];
  k->smax = dirs[3];
  return RPLGPU_OK;
}

}  // namespace

int32_t rplgpu_filter_laserscan_batch_dev(rplgpu_handle_t h, const float *d_ranges, const float *d_intensities,
                                          uint32_t n_stride, const uint32_t *d_beam_count, uint32_t B,
                                          const rplgpu_params_t *p, const rplgpu_scan_filter_t *f,
                                          float *d_ranges_out, float *d_intensities_out, uint32_t *d_removed) {
  if (!h || !p || !f) return RPLGPU_ERR_INVALID_ARG;
  rpl::FilterK k;
  if (int32_t rc = filter_kernel_args(h, f, &k)) return rc;
  if (B == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_beam_count || !d_ranges_out || !d_intensities_out || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (d_ranges_out == d_ranges || d_intensities_out == d_intensities) {
    h->err = "rplgpu_filter_laserscan_batch_dev: the filters do not work in place";
    return RPLGPU_ERR_INVALID_ARG;
  }
  k.inc_mode = p->scan_processing ? rpl::kFilterIncModeA : rpl::kFilterIncModeB;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_removed) RPL_HIP(h, hipMemsetAsync(d_removed, 0, (size_t)B * 8u, h->stream));
  RPL_HIP(h, rpl::launch_filter_scans(h->stream, d_ranges, d_intensities, n_stride, d_beam_count, B, k,
                                      d_ranges_out, d_intensities_out, d_removed));
  return RPLGPU_OK;
}

int32_t rplgpu_filter_merged_scans_dev(rplgpu_handle_t h, const float *d_ranges, const float *d_intensities,
                                       uint32_t G, const rplgpu_scan_merge_t *m, const rplgpu_scan_filter_t *f,
                                       float *d_ranges_out, float *d_intensities_out, uint32_t *d_removed) {
  if (!h || !m || !f) return RPLGPU_ERR_INVALID_ARG;
  rpl::FilterK k;
  if (int32_t rc = filter_kernel_args(h, f, &k)) return rc;
  float inc = 0.0f;
  if (rplgpu_scan_merge_edges(m, nullptr, &inc) != RPLGPU_OK) {
    h->err = "rplgpu_filter_merged_scans_dev: invalid rplgpu_scan_merge_t";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0) return RPLGPU_OK;
  if (!d_ranges || !d_intensities || !d_ranges_out || !d_intensities_out) return RPLGPU_ERR_INVALID_ARG;
  if (d_ranges_out == d_ranges || d_intensities_out == d_intensities) {
    h->err = "rplgpu_filter_merged_scans_dev: the filters do not work in place";
    return RPLGPU_ERR_INVALID_ARG;
  }
  k.inc_mode = rpl::kFilterIncGiven;
  k.inc = inc;
  k.count = m->count;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_removed) RPL_HIP(h, hipMemsetAsync(d_removed, 0, (size_t)G * 8u, h->stream));
  RPL_HIP(h, rpl::launch_filter_scans(h->stream, d_ranges, d_intensities, m->count, nullptr, G, k,
                                      d_ranges_out, d_intensities_out, d_removed));
  return RPLGPU_OK;
}

int32_t rplgpu_filter_laserscan(rplgpu_handle_t h, const float *ranges, const float *intensities, uint32_t count,
                                float angle_increment, const rplgpu_scan_filter_t *f, float *ranges_out,
                                float *intensities_out, uint32_t removed[2]) {
  if (!h || !f) return RPLGPU_ERR_INVALID_ARG;
  rpl::FilterK k;
  if (int32_t rc = filter_kernel_args(h, f, &k)) return rc;
  if (!std::isfinite(angle_increment) || !(angle_increment > 0.0f)) {
    h->err = "rplgpu_filter_laserscan: angle_increment must be finite and positive";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (count && (!ranges || !intensities || !ranges_out || !intensities_out)) return RPLGPU_ERR_INVALID_ARG;
  if (count && (ranges_out == ranges || intensities_out == intensities)) {
    h->err = "rplgpu_filter_laserscan: the filters do not work in place";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (count > h->max_n) return RPLGPU_ERR_CAPACITY;
  if (removed) removed[0] = removed[1] = 0u;
  if (count == 0) return RPLGPU_OK;
  k.inc_mode = rpl::kFilterIncGiven;
  k.inc = angle_increment;
  k.count = count;
  RPL_HIP(h, hipSetDevice(h->device));
  // staging as rplgpu_laserscan_to_cloud: ranges | intensities in (d_nodes holds 8 B per sample),
  // ranges | intensities | the two counts out (d_out holds 16 B per sample)
  const size_t n = count;
  std::memcpy(h->h_pin, ranges, n * 4);
  std::memcpy(h->h_pin + n * 4, intensities, n * 4);
  RPL_HIP(h, hipMemcpyAsync(h->d_nodes, h->h_pin, n * 8, hipMemcpyHostToDevice, h->stream));
  const float *d_r = reinterpret_cast<const float *>(h->d_nodes);
  float *d_o = reinterpret_cast<float *>(h->d_out);
  uint32_t *d_rm = reinterpret_cast<uint32_t *>(h->d_out + n * 8);
  RPL_HIP(h, hipMemsetAsync(d_rm, 0, 8, h->stream));
  RPL_HIP(h, rpl::launch_filter_scans(h->stream, d_r, d_r + n, count, nullptr, 1, k, d_o, d_o + n, d_rm));
  unsigned char *h_out = stage_out(h);
  RPL_HIP(h, hipMemcpyAsync(h_out, h->d_out, n * 8 + 8, hipMemcpyDeviceToHost, h->stream));
  RPL_HIP(h, hipStreamSynchronize(h->stream));
  std::memcpy(ranges_out, h_out, n * 4);
  std::memcpy(intensities_out, h_out + n * 4, n * 4);
  if (removed) std::memcpy(removed, h_out + n * 8, 8);
  return RPLGPU_OK;
}

// ---- E11: one ray-cast occupancy grid per group of scans (include/rplgpu_msg.h) ---------------------

void rplgpu_default_occ_grid(rplgpu_occ_grid_t *grid) {
  if (!grid) return;
  grid->origin_x = -25.6f;
  grid->origin_y = -25.6f;
  grid->resolution = 0.05f;
  grid->width = 1024;
  grid->height = 1024;
  grid->range_min = 0.0f;
  grid->obstacle_max = 25.0f;
  grid->raytrace_max = 30.0f;
}

int32_t rplgpu_occ_grid_check(const rplgpu_occ_grid_t *g) {
  if (!g) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(g->origin_x) || !std::isfinite(g->origin_y) || !std::isfinite(g->resolution) ||
      !std::isfinite(g->range_min) || !std::isfinite(g->obstacle_max) || !std::isfinite(g->raytrace_max))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(g->resolution > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (g->width == 0 || g->width > RPLGPU_MAX_OCC_DIM || g->height == 0 || g->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (!(0.0f <= g->range_min && g->range_min < g->obstacle_max && g->obstacle_max <= g->raytrace_max))
    return RPLGPU_ERR_INVALID_ARG;
  if ((double)g->raytrace_max / (double)g->resolution > (double)RPLGPU_MAX_OCC_STEPS) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

static rpl::OccK occ_kernel_args(const rplgpu_occ_grid_t &g) {
  return rpl::OccK{g.origin_x, g.origin_y, g.resolution, g.width, g.height, g.range_min, g.obstacle_max,
                   g.raytrace_max};
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t occ_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                        const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                        const float *d_motion, const float *d_pose2d, const float *d_t0,
                        const rplgpu_occ_grid_t *grid, const int8_t *d_prev, int8_t *d_grid,
                        uint64_t grid_stride, uint32_t *d_cells, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !grid || !d_grid || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_occupancy_grid_dev: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (grid_stride < (uint64_t)grid->width * grid->height || (grid_stride & 3u) ||
      (reinterpret_cast<uintptr_t>(d_grid) & 3u)) {
    h->err = "rplgpu_occupancy_grid_dev: grid_stride must be >= width * height and a multiple of 4, d_grid 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_prev == d_grid) {
    h->err = "rplgpu_occupancy_grid_dev: d_prev must not be d_grid (the grid is its own scratch)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if ((d_motion && !device_readable(h, d_motion, "d_motion")) ||
      (d_pose2d && !device_readable(h, d_pose2d, "d_pose2d")) ||
      (d_prev && !device_readable(h, d_prev, "d_prev")) || !device_readable(h, d_grid, "d_grid") ||
      (d_cells && !device_readable(h, d_cells, "d_cells")) || (d_status && !device_readable(h, d_status, "d_status")))
    return RPLGPU_ERR_INVALID_ARG;
  if (d_t0 && !d_motion) {
    h->err = "rplgpu_occupancy_grid_dev: scan time offsets are set (rplgpu_set_scan_time_offsets_dev) but d_motion is NULL";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (p->ror_enable && !(p->ror_radius > 0.0f && p->ror_radius <= 1.0e6f)) {
    h->err = "ror_radius must be in (0, 1e6] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  group = std::min(group, B);  // as E8: "all sensors in one grid" may be asked for with any group >= B
  if ((uint64_t)group * std::min(n_stride, rpl::kMaxN) > (1ull << 24)) {
    h->err = "rplgpu_occupancy_grid_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_CAPACITY;
  }
  const uint32_t G = (B + group - 1u) / group;
  RPL_HIP(h, hipSetDevice(h->device));
  rpl::KParams kp = to_kparams(*p);
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  rpl::Tables T = tables_of(h);
  T.scan_t0 = d_t0;
  const rpl::OccK k = occ_kernel_args(*grid);
  const uint32_t *mask = nullptr;
  if (p->ror_enable) {  // E1 AND E5 keep bits, the mask E8's two-kernel path and E9 apply
    RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, T, h->d_rormask,
                                    kMaskStride));
    mask = h->d_rormask;
  }
  if (d_cells) RPL_HIP(h, hipMemsetAsync(d_cells, 0, (size_t)G * 12u, h->stream));
  if (d_status) RPL_HIP(h, hipMemsetAsync(d_status, 0, (size_t)G * 4u, h->stream));
  RPL_HIP(h, rpl::launch_occ_prepare(h->stream, d_grid, grid_stride, G, k));
  RPL_HIP(h, rpl::launch_occ_walk(h->stream, d_nodes, n_stride, d_n_per_scan, B, group, kp, T, mask, kMaskStride,
                                  d_motion, d_pose2d, k, d_grid, grid_stride, d_status));
  RPL_HIP(h, rpl::launch_occ_finish(h->stream, d_grid, grid_stride, G, k, d_prev, d_cells));
  return RPLGPU_OK;
}

int32_t rplgpu_occupancy_grid_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                  const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                                  const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                                  const rplgpu_occ_grid_t *grid, const int8_t *d_prev, int8_t *d_grid,
                                  uint64_t grid_stride, uint32_t *d_cells, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return occ_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, grid, d_prev,
                  d_grid, grid_stride, d_cells, d_status);
}

int32_t rplgpu_occupancy_grid(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                              const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                              const float *motion, const float *pose2d, const float *t0,
                              const rplgpu_occ_grid_t *grid, const int8_t *prev, int8_t *grid_out,
                              uint32_t cells[3], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !grid || !grid_out || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_occupancy_grid: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)grid->width * grid->height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t nb = (size_t)n_scans * n_stride * 8u;
  // one allocation per call (a convenience door, not the hot path): grid | prev | nodes | lengths |
  // motion | pose | t0 | cells + status, every part 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t o_prev = up16(stride), o_nodes = o_prev + up16(prev ? stride : 0), o_len = o_nodes + up16(nb),
               o_mo = o_len + up16(4u * n_scans), o_po = o_mo + up16(motion ? 16u * n_scans : 0),
               o_t0 = o_po + up16(pose2d ? 24u * n_scans : 0), o_small = o_t0 + up16(t0 ? 4u * n_scans : 0),
               total = o_small + 16u;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_occupancy_grid: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[4] = {0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d + o_nodes, nodes, nb, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_len, n_per_scan, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (prev) RPL_HIP(h, hipMemcpyAsync(d + o_prev, prev, cells_n, hipMemcpyHostToDevice, h->stream));
    if (motion) RPL_HIP(h, hipMemcpyAsync(d + o_mo, motion, 16u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (pose2d) RPL_HIP(h, hipMemcpyAsync(d + o_po, pose2d, 24u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (t0) RPL_HIP(h, hipMemcpyAsync(d + o_t0, t0, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    uint32_t *d_small = reinterpret_cast<uint32_t *>(d + o_small);
    const int32_t rc = occ_impl(
        h, reinterpret_cast<const rplgpu_node_t *>(d + o_nodes), n_stride,
        reinterpret_cast<const uint32_t *>(d + o_len), n_scans, n_scans, p,
        motion ? reinterpret_cast<const float *>(d + o_mo) : nullptr,
        pose2d ? reinterpret_cast<const float *>(d + o_po) : nullptr,
        t0 ? reinterpret_cast<const float *>(d + o_t0) : nullptr, grid,
        prev ? reinterpret_cast<const int8_t *>(d + o_prev) : nullptr, reinterpret_cast<int8_t *>(d), stride,
        d_small, d_small + 3);
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(grid_out, d, cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 16, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  if (cells) std::memcpy(cells, small, 12);
  if (status) *status = small[3];
  return RPLGPU_OK;
}

int32_t rplgpu_msg_occupancy_layout(size_t frame_id_len, uint32_t width, uint32_t height,
                                    rplgpu_occupancy_layout_t *out) {
  if (!out || frame_id_len > (1u << 20) || width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 ||
      height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  rplmsg::Writer w(nullptr, 0);
  std::string fid(frame_id_len, 'x');
  rplmsg::write_occupancy(w, fid.data(), frame_id_len, rplgpu_stamp_t{0, 0}, 1.0f, width, height, 0.0f, 0.0f, out);
  return RPLGPU_OK;
}

int32_t rplgpu_occupancy_grid_msgs_dev(rplgpu_handle_t h, const int8_t *d_grid, uint64_t grid_stride, uint32_t G,
                                       const rplgpu_occ_grid_t *grid, const char *frame_id,
                                       const rplgpu_stamp_t *d_stamps, uint8_t *d_msgs, uint32_t msg_stride,
                                       uint32_t *d_msg_len, uint32_t *d_status) {
  if (!h || !grid || !frame_id) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_occupancy_grid_msgs_dev: invalid rplgpu_occ_grid_t";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0) return RPLGPU_OK;
  if (!d_grid || !d_stamps || !d_msgs || !d_msg_len || (msg_stride & 3u) || (grid_stride & 3u) ||
      grid_stride < (uint64_t)grid->width * grid->height || (reinterpret_cast<uintptr_t>(d_grid) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_msgs) & 3u))
    return RPLGPU_ERR_INVALID_ARG;
  const size_t fl = std::strlen(frame_id);
  if (fl > rplmsg::kMaxFrameId) {
    h->err = "frame_id longer than 255 bytes";
    return RPLGPU_ERR_INVALID_ARG;
  }
  rplmsg::Prefix P;
  std::memset(&P, 0, sizeof(P));
  rplmsg::Writer w(reinterpret_cast<uint8_t *>(P.words), sizeof(P.words));
  rplgpu_occupancy_layout_t L;
  rplmsg::write_occupancy(w, frame_id, fl, rplgpu_stamp_t{0, 0}, grid->resolution, grid->width, grid->height,
                          grid->origin_x, grid->origin_y, &L);
  P.stamp_off = 4;
  P.len = L.data_off;  // every scalar and the data length word come with the template
  P.a_off = L.map_load_time_off;
  if (P.len > sizeof(P.words) || (P.len & 3u)) {
    h->err = "message prefix does not fit the device template";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_msg_occupancy(h->stream, d_grid, grid_stride, grid->width * grid->height, G, d_stamps, P,
                                       d_msgs, msg_stride, d_msg_len, d_status));
  return RPLGPU_OK;
}

// ---- E12: the grids of E11 inflated into costmaps (include/rplgpu_msg.h) -------------------------------

void rplgpu_default_inflation(rplgpu_inflation_t *f) {
  if (!f) return;
  f->inscribed_radius = 0.22f;
  f->inflation_radius = 0.55f;
  f->cost_scaling_factor = 3.0f;
  f->inflate_unknown = 0;
}

// the check, and Rc of a spec that passes it
static int32_t inflation_reach(const rplgpu_inflation_t *f, float resolution, uint32_t *rc) {
  if (!f) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(f->inscribed_radius) || !std::isfinite(f->inflation_radius) ||
      !std::isfinite(f->cost_scaling_factor) || !std::isfinite(resolution))
    return RPLGPU_ERR_INVALID_ARG;
  if (f->inscribed_radius < 0.0f || f->inflation_radius < 0.0f || f->cost_scaling_factor < 0.0f ||
      !(resolution > 0.0f) || f->inflation_radius < f->inscribed_radius || f->inflate_unknown > 1u)
    return RPLGPU_ERR_INVALID_ARG;
  const double cells = std::ceil((double)f->inflation_radius / (double)resolution);
  if (!(cells <= (double)RPLGPU_MAX_INFLATION_CELLS)) return RPLGPU_ERR_INVALID_ARG;
  *rc = (uint32_t)cells;
  return RPLGPU_OK;
}

int32_t rplgpu_inflation_check(const rplgpu_inflation_t *f, float resolution) {
  uint32_t rc = 0;
  return inflation_reach(f, resolution, &rc);
}

int32_t rplgpu_inflation_table(const rplgpu_inflation_t *f, float resolution, uint8_t *table, uint32_t table_cap,
                               uint32_t *rc_out) {
  uint32_t rc = 0;
  if (inflation_reach(f, resolution, &rc) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  if (rc_out) *rc_out = rc;
  if (!table) return RPLGPU_ERR_INVALID_ARG;
  if (table_cap < rc * rc + 1u) return RPLGPU_ERR_CAPACITY;
  const double res = (double)resolution, inscribed = (double)f->inscribed_radius;
  table[0] = 100;
  for (uint32_t k = 1; k <= rc * rc; ++k) {
    const double d = std::sqrt((double)k) * res;
    table[k] = d <= inscribed
                   ? (uint8_t)99
                   : (uint8_t)(int)(98.0 * std::exp(-(double)f->cost_scaling_factor * (d - inscribed)));
  }
  return RPLGPU_OK;
}

int32_t rplgpu_inflate_grids_dev(rplgpu_handle_t h, const int8_t *d_in, uint64_t in_stride, int8_t *d_out,
                                 uint64_t out_stride, uint32_t G, uint32_t width, uint32_t height,
                                 const uint8_t *d_table, uint32_t rc, uint32_t inflate_unknown, uint32_t *d_cells) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  if (!d_in || !d_out || !d_table || G == 0) {
    h->err = "rplgpu_inflate_grids_dev: d_in, d_out and d_table must be given and G >= 1";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_in == d_out) {
    h->err = "rplgpu_inflate_grids_dev: d_out must not be d_in (a tile reads the cells around it)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (rc > RPLGPU_MAX_INFLATION_CELLS || inflate_unknown > 1u) {
    h->err = "rplgpu_inflate_grids_dev: rc above RPLGPU_MAX_INFLATION_CELLS or inflate_unknown above 1";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_inflate_grids_dev: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t n_cells = (uint64_t)width * height;
  if (in_stride < n_cells || (in_stride & 3u) || out_stride < n_cells || (out_stride & 3u) ||
      (reinterpret_cast<uintptr_t>(d_in) & 3u) || (reinterpret_cast<uintptr_t>(d_out) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_table) & 3u) || (reinterpret_cast<uintptr_t>(d_cells) & 3u)) {
    h->err = "rplgpu_inflate_grids_dev: strides must be >= width * height and multiples of 4, pointers 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t tiles = (uint64_t)((width + 63u) / 64u) * ((height + 63u) / 64u);
  if (G * tiles > 0x7FFFFFFFull) {
    h->err = "rplgpu_inflate_grids_dev: G x tiles above 2^31";
    return RPLGPU_ERR_CAPACITY;
  }
  if (!device_readable(h, d_in, "d_in") || !device_readable(h, d_out, "d_out") ||
      !device_readable(h, d_table, "d_table") || (d_cells && !device_readable(h, d_cells, "d_cells")))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_cells) RPL_HIP(h, hipMemsetAsync(d_cells, 0, (size_t)G * 16u, h->stream));
  RPL_HIP(h, rpl::launch_inflate(h->stream, d_in, in_stride, d_out, out_stride, G, width, height, d_table, rc,
                                 inflate_unknown, d_cells));
  return RPLGPU_OK;
}

int32_t rplgpu_inflate_grid(rplgpu_handle_t h, const int8_t *in, uint32_t width, uint32_t height, float resolution,
                            const rplgpu_inflation_t *f, int8_t *out, uint32_t cells[4]) {
  if (!h || !in || !out || !f || in == out) return RPLGPU_ERR_INVALID_ARG;
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_inflate_grid: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  std::vector<uint8_t> table((size_t)RPLGPU_MAX_INFLATION_CELLS * RPLGPU_MAX_INFLATION_CELLS + 1u);
  uint32_t reach = 0;
  if (rplgpu_inflation_table(f, resolution, table.data(), (uint32_t)table.size(), &reach) != RPLGPU_OK) {
    h->err = "rplgpu_inflate_grid: invalid rplgpu_inflation_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)width * height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t n_table = (size_t)reach * reach + 1u;
  // one allocation per call (a convenience door, not the hot path): in | out | table | cells, 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t o_out = up16(stride), o_table = o_out + up16(stride), o_cells = o_table + up16(n_table),
               total = o_cells + 16u;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_inflate_grid: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[4] = {0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d, in, cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_table, table.data(), n_table, hipMemcpyHostToDevice, h->stream));
    const int32_t rc = rplgpu_inflate_grids_dev(h, reinterpret_cast<const int8_t *>(d), stride,
                                                reinterpret_cast<int8_t *>(d + o_out), stride, 1, width, height,
                                                d + o_table, reach, f->inflate_unknown,
                                                reinterpret_cast<uint32_t *>(d + o_cells));
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(out, d + o_out, cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d + o_cells, 16, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  if (cells) std::memcpy(cells, small, 16);
  return RPLGPU_OK;
}

// ---- E13: a time step's scans matched to a likelihood field (include/rplgpu_msg.h) ---------------------------

void rplgpu_default_scan_match(rplgpu_scan_match_t *m) {
  if (!m) return;
  m->origin_x = -25.6f;
  m->origin_y = -25.6f;
  m->resolution = 0.05f;
  m->width = 1024;
  m->height = 1024;
  m->shift_x = 6;
  m->shift_y = 6;
  m->rot_steps = 10;
  m->rot_step = (float)(0.25 * M_PI / 180.0);
}

int32_t rplgpu_scan_match_check(const rplgpu_scan_match_t *m) {
  if (!m) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(m->origin_x) || !std::isfinite(m->origin_y) || !std::isfinite(m->resolution) ||
      !std::isfinite(m->rot_step))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(m->resolution > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (m->width == 0 || m->width > RPLGPU_MAX_OCC_DIM || m->height == 0 || m->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (m->shift_x > RPLGPU_MAX_MATCH_SHIFT || m->shift_y > RPLGPU_MAX_MATCH_SHIFT ||
      m->rot_steps > RPLGPU_MAX_MATCH_ROT)
    return RPLGPU_ERR_INVALID_ARG;
  if (m->rot_steps > 0 && (!(m->rot_step > 0.0f) || (double)m->rot_steps * (double)m->rot_step > M_PI / 2.0))
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

int32_t rplgpu_scan_match_rotations(const rplgpu_scan_match_t *m, float *cs) {
  if (!cs || rplgpu_scan_match_check(m) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  const int K = (int)m->rot_steps;
  for (int k = -K; k <= K; ++k) {
    const double a = (double)k * (double)m->rot_step;
    cs[2 * (k + K)] = (float)std::cos(a);
    cs[2 * (k + K) + 1] = (float)std::sin(a);
  }
  return RPLGPU_OK;
}

uint32_t rplgpu_scan_match_volume(const rplgpu_scan_match_t *m) {
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) return 0;
  return (2u * m->rot_steps + 1u) * (2u * m->shift_y + 1u) * (2u * m->shift_x + 1u);
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t match_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                          const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                          const float *d_motion, const float *d_pose2d, const float *d_t0, const float *d_pivot,
                          const rplgpu_scan_match_t *m, const int8_t *d_field, uint64_t field_stride,
                          uint32_t field_per_group, uint32_t *d_scores, uint64_t score_stride, uint32_t *d_best,
                          uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !m || !d_field || !d_scores || !d_best || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_match_scans_dev: invalid rplgpu_scan_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (field_stride < (uint64_t)m->width * m->height || (field_stride & 3u) ||
      (reinterpret_cast<uintptr_t>(d_field) & 3u)) {
    h->err = "rplgpu_match_scans_dev: field_stride must be >= width * height and a multiple of 4, d_field 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint32_t volume = rplgpu_scan_match_volume(m);
  if (score_stride < volume || (reinterpret_cast<uintptr_t>(d_scores) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_best) & 3u) || (reinterpret_cast<uintptr_t>(d_status) & 3u)) {
    h->err = "rplgpu_match_scans_dev: score_stride must be >= the volume size, d_scores / d_best / d_status 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if ((d_motion && !device_readable(h, d_motion, "d_motion")) ||
      (d_pose2d && !device_readable(h, d_pose2d, "d_pose2d")) ||
      (d_pivot && !device_readable(h, d_pivot, "d_pivot")) || !device_readable(h, d_field, "d_field") ||
      !device_readable(h, d_scores, "d_scores") || !device_readable(h, d_best, "d_best") ||
      (d_status && !device_readable(h, d_status, "d_status")))
    return RPLGPU_ERR_INVALID_ARG;
  if (d_t0 && !d_motion) {
    h->err = "rplgpu_match_scans_dev: scan time offsets are set (rplgpu_set_scan_time_offsets_dev) but d_motion is NULL";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (p->ror_enable && !(p->ror_radius > 0.0f && p->ror_radius <= 1.0e6f)) {
    h->err = "ror_radius must be in (0, 1e6] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  group = std::min(group, B);  // as E8: "all sensors in one match" may be asked for with any group >= B
  if ((uint64_t)group * n_stride > (1ull << 24)) {  // 127 x points stays below 2^32: no score wraps
    h->err = "rplgpu_match_scans_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint32_t G = (B + group - 1u) / group;
  const rpl::MatchK k{m->origin_x, m->origin_y, m->resolution, m->width, m->height,
                      m->shift_x, m->shift_y, m->rot_steps};
  rpl::MatchRot rot;  // at most 129 pairs, handed to the kernel by value: no copy on the stream
  std::memset(&rot, 0, sizeof(rot));
  if (rplgpu_scan_match_rotations(m, rot.cs) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  rpl::KParams kp = to_kparams(*p);
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  rpl::Tables T = tables_of(h);
  T.scan_t0 = d_t0;
  const uint32_t *mask = nullptr;
  if (p->ror_enable) {  // E1 AND E5 keep bits, the mask E9 and E11 apply
    RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, T, h->d_rormask,
                                    kMaskStride));
    mask = h->d_rormask;
  }
  if (d_status) RPL_HIP(h, hipMemsetAsync(d_status, 0, (size_t)G * 4u, h->stream));
  RPL_HIP(h, rpl::launch_match_prepare(h->stream, d_scores, score_stride, G, k, d_best));
  RPL_HIP(h, rpl::launch_match_score(h->stream, d_nodes, n_stride, d_n_per_scan, B, group, kp, T, mask, kMaskStride,
                                     d_motion, d_pose2d, d_pivot, k, rot, d_field, field_stride, field_per_group,
                                     d_scores, score_stride, d_best, d_status));
  RPL_HIP(h, rpl::launch_match_best(h->stream, d_scores, score_stride, G, k, d_best));
  return RPLGPU_OK;
}

int32_t rplgpu_match_scans_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const float *d_pivot,
                               const rplgpu_scan_match_t *m, const int8_t *d_field, uint64_t field_stride,
                               uint32_t field_per_group, uint32_t *d_scores, uint64_t score_stride,
                               uint32_t *d_best, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return match_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, d_pivot, m,
                    d_field, field_stride, field_per_group, d_scores, score_stride, d_best, d_status);
}

int32_t rplgpu_match_scans(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                           const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                           const float *motion, const float *pose2d, const float *t0, const float *pivot,
                           const rplgpu_scan_match_t *m, const int8_t *field, uint32_t *scores_out,
                           uint32_t best[8], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !m || !field || !best || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_match_scans: invalid rplgpu_scan_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)m->width * m->height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t nb = (size_t)n_scans * n_stride * 8u;
  const size_t volume = rplgpu_scan_match_volume(m);
  // one allocation per call (a convenience door, not the hot path): field | scores | nodes | lengths | motion |
  // pose | t0 | pivot | best + status, every part 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t o_sc = up16(stride), o_nodes = o_sc + up16(4u * volume), o_len = o_nodes + up16(nb),
               o_mo = o_len + up16(4u * n_scans), o_po = o_mo + up16(motion ? 16u * n_scans : 0),
               o_t0 = o_po + up16(pose2d ? 24u * n_scans : 0), o_pv = o_t0 + up16(t0 ? 4u * n_scans : 0),
               o_small = o_pv + up16(pivot ? 8u : 0), total = o_small + 48u;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_match_scans: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d, field, cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_nodes, nodes, nb, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_len, n_per_scan, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (motion) RPL_HIP(h, hipMemcpyAsync(d + o_mo, motion, 16u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (pose2d) RPL_HIP(h, hipMemcpyAsync(d + o_po, pose2d, 24u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (t0) RPL_HIP(h, hipMemcpyAsync(d + o_t0, t0, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (pivot) RPL_HIP(h, hipMemcpyAsync(d + o_pv, pivot, 8u, hipMemcpyHostToDevice, h->stream));
    uint32_t *d_small = reinterpret_cast<uint32_t *>(d + o_small);
    const int32_t rc = match_impl(
        h, reinterpret_cast<const rplgpu_node_t *>(d + o_nodes), n_stride,
        reinterpret_cast<const uint32_t *>(d + o_len), n_scans, n_scans, p,
        motion ? reinterpret_cast<const float *>(d + o_mo) : nullptr,
        pose2d ? reinterpret_cast<const float *>(d + o_po) : nullptr,
        t0 ? reinterpret_cast<const float *>(d + o_t0) : nullptr,
        pivot ? reinterpret_cast<const float *>(d + o_pv) : nullptr, m, reinterpret_cast<const int8_t *>(d), stride, 0,
        reinterpret_cast<uint32_t *>(d + o_sc), volume, d_small, d_small + 8);
    if (rc) return rc;
    if (scores_out)
      RPL_HIP(h, hipMemcpyAsync(scores_out, d + o_sc, 4u * volume, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 36, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  std::memcpy(best, small, 32);
  if (status) *status = small[8];
  return RPLGPU_OK;
}

// ---- E14: time steps accumulated into a hit / miss map at matched poses (include/rplgpu_msg.h) ----------------

void rplgpu_default_map_rule(rplgpu_map_rule_t *rule) {
  if (!rule) return;
  rule->min_observations = 2;
  rule->occupied_percent = 10;
  rule->mode = 0;
}

int32_t rplgpu_map_rule_check(const rplgpu_map_rule_t *rule) {
  if (!rule || rule->min_observations == 0 || rule->occupied_percent > 100u || rule->mode > 1u)
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t map_update_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const float *d_t0,
                               const rplgpu_occ_grid_t *grid, uint32_t *d_counts, uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !grid || !d_counts || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_map_update_dev: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(d_counts) & 7u) || (reinterpret_cast<uintptr_t>(d_status) & 3u)) {
    h->err = "rplgpu_map_update_dev: d_counts must be 8-byte aligned, d_status 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if ((d_motion && !device_readable(h, d_motion, "d_motion")) ||
      (d_pose2d && !device_readable(h, d_pose2d, "d_pose2d")) || !device_readable(h, d_counts, "d_counts") ||
      (d_status && !device_readable(h, d_status, "d_status")))
    return RPLGPU_ERR_INVALID_ARG;
  if (d_t0 && !d_motion) {
    h->err = "rplgpu_map_update_dev: scan time offsets are set (rplgpu_set_scan_time_offsets_dev) but d_motion is NULL";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (p->ror_enable && !(p->ror_radius > 0.0f && p->ror_radius <= 1.0e6f)) {
    h->err = "ror_radius must be in (0, 1e6] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  group = std::min(group, B);  // as E8: "all sensors in one group" may be asked for with any group >= B
  if ((uint64_t)group * std::min(n_stride, rpl::kMaxN) > (1ull << 24)) {
    h->err = "rplgpu_map_update_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_CAPACITY;
  }
  const uint32_t G = (B + group - 1u) / group;
  RPL_HIP(h, hipSetDevice(h->device));
  rpl::KParams kp = to_kparams(*p);
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  rpl::Tables T = tables_of(h);
  T.scan_t0 = d_t0;
  const rpl::OccK k = occ_kernel_args(*grid);
  const uint32_t *mask = nullptr;
  if (p->ror_enable) {  // E1 AND E5 keep bits, the mask E9, E11 and E13 apply
    RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, T, h->d_rormask,
                                    kMaskStride));
    mask = h->d_rormask;
  }
  if (d_status) RPL_HIP(h, hipMemsetAsync(d_status, 0, (size_t)G * 4u, h->stream));
  RPL_HIP(h, rpl::launch_map_walk(h->stream, d_nodes, n_stride, d_n_per_scan, B, group, kp, T, mask, kMaskStride,
                                  d_motion, d_pose2d, k, d_counts, d_status));
  return RPLGPU_OK;
}

int32_t rplgpu_map_update_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                              const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                              const float *d_motion, const float *d_pose2d, const rplgpu_occ_grid_t *grid,
                              uint32_t *d_counts, uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return map_update_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, grid,
                         d_counts, d_status);
}

int32_t rplgpu_map_grid_dev(rplgpu_handle_t h, const uint32_t *d_counts, uint32_t width, uint32_t height,
                            const rplgpu_map_rule_t *rule, const int8_t *d_prev, int8_t *d_grid,
                            uint64_t grid_stride, uint32_t *d_cells) {
  if (!h || !d_counts || !rule || !d_grid) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_map_rule_check(rule) != RPLGPU_OK) {
    h->err = "rplgpu_map_grid_dev: invalid rplgpu_map_rule_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_map_grid_dev: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (grid_stride < (uint64_t)width * height || (grid_stride & 3u) || (reinterpret_cast<uintptr_t>(d_grid) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_counts) & 7u) || (reinterpret_cast<uintptr_t>(d_cells) & 3u)) {
    h->err = "rplgpu_map_grid_dev: grid_stride must be >= width * height and a multiple of 4, d_grid / d_cells 4-byte and d_counts 8-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_prev == d_grid) {
    h->err = "rplgpu_map_grid_dev: d_prev must not be d_grid";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, d_counts, "d_counts") || (d_prev && !device_readable(h, d_prev, "d_prev")) ||
      !device_readable(h, d_grid, "d_grid") || (d_cells && !device_readable(h, d_cells, "d_cells")))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  if (d_cells) RPL_HIP(h, hipMemsetAsync(d_cells, 0, 16u, h->stream));
  RPL_HIP(h, rpl::launch_map_grid(h->stream, d_counts, width, height, rule->min_observations,
                                  rule->occupied_percent, rule->mode, d_prev, d_grid, d_cells));
  return RPLGPU_OK;
}

int32_t rplgpu_apply_match_dev(rplgpu_handle_t h, const uint32_t *d_best, const rplgpu_scan_match_t *m,
                               const float *d_pivot, const float *d_pose2d_in, uint32_t B, uint32_t group,
                               uint32_t flags, float *d_pose2d_out, float *d_pivot_out) {
  if (!h || !d_best || !m || !d_pose2d_out || group == 0 || flags > 1u) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_scan_match_check(m) != RPLGPU_OK) {
    h->err = "rplgpu_apply_match_dev: invalid rplgpu_scan_match_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(d_best) & 3u) || (reinterpret_cast<uintptr_t>(d_pivot) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_pose2d_in) & 3u) || (reinterpret_cast<uintptr_t>(d_pose2d_out) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_pivot_out) & 3u)) {
    h->err = "rplgpu_apply_match_dev: every pointer must be 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_pivot_out && d_pivot_out == d_pivot) {
    h->err = "rplgpu_apply_match_dev: d_pivot_out must not be d_pivot (every scan of a group reads the pivot)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B > h->max_b) {
    h->err = "batch larger than max_batch given to rplgpu_create";
    return RPLGPU_ERR_CAPACITY;
  }
  if (B == 0) return RPLGPU_OK;
  if (!device_readable(h, d_best, "d_best") || (d_pivot && !device_readable(h, d_pivot, "d_pivot")) ||
      (d_pose2d_in && !device_readable(h, d_pose2d_in, "d_pose2d_in")) ||
      !device_readable(h, d_pose2d_out, "d_pose2d_out") ||
      (d_pivot_out && !device_readable(h, d_pivot_out, "d_pivot_out")))
    return RPLGPU_ERR_INVALID_ARG;
  group = std::min(group, B);
  const rpl::MatchK k{m->origin_x, m->origin_y, m->resolution, m->width, m->height,
                      m->shift_x, m->shift_y, m->rot_steps};
  rpl::MatchRot rot;  // by value, as k_match_score takes it
  std::memset(&rot, 0, sizeof(rot));
  if (rplgpu_scan_match_rotations(m, rot.cs) != RPLGPU_OK) return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_apply_match(h->stream, d_best, k, rot, d_pivot, d_pose2d_in, B, group, flags, d_pose2d_out,
                                     d_pivot_out));
  return RPLGPU_OK;
}

int32_t rplgpu_map_update(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                          const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                          const float *motion, const float *pose2d, const float *t0, const rplgpu_occ_grid_t *grid,
                          uint32_t *counts, uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !grid || !counts || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_occ_grid_check(grid) != RPLGPU_OK) {
    h->err = "rplgpu_map_update: invalid rplgpu_occ_grid_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)grid->width * grid->height;
  const size_t nb = (size_t)n_scans * n_stride * 8u;
  // one allocation per call (a convenience door, not the hot path): counts | nodes | lengths | motion | pose |
  // t0 | status, every part 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t o_nodes = up16(8u * cells_n), o_len = o_nodes + up16(nb), o_mo = o_len + up16(4u * n_scans),
               o_po = o_mo + up16(motion ? 16u * n_scans : 0), o_t0 = o_po + up16(pose2d ? 24u * n_scans : 0),
               o_small = o_t0 + up16(t0 ? 4u * n_scans : 0), total = o_small + 16u;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_map_update: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small = 0;
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d, counts, 8u * cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_nodes, nodes, nb, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_len, n_per_scan, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (motion) RPL_HIP(h, hipMemcpyAsync(d + o_mo, motion, 16u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (pose2d) RPL_HIP(h, hipMemcpyAsync(d + o_po, pose2d, 24u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (t0) RPL_HIP(h, hipMemcpyAsync(d + o_t0, t0, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    uint32_t *d_small = reinterpret_cast<uint32_t *>(d + o_small);
    const int32_t rc = map_update_impl(
        h, reinterpret_cast<const rplgpu_node_t *>(d + o_nodes), n_stride,
        reinterpret_cast<const uint32_t *>(d + o_len), n_scans, n_scans, p,
        motion ? reinterpret_cast<const float *>(d + o_mo) : nullptr,
        pose2d ? reinterpret_cast<const float *>(d + o_po) : nullptr,
        t0 ? reinterpret_cast<const float *>(d + o_t0) : nullptr, grid, reinterpret_cast<uint32_t *>(d), d_small);
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(counts, d, 8u * cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(&small, d_small, 4, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  if (status) *status = small;
  return RPLGPU_OK;
}

int32_t rplgpu_map_grid(rplgpu_handle_t h, const uint32_t *counts, uint32_t width, uint32_t height,
                        const rplgpu_map_rule_t *rule, const int8_t *prev, int8_t *grid_out, uint32_t cells[4]) {
  if (!h || !counts || !rule || !grid_out) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_map_rule_check(rule) != RPLGPU_OK) {
    h->err = "rplgpu_map_grid: invalid rplgpu_map_rule_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) {
    h->err = "rplgpu_map_grid: width and height must be 1 .. RPLGPU_MAX_OCC_DIM";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)width * height, stride = (cells_n + 3u) & ~(size_t)3u;
  // one allocation per call: counts | grid | prev | cells, every part 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t o_grid = up16(8u * cells_n), o_prev = o_grid + up16(stride), o_small = o_prev + up16(prev ? stride : 0),
               total = o_small + 16u;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_map_grid: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[4] = {0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d, counts, 8u * cells_n, hipMemcpyHostToDevice, h->stream));
    if (prev) RPL_HIP(h, hipMemcpyAsync(d + o_prev, prev, cells_n, hipMemcpyHostToDevice, h->stream));
    const int32_t rc = rplgpu_map_grid_dev(h, reinterpret_cast<const uint32_t *>(d), width, height, rule,
                                           prev ? reinterpret_cast<const int8_t *>(d + o_prev) : nullptr,
                                           reinterpret_cast<int8_t *>(d + o_grid), stride,
                                           reinterpret_cast<uint32_t *>(d + o_small));
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(grid_out, d + o_grid, cells_n, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d + o_small, 16, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  if (cells) std::memcpy(cells, small, 16);
  return RPLGPU_OK;
}

// ---- E15: a list of arbitrary poses weighed against a likelihood field (include/rplgpu_msg.h) ------------------

void rplgpu_default_pose_score(rplgpu_pose_score_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->resolution = 0.05f;
  s->width = 1024;
  s->height = 1024;
}

int32_t rplgpu_pose_score_check(const rplgpu_pose_score_t *s) {
  if (!s) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(s->origin_x) || !std::isfinite(s->origin_y) || !std::isfinite(s->resolution))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(s->resolution > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (s->width == 0 || s->width > RPLGPU_MAX_OCC_DIM || s->height == 0 || s->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

int32_t rplgpu_pose_list(const double *xyt, uint32_t n, float *poses_out) {
  if (n > RPLGPU_MAX_POSES || (n && (!xyt || !poses_out))) return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t q = 0; q < n; ++q) {
    const double th = xyt[3u * q + 2u];
    poses_out[4u * q] = th == 0.0 ? 1.0f : (float)std::cos(th);
    poses_out[4u * q + 1u] = th == 0.0 ? 0.0f : (float)std::sin(th);  // (+0 for theta = -0 too)
    poses_out[4u * q + 2u] = (float)xyt[3u * q];
    poses_out[4u * q + 3u] = (float)xyt[3u * q + 1u];
  }
  return RPLGPU_OK;
}

// d_t0: the per-scan time offsets of E6 for this call (the handle's, or the host door's own), or NULL
static int32_t pose_impl(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                         const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                         const float *d_motion, const float *d_pose2d, const float *d_t0,
                         const rplgpu_pose_score_t *s, const float *d_poses, uint32_t P, uint64_t pose_stride,
                         uint32_t poses_per_group, const int8_t *d_field, uint64_t field_stride,
                         uint32_t field_per_group, uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_result,
                         uint32_t *d_status) {
  int32_t rc = check_batch(h, d_nodes, n_stride, d_n_per_scan, B);
  if (rc) return rc;
  if (!p || !s || !d_poses || !d_field || !d_weights || !d_result || group == 0) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_score_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_score_poses_dev: invalid rplgpu_pose_score_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_score_poses_dev: P must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (pose_stride < 4ull * P || (pose_stride & 3u) || (reinterpret_cast<uintptr_t>(d_poses) & 15u)) {
    h->err = "rplgpu_score_poses_dev: pose_stride must be >= 4 P floats and a multiple of 4, d_poses 16-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (field_stride < (uint64_t)s->width * s->height || (field_stride & 3u) ||
      (reinterpret_cast<uintptr_t>(d_field) & 3u)) {
    h->err = "rplgpu_score_poses_dev: field_stride must be >= width * height and a multiple of 4, d_field 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (weight_stride < P || (reinterpret_cast<uintptr_t>(d_weights) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_result) & 3u) || (reinterpret_cast<uintptr_t>(d_status) & 3u)) {
    h->err = "rplgpu_score_poses_dev: weight_stride must be >= P, d_weights / d_result / d_status 4-byte aligned";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (B == 0) return RPLGPU_OK;
  if ((d_motion && !device_readable(h, d_motion, "d_motion")) ||
      (d_pose2d && !device_readable(h, d_pose2d, "d_pose2d")) || !device_readable(h, d_poses, "d_poses") ||
      !device_readable(h, d_field, "d_field") || !device_readable(h, d_weights, "d_weights") ||
      !device_readable(h, d_result, "d_result") || (d_status && !device_readable(h, d_status, "d_status")))
    return RPLGPU_ERR_INVALID_ARG;
  if (d_t0 && !d_motion) {
    h->err = "rplgpu_score_poses_dev: scan time offsets are set (rplgpu_set_scan_time_offsets_dev) but d_motion is NULL";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (p->ror_enable && !(p->ror_radius > 0.0f && p->ror_radius <= 1.0e6f)) {
    h->err = "ror_radius must be in (0, 1e6] m";
    return RPLGPU_ERR_INVALID_ARG;
  }
  group = std::min(group, B);  // as E8: "all sensors in one time step" may be asked for with any group >= B
  if ((uint64_t)group * n_stride > (1ull << 24)) {  // 127 x points stays below 2^32: no weight wraps
    h->err = "rplgpu_score_poses_dev: group x n_stride above 2^24 samples";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint32_t G = (B + group - 1u) / group;
  if ((uint64_t)G * ((P + 255u) / 256u) > 0x7FFFFFFFull) {  // (launch_pose_prepare's grid; before anything is queued)
    h->err = "rplgpu_score_poses_dev: groups x P too large for one call";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const rpl::PoseK k{s->origin_x, s->origin_y, s->resolution, s->width, s->height};
  RPL_HIP(h, hipSetDevice(h->device));
  rpl::KParams kp = to_kparams(*p);
  kp.fast_d4000 = use_fast_d4000(h) ? 1 : 0;
  rpl::Tables T = tables_of(h);
  T.scan_t0 = d_t0;
  const uint32_t *mask = nullptr;
  if (p->ror_enable) {  // E1 AND E5 keep bits, the mask E9, E11 and E13 apply
    RPL_HIP(h, rpl::launch_ror_mask(h->stream, d_nodes, n_stride, d_n_per_scan, B, kp, T, h->d_rormask,
                                    kMaskStride));
    mask = h->d_rormask;
  }
  if (d_status) RPL_HIP(h, hipMemsetAsync(d_status, 0, (size_t)G * 4u, h->stream));
  RPL_HIP(h, rpl::launch_pose_prepare(h->stream, d_weights, weight_stride, G, P, d_result));
  RPL_HIP(h, rpl::launch_pose_score(h->stream, d_nodes, n_stride, d_n_per_scan, B, group, kp, T, mask, kMaskStride,
                                    d_motion, d_pose2d, k, d_poses, P, pose_stride, poses_per_group, d_field,
                                    field_stride, field_per_group, d_weights, weight_stride, d_result, d_status));
  RPL_HIP(h, rpl::launch_pose_best(h->stream, d_weights, weight_stride, G, P, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_score_poses_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const rplgpu_pose_score_t *s,
                               const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                               const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group,
                               uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_result,
                               uint32_t *d_status) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  return pose_impl(h, d_nodes, n_stride, d_n_per_scan, B, group, p, d_motion, d_pose2d, h->scan_t0, s, d_poses, P,
                   pose_stride, poses_per_group, d_field, field_stride, field_per_group, d_weights, weight_stride,
                   d_result, d_status);
}

int32_t rplgpu_score_poses(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                           const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                           const float *motion, const float *pose2d, const float *t0,
                           const rplgpu_pose_score_t *s, const float *poses, uint32_t P, const int8_t *field,
                           uint32_t *weights_out, uint32_t result[8], uint32_t *status) {
  if (!h || !nodes || !n_per_scan || !p || !s || !poses || !field || !result || n_scans == 0 || n_stride == 0)
    return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_score_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_score_poses: invalid rplgpu_pose_score_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_score_poses: P must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (n_scans > h->max_b || n_stride > h->max_n) return RPLGPU_ERR_CAPACITY;
  RPL_HIP(h, hipSetDevice(h->device));
  const size_t cells_n = (size_t)s->width * s->height, stride = (cells_n + 3u) & ~(size_t)3u;
  const size_t nb = (size_t)n_scans * n_stride * 8u;
  // one allocation per call (a convenience door, not the hot path): field | poses | weights | nodes | lengths |
  // motion | pose | t0 | result + status, every part 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t o_ps = up16(stride), o_wt = o_ps + up16(16u * (size_t)P), o_nodes = o_wt + up16(4u * (size_t)P),
               o_len = o_nodes + up16(nb), o_mo = o_len + up16(4u * n_scans),
               o_po = o_mo + up16(motion ? 16u * n_scans : 0), o_t0 = o_po + up16(pose2d ? 24u * n_scans : 0),
               o_small = o_t0 + up16(t0 ? 4u * n_scans : 0), total = o_small + 48u;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_score_poses: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d, field, cells_n, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_ps, poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_nodes, nodes, nb, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_len, n_per_scan, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (motion) RPL_HIP(h, hipMemcpyAsync(d + o_mo, motion, 16u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (pose2d) RPL_HIP(h, hipMemcpyAsync(d + o_po, pose2d, 24u * n_scans, hipMemcpyHostToDevice, h->stream));
    if (t0) RPL_HIP(h, hipMemcpyAsync(d + o_t0, t0, 4u * n_scans, hipMemcpyHostToDevice, h->stream));
    uint32_t *d_small = reinterpret_cast<uint32_t *>(d + o_small);
    const int32_t rc = pose_impl(
        h, reinterpret_cast<const rplgpu_node_t *>(d + o_nodes), n_stride,
        reinterpret_cast<const uint32_t *>(d + o_len), n_scans, n_scans, p,
        motion ? reinterpret_cast<const float *>(d + o_mo) : nullptr,
        pose2d ? reinterpret_cast<const float *>(d + o_po) : nullptr,
        t0 ? reinterpret_cast<const float *>(d + o_t0) : nullptr, s, reinterpret_cast<const float *>(d + o_ps), P,
        4ull * P, 0, reinterpret_cast<const int8_t *>(d), stride, 0, reinterpret_cast<uint32_t *>(d + o_wt), P,
        d_small, d_small + 8);
    if (rc) return rc;
    if (weights_out)
      RPL_HIP(h, hipMemcpyAsync(weights_out, d + o_wt, 4u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small, 36, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  std::memcpy(result, small, 32);
  if (status) *status = small[8];
  return RPLGPU_OK;
}

// ---- E16: a weighted pose list resampled and moved (include/rplgpu_msg.h) ---------------------------------------

uint64_t rplgpu_resample_scratch_words(uint32_t G, uint32_t P) { return rpl::resample_scratch_words(G, P); }

// the byte ranges [a, a + na) and [b, b + nb) share a byte
static bool ranges_overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

// E16's move: the delta composed on the right, float32, each product rounded, then the difference or sum (this
// unit is built with -ffp-contract=off); a NaN that the move makes is stored as 0x7FC00000
static void resample_move(const float *pose, const float *d, float *out) {
  const float c = pose[0], s = pose[1], x = pose[2], y = pose[3];
  const float dc = d[0], ds = d[1], dx = d[2], dy = d[3];
  const float p0 = c * dc, p1 = s * ds, p2 = s * dc, p3 = c * ds, p4 = c * dx, p5 = s * dy, p6 = s * dx, p7 = c * dy;
  float v[4] = {p0 - p1, p2 + p3, (p4 - p5) + x, (p6 + p7) + y};
  const uint32_t qnan = 0x7FC00000u;
  for (int k = 0; k < 4; ++k) {
    if (v[k] != v[k]) std::memcpy(&v[k], &qnan, 4);
  }
  std::memcpy(out, v, 16);
}

int32_t rplgpu_resample_host(const uint32_t *weights, uint32_t P, uint32_t M, uint32_t u, const float *poses,
                             const float *delta, uint32_t n_delta, float *poses_out, uint32_t *ancestors_out,
                             uint32_t result[8]) {
  if (!weights || !poses || !poses_out || !result || P == 0 || P > RPLGPU_MAX_POSES || M == 0 ||
      M > RPLGPU_MAX_POSES || (delta && n_delta != 1u && n_delta != M) ||
      ranges_overlap(poses, 16ull * P, poses_out, 16ull * M))
    return RPLGPU_ERR_INVALID_ARG;
  uint64_t S = 0, sq = 0;
  uint32_t carry = 0, nz = 0;
  for (uint32_t i = 0; i < P; ++i) {
    const uint64_t w = weights[i], w2 = w * w;
    S += w;
    sq += w2;
    carry += sq < w2 ? 1u : 0u;
    nz += w != 0 ? 1u : 0u;
  }
  const uint64_t q = S / M, rho = S % M;
  const uint64_t r = (uint64_t)u * (S >> 32) + (((uint64_t)u * (S & 0xffffffffull)) >> 32);
  uint32_t i = 0, distinct = 0, last = 0xFFFFFFFFu;
  uint64_t C = weights[0];  // C[i], inclusive
  for (uint32_t j = 0; j < M; ++j) {
    uint32_t a;
    if (S == 0) {
      a = j % P;
    } else {
      const uint64_t t = (uint64_t)j * q + ((uint64_t)j * rho + r) / M;  // < S: the walk ends inside the list
      while (C <= t) C += weights[++i];
      a = i;
    }
    if (a != last) ++distinct;  // (a is non-decreasing)
    last = a;
    if (delta)
      resample_move(poses + 4u * (size_t)a, delta + (n_delta == 1u ? 0u : 4u * (size_t)j), poses_out + 4u * (size_t)j);
    else
      std::memcpy(poses_out + 4u * (size_t)j, poses + 4u * (size_t)a, 16);
    if (ancestors_out) ancestors_out[j] = a;
  }
  result[0] = (uint32_t)S;
  result[1] = (uint32_t)(S >> 32);
  result[2] = (uint32_t)sq;
  result[3] = (uint32_t)(sq >> 32);
  result[4] = carry;
  result[5] = nz;
  result[6] = S == 0 ? std::min(M, P) : distinct;
  result[7] = S == 0 ? 1u : 0u;
  return RPLGPU_OK;
}

int32_t rplgpu_resample_poses_dev(rplgpu_handle_t h, const uint32_t *d_weights, uint64_t weight_stride,
                                  const float *d_poses, uint64_t pose_stride, uint32_t poses_per_group, uint32_t G,
                                  uint32_t P, uint32_t M, const uint32_t *d_u, const float *d_delta,
                                  uint32_t n_delta, uint64_t delta_stride, uint32_t delta_per_group,
                                  float *d_poses_out, uint64_t out_stride, uint32_t *d_ancestors,
                                  uint64_t anc_stride, uint32_t *d_result, uint32_t *d_scratch) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  auto off = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
  if (G == 0 || G > 65535u) {  // (the tiles of a group by the groups: a grid's second dimension)
    h->err = "rplgpu_resample_poses_dev: G must be in 1 .. 65535";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES || M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_resample_poses_dev: P and M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_weights || !d_poses || !d_poses_out || !d_result || !d_scratch || off(d_weights, 3) || off(d_poses, 15) ||
      off(d_poses_out, 15) || off(d_result, 3) || off(d_scratch, 7) || off(d_u, 3) || off(d_delta, 15) ||
      off(d_ancestors, 3)) {
    h->err = "rplgpu_resample_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for pose "
             "lists and deltas, 8 for d_scratch, 4 otherwise)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (weight_stride < P || pose_stride < 4ull * P || (pose_stride & 3u) || out_stride < 4ull * M ||
      (out_stride & 3u) || (d_ancestors && anc_stride < M)) {
    h->err = "rplgpu_resample_poses_dev: weight_stride >= P, pose_stride >= 4 P, out_stride >= 4 M (both multiples "
             "of 4) and anc_stride >= M are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_delta && ((n_delta != 1u && n_delta != M) || delta_stride < 4ull * n_delta || (delta_stride & 3u))) {
    h->err = "rplgpu_resample_poses_dev: n_delta must be 1 or M, delta_stride >= 4 n_delta and a multiple of 4";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t in_bytes = 4ull * ((poses_per_group ? (uint64_t)(G - 1u) * pose_stride : 0ull) + 4ull * P);
  const uint64_t out_bytes = 4ull * ((uint64_t)(G - 1u) * out_stride + 4ull * M);
  if (ranges_overlap(d_poses, in_bytes, d_poses_out, out_bytes)) {
    h->err = "rplgpu_resample_poses_dev: d_poses_out overlaps d_poses";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, d_weights, "d_weights") || !device_readable(h, d_poses, "d_poses") ||
      !device_readable(h, d_poses_out, "d_poses_out") || !device_readable(h, d_result, "d_result") ||
      !device_readable(h, d_scratch, "d_scratch") || (d_u && !device_readable(h, d_u, "d_u")) ||
      (d_delta && !device_readable(h, d_delta, "d_delta")) ||
      (d_ancestors && !device_readable(h, d_ancestors, "d_ancestors")))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_resample(h->stream, d_weights, weight_stride, d_poses, pose_stride, poses_per_group, G, P,
                                  M, d_u, d_delta, d_delta ? n_delta : 1u, delta_stride, delta_per_group,
                                  d_poses_out, out_stride, d_ancestors, anc_stride, d_result, d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_resample_poses(rplgpu_handle_t h, const uint32_t *weights, uint32_t P, uint32_t M, uint32_t u,
                              const float *poses, const float *delta, uint32_t n_delta, float *poses_out,
                              uint32_t *ancestors_out, uint32_t result[8]) {
  if (!h || !weights || !poses || !poses_out || !result) return RPLGPU_ERR_INVALID_ARG;
  if (P == 0 || P > RPLGPU_MAX_POSES || M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_resample_poses: P and M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (delta && n_delta != 1u && n_delta != M) {
    h->err = "rplgpu_resample_poses: n_delta must be 1 or M";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (ranges_overlap(poses, 16ull * P, poses_out, 16ull * M)) {
    h->err = "rplgpu_resample_poses: poses_out overlaps poses";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // one allocation per call (a convenience door, not the hot path): poses | out | deltas | weights | ancestors |
  // scratch | u + result, every part 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t nd = delta ? n_delta : 0u;
  const size_t o_out = up16(16u * (size_t)P), o_dl = o_out + up16(16u * (size_t)M), o_wt = o_dl + up16(16u * nd),
               o_anc = o_wt + up16(4u * (size_t)P), o_scr = o_anc + up16(4u * (size_t)M),
               o_small = o_scr + up16(4u * (size_t)rplgpu_resample_scratch_words(1, P)), total = o_small + 48u;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_resample_poses: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    uint32_t *d_small = reinterpret_cast<uint32_t *>(d + o_small);  // u, then the result at + 4 words
    RPL_HIP(h, hipMemcpyAsync(d, poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_wt, weights, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d_small, &u, 4, hipMemcpyHostToDevice, h->stream));
    if (delta) RPL_HIP(h, hipMemcpyAsync(d + o_dl, delta, 16u * nd, hipMemcpyHostToDevice, h->stream));
    const int32_t rc = rplgpu_resample_poses_dev(
        h, reinterpret_cast<const uint32_t *>(d + o_wt), P, reinterpret_cast<const float *>(d), 4ull * P, 0, 1, P, M,
        d_small, delta ? reinterpret_cast<const float *>(d + o_dl) : nullptr, n_delta, 4ull * nd, 0,
        reinterpret_cast<float *>(d + o_out), 4ull * M, reinterpret_cast<uint32_t *>(d + o_anc), M, d_small + 4,
        reinterpret_cast<uint32_t *>(d + o_scr));
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(poses_out, d + o_out, 16u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    if (ancestors_out)
      RPL_HIP(h, hipMemcpyAsync(ancestors_out, d + o_anc, 4u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d_small + 4, 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

// ---- E17: a weighted pose list reduced to a pose estimate (include/rplgpu_msg.h) -------------------------------------

void rplgpu_default_pose_estimate(rplgpu_pose_estimate_t *s) {
  if (!s) return;
  s->xy_scale = 1024.0f;
  s->gate_r2 = 512ull * 512ull;
  s->gate_dot = 15ll << 36;
}

int32_t rplgpu_pose_estimate_check(const rplgpu_pose_estimate_t *s) {
  if (!s) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(s->xy_scale) || !(s->xy_scale > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_estimate_scratch_words(uint32_t G, uint32_t P) { return rpl::estimate_scratch_words(G, P); }

// E17's quantisation of one pose entry: one float32 product (this unit is built with -ffp-contract=off), the range
// test, one round-to-nearest-even (the default rounding mode)
static bool estimate_quantise(const float *pose, float xy_scale, int32_t q[4]) {
  const float t[4] = {pose[2] * xy_scale, pose[3] * xy_scale, pose[0] * 1048576.0f, pose[1] * 1048576.0f};
  for (int k = 0; k < 4; ++k) {
    if (!(std::fabs(t[k]) < 8388608.0f)) return false;
  }
  for (int k = 0; k < 4; ++k) q[k] = (int32_t)std::rint(t[k]);  // X, Y, C, S
  return true;
}

int32_t rplgpu_estimate_host(const float *poses, uint32_t P, const uint32_t *weights,
                             const rplgpu_pose_estimate_t *s, uint32_t center, uint32_t result[72]) {
  if (!poses || !result || rplgpu_pose_estimate_check(s) != RPLGPU_OK || P == 0 || P > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t qc = std::min(center, P - 1u);
  int32_t c[4] = {0, 0, 0, 0};
  const bool c_in = estimate_quantise(poses + 4u * (size_t)qc, s->xy_scale, c);
  __int128 sum[2][8] = {};
  uint32_t count[2][2] = {{0, 0}, {0, 0}};
  for (uint32_t i = 0; i < P; ++i) {
    int32_t q[4];
    if (!estimate_quantise(poses + 4u * (size_t)i, s->xy_scale, q)) continue;
    const int64_t X = q[0], Y = q[1], C = q[2], S = q[3];
    const int64_t dX = X - c[0], dY = Y - c[1];
    const bool gate = c_in && (uint64_t)(dX * dX + dY * dY) <= s->gate_r2 && C * c[2] + S * c[3] >= s->gate_dot;
    const __int128 w = weights ? weights[i] : 1u;
    const __int128 term[8] = {w, w * X, w * Y, w * C, w * S, w * (X * X), w * (X * Y), w * (Y * Y)};
    for (int k = 0; k < (gate ? 2 : 1); ++k) {
      for (int m = 0; m < 8; ++m) sum[k][m] += term[m];
      count[k][0] += 1u;
      count[k][1] += w != 0 ? 1u : 0u;
    }
  }
  result[0] = (c_in ? 0u : 1u) | (count[0][0] != P ? 2u : 0u) | (sum[0][0] == 0 ? 4u : 0u) | (sum[1][0] == 0 ? 8u : 0u);
  result[1] = qc;
  result[2] = count[0][0];
  result[3] = count[0][1];
  result[4] = count[1][0];
  result[5] = count[1][1];
  result[6] = result[7] = 0u;
  for (int k = 0; k < 2; ++k) {
    for (int m = 0; m < 8; ++m) {
      const unsigned __int128 v = (unsigned __int128)sum[k][m];
      for (int j = 0; j < 4; ++j) result[8 + 32 * k + 4 * m + j] = (uint32_t)(v >> (32 * j));
    }
  }
  return RPLGPU_OK;
}

int32_t rplgpu_estimate_pose(const uint32_t result[72], float xy_scale, uint32_t set, double out[8]) {
  if (!result || !out || set > 1u || !std::isfinite(xy_scale) || !(xy_scale > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  double v[8];  // each sum rounded to fp64 once
  for (int m = 0; m < 8; ++m) {
    unsigned __int128 u = 0;
    for (int j = 3; j >= 0; --j) u = (u << 32) | result[8 + 32 * set + 4 * m + j];
    v[m] = (double)(__int128)u;
  }
  if (v[0] == 0.0) return RPLGPU_ERR_INVALID_ARG;  // (W < 2^52 is exact, so this is W == 0)
  const double scale = (double)xy_scale, scale2 = scale * scale;  // (24 x 24 bits: exact)
  const double mx = v[1] / v[0] / scale, my = v[2] / v[0] / scale;
  out[0] = mx;
  out[1] = my;
  out[2] = std::atan2(v[4], v[3]);
  out[3] = v[5] / v[0] / scale2 - mx * mx;
  out[4] = v[6] / v[0] / scale2 - mx * my;
  out[5] = v[7] / v[0] / scale2 - my * my;
  out[6] = std::hypot(v[3], v[4]) / (v[0] * 1048576.0);
  out[7] = v[0];
  return RPLGPU_OK;
}

int32_t rplgpu_estimate_poses_dev(rplgpu_handle_t h, const float *d_poses, uint64_t pose_stride,
                                  uint32_t poses_per_group, const uint32_t *d_weights, uint64_t weight_stride,
                                  uint32_t G, uint32_t P, const rplgpu_pose_estimate_t *s, const uint32_t *d_center,
                                  uint64_t center_stride, uint32_t *d_result, uint32_t *d_scratch) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  auto off = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
  if (rplgpu_pose_estimate_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_estimate_poses_dev: invalid rplgpu_pose_estimate_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0 || G > 65535u) {  // (the tiles of a group by the groups: a grid's second dimension)
    h->err = "rplgpu_estimate_poses_dev: G must be in 1 .. 65535";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_estimate_poses_dev: P must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_poses || !d_result || !d_scratch || off(d_poses, 15) || off(d_result, 3) || off(d_scratch, 7) ||
      off(d_weights, 3) || off(d_center, 3)) {
    h->err = "rplgpu_estimate_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for the "
             "pose list, 8 for d_scratch, 4 otherwise)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (pose_stride < 4ull * P || (pose_stride & 3u) || (d_weights && weight_stride < P)) {
    h->err = "rplgpu_estimate_poses_dev: pose_stride >= 4 P and a multiple of 4 and weight_stride >= P are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_center && center_stride == 0 && G > 1u) {
    h->err = "rplgpu_estimate_poses_dev: center_stride must not be 0 with more than one group";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, d_poses, "d_poses") || !device_readable(h, d_result, "d_result") ||
      !device_readable(h, d_scratch, "d_scratch") || (d_weights && !device_readable(h, d_weights, "d_weights")) ||
      (d_center && !device_readable(h, d_center, "d_center")))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_estimate(h->stream, d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P,
                                  s->xy_scale, s->gate_r2, s->gate_dot, d_center, center_stride, d_result,
                                  d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_estimate_poses(rplgpu_handle_t h, const float *poses, uint32_t P, const uint32_t *weights,
                              const rplgpu_pose_estimate_t *s, uint32_t center, uint32_t result[72]) {
  if (!h || !poses || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_estimate_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_estimate_poses: invalid rplgpu_pose_estimate_t (see include/rplgpu_msg.h)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_estimate_poses: P must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // one allocation per call (a convenience door, not the hot path): poses | weights | scratch | centre + result,
  // every part 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t o_wt = up16(16u * (size_t)P), o_scr = o_wt + up16(4u * (size_t)P),
               o_small = o_scr + up16(4u * (size_t)rplgpu_estimate_scratch_words(1, P)),
               total = o_small + 16u + 4u * RPLGPU_ESTIMATE_WORDS;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_estimate_poses: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t words[RPLGPU_ESTIMATE_WORDS];
  auto run = [&]() -> int32_t {
    uint32_t *d_small = reinterpret_cast<uint32_t *>(d + o_small);  // the centre word, then the result at + 4 words
    RPL_HIP(h, hipMemcpyAsync(d, poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (weights) RPL_HIP(h, hipMemcpyAsync(d + o_wt, weights, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d_small, &center, 4, hipMemcpyHostToDevice, h->stream));
    const int32_t rc = rplgpu_estimate_poses_dev(
        h, reinterpret_cast<const float *>(d), 4ull * P, 0, weights ? reinterpret_cast<const uint32_t *>(d + o_wt) : nullptr,
        P, 1, P, s, d_small, 0, d_small + 4, reinterpret_cast<uint32_t *>(d + o_scr));
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(words, d_small + 4, sizeof(words), hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  std::memcpy(result, words, sizeof(words));
  return RPLGPU_OK;
}

// ---- E18: a pose list's motion noise drawn on the device (include/rplgpu_msg.h) --------------------------------------

void rplgpu_default_motion_noise(rplgpu_motion_noise_t *s) {
  if (!s) return;
  s->seed = 0;
  s->step = 0;
  s->first = 0;
  s->reserved = 0;
}

static void philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
  }
  std::memcpy(out, c, 16);
}

int32_t rplgpu_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) return RPLGPU_ERR_INVALID_ARG;
  philox4x32(ctr, key, out);
  return RPLGPU_OK;
}

// E18's integer normal of one draw: the eight 16-bit halves of the block, minus their mean
static int32_t motion_draw(const rplgpu_motion_noise_t *s, uint32_t g, uint32_t j, uint32_t i) {
  const uint32_t ctr[4] = {s->first + j, (g << 2) | i, (uint32_t)s->step, (uint32_t)(s->step >> 32)};
  const uint32_t key[2] = {(uint32_t)s->seed, (uint32_t)(s->seed >> 32)};
  uint32_t w[4];
  philox4x32(ctr, key, w);
  int32_t z = -262140;
  for (int k = 0; k < 4; ++k) z += (int32_t)(w[k] & 0xFFFFu) + (int32_t)(w[k] >> 16);
  return z;
}

// E18's noise rotation by 2 atan(Z k) and the composition r o n: float32, every operation rounded once (this unit is
// built with -ffp-contract=off)
static void motion_noise(int32_t z, float k, float n[2]) {
  const float t = (float)z * k, q = t * t, den = 1.0f + q;
  n[0] = (1.0f - q) / den;
  n[1] = (t + t) / den;
}
static void motion_compose(const float r[2], const float n[2], float a[2]) {
  const float p0 = r[0] * n[0], p1 = r[1] * n[1], p2 = r[1] * n[0], p3 = r[0] * n[1];
  a[0] = p0 - p1;
  a[1] = p2 + p3;
}

int32_t rplgpu_sample_motion_host(const float odom[8], uint32_t group, uint32_t M, const rplgpu_motion_noise_t *s,
                                  float *delta_out, uint32_t result[8]) {
  if (!odom || !s || !delta_out || !result || group > 65534u || M == 0 || M > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const float r1[2] = {odom[0], odom[1]}, r2[2] = {odom[3], odom[4]};
  const float trans = odom[2], k1 = odom[5], kt = odom[6], k2 = odom[7];
  uint32_t nans = 0, zmax = 0;
  int64_t sum = 0;
  uint64_t squares = 0;
  for (uint32_t j = 0; j < M; ++j) {
    int32_t z[3];
    for (uint32_t i = 0; i < 3; ++i) {
      z[i] = motion_draw(s, group, j, i);
      zmax = std::max(zmax, (uint32_t)std::abs(z[i]));
      sum += z[i];
      squares += (uint64_t)((int64_t)z[i] * z[i]);
    }
    float n1[2], n2[2], a[2], b[2], d[2];
    motion_noise(z[0], k1, n1);
    motion_noise(z[2], k2, n2);
    motion_compose(r1, n1, a);
    motion_compose(r2, n2, b);
    motion_compose(a, b, d);
    const float noise = (float)z[1] * kt;
    const float tr = trans + noise;
    float v[4] = {d[0], d[1], a[0] * tr, a[1] * tr};
    const uint32_t qnan = 0x7FC00000u;
    bool any = false;
    for (int k = 0; k < 4; ++k) {
      if (v[k] != v[k]) {
        std::memcpy(&v[k], &qnan, 4);
        any = true;
      }
    }
    nans += any ? 1u : 0u;
    std::memcpy(delta_out + 4u * (size_t)j, v, 16);
  }
  result[0] = nans;
  result[1] = zmax;
  result[2] = (uint32_t)(uint64_t)sum;
  result[3] = (uint32_t)((uint64_t)sum >> 32);
  result[4] = (uint32_t)squares;
  result[5] = (uint32_t)(squares >> 32);
  result[6] = 0u;
  result[7] = nans ? 1u : 0u;
  return RPLGPU_OK;
}

int32_t rplgpu_motion_odometry(double dx, double dy, double dtheta, const double alpha[4], float out[8]) {
  if (!alpha || !out) return RPLGPU_ERR_INVALID_ARG;
  const double pi = 3.14159265358979323846;
  const double trans = std::sqrt(dx * dx + dy * dy);
  const double rot1 = trans >= 0.01 ? std::atan2(dy, dx) : 0.0;
  const double d = dtheta - rot1;
  const double rot2 = std::atan2(std::sin(d), std::cos(d));
  const double f1 = std::min(std::fabs(rot1), pi - std::fabs(rot1));
  const double f2 = std::min(std::fabs(rot2), pi - std::fabs(rot2));
  const double v1 = alpha[0] * f1 * f1 + alpha[1] * trans * trans;
  const double vt = alpha[2] * trans * trans + alpha[3] * (f1 * f1 + f2 * f2);
  const double v2 = alpha[0] * f2 * f2 + alpha[1] * trans * trans;
  const double sigma_z = std::sqrt(2863311530.0);
  out[0] = (float)std::cos(rot1);
  out[1] = (float)std::sin(rot1);
  out[2] = (float)trans;
  out[3] = (float)std::cos(rot2);
  out[4] = (float)std::sin(rot2);
  out[5] = (float)(std::sqrt(v1) / (2.0 * sigma_z));
  out[6] = (float)(std::sqrt(vt) / sigma_z);
  out[7] = (float)(std::sqrt(v2) / (2.0 * sigma_z));
  return RPLGPU_OK;
}

int32_t rplgpu_sample_motion_dev(rplgpu_handle_t h, const float *d_odom, uint32_t odom_per_group, uint32_t G,
                                 uint32_t M, const rplgpu_motion_noise_t *s, float *d_delta, uint64_t delta_stride,
                                 uint32_t *d_result) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  auto off = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
  if (!s) {
    h->err = "rplgpu_sample_motion_dev: the rplgpu_motion_noise_t is missing";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0 || G > 65535u) {  // (the tiles of a group by the groups: a grid's second dimension)
    h->err = "rplgpu_sample_motion_dev: G must be in 1 .. 65535";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_sample_motion_dev: M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_odom || !d_delta || !d_result || off(d_odom, 15) || off(d_delta, 15) || off(d_result, 3)) {
    h->err = "rplgpu_sample_motion_dev: a required pointer is missing or a pointer is misaligned (16 bytes for d_odom "
             "and d_delta, 4 for d_result)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (delta_stride < 4ull * M || (delta_stride & 3u)) {
    h->err = "rplgpu_sample_motion_dev: delta_stride >= 4 M and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, d_odom, "d_odom") || !device_readable(h, d_delta, "d_delta") ||
      !device_readable(h, d_result, "d_result"))
    return RPLGPU_ERR_INVALID_ARG;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_motion(h->stream, d_odom, odom_per_group, G, M, s->seed, s->step, s->first, d_delta,
                                delta_stride, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_sample_motion(rplgpu_handle_t h, const float odom[8], uint32_t M, const rplgpu_motion_noise_t *s,
                             float *delta_out, uint32_t result[8]) {
  if (!h || !odom || !s || !delta_out || !result) return RPLGPU_ERR_INVALID_ARG;
  if (M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_sample_motion: M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // one allocation per call (a convenience door, not the hot path): odometry | result | deltas, 16-byte aligned
  const size_t o_res = 32u, o_dl = 64u, total = o_dl + 16u * (size_t)M;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_sample_motion: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d, odom, 32, hipMemcpyHostToDevice, h->stream));
    const int32_t rc = rplgpu_sample_motion_dev(h, reinterpret_cast<const float *>(d), 0, 1, M, s,
                                                reinterpret_cast<float *>(d + o_dl), 4ull * M,
                                                reinterpret_cast<uint32_t *>(d + o_res));
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(delta_out, d + o_dl, 16u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d + o_res, 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

// ---- E19: a pose list seeded over a grid's free cells on the device (include/rplgpu_msg.h) ---------------------------

void rplgpu_default_pose_seed(rplgpu_pose_seed_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->resolution = 0.05f;
  s->width = 1024;
  s->height = 1024;
  s->free_lo = 0;
  s->free_hi = 0;
  s->flags = 0;
}

int32_t rplgpu_pose_seed_check(const rplgpu_pose_seed_t *s) {
  if (!s) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(s->origin_x) || !std::isfinite(s->origin_y) || !std::isfinite(s->resolution))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(s->resolution > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (s->width == 0 || s->width > RPLGPU_MAX_OCC_DIM || s->height == 0 || s->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (s->free_lo < -128 || s->free_lo > 127 || s->free_hi < -128 || s->free_hi > 127 || s->free_lo > s->free_hi)
    return RPLGPU_ERR_INVALID_ARG;
  if (s->flags > 1u) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_seed_scratch_words(uint32_t G_f, uint32_t width, uint32_t height) {
  return rpl::seed_scratch_words(G_f, width, height);
}

int32_t rplgpu_seed_headings(uint32_t H, float *cs) {
  if (!cs || H == 0 || H > 65536u) return RPLGPU_ERR_INVALID_ARG;
  const double two_pi = 6.283185307179586476925286766559;
  for (uint32_t k = 0; k < H; ++k) {
    const double a = two_pi * (double)k / (double)H;
    cs[2u * k] = k == 0 ? 1.0f : (float)std::cos(a);
    cs[2u * k + 1u] = k == 0 ? 0.0f : (float)std::sin(a);
  }
  return RPLGPU_OK;
}

// the E11 cell rule on the host: float32, every operation rounded once (this unit is built with -ffp-contract=off)
static bool seed_cell(float x, float y, const rplgpu_pose_seed_t *s, int32_t *cx, int32_t *cy) {
  const float du = x - s->origin_x, dv = y - s->origin_y;
  const float u = du / s->resolution, v = dv / s->resolution;
  const float fu = std::floor(u), fv = std::floor(v);
  if (!(std::fabs(fu) < 1048576.0f && std::fabs(fv) < 1048576.0f)) return false;
  *cx = (int32_t)fu;
  *cy = (int32_t)fv;
  return true;
}

int32_t rplgpu_seed_poses_host(const rplgpu_pose_seed_t *s, const int8_t *grid, const float *headings, uint32_t H,
                               uint32_t group, uint32_t M, const rplgpu_motion_noise_t *noise, float *poses_out,
                               uint32_t *cells_out, uint32_t result[8]) {
  if (rplgpu_pose_seed_check(s) != RPLGPU_OK || !grid || !headings || !noise || !poses_out || !result ||
      group > 65534u || H == 0 || H > 65536u || M == 0 || M > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t cells = s->width * s->height;
  auto is_free = [&](uint32_t i) { return grid[i] >= s->free_lo && grid[i] <= s->free_hi; };
  uint32_t F = 0;
  for (uint32_t i = 0; i < cells; ++i) F += is_free(i) ? 1u : 0u;
  const bool none = F == 0;
  if (none) F = cells;
  // the draws first, then ONE walk over the cells in index order hands every draw its cell: the outputs sorted by r
  std::vector<uint32_t> words(4u * (size_t)M), order(M), cell(M);
  const uint32_t key[2] = {(uint32_t)noise->seed, (uint32_t)(noise->seed >> 32)};
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t ctr[4] = {noise->first + j, (group << 2) | 3u, (uint32_t)noise->step,
                             (uint32_t)(noise->step >> 32)};
    philox4x32(ctr, key, &words[4u * (size_t)j]);
    order[j] = j;
  }
  auto rank = [&](uint32_t j) { return (uint32_t)(((uint64_t)words[4u * (size_t)j] * F) >> 32); };
  if (none) {
    for (uint32_t j = 0; j < M; ++j) cell[j] = rank(j);
  } else {
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rank(a) < rank(b); });
    uint32_t seen = 0, q = 0;  // free cells in front of cell i; outputs served
    for (uint32_t i = 0; i < cells && q < M; ++i) {
      if (!is_free(i)) continue;
      while (q < M && rank(order[q]) == seen) cell[order[q++]] = i;
      ++seen;
    }
  }
  uint32_t off = 0, lo = 0xFFFFFFFFu, hi = 0;
  const bool centres = (s->flags & 1u) != 0;
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t *p = &words[4u * (size_t)j];
    const uint32_t k = (uint32_t)(((uint64_t)p[1] * H) >> 32);
    const uint32_t cy = cell[j] / s->width, cx = cell[j] - cy * s->width;
    const float fx = centres ? 0.5f : ((float)(p[2] >> 24) + 0.5f) * (1.0f / 256.0f);
    const float fy = centres ? 0.5f : ((float)(p[3] >> 24) + 0.5f) * (1.0f / 256.0f);
    const float ux = (float)cx + fx, uy = (float)cy + fy;
    const float mx = ux * s->resolution, my = uy * s->resolution;
    const float x = s->origin_x + mx, y = s->origin_y + my;
    int32_t bx = 0, by = 0;
    if (!(seed_cell(x, y, s, &bx, &by) && bx == (int32_t)cx && by == (int32_t)cy)) ++off;
    lo = std::min(lo, cell[j]);
    hi = std::max(hi, cell[j]);
    std::memcpy(poses_out + 4u * (size_t)j, headings + 2u * (size_t)k, 8);  // bit for bit
    poses_out[4u * (size_t)j + 2u] = x;
    poses_out[4u * (size_t)j + 3u] = y;
    if (cells_out) cells_out[j] = cell[j];
  }
  result[0] = F;
  result[1] = off;
  result[2] = lo;
  result[3] = hi;
  result[4] = result[5] = result[6] = 0u;
  result[7] = (none ? 1u : 0u) | (off ? 2u : 0u);
  return RPLGPU_OK;
}

int32_t rplgpu_seed_poses_dev(rplgpu_handle_t h, const rplgpu_pose_seed_t *s, const int8_t *d_grid,
                              uint64_t grid_stride, uint32_t grid_per_group, const float *d_headings, uint32_t H,
                              uint32_t G, uint32_t M, const rplgpu_motion_noise_t *noise, float *d_poses_out,
                              uint64_t out_stride, uint32_t *d_cells_out, uint64_t cell_stride, uint32_t *d_result,
                              uint32_t *d_scratch) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  auto off = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
  if (rplgpu_pose_seed_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_seed_poses_dev: the rplgpu_pose_seed_t is missing or rplgpu_pose_seed_check refuses it";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!noise) {
    h->err = "rplgpu_seed_poses_dev: the rplgpu_motion_noise_t is missing";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0 || G > 65535u) {  // (the tiles of a group by the groups: a grid's second dimension)
    h->err = "rplgpu_seed_poses_dev: G must be in 1 .. 65535";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (M == 0 || M > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_seed_poses_dev: M must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (H == 0 || H > 65536u) {
    h->err = "rplgpu_seed_poses_dev: H must be in 1 .. 65536";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_grid || !d_headings || !d_poses_out || !d_result || !d_scratch || off(d_grid, 3) || off(d_headings, 7) ||
      off(d_poses_out, 15) || off(d_cells_out, 3) || off(d_result, 3) || off(d_scratch, 7)) {
    h->err = "rplgpu_seed_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for "
             "d_poses_out, 8 for d_headings and d_scratch, 4 for d_grid, d_cells_out and d_result)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t cells = (uint64_t)s->width * s->height;
  if (grid_stride < cells || (grid_stride & 3u)) {
    h->err = "rplgpu_seed_poses_dev: grid_stride >= width * height and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (out_stride < 4ull * M || (out_stride & 3u)) {
    h->err = "rplgpu_seed_poses_dev: out_stride >= 4 M and a multiple of 4 is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_cells_out && cell_stride < M) {
    h->err = "rplgpu_seed_poses_dev: cell_stride >= M is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, d_grid, "d_grid") || !device_readable(h, d_headings, "d_headings") ||
      !device_readable(h, d_poses_out, "d_poses_out") || !device_readable(h, d_result, "d_result") ||
      !device_readable(h, d_scratch, "d_scratch") || (d_cells_out && !device_readable(h, d_cells_out, "d_cells_out")))
    return RPLGPU_ERR_INVALID_ARG;
  rpl::SeedK k;
  k.origin_x = s->origin_x;
  k.origin_y = s->origin_y;
  k.resolution = s->resolution;
  k.width = s->width;
  k.height = s->height;
  k.free_lo = s->free_lo;
  k.free_hi = s->free_hi;
  k.centres = s->flags & 1u;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_seed(h->stream, k, d_grid, grid_stride, grid_per_group, d_headings, H, G, M, noise->seed,
                              noise->step, noise->first, d_poses_out, out_stride, d_cells_out, cell_stride, d_result,
                              d_scratch));
  return RPLGPU_OK;
}

int32_t rplgpu_seed_poses(rplgpu_handle_t h, const rplgpu_pose_seed_t *s, const int8_t *grid, const float *headings,
                          uint32_t H, uint32_t M, const rplgpu_motion_noise_t *noise, float *poses_out,
                          uint32_t *cells_out, uint32_t result[8]) {
  if (!h || !grid || !headings || !noise || !poses_out || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_seed_check(s) != RPLGPU_OK) {
    h->err = "rplgpu_seed_poses: the rplgpu_pose_seed_t is missing or rplgpu_pose_seed_check refuses it";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (M == 0 || M > RPLGPU_MAX_POSES || H == 0 || H > 65536u) {
    h->err = "rplgpu_seed_poses: M must be in 1 .. RPLGPU_MAX_POSES and H in 1 .. 65536";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // one allocation per call (a convenience door, not the hot path): result | headings | grid | scratch | cells | poses
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t cells = (size_t)s->width * s->height, gstride = (cells + 3u) & ~(size_t)3u;
  const size_t o_head = 32u, o_grid = o_head + up16(8u * (size_t)H), o_scr = o_grid + up16(gstride),
               o_cells = o_scr + up16(4u * (size_t)rplgpu_seed_scratch_words(1, s->width, s->height)),
               o_poses = o_cells + up16(4u * (size_t)M), total = o_poses + 16u * (size_t)M;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_seed_poses: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemsetAsync(d + o_grid, 0, up16(gstride), h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_head, headings, 8u * (size_t)H, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_grid, grid, cells, hipMemcpyHostToDevice, h->stream));
    const int32_t rc = rplgpu_seed_poses_dev(h, s, reinterpret_cast<const int8_t *>(d + o_grid), gstride, 0,
                                             reinterpret_cast<const float *>(d + o_head), H, 1, M, noise,
                                             reinterpret_cast<float *>(d + o_poses), 4ull * M,
                                             reinterpret_cast<uint32_t *>(d + o_cells), M,
                                             reinterpret_cast<uint32_t *>(d), reinterpret_cast<uint32_t *>(d + o_scr));
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(poses_out, d + o_poses, 16u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    if (cells_out) RPL_HIP(h, hipMemcpyAsync(cells_out, d + o_cells, 4u * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d, 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

// ---- E20: a pose list's occupied bins counted on the device (include/rplgpu_msg.h) -----------------------------------

void rplgpu_default_pose_bins(rplgpu_pose_bins_t *s) {
  if (!s) return;
  s->origin_x = -25.6f;
  s->origin_y = -25.6f;
  s->inv_size = 2.0f;
  s->nx = 103;
  s->ny = 103;
  s->flags = 0;
}

int32_t rplgpu_pose_bins_check(const rplgpu_pose_bins_t *s, uint32_t T) {
  if (!s) return RPLGPU_ERR_INVALID_ARG;
  if (!std::isfinite(s->origin_x) || !std::isfinite(s->origin_y) || !std::isfinite(s->inv_size))
    return RPLGPU_ERR_INVALID_ARG;
  if (!(s->inv_size > 0.0f)) return RPLGPU_ERR_INVALID_ARG;
  if (s->nx == 0 || s->nx > 65536u || s->ny == 0 || s->ny > 65536u) return RPLGPU_ERR_INVALID_ARG;
  if (T == 0 || T > RPLGPU_MAX_HEADING_BINS) return RPLGPU_ERR_INVALID_ARG;
  if ((uint64_t)s->nx * s->ny * T > (uint64_t)RPLGPU_MAX_POSE_BINS) return RPLGPU_ERR_INVALID_ARG;
  if (s->flags > 1u) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_bin_map_words(uint32_t nx, uint32_t ny, uint32_t T) {
  rplgpu_pose_bins_t s;
  rplgpu_default_pose_bins(&s);
  s.nx = nx;
  s.ny = ny;
  if (rplgpu_pose_bins_check(&s, T) != RPLGPU_OK) return 0;
  const uint64_t words = ((uint64_t)nx * ny * T + 31u) >> 5;
  return (words + 1u) & ~(uint64_t)1u;
}

// E20's quantisation of (c, s), E17's rule: one float32 product, the range test, one round-to-nearest-even; false for
// an entry that is out of range or quantises to (0, 0)
static bool bins_quantise(const float *cs, int32_t q[2]) {
  const float tc = cs[0] * 1048576.0f, ts = cs[1] * 1048576.0f;
  q[0] = q[1] = 0;
  if (!(std::fabs(tc) < 8388608.0f && std::fabs(ts) < 8388608.0f)) return false;
  q[0] = (int32_t)std::rint(tc);
  q[1] = (int32_t)std::rint(ts);
  return q[0] != 0 || q[1] != 0;
}
static uint32_t bins_half(const int32_t a[2]) { return (a[1] > 0 || (a[1] == 0 && a[0] > 0)) ? 0u : 1u; }
// a <= b in the angular order, both in range and not (0, 0)
static bool bins_le(const int32_t a[2], const int32_t b[2]) {
  const uint32_t ha = bins_half(a), hb = bins_half(b);
  if (ha != hb) return ha < hb;
  return (int64_t)a[0] * b[1] - (int64_t)a[1] * b[0] >= 0;
}

int32_t rplgpu_heading_edges_check(const float *cs, uint32_t T) {
  if (!cs || T == 0 || T > RPLGPU_MAX_HEADING_BINS) return RPLGPU_ERR_INVALID_ARG;
  int32_t prev[2], cur[2];
  if (!bins_quantise(cs, prev) || prev[0] != 1048576 || prev[1] != 0) return RPLGPU_ERR_INVALID_ARG;
  for (uint32_t k = 1; k < T; ++k) {
    if (!bins_quantise(cs + 2u * (size_t)k, cur)) return RPLGPU_ERR_INVALID_ARG;
    if (bins_le(cur, prev)) return RPLGPU_ERR_INVALID_ARG;  // not strictly behind its predecessor
    prev[0] = cur[0];
    prev[1] = cur[1];
  }
  return RPLGPU_OK;
}

int32_t rplgpu_bin_poses_host(const rplgpu_pose_bins_t *s, const float *poses, uint32_t P, const uint32_t *weights,
                              const float *edges, uint32_t T, uint32_t *map, uint32_t *bins_out,
                              uint32_t result[8]) {
  if (rplgpu_pose_bins_check(s, T) != RPLGPU_OK || !poses || !edges || !map || !result || P == 0 ||
      P > RPLGPU_MAX_POSES)
    return RPLGPU_ERR_INVALID_ARG;
  const uint32_t nb = s->nx * s->ny * T, words = (nb + 31u) >> 5;
  const bool keep = (s->flags & 1u) != 0;
  if (!keep) std::memset(map, 0, 4u * (size_t)words);
  std::vector<int32_t> eq(2u * (size_t)T);
  std::vector<unsigned char> e_ok(T);
  for (uint32_t k = 0; k < T; ++k) e_ok[k] = bins_quantise(edges + 2u * (size_t)k, &eq[2u * (size_t)k]) ? 1 : 0;
  uint32_t K = 0, counted = 0, outside = 0, skipped = 0, lo_bin = 0xFFFFFFFFu, hi_bin = 0;
  for (uint32_t i = 0; i < P; ++i) {
    const float *p = poses + 4u * (size_t)i;
    uint32_t b = 0xFFFFFFFFu;
    if (weights && weights[i] == 0u) {
      ++skipped;  // (whether or not it is in range)
    } else {
      const float dx = p[2] - s->origin_x, dy = p[3] - s->origin_y;
      const float fx = dx * s->inv_size, fy = dy * s->inv_size;  // (-ffp-contract=off: the difference rounded first)
      const bool x_in = fx >= 0.0f && fx < (float)s->nx;
      const bool y_in = fy >= 0.0f && fy < (float)s->ny;
      int32_t h[2];
      const bool h_in = bins_quantise(p, h);
      if (x_in && y_in && h_in) {
        const uint32_t bx = (uint32_t)std::floor(fx), by = (uint32_t)std::floor(fy);
        uint32_t lo = 0, hi = T;
        while (hi - lo > 1u) {
          const uint32_t mid = (lo + hi) >> 1;
          if (e_ok[mid] && bins_le(&eq[2u * (size_t)mid], h))
            lo = mid;
          else
            hi = mid;
        }
        b = (lo * s->ny + by) * s->nx + bx;
        ++counted;
        lo_bin = std::min(lo_bin, b);
        hi_bin = std::max(hi_bin, b);
        const uint32_t bit = 1u << (b & 31u);
        if (!(map[b >> 5] & bit)) ++K;  // a bit this call turns from 0 to 1
        map[b >> 5] |= bit;
      } else {
        ++outside;
      }
    }
    if (bins_out) bins_out[i] = b;
  }
  result[0] = K;
  result[1] = counted;
  result[2] = outside;
  result[3] = skipped;
  result[4] = lo_bin;
  result[5] = hi_bin;
  result[6] = 0u;
  result[7] = (counted == 0 ? 1u : 0u) | (outside != 0 ? 2u : 0u) | (keep ? 4u : 0u);
  return RPLGPU_OK;
}

int32_t rplgpu_bin_poses_dev(rplgpu_handle_t h, const rplgpu_pose_bins_t *s, const float *d_poses,
                             uint64_t pose_stride, uint32_t poses_per_group, const uint32_t *d_weights,
                             uint64_t weight_stride, uint32_t G, uint32_t P, const float *d_edges, uint32_t T,
                             uint32_t *d_map, uint64_t map_stride, uint32_t *d_bins_out, uint64_t bin_stride,
                             uint32_t *d_result) {
  if (!h) return RPLGPU_ERR_INVALID_ARG;
  auto off = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
  if (rplgpu_pose_bins_check(s, T) != RPLGPU_OK) {
    h->err = "rplgpu_bin_poses_dev: the rplgpu_pose_bins_t is missing or rplgpu_pose_bins_check refuses it or T";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (G == 0 || G > 65535u) {  // (the tiles of a group by the groups: a grid's second dimension)
    h->err = "rplgpu_bin_poses_dev: G must be in 1 .. 65535";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_bin_poses_dev: P must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!d_poses || !d_edges || !d_map || !d_result || off(d_poses, 15) || off(d_edges, 7) || off(d_map, 7) ||
      off(d_weights, 3) || off(d_bins_out, 3) || off(d_result, 3)) {
    h->err = "rplgpu_bin_poses_dev: a required pointer is missing or a pointer is misaligned (16 bytes for d_poses, "
             "8 for d_edges and d_map, 4 for d_weights, d_bins_out and d_result)";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (pose_stride < 4ull * P || (pose_stride & 3u) || (d_weights && weight_stride < P)) {
    h->err = "rplgpu_bin_poses_dev: pose_stride >= 4 P and a multiple of 4 and weight_stride >= P are required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  const uint64_t words = ((uint64_t)s->nx * s->ny * T + 31u) >> 5;
  if (map_stride < words || (map_stride & 1u)) {
    h->err = "rplgpu_bin_poses_dev: map_stride >= ceil(nx * ny * T / 32) and even is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (d_bins_out && bin_stride < P) {
    h->err = "rplgpu_bin_poses_dev: bin_stride >= P is required";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (!device_readable(h, d_poses, "d_poses") || !device_readable(h, d_edges, "d_edges") ||
      !device_readable(h, d_map, "d_map") || !device_readable(h, d_result, "d_result") ||
      (d_weights && !device_readable(h, d_weights, "d_weights")) ||
      (d_bins_out && !device_readable(h, d_bins_out, "d_bins_out")))
    return RPLGPU_ERR_INVALID_ARG;
  rpl::BinsK k;
  k.origin_x = s->origin_x;
  k.origin_y = s->origin_y;
  k.inv_size = s->inv_size;
  k.nx = s->nx;
  k.ny = s->ny;
  k.keep = s->flags & 1u;
  RPL_HIP(h, hipSetDevice(h->device));
  RPL_HIP(h, rpl::launch_bins(h->stream, k, d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P,
                              d_edges, T, d_map, map_stride, d_bins_out, bin_stride, d_result));
  return RPLGPU_OK;
}

int32_t rplgpu_bin_poses(rplgpu_handle_t h, const rplgpu_pose_bins_t *s, const float *poses, uint32_t P,
                         const uint32_t *weights, const float *edges, uint32_t T, uint32_t *map, uint32_t *bins_out,
                         uint32_t result[8]) {
  if (!h || !poses || !edges || !map || !result) return RPLGPU_ERR_INVALID_ARG;
  if (rplgpu_pose_bins_check(s, T) != RPLGPU_OK) {
    h->err = "rplgpu_bin_poses: the rplgpu_pose_bins_t is missing or rplgpu_pose_bins_check refuses it or T";
    return RPLGPU_ERR_INVALID_ARG;
  }
  if (P == 0 || P > RPLGPU_MAX_POSES) {
    h->err = "rplgpu_bin_poses: P must be in 1 .. RPLGPU_MAX_POSES";
    return RPLGPU_ERR_INVALID_ARG;
  }
  RPL_HIP(h, hipSetDevice(h->device));
  // one allocation per call (a convenience door, not the hot path): result | edges | map | weights | bins | poses
  auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
  const size_t words = ((size_t)s->nx * s->ny * T + 31u) >> 5, stride = (size_t)rplgpu_bin_map_words(s->nx, s->ny, T);
  const size_t o_edge = 32u, o_map = o_edge + up16(8u * (size_t)T), o_wt = o_map + up16(4u * stride),
               o_bins = o_wt + up16(4u * (size_t)P), o_poses = o_bins + up16(4u * (size_t)P),
               total = o_poses + 16u * (size_t)P;
  unsigned char *d = nullptr;
  if (hipMalloc((void **)&d, total) != hipSuccess) {
    h->err = "rplgpu_bin_poses: device allocation failed";
    (void)hipGetLastError();
    return RPLGPU_ERR_HIP;
  }
  uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> map_back(words), bins_back(bins_out ? P : 0u);
  auto run = [&]() -> int32_t {
    RPL_HIP(h, hipMemcpyAsync(d + o_poses, poses, 16u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(d + o_edge, edges, 8u * (size_t)T, hipMemcpyHostToDevice, h->stream));
    if (weights) RPL_HIP(h, hipMemcpyAsync(d + o_wt, weights, 4u * (size_t)P, hipMemcpyHostToDevice, h->stream));
    if (s->flags & 1u) RPL_HIP(h, hipMemcpyAsync(d + o_map, map, 4u * words, hipMemcpyHostToDevice, h->stream));
    const int32_t rc = rplgpu_bin_poses_dev(
        h, s, reinterpret_cast<const float *>(d + o_poses), 4ull * P, 0,
        weights ? reinterpret_cast<const uint32_t *>(d + o_wt) : nullptr, P, 1, P,
        reinterpret_cast<const float *>(d + o_edge), T, reinterpret_cast<uint32_t *>(d + o_map), stride,
        bins_out ? reinterpret_cast<uint32_t *>(d + o_bins) : nullptr, P, reinterpret_cast<uint32_t *>(d));
    if (rc) return rc;
    RPL_HIP(h, hipMemcpyAsync(map_back.data(), d + o_map, 4u * words, hipMemcpyDeviceToHost, h->stream));
    if (bins_out)
      RPL_HIP(h, hipMemcpyAsync(bins_back.data(), d + o_bins, 4u * (size_t)P, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipMemcpyAsync(small, d, 32, hipMemcpyDeviceToHost, h->stream));
    RPL_HIP(h, hipStreamSynchronize(h->stream));
    return RPLGPU_OK;
  };
  const int32_t rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);  // nothing queued may outlive the buffer
  (void)hipFree(d);
  if (rc) return rc;  // (no output changed)
  std::memcpy(map, map_back.data(), 4u * words);
  if (bins_out) std::memcpy(bins_out, bins_back.data(), 4u * (size_t)P);
  std::memcpy(result, small, 32);
  return RPLGPU_OK;
}

uint32_t rplgpu_kld_samples(uint32_t k, double epsilon, double z, uint32_t m_min, uint32_t m_max) {
  if (k <= 1u) return m_max;
  const double b = 2.0 / (9.0 * ((double)k - 1.0));
  const double x = 1.0 - b + std::sqrt(b) * z;
  const double n = std::ceil(((double)k - 1.0) / (2.0 * epsilon) * x * x * x);
  if (!(n >= (double)m_min)) return m_min;  // (NaN too)
  if (n > (double)m_max) return m_max;
  return (uint32_t)n;
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
  RPL_HIP(h, rpl::launch_decode(h->stream, ans_type, d_bytes, stream_stride, d_frame_off, d_gap,
                                d_n_frames, max_frames, B, sample_duration_us, d_state_in,
                                d_state_out, d_nodes, node_stride, d_n_nodes, d_reset_at,
                                reset_stride, d_n_reset, d_n_errors, d_status, nullptr, 0, nullptr,
                                nullptr, h->dec_stage, stage_todo));
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
  const uint32_t *only = nullptr;
  // (with a carried scan every stream takes the general path: the fused decoder neither decodes
  // the nodes in front of a call's first sync node nor those behind its last)
  if (!carry && rpl::decode_fusable(ans_type)) {
    RPL_HIP(h, rpl::launch_decode_fused(h->stream, ans_type, d_bytes, stream_stride, d_frame_off,
                                        d_gap, d_n_frames, max_frames, B, sample_duration_us,
                                        d_state_in, d_state_out, d_n_errors, d_status, max_count,
                                        d_batch, n_stride, scan_cap, d_n_per_scan, d_n_scans, t_todo,
                                        h->dec_stage));
    only = t_todo;
  }
  RPL_HIP(h, rpl::launch_decode(h->stream, ans_type, d_bytes, stream_stride, d_frame_off, d_gap,
                                d_n_frames, max_frames, B, sample_duration_us, d_state_in,
                                d_state_out, t_nodes, node_stride, t_nn, t_rst, reset_stride, t_nr,
                                d_n_errors, d_status, t_sync, sync_stride, t_ns, only, h->dec_stage,
                                d_frame_off ? t_stage_todo : nullptr));
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
  auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
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
