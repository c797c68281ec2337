// rpl_host.hpp — what the host translation units share: rplgpu_api.hip (handle, single scans, batches, clouds,
// decode, messages, exchange), rplgpu_scan_stages.hip (E9 - E14), rplgpu_pose_stages.hip (E15 - E23) and rplgpu_wide_stages.hip (E24).
//
// Host code only, internal to the library: everything in rpl::host has hidden visibility, so nothing declared here
// is an exported symbol.  rplgpu_api.hip defines the handle's helpers, rplgpu_scan_stages.hip the scan-stage
// prologue; the per-call buffer of the host-buffer doors is defined here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_launch.hpp"

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

#define RPL_HIP(ctx, call)                                                              \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
      return RPLGPU_ERR_HIP;                                                            \
    }                                                                                   \
  } while (0)

namespace rpl {
namespace host {
#pragma GCC visibility push(hidden)

constexpr uint32_t kMaskStride = rpl::kMaxN / 32u;  // keep-mask words per scan
constexpr size_t kTail = 64;  // bytes behind a staging region for the words that travel with it

// Single-scan staging (pinned, one allocation): nodes | tail | results (16 B / sample) | tail | flag.
// Both regions are rounded up to 64 bytes, so that for EVERY capacity the result area (it receives
// 16-byte stores) and the flag word's cache line start on a 64-byte boundary.
constexpr size_t round64(size_t v) { return (v + 63u) & ~(size_t)63u; }
constexpr size_t stage_out_off(size_t max_n) { return round64(max_n * 8) + kTail; }
// Single-scan staging (pinned host side): nodes | length word ... results | result words.
inline unsigned char *stage_out(const rplgpu_ctx *c) { return c->h_pin + stage_out_off(c->max_n); }

// ---- the handle's helpers (rplgpu_api.hip) ----------------------------------------------------------------------------
rpl::KParams to_kparams(const rplgpu_params_t &p);
rpl::Tables tables_of(rplgpu_ctx *c);
// `what` is device (or managed / mapped host) memory reachable from the handle's device; else c->err names it
bool device_readable(rplgpu_ctx *c, const void *ptr, const char *what);
int32_t check_batch(rplgpu_ctx *c, const void *nodes, uint32_t n_stride, const void *n_per_scan, uint32_t B,
                    bool own_buffers = false);  // (the handle's own staging: no pointer check)

// What the launch sites consult: the validators' verdicts, less what rplgpu_debug_force_ieee_div refuses.
inline bool use_fast_d4000(const rplgpu_ctx *c) { return c->div4000_ok && !(c->force_ieee & 1u); }
inline bool use_fast_leaf(const rplgpu_ctx *c) { return c->leaf_ok && !(c->force_ieee & 2u); }
inline bool use_fast_idx(const rplgpu_ctx *c) { return c->idx_ok && !(c->force_ieee & 4u); }

// ---- pointer checks ---------------------------------------------------------------------------------------------------
inline bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// device_readable over a short list, in the list's order; a NULL pointer that is not required passes
struct PtrCheck {
  const void *p;
  const char *name;
  bool required;
};
inline bool device_readable(rplgpu_ctx *c, std::initializer_list<PtrCheck> list) {
  for (const PtrCheck &e : list)
    if ((e.required || e.p) && !device_readable(c, e.p, e.name)) return false;
  return true;
}

// ---- the table of a call's byte ranges --------------------------------------------------------------------------------
struct Range {
  const void *p;
  uint64_t bytes;
  bool out;
};
// No output may share a byte with an input or with another output.  A pair is passed over when neither is an output,
// when either pointer is NULL or either length 0 (an optional argument that was not given), or when it is the pair
// (skip_a, skip_b) of entries, skip_a < skip_b, which the caller has found to be ONE range read and written element
// by element (an accepted in-place form).
template <size_t N>
inline bool ranges_clash(const Range (&ranges)[N], int skip_a = -1, int skip_b = -1) {
  for (size_t i = 0; i < N; ++i) {
    for (size_t j = i + 1; j < N; ++j) {
      const Range &a = ranges[i], &b = ranges[j];
      if (!(a.out || b.out) || !a.p || !b.p || !a.bytes || !b.bytes || ((int)i == skip_a && (int)j == skip_b)) continue;
      if (rpl::ranges_overlap(a.p, a.bytes, b.p, b.bytes)) return true;
    }
  }
  return false;
}

// a spec its check refused: c->err is "<fn>: invalid <type> (see include/rplgpu_msg.h)"
inline int32_t refuse_spec(rplgpu_ctx *c, const char *fn, const char *type) {
  c->err = std::string(fn) + ": invalid " + type + " (see include/rplgpu_msg.h)";
  return RPLGPU_ERR_INVALID_ARG;
}

// a refusal with its reason: c->err is "<fn>: <what>"; false
inline bool refuse(rplgpu_ctx *c, const char *fn, const char *what) {
  c->err = std::string(fn) + ": " + what;
  return false;
}

// the grid planes and the field planes of E26, E27 and E29 (d_potential NULL: the call takes none), `cells` a plane
inline bool planes_ok(rplgpu_ctx *c, const char *fn, uint64_t cells, const void *d_grid, uint64_t grid_stride,
                      const void *d_potential, uint64_t potential_stride) {
  return (grid_stride >= cells && !(grid_stride & 3u) && !misaligned(d_grid, 3u) &&
          (!d_potential || potential_stride >= cells) && !misaligned(d_potential, 3u)) ||
         refuse(c, fn, "grid_stride must be >= width * height and a multiple of 4, potential_stride >= width * height, "
                       "d_grid and d_potential 4-byte aligned");
}

// ---- the pose-list doors ----------------------------------------------------------------------------------------------
// What the doors of the pose-list stages refuse alike, in parts, because a door tests its pointers between the counts
// and the strides and the order of its tests is part of what a caller sees.  false: c->err is "<fn>: <what>".
struct PoseListDoor {
  rplgpu_ctx *c;
  const char *fn;
  bool refuse(const char *what) const { return rpl::host::refuse(c, fn, what); }
  // (the tiles of a group by the groups: a grid's second dimension)
  bool groups(uint32_t G) const { return (G != 0 && G <= 65535u) || refuse("G must be in 1 .. 65535"); }
  bool poses(uint32_t P) const {
    return (P != 0 && P <= RPLGPU_MAX_POSES) || refuse("P must be in 1 .. RPLGPU_MAX_POSES");
  }
  bool strides(uint32_t P, uint64_t pose_stride, const void *weights, uint64_t weight_stride) const {
    return (pose_stride >= 4ull * P && !(pose_stride & 3u) && (!weights || weight_stride >= P)) ||
           refuse("pose_stride >= 4 P and a multiple of 4 and weight_stride >= P are required");
  }
};

// ---- the scan-stage prologue (rplgpu_scan_stages.hip) -----------------------------------------------------------------
// What E11, E13, E14 and E15 run between their own argument checks and their launches (E9: admit() only).  A stage's
// own limit on `group` sits between the two calls, where it always sat.
struct ScanPrologue {
  uint32_t group = 0, G = 0;  // the group size in use and the number of groups (admit)
  rpl::KParams kp;            // (begin)
  rpl::Tables T;
  const uint32_t *mask = nullptr;  // E1 AND E5 keep bits when p->ror_enable, kMaskStride words per scan

  // the two refusals every scan stage shares, then group = min(group, B) (as E8: "all sensors in one group" may be
  // asked for with any group >= B).  d_t0: the per-scan time offsets of E6 for this call, or NULL.
  int32_t admit(rplgpu_ctx *h, const char *fn, const rplgpu_params_t *p, const float *d_motion, const float *d_t0,
                uint32_t B, uint32_t group_asked);
  // the handle's device, the kernel parameters and tables with d_t0, the keep mask queued, d_status cleared
  int32_t begin(rplgpu_ctx *h, const rplgpu_node_t *d_nodes, uint32_t n_stride, const uint32_t *d_n_per_scan,
                uint32_t B, const rplgpu_params_t *p, const float *d_t0, uint32_t *d_status);
};

// ---- the host-buffer doors --------------------------------------------------------------------------------------------
constexpr size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// The device buffer of one call of a host-buffer door (a convenience door, not the hot path): parts reserved one
// behind the other, each 16-byte aligned, ONE allocation around the body, freed before run() returns.
class DoorBuffer {
 public:
  static constexpr size_t kAbsent = ~(size_t)0;  // the part of an optional argument that was not given
  DoorBuffer(rplgpu_ctx *h, const char *fn) : h_(h), fn_(fn) {}
  size_t part(size_t bytes) {
    const size_t off = total_;
    total_ += up16(bytes);
    return off;
  }
  size_t part_if(bool present, size_t bytes) { return present ? part(bytes) : kAbsent; }
  // (inside the body) the device address of a part; NULL for kAbsent
  template <class T = unsigned char>
  T *at(size_t off) const {
    return off == kAbsent ? nullptr : reinterpret_cast<T *>(d_ + off);
  }
  // (inside the body) a host block queued into a part, a part queued out to a host block, on the handle's stream; a
  // NULL block, an absent part or no bytes: nothing
  hipError_t put(size_t off, const void *src, size_t bytes) const {
    if (!src || off == kAbsent || !bytes) return hipSuccess;
    return hipMemcpyAsync(d_ + off, src, bytes, hipMemcpyHostToDevice, h_->stream);
  }
  hipError_t get(void *dst, size_t off, size_t bytes) const {
    if (!dst || off == kAbsent || !bytes) return hipSuccess;
    return hipMemcpyAsync(dst, d_ + off, bytes, hipMemcpyDeviceToHost, h_->stream);
  }
  // body: the uploads, the _dev call, the downloads and ONE synchronise; its return code is the door's
  template <class Body>
  int32_t run(Body &&body) {
    if (hipMalloc((void **)&d_, total_) != hipSuccess) {
      h_->err = std::string(fn_) + ": device allocation failed";
      (void)hipGetLastError();
      return RPLGPU_ERR_HIP;
    }
    const int32_t rc = body();
    if (rc) (void)hipStreamSynchronize(h_->stream);  // nothing queued may outlive the buffer
    (void)hipFree(d_);
    d_ = nullptr;
    return rc;
  }

 private:
  rplgpu_ctx *h_;
  const char *fn_;
  size_t total_ = 0;
  unsigned char *d_ = nullptr;
};

// The scans of a door: nodes | lengths | motion (16 B per scan) | pose2d (24 B) | t0 (4 B), the last three optional.
// The constructor reserves the parts, upload() (inside the body) queues the copies and sets the device pointers.
struct DoorScans {
  DoorScans(DoorBuffer &buf, const rplgpu_node_t *nodes, uint32_t n_stride, const uint32_t *n_per_scan,
            uint32_t n_scans, const float *motion, const float *pose2d, const float *t0)
      : nodes_(nodes), n_per_scan_(n_per_scan), motion_(motion), pose2d_(pose2d), t0_(t0), n_(n_scans),
        nb_((size_t)n_scans * n_stride * 8u), o_nodes_(buf.part(nb_)), o_len_(buf.part(4u * (size_t)n_scans)),
        o_motion_(buf.part_if(motion, 16u * (size_t)n_scans)), o_pose2d_(buf.part_if(pose2d, 24u * (size_t)n_scans)),
        o_t0_(buf.part_if(t0, 4u * (size_t)n_scans)) {}
  int32_t upload(rplgpu_ctx *h, const DoorBuffer &buf) {
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_nodes_), nodes_, nb_, hipMemcpyHostToDevice, h->stream));
    RPL_HIP(h, hipMemcpyAsync(buf.at(o_len_), n_per_scan_, 4u * n_, hipMemcpyHostToDevice, h->stream));
    if (motion_) RPL_HIP(h, hipMemcpyAsync(buf.at(o_motion_), motion_, 16u * n_, hipMemcpyHostToDevice, h->stream));
    if (pose2d_) RPL_HIP(h, hipMemcpyAsync(buf.at(o_pose2d_), pose2d_, 24u * n_, hipMemcpyHostToDevice, h->stream));
    if (t0_) RPL_HIP(h, hipMemcpyAsync(buf.at(o_t0_), t0_, 4u * n_, hipMemcpyHostToDevice, h->stream));
    d_nodes = buf.at<const rplgpu_node_t>(o_nodes_);
    d_n_per_scan = buf.at<const uint32_t>(o_len_);
    d_motion = buf.at<const float>(o_motion_);
    d_pose2d = buf.at<const float>(o_pose2d_);
    d_t0 = buf.at<const float>(o_t0_);
    return RPLGPU_OK;
  }
  const rplgpu_node_t *d_nodes = nullptr;
  const uint32_t *d_n_per_scan = nullptr;
  const float *d_motion = nullptr, *d_pose2d = nullptr, *d_t0 = nullptr;  // NULL where the door was given none

 private:
  const rplgpu_node_t *nodes_;
  const uint32_t *n_per_scan_;
  const float *motion_, *pose2d_, *t0_;
  size_t n_, nb_, o_nodes_, o_len_, o_motion_, o_pose2d_, o_t0_;
};

#pragma GCC visibility pop
}  // namespace host
}  // namespace rpl
