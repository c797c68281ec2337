/*
 * rplgpu_msg.h — publish-ready messages: the LaserScan / PointCloud2
 * the path produces, laid out as the serialised (CDR) messages a ROS 2 publisher sends, so the
 * node hands the buffer to `publish(const rclcpp::SerializedMessage &)` without building a typed
 * message and without a further copy.
 *
 * What it replaces in the reference, per scan:
 *   sensor_msgs::msg::LaserScan scan_msg; ... scan_msg.ranges.assign / [index] = ...;
 *   scan_pub_->publish(scan_msg);                  src/rplidar_node.cpp:618-682
 * i.e. two std::vector<float> fills, then the middleware's own serialisation pass over them
 * (rosidl_typesupport_fastrtps_cpp + eProsima Fast-CDR; third-party, not in the reference tree:
 * the README names ROS 2 Jazzy, whose default rmw serialises with Fast-CDR 2.2.x as XCDR
 * version 1, PLAIN_CDR, little endian).  Here the device results are copied ONCE, by DMA,
 * straight to their final offsets inside the serialised message; for device-resident batches
 * a kernel assembles B messages in HBM.
 *
 * Wire format (OMG DDS-XTypes 1.3 §7.4.1 "plain CDR" as Fast-CDR emits it for ROS 2):
 *   4-byte encapsulation header 00 01 00 00 (CDR little endian, no options); every primitive
 *   aligned to its size counted from the byte AFTER that header; string = uint32 length
 *   including the terminating NUL, the bytes, the NUL; sequence<T> = uint32 element count, the
 *   elements; bool / uint8 = one byte; no padding after the last member.
 *   std_msgs/Header = { int32 stamp.sec, uint32 stamp.nanosec, string frame_id }.
 *   sensor_msgs/LaserScan = Header, float32 angle_min, angle_max, angle_increment,
 *     time_increment, scan_time, range_min, range_max, float32[] ranges, float32[] intensities.
 *   sensor_msgs/PointCloud2 = Header, uint32 height, width, PointField[] fields
 *     ({string name, uint32 offset, uint8 datatype, uint32 count}), bool is_bigendian,
 *     uint32 point_step, row_step, uint8[] data, bool is_dense — with the E3 layout of
 *     fields x,y,z,intensity FLOAT32 (=7) at 0/4/8/12, point_step 16, height 1,
 *     width = #points, row_step = 16*width, is_bigendian false, is_dense true.
 *
 * Parity: the reference holds no serialised vectors and Fast-CDR is not in this image, so the
 * byte layout is checked against an independent restatement of the format (oracle/cdr_oracle.py)
 * and hand-derived known-answer bytes — "parity unpinned" for the wire format itself; the float
 * payloads inside the messages are the same bit-exact results as rplgpu.h's entry points.
 */
#ifndef RPLGPU_MSG_H_
#define RPLGPU_MSG_H_

#include "rplgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rplgpu_stamp {
  int32_t sec;      /* builtin_interfaces/Time */
  uint32_t nanosec;
} rplgpu_stamp_t;

/* Byte offsets inside one serialised LaserScan (from the first byte of the encapsulation
 * header).  All are multiples of 4. */
typedef struct rplgpu_laserscan_layout {
  uint32_t scalars_off;         /* angle_min; the 7 float32 scalars follow each other */
  uint32_t ranges_len_off;      /* uint32 ranges.size() */
  uint32_t ranges_off;          /* ranges[0] */
  uint32_t intensities_len_off; /* uint32 intensities.size() */
  uint32_t intensities_off;     /* intensities[0] */
  uint32_t total_len;           /* serialised size */
} rplgpu_laserscan_layout_t;

/* Byte offsets inside one serialised PointCloud2. */
typedef struct rplgpu_cloud_layout {
  uint32_t width_off;    /* uint32 width (height precedes it) */
  uint32_t row_step_off; /* uint32 row_step (point_step precedes it) */
  uint32_t data_len_off; /* uint32 data.size() = 16 * n_points */
  uint32_t data_off;     /* first point; a multiple of 4 */
  uint32_t is_dense_off; /* the last byte */
  uint32_t total_len;
} rplgpu_cloud_layout_t;

/* ---- host-only: layout and everything but the bulk arrays (no device needed) ------------- */
/* frame_id_len = strlen(frame_id).  Returns RPLGPU_ERR_INVALID_ARG if the message would not
 * fit 32-bit offsets. */
int32_t rplgpu_msg_laserscan_layout(size_t frame_id_len, uint32_t count,
                                    rplgpu_laserscan_layout_t *out);
int32_t rplgpu_msg_cloud_layout(size_t frame_id_len, uint32_t n_points,
                                rplgpu_cloud_layout_t *out);
/* Write encapsulation header, Header, the 7 scalars of `meta` and both sequence lengths
 * (meta->count) into msg[0..cap); the float arrays at ranges_off / intensities_off are left
 * for the caller (or the DMA) to fill.  RPLGPU_ERR_CAPACITY if total_len > cap. */
int32_t rplgpu_msg_laserscan_header(const char *frame_id, rplgpu_stamp_t stamp,
                                    const rplgpu_scan_meta_t *meta, uint8_t *msg, size_t cap,
                                    rplgpu_laserscan_layout_t *layout);
/* Write everything of a PointCloud2 but the points (16 * n_points bytes at data_off). */
int32_t rplgpu_msg_cloud_header(const char *frame_id, rplgpu_stamp_t stamp, uint32_t n_points,
                                uint8_t *msg, size_t cap, rplgpu_cloud_layout_t *layout);

/* ---- pinned message buffers ---------------------------------------------------------------- */
/* Page-locked host memory: a message buffer obtained here receives the device results by DMA
 * with no staging copy (any other host pointer works too, through the runtime's staging). */
int32_t rplgpu_host_alloc(rplgpu_handle_t h, size_t bytes, void **out);
int32_t rplgpu_host_free(rplgpu_handle_t h, void *p);

/* ---- single scan: raw nodes -> one serialised message in a HOST buffer --------------------- */
/* == the body of publish_scan (src/rplidar_node.cpp:568-680) plus the serialisation of the
 * result.  *msg_len = 0 and meta->published = 0 when publish_scan would have returned without
 * publishing (:561,:611).  cap must hold the message for the worst case count == n
 * (rplgpu_msg_laserscan_layout(strlen(frame_id), n)). */
int32_t rplgpu_scan_to_laserscan_msg(rplgpu_handle_t h, const rplgpu_node_t *nodes, size_t n,
                                     const rplgpu_params_t *p, double scan_duration,
                                     const char *frame_id, rplgpu_stamp_t stamp, uint8_t *msg,
                                     size_t cap, size_t *msg_len, rplgpu_scan_meta_t *meta);
/* ext E1-E5 -> serialised PointCloud2 (an empty cloud is a valid message: width 0). */
int32_t rplgpu_scan_to_cloud_msg(rplgpu_handle_t h, const rplgpu_node_t *nodes, size_t n,
                                 const rplgpu_params_t *p, const char *frame_id,
                                 rplgpu_stamp_t stamp, uint8_t *msg, size_t cap, size_t *msg_len,
                                 uint32_t *n_points, uint32_t *status);

/* ---- batches: B serialised messages assembled in DEVICE memory ----------------------------- */
/* From the outputs of rplgpu_laserscan_batch_dev (same d_ranges / d_intensities / n_stride /
 * d_beam_count): message b at d_msgs + b*msg_stride (msg_stride a multiple of 4), its length
 * in d_msg_len[b]; 0 = not published (beam count 0) or msg_stride too small (then d_status[b]
 * gets RPLGPU_SCAN_OUT_TRUNCATED).  A scan has count = min(d_beam_count[b], n_stride) beams, as in
 * E7 and E10: a count above the stride never reads the next scan's slot, and the message (its
 * scalars and length words included) is that of n_stride beams.  The scalars are computed on the device with the
 * reference's own expressions (:623-627,:634-638,:665-669; IEEE fp64 divides).
 * d_stamps: B stamps; d_scan_duration: B doubles; both device pointers. */
int32_t rplgpu_laserscan_msgs_dev(rplgpu_handle_t h, const float *d_ranges,
                                  const float *d_intensities, uint32_t n_stride,
                                  const uint32_t *d_beam_count, uint32_t B,
                                  const rplgpu_params_t *p, const char *frame_id,
                                  const rplgpu_stamp_t *d_stamps, const double *d_scan_duration,
                                  uint8_t *d_msgs, uint32_t msg_stride, uint32_t *d_msg_len,
                                  uint32_t *d_status);
/* From the outputs of rplgpu_cloud_batch_dev (d_scan_start = NULL: scan b at
 * d_xyzi + b*out_stride points) or rplgpu_cloud_arena_dev (d_xyzi = the arena, d_scan_start =
 * its per-scan starts).  Same message slots as above. */
int32_t rplgpu_cloud_msgs_dev(rplgpu_handle_t h, const float *d_xyzi, uint32_t out_stride,
                              const uint64_t *d_scan_start, const uint32_t *d_n_points,
                              uint32_t B, const char *frame_id, const rplgpu_stamp_t *d_stamps,
                              uint8_t *d_msgs, uint32_t msg_stride, uint32_t *d_msg_len,
                              uint32_t *d_status);

/* ---- LaserScan -> PointCloud2 projection (E7; row 3's `laser_geometry`-style cloud source) ---
 * Input: what publish_scan produces (src/rplidar_node.cpp:618-662 Mode A, :663-680 Mode B) —
 * the outputs of rplgpu_laserscan_batch_dev, still in HBM.  For scan b with count =
 * d_beam_count[b] and angle_increment as the reference computes it (Mode A :635, Mode B
 * :666-668; p->scan_processing selects), beam i is kept iff ranges[i] is finite (Mode A's empty
 * bins are +inf, :640) and, with p->clip_enable, range_min <= ranges[i] <= range_max; then
 *   theta = angle_min + float(i) * angle_increment            (float32; angle_min = 0, :623)
 *   x = ranges[i] * (float)cos((double)theta);  y = ranges[i] * (float)sin((double)theta);  z = 0
 *   intensity = intensities[i]
 * in beam order, E3 layout (16-byte points), d_n_points[b] points at d_xyzi + b*out_stride.
 * The serialised message of such a cloud is rplgpu_cloud_msgs_dev on the result. */
int32_t rplgpu_laserscan_to_cloud_batch_dev(rplgpu_handle_t h, const float *d_ranges,
                                            const float *d_intensities, uint32_t n_stride,
                                            const uint32_t *d_beam_count, uint32_t B,
                                            const rplgpu_params_t *p, float *d_xyzi,
                                            uint32_t out_stride, uint32_t *d_n_points,
                                            uint32_t *d_status);
/* One scan, HOST buffers: ranges / intensities as a published LaserScan holds them (count
 * beams, count <= max_samples_per_scan); xyzi: count * 4 floats. */
int32_t rplgpu_laserscan_to_cloud(rplgpu_handle_t h, const float *ranges,
                                  const float *intensities, uint32_t count,
                                  const rplgpu_params_t *p, float *xyzi, uint32_t *n_points);

/* ---- several sensors -> one fused cloud (first step) ------------------ */
/* Rigid transform of the clouds of B scans, in place: d_pose holds B row-major 3x4 matrices
 * [R | t] (tf2: target frame <- frame_id of scan b; the reference itself only ever broadcasts
 * the identity, src/rplidar_node.cpp:183-197).  Same addressing as rplgpu_cloud_msgs_dev
 * (d_scan_start = NULL: per-scan regions of out_stride points; else the arena).  float32,
 *   x' = ((r00*x + r01*y) + r02*z) + t0   (products, then sums left to right, no FMA),
 * y', z' likewise, intensity untouched. */
int32_t rplgpu_transform_clouds_dev(rplgpu_handle_t h, float *d_xyzi, uint32_t out_stride,
                                    const uint64_t *d_scan_start, const uint32_t *d_n_points,
                                    uint32_t B, const float *d_pose);
/* Motion de-skew of the plain cloud (E1 clip, E2 polar -> XYZ, optionally the E5 mask; not
 * with voxel_enable): d_motion holds per scan (vx, vy, wz, time_increment) — the sensor's planar
 * twist in its own frame at the first sample [m/s, m/s, rad/s] and the time between samples [s]
 * (LaserScan.time_increment, src/rplidar_node.cpp:637,668).  Sample i (its index in the scan as
 * handed in, i.e. acquisition order) was taken at tau = float(i) * time_increment; its point
 * moves to the sensor pose at the first sample:
 *   a = wz * tau;  a2 = a * a
 *   s = a * (1 + a2 * (-1/6 + a2 * (1/120)))            (Horner, every operation rounded to
 *   c = 1 + a2 * (-1/2 + a2 * (1/24 + a2 * (-1/720)))    float32 once, no FMA)
 *   x' = (c*x - s*y) + vx*tau;   y' = (s*x + c*y) + vy*tau
 * stated for |a| <= 0.5 rad.  These ARE the definition of E6 (the oracle evaluates the same
 * polynomials, so parity does not depend on their accuracy); against the true rotation s is short by
 * a^7 / 5040 and c by a^8 / 40320: 2e-8 / 7e-10 at 0.27 rad (a 10 Hz scan at 2.7 rad/s), 1.5e-6 / 1e-7
 * at 0.5 rad (round 6 corrects the "< 2e-8 at 0.5 rad" this comment used to claim).  Output as
 * rplgpu_cloud_batch_dev. */
int32_t rplgpu_cloud_deskew_batch_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                      uint32_t n_stride, const uint32_t *d_n_per_scan, uint32_t B,
                                      const rplgpu_params_t *p, const float *d_motion,
                                      float *d_xyzi, uint32_t out_stride, uint32_t *d_n_points,
                                      uint32_t *d_status);
/* E8 — ONE voxel grid for a GROUP of scans (row 4: de-skew in front of the voxel grid, and the
 * cross-sensor voxel grid).  Scans [g*group, (g+1)*group) of the batch — e.g. the 8 sensors of one
 * time step, or a single scan (group = 1) — are voxelised together: every kept sample (E1 clip,
 * E5 mask when ror_enable) gives (x, y) by E2; then, in float32, one rounding per operation:
 *   E6 de-skew with the scan's (vx, vy, wz, time_increment) from d_motion (NULL: none) —
 *     tau = float(i) * time_increment, formulas of rplgpu_cloud_deskew_batch_dev above;
 *   the scan's planar pose from d_pose2d (NULL: identity), 6 floats per scan
 *     (r00 r01 tx r10 r11 ty):  x'' = (r00*x' + r01*y') + tx;  y'' = (r10*x' + r11*y') + ty;
 * and the E4 voxel grid (leaf p->voxel_leaf) runs over ALL points of the group: one output point
 * per occupied cell = centroid (fp64 sum / count, rounded to float), mean intensity, z = 0, cells
 * in (iy, ix) order.  Outputs as rplgpu_cloud_arena_dev, indexed by GROUP: d_group_start[g],
 * d_n_points[g], d_status[g] for g < ceil(B / group); *d_cursor = all points.
 * The raw scans are streamed once; a group's run records beyond the on-chip queue go through the
 * handle's record store (L2).  The reference publishes time_increment / scan_time
 * (src/rplidar_node.cpp:627,637-638) and an identity transform (:183-197); nothing there
 * consumes them — this is the consumer. */
int32_t rplgpu_cloud_fused_voxel_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes,
                                     uint32_t n_stride, const uint32_t *d_n_per_scan, uint32_t B,
                                     uint32_t group, const rplgpu_params_t *p,
                                     const float *d_motion, const float *d_pose2d, float *d_arena,
                                     uint64_t arena_capacity, uint64_t *d_cursor,
                                     uint64_t *d_group_start, uint32_t *d_n_points,
                                     uint32_t *d_status);
/* Time alignment inside a group (row 4, the temporal side): the scans fused into one grid do not
 * start at the same instant — every sensor free-runs, and a node stamps its LaserScan with its own
 * start time (src/rplidar_node.cpp:620) and publishes time_increment / scan_time (:627,637-638).  d_t0 holds
 * per scan of the batch the time [s] of its FIRST sample relative to the instant the group is fused
 * at (scan stamp - fused stamp; negative: the scan started earlier).  While set, E6 — in
 * rplgpu_cloud_deskew_batch_dev and rplgpu_cloud_fused_voxel_dev, which then require d_motion —
 * moves every point to the sensor pose at the FUSED instant instead of the scan's first sample:
 *   tau = t0 + float(i) * time_increment      (product rounded to float32, then the sum)
 * and the formulas of rplgpu_cloud_deskew_batch_dev apply unchanged.  NULL (the default) switches it
 * off: tau = float(i) * time_increment, bit for bit as before.  The buffer is the caller's and must
 * stay valid until the launches that use it have completed.
 * DOMAIN: the sin / cos polynomials of E6 are stated for |a| = |wz * tau| <= 0.5 rad, and with an
 * offset tau covers [t0, t0 + n * time_increment]: the caller must keep |wz| * max(|t0|, |t0 + n *
 * time_increment|) <= 0.5 rad (a few scan periods of offset at a realistic yaw rate leave it: 1 rad/s
 * and t0 = 0.6 s already do).  Nothing checks this — beyond the domain the rotation is still the
 * degree-5 / -6 Taylor value (s short by 5.5e-6 at 0.6 rad, 2e-4 at 1 rad), and the oracle computes the same.
 * NOT consulted by: rplgpu_cloud_arena_dev, rplgpu_cloud_arena_xyi_dev, rplgpu_cloud_batch_dev,
 * rplgpu_scan_to_cloud[_msg] and the LaserScan entry points (no E6 there), nor by
 * rplgpu_cloud_fused_voxel_dev when d_motion is NULL together with NULL offsets (with offsets set and
 * d_motion NULL that call is refused: RPLGPU_ERR_INVALID_ARG). */
int32_t rplgpu_set_scan_time_offsets_dev(rplgpu_handle_t h, const float *d_t0);
/* The whole arena as ONE serialised PointCloud2 (the fused cloud of BASELINE config 5):
 * width = min(*d_total_points, arena_capacity) with d_total_points the arena cursor of
 * rplgpu_cloud_arena_dev — no host round trip.  *d_msg_len (device) = serialised size, or 0 +
 * RPLGPU_SCAN_OUT_TRUNCATED in *d_status when msg_capacity is too small. */
int32_t rplgpu_fused_cloud_msg_dev(rplgpu_handle_t h, const float *d_arena,
                                   const uint64_t *d_total_points, uint64_t arena_capacity,
                                   const char *frame_id, rplgpu_stamp_t stamp, uint8_t *d_msg,
                                   uint64_t msg_capacity, uint64_t *d_msg_len, uint32_t *d_status);

/* ---- E9: several sensors -> ONE LaserScan in the common frame (row 4, the scan merger) ---------
 * What Nav2 costmaps, AMCL and slam_toolbox read: a virtual scan of `count` beams over
 * [angle_min, angle_max) that keeps, per beam, the nearest return of every sensor of a time step.
 *   inc = (float)(((double)angle_max - (double)angle_min) / (double)count)   (Mode A's :634, any span)
 * A spec is refused (RPLGPU_ERR_INVALID_ARG) when a value is not finite, count is 0 or above
 * RPLGPU_MAX_MERGE_BEAMS, inc <= 0 or inc > (float)(pi / 2), angle_max - angle_min (fp64) > 2 pi (1 + 2^-20),
 * or !(0 <= range_min < range_max). */
#define RPLGPU_MAX_MERGE_BEAMS 16384u
typedef struct rplgpu_scan_merge {
  float angle_min, angle_max; /* the virtual scan covers [angle_min, angle_max) in the common frame */
  uint32_t count;             /* beams, 1 .. RPLGPU_MAX_MERGE_BEAMS */
  float range_min, range_max; /* range gate in the common frame; also LaserScan.range_min / range_max */
  float scan_time;            /* LaserScan.scan_time of the merged message */
} rplgpu_scan_merge_t;
/* Host only (no handle, no device): validates the spec, writes inc and the edge table
 *   phi_k = (double)angle_min + (double)k * (double)inc,  e_k = ((float)cos(phi_k), (float)sin(phi_k)),
 * k = 0 .. count, as edges[2k], edges[2k + 1] (2 * (count + 1) floats; either pointer may be NULL).
 * The device path builds its table with this very function. */
int32_t rplgpu_scan_merge_edges(const rplgpu_scan_merge_t *m, float *edges, float *inc);
/* E9 for groups of scans: scans [g*group, (g+1)*group) of the batch (group clamped to B as in E8) give
 * merged scan g.  Every sample E1 keeps (and E5 too with p->ror_enable) becomes (x, y) by exactly the
 * float32 operations of rplgpu_cloud_fused_voxel_dev: E2 (p->inverted honoured), E6 de-skew from d_motion
 * with the offsets of rplgpu_set_scan_time_offsets_dev (offsets set and d_motion NULL: refused), the planar
 * pose from d_pose2d.  voxel_enable and scan_processing are ignored.  Then
 *   r2 = RN(RN(x*x) + RN(y*y)) (no FMA), range = sqrtf(r2) correctly rounded;
 *   the point takes part iff range_min <= range <= range_max;
 *   cross_k = (double)e_k.x * (double)y - (double)e_k.y * (double)x  (exact products, one rounding: exact sign);
 *   its beam is the SMALLEST k in [0, count) with cross_k >= 0 && cross_k+1 < 0; none: dropped
 *   (neighbouring beams share an edge, so the beams tile without gaps; on a full circle the sliver between
 *   e_count and e_0 goes to the smaller k).
 * Per beam the point with the smallest r2 wins, ties to the smallest (slot in group, sample index):
 *   ranges[k] = sqrtf(r2), intensities[k] = its E3 intensity; an empty beam holds +inf and 0.
 * Merged scan g at d_ranges + g*count, d_intensities + g*count; d_beams_hit[g] = its non-empty beams;
 * d_status[g] (optional) = RPLGPU_SCAN_OUT_TRUNCATED when a scan of the group was longer than n_stride.
 * Asynchronous on the handle's stream; the argument and capacity checks of rplgpu_cloud_fused_voxel_dev. */
int32_t rplgpu_merge_scans_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                               const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                               const rplgpu_scan_merge_t *m, float *d_ranges, float *d_intensities,
                               uint32_t *d_beams_hit, uint32_t *d_status);
/* G serialised LaserScans of merged scans (d_ranges / d_intensities as rplgpu_merge_scans_dev wrote them):
 * angle_min, angle_max, range_min, range_max and scan_time of `m`, angle_increment = inc,
 * time_increment = 0 (the points are already moved to one instant), always count beams.  Message g at
 * d_msgs + g*msg_stride (a multiple of 4), its length in d_msg_len[g]; 0 + RPLGPU_SCAN_OUT_TRUNCATED in
 * d_status[g] (optional) when msg_stride is too small.  d_stamps: G stamps (device). */
int32_t rplgpu_merged_laserscan_msgs_dev(rplgpu_handle_t h, const float *d_ranges,
                                         const float *d_intensities, uint32_t G,
                                         const rplgpu_scan_merge_t *m, const char *frame_id,
                                         const rplgpu_stamp_t *d_stamps, uint8_t *d_msgs,
                                         uint32_t msg_stride, uint32_t *d_msg_len, uint32_t *d_status);

/* ---- E10: scan-shadow and speckle filters on LaserScan arrays (the `laser_filters` staples) ------
 * A stage between the LaserScan producers (rplgpu_laserscan_batch_dev, rplgpu_ascend_laserscan_batch_dev,
 * rplgpu_merge_scans_dev) and their consumers (the message functions, E7): same layout in and out.
 * Nothing in the reference filters a scan, so these rules ARE the definition (parity unpinned, as E5-E9).
 *
 * A beam is finite when its range is a finite float.  With circular = 1 indices are taken modulo count
 * and W and N are each limited to (count - 1) / 2, so no beam meets itself; with circular = 0 indices
 * outside [0, count) do not exist.
 * SHADOW, detection.  Beam i finite with range r1; neighbour j = i +- y, 1 <= y <= W, finite with range r2:
 *   delta = (float)y * inc; the pair is examined only while delta <= 0.5f;
 *   s, c = the E6 polynomials (rplgpu_cloud_deskew_batch_dev above) at a = delta, float32, no FMA;
 *   a = r2 * s;  b = r1 - r2 * c            (float32: the product, then the difference)
 *   it is a shadow pair iff (double)cmin*(double)a - (double)smin*(double)b < 0    (atan2(a, b) < min_angle)
 *                        or (double)cmax*(double)a - (double)smax*(double)b > 0    (atan2(a, b) > max_angle)
 *   (exact products, one rounding: exact sign; no angle is ever computed).  Beam i is DETECTED when it has
 *   at least one shadow pair.
 * SHADOW, removal.  Beam k is removed iff it is finite and some detected beam i with |i - k| <= N has
 *   r[i] < r[k]: only the farther points go, and every decision reads the input ranges.
 * SPECKLE, on the ranges after shadow removal (removed beams are not finite).  Beams k and k + 1 are
 *   linked iff both are finite and fabsf(r[k+1] - r[k]) <= D (float32 difference); a run is a maximal
 *   chain of linked beams; with circular the link count-1 -> 0 exists and a run that closes the circle has
 *   count beams.  A finite beam is removed iff its run has fewer than L beams.  (A run's length is its true
 *   length: an implementation may stop counting on either side of a beam after min(L, count) - 1 links and
 *   take min(left + right + 1, count), which decides the same.)
 * A removed beam's range is the quiet NaN 0x7FC00000 (what laser_filters leaves; E7 drops it); every
 * other beam below count keeps its input bits (+inf empty bins and NaNs included); intensities are a bit
 * copy; beams at or beyond count are not written.  Both filters off: a plain copy. */
#define RPLGPU_MAX_FILTER_WINDOW 64u
typedef struct rplgpu_scan_filter {
  int32_t  shadow_enable;
  float    shadow_min_angle, shadow_max_angle; /* rad; 0 < min < pi/2 < max < pi (defaults 10 deg, 170 deg) */
  uint32_t shadow_window;     /* W: 1 .. RPLGPU_MAX_FILTER_WINDOW (default 2) */
  uint32_t shadow_neighbors;  /* N: 0 .. RPLGPU_MAX_FILTER_WINDOW (default 1) */
  int32_t  speckle_enable;
  float    speckle_max_range_difference; /* D >= 0, metres (default 0.05) */
  uint32_t speckle_min_run;   /* L: 1 .. RPLGPU_MAX_FILTER_WINDOW (default 4) */
  int32_t  circular;          /* beams count-1 and 0 are neighbours (default 1: full-circle scans) */
} rplgpu_scan_filter_t;

/* Both filters on, with the defaults named above. */
void rplgpu_default_scan_filter(rplgpu_scan_filter_t *f);
/* Host only (no handle, no device): validates f — finite values and the ranges above (angles compared
 * in fp64), whether or not a filter is enabled; dirs (may be NULL) receives
 *   cmin, smin, cmax, smax = (float)cos((double)min_angle), (float)sin((double)min_angle), ... max_angle.
 * The device path uses this function. */
int32_t rplgpu_scan_filter_check(const rplgpu_scan_filter_t *f, float dirs[4]);

/* The outputs of rplgpu_laserscan_batch_dev / rplgpu_ascend_laserscan_batch_dev, filtered: scan b has
 * count = min(d_beam_count[b], n_stride) beams at d_ranges + b*n_stride and, computed on the device as
 * the reference does (and E7),  inc = (float)(2 pi / (double)count) with p->scan_processing (Mode A, :635),
 * else (float)(2 pi / (double)max(count - 1, 1)) (Mode B, :666-668); nothing else of *p is used.
 * d_removed (optional): 2 words per scan — beams the shadow filter removed, beams the speckle filter
 * removed in addition.  RPLGPU_ERR_INVALID_ARG for an output pointer equal to its input, a missing
 * required pointer, n_stride = 0 or an invalid filter.  Only equal pointers are refused: output buffers that
 * overlap the inputs in any other way are the caller's error and give undefined results (a tile reads
 * its neighbours' beams while other tiles write).  Asynchronous on the handle's stream. */
int32_t rplgpu_filter_laserscan_batch_dev(rplgpu_handle_t h, const float *d_ranges, const float *d_intensities,
                                          uint32_t n_stride, const uint32_t *d_beam_count, uint32_t B,
                                          const rplgpu_params_t *p, const rplgpu_scan_filter_t *f,
                                          float *d_ranges_out, float *d_intensities_out, uint32_t *d_removed);
/* The outputs of rplgpu_merge_scans_dev, filtered: G scans of m->count beams, m->count apart, inc from
 * rplgpu_scan_merge_edges; f->circular is honoured as given (set it only for a full-circle spec). */
int32_t rplgpu_filter_merged_scans_dev(rplgpu_handle_t h, const float *d_ranges, const float *d_intensities,
                                       uint32_t G, const rplgpu_scan_merge_t *m, const rplgpu_scan_filter_t *f,
                                       float *d_ranges_out, float *d_intensities_out, uint32_t *d_removed);
/* One scan, HOST buffers: count <= max_samples_per_scan beams (else RPLGPU_ERR_CAPACITY) with the given
 * angle_increment (finite, > 0); removed (optional) as above.  Returns when the results are in place. */
int32_t rplgpu_filter_laserscan(rplgpu_handle_t h, const float *ranges, const float *intensities, uint32_t count,
                                float angle_increment, const rplgpu_scan_filter_t *f, float *ranges_out,
                                float *intensities_out, uint32_t removed[2]);

/* ---- E11: one ray-cast occupancy grid per group of scans (row 4; the costmap obstacle layer's mark-and-clear) --
 * What Nav2 costmaps, AMCL and slam_toolbox do first with a time step's scans: every beam is traced from
 * ITS sensor through the grid, the cells it passes are cleared and the cell it ends in is marked.  E8 gives
 * occupied cells only and E9 beams that all start at the base origin; here every ray starts where its own
 * sensor stands.  Nothing in the reference builds a grid, so these rules ARE the definition (parity unpinned,
 * as E5-E10). */
#define RPLGPU_MAX_OCC_DIM   4096u
#define RPLGPU_MAX_OCC_STEPS 8192u
typedef struct rplgpu_occ_grid {
  float    origin_x, origin_y;  /* common-frame position of the lower-left corner of cell (0, 0) */
  float    resolution;          /* metres per cell, > 0 */
  uint32_t width, height;       /* cells, 1 .. RPLGPU_MAX_OCC_DIM each */
  float    range_min;           /* returns nearer to their sensor than this are ignored (robot body), >= 0 */
  float    obstacle_max;        /* a return marks its cell iff d <= obstacle_max */
  float    raytrace_max;        /* rays clear up to this distance; longer rays are cut here */
} rplgpu_occ_grid_t;
/* resolution 0.05 m, 1024 x 1024 cells, origin (-25.6, -25.6), range_min 0, obstacle_max 25, raytrace_max 30 */
void rplgpu_default_occ_grid(rplgpu_occ_grid_t *grid);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for a value that is not finite, resolution <= 0,
 * a dimension of 0 or above RPLGPU_MAX_OCC_DIM, !(0 <= range_min < obstacle_max <= raytrace_max), or
 * (double)raytrace_max / (double)resolution > RPLGPU_MAX_OCC_STEPS (which bounds every ray walk, however
 * it is walked).  The device path uses this function. */
int32_t rplgpu_occ_grid_check(const rplgpu_occ_grid_t *grid);
/* POINTS: those of rplgpu_merge_scans_dev, from the same float32 operations — E1 (E5 too with p->ror_enable),
 * E2 (p->inverted honoured), E6 de-skew from d_motion with the offsets of rplgpu_set_scan_time_offsets_dev
 * (offsets set and d_motion NULL: refused), the planar pose.  voxel_enable and scan_processing are ignored.
 * The sensor of scan sc stands at (sx, sy) = (d_pose2d[6 sc + 2], d_pose2d[6 sc + 5]) — where it is at the
 * fused instant, to which E6 has moved every point; (0, 0) without d_pose2d.
 * CELL of a position (x, y), float32, no FMA, IEEE divides:
 *   u = (x - origin_x) / resolution;  fu = floorf(u);  fv likewise from y;
 *   the position has NO cell when fu or fv is NaN or has magnitude >= 1048576 (the cell-range case);
 *   otherwise its cell is (cx, cy) = ((int)fu, (int)fv), which may lie outside the grid.
 * PER POINT, dx = x - sx, dy = y - sy:
 *   d = sqrtf(RN(RN(dx*dx) + RN(dy*dy)));  the point is ignored when d is not finite or d < range_min
 *   (so a NaN or Inf point, e.g. from a NaN in d_motion, is ignored HERE and never sets a status bit);
 *   d <= raytrace_max: the end position is (x, y) and the ray is WHOLE;
 *   else t = raytrace_max / d, the end position is (sx + dx * t, sy + dy * t) (one product, then one sum
 *   per coordinate) and the ray is CUT;
 *   a ray whose sensor position or end position has no cell is dropped and sets RPLGPU_SCAN_CELL_RANGE in
 *   d_status[g].
 * THE WALK, all-integer Bresenham from the sensor cell (x0, y0) to the end cell (x1, y1):
 *   ax = |x1 - x0|, ay = |y1 - y0|, stepx = sign(x1 - x0), stepy = sign(y1 - y0), err = ax - ay;
 *   visit (x0, y0); while the current cell is not (x1, y1): e2 = 2 err, and with this one e2
 *     if (e2 > -ay) { err -= ay; x += stepx; }   if (e2 < ax) { err += ax; y += stepy; }   visit the cell.
 *   Visits outside [0, width) x [0, height) do nothing.
 * A whole ray CLEARS every visited cell except its end cell and MARKS the end cell iff d <= obstacle_max.  A
 * cut ray clears every visited cell, the end cell included, and marks nothing.
 * RESULT for group g (scans [g*group, (g+1)*group), group clamped to B as in E8), int8 in
 * nav_msgs/OccupancyGrid row-major order at index cy * width + cx, at d_grid + g * grid_stride:
 *   100 for a cell any ray marks;  0 for a cell some ray clears and none marks;  otherwise the cell's value
 *   in d_prev + g * grid_stride (group g's previous grid, same layout), or -1 when d_prev is NULL.
 * Marks beat clears and both beat history, so the result depends on no order.
 * d_cells (optional): per group the number of result cells that are 0, 100 and -1 (3 words).  d_status[g]
 * (optional): RPLGPU_SCAN_OUT_TRUNCATED when a scan of the group was longer than n_stride (as E9), and
 * RPLGPU_SCAN_CELL_RANGE as above.
 * grid_stride >= width * height and a multiple of 4, d_grid 4-byte aligned (the walk uses 32-bit atomics on
 * the output itself: the grid is its own scratch, bytes at and beyond width * height of a group are left
 * alone).  d_prev == d_grid is refused; any other overlap is the caller's error.  The argument and capacity
 * checks of rplgpu_cloud_fused_voxel_dev.  Asynchronous on the handle's stream. */
int32_t rplgpu_occupancy_grid_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                  const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                                  const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                                  const rplgpu_occ_grid_t *grid, const int8_t *d_prev, int8_t *d_grid,
                                  uint64_t grid_stride, uint32_t *d_cells, uint32_t *d_status);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp): n_scans <= max_batch scans of n_per_scan[i]
 * samples, n_stride apart; motion / pose2d / prev may be NULL; t0 (NULL: none) are the scans' time offsets
 * for this call only; grid_out: width * height bytes; cells (optional): 3 words; status (optional): 1 word.
 * Allocates its device buffers per call and returns when the result is in place. */
int32_t rplgpu_occupancy_grid(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                              const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                              const float *motion, const float *pose2d, const float *t0,
                              const rplgpu_occ_grid_t *grid, const int8_t *prev, int8_t *grid_out,
                              uint32_t cells[3], uint32_t *status);
/* Byte offsets inside one serialised nav_msgs/OccupancyGrid = Header, MapMetaData info { Time map_load_time,
 * float32 resolution, uint32 width, height, Pose origin { float64 position x y z, orientation x y z w } },
 * int8[] data.  float64 is aligned to 8 counted from the byte after the encapsulation header. */
typedef struct rplgpu_occupancy_layout {
  uint32_t map_load_time_off; /* int32 sec, uint32 nanosec */
  uint32_t resolution_off;    /* float32 resolution; uint32 width and height follow */
  uint32_t origin_off;        /* 7 float64 */
  uint32_t data_len_off;      /* uint32 data.size() = width * height */
  uint32_t data_off;          /* data[0]; a multiple of 4 */
  uint32_t total_len;
} rplgpu_occupancy_layout_t;
int32_t rplgpu_msg_occupancy_layout(size_t frame_id_len, uint32_t width, uint32_t height,
                                    rplgpu_occupancy_layout_t *out);
/* G serialised OccupancyGrids of the grids rplgpu_occupancy_grid_dev wrote: header stamp and
 * info.map_load_time = d_stamps[g], resolution / width / height of `grid`, origin position (origin_x,
 * origin_y, 0) and orientation (0, 0, 0, 1).  Message g at d_msgs + g*msg_stride (a multiple of 4), its
 * length in d_msg_len[g]; 0 + RPLGPU_SCAN_OUT_TRUNCATED in d_status[g] (optional) when msg_stride is too small. */
int32_t rplgpu_occupancy_grid_msgs_dev(rplgpu_handle_t h, const int8_t *d_grid, uint64_t grid_stride, uint32_t G,
                                       const rplgpu_occ_grid_t *grid, const char *frame_id,
                                       const rplgpu_stamp_t *d_stamps, uint8_t *d_msgs, uint32_t msg_stride,
                                       uint32_t *d_msg_len, uint32_t *d_status);

/* ---- E12: the grids of E11 inflated into costmaps (row f7; the costmap inflation layer) ----------------------
 * What every consumer of an obstacle grid runs first (Nav2 planners and controllers, anything that checks a
 * footprint): each lethal cell is grown by the robot's inscribed radius and a decaying cost is laid around
 * it, out to the inflation radius.  On the CPU a priority-queue flood over the whole grid per update; here
 * one data-parallel pass over the bytes E11 left in device memory, on the same stream.  Nothing in the
 * reference inflates a grid, so these rules ARE the definition (parity unpinned, as E5-E11). */
#define RPLGPU_MAX_INFLATION_CELLS 64u
typedef struct rplgpu_inflation {
  float    inscribed_radius;     /* m, >= 0 */
  float    inflation_radius;     /* m, >= inscribed_radius */
  float    cost_scaling_factor;  /* 1/m, >= 0 */
  uint32_t inflate_unknown;      /* 0 / 1 */
} rplgpu_inflation_t;
/* inscribed_radius 0.22 m, inflation_radius 0.55 m, cost_scaling_factor 3.0 / m, inflate_unknown 0 */
void rplgpu_default_inflation(rplgpu_inflation_t *f);
/* Host only (no handle, no device).  Rc = (uint32_t)ceil((double)inflation_radius / (double)resolution), the
 * reach in cells, every float widened to double first: 12, not 11, for the defaults at 0.05 m, because
 * (double)0.55f / (double)0.05f > 11.  RPLGPU_ERR_INVALID_ARG for a value that is not finite, a negative
 * value, resolution <= 0, inflation_radius < inscribed_radius, inflate_unknown > 1 or
 * Rc > RPLGPU_MAX_INFLATION_CELLS. */
int32_t rplgpu_inflation_check(const rplgpu_inflation_t *f, float resolution);
/* Host only.  The COST TABLE of a checked spec, Rc * Rc + 1 bytes indexed by the squared cell distance k:
 *   table[0] = 100;  for k >= 1, d = sqrt((double)k) * (double)resolution:
 *   d <= (double)inscribed_radius: 99;  otherwise
 *   (uint8_t)(int)(98.0 * exp(-(double)cost_scaling_factor * (d - (double)inscribed_radius))), truncated: 0 .. 98.
 * The scale in which Nav2 publishes a costmap as an OccupancyGrid (100 lethal, 99 inscribed, 1 .. 98 the
 * rest), so the result goes straight into rplgpu_occupancy_grid_msgs_dev.  The table is non-increasing in k.
 * *rc_out (optional) = Rc.  RPLGPU_ERR_CAPACITY when table_cap < Rc * Rc + 1 (rc_out is set all the same),
 * RPLGPU_ERR_INVALID_ARG for a spec the check refuses. */
int32_t rplgpu_inflation_table(const rplgpu_inflation_t *f, float resolution, uint8_t *table, uint32_t table_cap,
                               uint32_t *rc_out);
/* PER CELL c of grid g, input byte v (int8) at d_in + g * in_stride + cy * width + cx:
 *   D2(c) = the minimum of dx*dx + dy*dy over all cells q of the SAME grid whose input is >= 100 (cells
 *   outside [0, width) x [0, height) hold nothing);
 *   cost = d_table[D2] when such a q exists and D2 <= rc * rc, otherwise 0;
 *   v >= 100: 100;   0 <= v <= 99: max(v, cost) (the history values E11 copied from d_prev survive when
 *   they are larger);   v < 0 (unknown): cost when (inflate_unknown ? cost > 0 : cost >= 99), otherwise -1.
 * The result at d_out + g * out_stride + cy * width + cx is a function of the input set alone: no order, no
 * ties.  d_table: rc * rc + 1 bytes in DEVICE memory that the caller uploads once (inflation parameters are
 * node parameters); a table the caller made itself is allowed as long as it is non-increasing in k and holds
 * values 0 .. 100 (the kernel may stop looking once no nearer lethal cell can exist).  Nothing is stored on the
 * handle and nothing is copied from host memory.  d_cells (optional): per grid the number of result cells that
 * are 100, 99, 1 .. 98 and -1 (4 words; cleared on the stream by the call).
 * RPLGPU_ERR_INVALID_ARG for d_in == d_out (any other overlap is the caller's error), rc >
 * RPLGPU_MAX_INFLATION_CELLS, inflate_unknown > 1, a dimension of 0 or above RPLGPU_MAX_OCC_DIM, a stride
 * < width * height or not a multiple of 4, a pointer that is not 4-byte aligned (the E11 rules: the two calls
 * chain), G == 0 or a NULL d_in / d_out / d_table.  d_in is read in whole 32-bit words (the up to 3 bytes
 * behind the last cell of a grid, inside in_stride, are read and ignored); bytes of d_out at and beyond
 * width * height of a grid are never changed.  Asynchronous on the handle's stream. */
int32_t rplgpu_inflate_grids_dev(rplgpu_handle_t h, const int8_t *d_in, uint64_t in_stride, int8_t *d_out,
                                 uint64_t out_stride, uint32_t G, uint32_t width, uint32_t height,
                                 const uint8_t *d_table, uint32_t rc, uint32_t inflate_unknown, uint32_t *d_cells);
/* ONE grid, HOST buffers (the node-side door, rplgpu_host.hpp): checks the spec, builds and uploads the table,
 * allocates its device buffers per call and returns when `out` (width * height bytes, not `in`) is in place;
 * cells (optional): 4 words as above. */
int32_t rplgpu_inflate_grid(rplgpu_handle_t h, const int8_t *in, uint32_t width, uint32_t height, float resolution,
                            const rplgpu_inflation_t *f, int8_t *out, uint32_t cells[4]);

/* ---- E13: a time step's scans matched to a likelihood field (row 4; the localisation side's scan matcher) ------
 * What AMCL and slam_toolbox, the second and third reader of everything above, do with a time step's scans and a
 * map: correlative scan matching (Olson's real-time correlative matcher, Cartographer's
 * RealTimeCorrelativeScanMatcher2D, Karto's CorrelateScan, the sensor half of a likelihood-field model).  The
 * points are laid over a field at every pose of a small search window, the field values under them are added up
 * and the best pose is kept: points x rotations x shifts look-ups per time step.  The field is any int8 grid in
 * the E11 layout; rplgpu_inflate_grids_dev with a caller-made non-increasing table turns an E11 grid into exactly
 * a likelihood field table[D2].  Nothing in the reference matches scans, so these rules ARE the definition (parity
 * unpinned, as E5-E12).  After the float32 rotation everything is integers: the result depends on no order. */
#define RPLGPU_MAX_MATCH_SHIFT 32u   /* cells, per axis */
#define RPLGPU_MAX_MATCH_ROT   64u   /* rotation steps either side of 0 */
typedef struct rplgpu_scan_match {
  float    origin_x, origin_y;   /* the field's grid: as rplgpu_occ_grid_t */
  float    resolution;
  uint32_t width, height;        /* 1 .. RPLGPU_MAX_OCC_DIM */
  uint32_t shift_x, shift_y;     /* Tx, Ty: candidates shift by i in [-Tx, Tx], j in [-Ty, Ty] whole cells; 0 .. RPLGPU_MAX_MATCH_SHIFT */
  uint32_t rot_steps;            /* K: candidates rotate by k * rot_step, k in [-K, K]; 0 .. RPLGPU_MAX_MATCH_ROT */
  float    rot_step;             /* rad, > 0 when K > 0; K * rot_step <= pi/2 (fp64) */
} rplgpu_scan_match_t;
/* E11's default grid (0.05 m, 1024 x 1024 cells, origin (-25.6, -25.6)), Tx = Ty = 6, K = 10,
 * rot_step = (float)(0.25 * pi / 180) */
void rplgpu_default_scan_match(rplgpu_scan_match_t *m);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for a value that is not finite, resolution <= 0, a
 * dimension of 0 or above RPLGPU_MAX_OCC_DIM, a shift above RPLGPU_MAX_MATCH_SHIFT, K above RPLGPU_MAX_MATCH_ROT,
 * or K > 0 with rot_step <= 0 or (double)K * (double)rot_step > pi/2 (M_PI / 2 as a double).  With K = 0
 * rot_step only has to be finite.  The device path uses this function. */
int32_t rplgpu_scan_match_check(const rplgpu_scan_match_t *m);
/* Host only.  The ROTATION TABLE of a checked spec, 2 * (2K + 1) floats:
 *   cs[2 (k + K)], cs[2 (k + K) + 1] = (float)cos((double)k * (double)rot_step), (float)sin(the same), k = -K .. K;
 * entry k = 0 is exactly (1, 0).  The device path builds its table with this very function. */
int32_t rplgpu_scan_match_rotations(const rplgpu_scan_match_t *m, float *cs);
/* Host only.  (2K + 1) * (2Ty + 1) * (2Tx + 1), the words of one group's score volume; 0 for a spec the check
 * refuses. */
uint32_t rplgpu_scan_match_volume(const rplgpu_scan_match_t *m);
/* POINTS: those of rplgpu_occupancy_grid_dev, from the same float32 operations — E1 (E5 too with p->ror_enable),
 * E2 (p->inverted honoured), E6 de-skew from d_motion with the offsets of rplgpu_set_scan_time_offsets_dev
 * (offsets set and d_motion NULL: refused), the planar pose d_pose2d — here the caller's PRIOR for each sensor in
 * the field's frame.  Groups as E8 / E9 / E11 (group clamped to B).  A point whose x or y is not finite is
 * ignored and sets no status bit.  (px, py) = (d_pivot[2g], d_pivot[2g + 1]) is the point about which group g's
 * candidates rotate, the base's prior position; d_pivot NULL: (0, 0).
 * CANDIDATE (k, j, i), k in [-K, K], j in [-Ty, Ty], i in [-Tx, Tx]; per point (x, y), float32, no FMA, (c, s)
 * the rotation table's entry k:
 *   qx = x - px;  qy = y - py;
 *   rx = (c*qx - s*qy) + px;  ry = (s*qx + c*qy) + py      (each product rounded, then the difference, then the sum)
 *   (cx, cy) = the E11 CELL of (rx, ry) in the spec's grid (same rule, same IEEE divides);  a rotated position
 *   with no cell contributes nothing to rotation k and sets RPLGPU_SCAN_CELL_RANGE in d_status[g];
 *   the candidate's cell for the point is (cx + i, cy + j): shifts are whole cells;
 *   f = max((int8)d_field[g_f * field_stride + (cy + j) * width + (cx + i)], 0);  a cell outside
 *   [0, width) x [0, height) gives 0, and so does an unknown (negative) byte;  g_f = g when field_per_group is
 *   not 0, else 0 (one map serves every time step).
 * SCORE: score[g][k][j][i] = the sum of f over the group's points, uint32, at
 *   d_scores + g * score_stride + ((k + K) * (2Ty + 1) + (j + Ty)) * (2Tx + 1) + (i + Tx);
 * score_stride >= the volume size, in words; words at and beyond the volume of a group are never changed.  With
 * group * n_stride <= 2^24 (otherwise RPLGPU_ERR_INVALID_ARG) 127 * points < 2^32: no sum wraps.
 * BEST: eight 32-bit words per group at d_best + 8 g:
 *   0      the largest score of the group's volume
 *   1 - 3  k, j, i (int32) of the candidate that has it;  among candidates with that score, in this order: the
 *          smallest i*i + j*j, the smallest |k|, the smallest k, the smallest j, the smallest i — the prior wins
 *          a tie and a uniform field returns (0, 0, 0)
 *   4      the number of the group's finite points
 *   5      the score of candidate (0, 0, 0)
 *   6      the number of candidates whose score equals the best (1: unambiguous)
 *   7      0
 * A group without points has score 0 everywhere and best 0 at (0, 0, 0).
 * APPLYING IT: the correction is the rigid motion "rotate by k * rot_step about (px, py), then translate by
 * (i, j) * resolution", composed in front of every d_pose2d of the group: with (c, s) the table's entry k,
 *   R' = [c -s; s c] R;   t' = [c -s; s c] (t - pivot) + pivot + (i, j) * resolution
 * is the pose the next rplgpu_occupancy_grid_dev call takes.
 * d_field 4-byte aligned, field_stride >= width * height and a multiple of 4 (the E11 / E12 rules: the three
 * calls chain); the field is only read, and only its width * height bytes per grid.  d_scores and d_best are
 * required and 4-byte aligned; the volume is the call's own scratch (as E11's grid is): nothing is stored on the
 * handle, nothing is copied from pageable memory.  d_status[g] (optional): RPLGPU_SCAN_OUT_TRUNCATED as E9 / E11
 * and RPLGPU_SCAN_CELL_RANGE as above.  The argument and capacity checks of rplgpu_cloud_fused_voxel_dev;
 * RPLGPU_ERR_INVALID_ARG also for a spec the check refuses, group = 0, a missing d_field / d_scores / d_best, the
 * alignment and stride rules above, score_stride below the volume size, and offsets set with d_motion NULL.  A
 * refused call changes no output.  Asynchronous on the handle's stream. */
int32_t rplgpu_match_scans_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const float *d_pivot,
                               const rplgpu_scan_match_t *m, const int8_t *d_field, uint64_t field_stride,
                               uint32_t field_per_group, uint32_t *d_scores, uint64_t score_stride,
                               uint32_t *d_best, uint32_t *d_status);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp): n_scans <= max_batch scans as
 * rplgpu_occupancy_grid takes them; pivot: 2 floats or NULL; field: width * height bytes; scores_out (optional):
 * the volume, rplgpu_scan_match_volume words; best: 8 words; status (optional): 1 word.  Allocates its device
 * buffers per call and returns when the results are in place. */
int32_t rplgpu_match_scans(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                           const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                           const float *motion, const float *pose2d, const float *t0, const float *pivot,
                           const rplgpu_scan_match_t *m, const int8_t *field, uint32_t *scores_out,
                           uint32_t best[8], uint32_t *status);

/* ---- E14: time steps accumulated into a hit / miss map at matched poses (row 4; the mapping side's map update) ----
 * What slam_toolbox / Karto and every 2-D mapper among E11's readers keep: a map that MANY time steps have voted on,
 * each at its own (matched) pose.  E11 gives the grid of one time step and E13 matches against one field; here a
 * persistent count map sums the rays of every call, a cell rule turns the counts into the int8 grid E12 and E13
 * take, and a small kernel applies E13's eight result words to the poses, so match -> correct -> map -> field ->
 * match stays on one stream with no host round trip.  Counts are integer sums: the result depends on no order.
 * Nothing in the reference builds a map, so these rules ARE the definition (parity unpinned, as E5-E13).
 *
 * THE COUNT MAP: two uint32_t per cell in E11's row-major cell order, d_counts[2 * (cy * width + cx)] = misses,
 * [... + 1] = hits; 8-byte aligned, caller-owned and PERSISTENT: a call ADDS to what is there.  The caller zeroes
 * it (a plain hipMemsetAsync on the handle's stream); there is no prepare kernel and nothing is kept on the handle.
 * Words at and beyond 2 * width * height are never touched.
 *
 * rplgpu_map_update_dev: POINTS, the sensor position, CELL, the PER POINT rules (ignored / WHOLE / CUT / dropped
 * with RPLGPU_SCAN_CELL_RANGE) and THE WALK are those of rplgpu_occupancy_grid_dev, word for word; `grid` is
 * checked by rplgpu_occ_grid_check.  Every ray of ALL B scans goes into the ONE map; `group` (clamped to B as
 * elsewhere) only picks the status word d_status[g] (optional: RPLGPU_SCAN_OUT_TRUNCATED and RPLGPU_SCAN_CELL_RANGE
 * as E11; cleared on the stream by the call).  Per ray, in E11's words: every cell the ray CLEARS gets misses += 1,
 * the cell it MARKS gets hits += 1; so a whole ray beyond obstacle_max leaves its end cell alone, a cut ray counts
 * a miss in its end cell, and visits outside the grid do nothing.  Equal rays are NOT a set here: each counts.
 * Defined while every counter stays below 2^32; beyond that is the caller's error, like overlap.
 * On a zeroed map and for one group this makes one identity exact: hits > 0 <=> E11 says 100, and
 * hits == 0 && misses > 0 <=> E11 says 0.
 * The argument and capacity checks of rplgpu_occupancy_grid_dev, plus RPLGPU_ERR_INVALID_ARG for a d_counts that
 * is NULL or not 8-byte aligned.  A refused call changes nothing.  Asynchronous on the handle's stream. */
int32_t rplgpu_map_update_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                              const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                              const float *d_motion, const float *d_pose2d, const rplgpu_occ_grid_t *grid,
                              uint32_t *d_counts, uint32_t *d_status);
/* THE CELL RULE, per cell with h = hits, m = misses, n = h + m, every product and sum in 64 bits:
 *   n < min_observations: the cell's byte in d_prev (E11's layout), or -1 when d_prev is NULL;
 *   mode 0: 100 when h > 0 and 100 * h >= occupied_percent * n, else 0 (with occupied_percent 0 and
 *           min_observations 1 this is E11's "marks beat clears"; the defaults are Karto's min_pass_through and
 *           occupancy_threshold);
 *   mode 1: (200 * h + n) / (2 * n), integer division: the percentage of hits rounded half up, 0 .. 100. */
typedef struct rplgpu_map_rule {
  uint32_t min_observations;  /* >= 1 */
  uint32_t occupied_percent;  /* 0 .. 100 */
  uint32_t mode;              /* 0: three-valued, 1: percentage */
} rplgpu_map_rule_t;
/* min_observations 2, occupied_percent 10, mode 0 */
void rplgpu_default_map_rule(rplgpu_map_rule_t *rule);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, min_observations 0, occupied_percent above
 * 100 or a mode above 1.  The device path uses this function. */
int32_t rplgpu_map_rule_check(const rplgpu_map_rule_t *rule);
/* The count map as ONE int8 grid at d_grid in E11's layout and under E11's rules: d_grid 4-byte aligned,
 * grid_stride >= width * height and a multiple of 4, bytes at and beyond width * height never changed, d_prev ==
 * d_grid refused.  The result therefore goes straight into rplgpu_inflate_grids_dev,
 * rplgpu_occupancy_grid_msgs_dev, rplgpu_match_scans_dev and E11's own d_prev.  d_counts is only read.  d_cells
 * (optional): 4 words, the cells that are -1, 0, 100 and anything else; cleared on the stream by the call.
 * RPLGPU_ERR_INVALID_ARG for a rule the check refuses, a dimension of 0 or above RPLGPU_MAX_OCC_DIM, a missing or
 * misaligned d_counts (8 bytes) / d_grid / d_cells (4 bytes) and the stride rules above.  A refused call changes
 * nothing.  Asynchronous on the handle's stream. */
int32_t rplgpu_map_grid_dev(rplgpu_handle_t h, const uint32_t *d_counts, uint32_t width, uint32_t height,
                            const rplgpu_map_rule_t *rule, const int8_t *d_prev, int8_t *d_grid,
                            uint64_t grid_stride, uint32_t *d_cells);
/* E13's APPLYING IT on the device.  `m` is a checked rplgpu_scan_match_t: its resolution, K and rot_step are used,
 * and the rotation table is that of rplgpu_scan_match_rotations.  For scan sc of group g (group clamped to B),
 * (k, j, i) are words 1 - 3 of d_best + 8 g, (c, s) is the table's entry k and (px, py) = (d_pivot[2g],
 * d_pivot[2g + 1]), (0, 0) when d_pivot is NULL.  With the pose (r00 r01 tx r10 r11 ty) = d_pose2d_in + 6 sc
 * (NULL: identity poses), in float32, no FMA, each product rounded, then the difference or sum, in this order:
 *   r00' = c*r00 - s*r10;  r01' = c*r01 - s*r11;  r10' = s*r00 + c*r10;  r11' = s*r01 + c*r11;
 *   qx = tx - px;  qy = ty - py;
 *   tx' = ((c*qx - s*qy) + px) + (float)i * resolution;  ty' = ((s*qx + c*qy) + py) + (float)j * resolution
 * go to d_pose2d_out + 6 sc, and d_pivot_out (optional) gets (px + (float)i * resolution, py + (float)j *
 * resolution) for every group.  d_pose2d_out == d_pose2d_in is allowed (element-wise); d_pivot_out == d_pivot is
 * refused (every scan of a group reads the pivot).  flags bit 0: a group whose word 6 != 1 or whose word 0 == 0
 * (ambiguous or empty) keeps its poses and pivot unchanged, bit for bit; other bits must be 0.  A k outside
 * [-K, K] in d_best (a caller's error) is treated as that group's "keep": no table index leaves the table.
 * k = 0 is numerically the identity, not a bit identity: +0 + -0 can change a sign bit.
 * RPLGPU_ERR_INVALID_ARG for a spec the check refuses, group = 0, a missing d_best / d_pose2d_out, a pointer that
 * is not 4-byte aligned, flags above 1; RPLGPU_ERR_CAPACITY for B above the handle's max_batch.  A refused call
 * changes nothing.  Asynchronous on the handle's stream. */
int32_t rplgpu_apply_match_dev(rplgpu_handle_t h, const uint32_t *d_best, const rplgpu_scan_match_t *m,
                               const float *d_pivot, const float *d_pose2d_in, uint32_t B, uint32_t group,
                               uint32_t flags, float *d_pose2d_out, float *d_pivot_out);
/* ONE call's scans, HOST buffers (the node-side door, rplgpu_host.hpp): n_scans <= max_batch scans as
 * rplgpu_occupancy_grid takes them, all into the one map; counts: 2 * width * height words, read, added to and
 * written back; status (optional): 1 word.  Allocates its device buffers per call and returns when the counts are
 * in place: a door, not a hot path. */
int32_t rplgpu_map_update(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                          const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                          const float *motion, const float *pose2d, const float *t0, const rplgpu_occ_grid_t *grid,
                          uint32_t *counts, uint32_t *status);
/* HOST buffers: counts (2 * width * height words) through the rule into grid_out (width * height bytes); prev
 * (optional): width * height bytes; cells (optional): 4 words as above.  Allocates per call as well. */
int32_t rplgpu_map_grid(rplgpu_handle_t h, const uint32_t *counts, uint32_t width, uint32_t height,
                        const rplgpu_map_rule_t *rule, const int8_t *prev, int8_t *grid_out, uint32_t cells[4]);

/* ---- E15: a list of arbitrary poses weighed against a likelihood field (row 4; the localisation side's particle
 * weights) ----
 * What AMCL, the localisation reader among E11's three, does with a time step's scans and a map: a particle filter
 * asks E13's question not on a lattice around one prior but at a LIST of arbitrary poses, thousands of them,
 * anywhere on the map and at any heading.  Global localisation, recovery after a kidnap and seeding E13 with a
 * prior worth refining have the same shape.  The field is what E13 takes (rplgpu_inflate_grids_dev with a
 * caller-made table over an E11 or E14 grid), and the weight of a pose is E13's score: the sum of the field bytes
 * under the points.  That sum is AMCL's form too; the per-beam term is whatever monotone function the caller wrote
 * into the table.  poses x points look-ups per time step, all of them on the device, which is why nothing is
 * sub-sampled here.  Nothing in the reference weighs poses, so these rules ARE the definition (parity unpinned, as
 * E5-E14).  After the float32 pose transform everything is integers: the result depends on no order. */
#define RPLGPU_MAX_POSES 1048576u
typedef struct rplgpu_pose_score {
  float    origin_x, origin_y;   /* the field's grid: as rplgpu_occ_grid_t / rplgpu_scan_match_t */
  float    resolution;
  uint32_t width, height;        /* 1 .. RPLGPU_MAX_OCC_DIM */
} rplgpu_pose_score_t;
/* E11's default grid (0.05 m, 1024 x 1024 cells, origin (-25.6, -25.6)) */
void rplgpu_default_pose_score(rplgpu_pose_score_t *s);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, a value that is not finite, resolution <= 0
 * or a dimension of 0 or above RPLGPU_MAX_OCC_DIM.  The device path uses this function. */
int32_t rplgpu_pose_score_check(const rplgpu_pose_score_t *s);
/* Host only.  THE POSE LIST: n poses (x, y, theta), 3 doubles each at xyt, become 4 floats each at poses_out:
 *   ((float)cos(theta), (float)sin(theta), (float)x, (float)y),
 * cos and sin taken in fp64 and rounded once; theta == 0 gives exactly (1, 0).  A value that is not finite is
 * passed on as it rounds (the device defines such a pose, see below).  RPLGPU_ERR_INVALID_ARG for n above
 * RPLGPU_MAX_POSES or a NULL pointer with n > 0.  A caller may fill the four floats itself: any (c, s) is defined. */
int32_t rplgpu_pose_list(const double *xyt, uint32_t n, float *poses_out);
/* POINTS: those of rplgpu_occupancy_grid_dev, from the same float32 operations — E1 (E5 too with p->ror_enable),
 * E2 (p->inverted honoured), E6 de-skew from d_motion with the offsets of rplgpu_set_scan_time_offsets_dev
 * (offsets set and d_motion NULL: refused), the planar pose d_pose2d — here each sensor's MOUNT pose in the base
 * frame (E9's use of it; NULL: identity), so the points are in the base frame and a pose of the list is the base in
 * the field's frame.  Groups as E8 / E9 / E11 / E13 (group clamped to B).  A point whose x or y is not finite is
 * ignored and sets no status bit.
 * POSE q of group g, q in [0, P): (c, s, tx, ty) = the four floats at d_poses + g_p * pose_stride + 4 q, g_p = g
 * when poses_per_group is not 0, else 0 (one list serves every time step).  pose_stride is counted in floats, is
 * >= 4 P and a multiple of 4; d_poses is 16-byte aligned.  The device evaluates no trigonometric function and does
 * not check c*c + s*s = 1: any matrix [c -s; s c] is defined (a scale, the zero matrix).  Per point (x, y), float32,
 * no FMA, each product rounded, then the difference or sum, then the translation:
 *   rx = (c*x - s*y) + tx;   ry = (s*x + c*y) + ty
 *   (cx, cy) = the E11 CELL of (rx, ry) in the spec's grid (same rule, same IEEE divides);  a position with no cell
 *   (NaN or Inf, e.g. from a pose entry that is not finite, or a magnitude >= 1048576 cells) contributes nothing
 *   and sets RPLGPU_SCAN_CELL_RANGE in d_status[g];
 *   f = max((int8)d_field[g_f * field_stride + cy * width + cx], 0);  a cell outside [0, width) x [0, height)
 *   gives 0, and so does an unknown (negative) byte;  g_f = g when field_per_group is not 0, else 0.
 * WEIGHT: d_weights[g * weight_stride + q] = the sum of f over the group's points, uint32; weight_stride >= P, in
 * words; words at and beyond P of a group are never changed.  With group * n_stride <= 2^24 (otherwise
 * RPLGPU_ERR_INVALID_ARG, as E13) 127 * points < 2^32: no sum wraps.
 * RESULT: eight 32-bit words per group at d_result + 8 g:
 *   0      the largest weight of the group's list
 *   1      the smallest q that has it
 *   2      the number of poses that have it (1: unambiguous)
 *   3      the number of poses whose weight is 0
 *   4      the number of the group's finite points
 *   5      the weight of pose 0 (by convention the caller's odometry pose, as E13's word 5)
 *   6, 7   the sum of all P weights, low and high word (the filter's normaliser: P * 127 * 2^24 needs 64 bits)
 * A group without points has every weight 0: words 0 and 1 are 0, words 2 and 3 are P.
 * TWO IDENTITIES follow from the rules and hold independent kernels to each other:
 *   (a) with d_pivot NULL, candidate (k, 0, 0) of rplgpu_match_scans_dev sees exactly the positions of the pose
 *       (c_k, s_k, 0, 0) of rplgpu_scan_match_rotations: on the same points and field, with the table's 2K + 1
 *       entries as the list, weights[k + K] == score[k][0][0] for every k;
 *   (b) for an E11 spec with range_min 0 in which every kept point lies within obstacle_max of its sensor, the pose
 *       (1, 0, 0, 0) on the same d_pose2d has the weight  sum over cells of hits[cell] * max(field[cell], 0),  hits
 *       from rplgpu_map_update_dev on a zeroed map.
 * d_field 4-byte aligned, field_stride >= width * height and a multiple of 4 (E13's rules: the calls chain); the
 * field and the pose list are only read.  d_weights and d_result are required and 4-byte aligned; the weights are
 * the call's own scratch and result (as E13's volume is): nothing is stored on the handle, nothing is copied from
 * pageable memory.  d_status[g] (optional): RPLGPU_SCAN_OUT_TRUNCATED as E9 / E11 / E13 and RPLGPU_SCAN_CELL_RANGE
 * as above.  The argument and capacity checks of rplgpu_cloud_fused_voxel_dev; RPLGPU_ERR_INVALID_ARG also for a
 * spec the check refuses, group = 0, P = 0 or above RPLGPU_MAX_POSES, a missing or misaligned d_poses / d_field /
 * d_weights / d_result, a misaligned d_status, the stride rules above, and offsets set with d_motion NULL.  A
 * refused call changes no output.  Asynchronous on the handle's stream. */
int32_t rplgpu_score_poses_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const rplgpu_pose_score_t *s,
                               const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                               const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group,
                               uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_result, uint32_t *d_status);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp): n_scans <= max_batch scans as
 * rplgpu_occupancy_grid takes them; poses: 4 P floats as rplgpu_pose_list writes them; field: width * height
 * bytes; weights_out (optional): P words; result: 8 words; status (optional): 1 word.  Allocates its device
 * buffers per call and returns when the results are in place. */
int32_t rplgpu_score_poses(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                           const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                           const float *motion, const float *pose2d, const float *t0,
                           const rplgpu_pose_score_t *s, const float *poses, uint32_t P, const int8_t *field,
                           uint32_t *weights_out, uint32_t result[8], uint32_t *status);

/* ---- E16: a weighted pose list resampled and moved (row 4; the particle filter's step between two sensor updates)
 * ----
 * E15 ends with one uint32 weight per pose; the filter's next step draws a new list in proportion to the weights
 * and moves it by the odometry increment.  Here that step runs on the device, so that score -> resample -> score
 * queues on one stream without a read: the weights and the list of one rplgpu_score_poses_dev call go in, the list
 * for the next one comes out.  Nothing in the reference resamples, so these rules ARE the definition (parity
 * unpinned, as E5-E15).  The draw is integers and the move is fixed float32 operations: the result is byte-exact,
 * depends on no order and uses no atomic on a value.  The device owns no random generator: the caller supplies ONE
 * uint32 per group.
 *
 * INPUTS, per group g of G: P weights w[i] = d_weights[g * weight_stride + i] (E15's output layout: the calls
 * chain); P poses of four floats at d_poses + g_p * pose_stride + 4 i, g_p = g when poses_per_group is not 0, else 0
 * (pose_stride in floats, >= 4 P and a multiple of 4, d_poses 16-byte aligned: E15's rules); u = d_u[g], or 0 for
 * every group when d_u is NULL; M, the number of outputs.  1 <= P, M <= RPLGPU_MAX_POSES.
 * SYSTEMATIC (LOW-VARIANCE) RESAMPLING, all in integers:
 *   S = the sum of the w[i] (below 2^52);  C[i] = w[0] + ... + w[i];
 *   r = floor(u * S / 2^32) = u * (S >> 32) + ((u * (S & 0xffffffff)) >> 32), 64-bit; always r < S when S > 0;
 *   t_j = floor((j * S + r) / M) for output j in [0, M) = j * q + (j * rho + r) / M with S = q * M + rho (every term
 *   below 2^63; j * S itself does not fit);
 *   ancestor a[j] = the smallest i with C[i] > t_j.
 * It follows that t_j < S (every output has an ancestor), that a weight of 0 is never drawn, that pose i is drawn
 * floor or ceil of M * w[i] / S times and that a[] is non-decreasing.
 *   S = 0 (every pose dead): a[j] = j mod P and bit 0 of result word 7 is set; nothing divides by zero.
 * MOVE: with d_delta NULL output j is the 16 bytes of pose a[j], bit for bit (NaN payloads and -0 are kept).
 * Otherwise a delta (dc, ds, dx, dy) is composed on the right — the base moves in its own frame by the odometry
 * increment — in float32, no FMA, each product rounded, then the difference or sum, the shape of E15's transform:
 *   c' = c*dc - s*ds;   s' = s*dc + c*ds;   x' = (c*dx - s*dy) + x;   y' = (s*dx + c*dy) + y
 * A result that is NaN is stored as 0x7FC00000 (which payload and sign a produced NaN carries is left to the
 * implementation by IEEE 754; this keeps the output byte-exact everywhere).  n_delta is 1 (one delta per group: plain
 * odometry) or M (one per output at d_delta + g_d * delta_stride + 4 j: odometry with the caller's noise already
 * folded in); g_d = g when delta_per_group is not 0, else 0; delta_stride in floats, >= 4 n_delta and a multiple of
 * 4; d_delta 16-byte aligned.  The device evaluates no trigonometric function and does not renormalise (c, s): a
 * caller rebuilds the list through rplgpu_pose_list when the drift of c*c + s*s matters.  The delta (1, 0, 0, 0) is
 * NOT the bit copy: c = -0 with a negative s becomes +0 (-0 * 1 - s * 0 = -0 - -0 = +0).
 * OUTPUTS: output j of group g at d_poses_out + g * out_stride + 4 j (out_stride in floats, >= 4 M and a multiple of
 * 4; 16-byte aligned; it must not overlap d_poses over the ranges used: refused); a[j] at d_ancestors + g *
 * anc_stride + j (optional; anc_stride >= M); eight 32-bit words per group at d_result + 8 g:
 *   0, 1      S, low and high word
 *   2, 3, 4   the sum of the w[i]^2, 96 bits, low to high (the host forms N_eff = S^2 / sum w^2 from words 0 - 4)
 *   5         the number of weights that are not 0
 *   6         the number of distinct ancestors among the M outputs (min(M, P) when S = 0)
 *   7         flags: bit 0 = S was 0
 * Words of an output array at and beyond M of a group are never changed.  d_weights, d_poses, d_delta and d_u are
 * only read (and must not change while the call runs: its launches read the weights twice).
 * SCRATCH is the caller's, as E13's volume is: rplgpu_resample_scratch_words(G, P) uint32 words at d_scratch, 8-byte
 * aligned; the function is host only and returns 0 for G = 0 or a P outside 1 .. RPLGPU_MAX_POSES.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for G = 0 or above 65535 (groups x tiles is a
 * launch grid), P or M of 0 or above RPLGPU_MAX_POSES, a missing d_weights / d_poses / d_poses_out / d_result /
 * d_scratch, a misaligned pointer (16 bytes: d_poses, d_poses_out, d_delta; 8: d_scratch; 4: the others), the stride
 * rules above with weight_stride >= P, n_delta not in {1, M} with d_delta set, and the overlap.  Asynchronous on the
 * handle's stream. */
uint64_t rplgpu_resample_scratch_words(uint32_t G, uint32_t P);
int32_t rplgpu_resample_poses_dev(rplgpu_handle_t h, const uint32_t *d_weights, uint64_t weight_stride,
                                  const float *d_poses, uint64_t pose_stride, uint32_t poses_per_group, uint32_t G,
                                  uint32_t P, uint32_t M, const uint32_t *d_u, const float *d_delta,
                                  uint32_t n_delta, uint64_t delta_stride, uint32_t delta_per_group,
                                  float *d_poses_out, uint64_t out_stride, uint32_t *d_ancestors,
                                  uint64_t anc_stride, uint32_t *d_result, uint32_t *d_scratch);
/* Host only (no handle, no device): the same rule in plain C++ for ONE group — the definition a reader can run.
 * weights: P words; poses: 4 P floats; delta: NULL, or 4 n_delta floats with n_delta 1 or M; poses_out: 4 M floats;
 * ancestors_out (optional): M words; result: 8 words.  RPLGPU_ERR_INVALID_ARG and nothing written for a NULL
 * weights / poses / poses_out / result, P or M of 0 or above RPLGPU_MAX_POSES, n_delta not in {1, M} with delta set,
 * and a poses_out that overlaps poses. */
int32_t rplgpu_resample_host(const uint32_t *weights, uint32_t P, uint32_t M, uint32_t u, const float *poses,
                             const float *delta, uint32_t n_delta, float *poses_out, uint32_t *ancestors_out,
                             uint32_t result[8]);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_resample_host.  Allocates its
 * device buffers and scratch per call and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_resample_poses(rplgpu_handle_t h, const uint32_t *weights, uint32_t P, uint32_t M, uint32_t u,
                              const float *poses, const float *delta, uint32_t n_delta, float *poses_out,
                              uint32_t *ancestors_out, uint32_t result[8]);

/* ---- E17: a weighted pose list reduced to a pose estimate (row 4; what the filter is built to produce) ----
 * E15 weighs a list and E16 redraws and moves it; what a localiser publishes is ONE pose with a covariance (AMCL's
 * PoseWithCovarianceStamped).  Here the sums that pose is formed from are made on the device, so that
 * score -> estimate -> resample -> move -> score queues on one stream without a read of the list.  Nothing in the
 * reference estimates, so these rules ARE the definition (parity unpinned, as E5-E16).  After one float32 product
 * and one round-to-nearest-even per pose entry everything is integers: the result has one answer, no order of
 * summation matters and no atomic touches a value.
 * SPEC: xy_scale, the quantum of x and y (1024: about 1 mm); gate_r2, the gate's squared radius in quanta; gate_dot,
 * the least C*C + S*S product in Q40 (the cosine of the gate's half angle).  The default is 1024, 512^2 (0.5 m) and
 * 15 * 2^36 (15/16 in Q40, about 20 degrees: it needs no cosine). */
#define RPLGPU_ESTIMATE_WORDS 72u
typedef struct rplgpu_pose_estimate {
  float    xy_scale;
  uint64_t gate_r2;
  int64_t  gate_dot;
} rplgpu_pose_estimate_t;
void rplgpu_default_pose_estimate(rplgpu_pose_estimate_t *s);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL and an xy_scale that is not finite or not > 0.
 * The device path uses this function. */
int32_t rplgpu_pose_estimate_check(const rplgpu_pose_estimate_t *s);
/* INPUTS, per group g of G: P poses of four floats (c, s, x, y) at d_poses + g_p * pose_stride + 4 i, g_p = g when
 * poses_per_group is not 0, else 0 (pose_stride in floats, >= 4 P and a multiple of 4, d_poses 16-byte aligned:
 * E15's and E16's rules); weights w[i] = d_weights[g * weight_stride + i] (E15's output layout, weight_stride >= P),
 * or w = 1 at every pose when d_weights is NULL (the list as E16 leaves it; weight_stride is then not looked at); the
 * centre word d_center[g * center_stride], a uint32 — meant to be E15's result word 1: d_center = d_result + 1 with
 * center_stride = 8 — and the centre index q_c = min(word, P - 1); q_c = 0 (E15's odometry pose by convention) when
 * d_center is NULL.  1 <= P <= RPLGPU_MAX_POSES.
 * QUANTISATION, float32, one product and one rounding, no FMA, no trigonometric function:
 *   tx = x * xy_scale;  ty = y * xy_scale;  tc = c * 1048576.0f;  ts = s * 1048576.0f;
 *   a pose is IN RANGE iff fabsf(t) < 8388608.0f for all four (false for NaN and +-Inf);
 *   X, Y, C, S = (int32) rintf(t), ties to even, so |.| <= 2^23.
 * A pose that is not in range contributes to nothing and sets flag bit 1.
 * GATE: empty, with flag bit 0 set, when the centre pose is not in range.  Otherwise an in-range pose i is in the
 * gate iff  (uint64)(dX*dX + dY*dY) <= gate_r2  with dX = X_i - X_c, dY = Y_i - Y_c  and
 * (int64)C_i*C_c + (int64)S_i*S_c >= gate_dot.  gate_r2 = 2^64 - 1 with gate_dot = INT64_MIN admits every in-range
 * pose.
 * SUMS: two sets — set 0 over every in-range pose, set 1 over the gate — of eight exact signed integers each:
 *   W = sum w,  sum wX,  sum wY,  sum wC,  sum wS,  sum wXX,  sum wXY,  sum wYY.
 * With w < 2^32, |X| <= 2^23 and P <= 2^20 every sum is below 2^98 in magnitude; each is stored as 128-bit two's
 * complement in four uint32 words, low to high.
 * RESULT: RPLGPU_ESTIMATE_WORDS words per group at d_result + 72 g:
 *   0                      flags: bit 0 = the centre is not in range, bit 1 = some pose is not in range,
 *                          bit 2 = set 0 has W = 0, bit 3 = set 1 has W = 0
 *   1                      q_c
 *   2, 3                   the poses in range;  those among them with w != 0
 *   4, 5                   the poses in the gate;  those among them with w != 0
 *   6, 7                   0
 *   8 + 32 k + 4 m .. + 3  sum m of set k, in the order above
 * d_poses, d_weights and d_center are only read (and must not change while the call runs: both launches read the
 * centre).  The means, the heading and the covariance are divisions the host does once: rplgpu_estimate_pose.
 * SCRATCH is the caller's, as E16's: rplgpu_estimate_scratch_words(G, P) uint32 words at d_scratch, 8-byte aligned
 * (its layout: the head of rpl_estimate.hip); the function is host only and returns 0 for arguments the call refuses.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a spec the check refuses, G = 0 or above 65535
 * (groups x tiles is a launch grid), P = 0 or above RPLGPU_MAX_POSES, a missing d_poses / d_result / d_scratch, a
 * misaligned pointer (16 bytes: d_poses; 8: d_scratch; 4: the others), the stride rules above, and center_stride = 0
 * with d_center set and G > 1.  Asynchronous on the handle's stream. */
uint64_t rplgpu_estimate_scratch_words(uint32_t G, uint32_t P);
int32_t rplgpu_estimate_poses_dev(rplgpu_handle_t h, const float *d_poses, uint64_t pose_stride,
                                  uint32_t poses_per_group, const uint32_t *d_weights, uint64_t weight_stride,
                                  uint32_t G, uint32_t P, const rplgpu_pose_estimate_t *s, const uint32_t *d_center,
                                  uint64_t center_stride, uint32_t *d_result, uint32_t *d_scratch);
/* Host only (no handle, no device): the same rule in plain C++ with __int128 for ONE group — the definition a reader
 * can run.  poses: 4 P floats; weights: P words or NULL (w = 1); center: the centre WORD (clamped as above); result:
 * 72 words.  RPLGPU_ERR_INVALID_ARG and nothing written for a NULL poses / result, a spec the check refuses and P = 0
 * or above RPLGPU_MAX_POSES. */
int32_t rplgpu_estimate_host(const float *poses, uint32_t P, const uint32_t *weights,
                             const rplgpu_pose_estimate_t *s, uint32_t center, uint32_t result[72]);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_estimate_host.  Allocates its
 * device buffers and scratch per call and returns when the result is in place: a door, not a hot path. */
int32_t rplgpu_estimate_poses(rplgpu_handle_t h, const float *poses, uint32_t P, const uint32_t *weights,
                              const rplgpu_pose_estimate_t *s, uint32_t center, uint32_t result[72]);
/* Host only: set `set` (0 or 1) of one group's result words as a pose, fp64 formed from the 128-bit integers:
 *   out[0], out[1]  mean x, mean y = (sum wX / W) / xy_scale, ...
 *   out[2]          theta = atan2(sum wS, sum wC)
 *   out[3 .. 5]     covariance xx, xy, yy = (sum wXX / W) / xy_scale^2 - mean x * mean x, ...
 *   out[6]          R = hypot(sum wC, sum wS) / (W * 2^20), the mean resultant length (1: every heading equal)
 *   out[7]          W
 * RPLGPU_ERR_INVALID_ARG and nothing written for NULL, a set above 1, an xy_scale that is not finite or not > 0, and
 * a set whose W is 0.  A convenience, NOT part of the byte-exact contract: every step is one fp64 rounding. */
int32_t rplgpu_estimate_pose(const uint32_t result[72], float xy_scale, uint32_t set, double out[8]);

/* ---- E18: a pose list's motion noise drawn on the device (row 4; the step that kept the filter's loop on the host)
 * ----
 * A particle filter without motion noise collapses after a few resamplings, so a real caller of E16 takes its
 * n_delta = M path: one delta per output with the noise folded in.  Drawn on the host that is 3 M normal variates,
 * M rotations and 16 M bytes copied per time step.  Here a kernel writes E16's d_delta (M deltas per group) from an
 * odometry increment, three noise scales and a counter-based generator, so that
 * sample -> resample and move -> score -> estimate queues on one stream without the host.  E16 is unchanged: its
 * n_delta = M, delta_per_group = 1 input is what this call produces.  Nothing in the reference draws noise, so these
 * rules ARE the definition (parity unpinned, as E5-E17).  The generator is integers and the rest is fixed float32
 * operations: the result is byte-exact and depends on no order.
 *
 * GENERATOR: Philox4x32-10.  One round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
 *   (hi(M1*c2) ^ c1 ^ k0,  lo(M1*c2),  hi(M0*c0) ^ c3 ^ k1,  lo(M0*c0)),   M0 = 0xD2511F53, M1 = 0xCD9E8D57,
 * hi and lo the halves of the 64-bit product; ten rounds, the key incremented by (0x9E3779B9, 0xBB67AE85) before
 * rounds 2 .. 10.  Counter 0 0 0 0 under key 0 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 * For output j of group g, draw i in {0, 1, 2} (rot1, trans, rot2):
 *   key     = (seed low word, seed high word)
 *   counter = ((first + j) mod 2^32,  (g << 2) | i,  step low word,  step high word).
 * step is the caller's time-step number: a new stream per step without reseeding.  first lets a list be made in
 * pieces or on several devices: output j of a call with first = f is output f + j of a call with first = 0, whatever M.
 * THE INTEGER NORMAL: Z = the sum of the eight 16-bit halves of the four output words, minus 262140.  An integer,
 * symmetric, |Z| <= 262140 (exact as a float32), of variance exactly 2863311530 (sigma_Z about 53509.92): Irwin-Hall
 * with eight terms, cut off at +-4.9 sigma.  That is the definition, not an approximation of something else.
 * ODOMETRY: eight floats per group at d_odom + 8 g_o, g_o = g when odom_per_group is not 0, else 0; d_odom 16-byte
 * aligned:  (c1, s1, trans, c2, s2, k1, kt, k2)  — rot1 as a unit vector, the translation along the heading after
 * rot1, rot2 as a unit vector, and the three noise scales per unit of Z (rplgpu_motion_odometry makes them from an
 * increment).  Any values are defined, as in E15: the device checks nothing and evaluates no trigonometric function.
 * ONE OUTPUT, float32, no FMA, every operation rounded once, divides the IEEE divide:
 *   t = (float)Z_i * k;  q = t*t;  den = 1.0f + q;  nc = (1.0f - q) / den;  ns = (t + t) / den
 *       (i = 0 with k1 -> n1;  i = 2 with k2 -> n2): the rotation by 2 atan(t), a unit vector without a cosine,
 *       exactly (1, +-0) at Z = 0
 *   tr = trans + (float)Z_1 * kt
 *   a = r1 o n1:  ac = c1*nc1 - s1*ns1;  as = s1*nc1 + c1*ns1       b = r2 o n2 likewise from (c2, s2) and n2
 *   dc = ac*bc - as*bs;   ds = as*bc + ac*bs;   dx = ac*tr;   dy = as*tr
 * A NaN is stored as 0x7FC00000 (E16's rule).  Output j of group g is the four floats (dc, ds, dx, dy) at
 * d_delta + g * delta_stride + 4 j: E16's layout with delta_per_group = 1.  delta_stride in floats, >= 4 M and a
 * multiple of 4; d_delta 16-byte aligned.  Words at and beyond 4 M of a group are never changed; d_odom is only read.
 * RESULT: eight 32-bit words per group at d_result + 8 g (4-byte aligned), zeroed by the call on the stream and then
 * accumulated with integer atomics (the values depend on no order):
 *   0      the outputs with at least one canonical-NaN entry
 *   1      the largest |Z| over the 3 M draws
 *   2, 3   the sum of Z, int64 two's complement, low and high word
 *   4, 5   the sum of Z^2 (below 2^58), low and high word
 *   6      0
 *   7      flags: bit 0 = word 0 is not 0
 * Words 1 - 5 let a caller see the generator's health at no cost: the mean of Z is 0 and its variance 2863311530.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a NULL spec, G = 0 or above 65535 (tiles x groups
 * is a launch grid), M = 0 or above RPLGPU_MAX_POSES, a missing d_odom / d_delta / d_result, a misaligned pointer
 * (16 bytes: d_odom, d_delta; 4: d_result) and a delta_stride below 4 M or no multiple of 4.  Asynchronous on the
 * handle's stream. */
typedef struct rplgpu_motion_noise {
  uint64_t seed;   /* the key */
  uint64_t step;   /* counter words 2 and 3: the time-step number */
  uint32_t first;  /* the index of the call's output 0 in the group's list */
  uint32_t reserved;  /* not looked at */
} rplgpu_motion_noise_t;
/* seed 0, step 0, first 0 */
void rplgpu_default_motion_noise(rplgpu_motion_noise_t *s);
int32_t rplgpu_sample_motion_dev(rplgpu_handle_t h, const float *d_odom, uint32_t odom_per_group, uint32_t G,
                                 uint32_t M, const rplgpu_motion_noise_t *s, float *d_delta, uint64_t delta_stride,
                                 uint32_t *d_result);
/* Host only (no handle, no device): the same rule in plain C++ for ONE group, whose number `group` (below 65535)
 * enters the counter as g above — the definition a reader can run.  odom: 8 floats; delta_out: 4 M floats; result: 8
 * words.  RPLGPU_ERR_INVALID_ARG and nothing written for a NULL pointer, a group above 65534 and M = 0 or above
 * RPLGPU_MAX_POSES. */
int32_t rplgpu_sample_motion_host(const float odom[8], uint32_t group, uint32_t M, const rplgpu_motion_noise_t *s,
                                  float *delta_out, uint32_t result[8]);
/* ONE group (group 0), HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_sample_motion_host.
 * Allocates its device buffers per call and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_sample_motion(rplgpu_handle_t h, const float odom[8], uint32_t M, const rplgpu_motion_noise_t *s,
                             float *delta_out, uint32_t result[8]);
/* Host only: one Philox4x32-10 block by the rule above, ctr: 4 words, key: 2 words, out: 4 words (out may be ctr).
 * RPLGPU_ERR_INVALID_ARG for a NULL pointer. */
int32_t rplgpu_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* Host only: an odometry increment (dx, dy, dtheta) in the OLD base frame and the four coefficients alpha of the
 * usual differential-drive model become the eight floats of ODOMETRY.  fp64, only * + - sqrt atan2 cos sin, products
 * and sums from left to right:
 *   trans = sqrt(dx*dx + dy*dy);   rot1 = atan2(dy, dx) when trans >= 0.01, else 0;
 *   d = dtheta - rot1;   rot2 = atan2(sin(d), cos(d));
 *   f1 = min(|rot1|, pi - |rot1|),  f2 = min(|rot2|, pi - |rot2|)  (a backward motion is not a large rotation);
 *   v1 = alpha[0]*f1*f1 + alpha[1]*trans*trans;   vt = alpha[2]*trans*trans + alpha[3]*(f1*f1 + f2*f2);
 *   v2 = alpha[0]*f2*f2 + alpha[1]*trans*trans;   sigma_Z = sqrt(2863311530.0);
 *   out = ((float)cos(rot1), (float)sin(rot1), (float)trans, (float)cos(rot2), (float)sin(rot2),
 *          (float)(sqrt(v1) / (2.0 * sigma_Z)),  (float)(sqrt(vt) / sigma_Z),  (float)(sqrt(v2) / (2.0 * sigma_Z))).
 * The rotation noise 2 atan(Z k) is 2 Z k for small angles, hence the 2.  RPLGPU_ERR_INVALID_ARG and nothing written
 * for a NULL alpha or out; values are not checked (a negative alpha gives a NaN scale).  A convenience, NOT part of
 * the byte-exact contract: every step is one fp64 rounding of this machine's libm. */
int32_t rplgpu_motion_odometry(double dx, double dy, double dtheta, const double alpha[4], float out[8]);

/* ---- E19: a pose list seeded over a grid's free cells on the device (row 4; how the filter's list comes to be) ----
 * E15 - E18 run a particle filter's loop on the device; this call makes the list the loop starts from, and the
 * poses AMCL's recovery injects when the average weight drops: M poses in E15 / E16's layout, drawn uniformly over
 * the FREE cells of a grid that is already on the device (E14's rplgpu_map_grid_dev output, an E11 / E12 grid),
 * written wherever the caller points — the tail of E16's output list is such a place.  So
 * initialise -> score -> estimate -> resample, move and inject -> score queues on one stream with no read of a map
 * or a list.  Nothing in the reference seeds poses, so these rules ARE the definition (parity unpinned, as E5-E18).
 * Everything is integers except four fixed float32 operations per coordinate: the output is byte-exact and depends
 * on no order.
 *
 * GRID: group g reads int8 cells at d_grid + g_f * grid_stride, g_f = g when grid_per_group is not 0, else 0; E11's
 * layout and rules (4-byte aligned, grid_stride >= width * height and a multiple of 4).  The grid is only read and
 * must not change while the call runs; bytes at and beyond width * height never count.  A cell is FREE iff
 * free_lo <= (int8)byte <= free_hi.  F = the number of free cells, ordered by their index cy * width + cx.
 * F = 0: every cell counts as free (F := width * height) and flag bit 0 is set; nothing divides by zero (E16's
 * S = 0 convention).
 * HEADING TABLE: H entries (c, s), 2 floats each, at d_headings (8-byte aligned), 1 <= H <= 65536, shared by all
 * groups; entries are copied bit for bit: the device evaluates no trigonometric function.
 * DRAW for output j of group g: one Philox4x32-10 block by E18's rule under E18's rplgpu_motion_noise_t,
 *   key     = (seed low word, seed high word)
 *   counter = ((first + j) mod 2^32,  (g << 2) | 3,  step low word,  step high word)
 * — draw index 3 is the one E18 leaves unused, so E19's stream never meets E18's under the same seed and step.  Of
 * the output words (p0, p1, p2, p3):
 *   r = (p0 * F) >> 32 (a 64-bit product, F <= 2^24): the cell is the r-th free cell, so each free cell is drawn
 *       with probability floor or ceil of 2^32 / F over 2^32;  (cx, cy) = (index mod width, index / width)
 *   k = (p1 * H) >> 32;  (c, s) = table entry k
 *   fx = ((float)(p2 >> 24) + 0.5f) * (1.0f / 256.0f), fy likewise from p3; both 0.5f with flags bit 0
 *   ux = (float)cx + fx (exact: 12 + 9 bits);  x = origin_x + ux * resolution, float32, no FMA: the product is
 *       rounded, then the sum;  y likewise.
 * OUTPUT j of group g is (c, s, x, y) at d_poses_out + g * out_stride + 4 j: E15 / E16's layout, out_stride in
 * floats, >= 4 M and a multiple of 4, d_poses_out 16-byte aligned — it may point into the middle of a longer list
 * (the injection).  Optionally the chosen cell index goes to d_cells_out + g * cell_stride + j (cell_stride >= M).
 * Words at and beyond M of a group are never changed.  With first = f output j is output f + j of a call with
 * first = 0, whatever M: a list can be made in pieces.
 * ROUND TRIP: float32 rounding can put (x, y) into a neighbouring cell when the origin is far from 0.  The rule does
 * not promise otherwise; it counts: an output is OFF-CELL when the E11 CELL of (x, y) (same rule, same IEEE divides,
 * the spec's origin and resolution) does not exist or is not (cx, cy).
 * RESULT: eight 32-bit words per group at d_result + 8 g (4-byte aligned), set by the call on the stream:
 *   0      F, after the F = 0 substitution
 *   1      the OFF-CELL outputs
 *   2      the smallest chosen cell index
 *   3      the largest chosen cell index
 *   4 - 6  0
 *   7      flags: bit 0 = no cell was free; bit 1 = word 1 is not 0
 * SCRATCH is the caller's, as in E16 / E17: rplgpu_seed_scratch_words(G_f, width, height) uint32 words, 8-byte
 * aligned, G_f = G when grid_per_group is not 0, else 1 (about 1.3 bits per cell: a bit mask of the free cells and
 * running counts, never a list of their indices).
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a spec the check refuses, a NULL noise spec,
 * G = 0 or above 65535, M = 0 or above RPLGPU_MAX_POSES, H = 0 or above 65536, a missing d_grid / d_headings /
 * d_poses_out / d_result / d_scratch, a misaligned pointer (16 bytes: d_poses_out; 8: d_headings, d_scratch; 4:
 * d_grid, d_cells_out, d_result), a grid_stride below width * height or no multiple of 4, an out_stride below 4 M or
 * no multiple of 4, and a cell_stride below M with d_cells_out set.  Asynchronous on the handle's stream. */
typedef struct rplgpu_pose_seed {
  float    origin_x, origin_y, resolution;  /* the grid: as rplgpu_pose_score_t */
  uint32_t width, height;                   /* 1 .. RPLGPU_MAX_OCC_DIM */
  int32_t  free_lo, free_hi;                /* a cell is FREE iff free_lo <= (int8)byte <= free_hi */
  uint32_t flags;                           /* bit 0: cell centres, no jitter; other bits 0 */
} rplgpu_pose_seed_t;
/* E11's default grid (0.05 m, 1024 x 1024 cells, origin (-25.6, -25.6)), free_lo = free_hi = 0 (the cells E11 or
 * E14 cleared), flags 0 */
void rplgpu_default_pose_seed(rplgpu_pose_seed_t *s);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, a value that is not finite, resolution <= 0,
 * a dimension of 0 or above RPLGPU_MAX_OCC_DIM, free_lo or free_hi outside [-128, 127], free_lo > free_hi, or flags
 * above 1.  The device path uses this function. */
int32_t rplgpu_pose_seed_check(const rplgpu_pose_seed_t *s);
/* Host only: the scratch of rplgpu_seed_poses_dev in uint32 words; 0 for G_f = 0 or above 65535 or a dimension of 0
 * or above RPLGPU_MAX_OCC_DIM. */
uint64_t rplgpu_seed_scratch_words(uint32_t G_f, uint32_t width, uint32_t height);
/* Host only: entry k of the H entries at cs = ((float)cos(2 pi k / H), (float)sin(the same)), taken in fp64 and
 * rounded once; entry 0 is exactly (1, 0).  RPLGPU_ERR_INVALID_ARG and nothing written for a NULL cs, H = 0 or above
 * 65536.  A convenience, NOT part of the byte-exact contract: every step is one fp64 rounding of this machine's
 * libm. */
int32_t rplgpu_seed_headings(uint32_t H, float *cs);
int32_t rplgpu_seed_poses_dev(rplgpu_handle_t h, const rplgpu_pose_seed_t *s, const int8_t *d_grid,
                              uint64_t grid_stride, uint32_t grid_per_group, const float *d_headings, uint32_t H,
                              uint32_t G, uint32_t M, const rplgpu_motion_noise_t *noise, float *d_poses_out,
                              uint64_t out_stride, uint32_t *d_cells_out, uint64_t cell_stride, uint32_t *d_result,
                              uint32_t *d_scratch);
/* Host only (no handle, no device): the same rule in plain C++ for ONE group, whose number `group` (below 65535)
 * enters the counter as g above — the definition a reader can run.  grid: width * height bytes; headings: 2 H
 * floats; poses_out: 4 M floats; cells_out (optional): M words; result: 8 words.  RPLGPU_ERR_INVALID_ARG and nothing
 * written for a spec the check refuses, a NULL pointer other than cells_out, a group above 65534, H = 0 or above
 * 65536 and M = 0 or above RPLGPU_MAX_POSES. */
int32_t rplgpu_seed_poses_host(const rplgpu_pose_seed_t *s, const int8_t *grid, const float *headings, uint32_t H,
                               uint32_t group, uint32_t M, const rplgpu_motion_noise_t *noise, float *poses_out,
                               uint32_t *cells_out, uint32_t result[8]);
/* ONE group (group 0), HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_seed_poses_host.
 * Allocates its device buffers per call and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_seed_poses(rplgpu_handle_t h, const rplgpu_pose_seed_t *s, const int8_t *grid, const float *headings,
                          uint32_t H, uint32_t M, const rplgpu_motion_noise_t *noise, float *poses_out,
                          uint32_t *cells_out, uint32_t result[8]);

/* ---- E20: a pose list's occupied bins counted on the device (row 4; how the filter sizes its next list) ----
 * E15 - E19 run a particle filter's loop on the device with M, the size of the next list, as the caller's number.
 * AMCL takes M from the list itself (KLD sampling): it bins the samples in (x, y, heading), counts the occupied bins
 * k and draws pf_resample_limit(k) samples — 500 when the filter has converged, 100 000 during global localisation.
 * This call is that count: the poses are binned by fixed float32 and integer rules and marked in a bit map; k and
 * the map come back byte-exact on the handle's stream, the host reads eight words, forms M with
 * rplgpu_kld_samples and passes it to E16, as it already does with N_eff.  Nothing in the reference bins poses, so
 * these rules ARE the definition (parity unpinned, as E5-E19).  Everything is integers after two float32 operations
 * per coordinate: the result depends on no order.
 *
 * INPUTS per group g of G: P poses (c, s, x, y) in E15 / E16 / E17's layout and under their rules (d_poses,
 * pose_stride in floats, >= 4 P and a multiple of 4, poses_per_group, 16-byte aligned); weights
 * d_weights[g * weight_stride + i] (weight_stride >= P).  With d_weights NULL every pose counts; otherwise a pose
 * with w == 0 is SKIPPED, so the call runs on E15's output before the resampling as well as on E16's after it.
 * 1 <= P <= RPLGPU_MAX_POSES, 1 <= G <= 65535.
 * POSITION BIN, float32, no FMA, every operation rounded once:
 *   fx = (x - origin_x) * inv_size;  fy likewise;
 *   in range iff fx >= 0.0f && fx < (float)nx, and the same for y (false for NaN; -0 is in range, bin 0);
 *   bx = (uint32) floorf(fx);  by likewise.
 * HEADING BIN, no trigonometric function on the device:
 *   (c, s) is quantised by E17's rule: tc = c * 1048576.0f, in range iff fabsf(tc) < 8388608.0f,
 *   C = (int32) rintf(tc), S likewise; a pose whose (C, S) is out of range or is (0, 0) is out of range.
 *   The T bin EDGES are a caller-made table of T entries (c, s) at d_edges (8-byte aligned, shared by all groups,
 *   only read), quantised the same way; rplgpu_seed_headings(T, ...) makes such a table, so E19's table serves.
 *   ANGULAR ORDER: half(C, S) = 0 when S > 0 || (S == 0 && C > 0), else 1;  a <= b iff half(a) < half(b), or the
 *   halves are equal and (int64) Ca * Sb - (int64) Sa * Cb >= 0 (exact: the products are below 2^47).  An edge that
 *   is out of range or (0, 0) is never <= anything.
 *   The bin is this bisection, for ANY table:
 *     lo = 0, hi = T;  while (hi - lo > 1) { mid = (lo + hi) >> 1;  if (e_mid <= h) lo = mid; else hi = mid; }
 *     ktheta = lo                                                                        (at most 10 steps)
 *   A table is VALID when entry 0 quantises to (2^20, 0) and the entries strictly increase in the order
 *   (rplgpu_heading_edges_check).  For a valid table ktheta = (the number of edges <= h) - 1: a heading exactly on
 *   an edge belongs to the bin that starts there.
 * BIN ID b = (ktheta * ny + by) * nx + bx;  NB = nx * ny * T.
 * MAP: group g's bit map is ceil(NB / 32) uint32 words at d_map + g * map_stride (map_stride in words, >=
 * ceil(NB / 32) and even; d_map 8-byte aligned); bin b is bit b & 31 of word b >> 5.  Without KEEP (flags bit 0)
 * the call clears those words on the stream first; with KEEP it ORs into what is there.  After the call a bit is
 * set iff it was set before (KEEP only) or some counted pose of the group has that bin.  Words at and beyond
 * ceil(NB / 32) are never changed, bits at and beyond NB never set.  The map is an OUTPUT, not scratch.
 * d_bins_out + g * bin_stride + i (optional, bin_stride >= P) receives b, or 0xFFFFFFFF for a pose that was skipped
 * or out of range; words at and beyond P are never changed.
 * RESULT: eight 32-bit words per group at d_result + 8 g (4-byte aligned), set by the call on the stream:
 *   0      K: the bits this call turned from 0 to 1 (without KEEP: the number of occupied bins)
 *   1      the poses counted
 *   2      the poses out of range (position or heading)
 *   3      the poses skipped for w == 0 (a pose both skipped and out of range counts here only)
 *   4, 5   the smallest and the largest bin id of a counted pose (0xFFFFFFFF and 0 when none was counted)
 *   6      0
 *   7      flags: bit 0 = word 1 is 0; bit 1 = word 2 is not 0; bit 2 = KEEP was set
 * Words 1 + 2 + 3 = P.  A list counted in pieces with KEEP (the first piece without it) has the whole list's map,
 * and its K values add up to the whole list's K.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a spec the check refuses, G = 0 or above 65535,
 * P = 0 or above RPLGPU_MAX_POSES, a missing d_poses / d_edges / d_map / d_result, a misaligned pointer (16 bytes:
 * d_poses; 8: d_edges, d_map; 4: the others), a pose_stride below 4 P or no multiple of 4, a weight_stride below P
 * with d_weights set, a map_stride below ceil(NB / 32) or odd, and a bin_stride below P with d_bins_out set.
 * Asynchronous on the handle's stream; no scratch beyond the map. */
#define RPLGPU_MAX_POSE_BINS 67108864u
#define RPLGPU_MAX_HEADING_BINS 1024u
typedef struct rplgpu_pose_bins {
  float    origin_x, origin_y;  /* the corner of bin (0, 0) */
  float    inv_size;            /* bins per metre (2.0f: 0.5 m) */
  uint32_t nx, ny;              /* 1 .. 65536 each */
  uint32_t flags;               /* bit 0: KEEP the map (do not clear it); other bits 0 */
} rplgpu_pose_bins_t;
/* origin (-25.6, -25.6), inv_size 2.0, 103 x 103 bins, flags 0: E11's default grid at AMCL's bin size (0.5 m) */
void rplgpu_default_pose_bins(rplgpu_pose_bins_t *s);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, a value that is not finite, inv_size <= 0,
 * nx or ny of 0 or above 65536, T of 0 or above RPLGPU_MAX_HEADING_BINS, (uint64) nx * ny * T above
 * RPLGPU_MAX_POSE_BINS, or flags above 1.  The device path uses this function. */
int32_t rplgpu_pose_bins_check(const rplgpu_pose_bins_t *s, uint32_t T);
/* Host only: the words of one group's map, ceil(nx * ny * T / 32) rounded up to even (a valid map_stride); 0 for
 * arguments rplgpu_pose_bins_check refuses. */
uint64_t rplgpu_bin_map_words(uint32_t nx, uint32_t ny, uint32_t T);
/* Host only: RPLGPU_OK when the T entries (c, s) at cs are a VALID table of edges (above), RPLGPU_ERR_INVALID_ARG
 * otherwise (a NULL cs, T = 0 or above RPLGPU_MAX_HEADING_BINS included). */
int32_t rplgpu_heading_edges_check(const float *cs, uint32_t T);
int32_t rplgpu_bin_poses_dev(rplgpu_handle_t h, const rplgpu_pose_bins_t *s, const float *d_poses,
                             uint64_t pose_stride, uint32_t poses_per_group, const uint32_t *d_weights,
                             uint64_t weight_stride, uint32_t G, uint32_t P, const float *d_edges, uint32_t T,
                             uint32_t *d_map, uint64_t map_stride, uint32_t *d_bins_out, uint64_t bin_stride,
                             uint32_t *d_result);
/* Host only (no handle, no device): the same rule in plain C++ for ONE group — the definition a reader can run.
 * poses: 4 P floats; weights (optional): P words; edges: 2 T floats; map: ceil(NB / 32) words, cleared or ORed
 * into by the KEEP flag as above; bins_out (optional): P words; result: 8 words.  RPLGPU_ERR_INVALID_ARG and
 * nothing written for a spec the check refuses, a NULL poses / edges / map / result and P = 0 or above
 * RPLGPU_MAX_POSES. */
int32_t rplgpu_bin_poses_host(const rplgpu_pose_bins_t *s, const float *poses, uint32_t P, const uint32_t *weights,
                              const float *edges, uint32_t T, uint32_t *map, uint32_t *bins_out,
                              uint32_t result[8]);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_bin_poses_host (with KEEP the
 * map at `map` is copied up first).  Allocates its device buffers per call and returns when the results are in
 * place: a door, not a hot path. */
int32_t rplgpu_bin_poses(rplgpu_handle_t h, const rplgpu_pose_bins_t *s, const float *poses, uint32_t P,
                         const uint32_t *weights, const float *edges, uint32_t T, uint32_t *map, uint32_t *bins_out,
                         uint32_t result[8]);
/* Host only, fp64: AMCL's pf_resample_limit.  k <= 1 gives m_max; otherwise b = 2 / (9 (k - 1)),
 * x = 1 - b + sqrt(b) * z, n = ceil((k - 1) / (2 epsilon) * x^3), clamped to [m_min, m_max] (epsilon = 0.01, z = 3:
 * k = 2 -> 527, 10 -> 1363, 100 -> 7332, 1000 -> 56 923 before the clamp).  A convenience, NOT part of the
 * byte-exact contract. */
uint32_t rplgpu_kld_samples(uint32_t k, double epsilon, double z, uint32_t m_min, uint32_t m_max);

/* ---- E21: a binned pose list clustered on the device, the heaviest cluster summed (row 4; the pose AMCL publishes) ----
 * The pose AMCL publishes is the mean of the HEAVIEST CLUSTER of its samples (pf_kdtree_cluster + pf_cluster_stats),
 * not a mean over the list; E17's gate around E15's best pose stood in for it.  E20 leaves what clustering needs on
 * the device — the bit map of occupied bins and one bin id per pose — so this call labels the connected components
 * of that map, weighs each one and reduces the heaviest to E17's exact integer sums: rplgpu_estimate_pose reads the
 * result unchanged, and bin -> cluster -> resample queues on one stream without a read of the map.  Nothing in the
 * reference clusters poses, so these rules ARE the definition (parity unpinned, as E5-E20).  After E17's quantisation
 * everything is integers: the result depends on no order of execution.
 *
 * BINS: bin b = (ktheta * ny + by) * nx + bx and NB = nx * ny * T, exactly as E20; bin b is OCCUPIED iff bit b & 31
 * of word b >> 5 of the group's map (d_map + g * map_stride, E20's layout and rules) is set.  Bits at and beyond NB
 * are not looked at.  K is the number of occupied bins.
 * NEIGHBOURS: two DIFFERENT occupied bins are neighbours iff |dbx| <= 1 and |dby| <= 1 and dktheta is 0, +1 or -1 —
 * taken modulo T when flags bit 0 (WRAP) is set, so that bin T - 1 is next to bin 0, and plainly otherwise.  There
 * is no wrap in x or y: bin (nx - 1, by) and bin (0, by + 1) have adjacent ids and are NOT neighbours.
 * CLUSTERS: a cluster is a connected component of the occupied bins under that relation; its LABEL is its smallest
 * bin id; N_c is the number of clusters.  A map made under KEEP may hold bits that no pose of this list has: such
 * bins still connect clusters, and a cluster may hold no pose.
 * POSES: pose i takes its bin from d_bins[g * bin_stride + i] (E20's d_bins_out; bin_stride >= P).  0xFFFFFFFF is
 * UNLABELLED; an id >= NB, or an id whose bit is not set in the map, is STRAY: counted, flagged (bit 4), and it
 * contributes to nothing; any other pose is LABELLED with its bin's cluster.
 * SUMS: a labelled pose is quantised by E17's rule (xy_scale for x and y, 2^20 for (c, s), in range iff
 * fabsf(t) < 8388608.0f for all four, rintf).  Out of range it sets flag bit 1 and contributes to no sum, count or
 * W (its label is still written).  Weights are read as in E17; d_weights NULL means w = 1.
 * CLUSTER WEIGHT: a cluster's W = sum w and its pose count are taken over its labelled in-range poses.  BEST is the
 * cluster with the largest W, ties going to the smaller label; it is defined whenever N_c >= 1.  SECOND is the same
 * choice among the other clusters, or none when N_c < 2.
 * RESULT: RPLGPU_CLUSTER_WORDS words per group at d_result + 80 g.  Words 0 - 71 are in E17's layout, so
 * rplgpu_estimate_pose works on them: set 0 covers every labelled in-range pose, set 1 the poses of BEST, the same
 * eight 128-bit sums in the same order.
 *   0        flags: bit 0 = N_c is 0; bit 1 = a labelled pose is out of E17's range; bit 2 = set 0 has W = 0;
 *            bit 3 = set 1 has W = 0; bit 4 = a stray entry; bit 5 = a bound was hit (below)
 *   1        BEST's label (0xFFFFFFFF: none)
 *   2, 3     the labelled in-range poses;  those among them with w != 0
 *   4, 5     the poses of BEST;  those among them with w != 0
 *   6, 7     N_c;  K
 *   8 .. 71  the sums, as E17
 *   72, 73   SECOND's label (0xFFFFFFFF: none);  its poses
 *   74, 75   SECOND's W, low and high word
 *   76, 77   the stray entries;  the unlabelled entries
 *   78, 79   0
 * BOUND: the call holds at most RPLGPU_MAX_POSES occupied bins (no list makes more; a KEEP map ORed over several
 * lists can).  With K above it the result is word 0 = 32, words 1 and 72 = 0xFFFFFFFF, word 7 = K and every other
 * word 0, every label written is 0xFFFFFFFF and no table row is written.  Bit 5 is also what a kernel sets when one
 * of its loops reaches its stated bound (rpl_clusters.hip); a correct build never does.  Word 7 tells the two apart:
 * bit 5 with word 7 above RPLGPU_MAX_POSES is this rule and the caller's map, bit 5 with word 7 at or below it is a
 * defect of the build.
 * OPTIONAL OUTPUTS: d_labels_out[g * label_stride + i] (label_stride >= P) receives pose i's label, or 0xFFFFFFFF
 * for an unlabelled or stray pose; words at and beyond P are never changed.  d_clusters + g * cluster_stride
 * receives 4-word rows {label, poses, W low, W high}: the first min(N_c, cluster_cap) clusters in ASCENDING LABEL
 * order; rows beyond that are never changed; cluster_stride >= 4 * cluster_cap.
 * d_map, d_bins, d_poses and d_weights are only read.  SCRATCH is the caller's, as E17's:
 * rplgpu_cluster_scratch_words(G, P, nx, ny, T) uint32 words at d_scratch, 8-byte aligned (its layout: the head of
 * rpl_clusters.hip); the function is host only and returns 0 for arguments the call refuses.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a spec the check refuses, G = 0 or above 65535,
 * P = 0 or above RPLGPU_MAX_POSES, a missing d_poses / d_map / d_bins / d_result / d_scratch, a misaligned pointer
 * (16 bytes: d_poses; 8: d_map, d_scratch; 4: the others), a pose_stride below 4 P or no multiple of 4, a
 * weight_stride below P with d_weights set, a map_stride below ceil(NB / 32) or odd, a bin_stride below P, a
 * label_stride below P with d_labels_out set, a cluster_stride below 4 cluster_cap with d_clusters set and
 * cluster_cap not 0, and an output (d_labels_out, d_clusters, d_result, d_scratch) that overlaps an input or another
 * output.  Asynchronous on the handle's stream. */
#define RPLGPU_CLUSTER_WORDS 80u
typedef struct rplgpu_pose_clusters {
  uint32_t nx, ny;     /* E20's nx, ny: the map's geometry */
  float    xy_scale;   /* E17's quantum for the sums (1024) */
  uint32_t flags;      /* bit 0: the heading axis WRAPS (bin T - 1 is next to bin 0); other bits 0 */
} rplgpu_pose_clusters_t;
/* 103 x 103 bins, xy_scale 1024, WRAP on: E20's default map and E17's default quantum */
void rplgpu_default_pose_clusters(rplgpu_pose_clusters_t *s);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, E20's limits on nx, ny, T and nx * ny * T, an
 * xy_scale that is not finite or not > 0, or flags above 1.  The device path uses this function. */
int32_t rplgpu_pose_clusters_check(const rplgpu_pose_clusters_t *s, uint32_t T);
uint64_t rplgpu_cluster_scratch_words(uint32_t G, uint32_t P, uint32_t nx, uint32_t ny, uint32_t T);
int32_t rplgpu_cluster_poses_dev(rplgpu_handle_t h, const rplgpu_pose_clusters_t *s, const float *d_poses,
                                 uint64_t pose_stride, uint32_t poses_per_group, const uint32_t *d_weights,
                                 uint64_t weight_stride, uint32_t G, uint32_t P, uint32_t T, const uint32_t *d_map,
                                 uint64_t map_stride, const uint32_t *d_bins, uint64_t bin_stride,
                                 uint32_t *d_labels_out, uint64_t label_stride, uint32_t *d_clusters,
                                 uint64_t cluster_stride, uint32_t cluster_cap, uint32_t *d_result,
                                 uint32_t *d_scratch);
/* Host only (no handle, no device): the same rule in plain C++ for ONE group — the definition a reader can run (a
 * flood fill over the occupied bins in ascending id, sums in __int128).  poses: 4 P floats; weights (optional): P
 * words; map: ceil(NB / 32) words; bins: P words; labels_out (optional): P words; clusters_out (optional): 4 *
 * cluster_cap words; result: 80 words.  RPLGPU_ERR_INVALID_ARG and nothing written for a spec the check refuses, a
 * NULL poses / map / bins / result and P = 0 or above RPLGPU_MAX_POSES. */
int32_t rplgpu_cluster_poses_host(const rplgpu_pose_clusters_t *s, const float *poses, uint32_t P,
                                  const uint32_t *weights, uint32_t T, const uint32_t *map, const uint32_t *bins,
                                  uint32_t *labels_out, uint32_t *clusters_out, uint32_t cluster_cap,
                                  uint32_t result[80]);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_cluster_poses_host.  Allocates
 * its device buffers and scratch per call and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_cluster_poses(rplgpu_handle_t h, const rplgpu_pose_clusters_t *s, const float *poses, uint32_t P,
                             const uint32_t *weights, uint32_t T, const uint32_t *map, const uint32_t *bins,
                             uint32_t *labels_out, uint32_t *clusters_out, uint32_t cluster_cap,
                             uint32_t result[80]);

/* ---- E22: a beam fan cast from every pose of a list into a grid (row 4; the beam model's expected ranges) ----
 * E15 weighs a pose by the field bytes under the scan's end points and never asks what lies between the pose and a
 * return.  The second sensor model of the localisation readers (AMCL's beam model, map_calc_range) does: from every
 * pose a ray runs along every beam through the map to the first obstacle, the EXPECTED range, which is then compared
 * with the measured one.  The same cast makes a simulated LaserScan from E14's map and checks a pose hypothesis for
 * visibility.  The grid is E11 / E12 / E14's int8 grid, the walk is E11's, the list is E15 / E16 / E19's, the
 * measured scan is E9's (or E10's) merged LaserScan in the base frame, and the weights and result words come out in
 * E15's layout, so E16, E17, E20 and E21 take them unchanged and seed -> cast -> estimate -> resample -> cast queues
 * on one stream without a read.  Nothing in the reference casts rays, so these rules ARE the definition (parity
 * unpinned, as E5-E21).  After two fixed float32 compositions per ray everything is integers: the result depends on
 * no order.
 *
 * BEAM TABLE: A entries (cb, sb), 2 floats each, at d_beams (8-byte aligned), 1 <= A <= RPLGPU_MAX_MERGE_BEAMS,
 * shared by all groups, only read; the device evaluates no trigonometric function.  P * A <= 2^28 (every count of a
 * group fits 32 bits).
 * RAY (q, a) of group g, q in [0, P), a in [0, A): pose (c, s, tx, ty) by E15's addressing (d_poses, pose_stride in
 * floats, >= 4 P and a multiple of 4, poses_per_group, 16-byte aligned).  Float32, no FMA, each product rounded, then
 * the difference or sum:
 *   dc = c*cb - s*sb;   ds = s*cb + c*sb                                               (E16's composition)
 *   Rm = (float)N * resolution;   ex = tx + dc*Rm;   ey = ty + ds*Rm                   (N = max_steps)
 *   (x0, y0) = the E11 CELL of (tx, ty);  (x1, y1) = the E11 CELL of (ex, ey): same rule, same IEEE divides.
 *   A ray whose start or end has no cell is DROPPED: its range word is 0xFFFFFFFF.
 * Any (c, s) is defined (a scale, the zero matrix, NaN: dropped).
 * THE WALK is E11's Bresenham, verbatim: ax = |x1 - x0|, ay = |y1 - y0|, stepx = sign(x1 - x0), stepy =
 * sign(y1 - y0), err = ax - ay; visit n = 0 is the cell (x0, y0).  AT EVERY VISIT of a cell (x, y), in this order:
 *   1. (x, y) outside [0, width) x [0, height):                    stop, kind LEFT (2)
 *   2. (int8)byte >= hit_lo:                                        stop, kind HIT (0)
 *   3. byte < 0 and unknown_stops:                                  stop, kind UNKNOWN (1)
 *   4. (x, y) == (x1, y1) or n == N:                                stop, kind NONE (3)
 *   5. otherwise e2 = 2 err, and with this one e2
 *        if (e2 > -ay) { err -= ay; x += stepx; }   if (e2 < ax) { err += ax; y += stepy; }   and n + 1.
 * N bounds every walk.  byte = d_grid[g_f * grid_stride + y * width + x], g_f = g when grid_per_group is not 0, else
 * 0; grid_stride >= width * height and a multiple of 4, d_grid 4-byte aligned (E15's field rules); only read.
 * RANGE WORD = D2 | kind << 28 with D2 = (x - x0)^2 + (y - y0)^2 of the stopping cell (<= 2^27: |x - x0| <= n <= N
 * <= 8192); bits 30 and 31 are 0, so no range word equals the dropped ray's.  It goes to
 * d_ranges_out[g * range_stride + q * A + a] (optional; range_stride in words, >= P * A); words at and beyond P * A
 * of a group are never changed.
 * WEIGHT, only with d_measured set: the measured range of beam a is
 *   z = d_measured[g * meas_stride + meas_first + a * meas_step]                       (E9's ranges; +inf: no return)
 * with meas_first + (A - 1) * meas_step < meas_stride.  z NaN (a beam E10 removed): the beam is SKIPPED for every
 * pose.  A dropped ray is skipped for its pose.  Otherwise, float32:
 *   mz = z / resolution (IEEE divide; +inf stays +inf)
 *   de = sqrtf((float)D2), correctly rounded, for kinds 0 - 2;  +inf for NONE
 *   both +inf:  t = d_table[2K + 1]                                                    (K = table_half)
 *   otherwise   d = mz - de;   t = d_table[K + (int)max(-K, min(K, floorf(d)))]
 * d_table: 2K + 2 bytes, uint8, the caller's, shared by all groups, only read: entry K + j is the term of a return
 * j cells (rounded down) behind the expected one, entries 0 and 2K take everything beyond, entry 2K + 1 is "no
 * return expected, none measured".  Gaussian hit, short, max and random are mixed by the caller, in cells.
 *   d_weights[g * weight_stride + q] = the sum of t over the pose's beams, uint32 (255 * 16384 < 2^32);
 *   weight_stride >= P; words at and beyond P of a group are never changed.
 * RESULT, only with d_measured set: eight words per group at d_result + 8 g, E15's exactly (largest weight, the
 * smallest q that has it, how many have it, the weights of 0, word 4, the weight of pose 0, the sum low and high);
 * word 4 = the beams whose z is not NaN.  Without d_measured, d_weights and d_result are ignored and never written.
 * CAST COUNTS: eight words per group at d_cast + 8 g (required, 4-byte aligned):
 *   0 - 3   the rays of kind HIT / UNKNOWN / LEFT / NONE
 *   4       the dropped rays                                       (words 0 + 1 + 2 + 3 + 4 = P * A)
 *   5       the largest D2 among the HIT rays (0 if none)
 *   6, 7    the sum over all rays of n at the stop (the cell steps walked), low and high word
 * At least one of d_ranges_out / d_measured must be set.
 * IDENTITIES that follow from the rules:
 *   (1) pose (c, s, tx, ty) with beam (1, 0) has the range word of pose (1, 0, tx, ty) with beam (c, s): c*1 - s*0
 *       and 1*c - 0*s both round to c (for finite c, s);
 *   (2) the weights recomputed on the host from the returned range words, the measured ranges and the table by the
 *       WEIGHT rule equal the device's;
 *   (3) a list cast in two pieces (pointer offsets into d_poses, d_ranges_out, d_weights) has the words and weights
 *       of the list cast at once, and the counts of the pieces add up (word 5: the larger);
 *   (4) the result words are what E15's RESULT rule gives on the returned weights.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a spec the check refuses, G = 0 or above 65535,
 * P = 0 or above RPLGPU_MAX_POSES, A = 0 or above RPLGPU_MAX_MERGE_BEAMS, P * A above 2^28, a missing d_poses /
 * d_beams / d_grid / d_cast, neither d_ranges_out nor d_measured, d_measured without d_table / d_weights / d_result,
 * a misaligned pointer (16 bytes: d_poses; 8: d_beams; 4: d_grid, d_measured, d_ranges_out, d_weights, d_result,
 * d_cast), a pose_stride below 4 P or no multiple of 4, a grid_stride below width * height or no multiple of 4, a
 * range_stride below P * A with d_ranges_out set, and with d_measured set a weight_stride below P or
 * meas_first + (A - 1) * meas_step >= meas_stride.  Asynchronous on the handle's stream; no scratch. */
#define RPLGPU_CAST_HIT     0u
#define RPLGPU_CAST_UNKNOWN 1u
#define RPLGPU_CAST_LEFT    2u
#define RPLGPU_CAST_NONE    3u
#define RPLGPU_CAST_DROPPED 0xFFFFFFFFu
#define RPLGPU_MAX_CAST_TABLE_HALF 4096u
#define RPLGPU_MAX_CAST_RAYS 268435456u
typedef struct rplgpu_range_cast {
  float    origin_x, origin_y, resolution;  /* the grid: as rplgpu_pose_score_t */
  uint32_t width, height;                   /* 1 .. RPLGPU_MAX_OCC_DIM */
  uint32_t max_steps;                       /* N, 1 .. RPLGPU_MAX_OCC_STEPS */
  int32_t  hit_lo;                          /* 1 .. 127: a cell stops a ray as HIT iff (int8)byte >= hit_lo */
  uint32_t unknown_stops;                   /* 0 / 1: a negative byte stops a ray as UNKNOWN */
  uint32_t table_half;                      /* K, 0 .. RPLGPU_MAX_CAST_TABLE_HALF */
} rplgpu_range_cast_t;
/* E11's default grid (0.05 m, 1024 x 1024 cells, origin (-25.6, -25.6)), N = 240 (12 m), hit_lo 100,
 * unknown_stops 1 (AMCL's rule), K = 40 */
void rplgpu_default_range_cast(rplgpu_range_cast_t *s);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, a value that is not finite, resolution <= 0, a
 * dimension of 0 or above RPLGPU_MAX_OCC_DIM, max_steps of 0 or above RPLGPU_MAX_OCC_STEPS, hit_lo outside
 * [1, 127], unknown_stops above 1 or table_half above RPLGPU_MAX_CAST_TABLE_HALF.  The device path uses this
 * function. */
int32_t rplgpu_range_cast_check(const rplgpu_range_cast_t *s);
/* Host only: the centre directions of E9's beams k = first + a * step, a in [0, A), as cs[2a], cs[2a + 1] =
 * ((float)cos(phi), (float)sin(phi)), phi = (double)angle_min + ((double)k + 0.5) * (double)inc with inc from
 * rplgpu_scan_merge_edges, taken in fp64 and rounded once.  With first and step as meas_first and meas_step the
 * table lines up with the merged scan's ranges.  RPLGPU_ERR_INVALID_ARG and nothing written for a NULL cs, a spec
 * rplgpu_scan_merge_edges refuses, A = 0 or above RPLGPU_MAX_MERGE_BEAMS, or first + (A - 1) * step >= m->count.  A
 * convenience, NOT part of the byte-exact contract, like rplgpu_seed_headings. */
int32_t rplgpu_cast_beams(const rplgpu_scan_merge_t *m, uint32_t first, uint32_t step, uint32_t A, float *cs);
/* Host only: a range word in metres, sqrt((double)D2) * (double)resolution for kinds 0 - 2, +inf for NONE, NaN for
 * a dropped ray. */
double rplgpu_cast_range_m(uint32_t word, float resolution);
int32_t rplgpu_cast_ranges_dev(rplgpu_handle_t h, const rplgpu_range_cast_t *s, const float *d_poses,
                               uint64_t pose_stride, uint32_t poses_per_group, uint32_t G, uint32_t P,
                               const float *d_beams, uint32_t A, const int8_t *d_grid, uint64_t grid_stride,
                               uint32_t grid_per_group, const float *d_measured, uint64_t meas_stride,
                               uint32_t meas_first, uint32_t meas_step, const uint8_t *d_table,
                               uint32_t *d_ranges_out, uint64_t range_stride, uint32_t *d_weights,
                               uint64_t weight_stride, uint32_t *d_result, uint32_t *d_cast);
/* Host only (no handle, no device): the same rule in plain C++ for ONE group — the definition a reader can run.
 * poses: 4 P floats; beams: 2 A floats; grid: width * height bytes; measured (optional): meas_count floats, which
 * stand for meas_stride; table: 2K + 2 bytes, weights_out: P words and result: 8 words, all three required with
 * measured and ignored without it; ranges_out (optional): P * A words; cast: 8 words.  RPLGPU_ERR_INVALID_ARG and
 * nothing written for a spec the check refuses, a NULL poses / beams / grid / cast, neither ranges_out nor
 * measured, P = 0 or above RPLGPU_MAX_POSES, A = 0 or above RPLGPU_MAX_MERGE_BEAMS, P * A above 2^28 and
 * meas_first + (A - 1) * meas_step >= meas_count. */
int32_t rplgpu_cast_ranges_host(const rplgpu_range_cast_t *s, const float *poses, uint32_t P, const float *beams,
                                uint32_t A, const int8_t *grid, const float *measured, uint32_t meas_count,
                                uint32_t meas_first, uint32_t meas_step, const uint8_t *table, uint32_t *ranges_out,
                                uint32_t *weights_out, uint32_t result[8], uint32_t cast[8]);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_cast_ranges_host.  Allocates
 * its device buffers per call and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_cast_ranges(rplgpu_handle_t h, const rplgpu_range_cast_t *s, const float *poses, uint32_t P,
                           const float *beams, uint32_t A, const int8_t *grid, const float *measured,
                           uint32_t meas_count, uint32_t meas_first, uint32_t meas_step, const uint8_t *table,
                           uint32_t *ranges_out, uint32_t *weights_out, uint32_t result[8], uint32_t cast[8]);

/* ---- E23: the beams a pose list disagrees with are left out of the weights (row 4; AMCL's beam skip) ----
 * E15 adds every point's field value into every pose's weight.  A return from something the map does not hold (a
 * person, a trolley) lands far from every obstacle at almost every pose of the list: it lowers every weight by the
 * same amount and the list loses contrast exactly when the room is busy.  AMCL's likelihood_field_prob model counts,
 * per beam, at how many particles the beam lands near an obstacle, leaves out the beams too few particles agree
 * with, and falls back to all beams when too many would go (the filter has then probably converged on a wrong
 * pose).  The per-beam count is a reduction ACROSS the pose list of all poses x points look-ups, which only the
 * device ever sees, so it cannot be done from outside E15.  The mask that comes out is worth having on its own: the
 * returns the map does not explain, that is, the moving obstacles.  Nothing in the reference does this, so these
 * rules ARE the definition (parity unpinned, as E5-E22).  All integers behind E15's float32 pose transform:
 * byte-exact, order-free, chainable.
 *
 * f(q, i): E15's field value of sample i at pose q, exactly — the same points (E1, E5, E2, E6, the mount pose), the
 * same transform without FMA, the E11 cell rule, 0 outside the grid, 0 for an unknown (negative) byte, 0 (and
 * RPLGPU_SCAN_CELL_RANGE) for a position without a cell.  P is the whole list of the group, whatever its poses are.
 *   AGREE   a look-up of sample i at pose q agrees iff f(q, i) >= agree_lo (1 .. 127).  A pose at which the sample
 *           has no cell simply does not agree, and stays in P.
 *   COUNT   count[i] = the number of poses q in [0, P) that agree; 0 for a sample that E1 or E5 drops, that is not
 *           finite, or that lies at or beyond the scan's clamped length min(n, n_stride).
 *   KEEP    a finite sample is kept by the rule iff (uint64)count[i] * keep_den > (uint64)keep_num * P: strict, as
 *           AMCL's obs_count / total > beam_skip_threshold.  1 <= keep_den <= 2^20, keep_num <= keep_den.
 *   FALL BACK  with F the group's finite points and K those kept by the rule, the group falls back iff F > 0 and
 *           (uint64)(F - K) * err_den >= (uint64)err_num * F: AMCL's skipped >= beams * beam_skip_error_threshold.
 *           1 <= err_den <= 2^20, err_num <= 2^20.  err_num == 0: every group with a finite point falls back, the
 *           stage is off.  err_num > err_den: no group ever does.
 *   WEIGHT  d_weights[g * weight_stride + q] = the sum of f(q, i) over the samples that ENTERED the weights: all F
 *           finite ones when the group fell back, else the K kept ones.  E15's layout, bound (group * n_stride <=
 *           2^24) and result words: d_result + 8 g holds E15's eight words computed from these weights, word 4 stays
 *           the number of finite points.  E16, E17, E20 and E21 take both unchanged.
 * OUTPUTS besides d_weights, d_result and d_status (E15's rules and refusals for all of them and for the points,
 * groups, pose list and field):
 *   d_counts[sc * count_stride + i], uint32, count_stride >= n_stride: count[i] of scan sc.  Every word [0, n_stride)
 *           of every scan of the call is written; words beyond are never changed.
 *   d_mask[sc * mask_stride + (i >> 5)] bit (i & 31): E5's keep-mask layout, mask_stride >= ceil(n_stride / 32).  1 iff
 *           the sample is finite and kept by the rule — the RULE's mask whether or not the group falls back, so it
 *           stays usable as the detection of what the map does not explain.  Every word [0, ceil(n_stride / 32)) of
 *           every scan is written; bits at and beyond n_stride are 0.
 *   d_agree + 8 g, eight words per group:
 *     0      F, the group's finite points
 *     1      K, those kept by the rule
 *     2      1 iff the group fell back
 *     3      the samples that entered the weights (F on a fallback, else K)
 *     4      the largest count
 *     5      the smallest count over the finite samples (0 when F = 0)
 *     6, 7   the sum of all counts, low and high word (up to 2^44)
 * FOUR IDENTITIES follow from the rules and hold the kernels of this stage to E15's:
 *   (1) with err_num = 0 the weights and d_result equal rplgpu_score_poses_dev's on the same inputs, byte for byte;
 *   (2) with a field of bytes 0 and 1 only and agree_lo = 1, words 6 and 7 of d_agree equal words 6 and 7 of E15's
 *       result (every agreeing look-up adds exactly 1 to one weight);
 *   (3) with P = 1, agree_lo = 1, keep_num = 0 and err_num > err_den the weight equals E15's, and the mask is exactly
 *       the set of samples with f >= 1;
 *   (4) with E5 off, for a group that did not fall back, the weights equal E15's on a copy of the batch in which every
 *       skipped sample (finite, mask bit 0) is replaced by a node E1 drops (distance 0).
 * d_counts, d_mask and d_agree are required, 4-byte aligned device memory.  RPLGPU_ERR_INVALID_ARG for everything
 * rplgpu_score_poses_dev refuses, a spec the check refuses, count_stride below n_stride and mask_stride below
 * ceil(n_stride / 32).  A refused call changes no output.  Asynchronous on the handle's stream; nothing is stored
 * on the handle, the call's scratch is its outputs. */
typedef struct rplgpu_beam_agree {
  float    origin_x, origin_y;   /* the field's grid: as rplgpu_pose_score_t */
  float    resolution;
  uint32_t width, height;        /* 1 .. RPLGPU_MAX_OCC_DIM */
  int32_t  agree_lo;             /* 1 .. 127 */
  uint32_t keep_num, keep_den;   /* 1 <= keep_den <= 2^20, keep_num <= keep_den */
  uint32_t err_num, err_den;     /* 1 <= err_den <= 2^20, err_num <= 2^20 */
} rplgpu_beam_agree_t;
#define RPLGPU_AGREE_MAX_DEN 1048576u
/* E11's default grid, agree_lo 1, keep 3 / 10 and err 9 / 10 (AMCL's beam_skip_threshold 0.3 and
 * beam_skip_error_threshold 0.9) */
void rplgpu_default_beam_agree(rplgpu_beam_agree_t *s);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, a grid rplgpu_pose_score_check refuses,
 * agree_lo outside [1, 127], keep_den or err_den of 0 or above 2^20, keep_num above keep_den, err_num above 2^20.
 * The device path uses this function. */
int32_t rplgpu_beam_agree_check(const rplgpu_beam_agree_t *s);
int32_t rplgpu_score_poses_agree_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                     const uint32_t *d_n_per_scan, uint32_t B, uint32_t group,
                                     const rplgpu_params_t *p, const float *d_motion, const float *d_pose2d,
                                     const rplgpu_beam_agree_t *s, const float *d_poses, uint32_t P,
                                     uint64_t pose_stride, uint32_t poses_per_group, const int8_t *d_field,
                                     uint64_t field_stride, uint32_t field_per_group, uint32_t *d_weights,
                                     uint64_t weight_stride, uint32_t *d_result, uint32_t *d_status,
                                     uint32_t *d_counts, uint64_t count_stride, uint32_t *d_mask,
                                     uint64_t mask_stride, uint32_t *d_agree);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), shaped as rplgpu_score_poses: counts_out
 * (optional): n_scans * n_stride words; mask_out (optional): n_scans * ceil(n_stride / 32) words; agree: 8 words.
 * Allocates its device buffers per call and returns when the results are in place. */
int32_t rplgpu_score_poses_agree(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                                 const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                                 const float *motion, const float *pose2d, const float *t0,
                                 const rplgpu_beam_agree_t *s, const float *poses, uint32_t P, const int8_t *field,
                                 uint32_t *weights_out, uint32_t result[8], uint32_t *status, uint32_t *counts_out,
                                 uint32_t *mask_out, uint32_t agree[8]);
/* Host only (no handle, no device): the same rule in plain C++ for ONE group, over POINTS — the definition a reader
 * can run, and a node's fallback without a device.  Point k is (x[k], y[k]) in the base frame (what E15's front end
 * makes of a sample that E1 and E5 keep; it may be not finite) and belongs to sample index[k] of scan slot[k]; each
 * (slot, index) appears at most once.  poses: 4 P floats; field: width * height bytes.  counts_out: n_scans *
 * n_stride words, mask_out: n_scans * ceil(n_stride / 32) words, weights_out: P words, result: 8, agree: 8, all
 * required and written whole; status (optional): RPLGPU_SCAN_CELL_RANGE or 0.  RPLGPU_ERR_INVALID_ARG and nothing
 * written for a spec the check refuses, a NULL pointer (x, y, slot, index only with n_points > 0), P = 0 or above
 * RPLGPU_MAX_POSES, n_scans = 0, n_stride = 0, n_scans * n_stride above 2^24, or a slot / index out of range. */
int32_t rplgpu_beam_agree_points_host(const float *x, const float *y, const uint32_t *slot, const uint32_t *index,
                                      uint32_t n_points, uint32_t n_scans, uint32_t n_stride, const float *poses,
                                      uint32_t P, const int8_t *field, const rplgpu_beam_agree_t *s,
                                      uint32_t *counts_out, uint32_t *mask_out, uint32_t *weights_out,
                                      uint32_t result[8], uint32_t agree[8], uint32_t *status);

/* ---- E24: scans matched over a wide window by bound and refine (row 4; the mapping side's loop closer) ----
 * E13 scores every pose of its window, so the window ends at 32 cells (1.6 m at 0.05 m): enough to track a pose
 * between two time steps, not to close a loop after drift, relocalise against a stored map or start E14's chain from
 * a poor prior.  Here the window reaches 256 cells a side and the answer is still E13's, by the branch and bound of
 * Cartographer's FastCorrelativeScanMatcher2D with ONE coarse level: a sliding maximum P of the field, an upper
 * bound U per BLOCK of s x s shifts read from P, E13 scores only for the blocks whose bound can still win.  Nothing
 * in the reference matches scans, so these rules ARE the definition (parity unpinned, as E5-E23).  After the float32
 * rotation everything is sums and maxima of bytes: the result depends on no order.
 *
 * POINTS, the pivot, CANDIDATE (k, j, i), the rotated cell (cx, cy), f = max(byte, 0) with 0 outside the grid
 * (written F(x, y) below), RPLGPU_SCAN_OUT_TRUNCATED / RPLGPU_SCAN_CELL_RANGE in d_status[g] and the bound group *
 * n_stride <= 2^24 are those of the E13 block above, word for word, with i in [-Tx, Tx], j in [-Ty, Ty] and Tx, Ty
 * up to RPLGPU_MAX_WIDE_SHIFT.  The ROTATION TABLE is exactly rplgpu_scan_match_rotations of an E13 spec with the
 * same rot_steps and rot_step.  score(k, j, i) below is E13's score of that candidate.
 * POOLED FIELD, s = RPLGPU_WIDE_MATCH_BLOCK: for x in [-(s-1), width) and y in [-(s-1), height)
 *   P(x, y) = max over a, b in [0, s) of F(x + a, y + b),
 * int8 (0 .. 127) in a grid of Wp = width + s - 1 by Hp = height + s - 1: P(x, y) sits at (y + s-1) * Wp + (x + s-1).
 * BLOCKS: nbx = ceil((2Tx + 1) / s), nby = ceil((2Ty + 1) / s).  Block (k, bj, bi) holds the candidates of rotation
 * k with i in [-Tx + bi*s, -Tx + bi*s + s-1] and at most Tx, j likewise (2T + 1 is odd: the last block of an axis is
 * always partial).  Its flat index is ((k + K) * nby + bj) * nbx + bi.
 * BOUND: U[g][k][bj][bi] = the sum over the group's points of P(cx - Tx + bi*s, cy - Ty + bj*s), 0 where P is not
 * defined; uint32 at d_bounds + g * bounds_stride + the block's flat index.  U is at least the score of every
 * candidate of its block.  The bounds volume is the call's own result, as E13's score volume is; words at and beyond
 * a group's rplgpu_wide_match_blocks words are never changed.
 * SEEDS: A is the block of the greatest U, among equals the lowest flat index; B is the block that holds (0, 0, 0).
 * b0 = the greatest score over the (in-window) candidates of both seeds.
 * LIST: every block with U >= b0; n is their number.
 *   PROVEN, n <= max_blocks: every candidate of every listed block is scored, and words 0 - 3 and 6 of d_best + 8 g
 *     are E13's words of the exhaustive volume over the wide window, tie rule included (largest score, then the
 *     smallest i*i + j*j, |k|, k, j, i).  A candidate of score >= b0 lies in a block of U >= b0, so the best, every
 *     candidate that ties with it and their number are all inside the list.
 *   UNPROVEN, n > max_blocks: nothing beyond the seeds is scored; words 0 - 3 and 6 are taken over the candidates
 *     of the two seeds alone (each once when A is B) and word 7 is RPLGPU_WIDE_MATCH_UNPROVEN.  The caller repeats
 *     with max_blocks >= word 4 of the work words, or accepts the result.
 *   Word 4 is always the group's finite points, word 5 always the score of (0, 0, 0), word 7 otherwise 0.
 * A group without points has U 0 everywhere and b0 0, so every block is listed: it is proven iff the volume has at
 * most max_blocks blocks, and then best is 0 at (0, 0, 0) with word 6 the number of candidates, as E13; unproven it
 * is 0 at (0, 0, 0) with word 6 the candidates of block 0 and of seed B.
 * WORK WORDS, eight per group at d_work + 8 g: 0 the blocks in the volume, 1 the greatest U, 2 seed A's flat index,
 * 3 b0, 4 n, 5 max_blocks, 6 and 7 zero.
 * APPLYING IT: d_best goes into rplgpu_apply_match_dev unchanged; that call reads k against K and takes any i, j,
 * and the caller hands it an E13 spec (rplgpu_scan_match_t) with the same grid, rot_steps and rot_step, any shifts. */
#define RPLGPU_WIDE_MATCH_BLOCK    8u      /* s: a block is 8 x 8 shifts, one wave of candidates */
#define RPLGPU_MAX_WIDE_SHIFT      256u    /* cells, per axis */
#define RPLGPU_MAX_WIDE_BLOCKS     65536u  /* the largest max_blocks */
#define RPLGPU_WIDE_MATCH_UNPROVEN 0x1u    /* word 7 of d_best */
typedef struct rplgpu_wide_match {
  float    origin_x, origin_y;   /* the field's grid: as rplgpu_scan_match_t */
  float    resolution;
  uint32_t width, height;        /* 1 .. RPLGPU_MAX_OCC_DIM */
  uint32_t shift_x, shift_y;     /* Tx, Ty: 0 .. RPLGPU_MAX_WIDE_SHIFT */
  uint32_t rot_steps;            /* K: 0 .. RPLGPU_MAX_MATCH_ROT */
  float    rot_step;             /* rad, E13's rules */
  uint32_t max_blocks;           /* the cap of the list, 1 .. RPLGPU_MAX_WIDE_BLOCKS */
} rplgpu_wide_match_t;
/* E11's default grid, Tx = Ty = 64, K = 10, rot_step = (float)(0.25 * pi / 180), max_blocks = 1024 */
void rplgpu_default_wide_match(rplgpu_wide_match_t *m);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for everything rplgpu_scan_match_check refuses with
 * RPLGPU_MAX_WIDE_SHIFT in place of RPLGPU_MAX_MATCH_SHIFT, and for max_blocks of 0 or above RPLGPU_MAX_WIDE_BLOCKS.
 * The device path uses this function. */
int32_t rplgpu_wide_match_check(const rplgpu_wide_match_t *m);
/* Host only.  (2K + 1) * nby * nbx, the words of one group's bounds volume; 0 for a spec the check refuses. */
uint32_t rplgpu_wide_match_blocks(const rplgpu_wide_match_t *m);
/* Host only.  The uint32 words of scratch a call over G groups takes: G * (272 + 65 * max_blocks), the cap's 64
 * score words a listed block, the list, the seeds and the counters; not decreasing in G and in max_blocks, and 0
 * for a spec the check refuses or G = 0. */
uint64_t rplgpu_wide_match_scratch_words(const rplgpu_wide_match_t *m, uint32_t G);
/* Host only: P of ONE field in plain C++, the definition a reader can run.  field: width * height bytes; pooled:
 * (width + s-1) * (height + s-1) bytes, written whole.  RPLGPU_ERR_INVALID_ARG and nothing written for a NULL
 * pointer or a dimension of 0 or above RPLGPU_MAX_OCC_DIM. */
int32_t rplgpu_pool_field_host(const int8_t *field, uint32_t width, uint32_t height, int8_t *pooled);
/* P of F fields on the handle's stream, an entry of its own so that a caller with a static map pools it once.
 * Field f is read at d_field + f * field_stride (E13's rules: 4-byte aligned, field_stride >= width * height and a
 * multiple of 4, only read) and its P written at d_pooled + f * pooled_stride (4-byte aligned, pooled_stride >=
 * Wp * Hp and a multiple of 4, which must not overlap the fields); bytes at and beyond Wp * Hp of a pooled field are
 * never changed.  Only the grid of `m` is used, but the whole spec is checked.  RPLGPU_ERR_INVALID_ARG for a spec
 * the check refuses, a missing or misaligned pointer, the stride rules, F above 65535; F = 0 does nothing.  A refused
 * call changes no output. */
int32_t rplgpu_pool_field_dev(rplgpu_handle_t h, const rplgpu_wide_match_t *m, const int8_t *d_field,
                              uint64_t field_stride, uint32_t F, int8_t *d_pooled, uint64_t pooled_stride);
/* The match.  E13's arguments with the new spec; d_pooled holds P of the very fields at d_field (pooled field g_f
 * beside field g_f; both are only read), d_bounds / bounds_stride (>= rplgpu_wide_match_blocks) the bounds volumes,
 * d_best and d_work eight words a group, d_status optional.  SCRATCH is the caller's: rplgpu_wide_match_scratch_words
 * (m, G) uint32 words at d_scratch, 8-byte aligned, G the number of groups; it holds nothing a second call may rely
 * on, and words beyond it are never touched, whatever n is.  Nothing is stored on the handle, nothing is copied from
 * pageable memory, and there is no host round trip between bound, select and refine: the list's length stays on the
 * device.  RPLGPU_ERR_INVALID_ARG for everything rplgpu_match_scans_dev refuses (the spec by rplgpu_wide_match_check,
 * bounds for scores), a missing or misaligned d_pooled / d_work (4 bytes) / d_scratch (8 bytes) and the pooled
 * stride rules above.  A refused call changes no output.  Asynchronous on the handle's stream. */
int32_t rplgpu_match_wide_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                              const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                              const float *d_motion, const float *d_pose2d, const float *d_pivot,
                              const rplgpu_wide_match_t *m, const int8_t *d_field, uint64_t field_stride,
                              uint32_t field_per_group, const int8_t *d_pooled, uint64_t pooled_stride,
                              uint32_t *d_bounds, uint64_t bounds_stride, uint32_t *d_scratch, uint32_t *d_best,
                              uint32_t *d_work, uint32_t *d_status);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), shaped as rplgpu_match_scans: pools the field
 * itself; bounds_out (optional): rplgpu_wide_match_blocks words; best: 8 words; work: 8 words; status (optional).
 * Allocates its device buffers per call and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_match_wide(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                          const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                          const float *motion, const float *pose2d, const float *t0, const float *pivot,
                          const rplgpu_wide_match_t *m, const int8_t *field, uint32_t *bounds_out, uint32_t best[8],
                          uint32_t work[8], uint32_t *status);

/* ---- E25: poses refined below a cell by Gauss-Newton on the interpolated field (row 4; the matcher's last stage) ----
 * E13 / E24 answer on a lattice of whole cells and rotation steps, E15 scores a pose by the byte under each point.
 * Every 2-D matcher among E11's readers then refines below the cell: Hector's Gauss-Newton on the bilinearly
 * interpolated map, Cartographer's Ceres matcher behind its correlative one.  Here that stage runs on the device:
 * for every pose of a list the normal equations of ONE Gauss-Newton step of the group's points against the bilinear
 * field, a tiny kernel that takes the step, n rounds queued on one stream, and two joining kernels to E13 / E24 on
 * one side and E11 / E14 on the other.  Nothing in the reference refines a pose, so these rules ARE the definition
 * (parity unpinned, as E5-E24).  After a fixed float32 front everything is integers: the sums have one answer and
 * depend on no order; the step is a fixed sequence of correctly rounded fp64 operations with a host twin.
 *
 * POINTS: those of rplgpu_score_poses_dev, word for word (E1, E5 with p->ror_enable, E2, E6, d_pose2d as each
 * sensor's MOUNT pose in the base frame, groups clamped to B, a point that is not finite ignored, group * n_stride
 * <= 2^24).  POSES: E15's as well, (c, s, tx, ty) at d_poses + g_p * pose_stride + 4 q, the same alignment, stride
 * and poses_per_group rules; no trigonometric function runs on the device.
 * PER POINT (x, y) AND POSE, float32, no FMA, every operation rounded once, `/` the IEEE divide:
 *   ax = c*x - s*y;  ay = s*x + c*y;  rx = ax + tx;  ry = ay + ty                       (E15's positions)
 *   hu = ((rx - origin_x) / resolution) * 256.0f - 128.0f;  hv likewise from ry and origin_y
 *   lx = ax / resolution;  ly = ay / resolution                                       (the lever about the base, cells)
 * The point is DROPPED for this pose unless |hu| < 2^28, |hv| < 2^28, |lx| < 8192 and |ly| < 8192 (a NaN fails all
 * four): it contributes nothing, counts in word 28 and sets RPLGPU_SCAN_CELL_RANGE in d_status[g].  From here on
 * integers:
 *   U = (int)floorf(hu);  i0 = U >> 8 (arithmetic);  a = U & 255;   V_, j0, b likewise from hv
 *   Lx = (int)rintf(lx * 16.0f);  Ly likewise                      (ties to even; |L| <= 2^17)
 *   m(ix, iy) = max((int8)field[iy * width + ix], 0), 0 outside [0, width) x [0, height)   (field g_f as E15)
 *   m00 = m(i0, j0), m10 = m(i0+1, j0), m01 = m(i0, j0+1), m11 = m(i0+1, j0+1)
 *   V  = (256-a)(256-b) m00 + a (256-b) m10 + (256-a) b m01 + a b m11           (Q16, 0 .. 127 * 65536)
 *   Gx = (256-b)(m10 - m00) + b (m11 - m01);  Gy = (256-a)(m01 - m00) + a (m11 - m10)   (Q8 per cell, |G| < 2^15)
 *   Gt = Gy * Lx - Gx * Ly                                                      (Q12 per radian, |Gt| < 2^33)
 *   E  = target * 65536 - V                                                     (|E| < 2^23)
 * Cell centres are the interpolation nodes (the -128): a point on a cell centre has a = b = 0 and V = 65536 m00.
 * SUMS: RPLGPU_REFINE_WORDS = 32 uint32 per pose at d_sums + g * sums_stride + 32 q (sums_stride in words, >= 32 P
 * and a multiple of 4, d_sums 16-byte aligned), little-endian two's complement; with the 2^24 points a group can have:
 *   words   value    width  bound        words   value    width  bound
 *   0 - 1   S Gx^2   u64    2^54         12 - 14 S Gx Gt  i96    2^72
 *   2 - 3   S Gx Gy  i64    2^54         15 - 17 S Gy Gt  i96    2^72
 *   4 - 5   S Gy^2   u64    2^54         18 - 20 S Gt^2   u96    2^90
 *   6 - 7   S Gx E   i64    2^62         21 - 23 S Gt E   i96    2^80
 *   8 - 9   S Gy E   i64    2^62         24 - 26 S E^2    u96    2^70
 *   10 - 11 S V      u64    2^47         27 n, the points that contributed;  28 the dropped points;  29 - 31 zero
 * One point can push S Gt^2 past 2^64.  A group without points has 32 zero words per pose; words at and beyond 32 P
 * of a group are never changed.
 * STEP, fp64, every operation below rounded once, none fused.  d64(v) is the IEEE conversion of a 64-bit value (signed
 * or unsigned as the table says); d96(w0, w1, w2) = ((double)w2 * 2^32 + (double)w1) * 2^32 + (double)w0 with w2 read
 * as int32 for i96 and uint32 for u96, w1 and w0 as uint32.  Scalings by powers of two (exact):
 *   a11 = d(S Gx^2) 2^-16;  a12 = d(S Gx Gy) 2^-16;  a22 = d(S Gy^2) 2^-16;  a13 = d(S Gx Gt) 2^-20;
 *   a23 = d(S Gy Gt) 2^-20;  a33 = d(S Gt^2) 2^-24;  g1 = d(S Gx E) 2^-24;  g2 = d(S Gy E) 2^-24;  g3 = d(S Gt E) 2^-28
 *   aii = aii + (double)damping * aii                                            (i = 1, 2, 3)
 *   c11 = a22*a33 - a23*a23;  c12 = a13*a23 - a12*a33;  c13 = a12*a23 - a13*a22;
 *   c22 = a11*a33 - a13*a13;  c23 = a12*a13 - a11*a23;  c33 = a11*a22 - a12*a12;
 *   det = (a11*c11 + a12*c12) + a13*c13
 *   dx = ((c11*g1 + c12*g2) + c13*g3) / det;  dy = ((c12*g1 + c22*g2) + c23*g3) / det;
 *   dt = ((c13*g1 + c23*g2) + c33*g3) / det                                      (dx, dy in cells, dt in rad)
 * NO STEP, the pose copied bit for bit and the step words 0: n < min_points (RPLGPU_REFINE_FEW), else det not > 0 or
 * not finite, or one of dx, dy, dt not finite (RPLGPU_REFINE_SINGULAR).  Otherwise RPLGPU_REFINE_STEPPED, and dx, dy
 * are clamped to +-(double)max_step_cells (RPLGPU_REFINE_CLAMP_X / _Y), dt to +-(double)max_rot (RPLGPU_REFINE_CLAMP_T);
 *   h = 0.5*dt;  hh = h*h;  den = 1.0 + hh;  dc = (1.0 - hh) / den;  ds = (h + h) / den
 * is the exact rotation by 2 atan h, (1, 0) for dt = 0.  Then in float32, no FMA, as E16's move, with fc = (float)dc,
 * fs = (float)ds, mx = (float)(dx * (double)resolution), my likewise:
 *   c' = c*fc - s*fs;  s' = s*fc + c*fs;  tx' = tx + mx;  ty' = ty + my;   a NaN is stored as 0x7FC00000.
 * STEP WORDS (optional), four per pose at d_step + g * step_stride + 4 q: the bits of mx, my, (float)dt, and the flags.
 * RESULT, eight words per group at d_result + 8 g: 0 the poses stepped, 1 not stepped for too few points, 2 not
 * stepped for singular or not finite, 3 the poses with a clamp (the step's words; 0 after rplgpu_refine_sums_dev
 * alone); 4 the smallest q with the greatest S V, 5 and 6 that S V low and high, 7 the group's finite points (the
 * sums' words; rplgpu_refine_step_dev leaves them alone). */
#define RPLGPU_REFINE_WORDS    32u
#define RPLGPU_REFINE_PLANES   29u   /* the 64-bit scratch planes per pose: one per live word of the sums */
#define RPLGPU_REFINE_MAX_ITERS 16u
#define RPLGPU_REFINE_STEPPED  0x01u
#define RPLGPU_REFINE_FEW      0x02u
#define RPLGPU_REFINE_SINGULAR 0x04u
#define RPLGPU_REFINE_CLAMP_X  0x08u
#define RPLGPU_REFINE_CLAMP_Y  0x10u
#define RPLGPU_REFINE_CLAMP_T  0x20u
typedef struct rplgpu_pose_refine {
  float    origin_x, origin_y;   /* the field's grid: as rplgpu_pose_score_t */
  float    resolution;
  uint32_t width, height;        /* 1 .. RPLGPU_MAX_OCC_DIM */
  uint32_t target;               /* 1 .. 127: the field value a perfectly placed point has */
  float    damping;              /* >= 0: aii += damping * aii (Levenberg-Marquardt's diagonal) */
  float    max_step_cells;       /* > 0: the clamp of dx and dy */
  float    max_rot;              /* rad, > 0: the clamp of dt */
  uint32_t min_points;           /* >= 3 */
} rplgpu_pose_refine_t;
/* E11's default grid, target 127, damping 0, max_step_cells 2, max_rot 0.1, min_points 16 */
void rplgpu_default_pose_refine(rplgpu_pose_refine_t *r);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, everything rplgpu_pose_score_check refuses in
 * the grid, a target of 0 or above 127, a damping that is negative or not finite, a max_step_cells or max_rot that is
 * not > 0 or not finite, min_points below 3.  The device path uses this function. */
int32_t rplgpu_pose_refine_check(const rplgpu_pose_refine_t *r);
/* Host only.  The uint32 words of scratch a call over G groups of P poses takes: 2 * RPLGPU_REFINE_PLANES * G * P
 * (one 64-bit word per pose and live word of the sums: the kernel adds 32-bit limbs into 64-bit planes, so no carry
 * crosses an atomic); 0 for G = 0, P = 0 or P above RPLGPU_MAX_POSES. */
uint64_t rplgpu_refine_scratch_words(uint32_t G, uint32_t P);
/* Host only: the SUMS of ONE group in plain C++ over n points already in the base frame (a point that is not finite
 * is ignored), for P poses of four floats; sums_out: 32 P words, written whole; result (optional): the eight words
 * with 0 - 3 zero; status (optional): RPLGPU_SCAN_CELL_RANGE or 0.  RPLGPU_ERR_INVALID_ARG and nothing written for a
 * spec the check refuses, a NULL pointer, P = 0 or above RPLGPU_MAX_POSES, n above 2^24. */
int32_t rplgpu_refine_sums_host(const float *x, const float *y, uint32_t n, const float *poses, uint32_t P,
                                const int8_t *field, const rplgpu_pose_refine_t *r, uint32_t *sums_out,
                                uint32_t result[8], uint32_t *status);
/* Host only: the STEP of ONE pose in plain C++, the sequence above operation for operation (the device runs the same
 * sequence through __dmul_rn / __dadd_rn / __ddiv_rn).  sums: 32 words; pose_out may be pose; step (optional): the
 * four step words.  Returns the flags, or RPLGPU_ERR_INVALID_ARG (negative) and nothing written for a spec the check
 * refuses or a NULL pointer. */
int32_t rplgpu_refine_step_host(const uint32_t sums[32], const rplgpu_pose_refine_t *r, const float pose[4],
                                float pose_out[4], uint32_t step[4]);
/* Host only: the covariance Hector and Karto publish with a match.  A = the matrix of STEP without the damping;
 * cov9 = S A^-1 S row-major over (x, y, theta) with S = diag(resolution, resolution, 1): metres and radians.  fp64,
 * the cofactors and det of STEP.  RPLGPU_ERR_INVALID_ARG and nine zeros for a det that is not > 0 or not finite;
 * RPLGPU_ERR_INVALID_ARG and nothing written for a spec the check refuses or a NULL pointer. */
int32_t rplgpu_refine_covariance(const uint32_t sums[32], const rplgpu_pose_refine_t *r, double cov9[9]);
/* The SUMS on the handle's stream: E15's arguments with the new spec, d_sums / sums_stride as above, d_result eight
 * words a group (words 0 - 3 zeroed), d_status optional (RPLGPU_SCAN_OUT_TRUNCATED and RPLGPU_SCAN_CELL_RANGE, cleared
 * on the stream by the call).  SCRATCH is the caller's: rplgpu_refine_scratch_words(G, P) uint32 words at d_scratch,
 * 8-byte aligned, cleared by the call's own prepare launch; words beyond it are never touched.  The field and the
 * poses are only read.  RPLGPU_ERR_INVALID_ARG for everything rplgpu_score_poses_dev refuses (the spec by
 * rplgpu_pose_refine_check, sums for weights), a missing d_scratch or one not 8-byte aligned, a d_sums not 16-byte
 * aligned.  A refused call changes no output.  Asynchronous on the handle's stream. */
int32_t rplgpu_refine_sums_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                               const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                               const float *d_motion, const float *d_pose2d, const rplgpu_pose_refine_t *r,
                               const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                               const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group,
                               uint32_t *d_sums, uint64_t sums_stride, uint32_t *d_scratch, uint32_t *d_result,
                               uint32_t *d_status);
/* The STEP of G groups of P poses: pose q of group g is read as above, its sums at d_sums + g * sums_stride + 32 q,
 * and the stepped pose goes to d_poses_out + g * out_stride + 4 q (out_stride in floats, >= 4 P and a multiple of 4,
 * 16-byte aligned), the step words (optional) to d_step + g * step_stride + 4 q (step_stride >= 4 P words), result
 * words 0 - 3 to d_result + 8 g.  d_poses_out == d_poses is allowed, element-wise, when out_stride == pose_stride
 * and every group reads its own list (poses_per_group not 0, or G = 1); any other overlap of the two is refused.
 * RPLGPU_ERR_INVALID_ARG also for a spec the check refuses, G = 0 or above 65535, P = 0 or above RPLGPU_MAX_POSES, a
 * missing or misaligned pointer and the stride rules.  A refused call changes no output.  Asynchronous. */
int32_t rplgpu_refine_step_dev(rplgpu_handle_t h, const uint32_t *d_sums, uint64_t sums_stride,
                               const rplgpu_pose_refine_t *r, const float *d_poses, uint64_t pose_stride,
                               uint32_t poses_per_group, uint32_t G, uint32_t P, float *d_poses_out,
                               uint64_t out_stride, uint32_t *d_step, uint64_t step_stride, uint32_t *d_result);
/* `iters` rounds (1 .. RPLGPU_REFINE_MAX_ITERS) of SUMS + STEP queued on the stream with no read in between: round
 * 0 reads d_poses, every later round the list the round before left in d_poses_out (every group its own).  Behind
 * the call d_sums, d_step and d_result are the LAST round's (so the sums are those of the list BEFORE the last step)
 * and d_poses_out is the final list; d_status collects every round.  iters = 1 is exactly rplgpu_refine_sums_dev
 * followed by rplgpu_refine_step_dev.  The refusals of both; a refused call changes no output. */
int32_t rplgpu_refine_poses_dev(rplgpu_handle_t h, const rplgpu_node_t *d_nodes, uint32_t n_stride,
                                const uint32_t *d_n_per_scan, uint32_t B, uint32_t group, const rplgpu_params_t *p,
                                const float *d_motion, const float *d_pose2d, const rplgpu_pose_refine_t *r,
                                const float *d_poses, uint32_t P, uint64_t pose_stride, uint32_t poses_per_group,
                                const int8_t *d_field, uint64_t field_stride, uint32_t field_per_group,
                                uint32_t iters, float *d_poses_out, uint64_t out_stride, uint32_t *d_sums,
                                uint64_t sums_stride, uint32_t *d_step, uint64_t step_stride, uint32_t *d_scratch,
                                uint32_t *d_result, uint32_t *d_status);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), shaped as rplgpu_score_poses: poses 4 P floats;
 * poses_out: 4 P floats; sums_out (optional): 32 P words; step_out (optional): 4 P words; result: 8 words; status
 * (optional).  Allocates its device buffers per call and returns when the results are in place. */
int32_t rplgpu_refine_poses(rplgpu_handle_t h, const rplgpu_node_t *nodes, uint32_t n_stride,
                            const uint32_t *n_per_scan, uint32_t n_scans, const rplgpu_params_t *p,
                            const float *motion, const float *pose2d, const float *t0,
                            const rplgpu_pose_refine_t *r, const float *poses, uint32_t P, const int8_t *field,
                            uint32_t iters, float *poses_out, uint32_t *sums_out, uint32_t *step_out,
                            uint32_t result[8], uint32_t *status);
/* JOINING E13 / E24: the eight result words of group g at d_best + 8 g become ONE pose (c', s', x', y') at
 * d_poses_out + g * out_stride (out_stride in floats, >= 4 and a multiple of 4, 16-byte aligned): a list of P = 1 with
 * poses_per_group = 1.  `m` is a checked rplgpu_scan_match_t: its resolution, K and the table
 * of rplgpu_scan_match_rotations are used.  The base prior (c0, s0, x0, y0) = the four floats at d_prior + 4 g, or
 * (1, 0, px, py) when d_prior is NULL; (px, py) = d_pivot[2g], d_pivot[2g + 1], (0, 0) when NULL; (k, j, i) words
 * 1 - 3, (c, s) the table's entry k.  E13's APPLYING IT in float32, no FMA, in this order:
 *   c' = c*c0 - s*s0;  s' = s*c0 + c*s0;  qx = x0 - px;  qy = y0 - py;
 *   x' = ((c*qx - s*qy) + px) + (float)i * resolution;  y' = ((s*qx + c*qy) + py) + (float)j * resolution
 * A k outside [-K, K] keeps the prior, bit for bit.  RPLGPU_ERR_INVALID_ARG for a spec the check refuses, G = 0 or
 * above 65535, a missing d_best / d_poses_out, a misaligned pointer, the stride rule.  A refused call changes nothing. */
int32_t rplgpu_match_poses_dev(rplgpu_handle_t h, const uint32_t *d_best, const rplgpu_scan_match_t *m,
                               const float *d_pivot, const float *d_prior, uint32_t G, float *d_poses_out,
                               uint64_t out_stride);
/* JOINING E11 / E14: pose q_g of group g's list, (c, s, x, y) at d_poses + g_p * pose_stride + 4 q_g, composed in
 * front of every mount pose of the group.  q_g = q when d_result is NULL, else word 4 of d_result + 8 g (E25's best
 * pose); a q_g >= P copies the mount poses unchanged.  For scan sc of group g (group clamped to B) with the mount
 * (r00 r01 tx r10 r11 ty) = d_pose2d_in + 6 sc (NULL: identity), float32, no FMA:
 *   r00' = c*r00 - s*r10;  r01' = c*r01 - s*r11;  r10' = s*r00 + c*r10;  r11' = s*r01 + c*r11;
 *   tx' = (c*tx - s*ty) + x;  ty' = (s*tx + c*ty) + y
 * go to d_pose2d_out + 6 sc, the poses rplgpu_map_update_dev and rplgpu_occupancy_grid_dev take.  d_pose2d_out ==
 * d_pose2d_in is allowed (element-wise).  RPLGPU_ERR_INVALID_ARG for group = 0, P = 0 or above RPLGPU_MAX_POSES, a
 * missing d_poses / d_pose2d_out, a misaligned pointer, the E15 stride rules; RPLGPU_ERR_CAPACITY for B above the
 * handle's max_batch.  A refused call changes nothing.  Asynchronous on the handle's stream. */
int32_t rplgpu_compose_poses_dev(rplgpu_handle_t h, const float *d_poses, uint64_t pose_stride,
                                 uint32_t poses_per_group, uint32_t P, const uint32_t *d_result, uint32_t q,
                                 const float *d_pose2d_in, uint32_t B, uint32_t group, float *d_pose2d_out);

/* ---- E26: a cost-to-goal field over a costmap, and the paths down it (row 4; the first reader of E12 as a costmap) ----
 * E12 makes the costmap every planner starts from; E13 - E25 read an int8 grid only as a likelihood field.  This is
 * the step a costmap's user takes next: the navigation function of NavFn / global_planner — the least cost from every
 * cell to a goal, Dijkstra over the costmap — and the path that follows it downhill.  Nothing in the reference plans,
 * so these rules ARE the definition (parity unpinned, as E5-E25).  Everything is integers: the field is the one
 * solution of a min-plus fixed-point equation, depends on no order and is held to its oracle byte for byte.
 *
 * CELL WEIGHT of input byte v (int8, E11's layout, cell (cx, cy) at cy * width + cx):
 *   v >= lethal: impassable;   0 <= v < lethal: w = neutral + factor * v;
 *   v < 0: w = unknown_cost, impassable when that is 0.          Every passable w is in 1 .. RPLGPU_NAV_MAX_COST.
 * STEPS, numbered 0 .. 7 as (dx, dy) with the factor k:
 *   0 (+1, 0)  1 (-1, 0)  2 (0, +1)  3 (0, -1)   k = 5;      4 (+1, +1)  5 (-1, +1)  6 (+1, -1)  7 (-1, -1)   k = 7
 * A step from c to its neighbour n inside the grid is ALLOWED when c is passable; a diagonal one also needs both
 * cells it passes between, (cx + dx, cy) and (cx, cy + dy), passable by their bytes (no corner cutting).  n's own
 * byte does not matter.
 * FIELD D, one uint32 per cell, RPLGPU_NAV_UNREACHED = 0xFFFFFFFF:
 *   D = 0 at every goal cell, whatever its byte;
 *   otherwise D(c) = min over the allowed steps c -> n with D(n) reached of D(n) + k * w(c) if that is <= cap, else
 *   UNREACHED (so an impassable cell that is no goal is UNREACHED).
 * Every w >= 1, so there is exactly one solution: the least path cost to a goal, cut at cap (consistently: every
 * cell further along a least path has a smaller value).  Nothing overflows: cap + 7 * 2047 < 2^32.
 * GOALS per grid g: d_n_goals[g] cell indices (cy * width + cx) at d_goals + g * goal_stride, in device memory; of
 * these the first RPLGPU_NAV_MAX_GOALS = 1024 are read.  An index >= width * height, and every index beyond the
 * first 1024, is IGNORED and counted; an index in range is TAKEN and counted, duplicates each time.  No goal taken:
 * everything UNREACHED.
 * PATH from a start cell c0: while D(c) != 0, step to the allowed neighbour n of LOWEST step number with D(n) reached
 * and D(n) + k * w(c) == D(c).  D falls strictly, so the walk ends, and the cells written cost exactly D(c0).  The
 * cells' indices go to the path's words, c0 first.  Four INFO words a path: 0 the cells written (start and goal
 * included), 1 the flags, 2 D(c0) (UNREACHED under NO_START), 3 the last cell written (the start index as given when
 * none was).  Flags, one of:
 *   RPLGPU_NAV_PATH_REACHED    the last cell written has D = 0
 *   RPLGPU_NAV_PATH_NO_START   the index is >= width * height; nothing written
 *   RPLGPU_NAV_PATH_UNREACHED  D(c0) is UNREACHED; nothing written
 *   RPLGPU_NAV_PATH_TRUNCATED  max_len cells written and the last has D != 0
 *   RPLGPU_NAV_PATH_BROKEN     no neighbour satisfies the equality at the last cell written: only when the potential
 *                              is not the finished field of this grid and spec
 * Words of a path at and beyond its length are never changed.
 * TILES: RPLGPU_NAV_TILE = 64 cells a side, ntx = ceil(width / 64), nty = ceil(height / 64); tile (tx, ty) of a grid
 * is tile ty * ntx + tx.  The device relaxes tile by tile, one launch a ROUND; a tile is DIRTY when a word it reads
 * may have changed since it last ran. */
#define RPLGPU_NAV_TILE        64u
#define RPLGPU_NAV_MAX_COST    2047u
#define RPLGPU_NAV_MAX_CAP     0xFFFF0000u
#define RPLGPU_NAV_MAX_ROUNDS  4096u
#define RPLGPU_NAV_MAX_GOALS   1024u
#define RPLGPU_NAV_MAX_STARTS  65536u
#define RPLGPU_NAV_MAX_TILES   0x800000u   /* G * ntx * nty of one call: a round's launch stays below 2^32 threads */
#define RPLGPU_NAV_UNREACHED   0xFFFFFFFFu
#define RPLGPU_NAV_UNFINISHED  0x01u   /* result word 1: dirty tiles are left, the field is not the answer yet */
#define RPLGPU_NAV_PATH_REACHED    0x01u
#define RPLGPU_NAV_PATH_NO_START   0x02u
#define RPLGPU_NAV_PATH_UNREACHED  0x04u
#define RPLGPU_NAV_PATH_TRUNCATED  0x08u
#define RPLGPU_NAV_PATH_BROKEN     0x10u
typedef struct rplgpu_nav_field {
  uint32_t width, height;   /* 1 .. RPLGPU_MAX_OCC_DIM */
  uint32_t lethal;          /* 1 .. 100: bytes at and above it are impassable */
  uint32_t neutral;         /* 1 .. 255: the weight of a free cell */
  uint32_t factor;          /* 0 .. 16: the weight added per cost unit */
  uint32_t unknown_cost;    /* 0: unknown is impassable; else 1 .. RPLGPU_NAV_MAX_COST */
  uint32_t cap;             /* 0 .. RPLGPU_NAV_MAX_CAP: values above it are UNREACHED */
  uint32_t rounds;          /* 1 .. RPLGPU_NAV_MAX_ROUNDS: the launches one call queues */
} rplgpu_nav_field_t;
/* 1024 x 1024, lethal 99, neutral 50, factor 2, unknown_cost 0, cap RPLGPU_NAV_MAX_CAP, rounds
 * rplgpu_nav_field_default_rounds(1024, 1024) */
void rplgpu_default_nav_field(rplgpu_nav_field_t *f);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, a value outside the ranges above, and
 * neutral + factor * (lethal - 1) > RPLGPU_NAV_MAX_COST.  The device path uses this function. */
int32_t rplgpu_nav_field_check(const rplgpu_nav_field_t *f);
/* Host only: 2 * (ntx + nty) + 2, enough for a field whose least paths cross every tile border once in each
 * direction; 0 for a width or height outside 1 .. RPLGPU_MAX_OCC_DIM.  A maze needs more: resume. */
uint32_t rplgpu_nav_field_default_rounds(uint32_t width, uint32_t height);
/* Host only: the uint32 words of scratch rplgpu_nav_field_dev takes for G grids, 2 * ntx * nty * G (two planes of
 * one dirty word per tile); 0 for a spec the check refuses, G = 0 or G * ntx * nty above RPLGPU_NAV_MAX_TILES. */
uint64_t rplgpu_nav_field_scratch_words(const rplgpu_nav_field_t *f, uint32_t G);
/* Host only: the FIELD of ONE grid by a binary-heap Dijkstra from the goals, the definition a reader can run.
 * goals: n_goals indices (NULL with 0); potential: width * height words, written whole; result (optional): the
 * eight words below with 0, 1, 6 and 7 zero.  `rounds` is not used.  RPLGPU_ERR_INVALID_ARG and nothing written for
 * a spec the check refuses or a NULL pointer. */
int32_t rplgpu_nav_field_host(const rplgpu_nav_field_t *f, const int8_t *grid, const uint32_t *goals,
                              uint32_t n_goals, uint32_t *potential, uint32_t result[8]);
/* Host only: ONE PATH down `potential` in plain C++; path: max_len words (>= 1), info: the four words.  Returns the
 * flags, or RPLGPU_ERR_INVALID_ARG (negative) and nothing written for a spec the check refuses, a NULL pointer or
 * max_len = 0. */
int32_t rplgpu_nav_path_host(const rplgpu_nav_field_t *f, const int8_t *grid, const uint32_t *potential,
                             uint32_t start, uint32_t *path, uint32_t max_len, uint32_t info[4]);
/* The FIELD of G grids on the handle's stream: grid g at d_grid + g * grid_stride (E12's rules: the stride >= width
 * * height and a multiple of 4, the pointer 4-byte aligned; only read), its field at d_potential + g *
 * potential_stride (words; >= width * height; 4-byte aligned; words at and beyond width * height of a grid are never
 * changed), its goals as above (goal_stride in words, >= 1), d_n_goals G words.  The call queues an init launch, the
 * goals (which mark dirty every tile that reads a goal cell, its neighbours across a tile border too), `rounds` rounds
 * and two closing launches with no host round trip; no workgroup ever waits for another, and
 * a round's tile that is not dirty leaves at once.  resume = 0 starts afresh.  resume = 1 continues from d_potential
 * and from the dirty words a previous call with the SAME arguments left in d_scratch — THE ONE STAGE WHOSE SCRATCH
 * HOLDS SOMETHING A SECOND CALL RELIES ON: between such calls the caller leaves d_scratch, d_potential, the grid and
 * the goals alone.  A finished field resumed stays byte-identical.
 * RESULT, eight words per grid at d_result + 8 g: 0 the dirty tiles left (0 = finished), 1 the flags
 * (RPLGPU_NAV_UNFINISHED), 2 the goals taken, 3 the goals ignored, 4 the reached cells, 5 the greatest reached D
 * (0 when none), 6 the tile visits of this call, 7 the rounds of this call that had a dirty tile.  4 and 5 describe
 * d_potential as the call left it.  While a field is unfinished, words 4 - 7 and the field itself are not defined
 * byte for byte; only this is: every word is UNREACHED or >= the answer.  6 and 7 depend on the schedule even for a
 * finished field.
 * RPLGPU_ERR_INVALID_ARG for a spec the check refuses, G = 0 or above 65535, a missing or misaligned pointer, the
 * stride rules, resume above 1; RPLGPU_ERR_CAPACITY for G * ntx * nty above RPLGPU_NAV_MAX_TILES
 * = 2^23, before anything is queued.  A refused call changes no output.
 * Asynchronous on the handle's stream; nothing is stored on the handle. */
int32_t rplgpu_nav_field_dev(rplgpu_handle_t h, const rplgpu_nav_field_t *f, const int8_t *d_grid,
                             uint64_t grid_stride, uint32_t G, const uint32_t *d_goals, uint64_t goal_stride,
                             const uint32_t *d_n_goals, uint32_t *d_potential, uint64_t potential_stride,
                             uint32_t *d_scratch, uint32_t resume, uint32_t *d_result);
/* S PATHS per grid (1 .. RPLGPU_NAV_MAX_STARTS), one thread a path (a dependent chain of neighbour reads: not the
 * hot path): the start of path s of grid g at d_starts[g * S + s], its cells at d_paths + (g * S + s) * max_len,
 * its info at d_info + 4 (g * S + s).  The grid and the potential are only read.  RPLGPU_ERR_INVALID_ARG for a spec
 * the check refuses, G = 0 or above 65535, S out of range, max_len = 0, a missing or misaligned (4-byte) pointer,
 * the stride rules of rplgpu_nav_field_dev.  A refused call changes no output.  Asynchronous. */
int32_t rplgpu_nav_paths_dev(rplgpu_handle_t h, const rplgpu_nav_field_t *f, const int8_t *d_grid,
                             uint64_t grid_stride, const uint32_t *d_potential, uint64_t potential_stride,
                             uint32_t G, const uint32_t *d_starts, uint32_t S, uint32_t *d_paths, uint32_t max_len,
                             uint32_t *d_info);
/* ONE grid, HOST buffers (the node-side door, rplgpu_host.hpp): allocates its device buffers per call, calls
 * rplgpu_nav_field_dev with resume until the field is finished or 64 calls have passed, and returns when the results
 * are in place.  potential: width * height words; result: 8 words, 6 and 7 summed over the calls.  starts (optional,
 * S of them): with them paths (S * max_len words, copied in first so that words beyond a path stay) and info (4 S
 * words) are required. */
int32_t rplgpu_nav_field(rplgpu_handle_t h, const rplgpu_nav_field_t *f, const int8_t *grid, const uint32_t *goals,
                         uint32_t n_goals, uint32_t *potential, uint32_t result[8], const uint32_t *starts,
                         uint32_t S, uint32_t *paths, uint32_t max_len, uint32_t *info);

/* ---- E27: candidate motions rolled out of a pose and scored (row 4; the first reader of E26's field) ----
 * E11 -> E12 -> E26 end in a costmap and a cost-to-goal field D; the local planner is what reads both.  DWB / DWA rolls
 * constant-velocity arcs out of the current pose and scores them by the worst cost under the footprint along the arc
 * (ObstacleFootprint) and by look-ups into the field (GoalDist / PathDist); MPPI does the same with noisy control
 * sequences, which E18 already writes on the device.  The roll's step is E16's MOVE, the look-up E15's transform and
 * E11's CELL.  Nothing in the reference plans or controls, so these rules ARE the definition (parity unpinned, as
 * E5-E26).  float32 operations, each rounded once, no FMA, IEEE divides; after the cell rule everything is integers:
 * the result depends on no order.
 *
 * START of group g: four floats (c, s, x, y) at d_start + 4 g_s, E15's pose form; g_s = g when start_per_group is
 * not 0, else 0; 16-byte aligned.  Any values are defined: the device evaluates no trigonometric function and does
 * not renormalise.
 * DELTAS: four floats (dc, ds, dx, dy) each, E16 / E18's layout, at d_delta + g_d * delta_stride (g_d = g when
 * delta_per_group is not 0, else 0; 16-byte aligned; delta_stride in floats and a multiple of 4).
 *   delta_per_step = 0: candidate k has the ONE delta at 4 k and applies it T times (an arc); delta_stride >= 4 K.
 *   delta_per_step = 1: step t (1-based) of candidate k uses the delta at 4 (k T + t - 1) (a control sequence);
 *   delta_stride >= 4 K T.  This is the output of rplgpu_sample_motion_dev with M = K T.
 * ROLL: pose_0 is the start; pose_t = pose_(t-1) composed with the delta on the right by E16's MOVE, operation for
 * operation:  c' = c*dc - s*ds;  s' = s*dc + c*ds;  x' = (c*dx - s*dy) + x;  y' = (s*dx + c*dy) + y;  a NaN result
 * is 0x7FC00000.  The composition is sequential by definition (float rounding is not associative).
 * FOOTPRINT: F points (fx, fy), 1 <= F <= RPLGPU_ROLLOUT_MAX_FOOTPRINT, two floats each at d_footprint (8-byte
 * aligned), one list for the whole call, in the base frame; (0, 0) alone is "the centre".  At pose t a point is at
 *   rx = (c*fx - s*fy) + x;   ry = (s*fx + c*fy) + y
 * and its cell is E11's CELL in the spec's grid.  Its VALUE p:
 *   no cell (NaN, Inf, a magnitude >= 1048576 cells): BLOCKED, and the point is OFF RANGE;
 *   a cell outside [0, width) x [0, height): BLOCKED;
 *   else v = (int8)d_grid[g_c * grid_stride + cy * width + cx] (E12's output layout, E26's stride rules; g_c = g
 *   when grid_per_group is not 0, else 0);  p = v for v >= 0, else unknown_value;  p >= lethal is BLOCKED.
 * Pose t is BLOCKED when any of its points is; else m_t = the max of p over its points.
 * CANDIDATE: n = the number of poses before the first blocked one among t = 1 .. T (T when none); poses behind n
 * contribute nothing.  cost_sum = the sum of m_t over t = 1 .. n, cost_max their max (0 when n = 0).  The CENTRE of
 * pose t is the cell of (x_t, y_t) itself; D_t = the word of d_potential (E26's layout: d_potential + g_c *
 * potential_stride) at that cell, RPLGPU_NAV_UNREACHED without a cell or outside the grid.  D_end = D_n, D_min = the
 * min of D_t over t = 1 .. n, both UNREACHED when n = 0; with d_potential NULL both are 0 whatever n.
 *   FLAGS: RPLGPU_ROLLOUT_BLOCKED n < T;  RPLGPU_ROLLOUT_CELL_RANGE n < T and a point of pose n + 1, the first
 *   blocked one, is off range;  RPLGPU_ROLLOUT_END_UNREACHED d_potential given and D_end UNREACHED;
 *   RPLGPU_ROLLOUT_ADMISSIBLE n >= min_steps and not END_UNREACHED.
 *   SCORE, uint64: a_end*D_end + a_min*D_min + a_sum*cost_sum + a_max*cost_max (below 2^50) when admissible (D_min
 *   is then reached, because D_n is among its terms), else 2^64 - 1.
 * OUTPUT, eight words per candidate at d_out + g * out_stride + 8 k (out_stride in words, >= 8 K and a multiple of
 * 4; 16-byte aligned): 0 n, 1 the flags, 2 cost_sum, 3 cost_max, 4 D_end, 5 D_min, 6 and 7 the score, low and high.
 * pose_n (the start's 16 bytes bit for bit when n = 0) goes to d_end_poses + g * end_stride + 4 k when that is given
 * (E15's list form, so that it chains: end_stride in floats, >= 4 K and a multiple of 4; 16-byte aligned).  Words at
 * and beyond K of a group are never changed.
 * RESULT, eight words per group at d_result + 8 g: 0 the admissible candidates, 1 the smallest k with the lowest
 * score among them (RPLGPU_ROLLOUT_NONE when none), 2 and 3 that score (all ones when none), 4 how many admissible
 * candidates have it (0 when none), 5 the candidates with BLOCKED, 6 those with CELL_RANGE, 7 flags (bit 0: none is
 * admissible).
 * AN IDENTITY that holds independent code to each other: with a footprint that is never blocked, d_end_poses of
 * (T, delta_per_step = 0) equals T chained calls of E16's move (rplgpu_resample_poses_dev with P = 1, weight 1,
 * M = K, n_delta = M; likewise rplgpu_resample_host), byte for byte. */
#define RPLGPU_ROLLOUT_MAX_STEPS      256u
#define RPLGPU_ROLLOUT_MAX_FOOTPRINT   64u
#define RPLGPU_ROLLOUT_MAX_WEIGHT   65535u
#define RPLGPU_ROLLOUT_NONE    0xFFFFFFFFu
#define RPLGPU_ROLLOUT_TILE            32u   /* candidates a workgroup takes: one scratch record each */
#define RPLGPU_ROLLOUT_MAX_TILES 0x800000u   /* G * ceil(K / tile) of one call: the launch stays below 2^32 threads */
#define RPLGPU_ROLLOUT_BLOCKED        0x1u
#define RPLGPU_ROLLOUT_CELL_RANGE     0x2u
#define RPLGPU_ROLLOUT_END_UNREACHED  0x4u
#define RPLGPU_ROLLOUT_ADMISSIBLE     0x8u
typedef struct rplgpu_rollout {
  float    origin_x, origin_y, resolution;  /* the costmap's grid, as rplgpu_pose_score_t */
  uint32_t width, height;                   /* 1 .. RPLGPU_MAX_OCC_DIM */
  uint32_t lethal;         /* 1 .. 100: a value at or above it blocks (E26's meaning) */
  uint32_t unknown_value;  /* 0 .. 100: what a negative byte counts as; at or above lethal it blocks */
  uint32_t steps;          /* T, 1 .. RPLGPU_ROLLOUT_MAX_STEPS */
  uint32_t min_steps;      /* 1 .. T: unblocked poses a candidate needs to be admissible (T = DWB's rule) */
  uint32_t a_end, a_min, a_sum, a_max;  /* 0 .. RPLGPU_ROLLOUT_MAX_WEIGHT: the four critics' scales */
} rplgpu_rollout_t;
/* E11's grid (0.05 m, 1024 x 1024, origin (-25.6, -25.6)), lethal 99, unknown_value 100, steps 32, min_steps 32,
 * a_end 1, a_min 0, a_sum 1, a_max 0 */
void rplgpu_default_rollout(rplgpu_rollout_t *r);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL, a grid value that is not finite,
 * resolution <= 0, a value outside the ranges above, min_steps > steps.  The device path uses this function. */
int32_t rplgpu_rollout_check(const rplgpu_rollout_t *r);
/* Host only: the uint32 words of scratch the device call takes, 8 * ceil(K / RPLGPU_ROLLOUT_TILE) * G (a record of
 * eight words per workgroup); 0 for G = 0 or above 65535, a K outside 1 .. RPLGPU_MAX_POSES or G * ceil(K /
 * RPLGPU_ROLLOUT_TILE) above RPLGPU_ROLLOUT_MAX_TILES. */
uint64_t rplgpu_rollout_scratch_words(uint32_t G, uint32_t K);
/* Host only, a convenience that is NOT part of the byte-exact contract (as rplgpu_motion_odometry is not): K body
 * velocities (vx, vy, w), three doubles each, held for dt seconds become K deltas of four floats.  In fp64:
 * th = w dt, dc = cos th, ds = sin th; for |th| < 1e-9 dx = vx dt, dy = vy dt, else the exact arc
 * dx = (vx sin th - vy (1 - cos th)) / w, dy = (vx (1 - cos th) + vy sin th) / w; each value rounded once to float.
 * w = 0 gives exactly (1, 0, vx dt, vy dt).  RPLGPU_ERR_INVALID_ARG for a NULL pointer, K = 0 or above
 * RPLGPU_MAX_POSES. */
int32_t rplgpu_rollout_deltas(const double *vxyw, uint32_t K, double dt, float *delta_out);
/* Host only: the rules above in plain C++ for ONE group, the definition a reader can run.  start: 4 floats; delta:
 * 4 K floats, or 4 K T with delta_per_step = 1; footprint: 2 F floats; grid: width * height bytes; potential: NULL
 * or width * height words; out: 8 K words; end_poses (optional): 4 K floats; result: 8 words.
 * RPLGPU_ERR_INVALID_ARG and nothing written for a spec the check refuses, a NULL start / delta / footprint / grid /
 * out / result, K = 0 or above RPLGPU_MAX_POSES, K * T above 2^24, F outside 1 .. RPLGPU_ROLLOUT_MAX_FOOTPRINT,
 * delta_per_step above 1. */
int32_t rplgpu_rollout_host(const rplgpu_rollout_t *r, const float *start, const float *delta,
                            uint32_t delta_per_step, const float *footprint, uint32_t F, const int8_t *grid,
                            const uint32_t *potential, uint32_t K, uint32_t *out, float *end_poses,
                            uint32_t result[8]);
/* K candidates for each of G groups on the handle's stream: two launches (a workgroup per tile of
 * RPLGPU_ROLLOUT_TILE candidates of one group, then one workgroup per group that folds the tiles' records), no
 * workgroup waits for another, nothing is stored on the handle.  d_scratch: rplgpu_rollout_scratch_words of (G, K)
 * words, 16-byte aligned, the caller's; it holds nothing a later call relies on.  d_grid 4-byte aligned, grid_stride
 * >= width * height and a multiple of 4; d_potential NULL or 4-byte aligned with potential_stride >= width * height;
 * both only read, as the start, the deltas and the footprint are.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a spec the check refuses, G = 0 or above 65535,
 * K = 0 or above RPLGPU_MAX_POSES, K * T above 2^24, F outside 1 .. RPLGPU_ROLLOUT_MAX_FOOTPRINT, delta_per_step
 * above 1, a missing d_start / d_delta / d_footprint / d_grid / d_out / d_result / d_scratch, a misaligned pointer
 * (16 bytes: d_start, d_delta, d_out, d_end_poses, d_scratch; 8: d_footprint; 4: the others), the stride rules
 * above, and an output (d_out, d_end_poses, d_result, d_scratch) that overlaps an input or another output over the
 * ranges used; RPLGPU_ERR_CAPACITY for G * ceil(K / RPLGPU_ROLLOUT_TILE) above RPLGPU_ROLLOUT_MAX_TILES = 2^23.
 * Asynchronous on the handle's stream. */
int32_t rplgpu_rollout_dev(rplgpu_handle_t h, const rplgpu_rollout_t *r, const float *d_start,
                           uint32_t start_per_group, const float *d_delta, uint64_t delta_stride,
                           uint32_t delta_per_group, uint32_t delta_per_step, const float *d_footprint, uint32_t F,
                           const int8_t *d_grid, uint64_t grid_stride, const uint32_t *d_potential,
                           uint64_t potential_stride, uint32_t grid_per_group, uint32_t G, uint32_t K,
                           uint32_t *d_out, uint64_t out_stride, float *d_end_poses, uint64_t end_stride,
                           uint32_t *d_result, uint32_t *d_scratch);
/* ONE group, HOST buffers (the node-side door, rplgpu_host.hpp), arguments as rplgpu_rollout_host.  Allocates its
 * device buffers and scratch per call and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_rollout(rplgpu_handle_t h, const rplgpu_rollout_t *r, const float *start, const float *delta,
                       uint32_t delta_per_step, const float *footprint, uint32_t F, const int8_t *grid,
                       const uint32_t *potential, uint32_t K, uint32_t *out, float *end_poses, uint32_t result[8]);

/* ---- E28: rolled-out candidates weighed and blended into new controls (row 4; MPPI's update behind E27) ----
 * E18 draws noisy per-step deltas, E27 rolls K candidates of T steps and leaves eight words per candidate.  What MPPI
 * does next is a softmax-weighted mean of the candidates' controls, then new candidates around that mean.  E28 is
 * both on the device, so that spread -> E27 -> update -> spread runs on one stream with no read of a candidate.
 * Nothing in the reference plans or controls, so these rules ARE the definition (parity unpinned, as E5-E27).
 *
 * A. THE UPDATE (rplgpu_mppi_update_dev).  Inputs per group g: E27's d_out (eight words a candidate at d_out +
 * g * out_stride + 8 k, E27's stride rules), E27's eight result words at d_rollout_result + 8 g, the deltas E27 rolled
 * (d_delta / delta_stride / delta_per_group and the spec's delta_per_step exactly as E27 reads them; T_e = steps when
 * delta_per_step is 1, else 1; the entry of candidate k at step t, 0-based, is at 4 (k T_e + t)), a table of
 * table_len = N uint16 entries at d_table (2-byte aligned, one for all groups) and optionally a nominal sequence of
 * T_e deltas at d_nominal + g_n * nominal_stride (g_n = g when nominal_per_group is not 0, else 0; 16-byte aligned;
 * the stride in floats, >= 4 T_e and a multiple of 4).
 * WEIGHT of candidate k: w = 0 unless word 1 of the candidate has RPLGPU_ROLLOUT_ADMISSIBLE and bit 0 of word 7 of the
 * group's result is clear.  Otherwise s = the candidate's words 6, 7 and m = the result's words 2, 3, both uint64;
 * d = s - m, or 0 when s < m (any input is defined);  i = d >> shift;  the index is CLAMPED when i > N - 1;
 * w = table[min(i, N - 1)].  Nothing is exponentiated on the device: the temperature lives in the table
 * (rplgpu_mppi_table makes one), as E22's byte table carries its sensor model.
 * QUANTISATION of a delta (dc, ds, dx, dy): float32, every operation rounded once, no FMA, IEEE divide.
 *   h = ds / (1.0f + dc)  (the tangent of half the angle: E18's and E25's parametrisation, no trigonometric function)
 *   th = h * 1048576.0f;  tx = dx * xy_scale;  ty = dy * xy_scale
 * IN RANGE iff fabsf(t) < 8388608.0f for all three (NaN and +-Inf are not, nor is the half turn dc = -1);
 * H, X, Y = (int32) rintf(t), ties to even.
 * SUMS: per step t of T_e, over the candidates with w != 0 whose delta at t is in range, four exact integers
 * W_t = sum w, sum w H, sum w X, sum w Y (each below 2^59), int64 two's complement, low word first: eight words a
 * step at d_sums + g * sums_stride + 8 t (sums_stride in words, >= 8 T_e and a multiple of 4; 16-byte aligned).
 * FINISH per step, in fp64 with every operation rounded once ((double) of an int64 is one round to nearest even):
 *   W_t > 0:  hb = (sum w H / W_t) * 2^-20;  hh = hb * hb;  den = 1 + hh;
 *             dc = (float)((1 - hh) / den);  ds = (float)((hb + hb) / den)      (a unit vector without a square root)
 *             dx = (float)((sum w X / W_t) / (double)xy_scale);  dy likewise
 *   W_t = 0:  step t of d_nominal bit for bit, or (1, 0, 0, 0) when d_nominal is NULL.
 * T_e deltas go to d_nominal_out + g * nominal_out_stride + 4 t (E16's layout; 16-byte aligned; the stride in floats,
 * >= 4 T_e and a multiple of 4).  d_nominal_out may equal d_nominal with equal strides and nominal_per_group not 0 (or
 * G = 1): the finish reads step t before it writes step t.
 * d_weights (required): w of candidate k at d_weights + g * weight_stride + k, E15's layout (weight_stride >= K), so
 * that E16 can resample the candidates and E17 reduce their end poses with these weights.
 * RESULT, eight words per group at d_result + 8 g: 0 the candidates with w != 0;  1 the candidates that pass the
 * weight's gate and whose index was clamped;  2, 3 sum w;  4, 5 sum w^2 (below 2^52; N_eff = (sum w)^2 / sum w^2);
 * 6 the (candidate, step) entries not in range among candidates with w != 0;  7 flags: RPLGPU_MPPI_NO_WEIGHT word 0
 * is 0, RPLGPU_MPPI_OFF_RANGE word 6 is not 0, RPLGPU_MPPI_EMPTY_STEP some step had W_t = 0.
 * Words beyond K, 8 T_e and 4 T_e of a group are never changed.
 *
 * B. THE SPREAD (rplgpu_mppi_spread_dev): the next iteration's candidates.  T_n nominal deltas a group (A's output;
 * d_nominal + g_n * nominal_stride) and K x T noise deltas in E27's per-step layout (d_noise + g_z * noise_stride, the
 * output of rplgpu_sample_motion_dev with M = K T around the identity odometry (1, 0, 0, 1, 0, k1, kt, k2)):
 *   out[k][t] = nominal[min(t + shift, T_n - 1)] composed with noise[k][t]     (t 0-based; shift: the receding horizon)
 * by E16's MOVE operation for operation with the nominal delta as the pose; a NaN is stored as 0x7FC00000.  With
 * keep_first not 0, candidate 0 is the (shifted) nominal bit for bit.  The output (d_out + g * out_stride) is E27's
 * delta_per_step = 1 input.  d_out may equal d_noise with equal strides and noise_per_group not 0 (or G = 1).
 * AN IDENTITY that holds independent code to each other: without keep_first, step t of all candidates equals
 * rplgpu_resample_host with P = 1, the nominal step as the pose, weight 1, M = K, n_delta = M, byte for byte. */
#define RPLGPU_MPPI_MAX_SHIFT          49u
#define RPLGPU_MPPI_MAX_TABLE       65536u
#define RPLGPU_MPPI_MAX_SPREAD_SHIFT  256u
#define RPLGPU_MPPI_PER_LANE            8u   /* candidates a lane of the sums launch folds in registers */
#define RPLGPU_MPPI_MAX_BLOCKS   0x800000u   /* workgroups of one launch: it stays below 2^32 threads */
#define RPLGPU_MPPI_NO_WEIGHT         0x1u
#define RPLGPU_MPPI_OFF_RANGE         0x2u
#define RPLGPU_MPPI_EMPTY_STEP        0x4u
typedef struct rplgpu_mppi {
  float    xy_scale;        /* finite, > 0: quanta per metre of dx, dy (1024 = E17's quantum) */
  uint32_t shift;           /* 0 .. RPLGPU_MPPI_MAX_SHIFT: score units per table entry, as a power of two */
  uint32_t table_len;       /* N, 1 .. RPLGPU_MPPI_MAX_TABLE */
  uint32_t steps;           /* T, 1 .. RPLGPU_ROLLOUT_MAX_STEPS: E27's */
  uint32_t delta_per_step;  /* 0 or 1: E27's */
} rplgpu_mppi_t;
/* xy_scale 1024, shift 0, table_len 1024, steps 32, delta_per_step 1 */
void rplgpu_default_mppi(rplgpu_mppi_t *m);
/* Host only.  RPLGPU_ERR_INVALID_ARG for NULL, an xy_scale that is not finite or not > 0, a value outside the ranges
 * above.  The device path uses this function. */
int32_t rplgpu_mppi_check(const rplgpu_mppi_t *m);
/* Host only: the uint32 words of scratch the update takes for G groups of K candidates and T_e steps:
 * 8 ceil(K / 256) G (a record per workgroup of the weights launch) + 12 C T_e G (a record per workgroup and step of
 * the sums launch), C = ceil(K / (RPLGPU_MPPI_PER_LANE * 256 / TW)), TW = the power of two at or above T_e.  0 for
 * G = 0 or above 65535, a K outside 1 .. RPLGPU_MAX_POSES, a T_e outside 1 .. RPLGPU_ROLLOUT_MAX_STEPS, K T_e above
 * 2^24, or a launch above RPLGPU_MPPI_MAX_BLOCKS workgroups. */
uint64_t rplgpu_mppi_scratch_words(uint32_t G, uint32_t K, uint32_t T_e);
/* Host only, fp64, NOT part of the byte-exact contract (as rplgpu_rollout_deltas is not): the softmax table of
 * temperature lambda (in score units), out[i] = floor(65535 exp(-(i 2^shift) / lambda) + 0.5); out[0] is always 65535.
 * RPLGPU_ERR_INVALID_ARG for a NULL out, a lambda that is not finite or not > 0, shift above RPLGPU_MPPI_MAX_SHIFT,
 * N outside 1 .. RPLGPU_MPPI_MAX_TABLE. */
int32_t rplgpu_mppi_table(double lambda, uint32_t shift, uint32_t N, uint16_t *out);
/* Host only: A's rules in plain C++ for ONE group.  out: 8 K words; rollout_result: 8 words; delta: 4 K T_e floats;
 * table: N entries; nominal: NULL or 4 T_e floats; weights: K words; sums: 8 T_e words; nominal_out: 4 T_e floats
 * (it may be nominal itself); result: 8 words.  RPLGPU_ERR_INVALID_ARG and nothing written for a spec the check
 * refuses, a NULL pointer other than nominal, K = 0 or above RPLGPU_MAX_POSES, K * T above 2^24. */
int32_t rplgpu_mppi_update_host(const rplgpu_mppi_t *m, const uint32_t *out, const uint32_t rollout_result[8],
                                const float *delta, const uint16_t *table, const float *nominal, uint32_t K,
                                uint32_t *weights, uint32_t *sums, float *nominal_out, uint32_t result[8]);
/* A for each of G groups on the handle's stream: three launches (the weights with a record per workgroup, the sums
 * with a record per workgroup and step, then one workgroup per group that folds both kinds of record and does the
 * finish), no workgroup waits for another, nothing is stored on the handle.  d_scratch: rplgpu_mppi_scratch_words of
 * (G, K, T_e) words, 16-byte aligned, the caller's; it holds nothing a later call relies on.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for a spec the check refuses, G = 0 or above 65535,
 * K = 0 or above RPLGPU_MAX_POSES, K * T above 2^24, a missing d_out / d_rollout_result / d_delta / d_table /
 * d_weights / d_sums / d_nominal_out / d_result / d_scratch, a misaligned pointer (16 bytes: d_out, d_delta,
 * d_nominal, d_sums, d_nominal_out, d_scratch; 2: d_table; 4: the others), the stride rules above, and an output
 * (d_weights, d_sums, d_nominal_out, d_result, d_scratch) that overlaps an input or another output over the ranges
 * used, but for d_nominal_out on d_nominal as above; RPLGPU_ERR_CAPACITY where a launch would pass
 * RPLGPU_MPPI_MAX_BLOCKS workgroups.  Asynchronous on the handle's stream. */
int32_t rplgpu_mppi_update_dev(rplgpu_handle_t h, const rplgpu_mppi_t *m, const uint32_t *d_out, uint64_t out_stride,
                               const uint32_t *d_rollout_result, const float *d_delta, uint64_t delta_stride,
                               uint32_t delta_per_group, const uint16_t *d_table, const float *d_nominal,
                               uint64_t nominal_stride, uint32_t nominal_per_group, uint32_t G, uint32_t K,
                               uint32_t *d_weights, uint64_t weight_stride, uint32_t *d_sums, uint64_t sums_stride,
                               float *d_nominal_out, uint64_t nominal_out_stride, uint32_t *d_result,
                               uint32_t *d_scratch);
/* ONE group, HOST buffers, arguments as rplgpu_mppi_update_host.  Allocates its device buffers and scratch per call
 * and returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_mppi_update(rplgpu_handle_t h, const rplgpu_mppi_t *m, const uint32_t *out,
                           const uint32_t rollout_result[8], const float *delta, const uint16_t *table,
                           const float *nominal, uint32_t K, uint32_t *weights, uint32_t *sums, float *nominal_out,
                           uint32_t result[8]);
/* Host only: B's rule in plain C++ for ONE group.  nominal: 4 T_n floats; noise: 4 K T floats; out: 4 K T floats (it
 * may be noise itself).  RPLGPU_ERR_INVALID_ARG and nothing written for a NULL pointer, K = 0 or above
 * RPLGPU_MAX_POSES, T or T_n outside 1 .. RPLGPU_ROLLOUT_MAX_STEPS, K * T above 2^24, shift above
 * RPLGPU_MPPI_MAX_SPREAD_SHIFT. */
int32_t rplgpu_mppi_spread_host(const float *nominal, uint32_t T_n, const float *noise, uint32_t K, uint32_t T,
                                uint32_t shift, uint32_t keep_first, float *out);
/* B for each of G groups on the handle's stream: one launch, a thread per (candidate, step).  All three pointers
 * 16-byte aligned; nominal_stride >= 4 T_n, noise_stride and out_stride >= 4 K T, all in floats and multiples of 4.
 * RPLGPU_ERR_INVALID_ARG, no output changed and nothing queued, for the host twin's refusals, G = 0 or above 65535, a
 * misaligned pointer, the stride rules and a d_out that overlaps an input other than d_noise as above;
 * RPLGPU_ERR_CAPACITY where the launch would pass RPLGPU_MPPI_MAX_BLOCKS workgroups.  Asynchronous. */
int32_t rplgpu_mppi_spread_dev(rplgpu_handle_t h, const float *d_nominal, uint64_t nominal_stride,
                               uint32_t nominal_per_group, uint32_t T_n, const float *d_noise, uint64_t noise_stride,
                               uint32_t noise_per_group, uint32_t G, uint32_t K, uint32_t T, uint32_t shift,
                               uint32_t keep_first, float *d_out, uint64_t out_stride);
/* ONE group, HOST buffers, arguments as rplgpu_mppi_spread_host: a door, not a hot path. */
int32_t rplgpu_mppi_spread(rplgpu_handle_t h, const float *nominal, uint32_t T_n, const float *noise, uint32_t K,
                           uint32_t T, uint32_t shift, uint32_t keep_first, float *out);

/* ---- E29: a map's frontiers found, grouped and the next goal picked (row 4; what hands E26 its goal) ----
 * Every stage from E26 on starts from a goal cell; a robot that builds E14's map has to decide where to drive next.
 * Yamauchi's frontiers (explore_lite, frontier_exploration) work on the two arrays already in device memory: the int8
 * grid of rplgpu_map_grid_dev / rplgpu_inflate_grids_dev and E26's field D taken with the robot's own cell as the
 * goal, the cost of reaching every cell from the robot.  E29 writes its choice in E26's goal layout, so map_grid ->
 * inflate -> field (from the robot) -> frontiers -> field (to the frontier) -> rollout -> update queues with no
 * read-back.  Nothing in the reference explores: these rules are the definition (parity unpinned, as E5-E28).
 * Everything is integers and depends on no order of execution.
 *
 * Per grid g of G: the int8 grid at d_grid + g * grid_stride (E11's layout, cell (cx, cy) at cy * width + cx; E12's
 * stride and alignment rules) and optionally E26's field at d_potential + g * potential_stride.  Both are only read.
 *   FREE      0 <= v < lethal (E26's meaning)             UNKNOWN   v < 0
 *   D(c)      the field's word; with d_potential = NULL it is 0 for every cell
 *   FRONTIER  c is FREE, D(c) != RPLGPU_NAV_UNREACHED and at least one of its four edge neighbours INSIDE the grid is
 *             UNKNOWN (outside the grid is not unknown).  F: the frontier cells of a grid.
 *   COMPONENTS  of the frontier cells under 8-adjacency, no wrap ((width - 1, cy) and (0, cy + 1) are no neighbours).
 *             A component's LABEL is its smallest cell index.  N: the components of a grid.
 *   per component, exact integers: n, its cells; sum cx and sum cy (two words each); the least of D(c) * 2^32 + c
 *             over its cells, which gives Dmin and, on ties, the smallest cell that holds it ("its cell").
 *   KEPT      n >= min_size.     COST of a kept component: dist_weight * Dmin - size_weight * n as an int64
 *             (explore_lite's potential_scale / gain_scale).
 *   BEST      the kept component of least cost, ties to the smaller label.
 *   BOUND     a call holds at most comp_cap components (1 .. RPLGPU_FRONTIER_MAX_COMPS, it sizes the scratch).  With
 *             N above it: flag bit 2; F, N and the labels are still exact and whole; words 3 - 14 are as if no
 *             component existed (5 = 0xFFFFFFFF, the others 0), bit 1 is set, no row is written, the goal count is 0.
 * RESULT, RPLGPU_FRONTIER_WORDS = 16 words per grid at d_result + 16 g: 0 the flags (RPLGPU_FRONTIER_NONE: F = 0;
 * _NO_KEPT: no BEST, so with F = 0 and under BOUND too; _BOUND; _LOOP: a kernel loop reached its stated bound, which a
 * correct build never does), 1 F, 2 N, 3 the kept components, 4 the cells of dropped components, 5 BEST's label
 * (0xFFFFFFFF: none), 6 its n, 7 its Dmin, 8 its cell, 9, 10 its sum cx (low, high), 11, 12 its sum cy, 13 the
 * greatest n of any component, 14 the rows written, 15 0.
 * ROW, RPLGPU_FRONTIER_ROW_WORDS = 8 words: {label, n, sum cx low, high, sum cy low, high, Dmin, cell}. */
#define RPLGPU_FRONTIER_WORDS      16u
#define RPLGPU_FRONTIER_ROW_WORDS  8u
#define RPLGPU_FRONTIER_MAX_COMPS  0x100000u
#define RPLGPU_FRONTIER_NONE       0x01u
#define RPLGPU_FRONTIER_NO_KEPT    0x02u
#define RPLGPU_FRONTIER_BOUND      0x04u
#define RPLGPU_FRONTIER_LOOP       0x08u
#define RPLGPU_FRONTIER_NO_LABEL   0xFFFFFFFFu
typedef struct rplgpu_frontiers {
  uint32_t width, height;   /* 1 .. RPLGPU_MAX_OCC_DIM */
  uint32_t lethal;          /* 1 .. 100: bytes in 0 .. lethal - 1 are FREE */
  uint32_t min_size;        /* >= 1: a component of fewer cells is dropped */
  uint32_t dist_weight;     /* 0 .. 65535 */
  uint32_t size_weight;     /* 0 .. 65535 */
} rplgpu_frontiers_t;
/* 1024 x 1024, lethal 99, min_size 8, dist_weight 1, size_weight 0 */
void rplgpu_default_frontiers(rplgpu_frontiers_t *f);
/* Host only (no handle, no device).  RPLGPU_ERR_INVALID_ARG for NULL and a value outside the ranges above.  The
 * device path uses this function. */
int32_t rplgpu_frontiers_check(const rplgpu_frontiers_t *f);
/* Host only: the uint32 words of scratch rplgpu_frontiers_dev takes, G times
 * 16 + up4(ceil(cells / 1024)) + 2 up4(cells) + 8 comp_cap with cells = width * height and up4 the next multiple of
 * four (a header, a count per 1024 cells, the parent plane, the rank plane, a table row per component); 0 for a spec the check refuses, G = 0 or above
 * 65535, comp_cap outside 1 .. RPLGPU_FRONTIER_MAX_COMPS and G * ntx * nty above RPLGPU_NAV_MAX_TILES. */
uint64_t rplgpu_frontiers_scratch_words(const rplgpu_frontiers_t *f, uint32_t G, uint32_t comp_cap);
/* Host only: ONE grid in plain C++, a flood fill over the frontier cells in ascending cell index.  potential,
 * labels_out (width * height words, written whole), rows (row_cap rows; the first min(kept, row_cap) are written),
 * goal_out and n_goal_out (one word each; both or neither) are optional; result: 16 words.
 * RPLGPU_ERR_INVALID_ARG and nothing written for a spec the check refuses, comp_cap out of range, a NULL grid or
 * result, rows = NULL with row_cap != 0, one of goal_out and n_goal_out without the other. */
int32_t rplgpu_frontiers_host(const rplgpu_frontiers_t *f, const int8_t *grid, const uint32_t *potential,
                              uint32_t comp_cap, uint32_t *labels_out, uint32_t *rows, uint32_t row_cap,
                              uint32_t *goal_out, uint32_t *n_goal_out, uint32_t result[16]);
/* G grids on the handle's stream, seven launches and no host round trip; no workgroup ever waits for another.
 * d_labels_out + g * label_stride (optional; label_stride >= width * height words): one word per cell, the label of a
 * frontier cell, RPLGPU_FRONTIER_NO_LABEL otherwise; words at and beyond width * height are never changed.
 * d_rows + g * row_stride (optional, required with row_cap != 0; row_stride >= 8 row_cap words): the rows of the
 * first min(kept, row_cap) kept components in ascending label order; rows beyond are never changed.
 * d_goal_out + g * goal_stride and d_n_goal_out[g] (optional, both or neither; goal_stride >= 1), in
 * rplgpu_nav_field_dev's d_goals / d_n_goals layout: BEST's cell and 1; with no BEST 0, the goal word untouched.
 * d_scratch: rplgpu_frontiers_scratch_words words, 16-byte aligned, the caller's; it holds nothing between calls.
 * RPLGPU_ERR_INVALID_ARG, nothing queued and no output changed, for a spec the check refuses, G = 0 or above 65535,
 * comp_cap out of range, a missing d_grid, d_result or d_scratch, a misaligned pointer (4 bytes; d_scratch 16), the
 * stride rules (E26's for the grid and the field), d_rows = NULL with row_cap != 0, one of the goal pointers without
 * the other, and an output (d_labels_out, d_rows, d_goal_out, d_n_goal_out, d_result, d_scratch) that overlaps an
 * input or another output over the ranges used; RPLGPU_ERR_CAPACITY for G * ntx * nty above RPLGPU_NAV_MAX_TILES.
 * Asynchronous; nothing is stored on the handle. */
int32_t rplgpu_frontiers_dev(rplgpu_handle_t h, const rplgpu_frontiers_t *f, const int8_t *d_grid,
                             uint64_t grid_stride, const uint32_t *d_potential, uint64_t potential_stride, uint32_t G,
                             uint32_t comp_cap, uint32_t *d_labels_out, uint64_t label_stride, uint32_t *d_rows,
                             uint64_t row_stride, uint32_t row_cap, uint32_t *d_goal_out, uint64_t goal_stride,
                             uint32_t *d_n_goal_out, uint32_t *d_result, uint32_t *d_scratch);
/* ONE grid, HOST buffers, arguments as rplgpu_frontiers_host.  Allocates its device buffers and scratch per call and
 * returns when the results are in place: a door, not a hot path. */
int32_t rplgpu_frontiers(rplgpu_handle_t h, const rplgpu_frontiers_t *f, const int8_t *grid, const uint32_t *potential,
                         uint32_t comp_cap, uint32_t *labels_out, uint32_t *rows, uint32_t row_cap, uint32_t *goal_out,
                         uint32_t *n_goal_out, uint32_t result[16]);

#ifdef __cplusplus
}
#endif
#endif /* RPLGPU_MSG_H_ */
