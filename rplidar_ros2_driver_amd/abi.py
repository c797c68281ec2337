"""ctypes binding over the C ABI of ``librplgpu.so`` (``include/rplgpu.h``).

This is the same door the reference's C++ node would use; Python is
only plumbing for tests and ``bench.py``.  Nothing here computes on samples and nothing
falls back to a CPU implementation: a missing library raises ``RplGpuError``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

# == sl_lidar_response_measurement_node_hq_t (reference src/sdk/include/sl_lidar_cmd.h:272-278)
NODE_DTYPE = np.dtype(
    [("angle_z_q14", "<u2"), ("dist_mm_q2", "<u4"), ("quality", "u1"), ("flag", "u1")]
)
assert NODE_DTYPE.itemsize == 8

MAX_SAMPLES_PER_SCAN = 32768

# == rplgpu_cell_t (include/rplgpu_comm.h): one voxel cell before the divide, the cell exchange's record
CELL_DTYPE = np.dtype([("key", "<u4"), ("count", "<u4"), ("isum", "<u4"), ("reserved", "<u4"),
                       ("sx", "<f8"), ("sy", "<f8")])
assert CELL_DTYPE.itemsize == 32

OK = 0
ERR_INVALID_ARG = -1
ERR_NO_DEVICE = -2
ERR_HIP = -3
ERR_CAPACITY = -4
ERR_ALL_INVALID = -5
ERR_SCAN_OVERFLOW = -6

SCAN_ALL_INVALID = 0x1
SCAN_CELL_RANGE = 0x2
WIDE_MATCH_BLOCK = 8          # RPLGPU_WIDE_MATCH_BLOCK (E24)
MAX_WIDE_SHIFT = 256          # RPLGPU_MAX_WIDE_SHIFT
MAX_WIDE_BLOCKS = 65536       # RPLGPU_MAX_WIDE_BLOCKS
WIDE_MATCH_UNPROVEN = 0x1     # word 7 of E24's result words
REFINE_WORDS = 32             # RPLGPU_REFINE_WORDS (E25): uint32 words of sums per pose
NAV_TILE = 64                 # RPLGPU_NAV_TILE (E26): cells a side of a tile of the field
NAV_MAX_COST = 2047           # RPLGPU_NAV_MAX_COST
NAV_MAX_CAP = 0xFFFF0000      # RPLGPU_NAV_MAX_CAP
NAV_MAX_ROUNDS = 4096         # RPLGPU_NAV_MAX_ROUNDS
NAV_MAX_GOALS = 1024          # RPLGPU_NAV_MAX_GOALS
NAV_MAX_STARTS = 65536        # RPLGPU_NAV_MAX_STARTS
NAV_MAX_TILES = 1 << 23       # RPLGPU_NAV_MAX_TILES: G x tiles of one call
NAV_UNREACHED = 0xFFFFFFFF    # RPLGPU_NAV_UNREACHED
NAV_UNFINISHED = 0x01         # RPLGPU_NAV_UNFINISHED (result word 1)
NAV_PATH_REACHED, NAV_PATH_NO_START, NAV_PATH_UNREACHED, NAV_PATH_TRUNCATED, NAV_PATH_BROKEN = 1, 2, 4, 8, 16
ROLLOUT_MAX_STEPS = 256       # RPLGPU_ROLLOUT_MAX_STEPS (E27)
ROLLOUT_MAX_FOOTPRINT = 64    # RPLGPU_ROLLOUT_MAX_FOOTPRINT
ROLLOUT_MAX_WEIGHT = 65535    # RPLGPU_ROLLOUT_MAX_WEIGHT
ROLLOUT_NONE = 0xFFFFFFFF     # RPLGPU_ROLLOUT_NONE (result word 1)
ROLLOUT_TILE = 32             # RPLGPU_ROLLOUT_TILE: candidates a workgroup takes
ROLLOUT_MAX_TILES = 1 << 23   # RPLGPU_ROLLOUT_MAX_TILES: G x tiles of one call
ROLLOUT_BLOCKED, ROLLOUT_CELL_RANGE, ROLLOUT_END_UNREACHED, ROLLOUT_ADMISSIBLE = 1, 2, 4, 8
MPPI_MAX_SHIFT = 49           # RPLGPU_MPPI_MAX_SHIFT (E28)
MPPI_MAX_TABLE = 65536        # RPLGPU_MPPI_MAX_TABLE
MPPI_MAX_SPREAD_SHIFT = 256   # RPLGPU_MPPI_MAX_SPREAD_SHIFT
MPPI_PER_LANE = 8             # RPLGPU_MPPI_PER_LANE: candidates a lane of the sums launch folds
MPPI_MAX_BLOCKS = 1 << 23     # RPLGPU_MPPI_MAX_BLOCKS: workgroups of one launch
MPPI_NO_WEIGHT, MPPI_OFF_RANGE, MPPI_EMPTY_STEP = 1, 2, 4
FRONTIER_WORDS = 16           # RPLGPU_FRONTIER_WORDS (E29): result words per grid
FRONTIER_ROW_WORDS = 8        # RPLGPU_FRONTIER_ROW_WORDS
FRONTIER_MAX_COMPS = 1 << 20  # RPLGPU_FRONTIER_MAX_COMPS: the greatest comp_cap
FRONTIER_NO_LABEL = 0xFFFFFFFF  # RPLGPU_FRONTIER_NO_LABEL
FRONTIER_NONE, FRONTIER_NO_KEPT, FRONTIER_BOUND, FRONTIER_LOOP = 1, 2, 4, 8
REFINE_PLANES = 29            # RPLGPU_REFINE_PLANES
REFINE_MAX_ITERS = 16         # RPLGPU_REFINE_MAX_ITERS
REFINE_STEPPED = 0x01         # E25's step flags
REFINE_FEW = 0x02
REFINE_SINGULAR = 0x04
REFINE_CLAMP_X = 0x08
REFINE_CLAMP_Y = 0x10
REFINE_CLAMP_T = 0x20
SCAN_TABLE_FULL = 0x4
SCAN_OUT_TRUNCATED = 0x8

MAX_MERGE_BEAMS = 16384  # RPLGPU_MAX_MERGE_BEAMS (include/rplgpu_msg.h)
MAX_FILTER_WINDOW = 64   # RPLGPU_MAX_FILTER_WINDOW (include/rplgpu_msg.h)
MAX_OCC_DIM = 4096       # RPLGPU_MAX_OCC_DIM (include/rplgpu_msg.h)
MAX_OCC_STEPS = 8192     # RPLGPU_MAX_OCC_STEPS (include/rplgpu_msg.h)
MAX_INFLATION_CELLS = 64  # RPLGPU_MAX_INFLATION_CELLS (include/rplgpu_msg.h)
MAX_POSES = 1048576       # RPLGPU_MAX_POSES (include/rplgpu_msg.h)
ESTIMATE_WORDS = 72       # RPLGPU_ESTIMATE_WORDS
CLUSTER_WORDS = 80        # RPLGPU_CLUSTER_WORDS
MAX_POSE_BINS = 67108864  # RPLGPU_MAX_POSE_BINS (include/rplgpu_msg.h)
MAX_HEADING_BINS = 1024   # RPLGPU_MAX_HEADING_BINS (include/rplgpu_msg.h)

SL_RESULT_OK = 0
SL_RESULT_OPERATION_FAIL = 0x80008001

# every symbol include/rplgpu.h declares (checked by the CPU-side ABI test)
ABI_SYMBOLS = [
    "rplgpu_abi_version",
    "rplgpu_create",
    "rplgpu_destroy",
    "rplgpu_last_error",
    "rplgpu_default_params",
    "rplgpu_set_stream",
    "rplgpu_synchronize",
    "rplgpu_ascend",
    "rplgpu_scan_to_laserscan",
    "rplgpu_scan_to_cloud",
    "rplgpu_ascend_batch_dev",
    "rplgpu_laserscan_batch_dev",
    "rplgpu_ascend_laserscan_batch_dev",
    "rplgpu_cloud_batch_dev",
    "rplgpu_pack_clouds_dev",
    "rplgpu_cloud_arena_dev",
    "rplgpu_fill_meta",
    "rplgpu_frame_size",
    "rplgpu_nodes_per_frame",
    "rplgpu_decode_max_frames",
    "rplgpu_decode_staged_frames",
    "rplgpu_frame_stream",
    "rplgpu_decode_batch_dev",
    "rplgpu_decode_scans_dev",
    "rplgpu_decode_scans_carry_dev",
    "rplgpu_segment_batch_dev",
    "rplgpu_scans_to_batch_dev",
    "rplgpu_decode_stream",
    # include/rplgpu_msg.h
    "rplgpu_msg_laserscan_layout",
    "rplgpu_msg_cloud_layout",
    "rplgpu_msg_laserscan_header",
    "rplgpu_msg_cloud_header",
    "rplgpu_host_alloc",
    "rplgpu_host_free",
    "rplgpu_scan_to_laserscan_msg",
    "rplgpu_scan_to_cloud_msg",
    "rplgpu_laserscan_msgs_dev",
    "rplgpu_cloud_msgs_dev",
    "rplgpu_transform_clouds_dev",
    "rplgpu_fused_cloud_msg_dev",
    "rplgpu_cloud_deskew_batch_dev",
    "rplgpu_laserscan_to_cloud_batch_dev",
    "rplgpu_laserscan_to_cloud",
    "rplgpu_cloud_fused_voxel_dev",
    "rplgpu_set_cell_key_output",
    "rplgpu_set_scan_time_offsets_dev",
    "rplgpu_set_voxel_aggregation",
    "rplgpu_set_ror_mode",
    "rplgpu_scan_merge_edges",
    "rplgpu_merge_scans_dev",
    "rplgpu_merged_laserscan_msgs_dev",
    "rplgpu_default_scan_filter",
    "rplgpu_scan_filter_check",
    "rplgpu_filter_laserscan_batch_dev",
    "rplgpu_filter_merged_scans_dev",
    "rplgpu_filter_laserscan",
    "rplgpu_default_occ_grid",
    "rplgpu_occ_grid_check",
    "rplgpu_occupancy_grid_dev",
    "rplgpu_occupancy_grid",
    "rplgpu_msg_occupancy_layout",
    "rplgpu_occupancy_grid_msgs_dev",
    "rplgpu_default_inflation",
    "rplgpu_inflation_check",
    "rplgpu_inflation_table",
    "rplgpu_inflate_grids_dev",
    "rplgpu_inflate_grid",
    "rplgpu_default_scan_match",
    "rplgpu_scan_match_check",
    "rplgpu_scan_match_rotations",
    "rplgpu_scan_match_volume",
    "rplgpu_match_scans_dev",
    "rplgpu_match_scans",
    "rplgpu_map_update_dev",
    "rplgpu_default_map_rule",
    "rplgpu_map_rule_check",
    "rplgpu_map_grid_dev",
    "rplgpu_apply_match_dev",
    "rplgpu_map_update",
    "rplgpu_map_grid",
    "rplgpu_default_pose_score",
    "rplgpu_pose_score_check",
    "rplgpu_pose_list",
    "rplgpu_score_poses_dev",
    "rplgpu_score_poses",
    "rplgpu_resample_scratch_words",
    "rplgpu_resample_poses_dev",
    "rplgpu_resample_host",
    "rplgpu_resample_poses",
    "rplgpu_default_pose_estimate",
    "rplgpu_pose_estimate_check",
    "rplgpu_estimate_scratch_words",
    "rplgpu_estimate_poses_dev",
    "rplgpu_estimate_host",
    "rplgpu_estimate_poses",
    "rplgpu_estimate_pose",
    "rplgpu_default_motion_noise",
    "rplgpu_sample_motion_dev",
    "rplgpu_sample_motion_host",
    "rplgpu_sample_motion",
    "rplgpu_philox4x32",
    "rplgpu_motion_odometry",
    "rplgpu_default_pose_seed",
    "rplgpu_pose_seed_check",
    "rplgpu_seed_scratch_words",
    "rplgpu_seed_headings",
    "rplgpu_seed_poses_dev",
    "rplgpu_seed_poses_host",
    "rplgpu_seed_poses",
    "rplgpu_default_pose_bins",
    "rplgpu_pose_bins_check",
    "rplgpu_bin_map_words",
    "rplgpu_heading_edges_check",
    "rplgpu_bin_poses_dev",
    "rplgpu_bin_poses_host",
    "rplgpu_bin_poses",
    "rplgpu_kld_samples",
    "rplgpu_default_pose_clusters",
    "rplgpu_pose_clusters_check",
    "rplgpu_cluster_scratch_words",
    "rplgpu_cluster_poses_dev",
    "rplgpu_cluster_poses_host",
    "rplgpu_cluster_poses",
    "rplgpu_default_range_cast",
    "rplgpu_range_cast_check",
    "rplgpu_cast_beams",
    "rplgpu_cast_range_m",
    "rplgpu_cast_ranges_dev",
    "rplgpu_cast_ranges_host",
    "rplgpu_cast_ranges",
    "rplgpu_default_beam_agree",
    "rplgpu_beam_agree_check",
    "rplgpu_score_poses_agree_dev",
    "rplgpu_score_poses_agree",
    "rplgpu_beam_agree_points_host",
    "rplgpu_default_wide_match",
    "rplgpu_wide_match_check",
    "rplgpu_wide_match_blocks",
    "rplgpu_wide_match_scratch_words",
    "rplgpu_pool_field_host",
    "rplgpu_pool_field_dev",
    "rplgpu_match_wide_dev",
    "rplgpu_match_wide",
    "rplgpu_default_pose_refine",
    "rplgpu_pose_refine_check",
    "rplgpu_refine_scratch_words",
    "rplgpu_refine_sums_host",
    "rplgpu_refine_step_host",
    "rplgpu_refine_covariance",
    "rplgpu_refine_sums_dev",
    "rplgpu_refine_step_dev",
    "rplgpu_refine_poses_dev",
    "rplgpu_refine_poses",
    "rplgpu_match_poses_dev",
    "rplgpu_compose_poses_dev",
    "rplgpu_default_nav_field",
    "rplgpu_nav_field_check",
    "rplgpu_nav_field_default_rounds",
    "rplgpu_nav_field_scratch_words",
    "rplgpu_nav_field_host",
    "rplgpu_nav_path_host",
    "rplgpu_nav_field_dev",
    "rplgpu_nav_paths_dev",
    "rplgpu_nav_field",
    "rplgpu_default_rollout",
    "rplgpu_rollout_check",
    "rplgpu_rollout_scratch_words",
    "rplgpu_rollout_deltas",
    "rplgpu_rollout_host",
    "rplgpu_rollout_dev",
    "rplgpu_rollout",
    "rplgpu_default_mppi",
    "rplgpu_mppi_check",
    "rplgpu_mppi_scratch_words",
    "rplgpu_mppi_table",
    "rplgpu_mppi_update_host",
    "rplgpu_mppi_update_dev",
    "rplgpu_mppi_update",
    "rplgpu_mppi_spread_host",
    "rplgpu_mppi_spread_dev",
    "rplgpu_mppi_spread",
    "rplgpu_default_frontiers",
    "rplgpu_frontiers_check",
    "rplgpu_frontiers_scratch_words",
    "rplgpu_frontiers_host",
    "rplgpu_frontiers_dev",
    "rplgpu_frontiers",
    # include/rplgpu_comm.h
    "rplgpu_comm_unique_id",
    "rplgpu_comm_init",
    "rplgpu_comm_destroy",
    "rplgpu_comm_size",
    "rplgpu_cloud_meta_words",
    "rplgpu_pack_cloud_meta_dev",
    "rplgpu_allgather_clouds_dev",
    "rplgpu_gather_clouds_dev",
    "rplgpu_cloud_fused_cells_dev",
    "rplgpu_gather_cells_dev",
    "rplgpu_merge_cells_dev",
    "rplgpu_merge_cells_host",
    "rplgpu_comm_fence",
    "rplgpu_comm_fence_lag",
    "rplgpu_unpack_gathered_dev",
    "rplgpu_pack_cloud_xyi_dev",
    "rplgpu_cloud_arena_xyi_dev",
    "rplgpu_allgather_clouds_xyi_dev",
    "rplgpu_unpack_gathered_xyi_dev",
    "rplgpu_pack_cloud_meta_host",
    "rplgpu_pack_cloud_xyi_host",
    "rplgpu_unpack_gathered_host",
]


class RplGpuError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"rplgpu error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """Mirror of ``rplgpu_params_t``."""

    _fields_ = [
        ("is_new_protocol", C.c_int32),
        ("inverted", C.c_int32),
        ("scan_processing", C.c_int32),
        ("clip_enable", C.c_int32),
        ("q_min", C.c_uint32),
        ("range_min", C.c_float),
        ("range_max", C.c_float),
        ("voxel_leaf", C.c_float),
        ("ror_radius", C.c_float),
        ("ror_min_neighbors", C.c_uint32),
        ("ror_enable", C.c_int32),
        ("voxel_enable", C.c_int32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "Params":
        p = cls(0, 0, 1, 0, 0, 0.15, 12.0, 0.05, 0.10, 2, 0, 0)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class ScanMeta(C.Structure):
    """Mirror of ``rplgpu_scan_meta_t``."""

    _fields_ = [
        ("angle_min", C.c_float),
        ("angle_max", C.c_float),
        ("angle_increment", C.c_float),
        ("time_increment", C.c_float),
        ("scan_time", C.c_float),
        ("range_min", C.c_float),
        ("range_max", C.c_float),
        ("count", C.c_uint32),
        ("published", C.c_int32),
    ]


class Stamp(C.Structure):
    """Mirror of ``rplgpu_stamp_t`` (builtin_interfaces/Time)."""

    _fields_ = [("sec", C.c_int32), ("nanosec", C.c_uint32)]


class LaserScanLayout(C.Structure):
    """Mirror of ``rplgpu_laserscan_layout_t``."""

    _fields_ = [(k, C.c_uint32) for k in (
        "scalars_off", "ranges_len_off", "ranges_off", "intensities_len_off",
        "intensities_off", "total_len")]


class CloudLayout(C.Structure):
    """Mirror of ``rplgpu_cloud_layout_t``."""

    _fields_ = [(k, C.c_uint32) for k in (
        "width_off", "row_step_off", "data_len_off", "data_off", "is_dense_off", "total_len")]


class ScanMerge(C.Structure):
    """Mirror of ``rplgpu_scan_merge_t`` (E9: the virtual scan the sensors of a group merge into)."""

    _fields_ = [
        ("angle_min", C.c_float),
        ("angle_max", C.c_float),
        ("count", C.c_uint32),
        ("range_min", C.c_float),
        ("range_max", C.c_float),
        ("scan_time", C.c_float),
    ]


class ScanFilter(C.Structure):
    """Mirror of ``rplgpu_scan_filter_t`` (E10: scan-shadow and speckle filters on a LaserScan)."""

    _fields_ = [
        ("shadow_enable", C.c_int32),
        ("shadow_min_angle", C.c_float),
        ("shadow_max_angle", C.c_float),
        ("shadow_window", C.c_uint32),
        ("shadow_neighbors", C.c_uint32),
        ("speckle_enable", C.c_int32),
        ("speckle_max_range_difference", C.c_float),
        ("speckle_min_run", C.c_uint32),
        ("circular", C.c_int32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "ScanFilter":
        """The library's own defaults (``rplgpu_default_scan_filter``), then the overrides."""
        f = cls()
        load_library().rplgpu_default_scan_filter(C.byref(f))
        for k, v in kw.items():
            if not hasattr(f, k):
                raise AttributeError(k)
            setattr(f, k, v)
        return f


class OccGrid(C.Structure):
    """Mirror of ``rplgpu_occ_grid_t`` (E11: the ray-cast occupancy grid of a group of scans)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("range_min", C.c_float),
        ("obstacle_max", C.c_float),
        ("raytrace_max", C.c_float),
    ]

    @classmethod
    def defaults(cls, **kw) -> "OccGrid":
        """The library's own defaults (``rplgpu_default_occ_grid``), then the overrides."""
        g = cls()
        load_library().rplgpu_default_occ_grid(C.byref(g))
        for k, v in kw.items():
            if not hasattr(g, k):
                raise AttributeError(k)
            setattr(g, k, v)
        return g


class Inflation(C.Structure):
    """Mirror of ``rplgpu_inflation_t`` (E12: the costmap inflation layer over the grids of E11)."""

    _fields_ = [
        ("inscribed_radius", C.c_float),
        ("inflation_radius", C.c_float),
        ("cost_scaling_factor", C.c_float),
        ("inflate_unknown", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "Inflation":
        """The library's own defaults (``rplgpu_default_inflation``), then the overrides."""
        f = cls()
        load_library().rplgpu_default_inflation(C.byref(f))
        for k, v in kw.items():
            if not hasattr(f, k):
                raise AttributeError(k)
            setattr(f, k, v)
        return f


class ScanMatch(C.Structure):
    """Mirror of ``rplgpu_scan_match_t`` (E13: a time step's scans matched to a likelihood field)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("shift_x", C.c_uint32),
        ("shift_y", C.c_uint32),
        ("rot_steps", C.c_uint32),
        ("rot_step", C.c_float),
    ]

    @classmethod
    def defaults(cls, **kw) -> "ScanMatch":
        """The library's own defaults (``rplgpu_default_scan_match``), then the overrides."""
        m = cls()
        load_library().rplgpu_default_scan_match(C.byref(m))
        for k, v in kw.items():
            if not hasattr(m, k):
                raise AttributeError(k)
            setattr(m, k, v)
        return m


class MapRule(C.Structure):
    """Mirror of ``rplgpu_map_rule_t`` (E14: hit / miss counts to the cells of an occupancy grid)."""

    _fields_ = [
        ("min_observations", C.c_uint32),
        ("occupied_percent", C.c_uint32),
        ("mode", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "MapRule":
        """The library's own defaults (``rplgpu_default_map_rule``), then the overrides."""
        r = cls()
        load_library().rplgpu_default_map_rule(C.byref(r))
        for k, v in kw.items():
            if not hasattr(r, k):
                raise AttributeError(k)
            setattr(r, k, v)
        return r


class PoseScore(C.Structure):
    """Mirror of ``rplgpu_pose_score_t`` (E15: a list of poses weighed against a likelihood field)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "PoseScore":
        """The library's own defaults (``rplgpu_default_pose_score``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_pose_score(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


class PoseEstimate(C.Structure):
    """Mirror of ``rplgpu_pose_estimate_t`` (E17: a weighted pose list reduced to a pose estimate)."""

    _fields_ = [
        ("xy_scale", C.c_float),
        ("gate_r2", C.c_uint64),
        ("gate_dot", C.c_int64),
    ]

    @classmethod
    def defaults(cls, **kw) -> "PoseEstimate":
        """The library's own defaults (``rplgpu_default_pose_estimate``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_pose_estimate(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s

    @classmethod
    def open_gate(cls, **kw) -> "PoseEstimate":
        """The defaults with the gate that admits every in-range pose (set 1 == set 0)."""
        return cls.defaults(**dict(dict(gate_r2=(1 << 64) - 1, gate_dot=-(1 << 63)), **kw))


class MotionNoise(C.Structure):
    """Mirror of ``rplgpu_motion_noise_t`` (E18: a pose list's motion noise drawn on the device)."""

    _fields_ = [
        ("seed", C.c_uint64),
        ("step", C.c_uint64),
        ("first", C.c_uint32),
        ("reserved", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "MotionNoise":
        """The library's own defaults (``rplgpu_default_motion_noise``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_motion_noise(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


class PoseSeed(C.Structure):
    """Mirror of ``rplgpu_pose_seed_t`` (E19: a pose list seeded over a grid's free cells on the device)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("free_lo", C.c_int32),
        ("free_hi", C.c_int32),
        ("flags", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "PoseSeed":
        """The library's own defaults (``rplgpu_default_pose_seed``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_pose_seed(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s

    def check(self) -> int:
        """``rplgpu_pose_seed_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_pose_seed_check(C.byref(self)))


class PoseBins(C.Structure):
    """Mirror of ``rplgpu_pose_bins_t`` (E20: a pose list's occupied bins counted on the device)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("inv_size", C.c_float),
        ("nx", C.c_uint32),
        ("ny", C.c_uint32),
        ("flags", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "PoseBins":
        """The library's own defaults (``rplgpu_default_pose_bins``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_pose_bins(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s

    def check(self, T: int) -> int:
        """``rplgpu_pose_bins_check`` with T heading bins: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_pose_bins_check(C.byref(self), T))


class PoseClusters(C.Structure):
    """Mirror of ``rplgpu_pose_clusters_t`` (E21: a binned pose list clustered on the device)."""

    _fields_ = [
        ("nx", C.c_uint32),
        ("ny", C.c_uint32),
        ("xy_scale", C.c_float),
        ("flags", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "PoseClusters":
        """The library's own defaults (``rplgpu_default_pose_clusters``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_pose_clusters(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s

    def check(self, T: int) -> int:
        """``rplgpu_pose_clusters_check`` with T heading bins: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_pose_clusters_check(C.byref(self), T))


class RangeCast(C.Structure):
    """Mirror of ``rplgpu_range_cast_t`` (E22: a beam fan cast from every pose of a list into a grid)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("max_steps", C.c_uint32),
        ("hit_lo", C.c_int32),
        ("unknown_stops", C.c_uint32),
        ("table_half", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "RangeCast":
        """The library's own defaults (``rplgpu_default_range_cast``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_range_cast(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s

    def check(self) -> int:
        """``rplgpu_range_cast_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_range_cast_check(C.byref(self)))


class BeamAgree(C.Structure):
    """Mirror of ``rplgpu_beam_agree_t`` (E23: the beams a pose list disagrees with are left out of the weights)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("agree_lo", C.c_int32),
        ("keep_num", C.c_uint32),
        ("keep_den", C.c_uint32),
        ("err_num", C.c_uint32),
        ("err_den", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "BeamAgree":
        """The library's own defaults (``rplgpu_default_beam_agree``), then the overrides."""
        s = cls()
        load_library().rplgpu_default_beam_agree(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s

    def check(self) -> int:
        """``rplgpu_beam_agree_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_beam_agree_check(C.byref(self)))


class WideMatch(C.Structure):
    """Mirror of ``rplgpu_wide_match_t`` (E24: scans matched over a wide window by bound and refine)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("shift_x", C.c_uint32),
        ("shift_y", C.c_uint32),
        ("rot_steps", C.c_uint32),
        ("rot_step", C.c_float),
        ("max_blocks", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "WideMatch":
        """The library's own defaults (``rplgpu_default_wide_match``), then the overrides."""
        m = cls()
        load_library().rplgpu_default_wide_match(C.byref(m))
        for k, v in kw.items():
            if not hasattr(m, k):
                raise AttributeError(k)
            setattr(m, k, v)
        return m

    def check(self) -> int:
        """``rplgpu_wide_match_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_wide_match_check(C.byref(self)))

    def scan_match(self, shift_x: int = 0, shift_y: int = 0) -> "ScanMatch":
        """The E13 spec with the same grid, rot_steps and rot_step: what ``apply_match_dev`` takes beside E24's
        result words, and the spec whose ``scan_match_rotations`` is E24's rotation table."""
        return ScanMatch(self.origin_x, self.origin_y, self.resolution, self.width, self.height, shift_x, shift_y,
                         self.rot_steps, self.rot_step)


class PoseRefine(C.Structure):
    """Mirror of ``rplgpu_pose_refine_t`` (E25: poses refined below a cell by Gauss-Newton on the field)."""

    _fields_ = [
        ("origin_x", C.c_float),
        ("origin_y", C.c_float),
        ("resolution", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("target", C.c_uint32),
        ("damping", C.c_float),
        ("max_step_cells", C.c_float),
        ("max_rot", C.c_float),
        ("min_points", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **kw) -> "PoseRefine":
        """The library's own defaults (``rplgpu_default_pose_refine``), then the overrides."""
        r = cls()
        load_library().rplgpu_default_pose_refine(C.byref(r))
        for k, v in kw.items():
            if not hasattr(r, k):
                raise AttributeError(k)
            setattr(r, k, v)
        return r

    def check(self) -> int:
        """``rplgpu_pose_refine_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_pose_refine_check(C.byref(self)))


class NavField(C.Structure):
    """Mirror of ``rplgpu_nav_field_t`` (E26: a cost-to-goal field over a costmap, and the paths down it)."""

    _fields_ = [(k, C.c_uint32) for k in (
        "width", "height", "lethal", "neutral", "factor", "unknown_cost", "cap", "rounds")]

    @classmethod
    def defaults(cls, **kw) -> "NavField":
        """The library's own defaults (``rplgpu_default_nav_field``), then the overrides; a width or height given
        without ``rounds`` takes ``rplgpu_nav_field_default_rounds`` of the new size."""
        f = cls()
        lib = load_library()
        lib.rplgpu_default_nav_field(C.byref(f))
        for k, v in kw.items():
            if not hasattr(f, k):
                raise AttributeError(k)
            setattr(f, k, v)
        if "rounds" not in kw and ("width" in kw or "height" in kw):
            f.rounds = int(lib.rplgpu_nav_field_default_rounds(f.width, f.height)) or f.rounds
        return f

    def check(self) -> int:
        """``rplgpu_nav_field_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_nav_field_check(C.byref(self)))


class Frontiers(C.Structure):
    """Mirror of ``rplgpu_frontiers_t`` (E29: a map's frontiers found, grouped and the next goal picked)."""

    _fields_ = [(k, C.c_uint32) for k in (
        "width", "height", "lethal", "min_size", "dist_weight", "size_weight")]

    @classmethod
    def defaults(cls, **kw) -> "Frontiers":
        """The library's own defaults (``rplgpu_default_frontiers``), then the overrides."""
        f = cls()
        load_library().rplgpu_default_frontiers(C.byref(f))
        for k, v in kw.items():
            if not hasattr(f, k):
                raise AttributeError(k)
            setattr(f, k, v)
        return f

    def check(self) -> int:
        """``rplgpu_frontiers_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_frontiers_check(C.byref(self)))


class Rollout(C.Structure):
    """Mirror of ``rplgpu_rollout_t`` (E27: candidate motions rolled out of a pose and scored)."""

    _fields_ = [(k, C.c_float) for k in ("origin_x", "origin_y", "resolution")] + [(k, C.c_uint32) for k in (
        "width", "height", "lethal", "unknown_value", "steps", "min_steps", "a_end", "a_min", "a_sum", "a_max")]

    @classmethod
    def defaults(cls, **kw) -> "Rollout":
        """The library's own defaults (``rplgpu_default_rollout``), then the overrides; ``steps`` given without
        ``min_steps`` takes ``min_steps = steps`` (DWB's rule)."""
        r = cls()
        load_library().rplgpu_default_rollout(C.byref(r))
        for k, v in kw.items():
            if not hasattr(r, k):
                raise AttributeError(k)
            setattr(r, k, v)
        if "steps" in kw and "min_steps" not in kw:
            r.min_steps = r.steps
        return r

    def check(self) -> int:
        """``rplgpu_rollout_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_rollout_check(C.byref(self)))


class Mppi(C.Structure):
    """Mirror of ``rplgpu_mppi_t`` (E28: rolled-out candidates weighed and blended into new controls)."""

    _fields_ = [("xy_scale", C.c_float)] + [(k, C.c_uint32) for k in (
        "shift", "table_len", "steps", "delta_per_step")]

    @classmethod
    def defaults(cls, **kw) -> "Mppi":
        """The library's own defaults (``rplgpu_default_mppi``), then the overrides."""
        m = cls()
        load_library().rplgpu_default_mppi(C.byref(m))
        for k, v in kw.items():
            if not hasattr(m, k):
                raise AttributeError(k)
            setattr(m, k, v)
        return m

    def check(self) -> int:
        """``rplgpu_mppi_check``: OK or ERR_INVALID_ARG."""
        return int(load_library().rplgpu_mppi_check(C.byref(self)))

    @property
    def steps_e(self) -> int:
        """T_e: the steps that carry a delta of their own."""
        return self.steps if self.delta_per_step else 1


class OccupancyLayout(C.Structure):
    """Mirror of ``rplgpu_occupancy_layout_t``."""

    _fields_ = [(k, C.c_uint32) for k in (
        "map_load_time_off", "resolution_off", "origin_off", "data_len_off", "data_off", "total_len")]


def library_path() -> Path:
    env = os.environ.get("RPLGPU_LIBRARY")
    if env:
        return Path(env)
    return Path(__file__).resolve().parent / "lib" / "librplgpu.so"


_LIB = None


def load_library() -> C.CDLL:
    """Load ``librplgpu.so`` (in-tree build).  Raises if it is missing — no fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not path.exists():
        raise RplGpuError(
            ERR_NO_DEVICE,
            f"{path} not built; run `python -c 'import __graft_entry__ as g; g.build()'`",
        )
    lib = C.CDLL(str(path))
    vp, u32, i32, sz = C.c_void_p, C.c_uint32, C.c_int32, C.c_size_t
    lib.rplgpu_abi_version.restype = i32
    lib.rplgpu_create.argtypes = [i32, u32, u32, C.POINTER(vp)]
    lib.rplgpu_destroy.argtypes = [vp]
    lib.rplgpu_last_error.argtypes = [vp]
    lib.rplgpu_last_error.restype = C.c_char_p
    lib.rplgpu_default_params.argtypes = [C.POINTER(Params)]
    lib.rplgpu_default_params.restype = None
    lib.rplgpu_set_stream.argtypes = [vp, vp]
    lib.rplgpu_set_voxel_aggregation.argtypes = [vp, i32]
    lib.rplgpu_set_ror_mode.argtypes = [vp, i32]
    lib.rplgpu_synchronize.argtypes = [vp]
    lib.rplgpu_ascend.argtypes = [vp, vp, sz, C.POINTER(u32)]
    lib.rplgpu_scan_to_laserscan.argtypes = [
        vp, vp, sz, C.POINTER(Params), C.c_double, vp, vp, C.POINTER(ScanMeta)]
    lib.rplgpu_scan_to_cloud.argtypes = [
        vp, vp, sz, C.POINTER(Params), vp, C.POINTER(u32), C.POINTER(u32)]
    lib.rplgpu_ascend_batch_dev.argtypes = [vp, vp, u32, vp, u32, vp]
    lib.rplgpu_laserscan_batch_dev.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp]
    lib.rplgpu_ascend_laserscan_batch_dev.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp,
                                                      vp, C.c_int32, vp]
    lib.rplgpu_cloud_batch_dev.argtypes = [
        vp, vp, u32, vp, u32, C.POINTER(Params), vp, u32, vp, vp]
    lib.rplgpu_pack_clouds_dev.argtypes = [vp, vp, u32, vp, u32, vp, vp]
    lib.rplgpu_cloud_arena_dev.argtypes = [
        vp, vp, u32, vp, u32, C.POINTER(Params), vp, C.c_uint64, vp, vp, vp, vp]
    lib.rplgpu_cloud_arena_xyi_dev.argtypes = [
        vp, vp, u32, vp, u32, C.POINTER(Params), vp, C.c_uint64, vp, vp, vp, vp]
    lib.rplgpu_fill_meta.argtypes = [C.POINTER(Params), u32, C.c_double, C.POINTER(ScanMeta)]
    lib.rplgpu_fill_meta.restype = None
    u8, u64 = C.c_uint8, C.c_uint64
    lib.rplgpu_frame_size.argtypes = [u8]
    lib.rplgpu_frame_size.restype = sz
    lib.rplgpu_nodes_per_frame.argtypes = [u8]
    lib.rplgpu_nodes_per_frame.restype = sz
    lib.rplgpu_decode_max_frames.argtypes = [u8]
    lib.rplgpu_decode_max_frames.restype = u32
    lib.rplgpu_decode_staged_frames.argtypes = [u8]
    lib.rplgpu_decode_staged_frames.restype = u32
    lib.rplgpu_frame_stream.argtypes = [u8, vp, sz, vp, vp, sz]
    lib.rplgpu_frame_stream.restype = sz
    lib.rplgpu_decode_batch_dev.argtypes = [vp, u8, u32, vp, u64, vp, vp, vp, u32, u32, vp, vp,
                                            vp, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_decode_scans_dev.argtypes = [vp, u8, u32, vp, u64, vp, vp, vp, u32, u32, vp, vp,
                                            u32, vp, u32, u32, vp, vp, vp, vp]
    lib.rplgpu_decode_scans_carry_dev.argtypes = [vp, u8, u32, vp, u64, vp, vp, vp, u32, u32, vp, vp,
                                                  u32, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32]
    lib.rplgpu_segment_batch_dev.argtypes = [vp, vp, u32, vp, vp, u32, vp, u32, u32, vp, u32, vp,
                                             u32, vp, vp]
    lib.rplgpu_scans_to_batch_dev.argtypes = [vp, vp, u32, vp, u32, vp, u32, vp, vp, u32, u32, vp]
    lib.rplgpu_decode_stream.argtypes = [vp, u8, u32, vp, sz, vp, vp, sz, C.POINTER(sz), vp, sz,
                                         C.POINTER(sz), C.POINTER(u32)]
    cs = C.c_char_p
    lib.rplgpu_msg_laserscan_layout.argtypes = [sz, u32, C.POINTER(LaserScanLayout)]
    lib.rplgpu_msg_cloud_layout.argtypes = [sz, u32, C.POINTER(CloudLayout)]
    lib.rplgpu_msg_laserscan_header.argtypes = [cs, Stamp, C.POINTER(ScanMeta), vp, sz,
                                                C.POINTER(LaserScanLayout)]
    lib.rplgpu_msg_cloud_header.argtypes = [cs, Stamp, u32, vp, sz, C.POINTER(CloudLayout)]
    lib.rplgpu_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.rplgpu_host_free.argtypes = [vp, vp]
    lib.rplgpu_scan_to_laserscan_msg.argtypes = [vp, vp, sz, C.POINTER(Params), C.c_double, cs,
                                                 Stamp, vp, sz, C.POINTER(sz), C.POINTER(ScanMeta)]
    lib.rplgpu_scan_to_cloud_msg.argtypes = [vp, vp, sz, C.POINTER(Params), cs, Stamp, vp, sz,
                                             C.POINTER(sz), C.POINTER(u32), C.POINTER(u32)]
    lib.rplgpu_laserscan_msgs_dev.argtypes = [vp, vp, vp, u32, vp, u32, C.POINTER(Params), cs,
                                              vp, vp, vp, u32, vp, vp]
    lib.rplgpu_cloud_msgs_dev.argtypes = [vp, vp, u32, vp, vp, u32, cs, vp, vp, u32, vp, vp]
    lib.rplgpu_transform_clouds_dev.argtypes = [vp, vp, u32, vp, vp, u32, vp]
    lib.rplgpu_fused_cloud_msg_dev.argtypes = [vp, vp, vp, u64, cs, Stamp, vp, u64, vp, vp]
    lib.rplgpu_cloud_deskew_batch_dev.argtypes = [
        vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, u32, vp, vp]
    lib.rplgpu_laserscan_to_cloud_batch_dev.argtypes = [vp, vp, vp, u32, vp, u32, C.POINTER(Params),
                                                        vp, u32, vp, vp]
    lib.rplgpu_laserscan_to_cloud.argtypes = [vp, vp, vp, u32, C.POINTER(Params), vp,
                                              C.POINTER(u32)]
    lib.rplgpu_cloud_fused_voxel_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp, vp,
                                                 u64, vp, vp, vp, vp]
    lib.rplgpu_set_cell_key_output.argtypes = [vp, vp]
    lib.rplgpu_set_scan_time_offsets_dev.argtypes = [vp, vp]
    lib.rplgpu_comm_unique_id.argtypes = [vp]
    lib.rplgpu_comm_init.argtypes = [vp, i32, i32, vp]
    lib.rplgpu_comm_destroy.argtypes = [vp]
    lib.rplgpu_comm_size.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.rplgpu_cloud_meta_words.argtypes = [u32]
    lib.rplgpu_cloud_meta_words.restype = u32
    lib.rplgpu_pack_cloud_meta_dev.argtypes = [vp, vp, vp, vp, u32, u64, u32, vp]
    lib.rplgpu_allgather_clouds_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    lib.rplgpu_gather_clouds_dev.argtypes = [vp, i32, vp, u64, u32, vp, u32, vp, vp]
    lib.rplgpu_comm_fence.argtypes = [vp]
    lib.rplgpu_comm_fence_lag.argtypes = [vp, u32]
    lib.rplgpu_unpack_gathered_dev.argtypes = [vp, vp, u64, vp, u32, u32, u32, vp, vp, vp, vp, vp]
    lib.rplgpu_pack_cloud_xyi_dev.argtypes = [vp, vp, vp, u64, vp]
    lib.rplgpu_allgather_clouds_xyi_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    lib.rplgpu_unpack_gathered_xyi_dev.argtypes = [vp, vp, u64, vp, u32, u32, u32, vp, vp, vp, vp, vp]
    lib.rplgpu_pack_cloud_meta_host.argtypes = [u64, vp, vp, u32, u64, u32, vp]
    lib.rplgpu_pack_cloud_xyi_host.argtypes = [vp, u64, u64, vp]
    lib.rplgpu_unpack_gathered_host.argtypes = [vp, u64, u32, vp, u32, u32, u32, vp, vp, vp, vp, vp]
    lib.rplgpu_cloud_fused_cells_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp, vp,
                                                 u64, vp, vp, vp, vp]
    lib.rplgpu_gather_cells_dev.argtypes = [vp, i32, vp, u64, vp, u32, vp, vp]
    lib.rplgpu_merge_cells_dev.argtypes = [vp, vp, u64, vp, u32, u32, u32, C.POINTER(Params), vp, u64, vp,
                                           vp, vp, vp]
    lib.rplgpu_merge_cells_host.argtypes = [vp, u64, vp, u32, u32, u32, C.POINTER(Params), vp, u64, vp, vp,
                                            vp, vp]
    lib.rplgpu_scan_merge_edges.argtypes = [C.POINTER(ScanMerge), vp, vp]
    lib.rplgpu_merge_scans_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp,
                                           C.POINTER(ScanMerge), vp, vp, vp, vp]
    lib.rplgpu_merged_laserscan_msgs_dev.argtypes = [vp, vp, vp, u32, C.POINTER(ScanMerge), cs, vp, vp, u32,
                                                     vp, vp]
    lib.rplgpu_default_scan_filter.argtypes = [C.POINTER(ScanFilter)]
    lib.rplgpu_default_scan_filter.restype = None
    lib.rplgpu_scan_filter_check.argtypes = [C.POINTER(ScanFilter), vp]
    lib.rplgpu_filter_laserscan_batch_dev.argtypes = [vp, vp, vp, u32, vp, u32, C.POINTER(Params),
                                                      C.POINTER(ScanFilter), vp, vp, vp]
    lib.rplgpu_filter_merged_scans_dev.argtypes = [vp, vp, vp, u32, C.POINTER(ScanMerge),
                                                   C.POINTER(ScanFilter), vp, vp, vp]
    lib.rplgpu_filter_laserscan.argtypes = [vp, vp, vp, u32, C.c_float, C.POINTER(ScanFilter), vp, vp, vp]
    lib.rplgpu_default_occ_grid.argtypes = [C.POINTER(OccGrid)]
    lib.rplgpu_default_occ_grid.restype = None
    lib.rplgpu_occ_grid_check.argtypes = [C.POINTER(OccGrid)]
    lib.rplgpu_occupancy_grid_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp,
                                              C.POINTER(OccGrid), vp, vp, u64, vp, vp]
    lib.rplgpu_occupancy_grid.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp,
                                          C.POINTER(OccGrid), vp, vp, vp, vp]
    lib.rplgpu_msg_occupancy_layout.argtypes = [sz, u32, u32, C.POINTER(OccupancyLayout)]
    lib.rplgpu_occupancy_grid_msgs_dev.argtypes = [vp, vp, u64, u32, C.POINTER(OccGrid), cs, vp, vp, u32, vp, vp]
    lib.rplgpu_default_inflation.argtypes = [C.POINTER(Inflation)]
    lib.rplgpu_default_inflation.restype = None
    lib.rplgpu_inflation_check.argtypes = [C.POINTER(Inflation), C.c_float]
    lib.rplgpu_inflation_table.argtypes = [C.POINTER(Inflation), C.c_float, vp, u32, vp]
    lib.rplgpu_inflate_grids_dev.argtypes = [vp, vp, u64, vp, u64, u32, u32, u32, vp, u32, u32, vp]
    lib.rplgpu_inflate_grid.argtypes = [vp, vp, u32, u32, C.c_float, C.POINTER(Inflation), vp, vp]
    lib.rplgpu_default_scan_match.argtypes = [C.POINTER(ScanMatch)]
    lib.rplgpu_default_scan_match.restype = None
    lib.rplgpu_scan_match_check.argtypes = [C.POINTER(ScanMatch)]
    lib.rplgpu_scan_match_rotations.argtypes = [C.POINTER(ScanMatch), vp]
    lib.rplgpu_scan_match_volume.argtypes = [C.POINTER(ScanMatch)]
    lib.rplgpu_scan_match_volume.restype = u32
    lib.rplgpu_match_scans_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp, vp,
                                           C.POINTER(ScanMatch), vp, u64, u32, vp, u64, vp, vp]
    lib.rplgpu_match_scans.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp, vp,
                                       C.POINTER(ScanMatch), vp, vp, vp, vp]
    lib.rplgpu_map_update_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp,
                                          C.POINTER(OccGrid), vp, vp]
    lib.rplgpu_default_map_rule.argtypes = [C.POINTER(MapRule)]
    lib.rplgpu_default_map_rule.restype = None
    lib.rplgpu_map_rule_check.argtypes = [C.POINTER(MapRule)]
    lib.rplgpu_map_grid_dev.argtypes = [vp, vp, u32, u32, C.POINTER(MapRule), vp, vp, u64, vp]
    lib.rplgpu_apply_match_dev.argtypes = [vp, vp, C.POINTER(ScanMatch), vp, vp, u32, u32, u32, vp, vp]
    lib.rplgpu_map_update.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp, C.POINTER(OccGrid),
                                      vp, vp]
    lib.rplgpu_map_grid.argtypes = [vp, vp, u32, u32, C.POINTER(MapRule), vp, vp, vp]
    lib.rplgpu_default_pose_score.argtypes = [C.POINTER(PoseScore)]
    lib.rplgpu_default_pose_score.restype = None
    lib.rplgpu_pose_score_check.argtypes = [C.POINTER(PoseScore)]
    lib.rplgpu_pose_list.argtypes = [vp, u32, vp]
    lib.rplgpu_score_poses_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp,
                                           C.POINTER(PoseScore), vp, u32, u64, u32, vp, u64, u32, vp, u64, vp, vp]
    lib.rplgpu_score_poses.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp,
                                       C.POINTER(PoseScore), vp, u32, vp, vp, vp, vp]
    lib.rplgpu_resample_scratch_words.argtypes = [u32, u32]
    lib.rplgpu_resample_scratch_words.restype = C.c_uint64
    lib.rplgpu_resample_poses_dev.argtypes = [vp, vp, u64, vp, u64, u32, u32, u32, u32, vp, vp, u32, u64, u32, vp,
                                              u64, vp, u64, vp, vp]
    lib.rplgpu_resample_host.argtypes = [vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_resample_poses.argtypes = [vp, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_default_pose_estimate.argtypes = [C.POINTER(PoseEstimate)]
    lib.rplgpu_default_pose_estimate.restype = None
    lib.rplgpu_pose_estimate_check.argtypes = [C.POINTER(PoseEstimate)]
    lib.rplgpu_estimate_scratch_words.argtypes = [u32, u32]
    lib.rplgpu_estimate_scratch_words.restype = C.c_uint64
    lib.rplgpu_estimate_poses_dev.argtypes = [vp, vp, u64, u32, vp, u64, u32, u32, C.POINTER(PoseEstimate), vp, u64,
                                              vp, vp]
    lib.rplgpu_estimate_host.argtypes = [vp, u32, vp, C.POINTER(PoseEstimate), u32, vp]
    lib.rplgpu_estimate_poses.argtypes = [vp, vp, u32, vp, C.POINTER(PoseEstimate), u32, vp]
    lib.rplgpu_estimate_pose.argtypes = [vp, C.c_float, u32, vp]
    lib.rplgpu_default_motion_noise.argtypes = [C.POINTER(MotionNoise)]
    lib.rplgpu_default_motion_noise.restype = None
    lib.rplgpu_sample_motion_dev.argtypes = [vp, vp, u32, u32, u32, C.POINTER(MotionNoise), vp, u64, vp]
    lib.rplgpu_sample_motion_host.argtypes = [vp, u32, u32, C.POINTER(MotionNoise), vp, vp]
    lib.rplgpu_sample_motion.argtypes = [vp, vp, u32, C.POINTER(MotionNoise), vp, vp]
    lib.rplgpu_philox4x32.argtypes = [vp, vp, vp]
    lib.rplgpu_motion_odometry.argtypes = [C.c_double, C.c_double, C.c_double, vp, vp]
    lib.rplgpu_default_pose_seed.argtypes = [C.POINTER(PoseSeed)]
    lib.rplgpu_default_pose_seed.restype = None
    lib.rplgpu_pose_seed_check.argtypes = [C.POINTER(PoseSeed)]
    lib.rplgpu_seed_scratch_words.argtypes = [u32, u32, u32]
    lib.rplgpu_seed_scratch_words.restype = C.c_uint64
    lib.rplgpu_seed_headings.argtypes = [u32, vp]
    lib.rplgpu_seed_poses_dev.argtypes = [vp, C.POINTER(PoseSeed), vp, u64, u32, vp, u32, u32, u32,
                                          C.POINTER(MotionNoise), vp, u64, vp, u64, vp, vp]
    lib.rplgpu_seed_poses_host.argtypes = [C.POINTER(PoseSeed), vp, vp, u32, u32, u32, C.POINTER(MotionNoise), vp, vp,
                                           vp]
    lib.rplgpu_seed_poses.argtypes = [vp, C.POINTER(PoseSeed), vp, vp, u32, u32, C.POINTER(MotionNoise), vp, vp, vp]
    lib.rplgpu_default_pose_bins.argtypes = [C.POINTER(PoseBins)]
    lib.rplgpu_default_pose_bins.restype = None
    lib.rplgpu_pose_bins_check.argtypes = [C.POINTER(PoseBins), u32]
    lib.rplgpu_bin_map_words.argtypes = [u32, u32, u32]
    lib.rplgpu_bin_map_words.restype = C.c_uint64
    lib.rplgpu_heading_edges_check.argtypes = [vp, u32]
    lib.rplgpu_bin_poses_dev.argtypes = [vp, C.POINTER(PoseBins), vp, u64, u32, vp, u64, u32, u32, vp, u32, vp, u64, vp,
                                         u64, vp]
    lib.rplgpu_bin_poses_host.argtypes = [C.POINTER(PoseBins), vp, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_bin_poses.argtypes = [vp, C.POINTER(PoseBins), vp, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_kld_samples.argtypes = [u32, C.c_double, C.c_double, u32, u32]
    lib.rplgpu_kld_samples.restype = C.c_uint32
    lib.rplgpu_default_pose_clusters.argtypes = [C.POINTER(PoseClusters)]
    lib.rplgpu_default_pose_clusters.restype = None
    lib.rplgpu_pose_clusters_check.argtypes = [C.POINTER(PoseClusters), u32]
    lib.rplgpu_cluster_scratch_words.argtypes = [u32, u32, u32, u32, u32]
    lib.rplgpu_cluster_scratch_words.restype = C.c_uint64
    lib.rplgpu_cluster_poses_dev.argtypes = [vp, C.POINTER(PoseClusters), vp, u64, u32, vp, u64, u32, u32, u32, vp, u64,
                                             vp, u64, vp, u64, vp, u64, u32, vp, vp]
    lib.rplgpu_cluster_poses_host.argtypes = [C.POINTER(PoseClusters), vp, u32, vp, u32, vp, vp, vp, vp, u32, vp]
    lib.rplgpu_cluster_poses.argtypes = [vp, C.POINTER(PoseClusters), vp, u32, vp, u32, vp, vp, vp, vp, u32, vp]
    lib.rplgpu_default_range_cast.argtypes = [C.POINTER(RangeCast)]
    lib.rplgpu_default_range_cast.restype = None
    lib.rplgpu_range_cast_check.argtypes = [C.POINTER(RangeCast)]
    lib.rplgpu_cast_beams.argtypes = [C.POINTER(ScanMerge), u32, u32, u32, vp]
    lib.rplgpu_cast_range_m.argtypes = [u32, C.c_float]
    lib.rplgpu_cast_range_m.restype = C.c_double
    lib.rplgpu_cast_ranges_dev.argtypes = [vp, C.POINTER(RangeCast), vp, u64, u32, u32, u32, vp, u32, vp, u64, u32, vp,
                                           u64, u32, u32, vp, vp, u64, vp, u64, vp, vp]
    lib.rplgpu_cast_ranges_host.argtypes = [C.POINTER(RangeCast), vp, u32, vp, u32, vp, vp, u32, u32, u32, vp, vp, vp,
                                            vp, vp]
    lib.rplgpu_cast_ranges.argtypes = [vp, C.POINTER(RangeCast), vp, u32, vp, u32, vp, vp, u32, u32, u32, vp, vp, vp,
                                       vp, vp]
    lib.rplgpu_default_beam_agree.argtypes = [C.POINTER(BeamAgree)]
    lib.rplgpu_default_beam_agree.restype = None
    lib.rplgpu_beam_agree_check.argtypes = [C.POINTER(BeamAgree)]
    lib.rplgpu_score_poses_agree_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp,
                                                 C.POINTER(BeamAgree), vp, u32, u64, u32, vp, u64, u32, vp, u64, vp,
                                                 vp, vp, u64, vp, u64, vp]
    lib.rplgpu_score_poses_agree.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp,
                                             C.POINTER(BeamAgree), vp, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.rplgpu_beam_agree_points_host.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp, u32, vp, C.POINTER(BeamAgree),
                                                  vp, vp, vp, vp, vp, vp]
    lib.rplgpu_default_wide_match.argtypes = [C.POINTER(WideMatch)]
    lib.rplgpu_default_wide_match.restype = None
    lib.rplgpu_wide_match_check.argtypes = [C.POINTER(WideMatch)]
    lib.rplgpu_wide_match_blocks.argtypes = [C.POINTER(WideMatch)]
    lib.rplgpu_wide_match_blocks.restype = u32
    lib.rplgpu_wide_match_scratch_words.argtypes = [C.POINTER(WideMatch), u32]
    lib.rplgpu_wide_match_scratch_words.restype = u64
    lib.rplgpu_pool_field_host.argtypes = [vp, u32, u32, vp]
    lib.rplgpu_pool_field_dev.argtypes = [vp, C.POINTER(WideMatch), vp, u64, u32, vp, u64]
    lib.rplgpu_match_wide_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp, vp,
                                          C.POINTER(WideMatch), vp, u64, u32, vp, u64, vp, u64, vp, vp, vp, vp]
    lib.rplgpu_match_wide.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp, vp,
                                      C.POINTER(WideMatch), vp, vp, vp, vp, vp]
    lib.rplgpu_default_pose_refine.argtypes = [C.POINTER(PoseRefine)]
    lib.rplgpu_default_pose_refine.restype = None
    lib.rplgpu_pose_refine_check.argtypes = [C.POINTER(PoseRefine)]
    lib.rplgpu_refine_scratch_words.argtypes = [u32, u32]
    lib.rplgpu_refine_scratch_words.restype = u64
    lib.rplgpu_refine_sums_host.argtypes = [vp, vp, u32, vp, u32, vp, C.POINTER(PoseRefine), vp, vp, vp]
    lib.rplgpu_refine_step_host.argtypes = [vp, C.POINTER(PoseRefine), vp, vp, vp]
    lib.rplgpu_refine_covariance.argtypes = [vp, C.POINTER(PoseRefine), vp]
    lib.rplgpu_refine_sums_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp,
                                           C.POINTER(PoseRefine), vp, u32, u64, u32, vp, u64, u32, vp, u64, vp, vp,
                                           vp]
    lib.rplgpu_refine_step_dev.argtypes = [vp, vp, u64, C.POINTER(PoseRefine), vp, u64, u32, u32, u32, vp, u64, vp,
                                           u64, vp]
    lib.rplgpu_refine_poses_dev.argtypes = [vp, vp, u32, vp, u32, u32, C.POINTER(Params), vp, vp,
                                            C.POINTER(PoseRefine), vp, u32, u64, u32, vp, u64, u32, u32, vp, u64, vp,
                                            u64, vp, u64, vp, vp, vp]
    lib.rplgpu_refine_poses.argtypes = [vp, vp, u32, vp, u32, C.POINTER(Params), vp, vp, vp, C.POINTER(PoseRefine),
                                        vp, u32, vp, u32, vp, vp, vp, vp, vp]
    lib.rplgpu_match_poses_dev.argtypes = [vp, vp, C.POINTER(ScanMatch), vp, vp, u32, vp, u64]
    lib.rplgpu_compose_poses_dev.argtypes = [vp, vp, u64, u32, u32, vp, u32, vp, u32, u32, vp]
    lib.rplgpu_default_nav_field.argtypes = [C.POINTER(NavField)]
    lib.rplgpu_default_nav_field.restype = None
    lib.rplgpu_nav_field_check.argtypes = [C.POINTER(NavField)]
    lib.rplgpu_nav_field_default_rounds.argtypes = [u32, u32]
    lib.rplgpu_nav_field_default_rounds.restype = u32
    lib.rplgpu_nav_field_scratch_words.argtypes = [C.POINTER(NavField), u32]
    lib.rplgpu_nav_field_scratch_words.restype = u64
    lib.rplgpu_nav_field_host.argtypes = [C.POINTER(NavField), vp, vp, u32, vp, vp]
    lib.rplgpu_nav_path_host.argtypes = [C.POINTER(NavField), vp, vp, u32, vp, u32, vp]
    lib.rplgpu_nav_field_dev.argtypes = [vp, C.POINTER(NavField), vp, u64, u32, vp, u64, vp, vp, u64, vp, u32, vp]
    lib.rplgpu_nav_paths_dev.argtypes = [vp, C.POINTER(NavField), vp, u64, vp, u64, u32, vp, u32, vp, u32, vp]
    lib.rplgpu_nav_field.argtypes = [vp, C.POINTER(NavField), vp, vp, u32, vp, vp, vp, u32, vp, u32, vp]
    lib.rplgpu_default_rollout.argtypes = [C.POINTER(Rollout)]
    lib.rplgpu_default_rollout.restype = None
    lib.rplgpu_rollout_check.argtypes = [C.POINTER(Rollout)]
    lib.rplgpu_rollout_scratch_words.argtypes = [u32, u32]
    lib.rplgpu_rollout_scratch_words.restype = u64
    lib.rplgpu_rollout_deltas.argtypes = [vp, u32, C.c_double, vp]
    lib.rplgpu_rollout_host.argtypes = [C.POINTER(Rollout), vp, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_rollout_dev.argtypes = [vp, C.POINTER(Rollout), vp, u32, vp, u64, u32, u32, vp, u32, vp, u64, vp, u64,
                                       u32, u32, u32, vp, u64, vp, u64, vp, vp]
    lib.rplgpu_rollout.argtypes = [vp, C.POINTER(Rollout), vp, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_default_mppi.argtypes = [C.POINTER(Mppi)]
    lib.rplgpu_default_mppi.restype = None
    lib.rplgpu_mppi_check.argtypes = [C.POINTER(Mppi)]
    lib.rplgpu_mppi_scratch_words.argtypes = [u32, u32, u32]
    lib.rplgpu_mppi_scratch_words.restype = u64
    lib.rplgpu_mppi_table.argtypes = [C.c_double, u32, u32, vp]
    lib.rplgpu_mppi_update_host.argtypes = [C.POINTER(Mppi), vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    lib.rplgpu_mppi_update_dev.argtypes = [vp, C.POINTER(Mppi), vp, u64, vp, vp, u64, u32, vp, vp, u64, u32, u32, u32,
                                           vp, u64, vp, u64, vp, u64, vp, vp]
    lib.rplgpu_mppi_update.argtypes = [vp, C.POINTER(Mppi), vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    lib.rplgpu_mppi_spread_host.argtypes = [vp, u32, vp, u32, u32, u32, u32, vp]
    lib.rplgpu_mppi_spread_dev.argtypes = [vp, vp, u64, u32, u32, vp, u64, u32, u32, u32, u32, u32, u32, vp, u64]
    lib.rplgpu_mppi_spread.argtypes = [vp, vp, u32, vp, u32, u32, u32, u32, vp]
    lib.rplgpu_default_frontiers.argtypes = [C.POINTER(Frontiers)]
    lib.rplgpu_default_frontiers.restype = None
    lib.rplgpu_frontiers_check.argtypes = [C.POINTER(Frontiers)]
    lib.rplgpu_frontiers_scratch_words.argtypes = [C.POINTER(Frontiers), u32, u32]
    lib.rplgpu_frontiers_scratch_words.restype = u64
    lib.rplgpu_frontiers_host.argtypes = [C.POINTER(Frontiers), vp, vp, u32, vp, vp, u32, vp, vp, vp]
    lib.rplgpu_frontiers_dev.argtypes = [vp, C.POINTER(Frontiers), vp, u64, vp, u64, u32, u32, vp, u64, vp, u64, u32,
                                         vp, u64, vp, vp, vp]
    lib.rplgpu_frontiers.argtypes = [vp, C.POINTER(Frontiers), vp, vp, u32, vp, vp, u32, vp, vp, vp]
    for name in ABI_SYMBOLS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int:  # default
            fn.restype = i32
    _LIB = lib
    return lib


def _nodes_ptr(arr: np.ndarray) -> int:
    if arr.dtype != NODE_DTYPE or not arr.flags["C_CONTIGUOUS"]:
        raise TypeError("nodes must be a C-contiguous array of NODE_DTYPE")
    return arr.ctypes.data


class RplGpu:
    """One ``rplgpu_handle_t`` (== one lidar node instance / one GPU stream)."""

    def __init__(self, device: int = 0, max_samples_per_scan: int = MAX_SAMPLES_PER_SCAN,
                 max_batch: int = 4096):
        self._lib = load_library()
        self._pinned = {}
        h = C.c_void_p()
        rc = self._lib.rplgpu_create(device, max_samples_per_scan, max_batch, C.byref(h))
        if rc != OK:
            msg = self._lib.rplgpu_last_error(None) or b""
            raise RplGpuError(rc, "rplgpu_create failed: " + msg.decode())
        self._h = h
        self.device = device
        self.max_samples_per_scan = max_samples_per_scan
        self.max_batch = max_batch

    # -- lifecycle -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.rplgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, allow=()):
        if rc != OK and rc not in allow:
            msg = self._lib.rplgpu_last_error(self._h) or b""
            raise RplGpuError(rc, msg.decode())
        return rc

    def set_stream(self, hip_stream_ptr: int | None):
        self._check(self._lib.rplgpu_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)))

    def synchronize(self):
        self._check(self._lib.rplgpu_synchronize(self._h))

    # -- single scan, host buffers -----------------------------------------------------
    def ascend(self, nodes: np.ndarray) -> int:
        """In place; returns the SDK ``sl_result`` (0 or 0x80008001)."""
        res = C.c_uint32(0)
        self._check(self._lib.rplgpu_ascend(self._h, _nodes_ptr(nodes), len(nodes), C.byref(res)))
        return res.value

    def scan_to_laserscan(self, nodes: np.ndarray, params: Params, scan_duration: float = 0.1):
        n = len(nodes)
        ranges = np.empty(max(n, 1), np.float32)
        intens = np.empty(max(n, 1), np.float32)
        meta = ScanMeta()
        self._check(self._lib.rplgpu_scan_to_laserscan(
            self._h, _nodes_ptr(nodes), n, C.byref(params), scan_duration,
            ranges.ctypes.data, intens.ctypes.data, C.byref(meta)))
        return ranges[: meta.count], intens[: meta.count], meta

    def scan_to_cloud(self, nodes: np.ndarray, params: Params, allow_overflow: bool = False):
        n = len(nodes)
        xyzi = np.empty((max(n, 1), 4), np.float32)
        npts = C.c_uint32(0)
        status = C.c_uint32(0)
        self._check(self._lib.rplgpu_scan_to_cloud(
            self._h, _nodes_ptr(nodes), n, C.byref(params), xyzi.ctypes.data,
            C.byref(npts), C.byref(status)),
            allow=(ERR_SCAN_OVERFLOW,) if allow_overflow else ())
        return xyzi[: npts.value], status.value

    # -- device-resident batches (raw device pointers, e.g. torch ``data_ptr()``) ---------
    def ascend_batch_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int,
                         d_status: int = 0):
        self._check(self._lib.rplgpu_ascend_batch_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, d_status))

    def laserscan_batch_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int,
                            params: Params, d_ranges: int, d_intens: int, d_beam_count: int):
        self._check(self._lib.rplgpu_laserscan_batch_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, C.byref(params),
            d_ranges, d_intens, d_beam_count))

    def ascend_laserscan_batch_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int,
                                   params: Params, d_ranges: int, d_intens: int, d_beam_count: int,
                                   write_ascended: bool = False, d_status: int = 0):
        """S1 -> S3 (grab_scan_data with geometric correction, then publish_scan) in one pass."""
        self._check(self._lib.rplgpu_ascend_laserscan_batch_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, C.byref(params),
            d_ranges, d_intens, d_beam_count, int(bool(write_ascended)), d_status))

    def cloud_batch_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int,
                        params: Params, d_xyzi: int, out_stride: int, d_n_points: int,
                        d_status: int = 0):
        self._check(self._lib.rplgpu_cloud_batch_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, C.byref(params),
            d_xyzi, out_stride, d_n_points, d_status))

    def cloud_arena_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int,
                        params: Params, d_arena: int, arena_capacity: int, d_cursor: int,
                        d_scan_start: int, d_n_points: int, d_status: int = 0):
        """Voxelised clouds of the batch in one contiguous arena (no packing pass)."""
        self._check(self._lib.rplgpu_cloud_arena_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, C.byref(params), d_arena,
            arena_capacity, d_cursor, d_scan_start, d_n_points, d_status))

    def pack_clouds_dev(self, d_xyzi: int, out_stride: int, d_n_points: int, B: int,
                        d_packed: int, d_offsets: int):
        self._check(self._lib.rplgpu_pack_clouds_dev(
            self._h, d_xyzi, out_stride, d_n_points, B, d_packed, d_offsets))

    def fill_meta(self, params: Params, count: int, scan_duration: float) -> ScanMeta:
        meta = ScanMeta()
        self._lib.rplgpu_fill_meta(C.byref(params), count, scan_duration, C.byref(meta))
        return meta

    # -- serialised messages (include/rplgpu_msg.h) ----------------------
    def host_alloc(self, nbytes: int) -> np.ndarray:
        """Pinned host bytes (``rplgpu_host_alloc``) as a uint8 array; free with ``host_free``."""
        ptr = C.c_void_p()
        self._check(self._lib.rplgpu_host_alloc(self._h, nbytes, C.byref(ptr)))
        buf = (C.c_uint8 * nbytes).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=np.uint8)
        self._pinned[arr.ctypes.data] = ptr.value
        return arr

    def host_free(self, arr: np.ndarray):
        ptr = self._pinned.pop(arr.ctypes.data)
        self._check(self._lib.rplgpu_host_free(self._h, ptr))

    def scan_to_laserscan_msg(self, nodes: np.ndarray, params: Params, scan_duration: float,
                              frame_id: str, sec: int, nanosec: int, out: np.ndarray | None = None):
        """Serialised sensor_msgs/LaserScan of one scan: ``(bytes view, meta)``; the view is
        empty when publish_scan would not have published."""
        n = len(nodes)
        if out is None:
            out = np.empty(msg_laserscan_layout(len(frame_id.encode()), max(n, 1)).total_len,
                           np.uint8)
        meta = ScanMeta()
        ln = C.c_size_t(0)
        self._check(self._lib.rplgpu_scan_to_laserscan_msg(
            self._h, _nodes_ptr(nodes), n, C.byref(params), scan_duration, frame_id.encode(),
            Stamp(sec, nanosec), out.ctypes.data, out.nbytes, C.byref(ln), C.byref(meta)))
        return out[: ln.value], meta

    def scan_to_cloud_msg(self, nodes: np.ndarray, params: Params, frame_id: str, sec: int,
                          nanosec: int, out: np.ndarray | None = None,
                          allow_overflow: bool = False):
        """Serialised sensor_msgs/PointCloud2 of one scan: ``(bytes view, n_points, status)``."""
        n = len(nodes)
        if out is None:
            out = np.empty(msg_cloud_layout(len(frame_id.encode()), max(n, 1)).total_len, np.uint8)
        ln = C.c_size_t(0)
        npts, status = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.rplgpu_scan_to_cloud_msg(
            self._h, _nodes_ptr(nodes), n, C.byref(params), frame_id.encode(),
            Stamp(sec, nanosec), out.ctypes.data, out.nbytes, C.byref(ln), C.byref(npts),
            C.byref(status)), allow=(ERR_SCAN_OVERFLOW,) if allow_overflow else ())
        return out[: ln.value], npts.value, status.value

    def laserscan_msgs_dev(self, d_ranges: int, d_intens: int, n_stride: int, d_beam_count: int,
                           B: int, params: Params, frame_id: str, d_stamps: int,
                           d_scan_duration: int, d_msgs: int, msg_stride: int, d_msg_len: int,
                           d_status: int = 0):
        self._check(self._lib.rplgpu_laserscan_msgs_dev(
            self._h, d_ranges, d_intens, n_stride, d_beam_count, B, C.byref(params),
            frame_id.encode(), d_stamps, d_scan_duration, d_msgs, msg_stride, d_msg_len, d_status))

    def cloud_msgs_dev(self, d_xyzi: int, out_stride: int, d_scan_start: int, d_n_points: int,
                       B: int, frame_id: str, d_stamps: int, d_msgs: int, msg_stride: int,
                       d_msg_len: int, d_status: int = 0):
        self._check(self._lib.rplgpu_cloud_msgs_dev(
            self._h, d_xyzi, out_stride, d_scan_start, d_n_points, B, frame_id.encode(),
            d_stamps, d_msgs, msg_stride, d_msg_len, d_status))

    def transform_clouds_dev(self, d_xyzi: int, out_stride: int, d_scan_start: int,
                             d_n_points: int, B: int, d_pose: int):
        """In-place rigid transform of B clouds, one row-major 3x4 float pose per scan."""
        self._check(self._lib.rplgpu_transform_clouds_dev(
            self._h, d_xyzi, out_stride, d_scan_start, d_n_points, B, d_pose))

    def cloud_deskew_batch_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int,
                               params: Params, d_motion: int, d_xyzi: int, out_stride: int,
                               d_n_points: int, d_status: int = 0):
        """Plain clouds with motion de-skew; d_motion: B x (vx, vy, wz, time_increment) float32."""
        self._check(self._lib.rplgpu_cloud_deskew_batch_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, C.byref(params), d_motion, d_xyzi,
            out_stride, d_n_points, d_status))

    def laserscan_to_cloud_batch_dev(self, d_ranges: int, d_intens: int, n_stride: int,
                                     d_beam_count: int, B: int, params: Params, d_xyzi: int,
                                     out_stride: int, d_n_points: int, d_status: int = 0):
        """E7: the LaserScans of a batch projected to clouds (laser_geometry-style)."""
        self._check(self._lib.rplgpu_laserscan_to_cloud_batch_dev(
            self._h, d_ranges, d_intens, n_stride, d_beam_count, B, C.byref(params), d_xyzi,
            out_stride, d_n_points, d_status))

    def laserscan_to_cloud(self, ranges: np.ndarray, intens: np.ndarray, params: Params):
        """E7, one scan, host buffers: (count,) float32 ranges / intensities -> (m, 4) cloud."""
        ranges = np.ascontiguousarray(ranges, np.float32)
        intens = np.ascontiguousarray(intens, np.float32)
        count = len(ranges)
        xyzi = np.empty((max(count, 1), 4), np.float32)
        npts = C.c_uint32(0)
        self._check(self._lib.rplgpu_laserscan_to_cloud(
            self._h, ranges.ctypes.data, intens.ctypes.data, count, C.byref(params),
            xyzi.ctypes.data, C.byref(npts)))
        return xyzi[: npts.value]

    def cloud_fused_voxel_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int,
                              params: Params, d_motion: int, d_pose2d: int, d_arena: int,
                              arena_capacity: int, d_cursor: int, d_group_start: int, d_n_points: int,
                              d_status: int = 0):
        """E8: one voxel grid per group of `group` consecutive scans (de-skew + planar pose)."""
        self._check(self._lib.rplgpu_cloud_fused_voxel_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d,
            d_arena, arena_capacity, d_cursor, d_group_start, d_n_points, d_status))

    def merge_scans_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int,
                        params: Params, d_motion: int, d_pose2d: int, merge: ScanMerge, d_ranges: int,
                        d_intens: int, d_beams_hit: int, d_status: int = 0):
        """E9: one merged LaserScan (merge.count beams) per group of `group` consecutive scans."""
        self._check(self._lib.rplgpu_merge_scans_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d,
            C.byref(merge), d_ranges, d_intens, d_beams_hit, d_status))

    def merged_laserscan_msgs_dev(self, d_ranges: int, d_intens: int, G: int, merge: ScanMerge,
                                  frame_id: str, d_stamps: int, d_msgs: int, msg_stride: int,
                                  d_msg_len: int, d_status: int = 0):
        """G serialised LaserScans of merged scans (rplgpu_merged_laserscan_msgs_dev)."""
        self._check(self._lib.rplgpu_merged_laserscan_msgs_dev(
            self._h, d_ranges, d_intens, G, C.byref(merge), frame_id.encode(), d_stamps, d_msgs,
            msg_stride, d_msg_len, d_status))

    def occupancy_grid_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int,
                           params: Params, d_motion: int, d_pose2d: int, grid: OccGrid, d_prev: int,
                           d_grid: int, grid_stride: int, d_cells: int = 0, d_status: int = 0):
        """E11: one ray-cast occupancy grid (int8, grid.width x grid.height) per group of scans."""
        self._check(self._lib.rplgpu_occupancy_grid_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d,
            C.byref(grid), d_prev, d_grid, grid_stride, d_cells, d_status))

    def occupancy_grid(self, scans: np.ndarray, lens, params: Params, grid: OccGrid, motion=None,
                       pose2d=None, t0=None, prev=None):
        """E11, one group, host buffers: scans (S, n) NODE_DTYPE -> ``(grid (height, width) int8,
        (cells 0, cells 100, cells -1), status)``."""
        scans = np.ascontiguousarray(scans)
        if scans.dtype != NODE_DTYPE or scans.ndim != 2:
            raise TypeError("scans must be a 2-D array of abi.NODE_DTYPE")
        S, n = scans.shape
        lens = np.ascontiguousarray(lens, np.uint32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        motion, pose2d, t0 = f32(motion), f32(pose2d), f32(t0)
        prev = None if prev is None else np.ascontiguousarray(prev, np.int8)
        out = np.empty((grid.height, grid.width), np.int8)
        cells = np.zeros(3, np.uint32)
        status = np.zeros(1, np.uint32)
        ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.rplgpu_occupancy_grid(
            self._h, scans.ctypes.data, n, lens.ctypes.data, S, C.byref(params), ptr(motion), ptr(pose2d),
            ptr(t0), C.byref(grid), ptr(prev), out.ctypes.data, cells.ctypes.data, status.ctypes.data))
        return out, tuple(int(c) for c in cells), int(status[0])

    def occupancy_grid_msgs_dev(self, d_grid: int, grid_stride: int, G: int, grid: OccGrid, frame_id: str,
                                d_stamps: int, d_msgs: int, msg_stride: int, d_msg_len: int,
                                d_status: int = 0):
        """G serialised nav_msgs/OccupancyGrid messages of the grids occupancy_grid_dev wrote."""
        self._check(self._lib.rplgpu_occupancy_grid_msgs_dev(
            self._h, d_grid, grid_stride, G, C.byref(grid), frame_id.encode(), d_stamps, d_msgs, msg_stride,
            d_msg_len, d_status))

    def inflate_grids_dev(self, d_in: int, in_stride: int, d_out: int, out_stride: int, G: int, width: int,
                          height: int, d_table: int, rc: int, inflate_unknown: int = 0, d_cells: int = 0):
        """E12: G grids (int8, width x height) inflated into costmaps with the device table of
        ``inflation_table`` (rc * rc + 1 bytes); d_cells: 4 words per grid (100, 99, 1 .. 98, -1)."""
        self._check(self._lib.rplgpu_inflate_grids_dev(
            self._h, d_in, in_stride, d_out, out_stride, G, width, height, d_table, rc, inflate_unknown,
            d_cells))

    def inflate_grid(self, grid: np.ndarray, resolution: float, inflation: Inflation):
        """E12, one grid, host buffers: (height, width) int8 -> ``(costmap (height, width) int8,
        (cells 100, cells 99, cells 1 .. 98, cells -1))``."""
        grid = np.ascontiguousarray(grid, np.int8)
        if grid.ndim != 2:
            raise TypeError("grid must be a 2-D int8 array (height, width)")
        out = np.empty_like(grid)
        cells = np.zeros(4, np.uint32)
        self._check(self._lib.rplgpu_inflate_grid(
            self._h, grid.ctypes.data, grid.shape[1], grid.shape[0], resolution, C.byref(inflation),
            out.ctypes.data, cells.ctypes.data))
        return out, tuple(int(c) for c in cells)

    def match_scans_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int, params: Params,
                        d_motion: int, d_pose2d: int, d_pivot: int, match: ScanMatch, d_field: int,
                        field_stride: int, field_per_group: int, d_scores: int, score_stride: int, d_best: int,
                        d_status: int = 0):
        """E13: per group of scans the score volume (uint32, ``scan_match_volume`` words, score_stride apart) of
        the search window over the int8 field(s) at d_field, and eight result words at d_best + 8 g."""
        self._check(self._lib.rplgpu_match_scans_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d, d_pivot,
            C.byref(match), d_field, field_stride, field_per_group, d_scores, score_stride, d_best, d_status))

    def match_scans(self, scans: np.ndarray, lens, params: Params, match: ScanMatch, field: np.ndarray,
                    motion=None, pose2d=None, t0=None, pivot=None, want_scores: bool = True):
        """E13, one group, host buffers: scans (S, n) NODE_DTYPE and a (height, width) int8 field ->
        ``(scores (2K+1, 2Ty+1, 2Tx+1) uint32 or None, best (8,) uint32, status)``."""
        scans = np.ascontiguousarray(scans)
        if scans.dtype != NODE_DTYPE or scans.ndim != 2:
            raise TypeError("scans must be a 2-D array of abi.NODE_DTYPE")
        field = np.ascontiguousarray(field, np.int8)
        if field.shape != (match.height, match.width):
            raise TypeError("field must be a (height, width) int8 array")
        S, n = scans.shape
        lens = np.ascontiguousarray(lens, np.uint32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        motion, pose2d, t0, pivot = f32(motion), f32(pose2d), f32(t0), f32(pivot)
        scores = None
        if want_scores:
            scores = np.zeros((2 * match.rot_steps + 1, 2 * match.shift_y + 1, 2 * match.shift_x + 1), np.uint32)
        best = np.zeros(8, np.uint32)
        status = np.zeros(1, np.uint32)
        ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.rplgpu_match_scans(
            self._h, scans.ctypes.data, n, lens.ctypes.data, S, C.byref(params), ptr(motion), ptr(pose2d), ptr(t0),
            ptr(pivot), C.byref(match), field.ctypes.data, ptr(scores), best.ctypes.data, status.ctypes.data))
        return scores, best, int(status[0])

    def map_update_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int, params: Params,
                       d_motion: int, d_pose2d: int, grid: OccGrid, d_counts: int, d_status: int = 0):
        """E14: the rays of all B scans ADDED into the one count map at d_counts (uint32 misses, hits per cell)."""
        self._check(self._lib.rplgpu_map_update_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d, C.byref(grid),
            d_counts, d_status))

    def map_grid_dev(self, d_counts: int, width: int, height: int, rule: MapRule, d_prev: int, d_grid: int,
                     grid_stride: int, d_cells: int = 0):
        """E14: the count map through the cell rule into one int8 grid of E11's layout; d_cells: 4 words
        (-1, 0, 100, anything else)."""
        self._check(self._lib.rplgpu_map_grid_dev(
            self._h, d_counts, width, height, C.byref(rule), d_prev, d_grid, grid_stride, d_cells))

    def apply_match_dev(self, d_best: int, match: ScanMatch, d_pivot: int, d_pose2d_in: int, B: int, group: int,
                        flags: int, d_pose2d_out: int, d_pivot_out: int = 0):
        """E14: E13's result words at d_best composed in front of the poses (and pivots) of their groups."""
        self._check(self._lib.rplgpu_apply_match_dev(
            self._h, d_best, C.byref(match), d_pivot, d_pose2d_in, B, group, flags, d_pose2d_out, d_pivot_out))

    def map_update(self, scans: np.ndarray, lens, params: Params, grid: OccGrid, counts: np.ndarray, motion=None,
                   pose2d=None, t0=None):
        """E14, one call's scans, host buffers: scans (S, n) NODE_DTYPE added into ``counts`` ((height, width, 2)
        uint32, misses and hits, changed in place) -> status."""
        scans = np.ascontiguousarray(scans)
        if scans.dtype != NODE_DTYPE or scans.ndim != 2:
            raise TypeError("scans must be a 2-D array of abi.NODE_DTYPE")
        if (counts.dtype != np.uint32 or not counts.flags.c_contiguous
                or counts.shape != (grid.height, grid.width, 2)):
            raise TypeError("counts must be a C-contiguous (height, width, 2) uint32 array")
        S, n = scans.shape
        lens = np.ascontiguousarray(lens, np.uint32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        motion, pose2d, t0 = f32(motion), f32(pose2d), f32(t0)
        status = np.zeros(1, np.uint32)
        ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.rplgpu_map_update(
            self._h, scans.ctypes.data, n, lens.ctypes.data, S, C.byref(params), ptr(motion), ptr(pose2d), ptr(t0),
            C.byref(grid), counts.ctypes.data, status.ctypes.data))
        return int(status[0])

    def map_grid(self, counts: np.ndarray, rule: MapRule, prev=None):
        """E14, host buffers: counts (height, width, 2) uint32 -> ``(grid (height, width) int8,
        (cells -1, cells 0, cells 100, other cells))``."""
        counts = np.ascontiguousarray(counts, np.uint32)
        if counts.ndim != 3 or counts.shape[2] != 2:
            raise TypeError("counts must be a (height, width, 2) uint32 array")
        H, W = counts.shape[:2]
        prev = None if prev is None else np.ascontiguousarray(prev, np.int8)
        out = np.empty((H, W), np.int8)
        cells = np.zeros(4, np.uint32)
        self._check(self._lib.rplgpu_map_grid(
            self._h, counts.ctypes.data, W, H, C.byref(rule), 0 if prev is None else prev.ctypes.data,
            out.ctypes.data, cells.ctypes.data))
        return out, tuple(int(c) for c in cells)

    def score_poses_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int, params: Params,
                        d_motion: int, d_pose2d: int, spec: PoseScore, d_poses: int, P: int, pose_stride: int,
                        poses_per_group: int, d_field: int, field_stride: int, field_per_group: int, d_weights: int,
                        weight_stride: int, d_result: int, d_status: int = 0):
        """E15: per group of scans the weights (uint32, P words, weight_stride apart) of the P poses (c, s, tx, ty)
        at d_poses over the int8 field(s) at d_field, and eight result words at d_result + 8 g."""
        self._check(self._lib.rplgpu_score_poses_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d, C.byref(spec),
            d_poses, P, pose_stride, poses_per_group, d_field, field_stride, field_per_group, d_weights,
            weight_stride, d_result, d_status))

    def score_poses(self, scans: np.ndarray, lens, params: Params, spec: PoseScore, poses: np.ndarray,
                    field: np.ndarray, motion=None, pose2d=None, t0=None, want_weights: bool = True):
        """E15, one group, host buffers: scans (S, n) NODE_DTYPE, poses (P, 4) float32 as ``pose_list`` makes them
        and a (height, width) int8 field -> ``(weights (P,) uint32 or None, result (8,) uint32, status)``."""
        scans = np.ascontiguousarray(scans)
        if scans.dtype != NODE_DTYPE or scans.ndim != 2:
            raise TypeError("scans must be a 2-D array of abi.NODE_DTYPE")
        field = np.ascontiguousarray(field, np.int8)
        if field.shape != (spec.height, spec.width):
            raise TypeError("field must be a (height, width) int8 array")
        poses = np.ascontiguousarray(poses, np.float32)
        if poses.ndim != 2 or poses.shape[1] != 4:
            raise TypeError("poses must be a (P, 4) float32 array")
        S, n = scans.shape
        P = len(poses)
        lens = np.ascontiguousarray(lens, np.uint32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        motion, pose2d, t0 = f32(motion), f32(pose2d), f32(t0)
        weights = np.zeros(P, np.uint32) if want_weights else None
        result = np.zeros(8, np.uint32)
        status = np.zeros(1, np.uint32)
        ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.rplgpu_score_poses(
            self._h, scans.ctypes.data, n, lens.ctypes.data, S, C.byref(params), ptr(motion), ptr(pose2d), ptr(t0),
            C.byref(spec), poses.ctypes.data, P, field.ctypes.data, ptr(weights), result.ctypes.data,
            status.ctypes.data))
        return weights, result, int(status[0])

    def score_poses_agree_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int,
                              params: Params, d_motion: int, d_pose2d: int, spec: "BeamAgree", d_poses: int, P: int,
                              pose_stride: int, poses_per_group: int, d_field: int, field_stride: int,
                              field_per_group: int, d_weights: int, weight_stride: int, d_result: int, d_status: int,
                              d_counts: int, count_stride: int, d_mask: int, mask_stride: int, d_agree: int):
        """E23: ``score_poses_dev`` without the samples the pose list disagrees with (AMCL's beam skip): besides the
        weights and result words, per scan the counts (uint32, n_stride words, count_stride apart) and the keep mask
        (ceil(n_stride / 32) words, mask_stride apart), and eight agree words at d_agree + 8 g."""
        self._check(self._lib.rplgpu_score_poses_agree_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d, C.byref(spec),
            d_poses, P, pose_stride, poses_per_group, d_field, field_stride, field_per_group, d_weights,
            weight_stride, d_result, d_status, d_counts, count_stride, d_mask, mask_stride, d_agree))

    def score_poses_agree(self, scans: np.ndarray, lens, params: Params, spec: "BeamAgree", poses: np.ndarray,
                          field: np.ndarray, motion=None, pose2d=None, t0=None):
        """E23, one group, host buffers, arguments as ``score_poses`` -> ``(weights (P,) uint32, result (8,) uint32,
        status, counts (S, n) uint32, mask (S, ceil(n / 32)) uint32, agree (8,) uint32)``."""
        scans = np.ascontiguousarray(scans)
        if scans.dtype != NODE_DTYPE or scans.ndim != 2:
            raise TypeError("scans must be a 2-D array of abi.NODE_DTYPE")
        field = np.ascontiguousarray(field, np.int8)
        if field.shape != (spec.height, spec.width):
            raise TypeError("field must be a (height, width) int8 array")
        poses = np.ascontiguousarray(poses, np.float32)
        if poses.ndim != 2 or poses.shape[1] != 4:
            raise TypeError("poses must be a (P, 4) float32 array")
        S, n = scans.shape
        P = len(poses)
        lens = np.ascontiguousarray(lens, np.uint32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        motion, pose2d, t0 = f32(motion), f32(pose2d), f32(t0)
        weights = np.zeros(P, np.uint32)
        result = np.zeros(8, np.uint32)
        status = np.zeros(1, np.uint32)
        counts = np.zeros((S, n), np.uint32)
        mask = np.zeros((S, (n + 31) // 32), np.uint32)
        agree = np.zeros(8, np.uint32)
        ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.rplgpu_score_poses_agree(
            self._h, scans.ctypes.data, n, lens.ctypes.data, S, C.byref(params), ptr(motion), ptr(pose2d), ptr(t0),
            C.byref(spec), poses.ctypes.data, P, field.ctypes.data, weights.ctypes.data, result.ctypes.data,
            status.ctypes.data, counts.ctypes.data, mask.ctypes.data, agree.ctypes.data))
        return weights, result, int(status[0]), counts, mask, agree

    def pool_field_dev(self, match: "WideMatch", d_field: int, field_stride: int, F: int, d_pooled: int,
                       pooled_stride: int):
        """E24: the pooled field P (the 8 x 8 sliding maximum of max(byte, 0), (height + 7) x (width + 7) int8) of
        each of the F fields at d_field, at d_pooled + f * pooled_stride."""
        self._check(self._lib.rplgpu_pool_field_dev(
            self._h, C.byref(match), d_field, field_stride, F, d_pooled, pooled_stride))

    def match_wide_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int, params: Params,
                       d_motion: int, d_pose2d: int, d_pivot: int, match: "WideMatch", d_field: int,
                       field_stride: int, field_per_group: int, d_pooled: int, pooled_stride: int, d_bounds: int,
                       bounds_stride: int, d_scratch: int, d_best: int, d_work: int, d_status: int = 0):
        """E24: per group of scans E13's best over a window of up to 256 cells a side, by bound and refine: the
        bounds volume (uint32, ``wide_match_blocks`` words, bounds_stride apart), eight result words at d_best + 8 g
        and eight work words at d_work + 8 g.  d_scratch: ``wide_match_scratch_words(match, G)`` uint32 words."""
        self._check(self._lib.rplgpu_match_wide_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d, d_pivot,
            C.byref(match), d_field, field_stride, field_per_group, d_pooled, pooled_stride, d_bounds, bounds_stride,
            d_scratch, d_best, d_work, d_status))

    def match_wide(self, scans: np.ndarray, lens, params: Params, match: "WideMatch", field: np.ndarray,
                   motion=None, pose2d=None, t0=None, pivot=None, want_bounds: bool = True):
        """E24, one group, host buffers: scans (S, n) NODE_DTYPE and a (height, width) int8 field ->
        ``(bounds (2K+1, nby, nbx) uint32 or None, best (8,) uint32, work (8,) uint32, status)``."""
        scans = np.ascontiguousarray(scans)
        if scans.dtype != NODE_DTYPE or scans.ndim != 2:
            raise TypeError("scans must be a 2-D array of abi.NODE_DTYPE")
        field = np.ascontiguousarray(field, np.int8)
        if field.shape != (match.height, match.width):
            raise TypeError("field must be a (height, width) int8 array")
        S, n = scans.shape
        lens = np.ascontiguousarray(lens, np.uint32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        motion, pose2d, t0, pivot = f32(motion), f32(pose2d), f32(t0), f32(pivot)
        bounds = None
        if want_bounds:
            s = WIDE_MATCH_BLOCK
            bounds = np.zeros((2 * match.rot_steps + 1, (2 * match.shift_y + s) // s, (2 * match.shift_x + s) // s),
                              np.uint32)
        best = np.zeros(8, np.uint32)
        work = np.zeros(8, np.uint32)
        status = np.zeros(1, np.uint32)
        ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.rplgpu_match_wide(
            self._h, scans.ctypes.data, n, lens.ctypes.data, S, C.byref(params), ptr(motion), ptr(pose2d), ptr(t0),
            ptr(pivot), C.byref(match), field.ctypes.data, ptr(bounds), best.ctypes.data, work.ctypes.data,
            status.ctypes.data))
        return bounds, best, work, int(status[0])

    def refine_sums_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int, params: Params,
                        d_motion: int, d_pose2d: int, spec: "PoseRefine", d_poses: int, P: int, pose_stride: int,
                        poses_per_group: int, d_field: int, field_stride: int, field_per_group: int, d_sums: int,
                        sums_stride: int, d_scratch: int, d_result: int, d_status: int = 0):
        """E25: per group of scans and pose of the list the 32 words of the Gauss-Newton sums against the bilinear
        field at d_sums + g * sums_stride + 32 q, eight result words at d_result + 8 g.  d_scratch:
        ``refine_scratch_words(G, P)`` uint32 words."""
        self._check(self._lib.rplgpu_refine_sums_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d, C.byref(spec),
            d_poses, P, pose_stride, poses_per_group, d_field, field_stride, field_per_group, d_sums, sums_stride,
            d_scratch, d_result, d_status))

    def refine_step_dev(self, d_sums: int, sums_stride: int, spec: "PoseRefine", d_poses: int, pose_stride: int,
                        poses_per_group: int, G: int, P: int, d_poses_out: int, out_stride: int, d_step: int,
                        step_stride: int, d_result: int):
        """E25: one Gauss-Newton step of every pose from its sums: the stepped list at d_poses_out, the step words
        (optional) at d_step, result words 0 - 3 at d_result + 8 g."""
        self._check(self._lib.rplgpu_refine_step_dev(
            self._h, d_sums, sums_stride, C.byref(spec), d_poses, pose_stride, poses_per_group, G, P, d_poses_out,
            out_stride, d_step, step_stride, d_result))

    def refine_poses_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int, params: Params,
                         d_motion: int, d_pose2d: int, spec: "PoseRefine", d_poses: int, P: int, pose_stride: int,
                         poses_per_group: int, d_field: int, field_stride: int, field_per_group: int, iters: int,
                         d_poses_out: int, out_stride: int, d_sums: int, sums_stride: int, d_step: int,
                         step_stride: int, d_scratch: int, d_result: int, d_status: int = 0):
        """E25: ``iters`` rounds of sums + step queued on the stream; the final list at d_poses_out, the last
        round's sums, step words and result words."""
        self._check(self._lib.rplgpu_refine_poses_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d, C.byref(spec),
            d_poses, P, pose_stride, poses_per_group, d_field, field_stride, field_per_group, iters, d_poses_out,
            out_stride, d_sums, sums_stride, d_step, step_stride, d_scratch, d_result, d_status))

    def refine_poses(self, scans: np.ndarray, lens, params: Params, spec: "PoseRefine", poses: np.ndarray,
                     field: np.ndarray, iters: int = 1, motion=None, pose2d=None, t0=None):
        """E25, one group, host buffers: scans (S, n) NODE_DTYPE, poses (P, 4) float32 and a (height, width) int8
        field -> ``(poses_out (P, 4) float32, sums (P, 32) uint32, step (P, 4) uint32, result (8,) uint32,
        status)``."""
        scans = np.ascontiguousarray(scans)
        if scans.dtype != NODE_DTYPE or scans.ndim != 2:
            raise TypeError("scans must be a 2-D array of abi.NODE_DTYPE")
        field = np.ascontiguousarray(field, np.int8)
        if field.shape != (spec.height, spec.width):
            raise TypeError("field must be a (height, width) int8 array")
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 4)
        S, n = scans.shape
        P = len(poses)
        lens = np.ascontiguousarray(lens, np.uint32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        motion, pose2d, t0 = f32(motion), f32(pose2d), f32(t0)
        out = np.zeros((P, 4), np.float32)
        sums = np.zeros((P, REFINE_WORDS), np.uint32)
        step = np.zeros((P, 4), np.uint32)
        result = np.zeros(8, np.uint32)
        status = np.zeros(1, np.uint32)
        ptr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.rplgpu_refine_poses(
            self._h, scans.ctypes.data, n, lens.ctypes.data, S, C.byref(params), ptr(motion), ptr(pose2d), ptr(t0),
            C.byref(spec), poses.ctypes.data, P, field.ctypes.data, iters, out.ctypes.data, sums.ctypes.data,
            step.ctypes.data, result.ctypes.data, status.ctypes.data))
        return out, sums, step, result, int(status[0])

    def match_poses_dev(self, d_best: int, match: "ScanMatch", d_pivot: int, d_prior: int, G: int, d_poses_out: int,
                        out_stride: int):
        """E25's joint to E13 / E24: the eight result words of every group applied to its base prior (0: the
        identity at the pivot), one pose (c, s, x, y) per group at d_poses_out + g * out_stride."""
        self._check(self._lib.rplgpu_match_poses_dev(
            self._h, d_best, C.byref(match), d_pivot, d_prior, G, d_poses_out, out_stride))

    def compose_poses_dev(self, d_poses: int, pose_stride: int, poses_per_group: int, P: int, d_result: int, q: int,
                          d_pose2d_in: int, B: int, group: int, d_pose2d_out: int):
        """E25's joint to E11 / E14: pose q (d_result 0) or word 4 of d_result + 8 g of every group's list composed
        in front of the group's mount poses, six floats per scan at d_pose2d_out."""
        self._check(self._lib.rplgpu_compose_poses_dev(
            self._h, d_poses, pose_stride, poses_per_group, P, d_result, q, d_pose2d_in, B, group, d_pose2d_out))

    def nav_field_dev(self, spec: "NavField", d_grid: int, grid_stride: int, G: int, d_goals: int, goal_stride: int,
                      d_n_goals: int, d_potential: int, potential_stride: int, d_scratch: int, resume: int,
                      d_result: int):
        """E26: the cost-to-goal field of G costmaps, ``spec.rounds`` rounds queued on the stream; eight result words
        at d_result + 8 g (word 0: the dirty tiles left, 0 = finished).  d_scratch: ``nav_field_scratch_words(spec,
        G)`` uint32 words, which a call with ``resume`` = 1 continues from."""
        self._check(self._lib.rplgpu_nav_field_dev(
            self._h, C.byref(spec), d_grid, grid_stride, G, d_goals, goal_stride, d_n_goals, d_potential,
            potential_stride, d_scratch, resume, d_result))

    def nav_paths_dev(self, spec: "NavField", d_grid: int, grid_stride: int, d_potential: int, potential_stride: int,
                      G: int, d_starts: int, S: int, d_paths: int, max_len: int, d_info: int):
        """E26: S paths per grid down the field, path s of grid g at d_paths + (g S + s) max_len, four info words
        at d_info + 4 (g S + s)."""
        self._check(self._lib.rplgpu_nav_paths_dev(
            self._h, C.byref(spec), d_grid, grid_stride, d_potential, potential_stride, G, d_starts, S, d_paths,
            max_len, d_info))

    def nav_field(self, spec: "NavField", grid: np.ndarray, goals, starts=None, max_len: int = 0, path_fill: int = 0):
        """E26, one grid, host buffers: a (height, width) int8 costmap and goal cell indices -> ``(potential
        (height, width) uint32, result (8,) uint32)``, with ``starts`` also ``paths (S, max_len) uint32`` (words
        beyond a path keep ``path_fill``) and ``info (S, 4) uint32``."""
        grid = np.ascontiguousarray(grid, np.int8)
        if grid.shape != (spec.height, spec.width):
            raise TypeError("grid must be a (height, width) int8 array")
        goals = np.ascontiguousarray(goals, np.uint32).reshape(-1)
        pot = np.zeros((spec.height, spec.width), np.uint32)
        result = np.zeros(8, np.uint32)
        if starts is None:
            self._check(self._lib.rplgpu_nav_field(
                self._h, C.byref(spec), grid.ctypes.data, goals.ctypes.data if len(goals) else 0, len(goals),
                pot.ctypes.data, result.ctypes.data, 0, 0, 0, 0, 0))
            return pot, result
        starts = np.ascontiguousarray(starts, np.uint32).reshape(-1)
        paths = np.full((len(starts), max_len), path_fill, np.uint32)
        info = np.zeros((len(starts), 4), np.uint32)
        self._check(self._lib.rplgpu_nav_field(
            self._h, C.byref(spec), grid.ctypes.data, goals.ctypes.data if len(goals) else 0, len(goals),
            pot.ctypes.data, result.ctypes.data, starts.ctypes.data, len(starts), paths.ctypes.data, max_len,
            info.ctypes.data))
        return pot, result, paths, info

    def frontiers_dev(self, spec: "Frontiers", d_grid: int, grid_stride: int, d_potential: int, potential_stride: int,
                      G: int, comp_cap: int, d_labels_out: int, label_stride: int, d_rows: int, row_stride: int,
                      row_cap: int, d_goal_out: int, goal_stride: int, d_n_goal_out: int, d_result: int,
                      d_scratch: int):
        """E29: the frontier cells of G grids (d_potential 0: every free cell counts as reached) grouped into
        components, sixteen result words at d_result + 16 g; optional labels, rows of the kept components and BEST's
        cell in E26's goal layout.  d_scratch: ``frontiers_scratch_words(spec, G, comp_cap)`` uint32 words."""
        self._check(self._lib.rplgpu_frontiers_dev(
            self._h, C.byref(spec), d_grid, grid_stride, d_potential, potential_stride, G, comp_cap, d_labels_out,
            label_stride, d_rows, row_stride, row_cap, d_goal_out, goal_stride, d_n_goal_out, d_result, d_scratch))

    def frontiers(self, spec: "Frontiers", grid, potential=None, comp_cap: int = 4096, row_cap: int = 0,
                  labels: bool = True, row_fill: int = 0, goal_fill: int = 0) -> dict:
        """E29, one grid, host buffers -> the dictionary of ``frontiers_host``."""
        a = _frontier_args(spec, grid, potential, comp_cap, row_cap, labels, row_fill, goal_fill)
        self._check(self._lib.rplgpu_frontiers(self._h, *a[0]))
        return a[1]

    def rollout_dev(self, spec: "Rollout", d_start: int, start_per_group: int, d_delta: int, delta_stride: int,
                    delta_per_group: int, delta_per_step: int, d_footprint: int, F: int, d_grid: int,
                    grid_stride: int, d_potential: int, potential_stride: int, grid_per_group: int, G: int, K: int,
                    d_out: int, out_stride: int, d_end_poses: int, end_stride: int, d_result: int, d_scratch: int):
        """E27: K candidates per group rolled ``spec.steps`` steps out of the group's start pose by their deltas (one
        each, or one per step with ``delta_per_step``), the F footprint points looked up in the costmap at d_grid and
        the centre in E26's field at d_potential (0: none); eight words per candidate at d_out + g out_stride + 8 k,
        the end poses (optional) and eight result words at d_result + 8 g.  d_scratch:
        ``rollout_scratch_words(G, K)`` uint32 words."""
        self._check(self._lib.rplgpu_rollout_dev(
            self._h, C.byref(spec), d_start, start_per_group, d_delta, delta_stride, delta_per_group, delta_per_step,
            d_footprint, F, d_grid, grid_stride, d_potential, potential_stride, grid_per_group, G, K, d_out,
            out_stride, d_end_poses, end_stride, d_result, d_scratch))

    def rollout(self, spec: "Rollout", start, delta, footprint, grid, potential=None):
        """E27, one group, host buffers: start (4,) float32, delta (K, 4) or (K, steps, 4) float32, footprint (F, 2)
        float32, a (height, width) int8 costmap and optionally E26's field of the same shape -> ``(out (K, 8) uint32,
        end_poses (K, 4) float32, result (8,) uint32)``."""
        a = _rollout_args(spec, start, delta, footprint, grid, potential)
        self._check(self._lib.rplgpu_rollout(self._h, C.byref(spec), *a[0]))
        return a[1]

    def mppi_update_dev(self, spec: "Mppi", d_out: int, out_stride: int, d_rollout_result: int, d_delta: int,
                        delta_stride: int, delta_per_group: int, d_table: int, d_nominal: int, nominal_stride: int,
                        nominal_per_group: int, G: int, K: int, d_weights: int, weight_stride: int, d_sums: int,
                        sums_stride: int, d_nominal_out: int, nominal_out_stride: int, d_result: int, d_scratch: int):
        """E28 A: per group the K candidates E27 scored (d_out, d_rollout_result) weighed through the uint16 table at
        d_table, the deltas E27 rolled summed per step under those weights (eight words a step at d_sums) and blended
        into ``spec.steps_e`` new deltas at d_nominal_out; the weights at d_weights (E15's layout), eight result words
        at d_result + 8 g.  d_scratch: ``mppi_scratch_words(G, K, spec.steps_e)`` uint32 words."""
        self._check(self._lib.rplgpu_mppi_update_dev(
            self._h, C.byref(spec), d_out, out_stride, d_rollout_result, d_delta, delta_stride, delta_per_group,
            d_table, d_nominal, nominal_stride, nominal_per_group, G, K, d_weights, weight_stride, d_sums, sums_stride,
            d_nominal_out, nominal_out_stride, d_result, d_scratch))

    def mppi_update(self, spec: "Mppi", out, rollout_result, delta, table, nominal=None):
        """E28 A, one group, host buffers: out (K, 8) uint32 and rollout_result (8,) uint32 from E27, delta (K, 4) or
        (K, steps, 4) float32, table (N,) uint16, nominal None or (steps_e, 4) float32 -> ``(weights (K,) uint32, sums
        (steps_e, 8) uint32, nominal_out (steps_e, 4) float32, result (8,) uint32)``."""
        a = _mppi_update_args(spec, out, rollout_result, delta, table, nominal)
        self._check(self._lib.rplgpu_mppi_update(self._h, C.byref(spec), *a[0]))
        return a[1]

    def mppi_spread_dev(self, d_nominal: int, nominal_stride: int, nominal_per_group: int, T_n: int, d_noise: int,
                        noise_stride: int, noise_per_group: int, G: int, K: int, T: int, shift: int, keep_first: int,
                        d_out: int, out_stride: int):
        """E28 B: per group out[k][t] = nominal[min(t + shift, T_n - 1)] composed with noise[k][t] (E16's move), the
        per-step deltas ``rollout_dev`` reads; candidate 0 is the nominal itself with keep_first."""
        self._check(self._lib.rplgpu_mppi_spread_dev(
            self._h, d_nominal, nominal_stride, nominal_per_group, T_n, d_noise, noise_stride, noise_per_group, G, K,
            T, shift, keep_first, d_out, out_stride))

    def mppi_spread(self, nominal, noise, shift: int = 0, keep_first: int = 0) -> np.ndarray:
        """E28 B, one group, host buffers: nominal (T_n, 4) and noise (K, T, 4) float32 -> (K, T, 4) float32."""
        a = _mppi_spread_args(nominal, noise, shift, keep_first)
        self._check(self._lib.rplgpu_mppi_spread(self._h, *a[0]))
        return a[1]

    def resample_poses_dev(self, d_weights: int, weight_stride: int, d_poses: int, pose_stride: int,
                           poses_per_group: int, G: int, P: int, M: int, d_u: int, d_delta: int, n_delta: int,
                           delta_stride: int, delta_per_group: int, d_poses_out: int, out_stride: int,
                           d_ancestors: int, anc_stride: int, d_result: int, d_scratch: int):
        """E16: per group the P weighted poses at d_poses resampled (systematic, the group's random word at d_u) into
        M poses at d_poses_out, moved by the delta(s) at d_delta when that is not 0; ancestors (optional) and eight
        result words at d_result + 8 g.  d_scratch: ``resample_scratch_words(G, P)`` uint32 words."""
        self._check(self._lib.rplgpu_resample_poses_dev(
            self._h, d_weights, weight_stride, d_poses, pose_stride, poses_per_group, G, P, M, d_u, d_delta, n_delta,
            delta_stride, delta_per_group, d_poses_out, out_stride, d_ancestors, anc_stride, d_result, d_scratch))

    def resample_poses(self, weights: np.ndarray, poses: np.ndarray, M: int, u: int = 0, delta=None):
        """E16, one group, host buffers: weights (P,) uint32 and poses (P, 4) float32 -> ``(poses_out (M, 4)
        float32, ancestors (M,) uint32, result (8,) uint32)``; delta: None, (4,) / (1, 4) or (M, 4) float32."""
        weights, poses, delta, n_delta = _resample_args(weights, poses, M, delta)
        out = np.zeros((M, 4), np.float32)
        anc = np.zeros(M, np.uint32)
        result = np.zeros(8, np.uint32)
        self._check(self._lib.rplgpu_resample_poses(
            self._h, weights.ctypes.data, len(weights), M, u, poses.ctypes.data,
            0 if delta is None else delta.ctypes.data, n_delta, out.ctypes.data, anc.ctypes.data,
            result.ctypes.data))
        return out, anc, result

    def estimate_poses_dev(self, d_poses: int, pose_stride: int, poses_per_group: int, d_weights: int,
                           weight_stride: int, G: int, P: int, spec: "PoseEstimate", d_center: int,
                           center_stride: int, d_result: int, d_scratch: int):
        """E17: per group the P poses at d_poses, weighed by d_weights (0: every weight 1), reduced to the
        ``ESTIMATE_WORDS`` result words at d_result + 72 g: two sets of eight 128-bit sums (every in-range pose; the
        gate around pose min(d_center[g * center_stride], P - 1), pose 0 when d_center is 0), counts and flags.
        d_scratch: ``estimate_scratch_words(G, P)`` uint32 words."""
        self._check(self._lib.rplgpu_estimate_poses_dev(
            self._h, d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P, C.byref(spec), d_center,
            center_stride, d_result, d_scratch))

    def estimate_poses(self, poses: np.ndarray, weights=None, spec: "PoseEstimate" = None, center: int = 0):
        """E17, one group, host buffers: poses (P, 4) float32 and weights (P,) uint32 or None (every weight 1) ->
        result (72,) uint32."""
        poses, weights, spec = _estimate_args(poses, weights, spec)
        result = np.zeros(ESTIMATE_WORDS, np.uint32)
        self._check(self._lib.rplgpu_estimate_poses(
            self._h, poses.ctypes.data, len(poses), 0 if weights is None else weights.ctypes.data, C.byref(spec),
            center, result.ctypes.data))
        return result

    def sample_motion_dev(self, d_odom: int, odom_per_group: int, G: int, M: int, spec: "MotionNoise", d_delta: int,
                          delta_stride: int, d_result: int):
        """E18: per group M deltas (E16's ``n_delta = M`` layout) at d_delta + g * delta_stride, drawn from the
        group's eight odometry floats at d_odom + 8 g (group 0's for every group when odom_per_group is 0) by
        Philox4x32-10 under ``spec``; eight result words at d_result + 8 g."""
        self._check(self._lib.rplgpu_sample_motion_dev(
            self._h, d_odom, odom_per_group, G, M, C.byref(spec), d_delta, delta_stride, d_result))

    def sample_motion(self, odom: np.ndarray, M: int, spec: "MotionNoise" = None):
        """E18, one group (group 0), host buffers: odom (8,) float32 -> ``(delta (M, 4) float32, result (8,)
        uint32)``."""
        odom, spec = _motion_args(odom, spec)
        delta = np.zeros((M, 4), np.float32)
        result = np.zeros(8, np.uint32)
        self._check(self._lib.rplgpu_sample_motion(
            self._h, odom.ctypes.data, M, C.byref(spec), delta.ctypes.data, result.ctypes.data))
        return delta, result

    def seed_poses_dev(self, spec: "PoseSeed", d_grid: int, grid_stride: int, grid_per_group: int, d_headings: int,
                       H: int, G: int, M: int, noise: "MotionNoise", d_poses_out: int, out_stride: int,
                       d_cells_out: int, cell_stride: int, d_result: int, d_scratch: int):
        """E19: per group M poses (E15 / E16's layout) at d_poses_out + g * out_stride, drawn uniformly over the free
        cells of the group's grid at d_grid + g * grid_stride (group 0's for every group when grid_per_group is 0),
        headings from the H-entry table, by Philox4x32-10 under ``noise`` (draw index 3); the chosen cell indices at
        d_cells_out (optional), eight result words at d_result + 8 g.  d_scratch: ``seed_scratch_words(G_f, width,
        height)`` uint32 words."""
        self._check(self._lib.rplgpu_seed_poses_dev(
            self._h, C.byref(spec), d_grid, grid_stride, grid_per_group, d_headings, H, G, M, C.byref(noise),
            d_poses_out, out_stride, d_cells_out, cell_stride, d_result, d_scratch))

    def seed_poses(self, grid: np.ndarray, headings: np.ndarray, M: int, spec: "PoseSeed" = None,
                   noise: "MotionNoise" = None):
        """E19, one group (group 0), host buffers: grid (height, width) int8, headings (H, 2) float32 -> ``(poses
        (M, 4) float32, cells (M,) uint32, result (8,) uint32)``."""
        grid, headings, spec, noise = _seed_args(grid, headings, spec, noise)
        poses = np.zeros((M, 4), np.float32)
        cells = np.zeros(M, np.uint32)
        result = np.zeros(8, np.uint32)
        self._check(self._lib.rplgpu_seed_poses(
            self._h, C.byref(spec), grid.ctypes.data, headings.ctypes.data, len(headings), M, C.byref(noise),
            poses.ctypes.data, cells.ctypes.data, result.ctypes.data))
        return poses, cells, result

    def bin_poses_dev(self, spec: "PoseBins", d_poses: int, pose_stride: int, poses_per_group: int, d_weights: int,
                      weight_stride: int, G: int, P: int, d_edges: int, T: int, d_map: int, map_stride: int,
                      d_bins_out: int, bin_stride: int, d_result: int):
        """E20: per group the P poses at d_poses (E15 / E16 / E17's layout) binned in (x, y, heading) under ``spec``
        and the T-entry edge table, marked in the group's bit map at d_map + g * map_stride (words); the bin ids at
        d_bins_out (optional), eight result words at d_result + 8 g.  A pose whose weight is 0 is skipped
        (d_weights 0: every pose counts)."""
        self._check(self._lib.rplgpu_bin_poses_dev(
            self._h, C.byref(spec), d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P, d_edges, T,
            d_map, map_stride, d_bins_out, bin_stride, d_result))

    def bin_poses(self, poses: np.ndarray, edges: np.ndarray, weights: np.ndarray = None, spec: "PoseBins" = None,
                  map_in: np.ndarray = None):
        """E20, one group, host buffers: poses (P, 4) float32, edges (T, 2) float32, weights (P,) uint32 or None ->
        ``(map (ceil(NB / 32),) uint32, bins (P,) uint32, result (8,) uint32)``; ``map_in`` is the map KEEP ORs into."""
        poses, edges, weights, spec, bmap = _bins_args(poses, edges, weights, spec, map_in)
        bins = np.zeros(len(poses), np.uint32)
        result = np.zeros(8, np.uint32)
        self._check(self._lib.rplgpu_bin_poses(
            self._h, C.byref(spec), poses.ctypes.data, len(poses), weights.ctypes.data if weights is not None else None,
            edges.ctypes.data, len(edges), bmap.ctypes.data, bins.ctypes.data, result.ctypes.data))
        return bmap, bins, result

    def cluster_poses_dev(self, spec: "PoseClusters", d_poses: int, pose_stride: int, poses_per_group: int,
                          d_weights: int, weight_stride: int, G: int, P: int, T: int, d_map: int, map_stride: int,
                          d_bins: int, bin_stride: int, d_labels_out: int, label_stride: int, d_clusters: int,
                          cluster_stride: int, cluster_cap: int, d_result: int, d_scratch: int):
        """E21: per group the occupied bins of E20's bit map at d_map labelled by connected component, the P poses
        (bin ids at d_bins, E20's ``d_bins_out``) given their cluster's label (d_labels_out, optional), the clusters
        weighed (4-word rows at d_clusters, optional) and the heaviest reduced to E17's sums: 80 result words at
        d_result + 80 g.  d_scratch: ``cluster_scratch_words(G, P, nx, ny, T)`` uint32 words."""
        self._check(self._lib.rplgpu_cluster_poses_dev(
            self._h, C.byref(spec), d_poses, pose_stride, poses_per_group, d_weights, weight_stride, G, P, T, d_map,
            map_stride, d_bins, bin_stride, d_labels_out, label_stride, d_clusters, cluster_stride, cluster_cap,
            d_result, d_scratch))

    def cluster_poses(self, poses: np.ndarray, bmap: np.ndarray, bins: np.ndarray, T: int, weights: np.ndarray = None,
                      spec: "PoseClusters" = None, cluster_cap: int = 0, clusters_in: np.ndarray = None):
        """E21, one group, host buffers: poses (P, 4) float32, the map (ceil(NB / 32),) uint32, bins (P,) uint32,
        weights (P,) uint32 or None -> ``(labels (P,) uint32, clusters (cluster_cap, 4) uint32, result (80,)
        uint32)``; ``clusters_in`` is what the rows beyond N_c keep."""
        poses, bmap, bins, weights, spec, table = _cluster_args(poses, bmap, bins, T, weights, spec, cluster_cap,
                                                                clusters_in)
        labels = np.zeros(len(poses), np.uint32)
        result = np.zeros(CLUSTER_WORDS, np.uint32)
        self._check(self._lib.rplgpu_cluster_poses(
            self._h, C.byref(spec), poses.ctypes.data, len(poses), weights.ctypes.data if weights is not None else None,
            T, bmap.ctypes.data, bins.ctypes.data, labels.ctypes.data, table.ctypes.data if cluster_cap else None,
            cluster_cap, result.ctypes.data))
        return labels, table, result

    def cast_ranges_dev(self, spec: "RangeCast", d_poses: int, pose_stride: int, poses_per_group: int, G: int, P: int,
                        d_beams: int, A: int, d_grid: int, grid_stride: int, grid_per_group: int, d_measured: int,
                        meas_stride: int, meas_first: int, meas_step: int, d_table: int, d_ranges_out: int,
                        range_stride: int, d_weights: int, weight_stride: int, d_result: int, d_cast: int):
        """E22: per group a ray from each of the P poses at d_poses (E15 / E16 / E19's layout) along each of the A
        beams (cb, sb) at d_beams through the int8 grid at d_grid + g * grid_stride by E11's walk; the range words
        ``D2 | kind << 28`` at d_ranges_out + g * range_stride + q * A + a (optional), eight cast counts at d_cast +
        8 g.  With d_measured (the merged scan's ranges, beam a at meas_first + a * meas_step) every ray is compared
        through the 2K + 2 bytes at d_table and summed into E15's weights at d_weights and result words at d_result."""
        self._check(self._lib.rplgpu_cast_ranges_dev(
            self._h, C.byref(spec), d_poses, pose_stride, poses_per_group, G, P, d_beams, A, d_grid, grid_stride,
            grid_per_group, d_measured, meas_stride, meas_first, meas_step, d_table, d_ranges_out, range_stride,
            d_weights, weight_stride, d_result, d_cast))

    def cast_ranges(self, poses: np.ndarray, beams: np.ndarray, grid: np.ndarray, spec: "RangeCast" = None,
                    measured: np.ndarray = None, table: np.ndarray = None, meas_first: int = 0, meas_step: int = 1,
                    want_ranges: bool = True):
        """E22, one group, host buffers: poses (P, 4) float32, beams (A, 2) float32, grid (height, width) int8,
        measured (n,) float32 and table (2K + 2,) uint8 or both None -> ``(ranges (P, A) uint32 or None, weights (P,)
        uint32 or None, result (8,) uint32 or None, cast (8,) uint32)``."""
        poses, beams, grid, spec, measured, table = _cast_args(poses, beams, grid, spec, measured, table)
        P, A = len(poses), len(beams)
        ranges = np.zeros((P, A), np.uint32) if want_ranges else None
        weights = np.zeros(P, np.uint32) if measured is not None else None
        result = np.zeros(8, np.uint32) if measured is not None else None
        cast = np.zeros(8, np.uint32)
        self._check(self._lib.rplgpu_cast_ranges(
            self._h, C.byref(spec), poses.ctypes.data, P, beams.ctypes.data, A, grid.ctypes.data,
            measured.ctypes.data if measured is not None else None, len(measured) if measured is not None else 0,
            meas_first, meas_step, table.ctypes.data if table is not None else None,
            ranges.ctypes.data if want_ranges else None, weights.ctypes.data if weights is not None else None,
            result.ctypes.data if result is not None else None, cast.ctypes.data))
        return ranges, weights, result, cast

    def filter_laserscan_batch_dev(self, d_ranges: int, d_intens: int, n_stride: int, d_beam_count: int,
                                   B: int, params: Params, flt: ScanFilter, d_ranges_out: int,
                                   d_intens_out: int, d_removed: int = 0):
        """E10: the LaserScans of a batch through the scan-shadow and speckle filters (same layout out);
        d_removed: 2 words per scan (by shadow, by speckle in addition)."""
        self._check(self._lib.rplgpu_filter_laserscan_batch_dev(
            self._h, d_ranges, d_intens, n_stride, d_beam_count, B, C.byref(params), C.byref(flt),
            d_ranges_out, d_intens_out, d_removed))

    def filter_merged_scans_dev(self, d_ranges: int, d_intens: int, G: int, merge: ScanMerge,
                                flt: ScanFilter, d_ranges_out: int, d_intens_out: int, d_removed: int = 0):
        """E10 on the G merged scans rplgpu_merge_scans_dev wrote."""
        self._check(self._lib.rplgpu_filter_merged_scans_dev(
            self._h, d_ranges, d_intens, G, C.byref(merge), C.byref(flt), d_ranges_out, d_intens_out,
            d_removed))

    def filter_laserscan(self, ranges: np.ndarray, intens: np.ndarray, angle_increment: float,
                         flt: ScanFilter):
        """E10, one scan, host buffers: ``(ranges_out, intensities_out, (by shadow, by speckle))``."""
        ranges = np.ascontiguousarray(ranges, np.float32)
        intens = np.ascontiguousarray(intens, np.float32)
        count = len(ranges)
        r_out = np.empty(max(count, 1), np.float32)
        i_out = np.empty(max(count, 1), np.float32)
        removed = np.zeros(2, np.uint32)
        self._check(self._lib.rplgpu_filter_laserscan(
            self._h, ranges.ctypes.data, intens.ctypes.data, count, angle_increment, C.byref(flt),
            r_out.ctypes.data, i_out.ctypes.data, removed.ctypes.data))
        return r_out[:count], i_out[:count], (int(removed[0]), int(removed[1]))

    def cloud_fused_cells_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, group: int,
                              params: Params, d_motion: int, d_pose2d: int, d_cells: int,
                              cells_capacity: int, d_cursor: int, d_group_start: int, d_n_cells: int,
                              d_status: int = 0):
        """cloud_fused_voxel_dev writing one CELL_DTYPE record per occupied cell (key order) per group."""
        self._check(self._lib.rplgpu_cloud_fused_cells_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, group, C.byref(params), d_motion, d_pose2d,
            d_cells, cells_capacity, d_cursor, d_group_start, d_n_cells, d_status))

    def set_voxel_aggregation(self, mode: int = 0):
        """0 = auto (from the previous batch launch's statistics), 1 = plain, 2 = two-class
        (include/rplgpu.h RPLGPU_VOXEL_AGG_*).  Results are identical in every mode."""
        self._check(self._lib.rplgpu_set_voxel_aggregation(self._h, int(mode)))

    def set_ror_mode(self, mode: int = 0):
        """0 = E5 inside the voxel kernel (arena entry points, one pass over the scans), 1 = two kernels
        (include/rplgpu.h RPLGPU_ROR_*).  Results are identical in both modes."""
        self._check(self._lib.rplgpu_set_ror_mode(self._h, int(mode)))

    def debug_ror_listed(self) -> int:
        """Work items the last E5-inside launch left to the two kernels (waits for the stream)."""
        n = C.c_uint32(0)
        self._lib.rplgpu_debug_ror_listed.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        self._check(self._lib.rplgpu_debug_ror_listed(self._h, C.byref(n)))
        return int(n.value)

    def set_scan_time_offsets_dev(self, d_t0: int = 0):
        """Per scan of the following de-skew / fused launches: the time [s] of its first sample relative
        to the fused instant (include/rplgpu_msg.h); 0 switches the offsets off."""
        self._check(self._lib.rplgpu_set_scan_time_offsets_dev(self._h, d_t0 or None))

    def set_cell_key_output(self, d_cell_keys: int = 0):
        """Optional voxel output: one u32 per output point, (iy + 32768) << 16 | (ix + 32768)."""
        self._check(self._lib.rplgpu_set_cell_key_output(self._h, d_cell_keys or None))

    # -- multi-GPU exchange (include/rplgpu_comm.h) ------------------------------------------
    @staticmethod
    def comm_unique_id() -> np.ndarray:
        """A fresh RCCL unique id (rank 0 makes it, the caller carries it to the other ranks)."""
        uid = np.zeros(128, np.uint8)
        rc = load_library().rplgpu_comm_unique_id(uid.ctypes.data)
        if rc:
            raise RplGpuError(rc, "rplgpu_comm_unique_id (is librccl.so loadable?)")
        return uid

    def comm_init(self, rank: int, world: int, uid: np.ndarray):
        uid = np.ascontiguousarray(uid, np.uint8)
        assert uid.nbytes == 128
        self._check(self._lib.rplgpu_comm_init(self._h, rank, world, uid.ctypes.data))

    def comm_size(self):
        """(ranks, this rank) of the handle's communicator as RCCL reports them; (0, -1) without one."""
        w, r = C.c_int32(0), C.c_int32(-1)
        self._check(self._lib.rplgpu_comm_size(self._h, C.byref(w), C.byref(r)))
        return int(w.value), int(r.value)

    def comm_destroy(self):
        self._check(self._lib.rplgpu_comm_destroy(self._h))

    def pack_cloud_meta_dev(self, d_cursor: int, d_scan_start: int, d_n_points: int, B: int,
                            slot_points: int, max_scans: int, d_meta: int):
        self._check(self._lib.rplgpu_pack_cloud_meta_dev(
            self._h, d_cursor, d_scan_start, d_n_points, B, slot_points, max_scans, d_meta))

    def allgather_clouds_dev(self, d_points_local: int, slot_points: int, d_meta_local: int,
                             meta_words: int, d_points_all: int, d_meta_all: int):
        self._check(self._lib.rplgpu_allgather_clouds_dev(
            self._h, d_points_local, slot_points, d_meta_local, meta_words, d_points_all, d_meta_all))

    def cloud_arena_xyi_dev(self, d_nodes: int, n_stride: int, d_n_per_scan: int, B: int, p: Params,
                            d_slot: int, slot_points: int, d_cursor: int, d_scan_start: int,
                            d_n_points: int, d_status: int = 0):
        """cloud_arena_dev writing 12-byte points (x, y, intensity) straight into an exchange slot."""
        self._check(self._lib.rplgpu_cloud_arena_xyi_dev(
            self._h, d_nodes, n_stride, d_n_per_scan, B, C.byref(p), d_slot, slot_points, d_cursor,
            d_scan_start, d_n_points, d_status))

    def pack_cloud_xyi_dev(self, d_arena: int, d_cursor: int, slot_points: int, d_slot: int):
        self._check(self._lib.rplgpu_pack_cloud_xyi_dev(self._h, d_arena, d_cursor, slot_points, d_slot))

    def gather_clouds_dev(self, root: int, d_points_local: int, slot_points: int, point_floats: int,
                          d_meta_local: int, meta_words: int, d_points_all: int = 0, d_meta_all: int = 0):
        """Gather to one rank (grouped ncclSend / ncclRecv): the all-gather's layout on `root` only."""
        self._check(self._lib.rplgpu_gather_clouds_dev(
            self._h, root, d_points_local, slot_points, point_floats, d_meta_local, meta_words,
            d_points_all, d_meta_all))

    def gather_cells_dev(self, root: int, d_cells_local: int, slot_cells: int, d_meta_local: int,
                         meta_words: int, d_cells_all: int = 0, d_meta_all: int = 0):
        """gather_clouds_dev for slots of 32-byte cell records."""
        self._check(self._lib.rplgpu_gather_cells_dev(
            self._h, root, d_cells_local, slot_cells, d_meta_local, meta_words, d_cells_all, d_meta_all))

    def merge_cells_dev(self, d_cells_all: int, slot_cells: int, d_meta_all: int, meta_words: int,
                        world: int, n_groups: int, params: Params, d_arena: int, arena_capacity: int,
                        d_cursor: int, d_group_start: int, d_n_points: int, d_status: int = 0):
        """Gathered cell slots -> one fused grid per group (the outputs of cloud_fused_voxel_dev)."""
        self._check(self._lib.rplgpu_merge_cells_dev(
            self._h, d_cells_all, slot_cells, d_meta_all, meta_words, world, n_groups, C.byref(params),
            d_arena, arena_capacity, d_cursor, d_group_start, d_n_points, d_status))

    def allgather_clouds_xyi_dev(self, d_slot_local: int, slot_points: int, d_meta_local: int,
                                 meta_words: int, d_slots_all: int, d_meta_all: int):
        self._check(self._lib.rplgpu_allgather_clouds_xyi_dev(
            self._h, d_slot_local, slot_points, d_meta_local, meta_words, d_slots_all, d_meta_all))

    def unpack_gathered_xyi_dev(self, d_slots_all: int, slot_points: int, d_meta_all: int,
                                meta_words: int, world: int, max_scans: int, d_packed: int,
                                d_total: int, d_scan_start_all: int, d_n_points_all: int,
                                d_status: int = 0):
        self._check(self._lib.rplgpu_unpack_gathered_xyi_dev(
            self._h, d_slots_all, slot_points, d_meta_all, meta_words, world, max_scans, d_packed,
            d_total, d_scan_start_all, d_n_points_all, d_status))

    def comm_fence(self, lag: int = 0):
        self._check(self._lib.rplgpu_comm_fence_lag(self._h, lag))

    def unpack_gathered_dev(self, d_points_all: int, slot_points: int, d_meta_all: int,
                            meta_words: int, world: int, max_scans: int, d_packed: int,
                            d_total: int, d_scan_start_all: int, d_n_points_all: int,
                            d_status: int = 0):
        self._check(self._lib.rplgpu_unpack_gathered_dev(
            self._h, d_points_all, slot_points, d_meta_all, meta_words, world, max_scans, d_packed,
            d_total, d_scan_start_all, d_n_points_all, d_status))

    def fused_cloud_msg_dev(self, d_arena: int, d_total_points: int, arena_capacity: int,
                            frame_id: str, sec: int, nanosec: int, d_msg: int, msg_capacity: int,
                            d_msg_len: int, d_status: int = 0):
        """The whole arena as one serialised PointCloud2 in device memory."""
        self._check(self._lib.rplgpu_fused_cloud_msg_dev(
            self._h, d_arena, d_total_points, arena_capacity, frame_id.encode(),
            Stamp(sec, nanosec), d_msg, msg_capacity, d_msg_len, d_status))

    # -- decode stage: recorded answer streams -> nodes -> scans -----
    def decode_stream(self, ans_type: int, data: np.ndarray, sample_duration_us: int = 125,
                      state=(0, 0)):
        """One stream, host buffers: host framing + GPU decode.  Returns
        ``(nodes, reset_at, n_errors, state_out)``."""
        data = np.ascontiguousarray(data, np.uint8)
        S = self._lib.rplgpu_frame_size(ans_type)
        npf = self._lib.rplgpu_nodes_per_frame(ans_type)
        cap = (len(data) // max(S, 1) + 1) * npf
        nodes = np.zeros(max(cap, 1), NODE_DTYPE)
        rst = np.zeros(len(data) // max(S, 1) + 2, np.uint32)
        st = np.zeros(4, np.int32)
        st[: len(state)] = state
        n, nr, ne = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0)
        self._check(self._lib.rplgpu_decode_stream(
            self._h, ans_type, sample_duration_us, data.ctypes.data, len(data), st.ctypes.data,
            nodes.ctypes.data, len(nodes), C.byref(n), rst.ctypes.data, len(rst), C.byref(nr),
            C.byref(ne)))
        return nodes[: n.value], rst[: nr.value], int(ne.value), (int(st[0]), int(st[1]))

    def decode_batch_dev(self, ans_type: int, sample_duration_us: int, d_bytes: int,
                         stream_stride: int, d_frame_off: int, d_gap: int, d_n_frames: int,
                         max_frames: int, B: int, d_state_in: int, d_state_out: int, d_nodes: int,
                         node_stride: int, d_n_nodes: int, d_reset_at: int = 0,
                         reset_stride: int = 0, d_n_reset: int = 0, d_n_errors: int = 0,
                         d_status: int = 0):
        self._check(self._lib.rplgpu_decode_batch_dev(
            self._h, ans_type, sample_duration_us, d_bytes, stream_stride, d_frame_off, d_gap,
            d_n_frames, max_frames, B, d_state_in, d_state_out, d_nodes, node_stride, d_n_nodes,
            d_reset_at, reset_stride, d_n_reset, d_n_errors, d_status))

    def decode_scans_dev(self, ans_type: int, sample_duration_us: int, d_bytes: int,
                         stream_stride: int, d_frame_off: int, d_gap: int, d_n_frames: int,
                         max_frames: int, B: int, d_state_in: int, d_state_out: int,
                         max_count: int, d_batch: int, n_stride: int, scan_cap: int,
                         d_n_per_scan: int, d_n_scans: int, d_n_errors: int, d_status: int):
        """Recorded streams -> completed scans in batch slots b*scan_cap + s (one call)."""
        self._check(self._lib.rplgpu_decode_scans_dev(
            self._h, ans_type, sample_duration_us, d_bytes, stream_stride, d_frame_off, d_gap,
            d_n_frames, max_frames, B, d_state_in, d_state_out, max_count, d_batch, n_stride,
            scan_cap, d_n_per_scan, d_n_scans, d_n_errors, d_status))

    def decode_scans_carry_dev(self, ans_type: int, sample_duration_us: int, d_bytes: int,
                               stream_stride: int, d_frame_off: int, d_gap: int, d_n_frames: int,
                               max_frames: int, B: int, d_state_in: int, d_state_out: int,
                               max_count: int, d_batch: int, n_stride: int, scan_cap: int,
                               d_n_per_scan: int, d_n_scans: int, d_n_errors: int, d_status: int,
                               d_carry_in: int, d_carry_len_in: int, d_carry_out: int,
                               d_carry_len_out: int, carry_stride: int):
        """decode_scans_dev for one piece of a longer recording: the scan open at the end of the
        call leaves in d_carry_out and enters the next call as d_carry_in."""
        self._check(self._lib.rplgpu_decode_scans_carry_dev(
            self._h, ans_type, sample_duration_us, d_bytes, stream_stride, d_frame_off or None,
            d_gap or None, d_n_frames, max_frames, B, d_state_in or None, d_state_out or None,
            max_count, d_batch, n_stride, scan_cap, d_n_per_scan, d_n_scans, d_n_errors or None,
            d_status, d_carry_in or None, d_carry_len_in or None, d_carry_out, d_carry_len_out,
            carry_stride))

    def segment_batch_dev(self, d_nodes: int, node_stride: int, d_n_nodes: int, d_reset_at: int,
                          reset_stride: int, d_n_reset: int, B: int, max_count: int,
                          d_out_nodes: int, out_stride: int, d_scan_off: int, scan_cap: int,
                          d_n_scans: int, d_status: int = 0):
        self._check(self._lib.rplgpu_segment_batch_dev(
            self._h, d_nodes, node_stride, d_n_nodes, d_reset_at, reset_stride, d_n_reset, B,
            max_count, d_out_nodes, out_stride, d_scan_off, scan_cap, d_n_scans, d_status))

    def scans_to_batch_dev(self, d_seg_nodes: int, seg_stride: int, d_scan_off: int,
                           scan_cap: int, d_n_scans: int, B: int, d_scan_base: int, d_batch: int,
                           n_stride: int, max_scans: int, d_n_per_scan: int):
        self._check(self._lib.rplgpu_scans_to_batch_dev(
            self._h, d_seg_nodes, seg_stride, d_scan_off, scan_cap, d_n_scans, B, d_scan_base,
            d_batch, n_stride, max_scans, d_n_per_scan))


def cloud_meta_words(max_scans: int) -> int:
    return int(load_library().rplgpu_cloud_meta_words(max_scans))


def msg_laserscan_layout(frame_id_len: int, count: int) -> LaserScanLayout:
    L = LaserScanLayout()
    rc = load_library().rplgpu_msg_laserscan_layout(frame_id_len, count, C.byref(L))
    if rc:
        raise RplGpuError(rc, "rplgpu_msg_laserscan_layout")
    return L


def msg_cloud_layout(frame_id_len: int, n_points: int) -> CloudLayout:
    L = CloudLayout()
    rc = load_library().rplgpu_msg_cloud_layout(frame_id_len, n_points, C.byref(L))
    if rc:
        raise RplGpuError(rc, "rplgpu_msg_cloud_layout")
    return L


def msg_laserscan_header(frame_id: str, sec: int, nanosec: int, meta: ScanMeta,
                         out: np.ndarray) -> LaserScanLayout:
    """Host-only: everything of a serialised LaserScan but the two float arrays, into ``out``."""
    L = LaserScanLayout()
    rc = load_library().rplgpu_msg_laserscan_header(
        frame_id.encode(), Stamp(sec, nanosec), C.byref(meta), out.ctypes.data, out.nbytes,
        C.byref(L))
    if rc:
        raise RplGpuError(rc, "rplgpu_msg_laserscan_header")
    return L


def msg_cloud_header(frame_id: str, sec: int, nanosec: int, n_points: int,
                     out: np.ndarray) -> CloudLayout:
    """Host-only: everything of a serialised PointCloud2 but the points, into ``out``."""
    L = CloudLayout()
    rc = load_library().rplgpu_msg_cloud_header(
        frame_id.encode(), Stamp(sec, nanosec), n_points, out.ctypes.data, out.nbytes, C.byref(L))
    if rc:
        raise RplGpuError(rc, "rplgpu_msg_cloud_header")
    return L


def frame_stream(ans_type: int, data: np.ndarray):
    """Host framing (``rplgpu_frame_stream``): ``(frame_off, gap)`` of a recorded byte stream."""
    lib = load_library()
    data = np.ascontiguousarray(data, np.uint8)
    S = lib.rplgpu_frame_size(ans_type)
    if not S:
        raise ValueError(f"unknown answer type {ans_type:#x}")
    cap = len(data) // S + 1
    off = np.zeros(cap, np.uint32)
    gap = np.zeros(cap, np.uint8)
    nf = lib.rplgpu_frame_stream(ans_type, data.ctypes.data, len(data), off.ctypes.data,
                                 gap.ctypes.data, cap)
    return off[:nf], gap[:nf]


# -- host twins of the exchange layout (include/rplgpu_comm.h; no device, no handle) -----------
def pack_cloud_meta_host(cursor: int, scan_start: np.ndarray, n_points: np.ndarray, slot_points: int,
                         max_scans: int) -> np.ndarray:
    """META block of a rank's arena, as ``rplgpu_pack_cloud_meta_dev`` writes it."""
    lib = load_library()
    ss = np.ascontiguousarray(scan_start, np.uint64)
    npnt = np.ascontiguousarray(n_points, np.uint32)
    words = int(lib.rplgpu_cloud_meta_words(max_scans))
    meta = np.zeros(words, np.uint32)
    rc = lib.rplgpu_pack_cloud_meta_host(int(cursor), ss.ctypes.data, npnt.ctypes.data, len(npnt),
                                         int(slot_points), int(max_scans), meta.ctypes.data)
    if rc:
        raise RplGpuError(rc, "rplgpu_pack_cloud_meta_host")
    return meta


def pack_cloud_xyi_host(arena: np.ndarray, cursor: int, slot_points: int) -> np.ndarray:
    """A rank's compact slot (slot_points x 3 float32) from its arena ((cap, 4) float32)."""
    a = np.ascontiguousarray(arena, np.float32)
    slot = np.zeros((int(slot_points), 3), np.float32)
    rc = load_library().rplgpu_pack_cloud_xyi_host(a.ctypes.data, int(cursor), int(slot_points),
                                                   slot.ctypes.data)
    if rc:
        raise RplGpuError(rc, "rplgpu_pack_cloud_xyi_host")
    return slot


def unpack_gathered_host(points_all: np.ndarray, slot_points: int, meta_all: np.ndarray, world: int,
                         max_scans: int):
    """Gathered slots ((world, slot_points, 3 | 4) float32) + META blocks ((world, words) uint32) ->
    (packed (total, 4), scan_start_all (world, max_scans) uint64, n_points_all (world, max_scans)
    uint32, status (world,) uint32), by the library's own layout code."""
    lib = load_library()
    pts = np.ascontiguousarray(points_all, np.float32)
    point_floats = int(pts.shape[-1])
    meta = np.ascontiguousarray(meta_all, np.uint32).reshape(world, -1)
    packed = np.zeros((world * int(slot_points), 4), np.float32)
    total = np.zeros(1, np.uint64)
    starts = np.zeros((world, max_scans), np.uint64)
    npts = np.zeros((world, max_scans), np.uint32)
    status = np.zeros(world, np.uint32)
    rc = lib.rplgpu_unpack_gathered_host(pts.ctypes.data, int(slot_points), point_floats,
                                         meta.ctypes.data, int(meta.shape[1]), int(world),
                                         int(max_scans), packed.ctypes.data, total.ctypes.data,
                                         starts.ctypes.data, npts.ctypes.data, status.ctypes.data)
    if rc:
        raise RplGpuError(rc, "rplgpu_unpack_gathered_host")
    return packed[: int(total[0])], starts, npts, status


def merge_cells_host(cells_all: np.ndarray, slot_cells: int, meta_all: np.ndarray, world: int,
                     n_groups: int, params: Params, arena_capacity: int | None = None):
    """Gathered cell slots ((world, slot_cells) CELL_DTYPE) + META blocks ((world, words) uint32) ->
    (arena (arena_capacity, 4) float32, cursor, group_start (n_groups,) uint64, n_points (n_groups,)
    uint32, status (n_groups,) uint32), by the library's own rules (rplgpu_merge_cells_host)."""
    lib = load_library()
    cells = np.ascontiguousarray(cells_all, CELL_DTYPE).reshape(-1)
    meta = np.ascontiguousarray(meta_all, np.uint32).reshape(world, -1)
    if cells.size < world * int(slot_cells):
        raise ValueError("cells_all holds fewer than world x slot_cells records")
    cap = int(world * int(slot_cells) if arena_capacity is None else arena_capacity)
    arena = np.zeros((max(cap, 1), 4), np.float32)
    cursor = np.zeros(1, np.uint64)
    starts = np.zeros(max(n_groups, 1), np.uint64)
    npts = np.zeros(max(n_groups, 1), np.uint32)
    status = np.zeros(max(n_groups, 1), np.uint32)
    rc = lib.rplgpu_merge_cells_host(cells.ctypes.data, int(slot_cells), meta.ctypes.data,
                                     int(meta.shape[1]), int(world), int(n_groups), C.byref(params),
                                     arena.ctypes.data, cap, cursor.ctypes.data, starts.ctypes.data,
                                     npts.ctypes.data, status.ctypes.data)
    if rc:
        raise RplGpuError(rc, "rplgpu_merge_cells_host")
    return arena[:cap], int(cursor[0]), starts[:n_groups], npts[:n_groups], status[:n_groups]


def scan_merge_edges(merge: ScanMerge):
    """Host only: (edges (count + 1, 2) float32, inc float32) of an E9 spec by the library's own
    rplgpu_scan_merge_edges.  Raises RplGpuError(ERR_INVALID_ARG) for a spec the library refuses."""
    lib = load_library()
    n = int(merge.count) + 1 if 0 < int(merge.count) <= MAX_MERGE_BEAMS else 1
    edges = np.zeros((n, 2), np.float32)
    inc = np.zeros(1, np.float32)
    rc = lib.rplgpu_scan_merge_edges(C.byref(merge), edges.ctypes.data, inc.ctypes.data)
    if rc:
        raise RplGpuError(rc, "rplgpu_scan_merge_edges")
    return edges, inc[0]


def scan_filter_check(flt: ScanFilter) -> np.ndarray:
    """Host only: validates an E10 filter by the library's own rplgpu_scan_filter_check and returns
    (cmin, smin, cmax, smax) float32.  Raises RplGpuError(ERR_INVALID_ARG) for a filter it refuses."""
    dirs = np.zeros(4, np.float32)
    rc = load_library().rplgpu_scan_filter_check(C.byref(flt), dirs.ctypes.data)
    if rc:
        raise RplGpuError(rc, "rplgpu_scan_filter_check")
    return dirs


def occ_grid_check(grid: OccGrid) -> None:
    """Host only: validates an E11 grid spec by the library's own rplgpu_occ_grid_check; raises
    RplGpuError(ERR_INVALID_ARG) for a spec the library refuses."""
    rc = load_library().rplgpu_occ_grid_check(C.byref(grid))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_occ_grid_check")


def msg_occupancy_layout(frame_id_len: int, width: int, height: int) -> OccupancyLayout:
    """Host only: byte offsets inside one serialised nav_msgs/OccupancyGrid."""
    lay = OccupancyLayout()
    rc = load_library().rplgpu_msg_occupancy_layout(frame_id_len, width, height, C.byref(lay))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_msg_occupancy_layout")
    return lay


def inflation_check(inflation: Inflation, resolution: float) -> None:
    """Host only: validates an E12 spec by the library's own rplgpu_inflation_check; raises
    RplGpuError(ERR_INVALID_ARG) for a spec the library refuses."""
    rc = load_library().rplgpu_inflation_check(C.byref(inflation), resolution)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_inflation_check")


def inflation_table(inflation: Inflation, resolution: float):
    """Host only: (table uint8 (Rc * Rc + 1,), Rc) of an E12 spec by the library's own
    rplgpu_inflation_table: the cost by squared cell distance."""
    table = np.zeros(MAX_INFLATION_CELLS * MAX_INFLATION_CELLS + 1, np.uint8)
    reach = np.zeros(1, np.uint32)
    rc = load_library().rplgpu_inflation_table(C.byref(inflation), resolution, table.ctypes.data, len(table),
                                               reach.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_inflation_table")
    r = int(reach[0])
    return table[:r * r + 1].copy(), r


def scan_match_check(match: ScanMatch) -> None:
    """Host only: validates an E13 spec by the library's own rplgpu_scan_match_check; raises
    RplGpuError(ERR_INVALID_ARG) for a spec the device path would refuse."""
    rc = load_library().rplgpu_scan_match_check(C.byref(match))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_scan_match_check")


def map_rule_check(rule: MapRule) -> None:
    """Host only: validates an E14 cell rule by the library's own rplgpu_map_rule_check; raises
    RplGpuError(ERR_INVALID_ARG) for a rule the device path would refuse."""
    rc = load_library().rplgpu_map_rule_check(C.byref(rule))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_map_rule_check")


def scan_match_rotations(match: ScanMatch) -> np.ndarray:
    """Host only: the (2K + 1, 2) float32 rotation table (cos, sin of k * rot_step, k = -K .. K) by the library's
    own rplgpu_scan_match_rotations."""
    cs = np.zeros((2 * match.rot_steps + 1, 2), np.float32)
    rc = load_library().rplgpu_scan_match_rotations(C.byref(match), cs.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_scan_match_rotations")
    return cs


def scan_match_volume(match: ScanMatch) -> int:
    """Host only: the words of one group's score volume, (2K + 1)(2Ty + 1)(2Tx + 1); 0 for an invalid spec."""
    return int(load_library().rplgpu_scan_match_volume(C.byref(match)))


def pose_score_check(spec: PoseScore) -> None:
    """Host only: validates an E15 spec by the library's own rplgpu_pose_score_check; raises
    RplGpuError(ERR_INVALID_ARG) for a spec the device path would refuse."""
    rc = load_library().rplgpu_pose_score_check(C.byref(spec))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_pose_score_check")


def pose_list(xyt) -> np.ndarray:
    """Host only: poses (P, 3) float64 (x, y, theta) -> the (P, 4) float32 list (cos, sin, x, y) that
    score_poses_dev takes, by the library's own rplgpu_pose_list."""
    xyt = np.ascontiguousarray(xyt, np.float64).reshape(-1, 3)
    out = np.zeros((len(xyt), 4), np.float32)
    rc = load_library().rplgpu_pose_list(xyt.ctypes.data, len(xyt), out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_pose_list")
    return out


def resample_scratch_words(G: int, P: int) -> int:
    """Host only: the uint32 words of scratch resample_poses_dev needs for G groups of P poses; 0 for G = 0 or a P
    outside 1 .. MAX_POSES."""
    return int(load_library().rplgpu_resample_scratch_words(G, P))


def _resample_args(weights, poses, M, delta):
    weights = np.ascontiguousarray(weights, np.uint32)
    poses = np.ascontiguousarray(poses, np.float32)
    if weights.ndim != 1 or poses.shape != (len(weights), 4):
        raise TypeError("weights must be (P,) uint32 and poses (P, 4) float32")
    n_delta = 0
    if delta is not None:
        delta = np.ascontiguousarray(delta, np.float32).reshape(-1, 4)
        n_delta = len(delta)
    return weights, poses, delta, n_delta


def resample_host(weights, poses, M: int, u: int = 0, delta=None):
    """Host only: E16's rule for one group by the library's own rplgpu_resample_host (no handle, no device);
    arguments and results as ``RplGpu.resample_poses``."""
    weights, poses, delta, n_delta = _resample_args(weights, poses, M, delta)
    ok = 0 < M <= MAX_POSES
    out = np.zeros((M if ok else 1, 4), np.float32)
    anc = np.zeros(M if ok else 1, np.uint32)
    result = np.zeros(8, np.uint32)
    rc = load_library().rplgpu_resample_host(
        weights.ctypes.data, len(weights), M, u, poses.ctypes.data, 0 if delta is None else delta.ctypes.data,
        n_delta, out.ctypes.data, anc.ctypes.data, result.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_resample_host")
    return out, anc, result


def estimate_scratch_words(G: int, P: int) -> int:
    """Host only: the uint32 words of scratch estimate_poses_dev needs for G groups of P poses; 0 for arguments the
    call refuses."""
    return int(load_library().rplgpu_estimate_scratch_words(G, P))


def pose_estimate_check(spec: PoseEstimate) -> None:
    """Host only: validates an E17 spec by the library's own rplgpu_pose_estimate_check; raises RplGpuError."""
    rc = load_library().rplgpu_pose_estimate_check(C.byref(spec))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_pose_estimate_check")


def _estimate_args(poses, weights, spec):
    poses = np.ascontiguousarray(poses, np.float32)
    if poses.ndim != 2 or poses.shape[1] != 4:
        raise TypeError("poses must be (P, 4) float32")
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.uint32)
        if weights.shape != (len(poses),):
            raise TypeError("weights must be (P,) uint32 or None")
    return poses, weights, PoseEstimate.defaults() if spec is None else spec


def estimate_host(poses, weights=None, spec: PoseEstimate = None, center: int = 0) -> np.ndarray:
    """Host only: E17's rule for one group by the library's own rplgpu_estimate_host (no handle, no device);
    arguments and result as ``RplGpu.estimate_poses``."""
    poses, weights, spec = _estimate_args(poses, weights, spec)
    result = np.zeros(ESTIMATE_WORDS, np.uint32)
    rc = load_library().rplgpu_estimate_host(poses.ctypes.data, len(poses),
                                             0 if weights is None else weights.ctypes.data, C.byref(spec), center,
                                             result.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_estimate_host")
    return result


def estimate_pose(result, xy_scale: float, set_: int = 0) -> np.ndarray:
    """Host only: set ``set_`` of one group's E17 result words as (mean x, mean y, theta, cov xx, xy, yy, R, W),
    fp64, by the library's own rplgpu_estimate_pose; raises RplGpuError for a set whose W is 0."""
    result = np.ascontiguousarray(result, np.uint32)
    if result.shape != (ESTIMATE_WORDS,):
        raise TypeError("result must be (72,) uint32")
    out = np.zeros(8, np.float64)
    rc = load_library().rplgpu_estimate_pose(result.ctypes.data, xy_scale, set_, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_estimate_pose")
    return out


def _motion_args(odom, spec):
    odom = np.ascontiguousarray(odom, np.float32)
    if odom.shape != (8,):
        raise TypeError("odom must be (8,) float32")
    return odom, MotionNoise.defaults() if spec is None else spec


def sample_motion_host(odom, M: int, spec: MotionNoise = None, group: int = 0):
    """Host only: E18's rule for one group (number ``group``) by the library's own rplgpu_sample_motion_host (no
    handle, no device); arguments and results as ``RplGpu.sample_motion``."""
    odom, spec = _motion_args(odom, spec)
    ok = 0 < M <= MAX_POSES
    delta = np.zeros((M if ok else 1, 4), np.float32)
    result = np.zeros(8, np.uint32)
    rc = load_library().rplgpu_sample_motion_host(odom.ctypes.data, group, M, C.byref(spec), delta.ctypes.data,
                                                  result.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_sample_motion_host")
    return delta, result


def philox4x32(ctr, key) -> np.ndarray:
    """Host only: one Philox4x32-10 block, ctr (4,) and key (2,) uint32 -> (4,) uint32, by the library's own
    rplgpu_philox4x32."""
    ctr = np.ascontiguousarray(ctr, np.uint32)
    key = np.ascontiguousarray(key, np.uint32)
    if ctr.shape != (4,) or key.shape != (2,):
        raise TypeError("ctr must be (4,) and key (2,) uint32")
    out = np.zeros(4, np.uint32)
    rc = load_library().rplgpu_philox4x32(ctr.ctypes.data, key.ctypes.data, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_philox4x32")
    return out


def motion_odometry(dx: float, dy: float, dtheta: float, alpha) -> np.ndarray:
    """Host only: an odometry increment in the old base frame and the model's four alphas -> E18's eight odometry
    floats (c1, s1, trans, c2, s2, k1, kt, k2), by the library's own rplgpu_motion_odometry."""
    alpha = np.ascontiguousarray(alpha, np.float64)
    if alpha.shape != (4,):
        raise TypeError("alpha must be (4,) float64")
    out = np.zeros(8, np.float32)
    rc = load_library().rplgpu_motion_odometry(dx, dy, dtheta, alpha.ctypes.data, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_motion_odometry")
    return out


def _seed_args(grid, headings, spec, noise):
    spec = PoseSeed.defaults() if spec is None else spec
    grid = np.ascontiguousarray(grid, np.int8)
    headings = np.ascontiguousarray(headings, np.float32)
    if grid.size != spec.width * spec.height:
        raise TypeError("grid must hold width * height int8 cells")
    if headings.ndim != 2 or headings.shape[1] != 2:
        raise TypeError("headings must be (H, 2) float32")
    return grid, headings, spec, MotionNoise.defaults() if noise is None else noise


def seed_scratch_words(G_f: int, width: int, height: int) -> int:
    """Host only: the uint32 words of scratch seed_poses_dev needs for G_f grids of width x height cells; 0 for
    arguments the call refuses."""
    return int(load_library().rplgpu_seed_scratch_words(G_f, width, height))


def seed_headings(H: int) -> np.ndarray:
    """Host only: the H headings (cos, sin)(2 pi k / H) as (H, 2) float32, by the library's own
    rplgpu_seed_headings."""
    out = np.zeros((max(H, 1), 2), np.float32)
    rc = load_library().rplgpu_seed_headings(H, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_seed_headings")
    return out


def seed_poses_host(grid, headings, M: int, spec: PoseSeed = None, noise: MotionNoise = None, group: int = 0):
    """Host only: E19's rule for one group (number ``group``) by the library's own rplgpu_seed_poses_host (no handle,
    no device); arguments and results as ``RplGpu.seed_poses``."""
    grid, headings, spec, noise = _seed_args(grid, headings, spec, noise)
    ok = 0 < M <= MAX_POSES
    poses = np.zeros((M if ok else 1, 4), np.float32)
    cells = np.zeros(M if ok else 1, np.uint32)
    result = np.zeros(8, np.uint32)
    rc = load_library().rplgpu_seed_poses_host(C.byref(spec), grid.ctypes.data, headings.ctypes.data, len(headings),
                                               group, M, C.byref(noise), poses.ctypes.data, cells.ctypes.data,
                                               result.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_seed_poses_host")
    return poses, cells, result


def _bins_args(poses, edges, weights, spec, map_in):
    spec = PoseBins.defaults() if spec is None else spec
    poses = np.ascontiguousarray(poses, np.float32)
    edges = np.ascontiguousarray(edges, np.float32)
    if poses.ndim != 2 or poses.shape[1] != 4:
        raise TypeError("poses must be (P, 4) float32")
    if edges.ndim != 2 or edges.shape[1] != 2:
        raise TypeError("edges must be (T, 2) float32")
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.uint32)
        if weights.shape != (len(poses),):
            raise TypeError("weights must be (P,) uint32")
    if spec.check(len(edges)) != OK:
        raise RplGpuError(ERR_INVALID_ARG, "rplgpu_pose_bins_check")
    words = (spec.nx * spec.ny * len(edges) + 31) // 32
    bmap = np.zeros(words, np.uint32) if map_in is None else np.array(map_in, np.uint32).reshape(-1)
    if bmap.size != words:
        raise TypeError("map_in must hold ceil(nx * ny * T / 32) words")
    return poses, edges, weights, spec, bmap


def bin_map_words(nx: int, ny: int, T: int) -> int:
    """Host only: the even number of uint32 words of one group's bit map (a valid map_stride); 0 for arguments the
    call refuses."""
    return int(load_library().rplgpu_bin_map_words(nx, ny, T))


def heading_edges_check(edges) -> int:
    """Host only: OK when the (T, 2) float32 table is a VALID table of bin edges (rplgpu_heading_edges_check)."""
    edges = np.ascontiguousarray(edges, np.float32)
    return int(load_library().rplgpu_heading_edges_check(edges.ctypes.data, len(edges)))


def kld_samples(k: int, epsilon: float = 0.01, z: float = 3.0, m_min: int = 500, m_max: int = 100000) -> int:
    """Host only: AMCL's pf_resample_limit by the library's own rplgpu_kld_samples."""
    return int(load_library().rplgpu_kld_samples(k, epsilon, z, m_min, m_max))


def bin_poses_host(poses, edges, weights=None, spec: PoseBins = None, map_in=None):
    """Host only: E20's rule for one group by the library's own rplgpu_bin_poses_host (no handle, no device);
    arguments and results as ``RplGpu.bin_poses``."""
    poses, edges, weights, spec, bmap = _bins_args(poses, edges, weights, spec, map_in)
    bins = np.zeros(max(len(poses), 1), np.uint32)
    result = np.zeros(8, np.uint32)
    rc = load_library().rplgpu_bin_poses_host(
        C.byref(spec), poses.ctypes.data, len(poses), weights.ctypes.data if weights is not None else None,
        edges.ctypes.data, len(edges), bmap.ctypes.data, bins.ctypes.data, result.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_bin_poses_host")
    return bmap, bins[:len(poses)], result


def _cluster_args(poses, bmap, bins, T, weights, spec, cluster_cap, clusters_in):
    spec = PoseClusters.defaults() if spec is None else spec
    poses = np.ascontiguousarray(poses, np.float32)
    bins = np.ascontiguousarray(bins, np.uint32)
    bmap = np.ascontiguousarray(bmap, np.uint32)
    if poses.ndim != 2 or poses.shape[1] != 4:
        raise TypeError("poses must be (P, 4) float32")
    if bins.shape != (len(poses),):
        raise TypeError("bins must be (P,) uint32")
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.uint32)
        if weights.shape != (len(poses),):
            raise TypeError("weights must be (P,) uint32")
    if spec.check(T) != OK:
        raise RplGpuError(ERR_INVALID_ARG, "rplgpu_pose_clusters_check")
    if bmap.shape != ((spec.nx * spec.ny * T + 31) // 32,):
        raise TypeError("the map must hold ceil(nx * ny * T / 32) words")
    table = np.zeros((cluster_cap, 4), np.uint32) if clusters_in is None else np.array(clusters_in, np.uint32)
    if table.shape != (cluster_cap, 4):
        raise TypeError("clusters_in must be (cluster_cap, 4) uint32")
    return poses, bmap, bins, weights, spec, table


def cluster_scratch_words(G: int, P: int, nx: int, ny: int, T: int) -> int:
    """Host only: the uint32 words of scratch cluster_poses_dev needs; 0 for arguments the call refuses."""
    return int(load_library().rplgpu_cluster_scratch_words(G, P, nx, ny, T))


def cluster_poses_host(poses, bmap, bins, T: int, weights=None, spec: PoseClusters = None, cluster_cap: int = 0,
                       clusters_in=None):
    """Host only: E21's rule for one group by the library's own rplgpu_cluster_poses_host (no handle, no device);
    arguments and results as ``RplGpu.cluster_poses``."""
    poses, bmap, bins, weights, spec, table = _cluster_args(poses, bmap, bins, T, weights, spec, cluster_cap,
                                                            clusters_in)
    labels = np.zeros(max(len(poses), 1), np.uint32)
    result = np.zeros(CLUSTER_WORDS, np.uint32)
    rc = load_library().rplgpu_cluster_poses_host(
        C.byref(spec), poses.ctypes.data, len(poses), weights.ctypes.data if weights is not None else None, T,
        bmap.ctypes.data, bins.ctypes.data, labels.ctypes.data, table.ctypes.data if cluster_cap else None,
        cluster_cap, result.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_cluster_poses_host")
    return labels[:len(poses)], table, result


CAST_HIT, CAST_UNKNOWN, CAST_LEFT, CAST_NONE = 0, 1, 2, 3
CAST_DROPPED = 0xFFFFFFFF
MAX_CAST_RAYS = 1 << 28


def _cast_args(poses, beams, grid, spec, measured, table):
    spec = RangeCast.defaults() if spec is None else spec
    poses = np.ascontiguousarray(poses, np.float32)
    beams = np.ascontiguousarray(beams, np.float32)
    grid = np.ascontiguousarray(grid, np.int8)
    if poses.ndim != 2 or poses.shape[1] != 4:
        raise TypeError("poses must be (P, 4) float32")
    if beams.ndim != 2 or beams.shape[1] != 2:
        raise TypeError("beams must be (A, 2) float32")
    if spec.check() != OK:
        raise RplGpuError(ERR_INVALID_ARG, "rplgpu_range_cast_check")
    if grid.shape != (spec.height, spec.width):
        raise TypeError("grid must be (height, width) int8")
    if (measured is None) != (table is None):
        raise TypeError("measured and table come together")
    if measured is not None:
        measured = np.ascontiguousarray(measured, np.float32)
        table = np.ascontiguousarray(table, np.uint8)
        if measured.ndim != 1 or table.shape != (2 * spec.table_half + 2,):
            raise TypeError("measured must be (n,) float32 and table (2 * table_half + 2,) uint8")
    return poses, beams, grid, spec, measured, table


def cast_beams(merge: ScanMerge, first: int, step: int, A: int) -> np.ndarray:
    """Host only: the centre directions (cos, sin) of E9's beams first + a * step as (A, 2) float32, by the library's
    own rplgpu_cast_beams."""
    out = np.zeros((max(A, 1), 2), np.float32)
    rc = load_library().rplgpu_cast_beams(C.byref(merge), first, step, A, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_cast_beams")
    return out[:A]


def cast_range_m(word: int, resolution: float) -> float:
    """Host only: a range word in metres (+inf for NONE, NaN for a dropped ray), rplgpu_cast_range_m."""
    return float(load_library().rplgpu_cast_range_m(int(word) & 0xFFFFFFFF, resolution))


def cast_ranges_host(poses, beams, grid, spec: RangeCast = None, measured=None, table=None, meas_first: int = 0,
                     meas_step: int = 1, want_ranges: bool = True):
    """Host only: E22's rule for one group by the library's own rplgpu_cast_ranges_host (no handle, no device);
    arguments and results as ``RplGpu.cast_ranges``."""
    poses, beams, grid, spec, measured, table = _cast_args(poses, beams, grid, spec, measured, table)
    P, A = len(poses), len(beams)
    ok = 0 < P and 0 < A and P * A <= MAX_CAST_RAYS
    ranges = np.zeros((P, A) if ok else (1, 1), np.uint32) if want_ranges else None
    weights = np.zeros(max(P, 1), np.uint32) if measured is not None else None
    result = np.zeros(8, np.uint32) if measured is not None else None
    cast = np.zeros(8, np.uint32)
    rc = load_library().rplgpu_cast_ranges_host(
        C.byref(spec), poses.ctypes.data, P, beams.ctypes.data, A, grid.ctypes.data,
        measured.ctypes.data if measured is not None else None, len(measured) if measured is not None else 0,
        meas_first, meas_step, table.ctypes.data if table is not None else None,
        ranges.ctypes.data if want_ranges else None, weights.ctypes.data if weights is not None else None,
        result.ctypes.data if result is not None else None, cast.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_cast_ranges_host")
    return ranges, (weights[:P] if weights is not None else None), result, cast


def beam_agree_points_host(x, y, slot, index, n_scans: int, n_stride: int, poses, field, spec: BeamAgree):
    """Host only: E23's rule for one group over points, by the library's own rplgpu_beam_agree_points_host (no
    handle, no device).  x, y: the points in the base frame, slot / index: their scan and sample; poses (P, 4)
    float32; field (height, width) int8 -> ``(counts (n_scans, n_stride) uint32, mask (n_scans, ceil(n_stride / 32))
    uint32, weights (P,) uint32, result (8,) uint32, agree (8,) uint32, status)``."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    slot = np.ascontiguousarray(slot, np.uint32)
    index = np.ascontiguousarray(index, np.uint32)
    if not (x.ndim == 1 and x.shape == y.shape == slot.shape == index.shape):
        raise TypeError("x, y, slot and index must be 1-D arrays of one length")
    poses = np.ascontiguousarray(poses, np.float32)
    if poses.ndim != 2 or poses.shape[1] != 4:
        raise TypeError("poses must be a (P, 4) float32 array")
    field = np.ascontiguousarray(field, np.int8)
    if field.shape != (spec.height, spec.width):
        raise TypeError("field must be a (height, width) int8 array")
    P = len(poses)
    ok = 0 < n_scans and 0 < n_stride and n_scans * n_stride <= 1 << 24
    counts = np.zeros((n_scans, n_stride) if ok else (1, 1), np.uint32)
    mask = np.zeros((n_scans, (n_stride + 31) // 32) if ok else (1, 1), np.uint32)
    weights = np.zeros(max(P, 1), np.uint32)
    result = np.zeros(8, np.uint32)
    agree = np.zeros(8, np.uint32)
    status = np.zeros(1, np.uint32)
    rc = load_library().rplgpu_beam_agree_points_host(
        x.ctypes.data, y.ctypes.data, slot.ctypes.data, index.ctypes.data, len(x), n_scans, n_stride,
        poses.ctypes.data, P, field.ctypes.data, C.byref(spec), counts.ctypes.data, mask.ctypes.data,
        weights.ctypes.data, result.ctypes.data, agree.ctypes.data, status.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_beam_agree_points_host")
    return counts, mask, weights[:P], result, agree, int(status[0])


def wide_match_check(match: WideMatch) -> None:
    """Host only: validates an E24 spec by the library's own rplgpu_wide_match_check; raises RplGpuError."""
    rc = load_library().rplgpu_wide_match_check(C.byref(match))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_wide_match_check")


def wide_match_blocks(match: WideMatch) -> int:
    """Host only: the words of one group's bounds volume, (2K + 1) * nby * nbx; 0 for a spec the check refuses."""
    return int(load_library().rplgpu_wide_match_blocks(C.byref(match)))


def wide_match_scratch_words(match: WideMatch, G: int) -> int:
    """Host only: the uint32 words of scratch ``match_wide_dev`` takes for G groups; 0 for a refused spec."""
    return int(load_library().rplgpu_wide_match_scratch_words(C.byref(match), G))


def pool_field_host(field) -> np.ndarray:
    """Host only: E24's pooled field of a (height, width) int8 field, (height + 7, width + 7) int8, by the library's
    own rplgpu_pool_field_host."""
    field = np.ascontiguousarray(field, np.int8)
    if field.ndim != 2:
        raise TypeError("field must be a (height, width) int8 array")
    H, W = field.shape
    out = np.zeros((H + WIDE_MATCH_BLOCK - 1, W + WIDE_MATCH_BLOCK - 1), np.int8)
    rc = load_library().rplgpu_pool_field_host(field.ctypes.data, W, H, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_pool_field_host")
    return out


def pose_refine_check(spec: PoseRefine) -> None:
    """Host only: validates an E25 spec by the library's own rplgpu_pose_refine_check; raises RplGpuError."""
    rc = load_library().rplgpu_pose_refine_check(C.byref(spec))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_pose_refine_check")


def refine_scratch_words(G: int, P: int) -> int:
    """Host only: the uint32 words of scratch ``refine_sums_dev`` / ``refine_poses_dev`` take; 0 when refused."""
    return int(load_library().rplgpu_refine_scratch_words(G, P))


def refine_sums_host(x, y, poses, field, spec: PoseRefine):
    """Host only: E25's sums of one group's points (already in the base frame) by the library's plain C++ twin ->
    ``(sums (P, 32) uint32, result (8,) uint32, status)``."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 4)
    field = np.ascontiguousarray(field, np.int8)
    if field.shape != (spec.height, spec.width) or x.shape != y.shape or x.ndim != 1:
        raise TypeError("field must be (height, width) int8, x and y equally long 1-D arrays")
    sums = np.zeros((len(poses), REFINE_WORDS), np.uint32)
    result = np.zeros(8, np.uint32)
    status = np.zeros(1, np.uint32)
    rc = load_library().rplgpu_refine_sums_host(x.ctypes.data, y.ctypes.data, len(x), poses.ctypes.data, len(poses),
                                                field.ctypes.data, C.byref(spec), sums.ctypes.data,
                                                result.ctypes.data, status.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_refine_sums_host")
    return sums, result, int(status[0])


def refine_step_host(sums, spec: PoseRefine, pose):
    """Host only: E25's step of one pose from its 32 words of sums by the library's plain C++ twin ->
    ``(pose_out (4,) float32, step (4,) uint32)``; step[3] holds the flags."""
    sums = np.ascontiguousarray(sums, np.uint32)
    pose = np.ascontiguousarray(pose, np.float32)
    if sums.shape != (REFINE_WORDS,) or pose.shape != (4,):
        raise TypeError("sums must be 32 uint32 words, pose 4 floats")
    out = np.zeros(4, np.float32)
    step = np.zeros(4, np.uint32)
    rc = load_library().rplgpu_refine_step_host(sums.ctypes.data, C.byref(spec), pose.ctypes.data, out.ctypes.data,
                                                step.ctypes.data)
    if rc < 0:
        raise RplGpuError(rc, "rplgpu_refine_step_host")
    return out, step


def refine_covariance(sums, spec: PoseRefine):
    """Host only: (x, y, theta) covariance in metres and radians from a pose's sums, (3, 3) float64, or None when
    the matrix is singular."""
    sums = np.ascontiguousarray(sums, np.uint32)
    if sums.shape != (REFINE_WORDS,) or spec.check() != OK:
        raise TypeError("sums must be 32 uint32 words and the spec a checked one")
    cov = np.zeros(9, np.float64)
    rc = load_library().rplgpu_refine_covariance(sums.ctypes.data, C.byref(spec), cov.ctypes.data)
    return cov.reshape(3, 3) if rc == OK else None


def nav_field_check(spec: NavField) -> None:
    """Host only: validates an E26 spec by the library's own rplgpu_nav_field_check; raises RplGpuError."""
    rc = load_library().rplgpu_nav_field_check(C.byref(spec))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_nav_field_check")


def nav_field_default_rounds(width: int, height: int) -> int:
    """Host only: 2 (ntx + nty) + 2; 0 for a size the check refuses."""
    return int(load_library().rplgpu_nav_field_default_rounds(width, height))


def nav_field_scratch_words(spec: NavField, G: int) -> int:
    """Host only: the uint32 words of scratch ``nav_field_dev`` takes; 0 when refused."""
    return int(load_library().rplgpu_nav_field_scratch_words(C.byref(spec), G))


def nav_field_host(spec: NavField, grid, goals):
    """Host only: rplgpu_nav_field_host, the binary-heap Dijkstra -> ``(potential (height, width) uint32, result
    (8,) uint32)``."""
    grid = np.ascontiguousarray(grid, np.int8)
    if spec.check() != OK or grid.shape != (spec.height, spec.width):
        raise RplGpuError(ERR_INVALID_ARG, "nav_field_host: a checked spec and a (height, width) int8 grid")
    goals = np.ascontiguousarray(goals, np.uint32).reshape(-1)
    pot = np.zeros((spec.height, spec.width), np.uint32)
    result = np.zeros(8, np.uint32)
    rc = load_library().rplgpu_nav_field_host(C.byref(spec), grid.ctypes.data, goals.ctypes.data if len(goals) else 0,
                                              len(goals), pot.ctypes.data, result.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_nav_field_host")
    return pot, result


def nav_path_host(spec: NavField, grid, potential, start: int, max_len: int, path_fill: int = 0):
    """Host only: rplgpu_nav_path_host -> ``(path (max_len,) uint32, info (4,) uint32)``."""
    grid = np.ascontiguousarray(grid, np.int8)
    potential = np.ascontiguousarray(potential, np.uint32)
    if spec.check() != OK or grid.shape != (spec.height, spec.width) or potential.shape != grid.shape or max_len < 1:
        raise RplGpuError(ERR_INVALID_ARG, "nav_path_host: a checked spec, a grid and a potential of its shape")
    path = np.full(max_len, path_fill, np.uint32)
    info = np.zeros(4, np.uint32)
    rc = load_library().rplgpu_nav_path_host(C.byref(spec), grid.ctypes.data, potential.ctypes.data, start,
                                             path.ctypes.data, max_len, info.ctypes.data)
    if rc < 0:
        raise RplGpuError(rc, "rplgpu_nav_path_host")
    return path, info


def frontiers_check(spec: Frontiers) -> None:
    """Host only: validates an E29 spec by the library's own rplgpu_frontiers_check; raises RplGpuError."""
    rc = load_library().rplgpu_frontiers_check(C.byref(spec))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_frontiers_check")


def frontiers_scratch_words(spec: Frontiers, G: int, comp_cap: int) -> int:
    """Host only: the uint32 words of scratch ``frontiers_dev`` takes; 0 when refused."""
    return int(load_library().rplgpu_frontiers_scratch_words(C.byref(spec), G, comp_cap))


def _frontier_args(spec, grid, potential, comp_cap, row_cap, labels, row_fill, goal_fill):
    """The argument list (behind the handle) that rplgpu_frontiers_host and rplgpu_frontiers share, and the
    dictionary of the arrays it points into."""
    grid = np.ascontiguousarray(grid, np.int8)
    if grid.shape != (spec.height, spec.width):
        raise RplGpuError(ERR_INVALID_ARG, "frontiers: a (height, width) int8 grid")
    if potential is not None:
        potential = np.ascontiguousarray(potential, np.uint32)
        if potential.shape != grid.shape:
            raise RplGpuError(ERR_INVALID_ARG, "frontiers: a potential of the grid's shape")
    out = {
        "labels": np.zeros(grid.shape, np.uint32) if labels else None,
        "rows": np.full((row_cap, 8), row_fill, np.uint32),
        "goal": np.full(1, goal_fill, np.uint32),
        "n_goal": np.zeros(1, np.uint32),
        "result": np.zeros(16, np.uint32),
        "grid": grid, "potential": potential,
    }
    args = (C.byref(spec), grid.ctypes.data, potential.ctypes.data if potential is not None else 0, comp_cap,
            out["labels"].ctypes.data if labels else 0, out["rows"].ctypes.data if row_cap else 0, row_cap,
            out["goal"].ctypes.data, out["n_goal"].ctypes.data, out["result"].ctypes.data)
    return args, out


def frontiers_host(spec: Frontiers, grid, potential=None, comp_cap: int = 4096, row_cap: int = 0,
                   labels: bool = True, row_fill: int = 0, goal_fill: int = 0) -> dict:
    """Host only: rplgpu_frontiers_host, the flood fill -> ``{"labels" (height, width) uint32 or None, "rows"
    (row_cap, 8) uint32 (rows beyond result[14] keep ``row_fill``), "goal" (1,), "n_goal" (1,), "result" (16,)}``."""
    a = _frontier_args(spec, grid, potential, comp_cap, row_cap, labels, row_fill, goal_fill)
    rc = load_library().rplgpu_frontiers_host(*a[0])
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_frontiers_host")
    return a[1]


def rollout_check(spec: Rollout) -> None:
    """Host only: validates an E27 spec by the library's own rplgpu_rollout_check; raises RplGpuError."""
    rc = load_library().rplgpu_rollout_check(C.byref(spec))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_rollout_check")


def rollout_scratch_words(G: int, K: int) -> int:
    """Host only: the uint32 words of scratch ``rollout_dev`` takes; 0 when refused."""
    return int(load_library().rplgpu_rollout_scratch_words(G, K))


def rollout_deltas(vxyw, dt: float) -> np.ndarray:
    """Host only: K body velocities (vx, vy, w) held for dt seconds -> the (K, 4) float32 deltas of E27's arcs, by
    the library's own rplgpu_rollout_deltas."""
    vxyw = np.ascontiguousarray(vxyw, np.float64).reshape(-1, 3)
    out = np.zeros((max(len(vxyw), 1), 4), np.float32)
    rc = load_library().rplgpu_rollout_deltas(vxyw.ctypes.data, len(vxyw), dt, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_rollout_deltas")
    return out


def _rollout_args(spec, start, delta, footprint, grid, potential):
    """-> (the arguments behind the spec, (out, end_poses, result)); the arrays stay alive in the first tuple."""
    start = np.ascontiguousarray(start, np.float32).reshape(-1)
    delta = np.ascontiguousarray(delta, np.float32)
    footprint = np.ascontiguousarray(footprint, np.float32).reshape(-1, 2)
    grid = np.ascontiguousarray(grid, np.int8)
    per_step = 1 if delta.ndim == 3 else 0
    if start.shape != (4,) or delta.ndim not in (2, 3) or delta.shape[-1] != 4 or len(delta) == 0 or \
            (per_step and delta.shape[1] != spec.steps) or grid.shape != (spec.height, spec.width):
        raise TypeError("start (4,), delta (K, 4) or (K, steps, 4), footprint (F, 2), grid (height, width) int8")
    if potential is not None:
        potential = np.ascontiguousarray(potential, np.uint32)
        if potential.shape != grid.shape:
            raise TypeError("potential must have the grid's shape")
    K = len(delta)
    out = np.zeros((K, 8), np.uint32)
    end = np.zeros((K, 4), np.float32)
    result = np.zeros(8, np.uint32)
    keep = (start, delta, footprint, grid, potential)
    args = (start.ctypes.data, delta.ctypes.data, per_step, footprint.ctypes.data, len(footprint), grid.ctypes.data,
            0 if potential is None else potential.ctypes.data, K, out.ctypes.data, end.ctypes.data,
            result.ctypes.data)
    return args, (out, end, result), keep


def rollout_host(spec: Rollout, start, delta, footprint, grid, potential=None):
    """Host only: E27's rules for one group by the library's own rplgpu_rollout_host (no handle, no device);
    arguments and results as ``RplGpu.rollout``."""
    a = _rollout_args(spec, start, delta, footprint, grid, potential)
    rc = load_library().rplgpu_rollout_host(C.byref(spec), *a[0])
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_rollout_host")
    return a[1]


def mppi_check(spec: Mppi) -> None:
    """Host only: validates an E28 spec by the library's own rplgpu_mppi_check; raises RplGpuError."""
    rc = load_library().rplgpu_mppi_check(C.byref(spec))
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_mppi_check")


def mppi_scratch_words(G: int, K: int, T_e: int) -> int:
    """Host only: the uint32 words of scratch ``mppi_update_dev`` takes; 0 when refused."""
    return int(load_library().rplgpu_mppi_scratch_words(G, K, T_e))


def mppi_table(lam: float, shift: int, N: int) -> np.ndarray:
    """Host only: the (N,) uint16 softmax table of temperature ``lam`` (score units), by the library's own
    rplgpu_mppi_table."""
    out = np.zeros(max(min(N, MPPI_MAX_TABLE), 1), np.uint16)
    rc = load_library().rplgpu_mppi_table(lam, shift, N, out.ctypes.data)
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_mppi_table")
    return out


def _mppi_update_args(spec, out, rollout_result, delta, table, nominal):
    """-> (the arguments behind the spec, (weights, sums, nominal_out, result), the arrays kept alive)"""
    out = np.ascontiguousarray(out, np.uint32)
    rres = np.ascontiguousarray(rollout_result, np.uint32).reshape(-1)
    delta = np.ascontiguousarray(delta, np.float32)
    table = np.ascontiguousarray(table, np.uint16).reshape(-1)
    T_e = spec.steps_e
    K = len(out)
    if out.ndim != 2 or out.shape[1] != 8 or K == 0 or rres.shape != (8,) or delta.size != 4 * K * T_e or \
            len(table) != spec.table_len:
        raise TypeError("out (K, 8), rollout_result (8,), delta (K, 4) or (K, steps, 4), table (table_len,) uint16")
    if nominal is not None:
        nominal = np.ascontiguousarray(nominal, np.float32)
        if nominal.size != 4 * T_e:
            raise TypeError("nominal must be (steps_e, 4) float32")
    weights = np.zeros(K, np.uint32)
    sums = np.zeros((T_e, 8), np.uint32)
    nout = np.zeros((T_e, 4), np.float32)
    result = np.zeros(8, np.uint32)
    args = (out.ctypes.data, rres.ctypes.data, delta.ctypes.data, table.ctypes.data,
            0 if nominal is None else nominal.ctypes.data, K, weights.ctypes.data, sums.ctypes.data, nout.ctypes.data,
            result.ctypes.data)
    return args, (weights, sums, nout, result), (out, rres, delta, table, nominal)


def mppi_update_host(spec: Mppi, out, rollout_result, delta, table, nominal=None):
    """Host only: E28 A's rules for one group by the library's own rplgpu_mppi_update_host (no handle, no device);
    arguments and results as ``RplGpu.mppi_update``."""
    a = _mppi_update_args(spec, out, rollout_result, delta, table, nominal)
    rc = load_library().rplgpu_mppi_update_host(C.byref(spec), *a[0])
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_mppi_update_host")
    return a[1]


def _mppi_spread_args(nominal, noise, shift, keep_first):
    nominal = np.ascontiguousarray(nominal, np.float32).reshape(-1, 4)
    noise = np.ascontiguousarray(noise, np.float32)
    if noise.ndim != 3 or noise.shape[2] != 4 or noise.size == 0 or len(nominal) == 0:
        raise TypeError("nominal (T_n, 4) and noise (K, T, 4) float32")
    K, T = noise.shape[:2]
    out = np.zeros((K, T, 4), np.float32)
    return (nominal.ctypes.data, len(nominal), noise.ctypes.data, K, T, shift, keep_first, out.ctypes.data), out, \
        (nominal, noise)


def mppi_spread_host(nominal, noise, shift: int = 0, keep_first: int = 0) -> np.ndarray:
    """Host only: E28 B's rule for one group by the library's own rplgpu_mppi_spread_host; arguments and result as
    ``RplGpu.mppi_spread``."""
    a = _mppi_spread_args(nominal, noise, shift, keep_first)
    rc = load_library().rplgpu_mppi_spread_host(*a[0])
    if rc != OK:
        raise RplGpuError(rc, "rplgpu_mppi_spread_host")
    return a[1]
