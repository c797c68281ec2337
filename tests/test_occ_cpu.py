"""E11 without a device: rplgpu_occ_grid_check and the message layout of include/rplgpu_msg.h against
tests/occ_oracle.py, the oracle's two walks against each other and against hand-made known answers of the
Bresenham rule, one hand-made serialised message, and the regime of every input of tests/test_gpu_occ.py."""
import struct

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import occ_cases as oc
from tests import occ_oracle as oo

F32 = np.float32
SYMBOLS = ("rplgpu_default_occ_grid", "rplgpu_occ_grid_check", "rplgpu_occupancy_grid_dev", "rplgpu_occupancy_grid",
           "rplgpu_msg_occupancy_layout", "rplgpu_occupancy_grid_msgs_dev")


def test_symbols_exported():
    lib = abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in abi.ABI_SYMBOLS
    assert abi.MAX_OCC_DIM == 4096 and abi.MAX_OCC_STEPS == 8192
    assert lib.rplgpu_abi_version() == 1


def _grid(**kw):
    s = oo.spec(**kw)
    return s, abi.OccGrid(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["range_min"],
                          s["obstacle_max"], s["raytrace_max"])


def test_default_grid():
    g = abi.OccGrid.defaults()
    s = oo.spec()
    for k in s:
        assert F32(getattr(g, k)) == F32(s[k]), k
    assert oo.spec_valid(s)
    abi.occ_grid_check(g)
    assert abi.load_library().rplgpu_occ_grid_check(None) == abi.ERR_INVALID_ARG


BAD = [
    dict(origin_x=float("nan")), dict(origin_y=float("inf")), dict(resolution=float("nan")),
    dict(range_min=float("nan")), dict(obstacle_max=float("inf")), dict(raytrace_max=float("inf")),
    dict(resolution=0.0), dict(resolution=-0.05),
    dict(width=0), dict(height=0), dict(width=4097), dict(height=4097),
    dict(range_min=-0.1), dict(range_min=25.0), dict(range_min=26.0), dict(obstacle_max=30.5),
    dict(resolution=1.0, obstacle_max=100.0, raytrace_max=8193.0),   # one step above the cap
    dict(raytrace_max=409.65),                                       # 0.05 m cells: 8193 steps
]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_invalid_grids_are_refused(bad):
    s, g = _grid(**bad)
    assert not oo.spec_valid(s)
    with pytest.raises(abi.RplGpuError) as e:
        abi.occ_grid_check(g)
    assert e.value.code == abi.ERR_INVALID_ARG


def test_boundary_grids_are_accepted():
    for kw in (dict(resolution=1.0, obstacle_max=100.0, raytrace_max=8192.0),  # exactly at the cap
               dict(width=4096, height=4096), dict(width=1, height=1),
               dict(obstacle_max=30.0), dict(range_min=0.0, obstacle_max=1e-3, raytrace_max=1e-3)):
        s, g = _grid(**kw)
        assert oo.spec_valid(s), kw
        abi.occ_grid_check(g)


@pytest.mark.parametrize("fid_len", [0, 1, 3, 4, 7])
@pytest.mark.parametrize("wh", [(1, 1), (3, 5), (257, 203)])
def test_layout_matches_restatement(fid_len, wh):
    w, h = wh
    lay = abi.msg_occupancy_layout(fid_len, w, h)
    off = {}
    msg = oo.occupancy_msg("f" * fid_len, 1, 2, 0.05, w, h, 0.0, 0.0, np.zeros(w * h, np.int8), off)
    for k, v in off.items():
        assert getattr(lay, k) == v, k
    assert lay.total_len == len(msg) and lay.data_off % 4 == 0 and (lay.origin_off - 4) % 8 == 0


def test_message_known_answer():
    """frame "ab", stamp (7, 9), 2 x 1 cells of 0.5 m at (-1, 2), data (100, -1): every byte by hand."""
    want = bytes([0, 1, 0, 0])                       # encapsulation: CDR little endian
    want += struct.pack("<iI", 7, 9)                 # header.stamp
    want += struct.pack("<I", 3) + b"ab\x00"         # frame_id: length with the NUL -> offset 19
    want += b"\x00"                                  # pad to 4 (counted from byte 4)
    want += struct.pack("<iI", 7, 9)                 # info.map_load_time
    want += struct.pack("<fII", 0.5, 2, 1)           # resolution, width, height -> offset 40: (40 - 4) % 8 = 4
    want += b"\x00" * 4                              # pad to 8
    want += struct.pack("<7d", -1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    want += struct.pack("<I", 2) + bytes([100, 255])
    assert oo.occupancy_msg("ab", 7, 9, 0.5, 2, 1, -1.0, 2.0, np.array([100, -1], np.int8)) == want
    lay = abi.msg_occupancy_layout(2, 2, 1)
    assert (lay.map_load_time_off, lay.resolution_off, lay.origin_off, lay.data_len_off, lay.data_off,
            lay.total_len) == (20, 28, 44, 100, 104, 106)


@pytest.mark.parametrize("dd", list(oc.KNOWN_RAYS), ids=[f"{a},{b}" for a, b in oc.KNOWN_RAYS])
def test_bresenham_known_answers(dd):
    cells = oc.KNOWN_RAYS[dd]
    for x0, y0 in ((0, 0), (8, 8), (-5, 3)):
        want = [(x0 + cx, y0 + cy) for cx, cy in cells]
        assert oo.walk_cells(x0, y0, x0 + dd[0], y0 + dd[1]) == want
    # both walks, as grids: everything but the end cell cleared, the end cell marked
    x0, y0 = oc.SMALL_SENSOR
    args = (np.array([x0]), np.array([y0]), np.array([x0 + dd[0]]), np.array([y0 + dd[1]]), np.array([False]),
            np.array([True]), 16, 16)
    for f in (oo.bits_python, oo.bits_vector):
        assert np.array_equal(oo.compose(*f(*args)), oc.known_grid(dd))
    if dd == (0, 0):
        assert (oc.known_grid(dd) == 0).sum() == 0 and (oc.known_grid(dd) == 100).sum() == 1
    # a cut ray clears its end cell too and marks nothing
    cut = list(args)
    cut[4], cut[5] = np.array([True]), np.array([False])
    for f in (oo.bits_python, oo.bits_vector):
        g = oo.compose(*f(*cut))
        assert (g == 100).sum() == 0 and (g == 0).sum() == len(cells)


def test_both_walks_agree_on_random_rays():
    rng = np.random.default_rng(11)
    n, W, H = 2000, 96, 80
    x0, y0 = rng.integers(-20, W + 20, n), rng.integers(-20, H + 20, n)
    x1, y1 = x0 + rng.integers(-70, 71, n), y0 + rng.integers(-70, 71, n)
    x1[:50], y1[:50] = x0[:50], y0[:50]          # zero length
    x1[50:100] = x0[50:100]                      # vertical
    y1[100:150] = y0[100:150]                    # horizontal
    cut = rng.random(n) < 0.3
    mark = ~cut & (rng.random(n) < 0.7)
    a = oo.bits_python(x0, y0, x1, y1, cut, mark, W, H)
    b = oo.bits_vector(x0, y0, x1, y1, cut, mark, W, H)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].sum() > 1000 and a[1].sum() > 100 and (a[0] & a[1]).sum() > 10


def test_cell_rule_and_cut():
    s = oo.spec(origin_x=-1.0, origin_y=0.0, resolution=0.5, width=8, height=8, range_min=0.5, obstacle_max=2.0,
                raytrace_max=3.0)
    has, cx, cy = oo.cells_of([-1.0, -1.25, 0.49, float("nan"), 6e5, 1.0], [0.0, -0.01, 0.5, 0.0, 0.0, -6e5], s)
    assert has.tolist() == [True, True, True, False, False, False]
    assert cx[:3].tolist() == [0, -1, 2] and cy[:3].tolist() == [0, -1, 1]
    x = np.array([0.25, 1.5, 2.5, 6.0, float("nan")], F32)
    r = oo.rays_of(x, np.zeros(5, F32), np.zeros(5, F32), np.zeros(5, F32), s)
    assert r["ray"].tolist() == [False, True, True, True, False]
    assert r["mark"].tolist() == [False, True, False, False, False]
    assert r["cut"].tolist() == [False, False, False, True, False]
    assert r["x1"][1:4].tolist() == [5, 7, 8] and not r["dropped"].any()  # 6 m cut at 3 m: u = 8


# ---- the regimes of the GPU inputs, worked out here ------------------------------------------------------------
def test_regime_small(oracle):
    oc.small_regime(oracle, oc.small_case(oracle))


def test_regime_edges(oracle):
    oc.edges_regime(oracle, oc.edges_case())


def test_regime_ranges(oracle):
    oc.ranges_regime(oracle, oc.ranges_case())


def test_regime_wall(oracle):
    oc.wall_regime(oracle, oc.wall_case())


def test_regime_cell_range(oracle):
    oc.cell_range_regime(oracle, oc.cell_range_case())


def test_regime_full(oracle):
    case = oc.full_case()
    oc.full_regime(oracle, case, oc.case_want(oracle, case, "full0"))


def test_regime_far(oracle):
    sides = oc.far_regime(oracle, oc.far_case())
    print(sides)


def test_regime_flush(oracle):
    pairs = oc.flush_regime(oracle, {W: oc.flush_case(W) for W in oc.FLUSH_WIDTHS})
    assert len(pairs) == 16


@pytest.mark.parametrize("outside", [False, True], ids=["inside", "outside"])
@pytest.mark.parametrize("wh", oc.TINY_GRIDS, ids=[f"{w}x{h}" for w, h in oc.TINY_GRIDS])
def test_regime_tiny(oracle, wh, outside):
    assert oc.tiny_regime(oracle, oc.tiny_case(*wh, outside)) == (not outside)


def test_regime_long(oracle):
    cases = oc.long_cases()
    oc.long_regime(oracle, cases)
    for case in cases:  # what the library's own check says of these specs
        s = case["spec"]
        abi.occ_grid_check(abi.OccGrid(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"],
                                       s["range_min"], s["obstacle_max"], s["raytrace_max"]))


def test_regime_ragged(oracle):
    case = oc.ragged_case()
    assert list(case["lens"][:8]) == [0, 1, 129, 1501, 2047, 2048, 2049, 4096] and case["lens"][8] == 0
    assert case["batch"].shape == (11, 4096) and case["group"] == 8
    oc.ragged_regime(oracle, case)


def test_message_grids_sit_on_the_intended_sides_of_the_launch_geometry():
    """tests/test_gpu_occ.py's message grids against k_msg_occupancy's kChunk words per workgroup and step and
    its cap of workgroups per message, both read from the source: one grid needs two workgroups and one trip,
    the other a second trip of the grid-stride loop and has three tail bytes."""
    chunk, most = oc.msg_kernel_constants()
    (w0, h0), (w1, h1) = oc.MSG_GRIDS
    assert chunk < (w0 * h0) // 4 <= 2 * chunk and 2 <= most
    assert most * chunk < (w1 * h1) // 4 <= 2 * most * chunk and (w1 * h1) % 4 == 3
    assert (257 * 203) // 4 <= chunk  # the grid of test_messages_match_restatement: one workgroup
    assert max(w0, h0, w1, h1) <= abi.MAX_OCC_DIM


def test_host_mirror_compiles_against_a_ros_shaped_occupancy_grid(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    tu = tmp_path / "check_occ.cpp"
    tu.write_text(r"""
#include <cstdint>
#include <vector>
#include "rplgpu_host.hpp"
namespace geometry_msgs { namespace msg {
struct Point { double x, y, z; };
struct Quaternion { double x, y, z, w; };
struct Pose { Point position; Quaternion orientation; };
}}
namespace nav_msgs { namespace msg {
struct MapMetaData { float resolution; uint32_t width, height; geometry_msgs::msg::Pose origin; };
struct OccupancyGrid { MapMetaData info; std::vector<int8_t> data; };
}}
struct __attribute__((packed)) sdk_node { uint16_t angle_z_q14; uint32_t dist_mm_q2; uint8_t quality, flag; };
bool use(rplgpu_host::ScanPath &p, const std::vector<std::vector<sdk_node>> &scans, const float *pose2d) {
  nav_msgs::msg::OccupancyGrid grid_msg;
  rplgpu_occ_grid_t g;
  rplgpu_default_occ_grid(&g);
  uint32_t cells[3], status;
  return p.configure(0, 8192, 8) &&
         p.fill_occupancy_grid(scans, rplgpu_host::ScanConfig(), g, pose2d, nullptr, nullptr, grid_msg) &&
         p.fill_occupancy_grid(scans, rplgpu_host::ScanConfig(), g, pose2d, nullptr, nullptr, grid_msg, cells, &status);
}
""")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{root / 'include'}",
           f"-I{root / 'rplidar_ros2_driver_amd' / 'host'}", str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
