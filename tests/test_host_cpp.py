"""The C++ host mirror (rplidar_ros2_driver_amd/host/rplgpu_host.hpp): it must compile against
ROS-shaped message types (CPU, no GPU), and — on a GPU box — the self-test binary that drives
it like the patched node would must reproduce the oracle byte for byte."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import NODE_DTYPE, Params
from tests import oracle_lib
from tests.cases import CASES

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "rplidar_ros2_driver_amd" / "host"

CHECK_TU = r"""
#include <cstdint>
#include <string>
#include <vector>
#include "sensor_msgs/msg/laser_scan.hpp"   // stand-in with the real field names (oracle/stubs)
#include "rplgpu_host.hpp"
namespace sensor_msgs { namespace msg {
struct PointField { std::string name; uint32_t offset; uint8_t datatype; uint32_t count; };
struct PointCloud2 { uint32_t height, width; std::vector<PointField> fields; bool is_bigendian;
                     uint32_t point_step, row_step; std::vector<uint8_t> data; bool is_dense; };
}}
struct __attribute__((packed)) sdk_node { uint16_t angle_z_q14; uint32_t dist_mm_q2; uint8_t quality, flag; };
struct Listener {  // shape of sl::internal::LIDARSampleDataListener (dataunpacker.h:48-60)
  void onHQNodeScanResetReq() {}
  void onHQNodeDecoded(unsigned long long, const rplgpu_node_t *) {}
};
bool replay(rplgpu_host::ScanPath &p, const std::vector<uint8_t> &bytes) {
  Listener l;
  int32_t state[4] = {0, 0, 0, 0};
  auto on_scan = [](std::vector<rplgpu_node_t> &) {};
  rplgpu_host::ScanAssembler<decltype(on_scan)> a(on_scan);
  return p.replay_recording(0x85, 125, bytes.data(), bytes.size(), l, state) &&
         p.replay_recording(0x82, 125, bytes.data(), bytes.size(), a, state);
}
struct rcl_like { uint8_t *buffer; size_t buffer_length, buffer_capacity; };
struct SerializedMessage {  // shape of rclcpp::SerializedMessage
  void reserve(size_t) {}
  rcl_like &get_rcl_serialized_message() { return raw; }
  rcl_like raw;
};
bool serialized(rplgpu_host::ScanPath &p, std::vector<sdk_node> &nodes) {
  SerializedMessage m;
  rplgpu_host::ScanConfig cfg;
  return p.fill_serialized_laser_scan(nodes, cfg, 0.1, "laser", 1, 2u, m) &&
         p.fill_serialized_point_cloud2(nodes, cfg, "laser", 1, 2u, m);
}
bool use(rplgpu_host::ScanPath &p, std::vector<sdk_node> &nodes) {
  sensor_msgs::msg::LaserScan scan_msg;
  sensor_msgs::msg::PointCloud2 cloud;
  rplgpu_host::ScanConfig cfg;
  uint32_t r = p.ascendScanData(nodes.data(), nodes.size());
  return r == 0 && p.fill_laser_scan(nodes, cfg, 0.1, scan_msg) && p.fill_point_cloud2(nodes, cfg, cloud);
}
"""


def test_host_header_compiles_against_ros_shaped_messages(tmp_path):
    tu = tmp_path / "check.cpp"
    tu.write_text(CHECK_TU)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
           f"-I{ROOT / 'include'}", f"-I{HOST}", f"-I{ROOT / 'oracle' / 'stubs'}", str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pose_rules_unit_is_plain_cpp(tmp_path):
    """csrc/rplgpu_pose_rules.cpp (the host twins, checks and tables of E15 - E23) and the stand-alone program that
    drives it build with the system g++ from those two files alone, warning-free, and the program accepts every
    call it should (no sanitizer here: tools/dev/pose_rules_asan.cpp's header has that recipe)."""
    rules = ROOT / "rplidar_ros2_driver_amd" / "csrc" / "rplgpu_pose_rules.cpp"
    text = rules.read_text()
    assert "hip/hip_runtime" not in text and "rpl_launch.hpp" not in text
    exe = tmp_path / "pose_rules"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
           f"-I{ROOT / 'include'}", f"-I{rules.parent}", str(rules),
           str(ROOT / "tools" / "dev" / "pose_rules_asan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def _build_selftest():
    r = subprocess.run(["make", "-C", str(HOST)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return HOST / "host_selftest"


@pytest.mark.gpu
def test_host_selftest_dummy_scans():
    exe = _build_selftest()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("360 beams") == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c1_like_360", "ring_8192_rot_jit", "kat2", "all_invalid",
                                  "c2_32000", "lead_trail_runs"])
@pytest.mark.parametrize("mode", [(0, 0, 1), (1, 1, 1), (0, 1, 0)])
def test_host_selftest_matches_oracle(tmp_path, oracle, name, mode):
    """grab_scan_data-style ascend (S1) -> publish_scan body (S3) -> PointCloud2, through the
    C++ host mirror, against the oracle on the same bytes."""
    is_new, inverted, scan_processing = mode
    exe = _build_selftest()
    nodes = CASES[name]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    nodes.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout), str(is_new), str(inverted),
                        str(scan_processing), "1", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = fout.read_bytes()
    pub, = struct.unpack_from("<I", buf, 0)
    meta = struct.unpack_from("<7f", buf, 4)
    count, = struct.unpack_from("<I", buf, 32)
    off = 36
    ranges = np.frombuffer(buf, np.float32, count, off); off += 4 * count
    intens = np.frombuffer(buf, np.float32, count, off); off += 4 * count
    sl_result, npts = struct.unpack_from("<II", buf, off); off += 8
    cloud = np.frombuffer(buf, np.float32, 4 * npts, off).reshape(npts, 4); off += 16 * npts
    asc = np.frombuffer(buf, NODE_DTYPE, len(nodes), off)

    want_asc, want_res = oracle.ascend(nodes)
    assert sl_result == want_res
    fed = want_asc if want_res == 0 else nodes
    assert oracle_lib.canon_equal_angle_runs(asc).tobytes() == \
        oracle_lib.canon_equal_angle_runs(fed).tobytes()
    p = Params.defaults(is_new_protocol=is_new, inverted=inverted,
                        scan_processing=scan_processing, range_max=40.0)
    # feed the oracle the very bytes the device path saw after S1
    wr, wi, wm = oracle.publish_scan(asc, oracle_lib.copy_params(p), 0.125)
    assert pub == wm.published and count == wm.count
    if pub:
        assert np.array(meta, np.float32).tobytes() == \
            np.array(wm.as_tuple()[:7], np.float32).tobytes()
        v = asc[asc["dist_mm_q2"] != 0]
        unique = len(np.unique(v["angle_z_q14"])) == len(v)
        if unique:
            assert ranges.tobytes() == wr.tobytes() and intens.tobytes() == wi.tobytes()
        elif scan_processing:
            assert ranges.tobytes() == wr.tobytes()  # Mode A ranges never depend on tie order
        else:  # Mode B with equal angles: the order inside a run is std::sort's (unstable)
            assert sorted(zip(ranges.tolist(), intens.tolist())) == \
                sorted(zip(wr.tolist(), wi.tolist()))
    pv = Params.defaults(is_new_protocol=is_new, inverted=inverted, clip_enable=1,
                         range_max=40.0, voxel_enable=1)
    wc, _, _ = oracle.cloud_pipeline(asc, oracle_lib.copy_params(pv))
    assert npts == len(wc)
    if npts:
        assert np.max(np.abs(cloud[:, :2].astype(np.float64) - wc[:, :2])) <= 1e-6
        assert cloud[:, 3].tobytes() == wc[:, 3].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c1_like_360", "ring_8192", "all_invalid", "c2_32000"])
@pytest.mark.parametrize("mode", [(0, 0, 1), (1, 1, 0)])
def test_host_selftest_serialized_messages(tmp_path, oracle, name, mode):
    """publish_scan ending in publish(SerializedMessage): the C++ host mirror must hand back the
    exact CDR bytes of the oracle's LaserScan / voxelised PointCloud2 for the same nodes."""
    import sys
    sys.path.insert(0, str(ROOT / "oracle"))
    import cdr_oracle as cdr
    is_new, inverted, scan_processing = mode
    exe = _build_selftest()
    nodes = CASES[name]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    nodes.tofile(fin)
    r = subprocess.run([str(exe), "serialized", str(fin), str(fout), str(is_new), str(inverted),
                        str(scan_processing), "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = fout.read_bytes()
    pub, la = struct.unpack_from("<II", buf, 0)
    scan_bytes = buf[8: 8 + la]
    lc, = struct.unpack_from("<I", buf, 8 + la)
    cloud_bytes = buf[12 + la: 12 + la + lc]
    p = Params.defaults(is_new_protocol=is_new, inverted=inverted,
                        scan_processing=scan_processing, range_max=40.0)
    wr, wi, wm = oracle.publish_scan(nodes, oracle_lib.copy_params(p), 0.125)
    assert pub == wm.published
    if pub:  # these cases have unique angles: the oracle's arrays are the only right answer
        assert scan_bytes == cdr.laserscan_msg("laser_frame", 1727000000, 123456789, wm, wr, wi)
    else:
        assert la == 0
    pv = Params.defaults(is_new_protocol=is_new, inverted=inverted, clip_enable=1,
                         range_max=40.0, voxel_enable=1)
    want, _, _ = oracle.cloud_pipeline(nodes, oracle_lib.copy_params(pv))
    back = cdr.deserialize("PointCloud2", cloud_bytes)
    assert back["header"] == {"stamp": {"sec": 1727000000, "nanosec": 123456789},
                              "frame_id": "laser_frame"}
    assert back["width"] == len(want) and back["height"] == 1 and back["is_dense"]
    got = back["data"].view(np.float32).reshape(-1, 4)
    if len(want):
        assert np.max(np.abs(got[:, :3].astype(np.float64) - want[:, :3])) <= 1e-6
        assert got[:, 3].tobytes() == want[:, 3].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("ans", [0x82, 0x84, 0x85, 0x86, 0x83, 0x81])
def test_host_replay_recording_matches_oracle(tmp_path, oracle, ans):
    """replay_recording + ScanAssembler (the C++ mirror of the SDK listener / ScanDataHolder)
    on a corrupted recording: same callbacks in the same order as the oracle's unpacker, same
    completed scans as the oracle's scan assembly."""
    from rplidar_ros2_driver_amd import capsules as cp
    exe = _build_selftest()
    data = cp.make_stream(ans, 260 if ans != 0x81 else 4000, 5, corrupt=True, payload="ring",
                          frames_per_rev=41.0)
    fin, fout = tmp_path / "stream.bin", tmp_path / "out.bin"
    data.tofile(fin)
    r = subprocess.run([str(exe), "replay", hex(ans), "125", str(fin), str(fout)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = fout.read_bytes()
    n_nodes, n_rst, n_err, n_scans = struct.unpack_from("<4I", buf, 0)
    off = 16
    nodes = np.frombuffer(buf, NODE_DTYPE, n_nodes, off); off += 8 * n_nodes
    rst = np.frombuffer(buf, np.uint32, n_rst, off); off += 4 * n_rst
    w_nodes, w_rst, w_err, _ = oracle.unpack(ans, data, 125)
    assert nodes.tobytes() == w_nodes.tobytes() and list(rst) == list(w_rst) and n_err == w_err
    w_scans, w_off = oracle.segment(w_nodes, w_rst, 8192)
    assert n_scans == len(w_off) - 1
    for sidx in range(n_scans):
        ln, = struct.unpack_from("<I", buf, off); off += 4
        scan = np.frombuffer(buf, NODE_DTYPE, ln, off); off += 8 * ln
        assert scan.tobytes() == w_scans[w_off[sidx]: w_off[sidx + 1]].tobytes()
