"""E9 on the device: rplgpu_merge_scans_dev against tests/merge_oracle.py bit for bit (ranges,
intensities, beams hit), the serialised messages of rplgpu_merged_laserscan_msgs_dev against
oracle/cdr_oracle.py, argument errors, and the E8 grid next to an interleaved merge."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import merge_oracle as mo

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import cdr_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _spec(count, angle_min=-math.pi, angle_max=math.pi, range_min=0.0, range_max=40.0, scan_time=0.1):
    d = dict(angle_min=angle_min, angle_max=angle_max, count=count, range_min=range_min, range_max=range_max,
             scan_time=scan_time)
    return d, abi.ScanMerge(angle_min, angle_max, count, range_min, range_max, scan_time)


def _poses(rng, B):
    ang = rng.uniform(-3, 3, B)
    return np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, B), np.sin(ang), np.cos(ang),
                     rng.uniform(-2, 2, B)], 1).astype(np.float32)


def _motion(rng, B, n):
    return np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                     for _ in range(B)]).astype(np.float32)


def _run(gpu, batch, group, p, spec_struct, motion=None, pose2d=None, t0=None, lens=None):
    """batch (B, n) NODE_DTYPE -> (ranges (G, count), intensities, beams hit (G,), status (G,))."""
    import torch
    dev = torch.device("cuda:0")
    B, n = batch.shape
    G = (B + min(group, B) - 1) // min(group, B)
    count = spec_struct.count
    d_nodes = torch.from_numpy(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = (torch.full((B,), n, dtype=torch.int32, device=dev) if lens is None
             else torch.from_numpy(np.asarray(lens, np.int32)).to(dev))
    d_mo = torch.from_numpy(motion).to(dev) if motion is not None else None
    d_po = torch.from_numpy(pose2d).to(dev) if pose2d is not None else None
    d_t0 = torch.from_numpy(t0).to(dev) if t0 is not None else None
    d_r = torch.full((G * count,), 7.0, dtype=torch.float32, device=dev)
    d_i = torch.full((G * count,), 7.0, dtype=torch.float32, device=dev)
    d_hit = torch.full((G,), 12345, dtype=torch.int32, device=dev)
    d_st = torch.full((G,), 99, dtype=torch.int32, device=dev)
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr() if d_t0 is not None else 0)
    try:
        gpu.merge_scans_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, group, p,
                            d_mo.data_ptr() if d_mo is not None else 0, d_po.data_ptr() if d_po is not None else 0,
                            spec_struct, d_r.data_ptr(), d_i.data_ptr(), d_hit.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    return (d_r.cpu().numpy().reshape(G, count), d_i.cpu().numpy().reshape(G, count),
            d_hit.cpu().numpy().astype(np.int64), d_st.cpu().numpy())


def _check(oracle, gpu, batch, group, p, spec, motion=None, pose2d=None, t0=None, groups=None):
    sd, ss = spec
    r, i, hit, st = _run(gpu, batch, group, p, ss, motion, pose2d, t0)
    B = len(batch)
    group = min(group, B)
    for g in (range(len(r)) if groups is None else groups):
        sl = slice(g * group, min(B, (g + 1) * group))
        wr, wi, wh = mo.merge_group(oracle, list(batch[sl]), p, sd,
                                    None if motion is None else motion[sl], None if pose2d is None else pose2d[sl],
                                    None if t0 is None else t0[sl])
        assert r[g].tobytes() == wr.tobytes(), (g, np.flatnonzero(r[g].view(np.uint32) != wr.view(np.uint32))[:8])
        assert i[g].tobytes() == wi.tobytes(), g
        assert hit[g] == wh, g
        assert st[g] == 0, g
    return r, i, hit


def test_one_sensor_identity(gpu, oracle):
    batch = np.stack([synth.make_scan(900, 0, 8000, noise_m=0.01)])
    p = Params.defaults(clip_enable=1, q_min=8, range_min=0.15, range_max=40.0)
    r, _, hit = _check(oracle, gpu, batch, 1, p, _spec(1440))
    assert 0 < hit[0] <= 1440 and np.isinf(r[0]).sum() == 1440 - hit[0]


@pytest.mark.parametrize("group", [2, 8])
@pytest.mark.parametrize("deskew", ["none", "motion", "motion_t0"])
def test_sensors_with_poses(gpu, oracle, group, deskew):
    n, G = 6000, 2
    B = group * G
    batch = synth.make_batch(910 + group, B, n, noise_m=0.01, r0_range=(1.0, 12.0))
    rng = np.random.default_rng(group)
    pose2d = _poses(rng, B)
    motion = _motion(rng, B, n) if deskew != "none" else None
    t0 = rng.uniform(-0.05, 0.05, B).astype(np.float32) if deskew == "motion_t0" else None
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    _check(oracle, gpu, batch, group, p, _spec(1440), motion, pose2d, t0)


@pytest.mark.parametrize("ror,clip,inverted,proto", [(1, 1, 0, 0), (1, 0, 1, 1), (0, 0, 0, 1), (0, 1, 1, 0)])
def test_filters_and_inversion(gpu, oracle, ror, clip, inverted, proto):
    n, group = 5000, 4
    batch = np.stack([synth.make_scan(920, b, n, noise_m=0.02, invalid_p=0.2, new_protocol=bool(proto),
                                      kind="uniform" if b == 1 else "ring") for b in range(group)])
    rng = np.random.default_rng(7)
    p = Params.defaults(clip_enable=clip, q_min=40, range_min=0.5, range_max=30.0, inverted=inverted,
                        is_new_protocol=proto, ror_enable=ror, ror_radius=0.10, ror_min_neighbors=2,
                        voxel_enable=1, voxel_leaf=0.05, scan_processing=0)  # (the last three: ignored)
    _check(oracle, gpu, batch, group, p, _spec(720, range_min=0.3, range_max=25.0), _motion(rng, group, n),
           _poses(rng, group))


@pytest.mark.parametrize("spec", [
    dict(count=720, angle_min=-math.pi / 2, angle_max=math.pi / 2),
    dict(count=360), dict(count=1440), dict(count=16384),
    dict(count=720, angle_min=0.0, angle_max=2 * math.pi),
    dict(count=1, angle_min=0.2, angle_max=0.2 + math.pi / 2),
    dict(count=100, angle_min=0.785, angle_max=0.785 + 1e-6),  # rounded edges that repeat: the linear fallback
], ids=["front180", "c360", "c1440", "c16384", "from0", "one_beam", "degenerate"])
def test_windows_and_beam_counts(gpu, oracle, spec):
    n, group = 7000, 3
    batch = synth.make_batch(930, group, n, noise_m=0.01, r0_range=(1.0, 12.0))
    if spec["count"] == 100:
        batch = batch[:, :1500]  # (the linear fallback: keep it small)
    rng = np.random.default_rng(3)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    kw = dict(spec)
    count = kw.pop("count")
    _check(oracle, gpu, batch, group, p, _spec(count, **kw), None, _poses(rng, group) if count != 100 else None)


def _nodes(q14, dist, quality):
    nd = np.zeros(len(q14), abi.NODE_DTYPE)
    nd["angle_z_q14"], nd["dist_mm_q2"], nd["quality"] = q14, dist, quality
    return nd


def test_constructed_points_edges_wrap_origin_ties(gpu, oracle):
    # angle 0 -> (cos, sin) = (1, 0) exactly: points on the +x axis lie ON e_0 of a spec from 0; with the
    # span a hair above 2 pi they also lie in the wrap sliver (beam count - 1 satisfies the rule too)
    amax = float(F32(2 * math.pi) * (1 + 2 ** -21))
    n = 64
    q = np.zeros(n, np.int64)
    q[8:16] = 16384  # 90 deg
    q[16:] = np.arange(n - 16) * 1024
    d = np.full(n, 8000, np.int64)  # 2 m
    d[1] = 12000
    d[2] = 8000  # a tie with sample 0 in r2: the first in acquisition order wins
    s0 = _nodes(q, d, (np.arange(n) * 4) % 256)
    s1 = s0.copy()
    s1["quality"] = 252  # the same points from a second sensor: every r2 ties, slot 0 wins
    s2 = _nodes(np.zeros(4, np.int64), np.full(4, 8000), [40, 40, 40, 40])  # moved to the origin by its pose
    batch = np.stack([s0, s1, np.concatenate([s2, np.zeros(n - 4, abi.NODE_DTYPE)])])
    pose2d = np.array([[1, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, 0], [1, 0, -2, 0, 1, 0]], np.float32)
    p = Params.defaults(clip_enable=0)
    sd, ss = _spec(1440, angle_min=0.0, angle_max=amax, range_min=0.0)
    r, i, hit = _check(oracle, gpu, batch, 3, p, (sd, ss), None, pose2d)
    assert r[0, 0] == F32(2.0) and i[0, 0] == F32(0.0)  # sample 0 of slot 0 (quality 0 >> 2)
    assert r[0, 1439] == np.inf


def test_empty_and_all_invalid_scans(gpu, oracle):
    n = 4096
    batch = synth.make_batch(940, 4, n)
    batch[1]["dist_mm_q2"] = 0
    batch[3]["dist_mm_q2"] = 0
    p = Params.defaults(clip_enable=1, range_min=0.15, range_max=40.0)
    sd, ss = _spec(360)
    r, i, hit, st = _run(gpu, batch, 2, p, ss, lens=[0, n, n, n])
    assert hit[0] == 0 and np.all(np.isinf(r[0])) and np.all(i[0] == 0)
    assert r[1].tobytes() == mo.merge_group(oracle, [batch[2], batch[3]], p, sd)[0].tobytes()
    assert hit.tolist()[1] > 0 and st.tolist() == [0, 0]


def test_c5_bench_scale(gpu, oracle):
    """8 sensors x 32 000 samples x 512 time steps, poses, motion and time offsets: every group bit for bit."""
    B, n, S = 4096, 32000, 8
    batch = synth.make_batch(2026 + 5, B, n, noise_m=0.01)
    rng = np.random.default_rng(2026)
    motion, pose2d = _motion(rng, B, n), _poses(rng, B)
    t0 = rng.uniform(-0.02, 0.02, B).astype(np.float32)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    _check(oracle, gpu, batch, S, p, _spec(1440), motion, pose2d, t0)


def test_messages_match_cdr_oracle(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    group, G, n = 4, 3, 3000
    batch = synth.make_batch(950, group * G, n)
    p = Params.defaults(clip_enable=1)
    sd, ss = _spec(500, angle_min=-2.0, angle_max=2.5, range_min=0.2, range_max=20.0, scan_time=0.125)
    r, i, _, _ = _run(gpu, batch, group, p, ss)
    frame = "base_link"
    lay = abi.LaserScanLayout()
    abi.load_library().rplgpu_msg_laserscan_layout(len(frame), 500, lay)
    stride = (lay.total_len + 3) & ~3
    stamps = np.array([(100 + g, 1000 * g) for g in range(G)], dtype=[("sec", "<i4"), ("nanosec", "<u4")])
    d_r = torch.from_numpy(r.reshape(-1).copy()).to(dev)
    d_i = torch.from_numpy(i.reshape(-1).copy()).to(dev)
    d_stamps = torch.from_numpy(stamps.view(np.uint8)).to(dev)
    inc = abi.scan_merge_edges(ss)[1]
    for slot_bytes in (stride, stride - 4):
        d_msgs = torch.zeros(G * slot_bytes, dtype=torch.uint8, device=dev)
        d_len = torch.full((G,), 77, dtype=torch.int32, device=dev)
        d_st = torch.zeros(G, dtype=torch.int32, device=dev)
        gpu.merged_laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), G, ss, frame, d_stamps.data_ptr(),
                                      d_msgs.data_ptr(), slot_bytes, d_len.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
        msgs, lens, st = d_msgs.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
        for g in range(G):
            if slot_bytes < lay.total_len:
                assert lens[g] == 0 and st[g] == abi.SCAN_OUT_TRUNCATED
                continue
            meta = dict(angle_min=F32(sd["angle_min"]), angle_max=F32(sd["angle_max"]), angle_increment=F32(inc),
                        time_increment=F32(0.0), scan_time=F32(0.125), range_min=F32(0.2), range_max=F32(20.0))
            want = cdr_oracle.laserscan_msg(frame, 100 + g, 1000 * g, meta, r[g], i[g])
            assert lens[g] == len(want) == lay.total_len
            assert msgs[g * slot_bytes: g * slot_bytes + lens[g]].tobytes() == want


def test_bad_arguments_leave_a_working_handle(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    n, B = 2000, 2
    batch = synth.make_batch(960, B, n)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    d_r = torch.zeros(B * 360, dtype=torch.float32, device=dev)
    d_i = torch.zeros(B * 360, dtype=torch.float32, device=dev)
    d_hit = torch.zeros(B, dtype=torch.int32, device=dev)
    d_t0 = torch.zeros(B, dtype=torch.float32, device=dev)
    p = Params.defaults(clip_enable=1)
    _, ss = _spec(360)
    host = np.zeros(B * 360, np.float32)

    def call(**kw):
        a = dict(nodes=d_nodes.data_ptr(), group=1, spec=ss, r=d_r.data_ptr(), hit=d_hit.data_ptr(), B=B)
        a.update(kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.merge_scans_dev(a["nodes"], n, d_len.data_ptr(), a["B"], a["group"], p, 0, 0, a["spec"], a["r"],
                                d_i.data_ptr(), a["hit"], 0)
        return e.value.code

    assert call(spec=abi.ScanMerge(0.0, 0.0, 360, 0.0, 1.0, 0.1)) == abi.ERR_INVALID_ARG
    assert call(spec=abi.ScanMerge(-1.0, 1.0, 0, 0.0, 1.0, 0.1)) == abi.ERR_INVALID_ARG
    assert call(group=0) == abi.ERR_INVALID_ARG
    assert call(nodes=0) == abi.ERR_INVALID_ARG
    assert call(r=0) == abi.ERR_INVALID_ARG
    assert call(r=host.ctypes.data) == abi.ERR_INVALID_ARG  # plain host memory
    assert call(B=gpu.max_batch + 1) == abi.ERR_CAPACITY
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        assert call() == abi.ERR_INVALID_ARG  # offsets set, d_motion NULL
    finally:
        gpu.set_scan_time_offsets_dev(0)
    with pytest.raises(abi.RplGpuError):
        gpu.merged_laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), 1, abi.ScanMerge(0.0, 0.0, 1, 0.0, 1.0, 0.1),
                                      "x", 0, 0, 0, 0)
    # the handle still works
    _check(oracle, gpu, batch, 1, p, _spec(360))


def test_fused_voxel_unchanged_by_an_interleaved_merge(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    n, group, G = 8000, 4, 2
    B = group * G
    batch = synth.make_batch(970, B, n, noise_m=0.01, r0_range=(2.0, 12.0))
    rng = np.random.default_rng(9)
    motion, pose2d = _motion(rng, B, n), _poses(rng, B)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, voxel_enable=1, voxel_leaf=0.05,
                        ror_enable=1, ror_radius=0.10, ror_min_neighbors=2)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    d_mo, d_po = torch.from_numpy(motion).to(dev), torch.from_numpy(pose2d).to(dev)

    def voxel():
        d_arena = torch.zeros(B * n, 4, dtype=torch.float32, device=dev)
        d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
        d_start = torch.zeros(G, dtype=torch.int64, device=dev)
        d_np = torch.zeros(G, dtype=torch.int32, device=dev)
        d_st = torch.zeros(G, dtype=torch.int32, device=dev)
        gpu.cloud_fused_voxel_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, group, p, d_mo.data_ptr(),
                                  d_po.data_ptr(), d_arena.data_ptr(), B * n, d_cur.data_ptr(), d_start.data_ptr(),
                                  d_np.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
        a, s, c = d_arena.cpu().numpy(), d_start.cpu().numpy(), d_np.cpu().numpy()
        return [a[s[g]: s[g] + c[g]].tobytes() for g in range(G)], d_st.cpu().numpy().tolist()

    before = voxel()
    _check(oracle, gpu, batch, group, p, _spec(1440), motion, pose2d)
    assert voxel() == before
