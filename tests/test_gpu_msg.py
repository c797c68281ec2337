"""GPU tests of the serialised-message stage (include/rplgpu_msg.h):
raw nodes -> publish-ready LaserScan / PointCloud2 bytes, single scan (DMA into the message)
and batches assembled on the device, against oracle publish_scan / cloud pipeline results
serialised by the independent restatement in oracle/cdr_oracle.py.  Byte-exact."""
import sys
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import oracle_lib
from tests.cases import CASES

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import cdr_oracle as cdr  # noqa: E402

pytestmark = pytest.mark.gpu

FID = "laser_frame"


def _unique_angles(nodes):
    v = nodes[nodes["dist_mm_q2"] != 0]
    return len(np.unique(v["angle_z_q14"])) == len(v)


@pytest.mark.parametrize("name", list(CASES))
def test_laserscan_msg_matches_oracle(gpu, oracle, name):
    nodes = CASES[name]
    for is_new, inverted, mode in [(0, 0, 1), (1, 1, 1), (0, 1, 0), (1, 0, 0)]:
        p = Params.defaults(is_new_protocol=is_new, inverted=inverted, scan_processing=mode,
                            range_max=40.0)
        wr, wi, wm = oracle.publish_scan(nodes, oracle_lib.copy_params(p), 0.125)
        msg, gm = gpu.scan_to_laserscan_msg(nodes, p, 0.125, FID, 1727000000, 123456789)
        assert bytes(gm) == bytes(wm)
        if not wm.published:
            assert len(msg) == 0  # publish_scan returns without publishing (:611-613)
            continue
        # the arrays inside the message are the arrays of the plain entry point ...
        gr, gi, _ = gpu.scan_to_laserscan(nodes, p, 0.125)
        assert msg.tobytes() == cdr.laserscan_msg(FID, 1727000000, 123456789, wm, gr, gi)
        # ... and the oracle's wherever upstream's unstable sort leaves no choice
        if _unique_angles(nodes):
            assert msg.tobytes() == cdr.laserscan_msg(FID, 1727000000, 123456789, wm, wr, wi)
        back = cdr.deserialize("LaserScan", msg.tobytes())
        assert len(back["ranges"]) == wm.count == len(back["intensities"])


def test_laserscan_msg_empty_and_capacity(gpu):
    p = Params.defaults()
    msg, m = gpu.scan_to_laserscan_msg(np.zeros(0, abi.NODE_DTYPE), p, 0.1, FID, 0, 0)
    assert len(msg) == 0 and not m.published  # :561-563
    nodes = CASES["c1_like_360"]
    small = np.zeros(abi.msg_laserscan_layout(len(FID), 359).total_len, np.uint8)
    with pytest.raises(abi.RplGpuError) as e:  # must hold the worst case count == n
        gpu.scan_to_laserscan_msg(nodes, p, 0.1, FID, 0, 0, out=small)
    assert e.value.code == abi.ERR_CAPACITY and not small.any()


@pytest.mark.parametrize("name", ["c1_like_360", "ring_8192_rot_jit", "c2_32000", "all_invalid"])
def test_cloud_msg_matches_oracle(gpu, oracle, name):
    nodes = CASES[name]
    for voxel in (0, 1):
        p = Params.defaults(clip_enable=1, range_max=40.0, voxel_enable=voxel, inverted=voxel)
        msg, npts, status = gpu.scan_to_cloud_msg(nodes, p, FID, 17, 42)
        xyzi, st2 = gpu.scan_to_cloud(nodes, p)
        assert status == st2 == 0 and npts == len(xyzi)
        assert msg.tobytes() == cdr.cloud_msg(FID, 17, 42, xyzi)
        if voxel:
            want, _, _ = oracle.cloud_pipeline(nodes, oracle_lib.copy_params(p))
        else:
            want = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p))
        back = cdr.deserialize("PointCloud2", msg.tobytes())
        assert back["width"] == len(want) and back["row_step"] == 16 * len(want)
        got = back["data"].view(np.float32).reshape(-1, 4)
        if len(want):
            assert np.max(np.abs(got[:, :3].astype(np.float64) - want[:, :3])) <= 1e-6
            assert got[:, 3].tobytes() == want[:, 3].tobytes()
    # an empty cloud is still a message (width 0)
    msg, npts, _ = gpu.scan_to_cloud_msg(np.zeros(0, abi.NODE_DTYPE), Params.defaults(), "", 0, 0)
    assert npts == 0 and msg.tobytes() == cdr.cloud_msg("", 0, 0, np.zeros((0, 4), np.float32))


def test_pinned_message_buffer(gpu, oracle):
    nodes = CASES["c2_32000"]
    p = Params.defaults(range_max=40.0)
    want, _ = gpu.scan_to_laserscan_msg(nodes, p, 0.1, FID, 5, 6)
    pin = gpu.host_alloc(abi.msg_cloud_layout(len(FID), len(nodes)).total_len + 5)
    try:
        pin[:] = 0xEE
        got, _ = gpu.scan_to_laserscan_msg(nodes, p, 0.1, FID, 5, 6, out=pin)
        assert got.tobytes() == want.tobytes()
        assert np.all(pin[len(got):][-5:] == 0xEE)
        # Mode A into a pinned buffer is ONE kernel that bins the scan and writes the message
        # around its arrays; any other buffer (and Mode B) takes the arrays through HBM and a
        # second kernel / copies: same bytes, every scan length class, and against the host
        # framing of the oracle's arrays
        for name in ("c1_like_360", "ring_8192_rot_jit", "all_invalid", "c2_32000"):
            sc = CASES[name]
            for kw in (dict(), dict(is_new_protocol=1, inverted=1), dict(scan_processing=0),
                       dict(clip_enable=1, q_min=20, range_max=12.0)):
                pp = Params.defaults(**{"range_max": 40.0, **kw})
                for cut in (len(sc), max(len(sc) - 1, 0), min(len(sc), 2049), min(len(sc), 700)):
                    part = sc[:cut]
                    a, ma = gpu.scan_to_laserscan_msg(part, pp, 0.0731, FID, -3, 999999999)
                    pin[:] = 0xEE
                    b, mb = gpu.scan_to_laserscan_msg(part, pp, 0.0731, FID, -3, 999999999, out=pin)
                    assert bytes(ma) == bytes(mb), (name, kw, cut)
                    assert a.tobytes() == b.tobytes(), (name, kw, cut)
                    if pp.scan_processing and len(part):
                        wr, wi, wm = oracle.publish_scan(part, oracle_lib.copy_params(pp), 0.0731)
                        assert bytes(mb) == bytes(wm)
                        if wm.published:
                            back = cdr.deserialize("LaserScan", b.tobytes())
                            assert back["ranges"].tobytes() == wr.tobytes(), (name, kw, cut)
        pv = Params.defaults(clip_enable=1, range_max=40.0, voxel_enable=1)
        wantc, n1, _ = gpu.scan_to_cloud_msg(nodes, pv, FID, 5, 6)
        gotc, n2, _ = gpu.scan_to_cloud_msg(nodes, pv, FID, 5, 6, out=pin)
        assert n1 == n2 and gotc.tobytes() == wantc.tobytes()
    finally:
        gpu.host_free(pin)


def _batch(torch, seed, B, n):
    batch = synth.make_batch(seed, B, n, jitter=2)
    lens = np.array([n - 17 * b for b in range(B)], np.uint32)
    lens[2] = 0
    dev = torch.device("cuda:0")
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    return batch, lens, d_nodes, d_len


@pytest.mark.parametrize("mode", [1, 0])
def test_laserscan_msgs_dev_matches_oracle(gpu, oracle, mode):
    import torch
    B, n = 20, 3000
    batch, lens, d_nodes, d_len = _batch(torch, 31 + mode, B, n)
    dev = d_nodes.device
    p = Params.defaults(range_max=40.0, scan_processing=mode, inverted=mode)
    d_r = torch.empty(B, n, dtype=torch.float32, device=dev)
    d_i = torch.empty(B, n, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    gpu.laserscan_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_r.data_ptr(),
                            d_i.data_ptr(), d_cnt.data_ptr())
    stamps = np.stack([np.arange(B) + 1_700_000_000, np.arange(B) * 37_000_001 % 10**9], 1)
    durs = 0.05 + 0.003 * np.arange(B)
    d_stamps = torch.from_numpy(stamps.astype(np.int32)).to(dev)
    d_dur = torch.from_numpy(durs).to(dev)
    stride = abi.msg_laserscan_layout(len(FID), n).total_len
    d_msgs = torch.full((B, stride), 0xEE, dtype=torch.uint8, device=dev)
    d_ml = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    gpu.laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), n, d_cnt.data_ptr(), B, p, FID,
                           d_stamps.data_ptr(), d_dur.data_ptr(), d_msgs.data_ptr(), stride,
                           d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    msgs, ml = d_msgs.cpu().numpy(), d_ml.cpu().numpy()
    r, i = d_r.cpu().numpy(), d_i.cpu().numpy()
    assert not d_st.cpu().numpy().any()
    for b in range(B):
        wr, wi, wm = oracle.publish_scan(batch[b, : lens[b]], oracle_lib.copy_params(p), durs[b])
        if not wm.published:
            assert ml[b] == 0 and np.all(msgs[b] == 0xEE)
            continue
        want = cdr.laserscan_msg(FID, int(stamps[b, 0]), int(stamps[b, 1]), wm,
                                 r[b, : wm.count], i[b, : wm.count])
        assert ml[b] == len(want)
        assert msgs[b, : ml[b]].tobytes() == want  # scalars computed on the device: bit-exact
        assert np.all(msgs[b, ml[b]:] == 0xEE)     # and nothing written past the message
        if mode:
            assert want == cdr.laserscan_msg(FID, int(stamps[b, 0]), int(stamps[b, 1]), wm, wr, wi)
    # a slot too small for some scans: those report length 0 + OUT_TRUNCATED, the rest are intact
    small = abi.msg_laserscan_layout(len(FID), int(np.sort(d_cnt.cpu().numpy())[B // 2])).total_len
    d_ml.fill_(-1)
    gpu.laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), n, d_cnt.data_ptr(), B, p, FID,
                           d_stamps.data_ptr(), d_dur.data_ptr(), d_msgs.data_ptr(), small,
                           d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    ml2, st = d_ml.cpu().numpy(), d_st.cpu().numpy()
    for b in range(B):
        fits = ml[b] <= small
        assert ml2[b] == (ml[b] if fits else 0)
        assert bool(st[b] & abi.SCAN_OUT_TRUNCATED) == (not fits)


def test_cloud_msgs_dev_from_regions_and_arena(gpu, oracle):
    import torch
    B, n = 20, 3000
    batch, lens, d_nodes, d_len = _batch(torch, 77, B, n)
    dev = d_nodes.device
    pv = Params.defaults(clip_enable=1, range_max=40.0, voxel_enable=1)
    out_stride = 3000
    d_xyzi = torch.zeros(B, out_stride, 4, dtype=torch.float32, device=dev)
    d_np = torch.zeros(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    gpu.cloud_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, pv, d_xyzi.data_ptr(),
                        out_stride, d_np.data_ptr(), d_st.data_ptr())
    stamps = np.stack([np.arange(B) - 3, np.arange(B) * 1001], 1)
    d_stamps = torch.from_numpy(stamps.astype(np.int32)).to(dev)
    stride = (abi.msg_cloud_layout(len(FID), out_stride).total_len + 3) & ~3
    d_msgs = torch.full((B, stride), 0xEE, dtype=torch.uint8, device=dev)
    d_ml = torch.full((B,), -1, dtype=torch.int32, device=dev)
    gpu.cloud_msgs_dev(d_xyzi.data_ptr(), out_stride, 0, d_np.data_ptr(), B, FID,
                       d_stamps.data_ptr(), d_msgs.data_ptr(), stride, d_ml.data_ptr(),
                       d_st.data_ptr())
    gpu.synchronize()
    assert not d_st.cpu().numpy().any()
    msgs, ml, npts = d_msgs.cpu().numpy(), d_ml.cpu().numpy(), d_np.cpu().numpy()
    xyzi = d_xyzi.cpu().numpy()
    for b in range(B):
        want_pts, _, _ = oracle.cloud_pipeline(batch[b, : lens[b]], oracle_lib.copy_params(pv))
        assert npts[b] == len(want_pts)
        want = cdr.cloud_msg(FID, int(stamps[b, 0]), int(stamps[b, 1]), xyzi[b, : npts[b]])
        assert ml[b] == len(want) and msgs[b, : ml[b]].tobytes() == want
        assert np.all(msgs[b, ml[b]:] == 0xEE)

    # the same clouds through the arena (completion order, per-scan starts)
    cap = int(npts.sum()) + 64
    d_arena = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
    d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
    d_start = torch.zeros(B, dtype=torch.int64, device=dev)
    gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, pv, d_arena.data_ptr(), cap,
                        d_cur.data_ptr(), d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())
    d_msgs2 = torch.full((B, stride), 0xEE, dtype=torch.uint8, device=dev)
    d_ml.fill_(-1)
    gpu.cloud_msgs_dev(d_arena.data_ptr(), 0, d_start.data_ptr(), d_np.data_ptr(), B, FID,
                       d_stamps.data_ptr(), d_msgs2.data_ptr(), stride, d_ml.data_ptr(),
                       d_st.data_ptr())
    gpu.synchronize()
    assert not d_st.cpu().numpy().any()
    assert np.array_equal(d_ml.cpu().numpy(), ml)
    assert d_msgs2.cpu().numpy().tobytes() == msgs.tobytes()


def test_c5_fused_cloud_message_with_sensor_poses(gpu, oracle):
    """BASELINE config 5 as one message: 8 sensors, each with its own mounting pose; per-sensor
    clip -> radius-outlier removal -> voxel grid into the arena, rigid transform of every cloud
    into the common frame, then the whole arena as ONE serialised PointCloud2 — all on the
    device.  Against the oracle clouds transformed by oracle/fusion_oracle.py and serialised by
    oracle/cdr_oracle.py."""
    import torch
    import fusion_oracle as fo
    S, n = 8, 32000
    batch = np.stack([synth.make_scan(700 + s, 0, n, noise_m=0.01) for s in range(S)])
    dev = torch.device("cuda:0")
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(S, n * 8)).to(dev)
    d_len = torch.full((S,), n, dtype=torch.int32, device=dev)
    p = Params.defaults(clip_enable=1, range_max=40.0, ror_enable=1, voxel_enable=1)
    cap = S * 16384
    d_arena = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
    d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
    d_start = torch.zeros(S, dtype=torch.int64, device=dev)
    d_np = torch.zeros(S, dtype=torch.int32, device=dev)
    d_st = torch.zeros(S, dtype=torch.int32, device=dev)
    gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), S, p, d_arena.data_ptr(), cap,
                        d_cur.data_ptr(), d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())
    poses = np.stack([fo.planar_pose(0.7 * s - 1.0, 0.35 * s, -0.2 * s, 0.05 * s) for s in range(S)])
    poses[3] = np.array([[0.36, 0.48, -0.8, 1.0], [-0.8, 0.6, 0.0, 2.0], [0.48, 0.64, 0.6, 0.5]],
                        np.float32)  # a tilted mount: full 3-D rotation
    d_pose = torch.from_numpy(poses.reshape(S, 12)).to(dev)
    gpu.transform_clouds_dev(d_arena.data_ptr(), 0, d_start.data_ptr(), d_np.data_ptr(), S,
                             d_pose.data_ptr())
    msg_cap = abi.msg_cloud_layout(len(FID), cap).total_len
    d_msg = torch.full((msg_cap,), 0xEE, dtype=torch.uint8, device=dev)
    d_ml = torch.zeros(1, dtype=torch.int64, device=dev)
    gpu.fused_cloud_msg_dev(d_arena.data_ptr(), d_cur.data_ptr(), cap, FID, 99, 7,
                            d_msg.data_ptr(), msg_cap, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    assert not d_st.cpu().numpy().any()
    total, ml = int(d_cur.item()), int(d_ml.item())
    starts, npts = d_start.cpu().numpy(), d_np.cpu().numpy()
    arena = d_arena.cpu().numpy()
    msg = d_msg.cpu().numpy()
    # the message is the arena, whatever order the scans completed in
    assert msg[:ml].tobytes() == cdr.cloud_msg(FID, 99, 7, arena[:total])
    assert np.all(msg[ml:] == 0xEE)
    for s in range(S):
        want, _, _ = oracle.cloud_pipeline(batch[s], oracle_lib.copy_params(p))
        assert npts[s] == len(want)
        got = arena[starts[s]: starts[s] + npts[s]]
        ref = fo.transform_cloud(want, poses[s])
        # the voxel centroids agree with the oracle to 1e-6 m (bit-exact for |x|,|y| >= 3 cm), the
        # transform adds at most a few ulp of the translated coordinates on top
        assert np.max(np.abs(got[:, :3].astype(np.float64) - ref[:, :3])) <= 3e-6
        assert got[:, 3].tobytes() == ref[:, 3].tobytes()
    # the transform itself, on exactly known inputs: bit for bit
    pts = np.random.default_rng(4).uniform(-40, 40, (S, 5000, 4)).astype(np.float32)
    d_pts = torch.from_numpy(pts).to(dev)
    d_cnt = torch.from_numpy(np.array([5000, 0, 1, 4999, 17, 4096, 4097, 5000], np.int32)).to(dev)
    gpu.transform_clouds_dev(d_pts.data_ptr(), 5000, 0, d_cnt.data_ptr(), S, d_pose.data_ptr())
    gpu.synchronize()
    out, cnt = d_pts.cpu().numpy(), d_cnt.cpu().numpy()
    for s in range(S):
        assert out[s, : cnt[s]].tobytes() == fo.transform_cloud(pts[s, : cnt[s]], poses[s]).tobytes()
        assert out[s, cnt[s]:].tobytes() == pts[s, cnt[s]:].tobytes()  # nothing past the cloud
    # a message buffer too small: length 0 + flag, nothing written
    d_msg.fill_(0xEE)
    gpu.fused_cloud_msg_dev(d_arena.data_ptr(), d_cur.data_ptr(), cap, FID, 99, 7,
                            d_msg.data_ptr(), ml - 1, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    assert int(d_ml.item()) == 0 and int(d_st[0].item()) & abi.SCAN_OUT_TRUNCATED
    assert bool((d_msg == 0xEE).all())


def test_allgather_clouds_on_device_single_rank_rccl(gpu):
    """The N > 1 exchange code with CUDA tensors and the nccl (= RCCL) backend, world size 1 —
    everything but a second GPU: device-side count, in-band table, views, splits."""
    import os
    import torch
    import torch.distributed as dist
    from rplidar_ros2_driver_amd.sharding import allgather_clouds, split_by_scan
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dev = torch.device("cuda:0")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        B, n = 12, 3000
        batch, lens, d_nodes, d_len = _batch(torch, 91, B, n)
        pv = Params.defaults(clip_enable=1, range_max=40.0, voxel_enable=1)
        cap = B * 4096
        d_arena = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
        d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
        d_start = torch.zeros(B, dtype=torch.int64, device=dev)
        d_np = torch.zeros(B, dtype=torch.int32, device=dev)
        d_st = torch.zeros(B, dtype=torch.int32, device=dev)
        gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, pv, d_arena.data_ptr(),
                            cap, d_cur.data_ptr(), d_start.data_ptr(), d_np.data_ptr(),
                            d_st.data_ptr())
        gpu.synchronize()
        want = d_arena.clone()
        clouds, counts, starts = allgather_clouds(d_arena, d_cur, d_np, scan_starts=d_start)
        assert allgather_clouds.last_in_band
        torch.cuda.synchronize()
        total = int(d_cur.item())
        assert len(clouds) == 1 and clouds[0].shape == (total, 4)
        assert torch.equal(clouds[0], want[:total])
        assert torch.equal(counts[0].cpu(), d_np.cpu().to(torch.int64))
        assert torch.equal(starts[0].cpu(), d_start.cpu())
        per_scan = split_by_scan(clouds[0], counts[0], starts[0])
        for b in range(B):
            a = int(d_start[b])
            assert torch.equal(per_scan[b], want[a: a + int(d_np[b])])
        # a buffer without room behind the points: the two-collective branch, same result
        tight = want[:total].clone()
        c2, n2, s2 = allgather_clouds(tight, total, d_np, scan_starts=d_start)
        assert not allgather_clouds.last_in_band
        assert torch.equal(c2[0], clouds[0]) and torch.equal(n2[0], counts[0])
    finally:
        if created:
            dist.destroy_process_group()


def test_deskewed_cloud_matches_oracle(gpu, oracle):
    """E6 motion de-skew of the plain cloud (include/rplgpu_msg.h): bit for bit against the
    numpy restatement applied to the oracle's cloud."""
    import torch
    import fusion_oracle as fo
    B, n = 6, 5000
    batch, lens, d_nodes, d_len = _batch(torch, 123, B, n)
    dev = d_nodes.device
    motion = np.array([[0.0, 0.0, 0.0, 0.0], [1.5, -0.7, 0.9, 2.0e-5], [0.0, 0.0, -3.0, 2.0e-5],
                       [-12.0, 4.0, 0.0, 1.0e-4], [0.3, 0.2, 0.5, 3.125e-6], [2.0, 2.0, 4.9, 2.0e-5]],
                      np.float32)
    d_motion = torch.from_numpy(motion).to(dev)
    d_xyzi = torch.zeros(B, n, 4, dtype=torch.float32, device=dev)
    d_np = torch.zeros(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    for clip in (0, 1):
        p = Params.defaults(clip_enable=clip, q_min=30 * clip, range_min=0.5, range_max=25.0,
                            inverted=clip)
        gpu.cloud_deskew_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p,
                                   d_motion.data_ptr(), d_xyzi.data_ptr(), n, d_np.data_ptr(),
                                   d_st.data_ptr())
        gpu.synchronize()
        got, npts = d_xyzi.cpu().numpy(), d_np.cpu().numpy()
        for b in range(B):
            nodes = batch[b, : lens[b]]
            plain = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p))
            d = nodes["dist_mm_q2"]
            dm = d.astype(np.float32) / np.float32(4000.0)
            keep = d != 0
            if clip:
                keep &= (nodes["quality"] >= 30) & (dm >= np.float32(0.5)) & (dm <= np.float32(25.0))
            idx = np.flatnonzero(keep)
            assert len(idx) == len(plain) == npts[b]
            want = fo.deskew_cloud(plain, idx, motion[b])
            assert got[b, : npts[b]].tobytes() == want.tobytes(), (clip, b)
            if b == 0:  # no motion: the plain cloud, untouched
                assert want.tobytes() == plain.tobytes()
    # time alignment (rplgpu_set_scan_time_offsets_dev): the scans did not start at the fused instant
    t0 = np.array([0.0, -0.031, 0.012, 0.05, -2.5e-4, 0.0], np.float32)
    d_t0 = torch.from_numpy(t0).to(dev)
    p = Params.defaults(clip_enable=1, q_min=10, range_min=0.5, range_max=25.0)

    def kept_index(nodes):
        dm = nodes["dist_mm_q2"].astype(np.float32) / np.float32(4000.0)
        return np.flatnonzero((nodes["dist_mm_q2"] != 0) & (nodes["quality"] >= 10) & (dm >= np.float32(0.5))
                              & (dm <= np.float32(25.0)))

    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        gpu.cloud_deskew_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_motion.data_ptr(),
                                   d_xyzi.data_ptr(), n, d_np.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    got, npts = d_xyzi.cpu().numpy(), d_np.cpu().numpy()
    moved = 0
    for b in range(B):
        nodes = batch[b, : lens[b]]
        plain = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p))
        idx = kept_index(nodes)
        assert len(idx) == npts[b]
        want = fo.deskew_cloud(plain, idx, motion[b], t0[b])
        assert got[b, : npts[b]].tobytes() == want.tobytes(), b
        moved += want.tobytes() != fo.deskew_cloud(plain, idx, motion[b]).tobytes()
    assert moved >= 3  # (scans 0 and 5 have a zero offset, scan 0 no motion either)
    # offsets off again: the launch is the one without them, bit for bit
    gpu.cloud_deskew_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_motion.data_ptr(),
                               d_xyzi.data_ptr(), n, d_np.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    got = d_xyzi.cpu().numpy()
    for b in range(B):
        nodes = batch[b, : lens[b]]
        plain = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p))
        idx = kept_index(nodes)
        assert got[b, : len(idx)].tobytes() == fo.deskew_cloud(plain, idx, motion[b]).tobytes()
    # voxel_enable is refused: de-skew belongs in front of the cell computation
    with pytest.raises(abi.RplGpuError):
        gpu.cloud_deskew_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B,
                                   Params.defaults(voxel_enable=1), d_motion.data_ptr(),
                                   d_xyzi.data_ptr(), n, d_np.data_ptr(), d_st.data_ptr())


# ------------------------------------------------ E7: LaserScan -> PointCloud2 projection (f3)
def test_laserscan_to_cloud_matches_oracle(gpu, oracle):
    """The `laser_geometry`-style cloud source of SURVEY.md §8(f) row 3: the binned LaserScan
    (what publish_scan fills, /root/reference src/rplidar_node.cpp:618-662) projected to E3
    points.  Keep mask / order exact; XYZ <= 1e-6 m (in fact bit-exact: fp64 sincos rounded once);
    intensity bit-exact."""
    import torch
    from tests.cases import CASES
    dev = torch.device("cuda:0")
    for name in ("c1_like_360", "ring_8192_rot_jit", "c2_32000", "kat2", "single_valid",
                 "all_invalid", "full_32768_unsorted"):
        nodes = CASES[name]
        for sp, inv, clip in ((1, 0, 0), (1, 1, 1), (0, 0, 0), (0, 1, 1)):
            p = Params.defaults(scan_processing=sp, inverted=inv, range_max=40.0)
            r, i, m = gpu.scan_to_laserscan(nodes, p, 0.1)
            pc = Params.defaults(scan_processing=sp, clip_enable=clip, range_min=0.3, range_max=9.0)
            want = oracle.laserscan_to_cloud(r, i, oracle_lib.copy_params(pc))
            got = gpu.laserscan_to_cloud(r, i, pc)
            assert got.shape == want.shape, (name, sp, inv, clip)
            if len(want):
                assert np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2])) <= 1e-6
                assert got[:, 2:].tobytes() == want[:, 2:].tobytes()
    # batch, device resident: LaserScans straight from rplgpu_laserscan_batch_dev, then the clouds
    # as serialised PointCloud2 messages (rplgpu_cloud_msgs_dev) — the whole row-3 chain in HBM
    B, n = 12, 6000
    batch = synth.make_batch(77, B, n, jitter=2)
    lens = np.array([n - 401 * b for b in range(B)], np.int32)
    lens[5] = 0
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.from_numpy(lens).to(dev)
    d_r = torch.empty(B, n, dtype=torch.float32, device=dev)
    d_i = torch.empty(B, n, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    p = Params.defaults(range_max=40.0)
    gpu.laserscan_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_r.data_ptr(),
                            d_i.data_ptr(), d_cnt.data_ptr())
    d_xyzi = torch.zeros(B, n, 4, dtype=torch.float32, device=dev)
    d_np = torch.zeros(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    gpu.laserscan_to_cloud_batch_dev(d_r.data_ptr(), d_i.data_ptr(), n, d_cnt.data_ptr(), B, p,
                                     d_xyzi.data_ptr(), n, d_np.data_ptr(), d_st.data_ptr())
    fid = "laser_frame"
    mstride = abi.msg_cloud_layout(len(fid), n).total_len
    mstride = (mstride + 3) & ~3
    d_msgs = torch.zeros(B, mstride, dtype=torch.uint8, device=dev)
    d_ml = torch.zeros(B, dtype=torch.int32, device=dev)
    d_stamps = torch.tensor([[100 + b, 7 * b] for b in range(B)], dtype=torch.int32, device=dev)
    gpu.cloud_msgs_dev(d_xyzi.data_ptr(), n, 0, d_np.data_ptr(), B, fid, d_stamps.data_ptr(),
                       d_msgs.data_ptr(), mstride, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    r, i, cnt = d_r.cpu().numpy(), d_i.cpu().numpy(), d_cnt.cpu().numpy()
    xyzi, npts = d_xyzi.cpu().numpy(), d_np.cpu().numpy()
    msgs, ml = d_msgs.cpu().numpy(), d_ml.cpu().numpy()
    for b in range(B):
        want = oracle.laserscan_to_cloud(r[b, : cnt[b]], i[b, : cnt[b]], oracle_lib.copy_params(p))
        assert npts[b] == len(want)
        got = xyzi[b, : npts[b]]
        if len(want):
            assert np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2])) <= 1e-6
            assert got[:, 2:].tobytes() == want[:, 2:].tobytes()
        assert msgs[b, : ml[b]].tobytes() == cdr.cloud_msg(fid, 100 + b, 7 * b, got)


# ------------------------------------------------ E8: one voxel grid per group of scans (row 4)
def _e8_oracle(oracle, scans, p, motion, pose2d, leaf, t0=None):
    """Spec of rplgpu_cloud_fused_voxel_dev from its parts (tests/fused_oracle.py): E1 + E2 per scan (C
    oracle), E5 on every scan's own points when p.ror_enable, E6 de-skew and the planar pose (numpy
    restatements in oracle/fusion_oracle.py), then E4 over all in-range points of the group (C oracle's
    voxel grid)."""
    from tests import fused_oracle
    assert np.float32(leaf) == np.float32(p.voxel_leaf)
    cloud, cells, counts, status = fused_oracle.fused_grid(oracle, scans, p, motion, pose2d, t0)
    assert status == 0
    return cloud, cells, counts


def test_fused_voxel_groups_match_oracle(gpu, oracle):
    """De-skew in front of the voxel grid (group = 1, motion) and the cross-sensor voxel grid
    (8 sensors with poses -> one grid per time step)."""
    import torch
    import fusion_oracle as fo
    dev = torch.device("cuda:0")
    n = 12000
    for group, G, noise in ((1, 6, 0.0), (8, 3, 0.01), (3, 2, 0.0)):
        B = group * G + (1 if group == 3 else 0)  # (3, 2): a last, partial group of one scan
        scans = [synth.make_scan(1000 + group, b, n, noise_m=noise, r0_range=(2.0, 12.0)) for b in range(B)]
        batch = np.stack(scans)
        rng = np.random.default_rng(group)
        motion = np.stack([[rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-0.4, 0.4),
                            0.1 / n] for _ in range(B)]).astype(np.float32)
        poses = np.stack([fo.planar_pose(rng.uniform(-3, 3), rng.uniform(-4, 4), rng.uniform(-4, 4))
                          for _ in range(B)])
        pose2d = np.ascontiguousarray(poses[:, :2][:, :, [0, 1, 3]].reshape(B, 6))
        p = Params.defaults(clip_enable=1, q_min=8, range_min=0.15, range_max=40.0, voxel_enable=1,
                            voxel_leaf=0.05)
        d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
        d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
        d_motion = torch.from_numpy(motion).to(dev)
        d_pose = torch.from_numpy(pose2d).to(dev)
        ng = (B + group - 1) // group
        cap = B * n
        for use_m, use_p in ((True, True), (True, False), (False, True), (False, False)):
            d_arena = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
            d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
            d_start = torch.zeros(ng, dtype=torch.int64, device=dev)
            d_np = torch.zeros(ng, dtype=torch.int32, device=dev)
            d_st = torch.zeros(ng, dtype=torch.int32, device=dev)
            gpu.cloud_fused_voxel_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, group, p,
                                      d_motion.data_ptr() if use_m else 0,
                                      d_pose.data_ptr() if use_p else 0, d_arena.data_ptr(), cap,
                                      d_cur.data_ptr(), d_start.data_ptr(), d_np.data_ptr(),
                                      d_st.data_ptr())
            gpu.synchronize()
            assert int(d_st.max()) == 0
            arena, start, npts = d_arena.cpu().numpy(), d_start.cpu().numpy(), d_np.cpu().numpy()
            assert int(d_cur.item()) == int(npts.sum())
            for g in range(ng):
                sl = slice(g * group, min(B, (g + 1) * group))
                want, wcells, _ = _e8_oracle(oracle, scans[sl], p, motion[sl] if use_m else None,
                                             pose2d[sl] if use_p else None, 0.05)
                got = arena[start[g]: start[g] + npts[g]]
                assert len(got) == len(want), (group, g, use_m, use_p)
                assert np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2])) <= 1e-6
                assert np.all(got[:, 2] == 0.0)
                assert got[:, 3].tobytes() == want[:, 3].tobytes()
            if group == 1 and not use_m and not use_p:
                # no motion, identity pose, groups of one: exactly rplgpu_cloud_arena_dev
                d_a2 = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
                d_s2 = torch.zeros(B, dtype=torch.int64, device=dev)
                d_n2 = torch.zeros(B, dtype=torch.int32, device=dev)
                gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_a2.data_ptr(), cap,
                                    d_cur.data_ptr(), d_s2.data_ptr(), d_n2.data_ptr(), d_st.data_ptr())
                gpu.synchronize()
                a2, s2, n2 = d_a2.cpu().numpy(), d_s2.cpu().numpy(), d_n2.cpu().numpy()
                for b in range(B):
                    assert npts[b] == n2[b]
                    assert arena[start[b]: start[b] + npts[b]].tobytes() == a2[s2[b]: s2[b] + n2[b]].tobytes()


def test_fused_voxel_time_alignment(gpu_mode, oracle):
    """The temporal side of row 4: the sensors of a time step start their scans at different instants;
    with rplgpu_set_scan_time_offsets_dev every point is de-skewed to the FUSED instant
    (tau = t0 + i * time_increment) before the shared grid.  Against the composition of the oracles, in
    every form of the voxel path; without motion the call is refused."""
    import torch
    import fusion_oracle as fo
    gpu = gpu_mode
    dev = torch.device("cuda:0")
    n, group, G = 9000, 4, 3
    B = group * G
    scans = [synth.make_scan(4100, b, n, noise_m=0.005, r0_range=(2.0, 10.0)) for b in range(B)]
    batch = np.stack(scans)
    rng = np.random.default_rng(41)
    motion = np.stack([[rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.8, 0.8), 0.1 / n]
                       for _ in range(B)]).astype(np.float32)
    t0 = rng.uniform(-0.08, 0.08, B).astype(np.float32)
    t0[1] = 0.0
    poses = np.stack([fo.planar_pose(rng.uniform(-3, 3), rng.uniform(-4, 4), rng.uniform(-4, 4)) for _ in range(B)])
    pose2d = np.ascontiguousarray(poses[:, :2][:, :, [0, 1, 3]].reshape(B, 6))
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, voxel_enable=1, voxel_leaf=0.05)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    d_motion = torch.from_numpy(motion).to(dev)
    d_pose = torch.from_numpy(pose2d).to(dev)
    d_t0 = torch.from_numpy(t0).to(dev)
    cap = B * n

    def run(with_motion=True):
        d_arena = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
        d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
        d_start = torch.zeros(G, dtype=torch.int64, device=dev)
        d_np = torch.zeros(G, dtype=torch.int32, device=dev)
        d_st = torch.zeros(G, dtype=torch.int32, device=dev)
        gpu.cloud_fused_voxel_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, group, p,
                                  d_motion.data_ptr() if with_motion else 0, d_pose.data_ptr(), d_arena.data_ptr(),
                                  cap, d_cur.data_ptr(), d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
        assert int(d_st.max()) == 0
        return d_arena.cpu().numpy(), d_start.cpu().numpy(), d_np.cpu().numpy()

    base = run()
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        arena, start, npts = run()
        with pytest.raises(abi.RplGpuError):
            run(with_motion=False)
    finally:
        gpu.set_scan_time_offsets_dev(0)
    differs = 0
    for g in range(G):
        sl = slice(g * group, (g + 1) * group)
        want, _, _ = _e8_oracle(oracle, scans[sl], p, motion[sl], pose2d[sl], 0.05, t0[sl])
        got = arena[start[g]: start[g] + npts[g]]
        assert len(got) == len(want), g
        assert np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2])) <= 1e-6
        assert got[:, 3].tobytes() == want[:, 3].tobytes()
        b0 = base[0][base[1][g]: base[1][g] + base[2][g]]
        differs += len(b0) != len(got) or b0.tobytes() != got.tobytes()
    assert differs == G  # the offsets move the points: every group's grid changes
    after = run()  # offsets off again: the launch without them
    for g in range(G):
        assert after[0][after[1][g]: after[1][g] + after[2][g]].tobytes() == \
            base[0][base[1][g]: base[1][g] + base[2][g]].tobytes()


def test_laserscan_msgs_dev_beam_count_above_the_stride(gpu):
    """A beam count above n_stride is a scan of n_stride beams (as E7 and E10 clamp it): the message and its
    length are those of 16 beams, built from the scan's own slot and never from the next one, and with a
    msg_stride that a message of 100000 beams would fit nothing behind the message is written."""
    import torch
    dev = torch.device("cuda:0")
    B, n = 5, 16
    rng = np.random.default_rng(16)
    r = rng.uniform(0.2, 30.0, (B, n)).astype(np.float32)
    i = rng.uniform(0.0, 60.0, (B, n)).astype(np.float32)
    p = Params.defaults(range_max=40.0)
    stamps = np.stack([np.arange(B) + 5, np.arange(B) * 11], 1).astype(np.int32)
    durs = 0.1 + 0.01 * np.arange(B)
    want_len = abi.msg_laserscan_layout(len(FID), n).total_len
    stride = (abi.msg_laserscan_layout(len(FID), 100000).total_len + 3) & ~3
    # (the arrays are followed by 100000 more floats, so that a library without the clamp reads other values
    # and never leaves the allocation)
    pad = np.full(100000, 3.0, np.float32)
    d_r = torch.from_numpy(np.concatenate([r.reshape(-1), pad])).to(dev)
    d_i = torch.from_numpy(np.concatenate([i.reshape(-1), pad])).to(dev)
    d_cnt = torch.full((B,), 100000, dtype=torch.int32, device=dev)
    d_stamps, d_dur = torch.from_numpy(stamps).to(dev), torch.from_numpy(durs).to(dev)
    d_msgs = torch.full((B, stride), 0xEE, dtype=torch.uint8, device=dev)
    d_ml = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    gpu.laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), n, d_cnt.data_ptr(), B, p, FID, d_stamps.data_ptr(),
                           d_dur.data_ptr(), d_msgs.data_ptr(), stride, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    msgs, ml = d_msgs.cpu().numpy(), d_ml.cpu().numpy()
    assert not d_st.cpu().numpy().any()
    for b in range(B):
        meta = gpu.fill_meta(p, n, float(durs[b]))
        want = cdr.laserscan_msg(FID, int(stamps[b, 0]), int(stamps[b, 1]), meta, r[b], i[b])
        assert ml[b] == len(want) == want_len
        assert msgs[b, :want_len].tobytes() == want
        assert np.all(msgs[b, want_len:] == 0xEE)  # the bytes behind it are untouched
