"""Handles of small and odd capacity.  rplgpu_create accepts max_samples_per_scan 1 .. 32768 and derives the
single-scan staging layout from it (nodes | tail | results | tail | completion flag in one pinned buffer);
every other test creates handles of 8192 or 32768 samples.  With the layout as it was — result area at
max_n * 8 + 64, flag at max_n * 24 + 128 — an odd capacity put the result area, which the cloud kernels fill
with 16-byte stores, on an 8-byte boundary, and any capacity that is no multiple of 8 put the flag word off
the 64-byte boundary its comment claimed.  Both regions are now rounded up to 64 bytes;
test_staging_layout_is_aligned_for_every_capacity pins that (it fails on the old layout), the other tests run
every single-scan host call and the check_batch entry points on such handles against the oracles."""
import contextlib
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import NODE_DTYPE, Params, RplGpu, abi
from tests import filter_oracle as fo
from tests import fused_oracle as fu
from tests import oracle_lib
from tests.test_gpu_merge import _check as merge_check
from tests.test_gpu_merge import _spec as merge_spec
from tests.test_gpu_msg import _unique_angles
from tests.test_gpu_parity import XYZ_TOL, _has_intensity_tie

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import cdr_oracle as cdr  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FID = "laser_frame"
CAPS = (1, 2, 7, 360, 361, 1001, 8191)
BATCHES = (1, 3)


@contextlib.contextmanager
def _handle(cap, max_batch, env=None):
    """A handle on the session's shared stream; `env` is set around rplgpu_create only."""
    from tests.conftest import _shared_stream
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = RplGpu(device=0, max_samples_per_scan=cap, max_batch=max_batch)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        h.set_stream(_shared_stream().cuda_stream)
        yield h
        h.synchronize()
    finally:
        h.close()


def _scan(n, seed):
    """n samples with unique angle words (the reference's unstable sorts leave no choice), rotated by a third
    of a turn and with neighbours swapped so that ascend has work, distances 0.15 .. 40 m, one in ten invalid."""
    rng = np.random.default_rng([seed, n])
    m = np.zeros(n, NODE_DTYPE)
    if n == 0:
        return m
    q = np.sort(rng.choice(65536, size=n, replace=False))
    q = np.roll(q, n // 3)
    for j in range(0, n - 1, 5):
        q[j], q[j + 1] = q[j + 1], q[j]
    m["angle_z_q14"] = q
    d = rng.integers(600, 160001, n)
    d[rng.random(n) < 0.1] = 0
    m["dist_mm_q2"] = d
    m["quality"] = rng.integers(0, 256, n)
    m["flag"] = rng.integers(0, 4, n)
    return m


def _struct(f):
    return abi.ScanFilter(**{k: f[k] for k, _ in abi.ScanFilter._fields_})


def _check_cloud(got, status, want, exact):
    assert status == 0 and got.shape[0] == len(want)
    if exact:
        assert got.tobytes() == np.ascontiguousarray(want, F32).tobytes()
    elif len(want):
        assert np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2])) <= XYZ_TOL
        assert got[:, 3].tobytes() == want[:, 3].astype(F32).tobytes()


def _check_single_scan_calls(h, oracle, nodes):
    """Every single-scan host call on `nodes`, compared as test_gpu_parity / test_gpu_msg / test_gpu_filter do."""
    n = len(nodes)
    if n == 0:
        assert h.ascend(nodes.copy()) == 0x80008001
        r, i, m = h.scan_to_laserscan(nodes, Params.defaults())
        assert len(r) == 0 and not m.published
        cloud, st = h.scan_to_cloud(nodes, Params.defaults())
        assert len(cloud) == 0 and st == 0
        msg, m = h.scan_to_laserscan_msg(nodes, Params.defaults(), 0.1, FID, 1, 2)
        assert len(msg) == 0 and not m.published
        msg, npts, _ = h.scan_to_cloud_msg(nodes, Params.defaults(), FID, 1, 2)
        assert npts == 0 and msg.tobytes() == cdr.cloud_msg(FID, 1, 2, np.zeros((0, 4), F32))
        assert len(h.laserscan_to_cloud(np.zeros(0, F32), np.zeros(0, F32), Params.defaults())) == 0
        ro, _, removed = h.filter_laserscan(np.zeros(0, F32), np.zeros(0, F32), 0.01, _struct(fo.flt()))
        assert len(ro) == 0 and removed == (0, 0)
        return
    assert _unique_angles(nodes)
    # ascend
    want, want_res = oracle.ascend(nodes)
    got = nodes.copy()
    assert h.ascend(got) == want_res
    if want_res == 0:
        assert np.array_equal(got["angle_z_q14"], want["angle_z_q14"])
        assert oracle_lib.canon_equal_angle_runs(got).tobytes() == oracle_lib.canon_equal_angle_runs(want).tobytes()
    else:
        assert got.tobytes() == nodes.tobytes()
    # LaserScan, Mode A and B, inverted or not; the message of each; E7 and E10 on the published arrays
    for sp in (1, 0):
        for inverted in (0, 1):
            p = Params.defaults(scan_processing=sp, inverted=inverted, range_max=40.0)
            assert not _has_intensity_tie(nodes, p)
            wr, wi, wm = oracle.publish_scan(nodes, oracle_lib.copy_params(p), 0.125)
            gr, gi, gm = h.scan_to_laserscan(nodes, p, 0.125)
            assert bytes(gm) == bytes(wm), (sp, inverted)
            msg, mm = h.scan_to_laserscan_msg(nodes, p, 0.125, FID, 1727000000, 123456789)
            assert bytes(mm) == bytes(wm)
            if not wm.published:
                assert len(msg) == 0
                continue
            assert gr.tobytes() == wr.tobytes() and gi.tobytes() == wi.tobytes(), (sp, inverted)
            assert msg.tobytes() == cdr.laserscan_msg(FID, 1727000000, 123456789, wm, wr, wi), (sp, inverted)
            if inverted:
                continue
            pc = h.laserscan_to_cloud(wr, wi, p)
            wpc = oracle.laserscan_to_cloud(wr, wi, oracle_lib.copy_params(p))
            assert pc.shape == wpc.shape
            assert len(wpc) == 0 or np.max(np.abs(pc.astype(np.float64) - wpc)) <= 1e-6
            f = fo.flt(circular=sp)
            ro, io, removed = h.filter_laserscan(wr, wi, float(wm.angle_increment), _struct(f))
            wf, n_sh, n_sp = fo.filter_scan(wr, wm.angle_increment, f)
            assert ro.view(np.uint32).tobytes() == wf.view(np.uint32).tobytes()
            assert io.tobytes() == wi.tobytes() and removed == (n_sh, n_sp)
    # clouds: plain, E5, E4, E5 + E4; the message of each
    for ror, voxel in ((0, 0), (1, 0), (0, 1), (1, 1)):
        p = Params.defaults(clip_enable=1, q_min=8, range_min=0.15, range_max=40.0, ror_enable=ror,
                            ror_radius=0.10, ror_min_neighbors=2, voxel_enable=voxel)
        if voxel:
            want, _, _ = oracle.cloud_pipeline(nodes, oracle_lib.copy_params(p))
        else:
            want = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p))
        got, status = h.scan_to_cloud(nodes, p)
        _check_cloud(got, status, want, exact=not voxel)
        msg, npts, st = h.scan_to_cloud_msg(nodes, p, FID, 17, 42)
        assert st == 0 and npts == len(got) and msg.tobytes() == cdr.cloud_msg(FID, 17, 42, got), (ror, voxel)


def _check_capacity_errors(h, cap):
    """n = capacity + 1: RPLGPU_ERR_CAPACITY from each single-scan call."""
    big = _scan(cap + 1, 5)
    arr = np.ones(cap + 1, F32)
    p = Params.defaults()
    calls = [lambda: h.ascend(big.copy()), lambda: h.scan_to_laserscan(big, p), lambda: h.scan_to_cloud(big, p),
             lambda: h.scan_to_laserscan_msg(big, p, 0.1, FID, 0, 0), lambda: h.scan_to_cloud_msg(big, p, FID, 0, 0),
             lambda: h.laserscan_to_cloud(arr, arr, p),
             lambda: h.filter_laserscan(arr, arr, 0.01, _struct(fo.flt()))]
    for k, call in enumerate(calls):
        with pytest.raises(abi.RplGpuError) as e:
            call()
        assert e.value.code == abi.ERR_CAPACITY, k


def test_staging_layout_is_aligned_for_every_capacity():
    """Result area and completion flag on 64-byte boundaries, regions that do not overlap, for every capacity
    rplgpu_create accepts (host arithmetic only)."""
    lib = abi.load_library()
    lib.rplgpu_debug_staging_layout.argtypes = [C.c_uint32, C.POINTER(C.c_uint64)]
    lib.rplgpu_debug_staging_layout.restype = C.c_int32
    out = (C.c_uint64 * 3)()
    assert lib.rplgpu_debug_staging_layout(0, out) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_debug_staging_layout(abi.MAX_SAMPLES_PER_SCAN + 1, out) == abi.ERR_INVALID_ARG
    for n in range(1, abi.MAX_SAMPLES_PER_SCAN + 1):
        assert lib.rplgpu_debug_staging_layout(n, out) == abi.OK
        out_off, flag_off, total = out[0], out[1], out[2]
        assert out_off % 64 == 0 and flag_off % 64 == 0, n
        assert out_off >= n * 8 + 64, n              # nodes, then the words that travel behind them
        assert flag_off >= out_off + n * 16 + 64, n  # results, then their words
        assert total >= flag_off + 64, n


@pytest.mark.parametrize("max_batch", BATCHES)
@pytest.mark.parametrize("cap", CAPS)
def test_single_scan_calls(oracle, cap, max_batch):
    with _handle(cap, max_batch) as h:
        # large then small, back to back: the count / status words behind the nodes and the results move with n
        for n in (cap, cap - 1, 0):
            _check_single_scan_calls(h, oracle, _scan(n, 11))
        _check_capacity_errors(h, cap)
        _check_single_scan_calls(h, oracle, _scan(cap, 12))  # the next call on the same handle
        _check_single_scan_calls(h, oracle, _scan(max(cap // 3, 1), 13))


@pytest.mark.parametrize("env", [{"RPLGPU_ZERO_COPY": "0"}, {"RPLGPU_SPIN_SYNC": "0"}], ids=["dma", "no_spin"])
@pytest.mark.parametrize("cap", [361, 1001])
def test_single_scan_calls_without_zero_copy_or_spinning(oracle, cap, env):
    before = dict(os.environ)
    with _handle(cap, 1, env) as h:
        assert dict(os.environ) == before  # set around the create only
        for n in (cap, cap - 1, 0):
            _check_single_scan_calls(h, oracle, _scan(n, 21))
        _check_capacity_errors(h, cap)
        _check_single_scan_calls(h, oracle, _scan(cap, 22))


@pytest.mark.parametrize("max_batch", BATCHES)
@pytest.mark.parametrize("cap", CAPS)
def test_batch_entry_points_at_full_capacity(oracle, cap, max_batch):
    """B == max_batch scans of n_stride == capacity samples through the entry points check_batch guards;
    B == max_batch + 1 is refused and leaves a working handle."""
    import torch
    dev = torch.device("cuda:0")
    B, n = max_batch, cap
    batch = np.stack([_scan(n, 30 + b) for b in range(B + 1)])
    lens = np.array([n] + [max(n - 1 - b, 0) for b in range(B)], np.int32)[: B + 1]
    with _handle(cap, max_batch) as h:
        d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B + 1, n * 8)).to(dev)
        d_len = torch.from_numpy(lens).to(dev)
        d_st = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        d_r = torch.full((B + 1, n), 7.0, dtype=torch.float32, device=dev)
        d_i = torch.full((B + 1, n), 7.0, dtype=torch.float32, device=dev)
        d_cnt = torch.full((B + 1,), 12345, dtype=torch.int32, device=dev)
        d_xyzi = torch.full((B + 1, n, 4), 7.0, dtype=torch.float32, device=dev)
        d_arena = torch.full(((B + 1) * n, 4), 7.0, dtype=torch.float32, device=dev)
        d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
        d_start = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        p = Params.defaults(range_max=40.0)
        pv = Params.defaults(clip_enable=1, range_max=40.0, voxel_enable=1)
        lib = abi.load_library()
        # one scan too many: refused by each, nothing launched
        args = (h._h, d_nodes.data_ptr(), n, d_len.data_ptr(), B + 1)
        assert lib.rplgpu_ascend_batch_dev(*args, d_st.data_ptr()) == abi.ERR_CAPACITY
        assert lib.rplgpu_laserscan_batch_dev(*args, C.byref(p), d_r.data_ptr(), d_i.data_ptr(),
                                              d_cnt.data_ptr()) == abi.ERR_CAPACITY
        assert lib.rplgpu_cloud_batch_dev(*args, C.byref(pv), d_xyzi.data_ptr(), n, d_cnt.data_ptr(),
                                          d_st.data_ptr()) == abi.ERR_CAPACITY
        assert lib.rplgpu_cloud_arena_dev(*args, C.byref(pv), d_arena.data_ptr(), (B + 1) * n, d_cur.data_ptr(),
                                          d_start.data_ptr(), d_cnt.data_ptr(), d_st.data_ptr()) == abi.ERR_CAPACITY
        sd, ss = merge_spec(16)
        assert lib.rplgpu_merge_scans_dev(*args, 1, C.byref(pv), 0, 0, C.byref(ss), d_r.data_ptr(), d_i.data_ptr(),
                                          d_cnt.data_ptr(), 0) == abi.ERR_CAPACITY
        h.synchronize()
        assert np.all(d_r.cpu().numpy() == 7.0) and np.all(d_cnt.cpu().numpy() == 12345)
        # B == max_batch
        h.laserscan_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_r.data_ptr(), d_i.data_ptr(),
                              d_cnt.data_ptr())
        d_np1 = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        h.cloud_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, pv, d_xyzi.data_ptr(), n, d_np1.data_ptr(),
                          d_st.data_ptr())
        h.synchronize()
        r, i, cnt = d_r.cpu().numpy(), d_i.cpu().numpy(), d_cnt.cpu().numpy()
        xyzi, npts = d_xyzi.cpu().numpy(), d_np1.cpu().numpy()
        assert cnt[B] == 12345 and np.all(r[B] == 7.0) and np.all(xyzi[B] == 7.0)
        assert not d_st.cpu().numpy().any()
        for b in range(B):
            wr, wi, wm = oracle.publish_scan(batch[b, : lens[b]], oracle_lib.copy_params(p), 0.1)
            assert cnt[b] == wm.count
            assert r[b, : wm.count].tobytes() == wr.tobytes() and i[b, : wm.count].tobytes() == wi.tobytes()
            want, _, _ = oracle.cloud_pipeline(batch[b, : lens[b]], oracle_lib.copy_params(pv))
            _check_cloud(xyzi[b, : npts[b]], 0, want, exact=False)
        # the same clouds through the arena
        d_np = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        h.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, pv, d_arena.data_ptr(), B * n, d_cur.data_ptr(),
                          d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())
        h.synchronize()
        arena, start, np2 = d_arena.cpu().numpy(), d_start.cpu().numpy(), d_np.cpu().numpy()
        assert np.array_equal(np2[:B], npts[:B]) and int(d_cur.item()) == int(npts[:B].sum())
        for b in range(B):
            assert arena[start[b]: start[b] + np2[b]].tobytes() == xyzi[b, : npts[b]].tobytes()
        assert np.all(arena[B * n:] == 7.0)
        # ascend, in place
        d_nodes2 = d_nodes.clone()
        h.ascend_batch_dev(d_nodes2.data_ptr(), n, d_len.data_ptr(), B, d_st.data_ptr())
        h.synchronize()
        asc, st = d_nodes2.cpu().numpy().view(NODE_DTYPE).reshape(B + 1, n), d_st.cpu().numpy()
        for b in range(B):
            want, res = oracle.ascend(batch[b, : lens[b]])
            assert (st[b] & abi.SCAN_ALL_INVALID != 0) == (res != 0)
            if res == 0:
                assert oracle_lib.canon_equal_angle_runs(asc[b, : lens[b]]).tobytes() == \
                    oracle_lib.canon_equal_angle_runs(want).tobytes()
            assert asc[b, lens[b]:].tobytes() == batch[b, lens[b]:].tobytes()
        assert asc[B].tobytes() == batch[B].tobytes()
        # E9: all B scans merged into one scan of 16 beams
        pm = Params.defaults(clip_enable=1, q_min=8, range_min=0.15, range_max=40.0)
        merge_check(oracle, h, batch[:B], B, pm, (sd, ss))


def test_e5_and_e4_with_the_smallest_scratch(oracle):
    """max_batch = 1: d_rormask, d_redo and d_need_sort have their smallest size.  E5 + E4 (and E5 alone) on a
    scan where the oracle removes points: the head of tests/fused_oracle.py's settled scan, variant 2 (a lone
    return on the first sample, far inside the ring), cut to 361 samples."""
    import torch
    dev = torch.device("cuda:0")
    n = 361
    nodes = np.ascontiguousarray(fu.settled_scan(3100, 2, 32000)[0][:n])
    p = Params.defaults(**fu.P_C5)
    p_off = Params.defaults(**{**fu.P_C5, "ror_enable": 0, "voxel_enable": 0})
    p_ror = Params.defaults(**{**fu.P_C5, "voxel_enable": 0})
    base = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p_off))
    kept = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p_ror))
    assert 0 < len(kept) < len(base)  # E5 removes something here
    want, _, _ = oracle.cloud_pipeline(nodes, oracle_lib.copy_params(p))
    with _handle(n, 1) as h:
        got, status = h.scan_to_cloud(nodes, p)
        _check_cloud(got, status, want, exact=False)
        got, status = h.scan_to_cloud(nodes, p_ror)
        _check_cloud(got, status, kept, exact=True)
        d_nodes = torch.from_numpy(nodes.view(np.uint8).reshape(1, n * 8)).to(dev)
        d_len = torch.full((1,), n, dtype=torch.int32, device=dev)
        d_xyzi = torch.full((2, n, 4), 7.0, dtype=torch.float32, device=dev)
        d_np = torch.zeros(1, dtype=torch.int32, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        for pp, ww, exact in ((p, want, False), (p_ror, kept, True)):
            h.cloud_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), 1, pp, d_xyzi.data_ptr(), n, d_np.data_ptr(),
                              d_st.data_ptr())
            h.synchronize()
            xyzi = d_xyzi.cpu().numpy()
            _check_cloud(xyzi[0, : int(d_np.item())], int(d_st.item()), ww, exact)
            assert np.all(xyzi[1] == 7.0)
