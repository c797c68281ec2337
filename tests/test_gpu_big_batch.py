"""Batches above 65535 scans: the second and third iteration of the five launchers that split a batch over
gridDim.y (launch_filter_scans, launch_msg_laserscan, launch_msg_cloud, launch_transform_clouds,
launch_msg_merged) and offset every per-scan pointer by hand for each piece.  The entry points behind them do
not hold B to the handle's max_batch, so the session's handle reaches them.

B = 131073 tiny scans built from 251 templates and from b itself (tests/big_batch_cases.py; the conditions
that make a forgotten offset visible: tests/test_big_batch_cpu.py).  The oracles — tests/filter_oracle.py,
oracle/cdr_oracle.py and the float32 restatement of rpl_fuse.hip — run on the templates; all B scans are
compared vectorised, bit for bit.  Outputs start sentinel-filled and carry a canary row behind scan B - 1."""
import sys
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi
from tests import big_batch_cases as bb

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import cdr_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
B, K, N = bb.B, bb.K, bb.N_STRIDE
FID = bb.FID
STAMP_OFF = 4  # encapsulation header, then builtin_interfaces/Time


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def data():
    """Everything the tests share, built once and never modified."""
    ranges, inten = bb.template_scans()
    kidx = bb.scan_template_index()
    d = dict(t_ranges=ranges, t_inten=inten, t_counts=bb.template_counts(), t_pts=bb.template_clouds(),
             t_npts=bb.template_point_counts(), kidx=kidx, stamps=bb.stamps(), durs=bb.durations(),
             pose=bb.poses(kidx), sample=bb.sample_b())
    d["counts"] = d["t_counts"][kidx]
    d["npts"] = d["t_npts"][kidx]
    return d


def _dev(torch, arr):
    arr = np.ascontiguousarray(arr)
    if arr.dtype == np.uint32:  # (the same words)
        arr = arr.view(np.int32)
    return torch.from_numpy(arr).to(torch.device("cuda:0"))


def _scans_on_device(torch, d, width=N):
    """(B + 1, width) ranges / intensities (the last row is never a scan), (B + 1,) counts."""
    r = np.full((B + 1, width), 3.0, F32)
    i = np.full((B + 1, width), 3.0, F32)
    r[:B], i[:B] = d["t_ranges"][d["kidx"], :width], d["t_inten"][d["kidx"], :width]
    cnt = np.concatenate([d["counts"], [width]]).astype(np.int32)
    return _dev(torch, r), _dev(torch, i), _dev(torch, cnt)


def _struct(f):
    return abi.ScanFilter(**{k: f[k] for k, _ in abi.ScanFilter._fields_})


def _filter_settings(circular):
    from tests import filter_oracle as fo
    return _struct(fo.flt(circular=circular, **bb.FILTER))


def _check_filtered(d, ro, io, rm, want_t, rm_t, counts, width, label):
    """All B scans against the templates' oracle rows; sentinels beyond the counts and in the canary row."""
    want = want_t[d["kidx"]]
    bad = np.flatnonzero((_bits(ro[:B]) != _bits(want)).any(1))
    assert len(bad) == 0, (label, len(bad), bad[:8].tolist())
    live = np.arange(width)[None, :] < counts[:, None]
    want_i = np.where(live, d["t_inten"][d["kidx"], :width], bb.SENTINEL).astype(F32)
    bad = np.flatnonzero((_bits(io[:B]) != _bits(want_i)).any(1))
    assert len(bad) == 0, (label, "intensities", len(bad), bad[:8].tolist())
    assert np.all(ro[B] == bb.SENTINEL) and np.all(io[B] == bb.SENTINEL), (label, "canary row")
    if rm is not None:
        bad = np.flatnonzero((rm[:B] != rm_t[d["kidx"]]).any(1))
        assert len(bad) == 0, (label, "removed", len(bad), bad[:8].tolist())
        assert rm[B].tolist() == [12345, 12345], (label, "canary counts")


# ------------------------------------------------------------------ E10 on LaserScans
@pytest.mark.parametrize("sp,circular", [(1, 1), (1, 0), (0, 1), (0, 0)],
                         ids=["modeA_circular", "modeA_open", "modeB_circular", "modeB_open"])
def test_filter_laserscan_batch(gpu, data, sp, circular):
    import torch
    d = data
    d_r, d_i, d_cnt = _scans_on_device(torch, d)
    p = Params.defaults(scan_processing=sp)
    want_t, rm_t = bb.filter_templates(d["t_ranges"], d["t_counts"], sp, circular)
    for with_counts in ((True, False) if (sp, circular) == (1, 1) else (True,)):
        d_ro = torch.full_like(d_r, float(bb.SENTINEL))
        d_io = torch.full_like(d_i, float(bb.SENTINEL))
        d_rm = torch.full((B + 1, 2), 12345, dtype=torch.int32, device=d_r.device)
        gpu.filter_laserscan_batch_dev(d_r.data_ptr(), d_i.data_ptr(), N, d_cnt.data_ptr(), B, p,
                                       _filter_settings(circular), d_ro.data_ptr(), d_io.data_ptr(),
                                       d_rm.data_ptr() if with_counts else 0)
        gpu.synchronize()
        rm = d_rm.cpu().numpy()
        _check_filtered(d, d_ro.cpu().numpy(), d_io.cpu().numpy(), rm if with_counts else None, want_t, rm_t,
                        d["counts"], N, (sp, circular, with_counts))
        if not with_counts:  # d_removed = NULL: nothing is counted anywhere
            assert np.all(rm == 12345)


# ------------------------------------------------------------------ E10 on merged scans, and their messages
def _merge_struct():
    m = bb.MERGE_SPEC
    return abi.ScanMerge(m["angle_min"], m["angle_max"], m["count"], m["range_min"], m["range_max"], m["scan_time"])


@pytest.mark.parametrize("circular", [1, 0], ids=["circular", "open"])
def test_filter_merged_scans_and_their_messages(gpu, data, circular):
    """rplgpu_filter_merged_scans_dev is the beam_count == nullptr branch (k.count) with G = 131073; the
    merged-scan messages (launch_msg_merged) are then built from its output."""
    import torch
    d = data
    C12 = bb.MERGED_COUNT
    spec = _merge_struct()
    inc = abi.scan_merge_edges(spec)[1]
    assert F32(inc) == bb.merged_inc()
    d_r, d_i, _ = _scans_on_device(torch, d, C12)
    want_t, rm_t = bb.filter_merged_templates(d["t_ranges"], circular)
    counts = np.full(B, C12)
    d_ro = torch.full_like(d_r, float(bb.SENTINEL))
    d_io = torch.full_like(d_i, float(bb.SENTINEL))
    d_rm = torch.full((B + 1, 2), 12345, dtype=torch.int32, device=d_r.device)
    gpu.filter_merged_scans_dev(d_r.data_ptr(), d_i.data_ptr(), B, spec, _filter_settings(circular),
                                d_ro.data_ptr(), d_io.data_ptr(), d_rm.data_ptr())
    gpu.synchronize()
    ro, io = d_ro.cpu().numpy(), d_io.cpu().numpy()
    _check_filtered(d, ro, io, d_rm.cpu().numpy(), want_t, rm_t, counts, C12, ("merged", circular))
    if not circular:
        return
    # the messages of the filtered scans
    lay = abi.msg_laserscan_layout(len(FID), C12)
    stride = (lay.total_len + 3 + 8) & ~3  # room behind every message for a canary
    d_stamps = _dev(torch, d["stamps"])
    d_msgs = torch.full((B + 1, stride), 0xEE, dtype=torch.uint8, device=d_r.device)
    d_ml = torch.full((B + 1,), 12345, dtype=torch.int32, device=d_r.device)
    d_st = torch.zeros(B + 1, dtype=torch.int32, device=d_r.device)
    gpu.merged_laserscan_msgs_dev(d_ro.data_ptr(), d_io.data_ptr(), B, spec, FID, d_stamps.data_ptr(),
                                  d_msgs.data_ptr(), stride, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    msgs, ml, st = d_msgs.cpu().numpy(), d_ml.cpu().numpy(), d_st.cpu().numpy()
    assert np.all(ml[:B] == lay.total_len) and ml[B] == 12345 and not st.any()
    assert np.all(msgs[B] == 0xEE) and np.all(msgs[:B, lay.total_len:] == 0xEE)
    words = msgs[:B, : lay.total_len].copy().view(np.uint32)
    assert np.array_equal(words[:, STAMP_OFF // 4: STAMP_OFF // 4 + 2], d["stamps"])
    want_r = want_t[d["kidx"]]
    assert np.array_equal(words[:, lay.ranges_len_off // 4], np.full(B, C12))
    assert np.array_equal(words[:, lay.ranges_off // 4: lay.ranges_off // 4 + C12], _bits(want_r))
    assert np.array_equal(words[:, lay.intensities_len_off // 4], np.full(B, C12))
    assert np.array_equal(words[:, lay.intensities_off // 4: lay.intensities_off // 4 + C12],
                          _bits(d["t_inten"][d["kidx"], :C12]))
    m = bb.MERGE_SPEC
    meta = dict(angle_min=F32(m["angle_min"]), angle_max=F32(m["angle_max"]), angle_increment=F32(inc),
                time_increment=F32(0.0), scan_time=F32(m["scan_time"]), range_min=F32(m["range_min"]),
                range_max=F32(m["range_max"]))
    for b in d["sample"]:
        want = cdr_oracle.laserscan_msg(FID, int(b), 7 * int(b), meta, want_r[b], d["t_inten"][d["kidx"][b], :C12])
        assert msgs[b, : lay.total_len].tobytes() == want, int(b)


# ------------------------------------------------------------------ LaserScan messages
def _laserscan_scalars(sp, counts, durs):
    """angle_increment, time_increment, scan_time as publish_scan states them (fp64 divides, one rounding)."""
    c = counts.astype(np.float64)
    den = c if sp else np.maximum(c - 1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (2.0 * np.pi / den).astype(F32), (durs / den).astype(F32), durs.astype(F32)


@pytest.mark.parametrize("sp", [1, 0], ids=["modeA", "modeB"])
def test_laserscan_msgs(gpu, data, sp):
    import torch
    d = data
    d_r, d_i, d_cnt = _scans_on_device(torch, d)
    dev = d_r.device
    p = Params.defaults(range_max=40.0, scan_processing=sp)
    d_stamps, d_dur = _dev(torch, d["stamps"]), _dev(torch, d["durs"])
    stride = abi.msg_laserscan_layout(len(FID), N).total_len
    d_msgs = torch.full((B + 1, stride), 0xEE, dtype=torch.uint8, device=dev)
    d_ml = torch.full((B + 1,), 12345, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    gpu.laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), N, d_cnt.data_ptr(), B, p, FID, d_stamps.data_ptr(),
                           d_dur.data_ptr(), d_msgs.data_ptr(), stride, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    msgs, ml, st = d_msgs.cpu().numpy(), d_ml.cpu().numpy(), d_st.cpu().numpy()
    counts = d["counts"]
    assert not st.any() and ml[B] == 12345 and np.all(msgs[B] == 0xEE)
    want_len = np.array([abi.msg_laserscan_layout(len(FID), c).total_len if c else 0 for c in range(N + 1)])
    bad = np.flatnonzero(ml[:B] != want_len[counts])
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    a_inc, t_inc, s_time = _laserscan_scalars(sp, counts, d["durs"])
    r_all, i_all = d["t_ranges"][d["kidx"]], d["t_inten"][d["kidx"]]
    for c in range(N + 1):
        idx = np.flatnonzero(counts == c)
        assert len(idx) > 0
        if c == 0:
            assert np.all(msgs[idx] == 0xEE)
            continue
        lay = abi.msg_laserscan_layout(len(FID), c)
        assert np.all(msgs[idx, lay.total_len:] == 0xEE), c  # nothing behind msg_len
        words = msgs[idx, : lay.total_len].copy().view(np.uint32)
        assert np.array_equal(words[:, STAMP_OFF // 4: STAMP_OFF // 4 + 2], d["stamps"][idx]), c
        s = lay.scalars_off // 4
        assert np.array_equal(words[:, s + 2], _bits(a_inc[idx])), c
        assert np.array_equal(words[:, s + 3], _bits(t_inc[idx])), c
        assert np.array_equal(words[:, s + 4], _bits(s_time[idx])), c
        assert np.all(words[:, lay.ranges_len_off // 4] == c) and np.all(words[:, lay.intensities_len_off // 4] == c)
        assert np.array_equal(words[:, lay.ranges_off // 4: lay.ranges_off // 4 + c], _bits(r_all[idx, :c])), c
        assert np.array_equal(words[:, lay.intensities_off // 4: lay.intensities_off // 4 + c],
                              _bits(i_all[idx, :c])), c
    for b in d["sample"]:
        c = int(counts[b])
        if c == 0:
            continue
        meta = gpu.fill_meta(p, c, float(d["durs"][b]))
        want = cdr_oracle.laserscan_msg(FID, int(b), 7 * int(b), meta, r_all[b, :c], i_all[b, :c])
        assert msgs[b, : ml[b]].tobytes() == want, int(b)
    if not sp:
        return
    # a slot too small for counts >= 9: length 0 and OUT_TRUNCATED exactly there, the others as before
    small = abi.msg_laserscan_layout(len(FID), 8).total_len
    d_msgs2 = torch.full((B + 1, small), 0xEE, dtype=torch.uint8, device=dev)
    d_ml.fill_(12345)
    gpu.laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), N, d_cnt.data_ptr(), B, p, FID, d_stamps.data_ptr(),
                           d_dur.data_ptr(), d_msgs2.data_ptr(), small, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    msgs2, ml2, st2 = d_msgs2.cpu().numpy(), d_ml.cpu().numpy(), d_st.cpu().numpy()
    fits = counts <= 8
    assert np.array_equal(ml2[:B], np.where(fits, ml[:B], 0)) and ml2[B] == 12345
    assert np.array_equal(st2[:B], np.where((counts > 0) & ~fits, abi.SCAN_OUT_TRUNCATED, 0)) and st2[B] == 0
    assert np.all(msgs2[:B][~fits] == 0xEE) and np.all(msgs2[B] == 0xEE)
    assert np.array_equal(msgs2[:B][fits], msgs[:B, :small][fits])


# ------------------------------------------------------------------ clouds: messages and the rigid transform
def _clouds_on_device(torch, d, arena):
    """Per-scan regions of MAX_POINTS points ((B + 1) slots, the last a canary), or the same slots as an
    arena whose per-scan starts are a seeded permutation of the slots (not monotone in b)."""
    P = bb.MAX_POINTS
    pts = d["t_pts"][d["kidx"]]
    slots = np.full((B + 1, P, 4), 3.0, F32)
    if arena:
        slot_of = np.random.default_rng(77).permutation(B)
        assert not np.all(np.diff(slot_of) > 0)
    else:
        slot_of = np.arange(B)
    slots[slot_of] = pts
    start = (slot_of * P).astype(np.int64)
    return slots, slot_of, _dev(torch, slots), (_dev(torch, start) if arena else None)


@pytest.mark.parametrize("arena", [False, True], ids=["regions", "arena"])
def test_cloud_msgs(gpu, data, arena):
    import torch
    d = data
    P = bb.MAX_POINTS
    slots, slot_of, d_xyzi, d_start = _clouds_on_device(torch, d, arena)
    dev = d_xyzi.device
    npts = d["npts"]
    d_np = _dev(torch, np.concatenate([npts, [P]]).astype(np.int32))
    d_stamps = _dev(torch, d["stamps"])
    stride = (abi.msg_cloud_layout(len(FID), P).total_len + 3) & ~3
    d_msgs = torch.full((B + 1, stride), 0xEE, dtype=torch.uint8, device=dev)
    d_ml = torch.full((B + 1,), 12345, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    gpu.cloud_msgs_dev(d_xyzi.data_ptr(), 0 if arena else P, d_start.data_ptr() if arena else 0, d_np.data_ptr(), B,
                       FID, d_stamps.data_ptr(), d_msgs.data_ptr(), stride, d_ml.data_ptr(), d_st.data_ptr())
    gpu.synchronize()
    msgs, ml, st = d_msgs.cpu().numpy(), d_ml.cpu().numpy(), d_st.cpu().numpy()
    assert not st.any() and ml[B] == 12345 and np.all(msgs[B] == 0xEE)
    assert d_xyzi.cpu().numpy().tobytes() == slots.tobytes()  # the clouds are only read
    want_len = np.array([abi.msg_cloud_layout(len(FID), c).total_len for c in range(P + 1)])
    bad = np.flatnonzero(ml[:B] != want_len[npts])
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    pts = d["t_pts"][d["kidx"]]
    for c in range(P + 1):
        idx = np.flatnonzero(npts == c)
        lay = abi.msg_cloud_layout(len(FID), c)
        assert np.all(msgs[idx, lay.total_len:] == 0xEE), c
        head = msgs[idx, : lay.data_off].copy().view(np.uint32)
        assert np.array_equal(head[:, STAMP_OFF // 4: STAMP_OFF // 4 + 2], d["stamps"][idx]), c
        assert np.all(head[:, lay.width_off // 4] == c) and np.all(head[:, lay.row_step_off // 4] == 16 * c)
        assert np.all(head[:, lay.data_len_off // 4] == 16 * c) and np.all(msgs[idx, lay.is_dense_off] == 1)
        body = msgs[idx, lay.data_off: lay.data_off + 16 * c]
        assert body.tobytes() == np.ascontiguousarray(pts[idx, :c]).tobytes(), c
    for b in d["sample"][::4]:
        want = cdr_oracle.cloud_msg(FID, int(b), 7 * int(b), pts[b, : npts[b]])
        assert msgs[b, : ml[b]].tobytes() == want, int(b)


@pytest.mark.parametrize("arena", [False, True], ids=["regions", "arena"])
def test_transform_clouds(gpu, data, arena):
    import torch
    d = data
    P = bb.MAX_POINTS
    slots, slot_of, d_xyzi, d_start = _clouds_on_device(torch, d, arena)
    npts = d["npts"]
    d_np = _dev(torch, np.concatenate([npts, [P]]).astype(np.int32))
    pose = np.concatenate([d["pose"], np.full((1, 12), 2.0, F32)])
    d_pose = _dev(torch, pose)
    gpu.transform_clouds_dev(d_xyzi.data_ptr(), 0 if arena else P, d_start.data_ptr() if arena else 0,
                             d_np.data_ptr(), B, d_pose.data_ptr())
    gpu.synchronize()
    got = d_xyzi.cpu().numpy()
    pts = d["t_pts"][d["kidx"]]
    moved = bb.transform_points(pts, d["pose"])
    live = (np.arange(P)[None, :] < npts[:, None])[:, :, None]
    want = np.where(live, moved, pts).astype(F32)  # points at or beyond the count stay as they were
    bad = np.flatnonzero((_bits(got[slot_of]) != _bits(want)).reshape(B, -1).any(1))
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    assert _bits(got[slot_of][..., 3]).tobytes() == _bits(pts[..., 3]).tobytes()  # intensity bits untouched
    assert got[B].tobytes() == slots[B].tobytes()  # the canary slot
    assert d_pose.cpu().numpy().tobytes() == pose.tobytes()
