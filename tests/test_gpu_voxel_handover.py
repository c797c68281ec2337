"""The hand-over from one scan to the next in k_cloud_voxel (csrc/rpl_voxel.hip) against the CPU oracle.

Between the end of one scan's emit and the next scan's first aggregated block the kernel
  * draws the next item while it stores the finished item's words, behind ONE barrier,
  * sets the item up and pops its first band in one step,
  * loads the wave's first raw pairs through a resource over the scan's SLOT before the scan's length has
    arrived, and zeroes what lies at or beyond the length afterwards,
  * reserves the scan's cells in the arena under the cell-head step of phase R.
None of it may change a result.  Every cloud here is compared with the oracle (orc_batch_cloud_check with the
batch's own lengths, orc_cloud_pipeline, tests/fused_oracle.py for a group), never with the library's own
output: cell count, count | intensity words and z bit for bit, x / y within the 1e-6 m the oracle's fp64
centroids are held to everywhere (tests/test_gpu_parity.py).

The inputs: slots of 4224 nodes holding a scan of every length around the speculative prologue (16 waves x 2
blocks x 128 samples = 4096: one sample, one block, the whole prologue, one block more, either side of each), the
slot's tail beyond the length filled with nodes that would make cells if read; one scan alone (a workgroup per
item, no draw) and 600 scans of mixed lengths (more items than workgroups: drawn from the counter)."""
import ctypes as C
import functools

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import fused_oracle, oracle_lib

pytestmark = pytest.mark.gpu

NS = 4224
LENS = (0, 1, 2, 123, 124, 125, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097, 4224)
B_MIX = 600
XYZ_TOL = 1e-6

P_PLAIN = dict(clip_enable=1, range_min=0.15, range_max=40.0, voxel_enable=1, voxel_leaf=0.05)
P_ROR = {**P_PLAIN, "ror_enable": 1, "ror_radius": 0.10, "ror_min_neighbors": 2}
# name -> (parameters, block aggregation (1 plain, 2 two-class), E5 mode (0 inside, 1 two kernels), group)
INSTANCES = {
    "plain": (P_PLAIN, 1, None, 0),
    "quality": ({**P_PLAIN, "q_min": 48}, 1, None, 0),
    "keepmask": (P_ROR, 1, 1, 0),
    "ror_inside": (P_ROR, 1, 0, 0),
    "two_class": (P_PLAIN, 2, None, 0),
    "group3": (P_PLAIN, 1, None, 3),
}


@functools.lru_cache(maxsize=None)
def _mixed():
    """(batch (600, 4224) of FULL slots, lens): scan s uses the first lens[s] nodes of its slot; every third
    scan carries 1 cm of range noise (blocks the two-class instance splits).  lens[s] = LENS[7 s mod 16]:
    any 16 consecutive scans hold every length once, neighbours differ, and the three scans of a group too."""
    batch = synth.make_batch(4100, B_MIX, NS, r0_range=(1.0, 12.0))
    batch[2::3] = synth.make_batch(4101, B_MIX, NS, r0_range=(1.0, 12.0), noise_m=0.01)[2::3]
    lens = np.array([LENS[(7 * s) % len(LENS)] for s in range(B_MIX)], np.int32)
    for s in range(len(LENS)):  # the tail would make cells if it were read
        assert lens[s] == NS or np.count_nonzero(batch[s]["dist_mm_q2"][lens[s]:] >= 4000) > 0
    batch.setflags(write=False)
    lens.setflags(write=False)
    return batch, lens


@functools.lru_cache(maxsize=None)
def _plain_refs():
    """The oracle's cloud of every scan of the mixed batch under P_PLAIN (computed once, never written to)."""
    orc = oracle_lib.load_oracle()
    batch, lens = _mixed()
    op = oracle_lib.copy_params(Params.defaults(**P_PLAIN))
    refs = [orc.cloud_pipeline(batch[s][:lens[s]], op)[0] for s in range(B_MIX)]
    for r in refs:
        r.setflags(write=False)
    return refs


def _launch(gpu, batch, lens, p, form="arena", cap=None, group=0):
    """One launch.  Returns (points (m, 4) float32 — 12-byte points widened with z = 0 —, start, npts, status,
    cursor or None)."""
    import torch
    dev = torch.device("cuda:0")
    B, n = batch.shape
    d_nodes = torch.from_numpy(np.array(batch).view(np.uint8).reshape(B, n * 8)).to(dev)  # (a writable copy)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    items = B if not group else (B + group - 1) // group
    d_np = torch.full((items,), -1, dtype=torch.int32, device=dev)
    d_st = torch.full((items,), -1, dtype=torch.int32, device=dev)
    if form == "legacy":
        d_xyzi = torch.full((B, n, 4), -1.0, dtype=torch.float32, device=dev)
        gpu.cloud_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_xyzi.data_ptr(), n, d_np.data_ptr(),
                            d_st.data_ptr())
        gpu.synchronize()
        pts, start, cursor = d_xyzi.cpu().numpy().reshape(B * n, 4), np.arange(B, dtype=np.int64) * n, None
    else:
        cap = B * n if cap is None else cap
        width = 3 if form == "xyi" else 4
        d_arena = torch.full((max(cap, 1) + 16, width), -1.0, dtype=torch.float32, device=dev)
        d_cur = torch.full((1,), 123, dtype=torch.int64, device=dev)
        d_start = torch.full((items,), -1, dtype=torch.int64, device=dev)
        args = (d_arena.data_ptr(), cap, d_cur.data_ptr(), d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())
        if group:
            gpu.cloud_fused_voxel_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, group, p, 0, 0, *args)
        elif form == "xyi":
            gpu.cloud_arena_xyi_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, *args)
        else:
            gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, *args)
        gpu.synchronize()
        raw = d_arena.cpu().numpy()
        assert np.all(raw[cap:] == -1.0), "written past the capacity"
        if form == "xyi":
            pts = np.zeros((len(raw), 4), np.float32)
            pts[:, 0], pts[:, 1], pts[:, 3] = raw[:, 0], raw[:, 1], raw[:, 2]
        else:
            pts = raw
        start, cursor = d_start.cpu().numpy(), int(d_cur.item())
    npts, st = d_np.cpu().numpy().astype(np.int64), d_st.cpu().numpy()
    assert npts.min() >= 0 and st.min() >= 0 and start.min() >= 0, "an item was never published"
    return pts, start.astype(np.int64), npts, st, cursor


def _configured(gpu, agg, ror_mode):
    class _Ctx:
        def __enter__(self):
            gpu.set_voxel_aggregation(agg)
            if ror_mode is not None:
                gpu.set_ror_mode(ror_mode)

        def __exit__(self, *exc):
            gpu.set_voxel_aggregation(0)
            gpu.set_ror_mode(0)
    return _Ctx()


def _same_cloud(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if len(want):
        assert np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2])) <= XYZ_TOL, what
        assert np.all(got[:, 2] == 0.0), what
        assert got[:, 3].tobytes() == want[:, 3].tobytes(), what


def _oracle_check(oracle, batch, lens, p, pts, start, npts):
    """orc_batch_cloud_check (oracle_lib.Oracle.batch_cloud_check) with the batch's OWN lengths: every scan's
    first lens[b] nodes through the cloud oracle on the host threads, compared with the device's cells."""
    B, n = batch.shape
    nodes = np.ascontiguousarray(batch)
    lens32 = np.ascontiguousarray(lens, np.uint32)
    pts = np.ascontiguousarray(pts, np.float32)
    start64 = np.ascontiguousarray(start, np.uint64)
    npts32 = np.ascontiguousarray(npts, np.uint32)
    res = np.zeros((B, 4), np.uint32)
    op = oracle_lib.copy_params(p)
    bad = int(oracle.lib.orc_batch_cloud_check(nodes.ctypes.data, n, lens32.ctypes.data, B, C.byref(op),
                                               pts.ctypes.data, start64.ctypes.data, npts32.ctypes.data, None,
                                               fused_oracle.threads(), res.ctypes.data))
    wrong = np.nonzero((res[:, 1] != 0) | (res[:, 2] != 0))[0]
    assert bad == 0, (wrong[:8], np.asarray(lens)[wrong[:8]], res[wrong[:8]])
    assert np.array_equal(res[:, 0].astype(np.int64), npts)
    worst = float(res[:, 3].copy().view(np.float32).max()) if B else 0.0
    assert worst <= XYZ_TOL, worst
    return res[:, 0].astype(np.int64)


def _check_groups(oracle, batch, lens, p, group, pts, start, npts, st):
    B = len(batch)
    assert int(st.max()) == 0
    for g in range(len(npts)):
        scans = [batch[s][:lens[s]] for s in range(g * group, min(B, (g + 1) * group))]
        want, _, _, status = fused_oracle.fused_grid(oracle, scans, p)
        assert status == 0
        _same_cloud(pts[start[g]:start[g] + npts[g]], want, ("group", g))


def _bookkeeping(start, npts, cursor):
    """The reservations tile [0, cursor) without gaps or overlaps; an item without cells reserves nothing and
    keeps the documented start of 0."""
    assert cursor == int(npts.sum())
    nz = np.nonzero(npts)[0]
    order = nz[np.argsort(start[nz], kind="stable")]
    assert np.array_equal(np.cumsum(npts[order]) - npts[order], start[order])
    assert np.all(start[npts == 0] == 0)


@pytest.mark.parametrize("name", list(INSTANCES))
def test_one_scan_alone_every_length(gpu, oracle, name):
    """A launch of ONE work item (a workgroup per item: no draw, the first item's setup only) for every length."""
    kw, agg, ror_mode, group = INSTANCES[name]
    p = Params.defaults(**kw)
    batch, lens = _mixed()
    per = group or 1
    n_items = (len(LENS) + per - 1) // per  # (groups of 3: the scans 0 .. 17, every length at least once)
    clouds, cells = [], []
    with _configured(gpu, agg, ror_mode):
        for i in range(n_items):
            sl = slice(i * per, (i + 1) * per)
            pts, start, npts, st, cursor = _launch(gpu, batch[sl], lens[sl], p, group=group)
            assert int(st[0]) == 0 and cursor == int(npts[0]) and int(start[0]) == 0
            clouds.append(pts[:npts[0]])
            cells.append(int(npts[0]))
    cells = np.array(cells, np.int64)
    pts = np.concatenate(clouds + [np.zeros((1, 4), np.float32)])
    start = np.cumsum(cells) - cells
    if group:
        _check_groups(oracle, batch[:n_items * per], lens, p, group, pts, start, cells, np.zeros(n_items, np.int32))
    else:
        _oracle_check(oracle, batch[:n_items], lens[:n_items], p, pts, start, cells)


@pytest.mark.parametrize("name", list(INSTANCES))
def test_mixed_lengths_drawn_from_the_counter(gpu, oracle, name):
    """600 scans of mixed lengths in one launch: more items than workgroups, so every workgroup hands over
    from a scan of one length to a scan of another, drawn from the counter."""
    kw, agg, ror_mode, group = INSTANCES[name]
    p = Params.defaults(**kw)
    batch, lens = _mixed()
    with _configured(gpu, agg, ror_mode):
        pts, start, npts, st, cursor = _launch(gpu, batch, lens, p, group=group)
        listed = gpu.debug_ror_listed() if name == "ror_inside" else 0
    assert listed == 0  # (clean rings: E5 is settled inside the pass, the instance under test)
    assert int(st.max()) == 0
    _bookkeeping(start, npts, cursor)
    if group:
        _check_groups(oracle, batch, lens, p, group, pts, start, npts, st)
    else:
        cells = _oracle_check(oracle, batch, lens, p, pts, start, npts)
        assert cells[lens == NS].min() > 0 and np.all(cells[lens == 0] == 0)


@pytest.mark.parametrize("form", ["arena", "xyi", "legacy"])
def test_arena_bookkeeping_in_every_form(gpu, form):
    """The mixed batch in the arena, 12-byte and per-scan-region forms: every scan's cells are the oracle's,
    the cursor is the sum of n_points, the reservations tile [0, cursor), an empty scan between two normal
    scans starts at 0."""
    p = Params.defaults(**P_PLAIN)
    batch, lens = _mixed()
    refs = _plain_refs()
    with _configured(gpu, 1, None):
        pts, start, npts, st, cursor = _launch(gpu, batch, lens, p, form=form)
    assert int(st.max()) == 0
    assert np.array_equal(npts, [len(r) for r in refs])
    if form != "legacy":
        _bookkeeping(start, npts, cursor)
        empty = np.nonzero(npts == 0)[0]
        assert any(0 < s < B_MIX - 1 and npts[s - 1] > 0 and npts[s + 1] > 0 for s in empty)
    for s in range(B_MIX):
        _same_cloud(pts[start[s]:start[s] + npts[s]], refs[s], (form, s, int(lens[s])))


@pytest.mark.parametrize("form", ["arena", "xyi"])
def test_arena_capacity_below_the_total(gpu, form):
    """include/rplgpu.h: the cursor ends up as the total number of points; points beyond the capacity are
    dropped and flagged RPLGPU_SCAN_OUT_TRUNCATED, the count is clamped."""
    p = Params.defaults(**P_PLAIN)
    batch, lens = _mixed()
    refs = _plain_refs()
    cells = np.array([len(r) for r in refs], np.int64)
    total = int(cells.sum())
    cap = total // 2
    with _configured(gpu, 1, None):
        pts, start, npts, st, cursor = _launch(gpu, batch, lens, p, form=form, cap=cap)
    assert cursor == total
    _bookkeeping(start, cells, total)  # (every scan reserved all of its cells, wherever they fell)
    cut = 0
    for s in range(B_MIX):
        kept = int(min(max(cap - start[s], 0), cells[s]))
        assert npts[s] == kept, (s, npts[s], kept)
        assert int(st[s]) == (abi.SCAN_OUT_TRUNCATED if kept < cells[s] else 0), (s, st[s])
        cut += kept < cells[s]
        _same_cloud(pts[start[s]:start[s] + kept], refs[s][:kept], (form, s))
    assert cut > 0


def test_hand_over_behind_the_band_path(gpu, oracle):
    """Scans that leave the single-band path between short clean ones: 8192 uniformly random ranges (more run
    records than the LDS queue's 7168: bands cut from the record store) and a ring of 4096 samples across
    more than 2048 rows of 2 cm cells (phase R refuses the band: bisected).  The scan behind each starts from
    the item setup alone."""
    n = 8192
    B = 300
    kw = {**P_PLAIN, "voxel_leaf": 0.02}
    p = Params.defaults(**kw)
    short, short_lens = _mixed()
    batch = np.zeros((B, n), abi.NODE_DTYPE)
    batch[:, :NS] = short[:B]
    lens = np.array(short_lens[:B], np.int32)
    big = {40: "uniform", 41: "rows", 150: "uniform", 151: "uniform", 290: "rows"}
    for s, kind in big.items():
        if kind == "uniform":
            batch[s] = synth.make_scan(4200, s, n, kind="uniform", invalid_p=0.0)
            lens[s] = n
        else:
            ring = synth.make_scan(4201, s, 4096, invalid_p=0.0)
            ring["dist_mm_q2"] = 36 * 4000
            batch[s, :4096] = ring
            lens[s] = 4096
    op = oracle_lib.copy_params(p)
    for s, kind in big.items():  # the regimes, from the oracle alone
        _, cells, _ = oracle.cloud_pipeline(batch[s][:lens[s]], op)
        if kind == "uniform":
            assert len(cells) > 7168
        else:
            assert len(cells) <= 7168 - 64 and int(cells[:, 1].max()) - int(cells[:, 1].min()) + 1 > 2048
    with _configured(gpu, 1, None):
        pts, start, npts, st, cursor = _launch(gpu, batch, lens, p)
    assert int(st.max()) == 0
    _bookkeeping(start, npts, cursor)
    _oracle_check(oracle, batch, lens, p, pts, start, npts)


def test_a_workgroup_per_item_and_one_item_more(gpu):
    """n_cu scans: one item per workgroup, nothing is drawn.  n_cu + 1: the first launch size with a draw."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert 0 < n_cu < B_MIX
    p = Params.defaults(**P_PLAIN)
    batch, lens = _mixed()
    refs = _plain_refs()
    with _configured(gpu, 1, None):
        for B in (n_cu - 1, n_cu, n_cu + 1):
            pts, start, npts, st, cursor = _launch(gpu, batch[:B], lens[:B], p)
            assert int(st.max()) == 0
            _bookkeeping(start, npts, cursor)
            for s in range(B):
                _same_cloud(pts[start[s]:start[s] + npts[s]], refs[s], (B, s, int(lens[s])))
