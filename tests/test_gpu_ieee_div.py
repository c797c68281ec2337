"""The IEEE-divide kernel instances and the divide validators.

Every kernel that divides by 4000, by the voxel leaf or by Mode A's angle_increment has a fast instance
(mul + 2 FMA, taken after k_validate_div / k_validate_idx passed on the device) and a fallback with the IEEE
divide.  On an MI355X validation passes, so the rest of the suite only ever launches the fast instances.  Here
a handle of its own runs under rplgpu_debug_force_ieee_div(7) — every launch site then behaves as if validation
had failed — and the suite's oracle comparisons are driven through it: Mode A FAST = false, the four non-debug
k_cloud_voxel<false, ...> instances, k_ror_mask<false>, merge_sample<false>, the two-step message path and the
rule that E5-inside is dropped without the fast divides.  Every result must be the bytes of the same call on
the ordinary handle, status words included, and is held to the oracle exactly as the existing tests hold the
fast instances: bit for bit for ranges, intensities, counts, cell keys, status words, plain clouds and
messages; the voxel centroids' x / y within the suite's 1e-6 m of the oracle's double-precision means (the
kernel sums in fixed point — that bound is the format's, DESIGN.md, not this test's).

The second half pins which side the ordinary suite runs (rplgpu_debug_fast_div == 7 after Mode A and voxel
calls at the leaves the suite uses) and shows that k_validate_div can say no (rplgpu_debug_validate_div with
wrong reciprocals).  test_ordinary_handle_runs_the_fast_divides prints the flags seen per leaf and
test_validator_one_ulp_reciprocal the count for a reciprocal one ulp off (it asserts nothing: whether one ulp is
caught at that exponent is a measurement, not a requirement).  Measured on an MI355X: the flags are 7 at the
leaves 0.05, 0.01 and 0.10; a reciprocal of 0 and one 2^-10 off each give 25 165 824 = 3 * 2^23 mismatches over
exponent 127, one a single ulp off gives 6."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth
from tests import fused_oracle as fz
from tests import oracle_lib
from tests import test_gpu_fused_cells as fc
from tests import test_gpu_fused_ror as fr
from tests import test_gpu_merge as tm
from tests.cases import CASES
from tests.test_gpu_msg import _unique_angles
from tests.test_gpu_parity import ROR_CASES, XYZ_TOL, _has_intensity_tie

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import cdr_oracle as cdr  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FID = "laser_frame"
AGG_PLAIN, AGG_TWO_CLASS = 1, 2
_CACHE = {}


def _lib():
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    lib.rplgpu_debug_fast_div.argtypes = [C.c_void_p]
    lib.rplgpu_debug_fast_div.restype = C.c_int32
    lib.rplgpu_debug_validate_div.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_uint32,
                                              C.POINTER(C.c_uint32)]
    lib.rplgpu_debug_validate_div.restype = C.c_int32
    return lib


def _force(h, mask):
    assert _lib().rplgpu_debug_force_ieee_div(h._h, mask) == abi.OK


def _fast_div(h):
    return _lib().rplgpu_debug_fast_div(h._h)


@pytest.fixture(scope="module")
def ieee():
    """A handle on the session's stream whose every divide is the IEEE one (mask 7)."""
    import torch

    from tests.conftest import _shared_stream
    h = RplGpu(device=0, max_samples_per_scan=32768, max_batch=64)
    h.set_stream(_shared_stream().cuda_stream)
    _force(h, 7)
    yield h
    torch.cuda.synchronize()
    h.close()


# ---- item 1: Mode A, FAST = false ---------------------------------------------------------------------------
def _laserscan_batch(h, batch, lens, p, ascend=False):
    import torch
    dev = torch.device("cuda:0")
    B, n = batch.shape
    d_nodes = torch.from_numpy(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8).copy()).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    d_r = torch.full((B, n), -7.0, dtype=torch.float32, device=dev)
    d_i = torch.full((B, n), -7.0, dtype=torch.float32, device=dev)
    d_cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    if ascend:
        h.ascend_laserscan_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_r.data_ptr(), d_i.data_ptr(),
                                     d_cnt.data_ptr(), True, d_st.data_ptr())
    else:
        h.laserscan_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_r.data_ptr(), d_i.data_ptr(),
                              d_cnt.data_ptr())
    h.synchronize()
    cnt = d_cnt.cpu().numpy()
    r, i = d_r.cpu().numpy(), d_i.cpu().numpy()
    return ([r[b, :cnt[b]] for b in range(B)], [i[b, :cnt[b]] for b in range(B)], cnt, d_st.cpu().numpy(),
            d_nodes.cpu().numpy())


def _check_mode_a(oracle, nodes, p, gr, gi, count, ctx):
    """One Mode A result against publish_scan, as test_laserscan_matches_oracle holds it."""
    wr, wi, wm = oracle.publish_scan(nodes, oracle_lib.copy_params(p), 0.125)
    assert count == wm.count, ctx
    assert gr.tobytes() == wr.tobytes(), ctx
    if not _has_intensity_tie(nodes, p):  # (a tie's winner is the unstable reference sort's: the ordinary handle decides)
        assert gi.tobytes() == wi.tobytes(), ctx
    return wr, wi, wm


@pytest.mark.parametrize("is_new", [0, 1])
@pytest.mark.parametrize("inverted", [0, 1])
@pytest.mark.parametrize("name", ["c1_like_360", "ring_8192_rot_jit", "c2_32000"])
def test_mode_a_ieee_matches_oracle_and_fast(ieee, gpu, oracle, name, inverted, is_new):
    nodes = CASES[name]
    n = len(nodes)
    p = Params.defaults(is_new_protocol=is_new, inverted=inverted, scan_processing=1, range_max=40.0)
    ctx = (name, inverted, is_new)
    # rplgpu_scan_to_laserscan
    gr, gi, gm = ieee.scan_to_laserscan(nodes, p, 0.125)
    fr_, fi_, fm = gpu.scan_to_laserscan(nodes, p, 0.125)
    wr, wi, wm = _check_mode_a(oracle, nodes, p, gr, gi, gm.count, ctx)
    assert bytes(gm) == bytes(wm) == bytes(fm) and wm.published, ctx
    assert gr.tobytes() == fr_.tobytes() and gi.tobytes() == fi_.tobytes(), ctx
    # rplgpu_laserscan_batch_dev: the scan, and the scan cut to an odd length
    batch = np.stack([nodes, nodes])
    lens = [n, n - n // 3 - 1]
    got = _laserscan_batch(ieee, batch, lens, p)
    fast = _laserscan_batch(gpu, batch, lens, p)
    for b in range(2):
        _check_mode_a(oracle, batch[b, :lens[b]], p, got[0][b], got[1][b], got[2][b], (ctx, b))
        assert got[0][b].tobytes() == fast[0][b].tobytes() and got[1][b].tobytes() == fast[1][b].tobytes(), (ctx, b)
    assert np.array_equal(got[2], fast[2])
    assert _fast_div(ieee) == 7  # what validation found is still what it reports


def test_mode_a_ieee_ascend_laserscan_batch(ieee, gpu, oracle):
    """rplgpu_ascend_laserscan_batch_dev, B = 3: the LaserScan of the raw nodes, and the ascended nodes."""
    B, n = 3, 8000
    batch = synth.make_batch(2301, B, n, jitter=3)
    batch[1] = synth.make_scan(2301, 1, n, jitter=50, rotate=True)
    lens = [n, n - 7, n - 1001]
    for inverted in (0, 1):
        p = Params.defaults(range_max=40.0, scan_processing=1, inverted=inverted)
        got = _laserscan_batch(ieee, batch, lens, p, ascend=True)
        fast = _laserscan_batch(gpu, batch, lens, p, ascend=True)
        for b in range(B):
            _check_mode_a(oracle, batch[b, :lens[b]], p, got[0][b], got[1][b], got[2][b], (inverted, b))
            assert got[0][b].tobytes() == fast[0][b].tobytes() and got[1][b].tobytes() == fast[1][b].tobytes()
        assert np.array_equal(got[2], fast[2]) and np.array_equal(got[3], fast[3]) and np.all(got[3] == 0)
        assert got[4].tobytes() == fast[4].tobytes()


@pytest.mark.parametrize("name", ["c1_like_360", "c2_32000"])
def test_mode_a_ieee_message_two_step_path(ieee, gpu, oracle, name):
    """rplgpu_scan_to_laserscan_msg into an aligned, device-addressable buffer: with the divides refused the
    call bins with Mode A FAST = false and frames with the message kernel — the bytes of the message spec
    (oracle/cdr_oracle.py over the oracle's arrays) and of the one-kernel path of the ordinary handle."""
    nodes = CASES[name]
    assert _unique_angles(nodes)  # (the oracle's arrays are then the only answer)
    need = abi.msg_laserscan_layout(len(FID), len(nodes)).total_len
    pin_i, pin_f = ieee.host_alloc(need), gpu.host_alloc(need)
    try:
        assert pin_i.ctypes.data % 4 == 0 and pin_f.ctypes.data % 4 == 0
        for kw in (dict(), dict(is_new_protocol=1, inverted=1)):
            p = Params.defaults(**{"range_max": 40.0, "scan_processing": 1, **kw})
            wr, wi, wm = oracle.publish_scan(nodes, oracle_lib.copy_params(p), 0.125)
            assert wm.published
            want = cdr.laserscan_msg(FID, 1727000000, 123456789, wm, wr, wi)
            pin_i[:] = 0xEE
            pin_f[:] = 0xEE
            got, gm = ieee.scan_to_laserscan_msg(nodes, p, 0.125, FID, 1727000000, 123456789, out=pin_i)
            fast, fm = gpu.scan_to_laserscan_msg(nodes, p, 0.125, FID, 1727000000, 123456789, out=pin_f)
            assert bytes(gm) == bytes(wm) == bytes(fm), kw
            assert got.tobytes() == want, kw
            assert fast.tobytes() == want, kw
            assert np.all(pin_i[len(got):] == 0xEE)
    finally:
        ieee.host_free(pin_i)
        gpu.host_free(pin_f)


# ---- items 2 and 3: the voxel kernel without the fast divides, E5 with the divides refused ------------------
VOXEL_FORMS = [(agg, clip, leaf) for agg in (AGG_PLAIN, AGG_TWO_CLASS) for clip in (1, 0) for leaf in (0.05, 0.01)]
VOXEL_IDS = [f"{'plain' if a == AGG_PLAIN else 'two_class'}-{'safe' if c else 'unsafe'}-leaf{l}" for a, c, l in VOXEL_FORMS]
ROR_OFF = dict(ror_enable=0)
ROR_ON = dict(ror_enable=1, ror_radius=0.10, ror_min_neighbors=2)


def _vparams(clip, leaf, **kw):
    """clip_enable = 1, range_max = 40: the host proves the cell range (SAFE); clip_enable = 0: it cannot."""
    return Params.defaults(**{**dict(clip_enable=clip, q_min=0, range_min=0.15, range_max=40.0, voxel_enable=1,
                                     voxel_leaf=leaf), **kw})


def _inputs(name):
    if ("in", name) not in _CACHE:
        if name == "batch4":  # rplgpu_cloud_batch_dev: a scan of uniformly random ranges (key bands at 1 cm), ragged
            batch = synth.make_batch(2310, 4, 8192, noise_m=0.01, jitter=2)
            batch[1] = synth.make_scan(2310, 1, 8192, kind="uniform", invalid_p=0.0)
            lens = np.array([8192, 8192, 4097, 0], np.int64)
        elif name == "arena64":  # rplgpu_cloud_arena_dev: 64 work items, the queue statistics are taken
            batch = synth.make_batch(2320, 64, 4000, noise_m=0.01, r0_range=(1.0, 25.0))
            batch[5] = synth.make_scan(2320, 5, 4000, kind="uniform", invalid_p=0.0)
            batch[9]["dist_mm_q2"] = 0
            lens = np.full(64, 4000, np.int64)
            lens[::7] -= np.arange(len(lens[::7])) * 61 + 1
            lens[3] = 0
        elif name == "fused6":  # the (3, 2) shape of test_fused_voxel_groups_match_oracle
            batch = np.stack([synth.make_scan(1003, b, 12000, noise_m=0.0, r0_range=(2.0, 12.0)) for b in range(6)])
            lens = np.full(6, 12000, np.int64)
        elif name == "tight4":  # rings of 3 .. 4 m under a radius of the order of their noise: ROR(0.015, >= 3) removes
            # 7 .. 12 % of a scan, hundreds of samples that the +-64 window leaves open (the kernel takes 8)
            batch = synth.make_batch(2330, 4, 8192, noise_m=0.01, r0_range=(3.0, 4.0))
            lens = np.full(4, 8192, np.int64)
        else:
            raise KeyError(name)
        _CACHE["in", name] = (batch, lens)
    return _CACHE["in", name]


def _wants(oracle, name, p, group=0, motion=None, pose=None, t0=None):
    """The oracle's (cloud, cells, counts, status) per work item, once per parameter set of the module."""
    key = ("w", name, group, p.clip_enable, p.voxel_leaf, p.ror_enable, p.ror_radius, p.ror_min_neighbors)
    if key not in _CACHE:
        batch, lens = _inputs(name)
        # (fr._kept's key has the E5 parameters but not ror_enable: it goes into the name)
        kept = fr._kept(oracle, f"ieee_{name}_ror{p.ror_enable}", batch, lens, p)
        if group:
            _CACHE[key] = fr._group_wants(oracle, batch, lens, p, kept, group, motion, pose, t0)
        else:
            _CACHE[key] = fr._scan_wants(oracle, batch, lens, p, kept)
    return _CACHE[key]


def _same_items(a, b, ctx):
    """Two fr._launch results: every work item's points, keys, count and status, byte for byte."""
    assert a["total"] == b["total"], ctx
    assert np.array_equal(a["npts"], b["npts"]) and np.array_equal(a["st"], b["st"]), ctx
    for i in range(len(a["npts"])):
        sa, sb, m = int(a["start"][i]), int(b["start"][i]), int(a["npts"][i])
        assert a["arena"][sa: sa + m].tobytes() == b["arena"][sb: sb + m].tobytes(), (ctx, i)
        assert a["keys"][sa: sa + m].tobytes() == b["keys"][sb: sb + m].tobytes(), (ctx, i)


def _cloud_batch(h, batch, lens, p):
    import torch
    dev = torch.device("cuda:0")
    B, n = batch.shape
    d_nodes = torch.from_numpy(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    d_xyzi = torch.full((B, n, 4), -7.0, dtype=torch.float32, device=dev)
    d_np = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    h.cloud_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_xyzi.data_ptr(), n, d_np.data_ptr(),
                      d_st.data_ptr())
    h.synchronize()
    npts, xyzi = d_np.cpu().numpy(), d_xyzi.cpu().numpy()
    return [xyzi[b, :npts[b]] for b in range(B)], d_st.cpu().numpy()


def _check_cloud(got, status, want, ctx):
    """One voxel cloud against the oracle's (cloud, cells, counts, status)."""
    cloud, cells, _, wstatus = want
    assert status == wstatus, (ctx, hex(int(status)))
    assert len(got) == len(cloud), ctx
    assert got[:, 3].tobytes() == cloud[:, 3].tobytes() and np.all(got[:, 2] == 0.0), ctx
    if len(cloud):
        assert np.max(np.abs(got[:, :2].astype(np.float64) - cloud[:, :2])) <= XYZ_TOL, ctx


def _listed(h):
    return h.debug_ror_listed()


@pytest.mark.parametrize("agg,clip,leaf", VOXEL_FORMS, ids=VOXEL_IDS)
def test_voxel_ieee_batch_and_arena(ieee, gpu, oracle, agg, clip, leaf):
    """k_cloud_voxel<false, SAFE, false, SPLIT> through rplgpu_cloud_batch_dev (B = 4, n = 8192) and
    rplgpu_cloud_arena_dev (B = 64), the arena also with E5 in both rplgpu_set_ror_mode values: the mask comes
    from k_ror_mask<false>, and E5-inside does not run (nothing is ever listed on this handle)."""
    ieee.set_voxel_aggregation(agg)
    try:
        p = _vparams(clip, leaf)
        batch, lens = _inputs("batch4")
        wants = _wants(oracle, "batch4", p)
        got, st = _cloud_batch(ieee, batch, lens, p)
        fast, fst = _cloud_batch(gpu, batch, lens, p)
        for b in range(len(batch)):
            _check_cloud(got[b], st[b], wants[b], ("batch", b))
            assert got[b].tobytes() == fast[b].tobytes() and st[b] == fst[b], ("batch", b)
        if leaf == 0.01:
            assert len(got[1]) > 7168  # (more cells than the LDS queue holds: the key bands)
        batch, lens = _inputs("arena64")
        for ror in (ROR_OFF, ROR_ON):
            p = _vparams(clip, leaf, **ror)
            wants = _wants(oracle, "arena64", p)
            for ror_mode in ((0, 1) if p.ror_enable else (0,)):
                ctx = ("arena", p.ror_enable, ror_mode)
                res = fr._launch(ieee, batch, lens, p, ror_mode=ror_mode)
                fr._check(res, wants, ctx)
                _same_items(res, fr._launch(gpu, batch, lens, p, ror_mode=ror_mode), ctx)
                assert _listed(ieee) == 0, ctx
    finally:
        ieee.set_voxel_aggregation(AGG_PLAIN)
    assert _fast_div(ieee) == 7


@pytest.mark.parametrize("agg,clip,leaf", VOXEL_FORMS, ids=VOXEL_IDS)
def test_voxel_ieee_single_scan(ieee, gpu, oracle, agg, clip, leaf):
    """rplgpu_scan_to_cloud at n = 360 and n = 32000."""
    ieee.set_voxel_aggregation(agg)
    try:
        p = _vparams(clip, leaf)
        for name in ("c1_like_360", "c2_32000"):
            nodes = CASES[name]
            key = ("single", name, clip, leaf)
            if key not in _CACHE:
                _CACHE[key] = fz.fused_grid(oracle, [nodes], p)
            got, st = ieee.scan_to_cloud(nodes, p)
            fast, fst = gpu.scan_to_cloud(nodes, p)
            _check_cloud(got, st, _CACHE[key], (name, clip, leaf))
            assert got.tobytes() == fast.tobytes() and st == fst == 0, name
    finally:
        ieee.set_voxel_aggregation(AGG_PLAIN)


def _fused_xf():
    motion, pose, t0 = fr._xf(6, 23, n=12000)
    return motion, pose, t0


def _records(cells_all, prod):
    """The records every rank wrote, in an order that does not depend on which group reserved its space first."""
    out = []
    for r, (cur, _, _) in enumerate(prod):
        rec = cells_all[r].cpu().numpy().view(np.uint32).reshape(-1, 8)[:cur]
        out.append(rec[np.lexsort(rec.T[::-1])].tobytes())
    return out


@pytest.mark.parametrize("agg,clip,leaf", VOXEL_FORMS, ids=VOXEL_IDS)
def test_voxel_ieee_fused_grid_and_cells(ieee, gpu, oracle, agg, clip, leaf, monkeypatch):
    """rplgpu_cloud_fused_voxel_dev and rplgpu_cloud_fused_cells_dev over groups of 3 (B = 6, n = 12000) with
    motion, pose2d and time offsets — the XF instances — without E5 and with it in both modes; the records of
    the cell form merge to the grid of the voxel form, and are the ordinary handle's records."""
    monkeypatch.setattr(fc, "S", 3)  # (tests/test_gpu_fused_cells.py's Case: sensors per time step)
    batch, lens = _inputs("fused6")
    motion, pose, t0 = _fused_xf()
    ieee.set_voxel_aggregation(agg)
    try:
        for ror in (ROR_OFF, ROR_ON):
            p = _vparams(clip, leaf, **ror)
            wants = _wants(oracle, "fused6", p, 3, motion, pose, t0)
            for ror_mode in ((0, 1) if p.ror_enable else (0,)):
                ctx = ("fused", p.ror_enable, ror_mode)
                res = fr._launch(ieee, batch, lens, p, group=3, motion=motion, pose=pose, t0=t0, ror_mode=ror_mode)
                fr._check(res, wants, ctx)
                _same_items(res, fr._launch(gpu, batch, lens, p, group=3, motion=motion, pose=pose, t0=t0,
                                            ror_mode=ror_mode), ctx)
                assert _listed(ieee) == 0, ctx
                # the cell form
                ieee.set_ror_mode(ror_mode)
                gpu.set_ror_mode(ror_mode)
                try:
                    ci = fc.Case(ieee, batch, p, motion=motion, pose=pose, t0=t0)
                    cf = fc.Case(gpu, batch, p, motion=motion, pose=pose, t0=t0)
                    assert ci.T == 2
                    assert ci.ref["bytes"] == cf.ref["bytes"] and list(ci.ref["status"]) == list(cf.ref["status"])
                    assert ci.ref["bytes"] == [res["arena"][res["start"][g]: res["start"][g] + res["npts"][g]].tobytes()
                                               for g in range(2)]
                    for split in ([[0, 1, 2]], [[1], [2, 0]]):
                        slot = ci.T * ci.n * 3
                        bi, bf = ci.buffers(len(split), slot), cf.buffers(len(split), slot)
                        pi = ci.produce(split, slot, *bi)
                        pf = cf.produce(split, slot, *bf)
                        assert [(c, list(nc), list(s)) for c, nc, s in pi] == [(c, list(nc), list(s)) for c, nc, s in pf]
                        assert _records(bi[0], pi) == _records(bf[0], pf), (ctx, split)
                        merged, _ = ci.merge(bi[0], slot, bi[1], bi[2], len(split))
                        assert merged["bytes"] == ci.ref["bytes"] and merged["total"] == ci.ref["total"], (ctx, split)
                        assert list(merged["status"]) == [w[3] for w in wants] == [0, 0]
                    assert _listed(ieee) == 0, ctx
                finally:
                    ieee.set_ror_mode(0)
                    gpu.set_ror_mode(0)
    finally:
        ieee.set_voxel_aggregation(AGG_PLAIN)


@pytest.mark.parametrize("agg", [AGG_PLAIN, AGG_TWO_CLASS])
def test_voxel_ieee_unsafe_far_return_sets_cell_range(ieee, gpu, oracle, agg):
    """!SAFE: tests/fused_oracle.py's far_single scan (one return at 35 m, cell 35 000 of a 1 mm grid).  Without
    E5 the return is dropped late and sets RPLGPU_SCAN_CELL_RANGE; with E5 it is removed first and nothing is
    flagged (k_ror_mask<false> in front of the range test)."""
    s = fz.range_scan("far_single")
    batch = np.stack([s, fz.range_scan("far_single", seed=3401), s])
    lens = np.full(3, fz.N_FULL, np.int64)
    ieee.set_voxel_aggregation(agg)
    try:
        for ror_enable in (0, 1):
            p = Params.defaults(**{**fz.range_params(0), "ror_enable": ror_enable})
            # (with E5: the input, parameters and cache entry of test_cell_range_counts_only_what_e5_keeps)
            kept = fr._kept(oracle, ("range", "far_single") if ror_enable else "ieee_far_single_ror0", batch, lens, p)
            wants = fr._scan_wants(oracle, batch, lens, p, kept)
            flagged = abi.SCAN_CELL_RANGE if not ror_enable else 0
            assert [wants[b][3] for b in range(3)] == [flagged] * 3
            for ror_mode in ((0, 1) if ror_enable else (0,)):
                ctx = ("far_single", ror_enable, ror_mode)
                res = fr._launch(ieee, batch, lens, p, ror_mode=ror_mode)
                fr._check(res, wants, ctx)
                _same_items(res, fr._launch(gpu, batch, lens, p, ror_mode=ror_mode), ctx)
                assert _listed(ieee) == 0, ctx
            got, st = ieee.scan_to_cloud(s, p, allow_overflow=True)
            fast, fst = gpu.scan_to_cloud(s, p, allow_overflow=True)
            _check_cloud(got, st, wants[0], ("far_single scan_to_cloud", ror_enable))
            assert got.tobytes() == fast.tobytes() and st == fst == flagged
    finally:
        ieee.set_voxel_aggregation(AGG_PLAIN)


def test_e5_inside_is_dropped_and_the_override_survives_a_new_leaf(ieee, gpu, oracle):
    """ROR(0.015 m, >= 3) on near rings with 1 cm noise: on the ordinary handle E5 runs inside the voxel kernel,
    which gives the scans up and lists them; on the forced handle the two kernels run from the start and
    nothing is listed — also at a leaf the handle has not seen, whose validation prepare_cloud runs (and
    passes) between setting the override and the launch."""
    batch, lens = _inputs("tight4")
    for leaf in (0.05, 0.02):
        p = Params.defaults(**{**fz.P_TIGHT, "voxel_leaf": leaf})
        wants = _wants(oracle, "tight4", p)
        kept = fr._kept(oracle, "ieee_tight4_ror1", batch, lens, p)
        assert all(0.05 <= 1.0 - float(k.mean()) <= 0.30 for _, _, k in kept)
        assert all(fz.open_behind_window(c, i, p.ror_radius, p.ror_min_neighbors) > fz.ROR_FEW for c, i, _ in kept)
        res = fr._launch(ieee, batch, lens, p)
        fr._check(res, wants, ("tight", leaf))
        assert res["listed"] == 0
        fast = fr._launch(gpu, batch, lens, p)
        _same_items(res, fast, ("tight", leaf))
        assert fast["listed"] > 0  # (the ordinary handle did take E5 inside: the zero above says something)
        assert _fast_div(ieee) == 7 and _fast_div(gpu) == 7


def test_ror_mask_ieee_plain_cloud(ieee, gpu, oracle):
    """k_ror_mask<false> in front of the plain cloud (voxel_enable = 0): the surviving cloud bit for bit."""
    nodes = ROR_CASES["ring_noise_4000"]
    for inverted in (0, 1):
        p = Params.defaults(inverted=inverted, clip_enable=1, range_min=0.15, range_max=40.0, ror_enable=1,
                            ror_radius=0.10, ror_min_neighbors=2)
        want = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(p))
        base = oracle.scan_to_cloud(nodes, oracle_lib.copy_params(Params.defaults(clip_enable=1, range_max=40.0)))
        assert 0 < len(want) < len(base)  # (E5 removes something here)
        got, st = ieee.scan_to_cloud(nodes, p)
        fast, fst = gpu.scan_to_cloud(nodes, p)
        assert st == fst == 0 and got.tobytes() == want.tobytes() == fast.tobytes()
        assert _listed(ieee) == 0


# ---- item 4: merge_sample<false> ----------------------------------------------------------------------------
def test_merge_ieee_sensors_with_poses(ieee, gpu, oracle):
    """The group 2, motion_t0 case of tests/test_gpu_merge.py's test_sensors_with_poses (n = 6000)."""
    group, n, G = 2, 6000, 2
    B = group * G
    batch = synth.make_batch(910 + group, B, n, noise_m=0.01, r0_range=(1.0, 12.0))
    rng = np.random.default_rng(group)
    pose2d = tm._poses(rng, B)
    motion = tm._motion(rng, B, n)
    t0 = rng.uniform(-0.05, 0.05, B).astype(np.float32)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    spec = tm._spec(1440)
    r, i, hit = tm._check(oracle, ieee, batch, group, p, spec, motion, pose2d, t0)
    fr_, fi_, fhit, fst = tm._run(gpu, batch, group, p, spec[1], motion, pose2d, t0)
    assert r.tobytes() == fr_.tobytes() and i.tobytes() == fi_.tobytes()
    assert np.array_equal(hit, fhit) and np.all(fst == 0) and np.all(hit > 0)


def test_merge_ieee_constructed_ties(ieee, oracle):
    """tests/test_gpu_merge.py's constructed case (points on e_0, the wrap sliver, the origin, r2 ties), its
    input and its assertions, on the forced handle."""
    tm.test_constructed_points_edges_wrap_origin_ties(ieee, oracle)


# ---- item 5: partial masks, and clearing ------------------------------------------------------------------
def test_partial_masks_and_clear(ieee, gpu, oracle):
    """Mask 1, 2 and 4 alone on a voxel case with E5 and a Mode A case, against the oracle: mask 2 leaves
    k_ror_mask its fast divide by 4000 under a voxel kernel without (fast_d4000 = 1, fast_div = 0), mask 1
    takes both, mask 4 touches Mode A only, which needs both of its divides.  Mask 0 on the same handle gives the
    ordinary handle's bytes again (every mask does: that is the point of the validation)."""
    lib = _lib()
    nodes = CASES["ring_8192_rot_jit"]
    pv = _vparams(1, 0.05, **ROR_ON)  # (8192 samples: E5 runs inside the voxel kernel wherever fast_div holds)
    pa = Params.defaults(scan_processing=1, range_max=40.0)
    want_v = fz.fused_grid(oracle, [nodes], pv)
    fast_v, fast_st = gpu.scan_to_cloud(nodes, pv)
    fast_a = gpu.scan_to_laserscan(nodes, pa, 0.125)
    try:
        assert lib.rplgpu_debug_force_ieee_div(ieee._h, 8) == abi.ERR_INVALID_ARG
        for mask in (1, 2, 4, 0):
            _force(ieee, mask)
            got, st = ieee.scan_to_cloud(nodes, pv)
            _check_cloud(got, st, want_v, ("mask", mask))
            assert got.tobytes() == fast_v.tobytes() and st == fast_st == 0, mask
            gr, gi, gm = ieee.scan_to_laserscan(nodes, pa, 0.125)
            _, _, wm = _check_mode_a(oracle, nodes, pa, gr, gi, gm.count, ("mask", mask))
            assert bytes(gm) == bytes(wm) == bytes(fast_a[2]), mask
            assert gr.tobytes() == fast_a[0].tobytes() and gi.tobytes() == fast_a[1].tobytes(), mask
            assert _fast_div(ieee) == 7, mask
    finally:
        _force(ieee, 7)


# ---- item 6: which side the ordinary suite runs -------------------------------------------------------------
def test_ordinary_handle_runs_the_fast_divides(gpu):
    """After a Mode A call and a voxel call at each leaf the suite and the benchmark use, validation has
    accepted the divide by 4000, by the leaf and Mode A's index divide: the rest of the suite tests, and
    bench.py times, the fast instances."""
    nodes = CASES["c1_like_360"]
    seen = {}
    for leaf in (0.05, 0.01, 0.10):
        r, _, m = gpu.scan_to_laserscan(nodes, Params.defaults(scan_processing=1, range_max=40.0), 0.1)
        assert m.published and len(r)
        cloud, st = gpu.scan_to_cloud(nodes, _vparams(1, leaf))
        assert st == 0 and len(cloud)
        seen[leaf] = _fast_div(gpu)
    print("rplgpu_debug_fast_div per leaf:", seen)
    assert seen == {0.05: 7, 0.01: 7, 0.10: 7}


# ---- item 7: the validator can fail -------------------------------------------------------------------------
def _mismatches(h, d, rd, e_lo, e_hi):
    n = C.c_uint32(0xFFFFFFFF)
    assert _lib().rplgpu_debug_validate_div(h._h, float(d), float(rd), e_lo, e_hi, C.byref(n)) == abi.OK
    return int(n.value)


def test_validator_accepts_the_exact_reciprocal(gpu):
    d = F32(0.05)
    assert _mismatches(gpu, d, F32(1.0) / d, 127, 127) == 0
    d = F32(4000.0)
    assert _mismatches(gpu, d, F32(1.0) / d, 127, 159) == 0


def test_validator_rejects_a_wrong_reciprocal(gpu):
    """Exponent 127 only: 2^23 operands, three compared quotients each."""
    d = F32(0.05)
    rd = F32(1.0) / d
    zero = _mismatches(gpu, d, F32(0.0), 127, 127)
    off = _mismatches(gpu, d, F32(rd * F32(1.0 + 2.0 ** -10)), 127, 127)
    print("k_validate_div mismatches: rd = 0:", zero, " rd * (1 + 2^-10):", off)
    assert zero > 2 ** 23   # every quotient is 0
    assert off > 2 ** 23    # the corrected quotient is ~2^-20 off, about 8 ulp
    # the count is cleared per call, and the entry point's own argument checks
    assert _mismatches(gpu, d, rd, 127, 127) == 0
    lib, n, d, rd = _lib(), C.c_uint32(5), float(d), float(rd)
    assert lib.rplgpu_debug_validate_div(gpu._h, d, rd, 128, 127, C.byref(n)) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_debug_validate_div(gpu._h, d, rd, 127, 255, C.byref(n)) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_debug_validate_div(gpu._h, d, rd, 127, 127, None) == abi.ERR_INVALID_ARG
    assert n.value == 5


def test_validator_one_ulp_reciprocal(gpu):
    """A reciprocal one ulp above RN(1 / 0.05f): how many of the 3 * 2^23 quotients differ is recorded, not
    asserted (6 on an MI355X: the two FMA steps absorb almost all of a one-ulp error at this exponent)."""
    d = F32(0.05)
    rd = np.nextafter(F32(1.0) / d, F32(np.inf))
    assert rd.dtype == np.float32 and rd != F32(1.0) / d
    print("k_validate_div mismatches with rd one ulp above RN(1/0.05f), exponent 127:", _mismatches(gpu, d, rd, 127, 127))
