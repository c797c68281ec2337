"""E5 (radius outlier removal) at the full scan size and E8 + E5 (one grid per group of sensors) against
the CPU oracle, on inputs for which the oracle itself removes points (tests/fused_oracle.py: settled inside
the kernel, on the radius, given up and redone, mixed groups) — per-scan clouds, the fused grid, the cell
records and their merge, and the cell-range status with E5 on.  Every comparison: number of cells, every
(iy, ix) key in the oracle's order, intensity bits, z == 0, max |dxy| <= 1e-6 m, status, gap-free arena,
cursor = sum of counts; in RPLGPU_ROR_INSIDE and RPLGPU_ROR_TWO_KERNELS.  The regime conditions of the
inputs are checked without a GPU in tests/test_fused_oracle_cpu.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import fused_oracle as fz

pytestmark = pytest.mark.gpu

XYZ_TOL = 1e-6
N = fz.N_FULL
S = 8
_CACHE = {}


def _kept(oracle, name, batch, lens, p):
    """scans_kept of a named input, once per (E1, E5) parameter set of the session."""
    key = (name, p.clip_enable, p.q_min, p.range_min, p.range_max, p.ror_radius, p.ror_min_neighbors)
    if key not in _CACHE:
        _CACHE[key] = fz.scans_kept(oracle, [batch[b, :lens[b]] for b in range(len(batch))], p)
    return _CACHE[key]


def _input(oracle, name):
    if ("in", name) not in _CACHE:
        if name == "settled":
            batch = fz.settled_batch(fz.SETTLED_SEED, fz.SETTLED_B, N)[0]
        elif name == "radius":
            batch, targets = fz.radius_batch(oracle, fz.RADIUS_SEED, N, Params.defaults(**fz.P_C5))
            _CACHE["targets"] = targets
        elif name == "redone":
            batch = fz.redone_batch(fz.REDONE_SEED, fz.REDONE_B, N)
        else:
            batch, lens = fz.mixed_batch(fz.MIXED_SEED, N)
            _CACHE["in", name] = (batch, lens)
            return batch, lens
        _CACHE["in", name] = (batch, np.full(len(batch), N, np.int64))
    return _CACHE["in", name]


def _xf(B, seed, n=N):
    rng = np.random.default_rng(seed)
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                       for _ in range(B)]).astype(np.float32)
    ang = rng.uniform(-3, 3, B)
    pose = np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, B), np.sin(ang), np.cos(ang),
                     rng.uniform(-2, 2, B)], 1).astype(np.float32)
    t0 = rng.uniform(-0.05, 0.0, B).astype(np.float32)
    return motion, pose, t0


def _launch(gpu, batch, lens, p, group=0, motion=None, pose=None, t0=None, ror_mode=0):
    import torch
    dev = torch.device("cuda:0")
    B, n = batch.shape
    d_nodes = torch.from_numpy(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    items = B if not group else (B + group - 1) // group
    cap = B * n
    d_arena = torch.full((cap, 4), -7.0, dtype=torch.float32, device=dev)
    d_keys = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
    d_start = torch.zeros(items, dtype=torch.int64, device=dev)
    d_np = torch.full((items,), -1, dtype=torch.int32, device=dev)
    d_st = torch.full((items,), -1, dtype=torch.int32, device=dev)
    dv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_mo, d_po, d_t0 = dv(motion), dv(pose), dv(t0)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    gpu.set_ror_mode(ror_mode)
    gpu.set_cell_key_output(d_keys.data_ptr())
    gpu.set_scan_time_offsets_dev(ptr(d_t0))
    try:
        if group:
            gpu.cloud_fused_voxel_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, group, p, ptr(d_mo), ptr(d_po),
                                      d_arena.data_ptr(), cap, d_cur.data_ptr(), d_start.data_ptr(),
                                      d_np.data_ptr(), d_st.data_ptr())
        else:
            gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_arena.data_ptr(), cap,
                                d_cur.data_ptr(), d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
        listed = gpu.debug_ror_listed() if (ror_mode == 0 and p.ror_enable) else None
    finally:
        gpu.set_scan_time_offsets_dev(0)
        gpu.set_cell_key_output(0)
        gpu.set_ror_mode(0)
    total = int(d_cur.item())
    return dict(arena=d_arena[:total].cpu().numpy(), keys=d_keys[:total].cpu().numpy().view(np.uint32),
                start=d_start.cpu().numpy(), npts=d_np.cpu().numpy().astype(np.int64), st=d_st.cpu().numpy(),
                total=total, listed=listed)


def _check(res, wants, ctx, only=None):
    """Every work item (or the items `only`) against its (cloud, cells, counts, status)."""
    npts, start, st = res["npts"], res["start"], res["st"]
    assert npts.min() >= 0 and st.min() >= 0, (ctx, "an item was never published")
    assert res["total"] == int(npts.sum()), ctx
    nz = np.nonzero(npts)[0]
    order = nz[np.argsort(start[nz], kind="stable")]
    assert np.array_equal(np.cumsum(npts[order]) - npts[order], start[order]), (ctx, "gaps in the arena")
    worst = 0.0
    for i in (range(len(wants)) if only is None else only):
        want, cells, _, status = wants[i]
        c = (ctx, "item", i)
        assert int(st[i]) == status, (c, hex(int(st[i])))
        assert int(npts[i]) == len(want), (c, int(npts[i]), len(want))
        got = res["arena"][start[i]: start[i] + npts[i]]
        assert np.array_equal(res["keys"][start[i]: start[i] + npts[i]], fz.cell_keys(cells)), c
        assert got[:, 3].tobytes() == want[:, 3].tobytes(), c
        assert np.all(got[:, 2] == 0.0), c
        if len(want):
            worst = max(worst, float(np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2]))))
    print(ctx, "items", len(wants), "max |dxy|", worst)
    assert worst <= XYZ_TOL, (ctx, worst)


def _scan_wants(oracle, batch, lens, p, kept, only=None):
    return {b: fz.fused_grid(oracle, [batch[b, :lens[b]]], p, kept=[kept[b]])
            for b in (range(len(batch)) if only is None else only)}


def _group_wants(oracle, batch, lens, p, kept, group, motion=None, pose=None, t0=None):
    out = []
    for g in range(0, len(batch), group):
        sl = slice(g, min(len(batch), g + group))
        out.append(fz.fused_grid(oracle, [batch[b, :lens[b]] for b in range(sl.start, sl.stop)], p,
                                 None if motion is None else motion[sl], None if pose is None else pose[sl],
                                 None if t0 is None else t0[sl], kept=kept[sl]))
    return out


# ---- per-scan clouds (rplgpu_cloud_arena_dev) ---------------------------------------------------------------
@pytest.mark.parametrize("q_min", fz.Q_MINS)
def test_per_scan_settled_inside_the_kernel(gpu_mode, oracle, q_min):
    """Input 1: the oracle removes 1 .. 8 points per scan and keeps triples only the +-64 window or the
    whole-scan count can see; nothing is listed."""
    batch, lens = _input(oracle, "settled")
    p = Params.defaults(**{**fz.P_C5, "q_min": q_min})
    kept = _kept(oracle, "settled", batch, lens, p)
    wants = _scan_wants(oracle, batch, lens, p, kept)
    assert all(1 <= int((~k).sum()) <= 8 for _, _, k in kept)
    for ror_mode in (0, 1):
        res = _launch(gpu_mode, batch, lens, p, ror_mode=ror_mode)
        _check(res, wants, ("settled", gpu_mode.mode_name, q_min, ror_mode))
        if ror_mode == 0:
            assert res["listed"] == 0, res["listed"]


@pytest.mark.parametrize("q_min", fz.Q_MINS)
def test_per_scan_on_the_radius(gpu_mode, oracle, q_min):
    """Input 2: two radii one float32 ulp apart decide whether a constructed return survives (its k-th
    neighbour's d2 lies between r_lo^2 and r_hi^2; on the odd scans d2 == r_hi^2 exactly)."""
    batch, lens = _input(oracle, "radius")
    targets = _CACHE["targets"]
    def params(b, which):
        return Params.defaults(**{**fz.P_C5, "q_min": q_min, "ror_radius": targets[b][which]})

    def want(bw):
        b, which = bw
        k = fz.scan_kept(oracle, batch[b], params(b, which))
        at = np.flatnonzero(k[1] == targets[b]["i"])
        assert bool(k[2][at[0]]) == (which == "r_hi")  # (the regime, once more where it is used)
        return {b: fz.fused_grid(oracle, [batch[b]], params(b, which), kept=[k])}

    todo = [(b, w) for b in range(len(targets)) for w in ("r_lo", "r_hi") if ("radius", b, w, q_min) not in _CACHE]
    with ThreadPoolExecutor(fz.threads()) as ex:
        for (b, w), val in zip(todo, ex.map(want, todo)):
            _CACHE["radius", b, w, q_min] = val
    for b, t in enumerate(targets):
        for which in ("r_lo", "r_hi"):
            p = params(b, which)
            key = ("radius", b, which, q_min)
            for ror_mode in (0, 1):
                res = _launch(gpu_mode, batch, lens, p, ror_mode=ror_mode)
                _check(res, _CACHE[key], ("radius", gpu_mode.mode_name, q_min, b, which, t["exact"], ror_mode), only=[b])


@pytest.mark.parametrize("q_min", fz.Q_MINS)
def test_per_scan_given_up_and_redone(gpu_mode, oracle, q_min):
    """Input 3: ROR(0.015 m, >= 3) removes 5 .. 30 % of every scan; the inside pass lists every scan and the
    two kernels (k_ror_mask over the listed items, the masked voxel kernel) redo it."""
    batch, lens = _input(oracle, "redone")
    p = Params.defaults(**{**fz.P_TIGHT, "q_min": q_min})
    kept = _kept(oracle, "redone", batch, lens, p)
    wants = _scan_wants(oracle, batch, lens, p, kept)
    for ror_mode in (0, 1):
        res = _launch(gpu_mode, batch, lens, p, ror_mode=ror_mode)
        _check(res, wants, ("redone", gpu_mode.mode_name, q_min, ror_mode))
        if ror_mode == 0:
            assert res["listed"] == len(batch), res["listed"]


# ---- the fused grid (rplgpu_cloud_fused_voxel_dev) ----------------------------------------------------------
def test_fused_grid_at_the_bench_shape(gpu_mode, oracle):
    """Exactly what bench.py times as c5.fused_grid — group 8, 32 000 samples, the seed + 5 batch with 1 cm
    noise, its motion / pose draws, ROR(0.10, >= 2) — on the first 16 groups.  This pins the configuration of
    the published number; E5 removes next to nothing from this data (17 of 3.7 million kept points in these
    128 scans, tests/test_fused_oracle_cpu.py), the inputs of the tests below are where E5 decides."""
    seed, B_bench, G = 2026, 4096, 16
    B = G * S
    batch = synth.make_batch(seed + 5, B, N, noise_m=0.01)
    lens = np.full(B, N, np.int64)
    rng = np.random.default_rng(seed)
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / N]
                       for _ in range(B_bench)]).astype(np.float32)
    ang = rng.uniform(-3, 3, B_bench)
    pose = np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, B_bench), np.sin(ang), np.cos(ang),
                     rng.uniform(-2, 2, B_bench)], 1).astype(np.float32)
    motion, pose = motion[:B], pose[:B]
    p = Params.defaults(**fz.P_C5)
    kept = _kept(oracle, "bench", batch, lens, p)
    if ("wants", "bench") not in _CACHE:
        _CACHE["wants", "bench"] = _group_wants(oracle, batch, lens, p, kept, S, motion, pose)
    for ror_mode in (0, 1):
        res = _launch(gpu_mode, batch, lens, p, group=S, motion=motion, pose=pose, ror_mode=ror_mode)
        _check(res, _CACHE["wants", "bench"], ("bench shape", gpu_mode.mode_name, ror_mode))
        if ror_mode == 0:
            assert res["listed"] == 0


FUSED_INPUTS = {"settled": ("settled", fz.P_C5), "radius_lo": ("radius", fz.P_C5), "radius_hi": ("radius", fz.P_C5),
                "redone": ("redone", fz.P_TIGHT), "mixed_c5": ("mixed", fz.P_C5), "mixed_tight": ("mixed", fz.P_TIGHT)}


def _fused_case(oracle, case):
    name, pp = FUSED_INPUTS[case]
    batch, lens = _input(oracle, name)
    if name == "radius":
        pp = {**pp, "ror_radius": _CACHE["targets"][0]["r_lo" if case.endswith("lo") else "r_hi"]}
    p = Params.defaults(**pp)
    return name, batch, lens, p, _kept(oracle, name, batch, lens, p)


@pytest.mark.parametrize("xf", ["none", "motion_pose", "motion_pose_t0"])
@pytest.mark.parametrize("case", list(FUSED_INPUTS))
def test_fused_grid_where_e5_decides(gpu_mode, oracle, case, xf):
    """Inputs 1 to 4 in groups of 8 (the mixed batch ends in a group of 3): de-skew + pose, the same with
    per-scan time offsets, and neither."""
    name, batch, lens, p, kept = _fused_case(oracle, case)
    assert sum(int((~k).sum()) for _, _, k in kept) > 0
    motion, pose, t0 = _xf(len(batch), 11)
    kw = {} if xf == "none" else dict(motion=motion, pose=pose, t0=t0 if xf.endswith("t0") else None)
    if ("wants", case, xf) not in _CACHE:
        _CACHE["wants", case, xf] = _group_wants(oracle, batch, lens, p, kept, S, **kw)
    wants = _CACHE["wants", case, xf]
    for ror_mode in (0, 1):
        res = _launch(gpu_mode, batch, lens, p, group=S, ror_mode=ror_mode, **kw)
        _check(res, wants, (case, xf, gpu_mode.mode_name, ror_mode))
        if ror_mode == 0:
            if case == "settled":
                assert res["listed"] == 0
            elif case == "redone":
                assert res["listed"] == len(wants)
            elif name == "mixed":
                assert res["listed"] >= 1


# ---- the cell records and their merge -----------------------------------------------------------------------
def _produce(gpu, batch, lens, p, motion, pose, split, T, ror_mode):
    """Every rank's rplgpu_cloud_fused_cells_dev over its sensors of every group; (records per rank, per rank
    (start, count, status) per group, the gathered device buffers)."""
    import torch
    dev = torch.device("cuda:0")
    B, n = batch.shape
    world = len(split)
    idxs = [np.array([t * S + s for t in range(T) for s in sensors if t * S + s < B]) for sensors in split]
    slot = max(len(i) for i in idxs) * 16384
    mw = abi.cloud_meta_words(T)
    cells_all = torch.zeros((world, slot * 8), dtype=torch.int32, device=dev)
    meta_all = torch.zeros((world, mw), dtype=torch.int32, device=dev)
    per_rank = []
    gpu.set_ror_mode(ror_mode)
    try:
        for r, (sensors, idx) in enumerate(zip(split, idxs)):
            k, nb = len(sensors), len(idx)
            ng = (nb + k - 1) // k
            d_nodes = torch.from_numpy(np.ascontiguousarray(batch[idx]).view(np.uint8).reshape(nb, n * 8)).to(dev)
            d_len = torch.from_numpy(np.asarray(lens[idx], np.int32)).to(dev)
            d_mo = torch.from_numpy(np.ascontiguousarray(motion[idx])).to(dev)
            d_po = torch.from_numpy(np.ascontiguousarray(pose[idx])).to(dev)
            cur = torch.zeros(1, dtype=torch.int64, device=dev)
            st = torch.zeros(T, dtype=torch.int64, device=dev)
            nc = torch.zeros(T, dtype=torch.int32, device=dev)
            sts = torch.zeros(T, dtype=torch.int32, device=dev)
            gpu.cloud_fused_cells_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), nb, k, p, d_mo.data_ptr(),
                                      d_po.data_ptr(), cells_all[r].data_ptr(), slot, cur.data_ptr(), st.data_ptr(),
                                      nc.data_ptr(), sts.data_ptr())
            gpu.pack_cloud_meta_dev(cur.data_ptr(), st.data_ptr(), nc.data_ptr(), ng, slot, T, meta_all[r].data_ptr())
            gpu.synchronize()
            assert int(cur.item()) <= slot and int(cur.item()) == int(nc.sum().item())
            per_rank.append((st.cpu().numpy()[:ng], nc.cpu().numpy()[:ng], sts.cpu().numpy()[:ng]))
    finally:
        gpu.set_ror_mode(0)
    return cells_all, meta_all, mw, slot, per_rank


@pytest.mark.parametrize("case", ["settled", "redone", "mixed_c5", "mixed_tight", "radius_hi"])
def test_cell_records_and_merge_where_e5_decides(gpu_mode, oracle, case):
    """The cell path on the same groups: rplgpu_cloud_fused_cells_dev over a 2-way and an 8-way split of every
    group; the records' per-cell counts, summed over the ranks, are the oracle grid's counts; rplgpu_merge_cells_dev
    gives the oracle's grid and rplgpu_merge_cells_host the same bytes."""
    import torch
    gpu = gpu_mode
    dev = torch.device("cuda:0")
    name, batch, lens, p, kept = _fused_case(oracle, case)
    motion, pose, _ = _xf(len(batch), 11)
    if ("wants", case, "motion_pose") not in _CACHE:
        _CACHE["wants", case, "motion_pose"] = _group_wants(oracle, batch, lens, p, kept, S, motion=motion, pose=pose)
    wants = _CACHE["wants", case, "motion_pose"]
    T = len(wants)
    for split in ([[0, 1, 2, 3], [4, 5, 6, 7]], [[s] for s in range(S)]):
        for ror_mode in (0, 1):
            ctx = (case, len(split), gpu.mode_name, ror_mode)
            cells_all, meta_all, mw, slot, per_rank = _produce(gpu, batch, lens, p, motion, pose, split, T, ror_mode)
            recs = cells_all.cpu().numpy().view(abi.CELL_DTYPE).reshape(len(split), slot)
            for g in range(T):
                parts = [recs[r][int(st[g]): int(st[g]) + int(nc[g])] for r, (st, nc, _) in enumerate(per_rank)
                         if g < len(nc)]
                assert all(np.all(np.diff(q["key"].astype(np.int64)) > 0) for q in parts), ctx
                allr = np.concatenate(parts)
                keys, inv = np.unique(allr["key"], return_inverse=True)
                counts = np.bincount(inv, weights=allr["count"], minlength=len(keys)).astype(np.int64)
                assert np.array_equal(keys, fz.cell_keys(wants[g][1])), (ctx, g)
                assert np.array_equal(counts, wants[g][2].astype(np.int64)), (ctx, g)
            cap = len(batch) * N
            arena = torch.full((cap, 4), -7.0, dtype=torch.float32, device=dev)
            cur = torch.zeros(1, dtype=torch.int64, device=dev)
            st = torch.zeros(T, dtype=torch.int64, device=dev)
            npn = torch.zeros(T, dtype=torch.int32, device=dev)
            sts = torch.full((T,), -1, dtype=torch.int32, device=dev)
            gpu.merge_cells_dev(cells_all.data_ptr(), slot, meta_all.data_ptr(), mw, len(split), T, p,
                                arena.data_ptr(), cap, cur.data_ptr(), st.data_ptr(), npn.data_ptr(), sts.data_ptr())
            gpu.synchronize()
            total = int(cur.item())
            a, st, npn, sts = arena[:total].cpu().numpy(), st.cpu().numpy(), npn.cpu().numpy().astype(np.int64), sts.cpu().numpy()
            assert total == int(npn.sum())
            worst = 0.0
            for g in range(T):
                want = wants[g][0]
                got = a[st[g]: st[g] + npn[g]]
                assert int(sts[g]) == wants[g][3] == 0 and len(got) == len(want), (ctx, g)
                assert got[:, 3].tobytes() == want[:, 3].tobytes() and np.all(got[:, 2] == 0.0), (ctx, g)
                if len(want):
                    worst = max(worst, float(np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2]))))
            print(ctx, "merge max |dxy|", worst)
            assert worst <= XYZ_TOL, (ctx, worst)
            h_arena, h_cur, h_st, h_np, h_sts = abi.merge_cells_host(recs, slot, meta_all.cpu().numpy().view(np.uint32),
                                                                     len(split), T, p, arena_capacity=cap)
            assert h_cur == total and list(h_np) == list(npn) and list(h_sts) == list(sts)
            assert [h_arena[int(h_st[g]): int(h_st[g]) + int(h_np[g])].tobytes() for g in range(T)] == \
                [a[st[g]: st[g] + npn[g]].tobytes() for g in range(T)]


# ---- the cell range with E5 on ------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("kind", fz.RANGE_KINDS)
def test_cell_range_counts_only_what_e5_keeps(gpu, oracle, kind, clip):
    """RPLGPU_SCAN_CELL_RANGE with E5 on, in the kernel instances that test the range per sample (clip_enable
    = 0, and clip_enable = 1 with a 1 mm leaf): a far return that E5 removes leaves the status 0 and
    rplgpu_scan_to_cloud returns OK; far returns that E5 keeps flag the scan and are dropped; an out-of-range
    sample still counts as an in-range sample's neighbour; the cells 32 766 | 32 767 are told apart.  Both E5
    modes, the batch and the single-scan entry point."""
    p = Params.defaults(**fz.range_params(clip))
    s = fz.range_scan(kind)
    batch = np.stack([s, fz.range_scan("far_single", seed=3401), s])
    lens = np.full(3, N, np.int64)
    kept = _kept(oracle, ("range", kind), batch, lens, p)
    wants = _scan_wants(oracle, batch, lens, p, kept)
    flagged = kind != "far_single"
    assert wants[0][3] == (abi.SCAN_CELL_RANGE if flagged else 0) and wants[1][3] == 0
    for ror_mode in (0, 1):
        res = _launch(gpu, batch, lens, p, ror_mode=ror_mode)
        _check(res, wants, ("range", kind, clip, ror_mode))
        gpu.set_ror_mode(ror_mode)
        try:
            cloud, st = gpu.scan_to_cloud(s, p, allow_overflow=flagged)  # (raises on RPLGPU_ERR_SCAN_OVERFLOW otherwise)
        finally:
            gpu.set_ror_mode(0)
        want = wants[0][0]
        assert st == wants[0][3], (kind, clip, ror_mode, hex(st))
        assert len(cloud) == len(want) and cloud[:, 3].tobytes() == want[:, 3].tobytes()
        assert np.max(np.abs(cloud[:, :2].astype(np.float64) - want[:, :2])) <= XYZ_TOL


def test_cell_range_fused_pose_carries_points_out(gpu, oracle):
    """E8: a pose translation of 10 m carries part of ONE sensor's ring past the cell range (1 mm leaf):
    the bit is set on that group only, the grid is the oracle's over the in-range points."""
    group, B = 4, 8
    batch = synth.make_batch(3500, B, N, noise_m=0.01, r0_range=(22.0, 24.0))
    lens = np.full(B, N, np.int64)
    p = Params.defaults(**fz.range_params(1))
    kept = _kept(oracle, "range_pose", batch, lens, p)
    ang = np.linspace(-1.0, 1.0, B)
    pose = np.stack([np.cos(ang), -np.sin(ang), np.zeros(B), np.sin(ang), np.cos(ang), np.zeros(B)], 1).astype(np.float32)
    pose[1, 2] = 10.0
    wants = _group_wants(oracle, batch, lens, p, kept, group, pose=pose)
    assert [w[3] for w in wants] == [abi.SCAN_CELL_RANGE, 0]
    for ror_mode in (0, 1):
        res = _launch(gpu, batch, lens, p, group=group, pose=pose, ror_mode=ror_mode)
        _check(res, wants, ("range pose", ror_mode))
