"""Spec of a group's voxel grid with E5 on (rplgpu_cloud_fused_voxel_dev, E8 + E5), and inputs for
which the reference alone shows that E5 decides something at the full scan size.
TEST INFRASTRUCTURE — imported by tests/ only.

The grid, from parts that exist: E1 + E2 by the C oracle (orc_scan_to_cloud), E5 on every scan's OWN
kept points in the sensor frame (orc_ror_mask: neighbours do not count the point itself), E6 and the
planar pose by oracle/fusion_oracle.py, the cell-range rule restated below, E4 by orc_voxel_grid over
the in-range points of the whole group.

The cell-range rule (include/rplgpu.h, RPLGPU_SCAN_CELL_RANGE), in float32: t = x / leaf,
f = floor(t); a point with |f.x| >= 32767 or |f.y| >= 32767 is dropped and sets the bit for its work
item (scan, or group).  Only points that survived E1 AND E5 count.

The generators (B in the issue's words): every one comes with a `*_regime` function that checks,
with the oracle alone, that the input is in the regime it claims."""
from __future__ import annotations

import os
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from rplidar_ros2_driver_amd import abi, synth
from tests import oracle_lib

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import fusion_oracle as fo  # noqa: E402

F32 = np.float32
CELL_LIMIT = F32(32767.0)
ROR_WINDOW = 64    # ror_resolve: indices either side of an open sample
ROR_FEW = 8        # ror_exhaustive: open samples a scan may have behind the window step
BLOCK = 124        # samples a block of the E5-inside pass owns


def threads() -> int:
    """Host threads for the per-scan orc_ror_mask calls (ctypes releases the GIL): what the process
    may use, never the machine's CPU count."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


# ---- per scan: E1 + E2, and E5's verdict on the scan's own points ---------------------------------
def e1_mask(nodes, p) -> np.ndarray:
    d = nodes["dist_mm_q2"]
    keep = d != 0
    if p.clip_enable:
        dm = d.astype(np.float32) / F32(4000.0)
        keep &= (dm >= F32(p.range_min)) & (dm <= F32(p.range_max)) & (nodes["quality"] >= p.q_min)
    return keep


def scan_kept(oracle, nodes, p):
    """(cloud (m, 4) of the samples E1 keeps, their sample indices, E5's keep mask over them)."""
    op = oracle_lib.copy_params(p)
    op.voxel_enable = 0
    op.ror_enable = 0
    nodes = np.ascontiguousarray(nodes)
    cloud = oracle.scan_to_cloud(nodes, op) if len(nodes) else np.zeros((0, 4), np.float32)
    idx = np.flatnonzero(e1_mask(nodes, p))
    assert len(idx) == len(cloud)
    if p.ror_enable and len(cloud):
        k = oracle.ror_mask(cloud, p.ror_radius, p.ror_min_neighbors)
    else:
        k = np.ones(len(cloud), bool)
    return cloud, idx.astype(np.int64), k


def scans_kept(oracle, scans, p):
    """scan_kept of every scan, on the thread pool."""
    scans = list(scans)
    if len(scans) <= 1 or not p.ror_enable:
        return [scan_kept(oracle, s, p) for s in scans]
    with ThreadPoolExecutor(threads()) as ex:
        return list(ex.map(lambda s: scan_kept(oracle, s, p), scans))


# ---- the group --------------------------------------------------------------------------------------
def group_points(oracle, scans, p, motion=None, pose2d=None, t0=None, kept=None):
    """(x, y, r2 float32, slot, sample index, intensity) of every point of a group after E1, E2, E5 on
    the scan's own points, E6 and the pose (the E9 tests' composition, tests/merge_oracle.py).
    `kept`: scans_kept(oracle, scans, p) when the caller has it already."""
    if kept is None:
        kept = scans_kept(oracle, scans, p)
    xs, ys, slots, idxs, ins = [], [], [], [], []
    for s, (cloud, idx, k) in enumerate(kept):
        cloud, idx = cloud[k], idx[k]
        if motion is not None:
            cloud = fo.deskew_cloud(cloud, idx, motion[s], None if t0 is None else t0[s])
        if pose2d is not None:
            r00, r01, tx, r10, r11, ty = pose2d[s]
            pose = np.array([[r00, r01, 0, tx], [r10, r11, 0, ty], [0, 0, 1, 0]], np.float32)
            cloud = fo.transform_cloud(cloud, pose)
        xs.append(cloud[:, 0])
        ys.append(cloud[:, 1])
        slots.append(np.full(len(idx), s, np.int64))
        idxs.append(idx.astype(np.int64))
        ins.append(cloud[:, 3])
    if not xs:
        z = np.zeros(0, np.float32)
        return z, z, z, np.zeros(0, np.int64), np.zeros(0, np.int64), z
    x, y = np.concatenate(xs).astype(np.float32), np.concatenate(ys).astype(np.float32)
    r2 = ((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32)
    return x, y, r2, np.concatenate(slots), np.concatenate(idxs), np.concatenate(ins).astype(np.float32)


def group_cloud_points(oracle, scans, p, motion=None, pose2d=None, t0=None, kept=None):
    """((m, 4) float32 points of the group in scan, then sample order, z = 0; the slot of each)."""
    x, y, _, slot, _, intens = group_points(oracle, scans, p, motion, pose2d, t0, kept)
    pts = np.zeros((len(x), 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 3] = x, y, intens
    return pts, slot


def in_cell_range(pts, leaf) -> np.ndarray:
    lf = F32(leaf)
    fx = np.floor((pts[:, 0] / lf).astype(np.float32))
    fy = np.floor((pts[:, 1] / lf).astype(np.float32))
    return (np.abs(fx) < CELL_LIMIT) & (np.abs(fy) < CELL_LIMIT)


def fused_grid(oracle, scans, p, motion=None, pose2d=None, t0=None, kept=None):
    """(cloud, cells[ix, iy], counts, status) of ONE work item: the scans of a group in one grid."""
    pts, _ = group_cloud_points(oracle, scans, p, motion, pose2d, t0, kept)
    inr = in_cell_range(pts, p.voxel_leaf)
    status = 0 if bool(inr.all()) else abi.SCAN_CELL_RANGE
    cloud, cells, counts = oracle.voxel_grid(pts[inr], p.voxel_leaf)
    return cloud, cells, counts, status


def cell_keys(cells) -> np.ndarray:
    """The library's key word of a cell: (iy + 32768) << 16 | (ix + 32768)."""
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    return (((c[:, 1] + 32768) << 16) | (c[:, 0] + 32768)).astype(np.uint32)


# ---- what the reference says about the exact steps a scan needs --------------------------------------
def open_behind_window(cloud, idx, radius, k) -> int:
    """Points of a scan with fewer than k neighbours among the samples at most ROR_WINDOW indices away
    (the oracle's float32 predicate): what only a whole-scan count can settle."""
    if len(cloud) == 0:
        return 0
    r2 = F32(radius) * F32(radius)
    x, y = cloud[:, 0], cloud[:, 1]
    cnt = np.zeros(len(cloud), np.int64)
    for s in range(1, ROR_WINDOW + 1):  # (kept points s places apart are at least s indices apart)
        if s >= len(cloud):
            break
        dx, dy = x[s:] - x[:-s], y[s:] - y[:-s]
        d2 = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
        hit = (d2 <= r2) & (idx[s:] - idx[:-s] <= ROR_WINDOW)
        cnt[s:] += hit
        cnt[:-s] += hit
    return int(np.count_nonzero(cnt < k))


# ---- input 1: settled inside the kernel ----------------------------------------------------------------
P_C5 = dict(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, voxel_enable=1, voxel_leaf=0.05, ror_enable=1,
            ror_radius=0.10, ror_min_neighbors=2)
P_TIGHT = {**P_C5, "ror_radius": 0.015, "ror_min_neighbors": 3}


def _put(s, i, range_m):
    s["dist_mm_q2"][i] = np.uint32(round(range_m * 4000.0))
    s["quality"][i] = 200  # (passes every q_min the tests use)


def settled_scan(seed, scan_index, n):
    """A 32 000-sample-class noisy ring (8 .. 25 m) with constructed returns far inside it, and what
    ROR(0.10 m, >= 2) must do with them: (nodes, indices E5 removes, indices of triples E5 keeps that
    the four index neighbours cannot settle).  Four variants by scan_index % 4:
      0  a single, an index-adjacent pair, an adjacent triple, a window triple (20 indices apart), a far
         triple (100 apart: only the whole-scan count sees it)
      1  the pair, the adjacent triple and the window triple ACROSS seams of the 124-sample blocks, a
         triple across the 0 / 2 pi seam (10, n - 30, n - 10), a single
      2  a single on the first sample, a pair on the last two, a window triple, a far triple
      3  adjacent triples on the first and on the last three samples, a single, a pair, a triple 60
         indices apart (its ends have one neighbour in the window: the whole-scan count keeps them)
    At most 6 constructed points per scan need the whole-scan step (the kernel takes 8).  Positions and the
    regime hold for n of the order of 32 000; a shorter scan (the second-writer test) keeps the shapes only."""
    assert n >= 3000
    s = synth.make_scan(seed, scan_index, n, noise_m=0.01, r0_range=(8.0, 25.0))
    at = lambda i: i * n // 32000          # noqa: E731  (positions are given for 32 000 samples)
    blk = lambda k: BLOCK * (k * n // 32000)  # noqa: E731
    rng = np.random.default_rng([seed, scan_index, 77])
    j = lambda: int(rng.integers(-40, 41))  # noqa: E731
    removed, late = [], []
    v = scan_index % 4

    def single(i, r):
        _put(s, i, r)
        removed.append(i)

    def pair(i, r):
        _put(s, i, r)
        _put(s, i + 1, r)
        removed.extend([i, i + 1])

    def triple(i, step, r, is_late=True):
        for q in (i, i + step, i + 2 * step):
            _put(s, q, r)
            if is_late:
                late.append(q)

    if v == 0:
        single(at(5000) + j(), 1.5)
        pair(at(9000) + j(), 2.0)
        triple(at(12000) + j(), 1, 1.0, is_late=False)
        triple(at(15000) + j(), 20, 1.0)
        triple(at(20000) + j(), 100, 1.0)
    elif v == 1:
        single(at(5000) + j(), 2.5)
        pair(blk(50) - 1, 2.0)
        triple(blk(70) - 1, 1, 1.0, is_late=False)
        triple(blk(90) - 10, 20, 1.0)
        for q in (10, n - 30, n - 10):
            _put(s, q, 0.7)
            late.append(q)
    elif v == 2:
        single(0, 1.5)
        pair(n - 2, 2.5)
        triple(at(15000) + j(), 20, 1.0)
        triple(at(20000) + j(), 100, 1.0)
    else:
        triple(0, 1, 1.0, is_late=False)
        triple(n - 3, 1, 2.0, is_late=False)
        single(at(7000) + j(), 1.5)
        pair(at(9000) + j(), 2.0)
        triple(at(17000) + j(), 60, 1.0)
    return s, np.array(sorted(removed)), np.array(sorted(late))


def settled_batch(seed, B, n):
    out = [settled_scan(seed, b, n) for b in range(B)]
    return np.stack([o[0] for o in out]), [o[1] for o in out], [o[2] for o in out]


def settled_regime(nodes, removed, late, kept, p):
    """The conditions of input 1 on one scan, from scan_kept's result alone."""
    cloud, idx, k = kept
    gone = idx[~k]
    assert 1 <= len(gone) <= ROR_FEW, len(gone)
    assert set(removed.tolist()) <= set(gone.tolist()), "a constructed single / pair survived"
    assert set(late.tolist()) <= set(idx[k].tolist()) and len(late) >= 3, "a constructed triple was removed"
    assert open_behind_window(cloud, idx, p.ror_radius, p.ror_min_neighbors) <= ROR_FEW


# ---- input 2: on the radius -----------------------------------------------------------------------------
RADIUS_RANGES = (2.0, 10.0, 30.0)


def _d2(a, b):
    dx, dy = F32(a[0]) - F32(b[0]), F32(a[1]) - F32(b[1])
    return F32(F32(dx * dx) + F32(dy * dy))  # products then sum


def _radius_for(d2):
    """(r_lo, r_hi): r_hi the smallest float32 with r * r >= d2 in float32, r_lo the float32 below it."""
    r = F32(np.sqrt(np.float64(d2)))
    while F32(r * r) >= d2:
        r = np.nextafter(r, F32(0.0))
    while F32(r * r) < d2:
        r = np.nextafter(r, F32(1.0))
    return np.nextafter(r, F32(0.0)), r


def radius_batch(oracle, seed, n, p):
    """12 scans (ranges 2 / 10 / 30 m x four quadrants), each a ring (12 .. 25 m) with one constructed
    return P (index i) that has ONE neighbour clearly inside the radius (index i + 1, same range) and one
    more, Q (index i - 1, ~0.1 m farther out), whose float32 d2 to P decides: ROR(r, >= 2) keeps P with
    r_hi and removes it with r_lo, two radii one ulp apart.  Q's distance word is searched over 64 values:
    odd scans take one with r_hi * r_hi == d2 exactly (the case that tells <= from <), even scans one
    without.  Returns (batch, list of dict(i, r_lo, r_hi, exact))."""
    op = oracle_lib.copy_params(p)
    op.voxel_enable = 0
    op.ror_enable = 0
    scans, targets = [], []
    for b in range(12):
        R = RADIUS_RANGES[b % 3]
        s = synth.make_scan(seed, b, n, noise_m=0.01, r0_range=(17.0, 19.0))
        i = (2 * (b // 3) + 1) * n // 8 + 37 * b
        s["dist_mm_q2"][i - 3:i + 4] = 0
        _put(s, i, R)
        _put(s, i + 1, R)
        _put(s, i - 1, R + 0.0995)
        base = int(s["dist_mm_q2"][i - 1])
        pick = None
        for off in range(64):
            s["dist_mm_q2"][i - 1] = base + off
            c = oracle.scan_to_cloud(s[i - 1:i + 1], op)
            d2 = _d2(c[1], c[0])
            r_lo, r_hi = _radius_for(d2)
            exact = bool(F32(r_hi * r_hi) == d2)
            if pick is None:
                pick = (off, r_lo, r_hi, exact)
            if exact == bool(b % 2):
                pick = (off, r_lo, r_hi, exact)
                break
        s["dist_mm_q2"][i - 1] = base + pick[0]
        scans.append(s)
        targets.append(dict(i=i, r_lo=float(pick[1]), r_hi=float(pick[2]), exact=pick[3]))
    return np.stack(scans), targets


def radius_regime(kept_lo, kept_hi, target):
    """The oracle removes P with r_lo and keeps it with r_hi."""
    for (cloud, idx, k), want in ((kept_lo, False), (kept_hi, True)):
        at = np.flatnonzero(idx == target["i"])
        assert len(at) == 1 and bool(k[at[0]]) == want, (target, want)


# ---- input 3: given up and redone ------------------------------------------------------------------------
REDONE_R0 = (11.0, 15.0)  # (ring ranges at which ROR(0.015, >= 3) removes 7 .. 20 % at q_min 0 and 48)


def redone_batch(seed, B, n):
    """The bench ring (1 cm noise) under a radius of the order of the noise: ROR(0.015 m, >= 3)."""
    return synth.make_batch(seed, B, n, noise_m=0.01, r0_range=REDONE_R0)


def redone_regime(kept):
    cloud, idx, k = kept
    frac = 1.0 - float(k.mean())
    assert 0.05 <= frac <= 0.30, frac


# ---- input 4: mixed groups --------------------------------------------------------------------------------
def cluttered_scan(seed, scan_index, n, count=40):
    """A noisy ring with `count` isolated returns: more than the kernel counts itself (listed)."""
    s = synth.make_scan(seed, scan_index, n, noise_m=0.01, r0_range=(8.0, 25.0))
    rng = np.random.default_rng([seed, scan_index, 78])
    for i in rng.choice(np.arange(200, n - 200, 400), size=count, replace=False):
        _put(s, int(i), float(rng.uniform(0.5, 3.0)))
    return s


def lonely_scan(seed, scan_index, n):
    """Everything invalid but five mutually distant returns: E5 removes the scan's every point."""
    s = synth.make_scan(seed, scan_index, n, noise_m=0.01)
    s["dist_mm_q2"][:] = 0
    for q, r in zip((100, n // 5, 2 * n // 5, 3 * n // 5, n - 100), (1.0, 3.0, 9.0, 20.0, 35.0)):
        _put(s, q, r)
    return s


MIXED_GROUP = 8


def mixed_batch(seed, n):
    """Two groups of 8 and a short third one (3 scans): settled scans (input 1), rings that only a tight
    radius thins (input 3), a cluttered scan, an empty scan (len 0), a scan E5 removes entirely, ragged
    lengths around multiples of the 124-sample block.  Returns (batch (19, n), lens)."""
    B = 2 * MIXED_GROUP + 3
    scans = [np.zeros(n, abi.NODE_DTYPE) for _ in range(B)]
    lens = np.full(B, n, np.int64)
    ragged = [BLOCK * 250, BLOCK * 250 + 1, BLOCK * 250 - 1, BLOCK * 251 + 62, n, n - 1, BLOCK * 200 + 123, BLOCK * 258]
    for b in range(B):
        L = min(n, ragged[b % len(ragged)])
        lens[b] = L
        if b % 4 == 1:
            s = synth.make_scan(seed + 1, b, L, noise_m=0.01, r0_range=REDONE_R0)
        elif b == 6:
            s = cluttered_scan(seed, b, L)
        else:
            s = settled_scan(seed, b, L)[0]
        scans[b][:L] = s
    lens[3] = 0                                   # an empty scan (its slot keeps stale nodes)
    scans[12][:] = lonely_scan(seed, 12, n)       # all of its points removed by E5
    lens[12] = n
    return np.stack(scans), lens


def mixed_regime(keptlist, lens, p):
    """Per group the oracle removes at least one point; the lonely scan loses all of its five; under
    ROR(0.10, >= 2) the cluttered scan has more open points than the kernel counts itself."""
    removed = [int((~k).sum()) for _, _, k in keptlist]
    for g in range(0, len(keptlist), MIXED_GROUP):
        assert sum(removed[g:g + MIXED_GROUP]) >= 1
    cloud, idx, k = keptlist[12]
    assert len(cloud) == 5 and not k.any()
    assert len(keptlist[3][0]) == 0 and lens[3] == 0
    cloud, idx, k = keptlist[6]
    assert open_behind_window(cloud, idx, p.ror_radius, p.ror_min_neighbors) > ROR_FEW


# ---- the cell range with E5 ---------------------------------------------------------------------------------
LEAF_FINE = 0.001  # cells of 1 mm: the cell range ends at +-32.767 m, inside range_max = 40 m


def range_params(clip_enable):
    """Parameters for which the host cannot prove the cell range safe (the !SAFE kernel instances)."""
    return {**P_C5, "clip_enable": clip_enable, "voxel_leaf": LEAF_FINE}


def range_scan(kind, n=32000, seed=3400):
    """A ring of 8 .. 26 m (inside the cell range at a 1 mm leaf) with constructed returns near +x:
      far_single     one return at 35 m (cell 35 000): E5 removes it, nobody may flag the scan for it
      far_triple     three index-adjacent returns at 35 m and three 5 indices apart at 36 m (kept at once /
                     by the +-64 window): the scan is flagged, the cloud is the grid of the other points
      kth_neighbour  P at 32.70 m with ONE in-range neighbour and one at 32.78 m, outside the range: E5
                     runs in front of the range test, so P survives ROR(0.10, >= 2)
      straddle       three returns on the x axis in the cells 32 765, 32 766 and 32 767: the last is out"""
    s = synth.make_scan(seed, 0, n, noise_m=0.01, r0_range=(8.0, 20.0))
    i = n // 400
    s["dist_mm_q2"][i - 8:i + 40] = 0
    if kind == "far_single":
        _put(s, i, 35.0)
    elif kind == "far_triple":
        for q in (i, i + 1, i + 2):
            _put(s, q, 35.0)
        for q in (i + 10, i + 15, i + 20):
            _put(s, q, 36.0)
    elif kind == "kth_neighbour":
        _put(s, i, 32.70)
        _put(s, i + 1, 32.705)
        _put(s, i - 1, 32.78)
    elif kind == "straddle":
        for q, d in zip((i, i + 1, i + 2), (131062, 131066, 131070)):
            _put(s, q, 1.0)
            s["dist_mm_q2"][q] = d
            s["angle_z_q14"][q] = 0
    else:
        raise ValueError(kind)
    return s


RANGE_KINDS = ("far_single", "far_triple", "kth_neighbour", "straddle")


def range_regime(kind, kept, p):
    """What the reference says about a range_scan: (points E5 keeps outside the cell range)."""
    cloud, idx, k = kept
    pts = cloud[k]
    out = ~in_cell_range(pts, p.voxel_leaf)
    far_e1 = ~in_cell_range(cloud, p.voxel_leaf)
    if kind == "far_single":
        assert far_e1.sum() == 1 and out.sum() == 0  # E1 keeps it, E5 removes it
    elif kind == "far_triple":
        assert far_e1.sum() == 6 and out.sum() == 6
    elif kind == "kth_neighbour":
        assert far_e1.sum() == 1 and out.sum() == 1
        x = pts[:, 0]
        assert np.count_nonzero((x > 32.6) & (x < 32.72)) == 2  # P and its in-range neighbour survive
    else:
        fx = np.floor((pts[:, 0] / F32(p.voxel_leaf)).astype(np.float32))
        assert sorted(fx[fx >= 32760].tolist()) == [32765.0, 32766.0, 32767.0] and out.sum() == 1
    return int(out.sum())


# ---- what the GPU tests run (tests/test_gpu_fused_ror.py); tests/test_fused_oracle_cpu.py checks the
# regimes of exactly these without a GPU ----------------------------------------------------------------------
N_FULL = 32000
Q_MINS = (0, 48)
SETTLED_SEED, SETTLED_B = 3100, 16
RADIUS_SEED = 3200
REDONE_SEED, REDONE_B = 2031, 16
MIXED_SEED = 3300
