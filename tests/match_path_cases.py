"""The inputs of tests/test_gpu_match_paths.py: E13 on the paths of k_match_score and k_match_best that the cases
of tests/match_cases.py do not reach — a workgroup's second pass, every layout of the candidate window, run-length
merging run by run, the tie key at its field limits, cells and field indices at the grid limits, hundreds of groups.
Every case has a regime check made from the oracle (tests/match_oracle.py) and the case's construction alone: it
asserts that the case exercises what it claims.  tests/test_match_paths_cpu.py runs every regime without a device.
If a regime check fails, the input is what changes, never the check.  TEST INFRASTRUCTURE — imported by tests/ only.

A case is the dict of tests/match_cases.py."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import occ_oracle as oo
from tests.occ_cases import nodes, pad, polar_nodes, rot_poses

F32 = np.float32
NO_CELL = -(1 << 40)  # the cell of a sample that gives no point


def truncated(case, n_keep):
    """The case with every scan cut to its first n_keep samples."""
    out = dict(case)
    out["lens"] = np.minimum(np.asarray(case["lens"]), n_keep)
    return out


def sample_cells(oracle, case, g):
    """(len, 2) int64: the cell (cx, cy) of every sample of group g's ONE scan at no rotation, NO_CELL where the
    sample gives no point or its point no cell.  From the oracle's points and their sample indices."""
    sl = mc.case_groups(case)[g]
    assert sl.stop - sl.start == 1
    b = sl.start
    L = min(int(case["lens"][b]), case["batch"].shape[1])
    pick = lambda a: None if a is None else a[sl]  # noqa: E731
    x, y, _, _, idx, _ = mo.group_points(oracle, [case["batch"][b][:L]], case["p"], pick(case.get("motion")),
                                         pick(case.get("pose2d")), pick(case.get("t0")))
    has, cx, cy = oo.cells_of(x, y, case["spec"])
    out = np.full((L, 2), NO_CELL, np.int64)
    out[idx[has], 0], out[idx[has], 1] = cx[has], cy[has]
    return out


def runs_of(cells):
    """[(start, length)] of the maximal runs of consecutive samples in one cell (NO_CELL never continues)."""
    L = len(cells)
    if L == 0:
        return []
    same = (cells[1:] == cells[:-1]).all(1) & (cells[1:, 0] != NO_CELL)
    starts = np.flatnonzero(np.concatenate([[True], ~same]))
    return list(zip(starts.tolist(), np.diff(np.concatenate([starts, [L]])).tolist()))


# ---- A: two passes per workgroup ------------------------------------------------------------------------------------
# k_match_score takes 2048 samples per pass and at most 8 workgroups per (scan, rotation): a workgroup walks a second
# pass only where n_stride > 16384.  At 18432 (nine passes) only workgroup z = 0 does, at 32768 every one.
TWO_PASS = 16384
LONG_LENS = {18432: (16385, 18431, 18432), 32768: (18433, 32767, 32768, 2049)}
WIDE_SPEC = mo.spec(shift_x=16, shift_y=16, rot_steps=1, rot_step=0.004, **mc.GROUP_GRID)


def _ring(seed, n):
    return synth.make_batch(seed, 1, n, noise_m=0.01, r0_range=(2.0, 5.5))[0].copy()


def _wall(L, rng):
    """match_cases._wall_scan with its last sample kept, whatever the 5 % of missing returns took."""
    s = mc._wall_scan(L, rng)
    th = math.radians(155)
    s[-1] = polar_nodes([th], [5.0 / math.sin(th)])[0]
    return s


def long_case(stride, wide=False):
    """Groups of ONE scan at n_stride = stride: the wall at every length of LONG_LENS[stride], a scan whose
    `stride` samples all land in one cell of value 100 (entries of weight 64 from two passes add in one register),
    a ring with 1 cm noise (the second pass's list is long and unlike the first).  wide: the T 16, K 1 window
    (1089 candidates, the registers path) on a random 256 x 256 field instead of the PASS_SPEC one."""
    rng = np.random.default_rng(1400 + stride)
    scans = [_wall(L, rng) for L in LONG_LENS[stride]]
    n_wall = len(scans)
    scans.append(mc._one_cell_scan(stride))
    scans.append(_ring(1401, stride))
    batch, lens = pad(scans, stride)
    xs = [4.5, 5.0, 5.5, 6.0][:n_wall] + [0.025, 0.0]  # (the wall's last samples, to the left, inside both grids)
    ys = [0.0] * n_wall + [3.025, 3.0 if not wide else 0.0]
    spec, field = (WIDE_SPEC, mc.random_field(1402, 1, 256, 256)) if wide else (mc.PASS_SPEC, mc._pass_field())
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=spec, fields=field,
                pose2d=rot_poses(np.zeros(len(scans)), xs, ys), n_wall=n_wall)


def long_key(stride, wide=False):
    return f"long{stride}{'w' if wide else ''}"


def long_regime(oracle, case, key):
    """Every scan longer than 16384 owes something to its samples from 16384 on: the volume of its first 16384
    samples differs in a candidate and in word 4 (at stride 18432 those are the samples of [16384, 18432) alone).
    The 2049-sample scan owes something to sample 2048, the only one of the second workgroup."""
    want = mc.case_want(oracle, case, key)
    n = case["batch"].shape[1]
    head = mc.case_want(oracle, truncated(case, TWO_PASS))
    short = mc.case_want(oracle, truncated(case, 2048))
    seen = 0
    for g, (vol, best, status) in enumerate(want):
        L = int(case["lens"][g])
        assert status == 0 and 0 < best[4] <= L <= n and best[0] > 0
        if L > TWO_PASS:
            assert (head[g][0] != vol).any() and head[g][1][4] < best[4], (g, L)
            seen += 1
        else:
            assert L == 2049 and (short[g][0] != vol).any() and short[g][1][4] + 1 == best[4]
    assert seen == len(want) - (1 if n == 32768 else 0) and n > TWO_PASS
    g = case["n_wall"]  # the one-cell scan
    vol, best, _ = want[g]
    if case["spec"] is mc.PASS_SPEC:
        K, Ty, Tx = (case["spec"][k] for k in ("rot_steps", "shift_y", "shift_x"))
        assert best[4] == n and vol[K, Ty, Tx] == 100 * n == best[0] == best[5]
    ring = sample_cells(oracle, case, g + 1)
    tail = len(runs_of(ring[TWO_PASS:TWO_PASS + 2048]))
    assert tail > 500 and not np.array_equal(ring[:2048], ring[TWO_PASS:TWO_PASS + 2048])
    return want


LONG_FRONT_N = 32768


def long_front_case(n=LONG_FRONT_N):
    """The parameters of match_cases.front_case (E5 on, inverted, motion with time offsets, a pivot away from the
    origin) on one scan of 32768 samples: the E5 keep bits are read up to word 1023, and isolated returns that E5
    removes stand on both sides of sample 16384.  (One scan: the oracle's E5 takes a second at this length.)"""
    B = 1
    batch = synth.make_batch(1410, B, n, noise_m=0.01, r0_range=(2.0, 5.5)).copy()
    for b in range(B):
        for i in (1000 + 37 * b, TWO_PASS + 1000 + 11 * b, n - 3000 - 5 * b):
            batch[b]["dist_mm_q2"][i - 2:i + 3] = 0
            batch[b]["dist_mm_q2"][i] = 4000
            batch[b]["quality"][i] = 200
    rng = np.random.default_rng(1411)
    ang = 2 * math.pi * np.arange(B) / B
    pose2d = rot_poses(ang + 0.3, 0.6 * np.cos(ang), 0.6 * np.sin(ang))
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                       for _ in range(B)]).astype(F32)
    t0 = rng.uniform(-0.02, 0.02, B).astype(F32)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, inverted=1, ror_enable=1,
                        ror_radius=0.10, ror_min_neighbors=2)
    return dict(batch=batch, lens=np.full(B, n), group=1, p=p, spec=mc.GROUP_SPEC,
                fields=mc.random_field(1412, 1, 256, 256), pose2d=pose2d, motion=motion, t0=t0,
                pivot=np.array([[0.4, -0.3]], F32))


def long_front_regime(oracle, case):
    """E5 decides something behind sample 16384 (without it more points are counted there and the volume differs),
    and the samples from 16384 on contribute."""
    want = mc.case_want(oracle, case, "long_front")
    p_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_off.ror_enable = 0
    off = mc.case_want(oracle, case, None, p_off)
    head = mc.case_want(oracle, truncated(case, TWO_PASS))
    head_off = mc.case_want(oracle, truncated(case, TWO_PASS), None, p_off)
    for g in range(len(want)):
        assert off[g][1][4] > want[g][1][4] > TWO_PASS and (off[g][0] != want[g][0]).any()
        assert head[g][1][4] < want[g][1][4] and (head[g][0] != want[g][0]).any()
        # the points E5 removes behind 16384: more than it removes before
        assert off[g][1][4] - want[g][1][4] > head_off[g][1][4] - head[g][1][4] > 0
    return want


# ---- B: window layouts ----------------------------------------------------------------------------------------------
def layout_of(Tx, Ty):
    """(nc, per, slices, owned) by the formula in k_match_score: nc candidates, a copy of the window takes `per`
    threads (whole waves, at most 1024), `slices` copies fit the workgroup; above 1024 candidates there is one
    copy and a thread owns up to `owned` of them."""
    nc = (2 * Tx + 1) * (2 * Ty + 1)
    per = min((nc + 63) & ~63, 1024)
    slices = 1024 // per if nc <= 1024 else 1
    return nc, per, slices, (nc + 1023) // 1024


# (Tx, Ty): the narrow layouts by `per` (64 .. 1024), both sides of the switch at 1024 candidates, rows of 65 and of
# 1, and the wide ones with 2, 3, 4 and 5 candidates per thread
LAYOUTS = [(10, 1), (6, 2), (32, 0), (0, 32), (6, 6), (7, 7), (8, 8), (9, 9), (10, 10), (11, 10), (11, 11), (12, 12),
           (13, 12), (13, 13), (14, 13), (14, 14), (15, 14), (15, 15), (15, 16), (16, 15), (32, 7),
           (16, 16), (22, 23), (23, 22), (27, 28), (32, 31), (31, 32), (32, 32)]


def layout_name(t):
    return f"tx{t[0]}_ty{t[1]}"


def layout_case(t):
    """match_cases.edge_case (points on and around every border of a small grid, the field with all seven bytes)
    at the window t = (Tx, Ty), K 1; the grid 64 or 61 cells wide by the layout's place in the list."""
    W = (64, 61)[LAYOUTS.index(t) % 2]
    case = mc.edge_case(W, mc.EDGE_H, t[0], t[1], 1, 0.01, n_random=120)
    case["nc"], case["per"], case["slices"], case["owned"] = layout_of(*t)
    return case


def layout_regime(oracle, t, case):
    s = case["spec"]
    assert (s["shift_x"], s["shift_y"]) == t and mo.volume_size(s) == 3 * case["nc"] == 3 * layout_of(*t)[0]
    return mc.edge_regime(oracle, layout_name(t), case)


# ---- C: runs, one by one ----------------------------------------------------------------------------------------------
# Every sample's cell is chosen by hand: a sensor in the middle of cell (0, 10) of a grid of 25 cm cells looks along
# +x, and a sample at angle 0 and 1.0 + 0.5 c metres lands in the middle of cell (4 + 2c, 10).  Consecutive samples
# with one distance are a run; every cell carries its own positive byte, so a lost or doubled sample changes the score
# of candidate (0, 0, 0) by that byte.
RUN_GRID = dict(origin_x=0.0, origin_y=0.0, resolution=0.25, width=32, height=32)
RUN_SPEC = mo.spec(shift_x=1, shift_y=1, rot_steps=0, rot_step=0.0, **RUN_GRID)
RUN_SPEC_K1 = mo.spec(shift_x=1, shift_y=1, rot_steps=1, rot_step=0.01, **RUN_GRID)
RUN_SENSOR = (0.125, 2.625)
RUN_ROW = 10
D_A, D_A2, D_B, D_C = 10000, 12000, 6000, 8000   # dist_mm_q2 of the run's cell (two of them) and of the two fillers
D_DROP = 0               # E1 drops it
D_FAR = 200000           # 50 m: cell 200 of 32, out of every shift's reach
D_NO_CELL = 1200000000   # 300 km: beyond cell 2^20, no cell at all
RUN_LMAX = 130
RUN_CENTRES = (64, 640, 2048)  # a 64-sample, a 128-sample (640 = 5 * 128) and a 2048-sample boundary


def cell_of_dist(d):
    return 4 + 2 * (d - 4000) // 2000, RUN_ROW


def run_field():
    yy, xx = np.mgrid[0:32, 0:32]
    return (1 + (7 * xx + 13 * yy) % 120).astype(np.int8)[None]


def _fill(n, first=0):
    """n samples alternating between the two filler cells."""
    return np.where((np.arange(n) + first) % 2 == 0, D_B, D_C).astype(np.int64)


def _run_case(dists, n, spec=RUN_SPEC):
    scans = [nodes(np.zeros(len(d), np.int64), np.asarray(d, np.int64)) for d in dists]
    batch, lens = pad(scans, n)
    B = len(scans)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=spec, fields=run_field(),
                pose2d=rot_poses(np.zeros(B), [RUN_SENSOR[0]] * B, [RUN_SENSOR[1]] * B),
                pivot=np.tile(np.array([RUN_SENSOR], F32), (B, 1)), dists=[np.asarray(d, np.int64) for d in dists])


SWEEP = [(s, L) for s in range(64) for L in range(1, 65 - s)]  # 2080 runs, one per 64-sample block


def sweep_case():
    """Every (start s, length L) with s + L <= 64 of a run inside a 64-aligned block of samples (the samples of
    half a wave), the rest of the block alternating between two other cells; the run's cell alternates block by
    block, so no run crosses a block.  2080 blocks: 65 scans of 2048 samples, a group each."""
    d = np.empty((len(SWEEP), 64), np.int64)
    for b, (s, L) in enumerate(SWEEP):
        d[b] = _fill(64)
        d[b, s:s + L] = (D_A, D_A2)[b % 2]
    return _run_case(list(d.reshape(65, 2048)), 2048)


def sweep_regime(oracle, case):
    """From the samples' cells in order: the (s, L) of the runs of the run's cells, block by block, are the full
    set; a block holds no other run; the longest run is 64."""
    want = mc.case_want(oracle, case, "run_sweep")
    seen = []
    run_cells = [cell_of_dist(D_A), cell_of_dist(D_A2)]
    for g in range(len(want)):
        cells = sample_cells(oracle, case, g)
        assert len(cells) == 2048 and want[g][1][4] == 2048 and want[g][2] == 0
        runs = runs_of(cells)
        for blk in range(32):
            mine = [(s - 64 * blk, L) for s, L in runs if 64 * blk <= s < 64 * blk + 64
                    and tuple(cells[s]) == run_cells[(32 * g + blk) % 2]]
            assert len(mine) == 1, (g, blk, mine)
            seen.append(mine[0])
        other = [L for s, L in runs if tuple(cells[s]) not in run_cells]
        assert max(other) == 1 and max(L for _, L in runs) <= 64
        score = sum(int(case["fields"][0][cy, cx]) for cx, cy in cells)
        assert want[g][0][0, 1, 1] == score  # candidate (0, 0, 0) counts every sample once
    assert seen == SWEEP and (0, 64) in seen and len(set(seen)) == 2080
    return want


def _centred(n, centres, L):
    d = _fill(n)
    for c in centres:
        a = max(0, c - L // 2)
        d[a:a + L] = D_A
    return d


def boundary_case(spec=RUN_SPEC, lengths=None):
    """Runs of every length 2 .. 130 centred on sample 64 (a wave's halves), 640 (two waves) and 2048 (two passes,
    two workgroups): a scan of 4096 samples per length.  (A run around 128 itself would touch the one around 64.)"""
    lengths = range(2, RUN_LMAX + 1) if lengths is None else lengths
    case = _run_case([_centred(4096, RUN_CENTRES, L) for L in lengths], 4096, spec)
    case["lengths"] = list(lengths)
    return case


def boundary_regime(oracle, case, key, centres=RUN_CENTRES):
    want = mc.case_want(oracle, case, key)
    K = case["spec"]["rot_steps"]
    for g, L in enumerate(case["lengths"]):
        cells = sample_cells(oracle, case, g)
        runs = {s: n for s, n in runs_of(cells) if n > 1}
        assert runs == {max(0, c - L // 2): L for c in centres}, (L, runs)
        for s in runs:
            assert tuple(cells[s]) == cell_of_dist(D_A)
        assert want[g][0][K, 1, 1] == sum(int(case["fields"][0][cy, cx]) for cx, cy in cells)
    return want


PASS_RUNS = (2, 3, 63, 64, 65, 127, 128, 129, 130)


def two_pass_run_case():
    """Runs centred on sample 16384 of 32768: where a workgroup's first pass ends and its second begins."""
    case = _run_case([_centred(32768, (TWO_PASS,), L) for L in PASS_RUNS], 32768)
    case["lengths"] = list(PASS_RUNS)
    return case


def broken_cases():
    """name -> (samples, the runs (start, length) they must show).  A run of the run's cell broken by a sample that
    E1 drops, by one out of every shift's reach and by one without a cell, each at an even and an odd sample and at
    a half-wave border; a run whose first sample is the scan's last kept one; a scan of odd length ending inside a
    run."""
    out = {}
    for name, breaker in (("dropped", D_DROP), ("far", D_FAR), ("no_cell", D_NO_CELL)):
        d = _fill(512)
        runs = []
        for a, L, hole in ((10, 20, 6), (101, 40, 7), (40, 48, 24), (200, 60, 1), (300, 130, 63), (450, 33, 31)):
            d[a:a + L] = D_A
            d[a + hole] = breaker
            runs += [(a, hole), (a + hole + 1, L - hole - 1)]
        out[name] = (d, sorted(r for r in runs if r[1] > 1))
    d = _fill(300)
    d[299] = D_A
    out["last_sample"] = (d, [])
    d = _fill(300)
    d[250] = D_A
    d[251:] = D_DROP
    out["last_kept"] = (d, [])
    d = _fill(333)
    d[300:] = D_A
    out["odd_in_run"] = (d, [(300, 33)])
    d = _fill(2049)
    d[2040:] = D_A
    out["odd_across_passes"] = (d, [(2040, 9)])
    return out


def broken_case():
    cs = broken_cases()
    case = _run_case([cs[k][0] for k in sorted(cs)], 2052)
    case["names"] = sorted(cs)
    return case


def broken_regime(oracle, case):
    want = mc.case_want(oracle, case, "run_broken")
    cs = broken_cases()
    for g, name in enumerate(case["names"]):
        d, runs = cs[name]
        cells = sample_cells(oracle, case, g)
        assert len(cells) == len(d)
        got = [r for r in runs_of(cells) if r[1] > 1]
        assert got == runs, (name, got, runs)
        here = cells[:, 0] != NO_CELL
        assert (here == ~np.isin(d, (D_DROP, D_NO_CELL))).all()
        assert want[g][2] == (abi.SCAN_CELL_RANGE if name == "no_cell" else 0), name
        assert want[g][1][4] == int((d != D_DROP).sum())  # a far point and one without a cell are finite points
        near = here & (d != D_FAR)
        assert want[g][0][0, 1, 1] == sum(int(case["fields"][0][cy, cx]) for cx, cy in cells[near])
        if name in ("last_sample", "last_kept"):
            last = np.flatnonzero(here)[-1]
            assert tuple(cells[last]) == cell_of_dist(D_A) and (cells[:last] != cells[last]).any(1).all()
    return want


# ---- D: the tie key and the count of equals at their limits ---------------------------------------------------------------
KEY_GRID = dict(origin_x=0.0, origin_y=0.0, resolution=0.25, width=80, height=80)
KEY_SENSOR = (7.625, 10.125)   # the middle of cell (30, 40)
KEY_CELL = (40, 40)            # one return at angle 0, 2.5 m
KEY_FULL = mo.spec(shift_x=32, shift_y=32, rot_steps=64, rot_step=0.02, **KEY_GRID)


KEY_DIST = 10000               # dist_mm_q2 of that return


def _key_case(spec, field, n_points=1, dist=KEY_DIST):
    scan = nodes(np.zeros(n_points, np.int64), np.full(n_points, dist, np.int64))
    batch, lens = pad([scan], max(n_points, 4))
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=spec, fields=field[None],
                pose2d=np.array([[1, 0, KEY_SENSOR[0], 0, 1, KEY_SENSOR[1]]], F32),
                pivot=np.array([KEY_SENSOR], F32))


def _turned_cell(spec, k, dist=KEY_DIST):
    """The cell of the one return (at dist_mm_q2 = dist) turned by k steps about the sensor."""
    rot = mo.rotations(spec)
    K = spec["rot_steps"]
    x = np.array([F32(KEY_SENSOR[0]) + F32(dist / 4000.0)], F32)
    y = np.array([KEY_SENSOR[1]], F32)
    has, cx, cy = mo.rotated_cells(x, y, KEY_SENSOR[0], KEY_SENSOR[1], rot[K + k, 0], rot[K + k, 1], spec)
    assert has.all()
    return int(cx[0]), int(cy[0])


KEY_NAMES = ("column", "corners", "full_volume", "full_volume_empty", "j_64_against_1", "k64_t0", "k64_t1",
             "uniform_3549")
_CACHE = {}


def key_cases():
    """name -> (case, expected (score, k, j, i) or None, expected number of equals or None)."""
    if "key" not in _CACHE:
        _CACHE["key"] = _key_cases()
        assert sorted(_CACHE["key"]) == sorted(KEY_NAMES)
    return _CACHE["key"]


def _key_cases():
    cx, cy = KEY_CELL
    out = {}
    zero = lambda: np.zeros((80, 80), np.int8)  # noqa: E731
    s = mo.spec(shift_x=32, shift_y=32, rot_steps=0, rot_step=0.0, **KEY_GRID)
    f = zero()
    for i, j in ((32, 32), (-32, 32), (32, -32), (-32, -32)):  # i*i + j*j = 2048, the largest there is
        f[cy + j, cx + i] = 90
    out["corners"] = (_key_case(s, f), (90, 0, -32, -32), 4)
    f = zero()
    f[cy + 32, cx + 5] = f[cy - 32, cx + 5] = 90               # j + Ty = 64 against 0
    out["column"] = (_key_case(s, f), (90, 0, -32, 5), 2)
    f = zero()
    f[cy + 32, cx + 1] = f[cy - 31, cx + 8] = 90               # 1024 + 1 = 961 + 64: j + Ty = 64 against 1
    out["j_64_against_1"] = (_key_case(s, f), (90, 0, -31, 8), 2)
    # a step of 0.02 rad moves the return by a fifth of a cell: the first distance from 2.5 m on at which the cells of
    # k = 64 and k = -64 are those of no other k
    s = mo.spec(shift_x=0, shift_y=0, rot_steps=64, rot_step=0.02, **KEY_GRID)
    for dist in range(KEY_DIST, KEY_DIST + 4000, 20):
        cells = [_turned_cell(s, k, dist) for k in range(-64, 65)]
        if cells.count(cells[0]) == 1 and cells.count(cells[-1]) == 1:
            break
    far = _turned_cell(s, 0, dist)
    f = zero()
    for k in (64, -64):
        c = _turned_cell(s, k, dist)
        f[c[1], c[0]] = 60
    out["k64_t0"] = (_key_case(s, f, dist=dist), (60, -64, 0, 0), 2)
    s = mo.spec(shift_x=1, shift_y=1, rot_steps=64, rot_step=0.02, **KEY_GRID)
    f = zero()
    c = _turned_cell(s, 64, dist)
    f[c[1], c[0]] = f[far[1], far[0] + 1] = 60                  # (64, 0, 0) against (0, 0, 1): distance first
    out["k64_t1"] = (_key_case(s, f, dist=dist), (60, 64, 0, 0), None)
    f = zero()
    f[cy - 2, cx + 5] = 77
    out["full_volume"] = (_key_case(KEY_FULL, f), None, None)
    out["full_volume_empty"] = (_key_case(KEY_FULL, f, dist=0), (0, 0, 0, 0), 129 * 65 * 65)
    s = mo.spec(shift_x=6, shift_y=6, rot_steps=10, rot_step=0.01, **KEY_GRID)
    out["uniform_3549"] = (_key_case(s, np.full((80, 80), 100, np.int8), n_points=5), (500, 0, 0, 0), 3549)
    return out


def key_regime(oracle, name, case, expect, equals):
    vol, best, status = mc.case_want(oracle, case, f"key_{name}")[0]
    s = case["spec"]
    assert status == 0 and (expect is None or tuple(best[:4]) == expect), (name, best)
    assert equals is None or best[6] == equals, (name, best)
    K, Ty, Tx = s["rot_steps"], s["shift_y"], s["shift_x"]
    if name == "corners":
        assert best[2] ** 2 + best[3] ** 2 == 2048
    if name in ("column", "j_64_against_1"):
        top = np.argwhere(vol == best[0])
        assert len(top) == 2 and top[:, 1].max() == 2 * Ty == 64  # the loser has j + Ty = 64
    if name == "k64_t0":
        assert vol[0, 0, 0] == vol[2 * K, 0, 0] == 60 and abs(int(best[1])) == 64 == K
    if name == "k64_t1":
        assert vol[2 * K, Ty, Tx] == vol[K, Ty, Tx + 1] == 60 and best[6] >= 2
    if name == "full_volume":
        # the one cell lies under the point at one shift of every rotation that leaves it within 32 cells
        assert mo.volume_size(s) == 545025 and best[0] == 77 and 2 <= best[6] <= 129 and best[4] == 1
        assert int((vol == 77).sum()) == best[6] and int((vol != 0).sum()) == best[6]
    if name == "full_volume_empty":
        assert not vol.any() and tuple(best) == (0, 0, 0, 0, 0, 0, 545025, 0)
    if name == "uniform_3549":
        assert (vol == 500).all() and best[4] == 5
    return best


# ---- E: grids at the limits ---------------------------------------------------------------------------------------------
BIG = {"4096x4096": (4096, 4096), "4096x1": (4096, 1), "1x4096": (1, 4096)}


def big_field(H, W, shift=0):
    """match_cases.pattern_field without the two (H, W) index planes."""
    return mc.FIELD_BYTES[(3 * np.arange(W)[None, :] + 5 * np.arange(H)[:, None] + shift) % 7][None]


def _big_points(W, H, res):
    """Cell centres on every border and corner of the grid and 1, 3, 32 and 33 cells outside it on every side: 32
    outside (cell -32, cell W + 31) is the last within reach of a shift of 32, 33 outside is dropped."""
    xs = [0, 1, W // 2, W - 2, W - 1, -1, -3, W, W + 2, -33, -32, W + 31, W + 32]
    ys = [0, 1, H // 2, H - 2, H - 1, -1, -3, H, H + 2, -33, -32, H + 31, H + 32]
    return (np.array([(x, y) for x in xs for y in ys], float) + 0.5) * res


def big_case(name):
    """T 32, K 1 on a grid at the 4096-cell limit of one or both axes: the biased 13-bit cells and the index
    cy * W + cx at their largest.  The sensor stands in the middle of the grid."""
    W, H = BIG[name]
    res = 0.05
    sensor = ((W / 2 + 0.37) * res, (H / 2 + 0.21) * res)
    rng = np.random.default_rng(1450 + W + 7 * H)
    rnd = rng.uniform([-3 * res, -3 * res], [(W + 3) * res, (H + 3) * res], (60, 2))
    scan = mc.nodes_to(np.concatenate([_big_points(W, H, res), rnd]), sensor)
    batch, lens = pad([scan], len(scan))
    s = mo.spec(origin_x=0.0, origin_y=0.0, resolution=res, width=W, height=H, shift_x=32, shift_y=32, rot_steps=1,
                rot_step=0.002)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=s, fields=big_field(H, W, W),
                pose2d=np.array([[1, 0, sensor[0], 0, 1, sensor[1]]], F32), pivot=np.array([sensor], F32))


def big_want(oracle, name, case):
    return mc.case_want(oracle, case, f"big_{name}", writer=mo.scores_gather)  # (correlate's box is the whole grid)


def big_regime(oracle, name, case):
    """edge_regime; and a listed cell (one within reach of the grid) has cx + 64 >= 4096 or cy + 64 >= 4096, a
    look-up inside the grid has cy * W + cx >= 2^23 where the grid has that many cells."""
    s = case["spec"]
    W, H = s["width"], s["height"]
    x, y = mc.case_points(oracle, case, 0)
    rot = mo.rotations(s)
    pv = case["pivot"][0]
    high, index = False, 0
    for kk in range(3):
        has, cx, cy = mo.rotated_cells(x, y, pv[0], pv[1], rot[kk, 0], rot[kk, 1], s)
        near = has & (cx >= -32) & (cx < W + 32) & (cy >= -32) & (cy < H + 32)
        high |= bool(((cx[near] + 64 >= 4096) | (cy[near] + 64 >= 4096)).any())
        if kk == 1:  # at no rotation the points stand as placed
            assert (~near).any() and cx[near].min() == -32 == cy[near].min()
            assert cx[near].max() == W + 31 and cy[near].max() == H + 31
        ax, ay = np.clip(cx[near] + 32, 0, W - 1), np.clip(cy[near] + 32, 0, H - 1)
        index = max(index, int((ay * W + ax).max()))
    assert high and index == W * H - 1 and (index >= 1 << 23 or W * H < 1 << 23), (name, high, index)
    want = big_want(oracle, name, case)
    assert want[0][1][0] > 0 and want[0][2] == 0
    return mc.edge_regime(oracle, name, case)


# ---- F: many groups ----------------------------------------------------------------------------------------------------------
MANY_B, MANY_GROUP, MANY_N = 1030, 3, 16
MANY_SPEC = mo.spec(origin_x=0.0, origin_y=0.0, resolution=0.25, width=5, height=3, shift_x=2, shift_y=1, rot_steps=1,
                    rot_step=0.05)
MANY_EMPTY = (0, 7, 100, 201, 342)
MANY_CELL_RANGE, MANY_TRUNCATED = 50, 300  # groups


def many_case(per_group):
    """1030 scans of 8 .. 16 samples in groups of 3: 344 groups, the last of one scan; one 5 x 3 field for all or
    one per group; a pivot per group.  Five groups are empty, a scan of group 50 stands 1e6 m away (CELL_RANGE), a
    scan of group 300 claims more samples than the stride holds."""
    rng = np.random.default_rng(1460)
    G = (MANY_B + MANY_GROUP - 1) // MANY_GROUP
    scans, tx, ty = [], [], []
    for b in range(MANY_B):
        m = int(rng.integers(8, MANY_N + 1)) if b // MANY_GROUP not in MANY_EMPTY else 0
        sensor = rng.uniform([-2.0, -2.0], [-1.0, -1.0])
        pts = rng.uniform([-0.5, -0.25], [1.75, 1.0], (m, 2))
        scans.append(mc.nodes_to(pts, sensor) if m else np.zeros(0, abi.NODE_DTYPE))
        tx.append(sensor[0])
        ty.append(sensor[1])
    batch, lens = pad(scans, MANY_N)
    tx[MANY_CELL_RANGE * MANY_GROUP + 1] = 1.0e6
    b = MANY_TRUNCATED * MANY_GROUP + 2
    batch[b] = mc.nodes_to(rng.uniform([-0.5, -0.25], [1.75, 1.0], (MANY_N, 2)), (tx[b], ty[b]))
    lens[b] = MANY_N + 3
    fields = mc.random_field(1461, G, 3, 5) if per_group else mc.pattern_field(3, 5)
    return dict(batch=batch, lens=lens, group=MANY_GROUP, p=Params.defaults(clip_enable=0), spec=MANY_SPEC,
                fields=fields, pose2d=rot_poses(np.zeros(MANY_B), tx, ty),
                pivot=rng.uniform([0.0, 0.0], [1.25, 0.75], (G, 2)).astype(F32))


def many_regime(oracle, case, key):
    want = mc.case_want(oracle, case, key)
    G = len(want)
    last = mc.case_groups(case)[-1]
    assert G == 344 and last.stop - last.start == 1
    assert sum(1 for _, best, _ in want if best[0] > 0) >= 300
    for g, (vol, best, status) in enumerate(want):
        planted = {MANY_CELL_RANGE: abi.SCAN_CELL_RANGE, MANY_TRUNCATED: abi.SCAN_OUT_TRUNCATED}.get(g, 0)
        assert status == planted, (g, status)
        assert (best[4] == 0 and not vol.any()) == (g in MANY_EMPTY), g
        if g:
            assert (vol != want[g - 1][0]).any(), g  # no two neighbours alike: a group read from the wrong place shows
    return want
