"""The inputs of tests/test_gpu_map.py (E14), each with a regime check made from the oracle (tests/map_oracle.py)
and the case's construction alone, never from the device: the check asserts that the case exercises what it
claims.  tests/test_map_cpu.py runs every regime without a device.  A case is a dict as in tests/occ_cases.py
(batch, lens, group, p, spec, pose2d / motion / t0); ALL its scans go into one map.
TEST INFRASTRUCTURE — imported by tests/ only."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi
from tests import map_oracle as mp
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import occ_cases as oc
from tests import occ_oracle as oo
from tests.occ_cases import case_groups, case_rays, nodes, pad, polar_nodes, rot_poses

F32 = np.float32
_CACHE = {}
MAP_WIN = 176  # k_map_walk keeps a scan's misses in a MAP_WIN x MAP_WIN counter window in LDS (kMapWin in
#                csrc/rpl_map.hip), its corner MAP_WIN / 2 below the sensor cell
HALF = MAP_WIN // 2
P_PLAIN = dict(clip_enable=0)


def kernel_window():
    """kMapWin as csrc/rpl_map.hip has it."""
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "rplidar_ros2_driver_amd" / "csrc" / "rpl_map.hip").read_text()
    return int(re.search(r"constexpr int kMapWin = (\d+);", src).group(1))


def case_want(oracle, case, key=None, python=False):
    """((H, W, 2) int64 counts of ALL the case's scans, [status per group with the truncated bit]); once per key."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    s = case["spec"]
    n = case["batch"].shape[1]
    total = np.zeros((s["height"], s["width"], 2), np.int64)
    status = []
    for g, sl in enumerate(case_groups(case)):
        counts, st = mp.counts_of_rays(case_rays(oracle, case, g), s, python)
        total += counts
        if any(int(case["lens"][b]) > n for b in range(sl.start, sl.stop)):
            st |= abi.SCAN_OUT_TRUNCATED
        status.append(st)
    out = (total, status)
    if key is not None:
        _CACHE[key] = out
    return out


def in_window(x0, y0, W, H):
    """(H, W) bool: the grid cells inside the window of a scan whose sensor cell is (x0, y0)."""
    cx, cy = np.arange(W)[None, :], np.arange(H)[:, None]
    return (cx >= x0 - HALF) & (cx < x0 + HALF) & (cy >= y0 - HALF) & (cy < y0 + HALF)


def at_cell(s, cx, cy):
    """The middle of cell (cx, cy) in metres."""
    return s["origin_x"] + (cx + 0.5) * s["resolution"], s["origin_y"] + (cy + 0.5) * s["resolution"]


# ---- the room: two time steps of three sensors ---------------------------------------------------------------------
ROOM_SPEC = oo.spec(origin_x=-5.0, origin_y=-5.0, resolution=0.05, width=200, height=200, range_min=0.0,
                    obstacle_max=25.0, raytrace_max=30.0)
ROOM_N = 720
ROOM_STEPS = (((-1.0, -0.5, 0.3), (1.5, -0.8, -1.0), (-2.0, 1.0, 2.0)),   # x, y, heading of the three sensors
              ((-0.8, -0.4, 0.4), (1.7, -0.7, -0.9), (-1.8, 1.1, 2.1)))


def room_case(step):
    """Time step `step` (0 / 1): three sensors x 720 samples of match_cases' room over 200 x 200 cells of 5 cm."""
    scans = []
    for sx, sy, head in ROOM_STEPS[step]:
        th = 2 * math.pi * np.arange(ROOM_N) / ROOM_N
        scans.append(polar_nodes(th, mc._ray_ranges((sx, sy), th + head)))
    batch, lens = pad(scans, ROOM_N)
    sen = ROOM_STEPS[step]
    return dict(batch=batch, lens=lens, group=3, p=Params.defaults(**P_PLAIN), spec=ROOM_SPEC,
                pose2d=rot_poses([s[2] for s in sen], [s[0] for s in sen], [s[1] for s in sen]))


def room_regime(oracle):
    """Cells with several hits, several misses, both; the second step changes the map."""
    c0, st0 = case_want(oracle, room_case(0), "room0")
    c1, st1 = case_want(oracle, room_case(1), "room1")
    assert st0 == [0] and st1 == [0]
    for c in (c0, c1):
        assert (c[..., 1] > 1).sum() >= 50 and (c[..., 0] > 20).sum() >= 50
        assert ((c[..., 1] > 0) & (c[..., 0] > 0)).sum() >= 20
    assert (c0 != c1).any() and c0.sum() > 3 * ROOM_N * 20
    return c0, c1


# ---- one ray, many times ----------------------------------------------------------------------------------------------
RAY_SPEC = oo.spec(origin_x=0.0, origin_y=0.0, resolution=0.05, width=256, height=64, range_min=0.0,
                   obstacle_max=25.0, raytrace_max=30.0)
RAY_CUT_SPEC = oo.spec(origin_x=0.0, origin_y=0.0, resolution=0.05, width=256, height=64, range_min=0.0,
                       obstacle_max=3.0, raytrace_max=4.0)
RAY_SENSOR = (20, 32)
RAY_CELLS = 120  # the ray's length in cells: beyond the window's edge at HALF
RAY_LENS = (32768, 2049, 16385, 18431)


def ray_case(n, scans=1, cut=False):
    """`scans` scans of n identical samples: angle 0 (exactly +x), 6 m = 120 cells from the middle of cell (20, 32).
    cut: raytrace_max 4 m, so the ray is cut 80 cells out and marks nothing."""
    s = RAY_CUT_SPEC if cut else RAY_SPEC
    one = nodes(np.zeros(n, np.int64), np.full(n, RAY_CELLS * 200, np.int64))  # 6 m in quarter millimetres
    batch, lens = pad([one] * scans, n)
    sx, sy = at_cell(s, *RAY_SENSOR)
    return dict(batch=batch, lens=lens, group=scans, p=Params.defaults(**P_PLAIN), spec=s,
                pose2d=rot_poses([0.0] * scans, [sx] * scans, [sy] * scans))


def ray_want(n, scans=1, cut=False):
    """The counts written out by hand: n x scans misses in every cell of the row from the sensor cell on, and the
    hits (or, cut, the last miss) in the end cell."""
    s = RAY_CUT_SPEC if cut else RAY_SPEC
    c = np.zeros((s["height"], s["width"], 2), np.int64)
    x0, y0 = RAY_SENSOR
    end = x0 + (80 if cut else RAY_CELLS)
    c[y0, x0:end, 0] = n * scans
    c[y0, end, 0 if cut else 1] = n * scans
    return c


def ray_regime(oracle):
    assert RAY_CELLS > HALF  # the ray leaves the window: LDS counters and global adds on one ray
    for n in RAY_LENS[1:]:
        for cut in (False, True):
            got, st = case_want(oracle, ray_case(n, 1, cut), f"ray{n}{cut}")
            assert st == [0] and np.array_equal(got, ray_want(n, 1, cut)), (n, cut)
    r = case_rays(oracle, ray_case(RAY_LENS[1]), 0)
    assert mp.run_lengths(r, 0) == [RAY_LENS[1]]


# ---- rays of length zero -----------------------------------------------------------------------------------------------
ZERO_SPEC = oo.spec(origin_x=0.0, origin_y=0.0, resolution=0.05, width=64, height=64)
ZERO_SENSOR = (30, 31)
ZERO_SHORT, ZERO_LONG = 70, 9


def zero_case():
    """One scan: 70 returns 1 cm from the sensor (the end cell IS the sensor cell: they mark it and clear nothing),
    in runs of equal samples, then 9 returns of 1 m that clear it."""
    th = np.concatenate([np.repeat([0.0, 1.0, 2.5, 4.0, 5.5], ZERO_SHORT // 5), np.linspace(0.2, 6.0, ZERO_LONG)])
    rr = np.concatenate([np.full(ZERO_SHORT, 0.01), np.full(ZERO_LONG, 1.0)])
    batch, lens = pad([polar_nodes(th, rr)], len(th))
    sx, sy = at_cell(ZERO_SPEC, *ZERO_SENSOR)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=ZERO_SPEC,
                pose2d=rot_poses([0.0], [sx], [sy]))


def zero_regime(oracle):
    case = zero_case()
    r = case_rays(oracle, case, 0)
    here = (r["x1"] == r["x0"]) & (r["y1"] == r["y0"])
    assert here.sum() == ZERO_SHORT and r["mark"][here].all() and r["ray"].sum() == ZERO_SHORT + ZERO_LONG
    c, st = case_want(oracle, case, "zero")
    assert tuple(c[ZERO_SENSOR[1], ZERO_SENSOR[0]]) == (ZERO_LONG, ZERO_SHORT) and st == [0]
    return case


# ---- runs of equal rays -------------------------------------------------------------------------------------------------
RUN_SPEC = oo.spec(origin_x=-8.0, origin_y=-8.0, resolution=0.05, width=320, height=320, range_min=1.0,
                   obstacle_max=25.0, raytrace_max=30.0)
RUN_N = 4099  # odd, two passes and three samples
RUN_LENGTHS = (2, 3, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130)
RUN_CENTRES = (64, 640, 2048)
RUN_TAIL = 20  # the run every scan ends inside


def _run_base():
    """4099 samples whose rays all differ from their neighbours': the range alternates between 3 and 3.5 m."""
    th = 2 * math.pi * np.arange(RUN_N) / RUN_N
    return polar_nodes(th, np.where(np.arange(RUN_N) % 2 == 0, 3.0, 3.5))


def _plant(scan, centre, L, r=4.2):
    a = max(0, centre - L // 2)
    th = 2 * math.pi * centre / RUN_N
    scan[a:a + L] = polar_nodes([th], [r])[0]
    return a


def runs_case():
    """13 scans with runs of 2 .. 130 equal rays centred on samples 64, 640 and 2048 (lane 32, a wave's end, the
    pass boundary), every scan ending inside a run of 20; then three scans whose run of 100 at sample 640 is
    broken in the middle: by a sample without a return (E1), by a return nearer than range_min, by both."""
    scans, planted = [], []
    for L in RUN_LENGTHS:
        s = _run_base()
        want = []
        for c in RUN_CENTRES:
            a = _plant(s, c, L)
            want.append(min(L, a + L) if a else L)
        _plant(s, RUN_N - RUN_TAIL // 2, RUN_TAIL, r=5.0)
        want.append(RUN_TAIL)
        scans.append(s)
        planted.append(sorted(want))
    for kind in range(3):
        s = _run_base()
        a = _plant(s, 640, 100)
        want = [50, 49]
        if kind in (0, 2):
            s["dist_mm_q2"][a + 50] = 0            # no return: E1 drops it
        if kind == 1:
            s[a + 50] = polar_nodes([0.3], [0.5])[0]  # nearer than range_min: ignored
        if kind == 2:
            s[a + 20] = polar_nodes([0.3], [0.5])[0]
            want = [20, 29, 49]
        _plant(s, RUN_N - RUN_TAIL // 2, RUN_TAIL, r=5.0)
        scans.append(s)
        planted.append(sorted(want + [RUN_TAIL]))
    batch, lens = pad(scans, RUN_N)
    B = len(scans)
    case = dict(batch=batch, lens=lens, group=B, p=Params.defaults(**P_PLAIN), spec=RUN_SPEC,
                pose2d=rot_poses(np.linspace(0.0, 1.0, B), np.linspace(-1.0, 1.0, B), np.linspace(0.5, -0.5, B)))
    return case, planted


def runs_regime(oracle):
    """The oracle's runs longer than one sample are exactly the planted ones, and the longest exceeds 64."""
    case, planted = runs_case()
    r = case_rays(oracle, case, 0)
    assert not r["dropped"].any()
    longest = 0
    for slot, want in enumerate(planted):
        got = sorted(n for n in mp.run_lengths(r, slot) if n > 1)
        assert got == want, (slot, got, want)
        longest = max(longest, max(got))
    assert longest > 64
    return longest


# ---- the window -----------------------------------------------------------------------------------------------------------
def _window_scan(rng, n=400):
    """Returns of 0.3 .. 8 m (up to 160 cells of 5 cm) at random angles, and four of 7 m along the axes."""
    th = np.concatenate([rng.uniform(0, 2 * math.pi, n), [0.0, math.pi / 2, math.pi, 3 * math.pi / 2]])
    rr = np.concatenate([rng.uniform(0.3, 8.0, n), np.full(4, 7.0)])
    return polar_nodes(th, rr)


# name -> (width, height, sensor cells)
WINDOW_GRIDS = {
    "middle": (400, 400, ((200, 200),)),
    "corners": (300, 260, ((10, 10), (289, 12), (8, 250), (292, 249))),
    "outside": (300, 300, ((-40, 150), (150, 395))),
    "narrow": (100, 300, ((50, 150),)),
    "1xN": (1, 300, ((0, 150),)),
    "Nx1": (300, 1, ((150, 0),)),
    "4096x1": (4096, 1, ((2000, 0),)),
    "w301": (301, 200, ((150, 100),)),
    "w302": (302, 200, ((151, 100),)),
    "w303": (303, 200, ((152, 101),)),
}


def window_case(name):
    W, H, sensors = WINDOW_GRIDS[name]
    s = oo.spec(origin_x=0.0, origin_y=0.0, resolution=0.05, width=W, height=H)
    rng = np.random.default_rng(1400 + len(name) + W)
    scans = [_window_scan(rng) for _ in sensors]
    batch, lens = pad(scans, len(scans[0]))
    xy = [at_cell(s, cx, cy) for cx, cy in sensors]
    return dict(batch=batch, lens=lens, group=len(sensors), p=Params.defaults(**P_PLAIN), spec=s, sensors=sensors,
                pose2d=rot_poses([0.0] * len(sensors), [p[0] for p in xy], [p[1] for p in xy]))


def window_regime(oracle, name):
    """Per sensor: misses inside and outside its window's rectangle, from the oracle's cells; in 'middle', beyond
    all four sides and in the rows and columns on either side of every border."""
    case = window_case(name)
    s = case["spec"]
    W, H = s["width"], s["height"]
    r = case_rays(oracle, case, 0)
    assert not r["dropped"].any()
    for slot, cell in enumerate(case["sensors"]):
        assert oc.sensor_cell(r, slot) == cell
        counts = mp.counts_vector(*mp.all_rays(oc.slot_rays(r, slot)), W, H)
        miss = counts[..., 0] > 0
        win = in_window(*cell, W, H)
        assert (miss & ~win).any(), (name, slot)
        if win.any():
            assert (miss & win).any(), (name, slot)
        if name == "middle":
            (x0, y0), (ys, xs) = cell, np.nonzero(miss)
            assert min((xs < x0 - HALF).sum(), (xs >= x0 + HALF).sum(), (ys < y0 - HALF).sum(),
                       (ys >= y0 + HALF).sum()) >= 100
            for d in (-HALF - 1, -HALF, HALF - 1, HALF):
                assert miss[:, x0 + d].any() and miss[y0 + d, :].any(), d
    if name == "outside":
        assert not in_window(*case["sensors"][1], W, H).any()
    return case


# ---- many workgroups ------------------------------------------------------------------------------------------------------
def many_same_case():
    """64 scans of 300 samples from ONE pose into one map, group 8: the cells near the sensor take adds from 64
    workgroups."""
    rng = np.random.default_rng(1410)
    scans = [polar_nodes(rng.uniform(0, 2 * math.pi, 300), rng.uniform(0.5, 6.0, 300)) for _ in range(64)]
    batch, lens = pad(scans, 300)
    return dict(batch=batch, lens=lens, group=8, p=Params.defaults(**P_PLAIN),
                spec=oo.spec(origin_x=-6.4, origin_y=-6.4, resolution=0.05, width=256, height=256),
                pose2d=rot_poses([0.2] * 64, [0.33] * 64, [-0.21] * 64))


MANY_B, MANY_GROUP, MANY_N = 1030, 3, 48
MANY_TRUNCATED, MANY_FAR = 100, 700


def many_short_case():
    """1030 scans of 48 samples in 344 groups of 3 (the last one short); scan 100 claims more samples than the
    stride holds, scan 700 stands 1e6 m away (no sensor cell: its rays are dropped and set the bit)."""
    rng = np.random.default_rng(1411)
    B, n = MANY_B, MANY_N
    th, rr = rng.uniform(0, 2 * math.pi, (B, n)), rng.uniform(0.5, 4.0, (B, n))
    batch = np.stack([polar_nodes(th[b], rr[b]) for b in range(B)])
    lens = np.full(B, n)
    lens[MANY_TRUNCATED] = n + 5
    tx, ty = rng.uniform(-3, 3, B), rng.uniform(-3, 3, B)
    tx[MANY_FAR] = 1.0e6
    return dict(batch=batch, lens=lens, group=MANY_GROUP, p=Params.defaults(**P_PLAIN),
                spec=oo.spec(origin_x=-6.4, origin_y=-6.4, resolution=0.05, width=256, height=256),
                pose2d=rot_poses(rng.uniform(0, 6, B), tx, ty))


def many_regime(oracle):
    c, st = case_want(oracle, many_same_case(), "many_same")
    assert len(st) == 8 and st == [0] * 8 and c[..., 0].max() >= 64 * 100
    c, st = case_want(oracle, many_short_case(), "many_short")
    assert len(st) == 344
    want = [0] * 344
    want[MANY_TRUNCATED // 3] = abi.SCAN_OUT_TRUNCATED
    want[MANY_FAR // 3] = abi.SCAN_CELL_RANGE
    assert st == want and c.sum() > 0


# ---- the front end --------------------------------------------------------------------------------------------------------
FRONT_B = 4


def front_case(inverted=0):
    """occ_cases.full_case's first scans: 8192 samples each, 1 cm noise, motion with time offsets, poses, E5 on."""
    case = oc.full_case(inverted, B=FRONT_B)
    case["group"] = FRONT_B
    return case


def front_regime(oracle):
    """E5 decides something: without it the counts differ."""
    case = front_case(0)
    want, st = case_want(oracle, case, "front0")
    p_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_off.ror_enable = 0
    off, _ = mp.counts_of_rays(oo.group_rays(oracle, list(case["batch"]), p_off, case["spec"], case["motion"],
                                             case["pose2d"], case["t0"]), case["spec"])
    assert (off != want).any() and st == [0]
    inv, _ = case_want(oracle, front_case(1), "front1")
    assert (inv != want).any()


# ---- the rule ---------------------------------------------------------------------------------------------------------------
BIG = 2 ** 31 - 1
# (misses, hits) pairs that sit on every edge of the rule, each with the rule they are meant for in mind; every
# pair is run under every rule of RULES
RULE_COUNTS = (
    (0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2),            # n = min_observations - 1 and = min_observations
    (9, 1), (10, 1), (8, 1), (19, 2), (91, 10), (90, 10), (89, 10),  # 100 h against 10 n and 11 n
    (3, 1), (2, 1), (4, 1),                                   # 100 h against 33 n / 25 n
    (5, 0), (1000, 0),                                        # h = 0 with pct = 0
    (BIG, BIG), (BIG, 1), (1, BIG), (2 ** 32 - 1, 0), (0, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 32 - 1),  # 64-bit products
    (199, 1), (200, 1), (198, 1),                             # mode 1: n = 200 -> 1, n = 201 -> 0
    (0, 7), (0, 200), (7, 7), (1, 2), (2, 1),                 # mode 1: h = n -> 100; halves
)
RULES = (mp.rule(), mp.rule(min_observations=1, occupied_percent=0), mp.rule(min_observations=1, occupied_percent=100),
         mp.rule(min_observations=3, occupied_percent=33), mp.rule(min_observations=11, occupied_percent=10),
         mp.rule(min_observations=1, mode=1), mp.rule(min_observations=5, mode=1))
RULE_SHAPES = ((7, 5), (6, 6), (9, 5), (6, 7))  # width * height = 3, 0, 1, 2 mod 4
RULE_BIG_SHAPE = (67, 31)                        # 2077 cells = 1 mod 4: 520 words, three workgroups of the rule's kernel


def rule_counts(W, H, seed=1420):
    """(H, W, 2) uint32: RULE_COUNTS laid out over the grid again and again, the rest small random counts."""
    rng = np.random.default_rng(seed + W)
    c = rng.integers(0, 4, (H * W, 2)).astype(np.uint32)
    k = len(RULE_COUNTS)
    for i in range(H * W):
        if i % 2 == 0 or i < 2 * k:
            c[i] = RULE_COUNTS[(i // 2) % k]
    return c.reshape(H, W, 2)


def rule_prev(W, H, seed=1421):
    return np.random.default_rng(seed + H).choice(np.array([-1, 0, 100, 37, -128, 127], np.int8), size=(H, W))


# the rule's table, worked out by hand from the text of include/rplgpu_msg.h: (rule, misses, hits, prev) -> byte
RULE_TABLE = (
    (mp.rule(), 1, 0, None, -1), (mp.rule(), 0, 1, 37, 37), (mp.rule(), 2, 0, None, 0), (mp.rule(), 1, 1, None, 100),
    (mp.rule(), 9, 1, None, 100), (mp.rule(), 10, 1, None, 0), (mp.rule(), 19, 2, None, 0), (mp.rule(), 18, 2, None, 100),
    (mp.rule(min_observations=1, occupied_percent=0), 5, 0, None, 0),
    (mp.rule(min_observations=1, occupied_percent=0), 1000, 1, None, 100),
    (mp.rule(min_observations=1, occupied_percent=0), 0, 0, None, -1),
    (mp.rule(min_observations=1, occupied_percent=100), 1, BIG, None, 0),
    (mp.rule(min_observations=1, occupied_percent=100), 0, BIG, None, 100),
    (mp.rule(min_observations=1, occupied_percent=50), BIG, BIG, None, 100),
    (mp.rule(min_observations=1, occupied_percent=51), BIG, BIG, None, 0),
    (mp.rule(min_observations=1, mode=1), 199, 1, None, 1), (mp.rule(min_observations=1, mode=1), 200, 1, None, 0),
    (mp.rule(min_observations=1, mode=1), 0, 9, None, 100), (mp.rule(min_observations=1, mode=1), 9, 0, None, 0),
    (mp.rule(min_observations=1, mode=1), 1, 1, None, 50), (mp.rule(min_observations=1, mode=1), 2, 1, None, 33),
    (mp.rule(min_observations=1, mode=1), 1, 2, None, 67), (mp.rule(min_observations=1, mode=1), BIG, BIG, None, 50),
    (mp.rule(min_observations=1, mode=1), 7, 1, None, 13),  # 12.5 rounds half up
    (mp.rule(min_observations=5, mode=1), 2, 2, 99, 99),
)


# ---- apply -------------------------------------------------------------------------------------------------------------------
APPLY_SPEC = mo.spec(origin_x=-6.4, origin_y=-6.4, resolution=0.05, width=256, height=256, shift_x=9, shift_y=7,
                     rot_steps=5, rot_step=float(F32(math.radians(0.7))))
APPLY_B, APPLY_GROUP = 301, 3  # 101 groups, the last one short; two workgroups of the kernel


def apply_case(seed=1430):
    """Random poses, pivots and best words: most groups unambiguous with k, j, i inside the window, and by
    construction groups with word 6 = 2, word 0 = 0, k = -K - 1, k = K + 1, k = 0x7FFFFFFF and k = 0 with i = j = 0."""
    rng = np.random.default_rng(seed)
    B, group = APPLY_B, APPLY_GROUP
    G = (B + group - 1) // group
    K, Ty, Tx = APPLY_SPEC["rot_steps"], APPLY_SPEC["shift_y"], APPLY_SPEC["shift_x"]
    best = np.zeros((G, 8), np.int64)
    best[:, 0] = rng.integers(1, 10 ** 6, G)
    best[:, 1] = rng.integers(-K, K + 1, G)
    best[:, 2] = rng.integers(-Ty, Ty + 1, G)
    best[:, 3] = rng.integers(-Tx, Tx + 1, G)
    best[:, 4] = rng.integers(1, 5000, G)
    best[:, 5] = rng.integers(0, 100, G)
    best[:, 6] = 1
    best[3, 6] = 2
    best[5, 0] = 0
    best[7, 1] = -K - 1
    best[9, 1] = K + 1
    best[11, 1] = 0x7FFFFFFF
    best[13, 1:4] = 0
    best[15, 1] = -K
    best[17, 1] = K
    a = rng.uniform(0, 2 * math.pi, B)
    pose = rot_poses(a, rng.uniform(-5, 5, B), rng.uniform(-5, 5, B))
    pivot = rng.uniform(-3, 3, (G, 2)).astype(F32)
    return dict(best=mo.best_words(best).reshape(G, 8), pose=pose, pivot=pivot, B=B, group=group, G=G, spec=APPLY_SPEC,
                special=dict(ambiguous=3, empty=5, below=7, above=9, wild=11, identity=13))


def apply_regime():
    c = apply_case()
    sp = c["special"]
    for flags in (0, 1):
        out, pout = mp.apply_match(c["best"], c["spec"], c["pivot"], c["pose"], c["B"], c["group"], flags)
        kept = [g for g in range(c["G"]) if out[3 * g:3 * g + 3].tobytes() == c["pose"][3 * g:3 * g + 3].tobytes()]
        must = {sp["below"], sp["above"], sp["wild"]} | ({sp["ambiguous"], sp["empty"]} if flags else set())
        assert must <= set(kept) and len(kept) <= len(must) + 3, (flags, kept)
        assert (sp["ambiguous"] in kept) == bool(flags)
        for g in must:
            assert pout[g].tobytes() == c["pivot"][g].tobytes()
    return c


# ---- the chain: map -> field -> match -> apply -> map ----------------------------------------------------------------------
CHAIN_DISP = mc.ROOM_DISPLACEMENTS[1]  # (k0, j0, i0) = (2, -3, 4)
CHAIN_RULE = mp.E11_RULE


def chain_want(oracle):
    """The oracle's run of the chain over match_cases' room: dict(counts0, grid0, field, best (8,) int64,
    prior (2, 6), corrected (2, 6), pivot_out (1, 2), counts (final), status)."""
    if "chain" in _CACHE:
        return _CACHE["chain"]
    from tests import inflate_oracle as io
    batch, lens, true_pose = mc.room_scans()
    p = Params.defaults(**mc.ROOM_P)
    occ = mc.room_occ_spec()
    counts0, st0 = mp.map_group(oracle, list(batch), p, occ, None, true_pose)
    grid0, _ = mp.grid_of_counts(counts0, CHAIN_RULE)
    field, _ = io.inflate(grid0, mc.ROOM_TABLE, mc.ROOM_RC, 1)
    prior = mo.displaced_poses(true_pose, mc.ROOM_PIVOT[0], mc.ROOM_SPEC, *CHAIN_DISP)
    _, best, st1 = mo.match_group(oracle, list(batch), p, mc.ROOM_SPEC, field, None, prior, None, mc.ROOM_PIVOT[0])
    corrected, pivot_out = mp.apply_match(mo.best_words(best)[None], mc.ROOM_SPEC, mc.ROOM_PIVOT, prior, 2, 2, 1)
    counts1, st2 = mp.map_group(oracle, list(batch), p, occ, None, corrected)
    _CACHE["chain"] = dict(counts0=counts0, grid0=grid0, field=field, best=best, prior=prior, corrected=corrected,
                           pivot_out=pivot_out, counts=counts0 + counts1, status=(st0, st1, st2), true_pose=true_pose)
    return _CACHE["chain"]


def chain_regime(oracle):
    """The oracle's best is the inverse of the displacement and unambiguous; the corrected poses are the true ones
    up to float32 rounding, so the second time step's rays sharpen the map rather than smear it."""
    w = chain_want(oracle)
    k0, j0, i0 = CHAIN_DISP
    assert tuple(w["best"][1:4]) == (-k0, -j0, -i0) and w["best"][6] == 1 and w["status"] == (0, 0, 0)
    assert np.abs(w["corrected"] - w["true_pose"]).max() < 1e-5 and (w["prior"] != w["true_pose"]).any()
    assert np.array_equal(w["field"], mc.room_field(oracle)[0])  # the E11 identity: E13's own room field
    return w
