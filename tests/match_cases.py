"""The inputs of tests/test_gpu_match.py (E13), each with a regime check made from the oracle alone
(tests/match_oracle.py): the check asserts that the case exercises what it claims, so a green test cannot be an
empty one.  tests/test_match_cpu.py runs every regime without a device.  If a regime check fails, the input is
what changes, never the check.  TEST INFRASTRUCTURE — imported by tests/ only.

A case is a dict: batch (B, n) nodes, lens, group, p, spec (tests/match_oracle.spec), fields (F, H, W) int8 with
F = 1 (one map for every group) or F = the number of groups, and optionally motion, pose2d, t0, pivot (G, 2)."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import inflate_oracle as io
from tests import match_oracle as mo
from tests import occ_oracle as oo
from tests.occ_cases import nodes, pad, polar_nodes, rot_poses

F32 = np.float32
_CACHE = {}
FIELD_BYTES = np.array([-1, -128, 0, 1, 99, 100, 127], np.int8)  # every kind of byte the rule names


def case_groups(case):
    B = len(case["batch"])
    group = min(case["group"], B)
    return [slice(g * group, min(B, (g + 1) * group)) for g in range((B + group - 1) // group)]


def case_field(case, g):
    f = case["fields"]
    return f[g] if len(f) > 1 else f[0]


def case_points(oracle, case, g, p=None):
    """(x, y) of group g (the scans cut to min(len, n_stride), as the library reads them)."""
    sl = case_groups(case)[g]
    n = case["batch"].shape[1]
    scans = [case["batch"][b][:min(int(case["lens"][b]), n)] for b in range(sl.start, sl.stop)]
    pick = lambda a: None if a is None else a[sl]  # noqa: E731
    x, y, *_ = mo.group_points(oracle, scans, p or case["p"], pick(case.get("motion")), pick(case.get("pose2d")),
                               pick(case.get("t0")))
    return x, y


def case_pivot(case, g):
    return None if case.get("pivot") is None else case["pivot"][g]


def case_want(oracle, case, key=None, p=None, writer=mo.scores_correlate):
    """Per group (volume, best int64 (8,), status with the truncated bit) of a case, computed once per key."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    n = case["batch"].shape[1]
    out = []
    for g, sl in enumerate(case_groups(case)):
        x, y = case_points(oracle, case, g, p)
        vol, best, status = mo.match_points(x, y, case_pivot(case, g), case["spec"], case_field(case, g), writer)
        if any(int(case["lens"][b]) > n for b in range(sl.start, sl.stop)):
            status |= abi.SCAN_OUT_TRUNCATED
        out.append((vol, best, status))
    if key is not None:
        _CACHE[key] = out
    return out


def random_field(seed, F, H, W):
    return np.random.default_rng(seed).choice(FIELD_BYTES, size=(F, H, W))


def pattern_field(H, W, shift=0):
    """(1, H, W): the seven bytes along x and y in steps that are coprime to 7, so even a 5 x 3 grid holds all."""
    yy, xx = np.mgrid[0:H, 0:W]
    return FIELD_BYTES[(3 * xx + 5 * yy + shift) % 7][None]


def nodes_to(points, sensor):
    """Nodes of a sensor at `sensor` (no rotation) whose returns lie at `points` ((m, 2), common frame), up to the
    angle and range quantisation."""
    d = np.asarray(points, float) - np.asarray(sensor, float)
    return polar_nodes(np.arctan2(d[:, 1], d[:, 0]), np.hypot(d[:, 0], d[:, 1]))


# ---- the room: recovery, chain, door --------------------------------------------------------------------------------
ROOM = np.array([(-3, -2), (3, -2), (3, 2), (1, 2), (1, 1.2), (0, 1.2), (0, 2), (-3, 2)], float)  # 6 x 4 m, a notch
ROOM_SENSORS = ((-1.0, -0.5, 0.3), (1.5, -0.8, -1.0))  # x, y, heading
ROOM_N = 1500
ROOM_GRID = dict(origin_x=-6.4, origin_y=-6.4, resolution=0.05, width=256, height=256)
ROOM_SPEC = mo.spec(shift_x=6, shift_y=6, rot_steps=3, rot_step=float(F32(math.radians(1.0))), **ROOM_GRID)
ROOM_PIVOT = np.array([[0.2, -0.1]], F32)
ROOM_RC = 8
ROOM_TABLE = np.array([max(0, 100 - int(12.0 * math.sqrt(k))) for k in range(ROOM_RC * ROOM_RC + 1)], np.uint8)
ROOM_DISPLACEMENTS = ((0, 0, 0), (2, -3, 4), (-3, 5, -5))  # (k0, j0, i0)
ROOM_P = dict(clip_enable=0)


def _ray_ranges(origin, angles):
    """Distance from `origin` along each angle to the room's wall."""
    ox, oy = origin
    dx, dy = np.cos(angles), np.sin(angles)
    best = np.full(len(angles), np.inf)
    for a, b in zip(ROOM, np.roll(ROOM, -1, 0)):
        ex, ey = b - a
        den = dx * ey - dy * ex
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((a[0] - ox) * ey - (a[1] - oy) * ex) / den
            u = ((a[0] - ox) * dy - (a[1] - oy) * dx) / den
        hit = (np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1)
        best = np.where(hit & (t < best), t, best)
    return best


def room_scans():
    """Two sensors x 1500 samples of the room, each sample a node made by hand from (angle, distance)."""
    if "room_scans" in _CACHE:
        return _CACHE["room_scans"]
    scans = []
    for sx, sy, head in ROOM_SENSORS:
        th = 2 * math.pi * np.arange(ROOM_N) / ROOM_N
        scans.append(polar_nodes(th, _ray_ranges((sx, sy), th + head)))
    batch, lens = pad(scans, ROOM_N)
    pose2d = rot_poses([s[2] for s in ROOM_SENSORS], [s[0] for s in ROOM_SENSORS], [s[1] for s in ROOM_SENSORS])
    _CACHE["room_scans"] = (batch, lens, pose2d)
    return _CACHE["room_scans"]


def room_occ_spec():
    return oo.spec(range_min=0.0, obstacle_max=25.0, raytrace_max=30.0, **ROOM_GRID)


def room_field(oracle):
    """(1, H, W) int8: the E11 oracle's grid of the room from the true poses, inflated by the E12 oracle with the
    hand-made non-increasing table (Rc 8, unknown cells inflated too): a likelihood field table[D2]."""
    if "room_field" not in _CACHE:
        batch, lens, pose2d = room_scans()
        grid, _, status = oo.occupancy_group(oracle, list(batch), Params.defaults(**ROOM_P), room_occ_spec(), None, pose2d)
        assert status == 0
        field, _ = io.inflate(grid, ROOM_TABLE, ROOM_RC, 1)
        _CACHE["room_field"] = (grid[None], field[None])
    return _CACHE["room_field"][1]


def room_case(oracle, disp):
    """The room's scans with the prior displaced by disp = (k0, j0, i0) against the room's field."""
    batch, lens, pose2d = room_scans()
    k0, j0, i0 = disp
    return dict(batch=batch, lens=lens, group=2, p=Params.defaults(**ROOM_P), spec=ROOM_SPEC, fields=room_field(oracle),
                pose2d=mo.displaced_poses(pose2d, ROOM_PIVOT[0], ROOM_SPEC, k0, j0, i0), pivot=ROOM_PIVOT, disp=disp)


def room_regime(oracle, case):
    """The oracle's best is the inverse of the displacement, and unambiguous."""
    assert (np.diff(ROOM_TABLE.astype(int)) <= 0).all() and ROOM_TABLE[0] == 100 and ROOM_TABLE.min() >= 0
    k0, j0, i0 = case["disp"]
    vol, best, status = case_want(oracle, case, f"room{case['disp']}")[0]
    assert status == 0 and best[4] == 2 * ROOM_N
    assert tuple(best[1:4]) == (-k0, -j0, -i0) and best[6] == 1, (case["disp"], best)
    assert (best[5] < best[0]) == (case["disp"] != (0, 0, 0))
    return best


# ---- ties -------------------------------------------------------------------------------------------------------------
TIE_GRID = dict(origin_x=0.0, origin_y=0.0, resolution=0.25, width=32, height=32)
TIE_SENSOR = (0.125, 2.625)     # the middle of cell (0, 10)
TIE_POINT_CELL = (10, 10)       # one return at angle 0, range 2.5 m: (2.625, 2.625), the middle of cell (10, 10)


def _tie_case(spec, field, n_points=1, pivot=None):
    scan = nodes(np.zeros(n_points, np.int64), np.full(n_points, 10000, np.int64))
    batch, lens = pad([scan], max(n_points, 4))
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=spec, fields=field[None],
                pose2d=np.array([[1, 0, TIE_SENSOR[0], 0, 1, TIE_SENSOR[1]]], F32), pivot=pivot)


def tie_cases():
    """name -> (case, expected (score, k, j, i), expected number of equals or None)."""
    cx, cy = TIE_POINT_CELL
    out = {}
    s0 = mo.spec(shift_x=3, shift_y=3, rot_steps=0, rot_step=0.0, **TIE_GRID)
    f = np.zeros((32, 32), np.int8)
    f[cy, cx + 1] = 50          # (i, j) = (1, 0): 1
    f[cy + 2, cx] = 50          # (0, 2): 4
    out["distance"] = (_tie_case(s0, f), (50, 0, 0, 1), 2)
    f = np.zeros((32, 32), np.int8)
    for i, j in ((1, 2), (-1, 2), (2, -1), (-2, -1)):  # all at 5: the smallest j, then the smallest i
        f[cy + j, cx + i] = 70
    out["signs"] = (_tie_case(s0, f), (70, 0, -1, -2), 4)
    # K 2, 0.15 rad about the sensor: the return moves 0.37 m per step, more than a cell.  100 inside a disc around
    # its cell but 0 in the cell itself: the four turned positions tie at no shift, |k| and then k decide
    s2 = mo.spec(shift_x=2, shift_y=2, rot_steps=2, rot_step=0.15, **TIE_GRID)
    yy, xx = np.mgrid[0:32, 0:32]
    f = np.where((xx - cx) ** 2 + (yy - cy) ** 2 <= 36, 100, 0).astype(np.int8)
    f[cy, cx] = 0
    out["rotations"] = (_tie_case(s2, f, pivot=np.array([TIE_SENSOR], F32)), (100, -1, 0, 0), None)
    f = np.full((32, 32), 100, np.int8)
    out["uniform"] = (_tie_case(s2, f, n_points=5, pivot=np.array([TIE_SENSOR], F32)), (500, 0, 0, 0),
                      mo.volume_size(s2))
    return out


def tie_regime(oracle, name, case, expect, equals):
    vol, best, status = case_want(oracle, case, f"tie_{name}")[0]
    assert status == 0 and tuple(best[:4]) == expect, (name, best)
    assert best[6] >= 2 and (equals is None or best[6] == equals), (name, best)
    if name == "rotations":
        K = case["spec"]["rot_steps"]
        c = case["spec"]["shift_y"], case["spec"]["shift_x"]
        at = [int(vol[K + k, c[0], c[1]]) for k in (-2, -1, 0, 1, 2)]
        assert at == [100, 100, 0, 100, 100], at
    return best


# ---- the edges of the window --------------------------------------------------------------------------------------------
EDGE_WIDTHS = (61, 62, 63, 64)
EDGE_H = 40


def _edge_points(W, H, res, rng, n_random):
    """Cell centres on every border and corner of a W x H grid, one and three cells outside it, and random ones."""
    xs = [0, 1, W // 2, W - 2, W - 1, -1, -3, W, W + 2]
    ys = [0, 1, H // 2, H - 2, H - 1, -1, -3, H, H + 2]
    cells = [(x, y) for x in xs for y in ys]
    pts = (np.array(cells, float) + 0.5) * res
    rnd = rng.uniform([-3 * res, -3 * res], [(W + 3) * res, (H + 3) * res], (n_random, 2))
    return np.concatenate([pts, rnd])


def edge_case(W=64, H=EDGE_H, Tx=6, Ty=6, K=1, rot_step=0.01, seed=1300, n_random=220):
    """One scan of hand-placed returns on and around every border and corner of a W x H grid of 5 cm cells, the
    field a pattern of the seven bytes."""
    rng = np.random.default_rng(seed + W + 7 * H)
    res = 0.05
    sensor = ((W / 2 + 0.37) * res, (H / 2 + 0.21) * res)
    scan = nodes_to(_edge_points(W, H, res, rng, n_random), sensor)
    batch, lens = pad([scan], len(scan))
    s = mo.spec(origin_x=0.0, origin_y=0.0, resolution=res, width=W, height=H, shift_x=Tx, shift_y=Ty, rot_steps=K,
                rot_step=rot_step)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=s,
                fields=pattern_field(H, W, W), pose2d=np.array([[1, 0, sensor[0], 0, 1, sensor[1]]], F32),
                pivot=np.array([sensor], F32))


def edge_cases():
    """name -> case: widths 61 .. 64 (rows starting at every byte of a word), a 5 x 3 grid with T 32, T 32 with
    K 0, K 64 with T 0, Tx != Ty."""
    out = {f"w{W}": edge_case(W) for W in EDGE_WIDTHS}
    out["tiny_t32"] = edge_case(5, 3, 32, 32, 1, 0.05, n_random=40)
    out["t32_k0"] = edge_case(64, EDGE_H, 32, 32, 0, 0.0, n_random=60)
    out["k64_t0"] = edge_case(64, EDGE_H, 0, 0, 64, 0.02)
    out["tx7_ty2"] = edge_case(63, EDGE_H, 7, 2, 1, 0.01)
    return out


def edge_regime(oracle, name, case):
    """Look-ups leave the grid on every side; every one of the seven bytes lies under some point at some candidate."""
    s = case["spec"]
    assert mo.spec_valid(s)
    W, H, Tx, Ty, K = s["width"], s["height"], s["shift_x"], s["shift_y"], s["rot_steps"]
    x, y = case_points(oracle, case, 0)
    rot = mo.rotations(s)
    pv = case["pivot"][0]
    seen = np.zeros(256, bool)
    sides = dict(left=False, right=False, below=False, above=False)
    field = case_field(case, 0)
    for kk in range(2 * K + 1):
        has, cx, cy = mo.rotated_cells(x, y, pv[0], pv[1], rot[kk, 0], rot[kk, 1], s)
        assert has.all()
        sides["left"] |= bool((cx - Tx < 0).any()) if Tx else bool((cx < 0).any())
        sides["right"] |= bool((cx + Tx >= W).any())
        sides["below"] |= bool((cy - Ty < 0).any()) if Ty else bool((cy < 0).any())
        sides["above"] |= bool((cy + Ty >= H).any())
        for j in range(-Ty, Ty + 1):
            for i in range(-Tx, Tx + 1):
                ax, ay = cx + i, cy + j
                ok = (ax >= 0) & (ax < W) & (ay >= 0) & (ay < H)
                seen[field[ay[ok], ax[ok]].view(np.uint8)] = True
    assert all(sides.values()), (name, sides)
    counts = {int(b): bool(seen[np.uint8(b)]) for b in FIELD_BYTES}
    assert all(counts.values()), (name, counts)
    return counts


# ---- passes and weights -------------------------------------------------------------------------------------------------
PASS_GRID = dict(origin_x=-10.0, origin_y=-2.0, resolution=0.05, width=400, height=200)
PASS_SPEC = mo.spec(shift_x=2, shift_y=3, rot_steps=1, rot_step=0.004, **PASS_GRID)
PASS_LENS = (1, 2047, 2048, 2049, 4097)
PASS_N = 4100
ONE_CELL = (230, 100)  # where the 4096 equal samples land


def _wall_scan(L, rng):
    """A sensor on the x axis facing the wall y = 5: runs of consecutive samples end in one cell; 5 % of the
    samples have no return."""
    th = np.linspace(math.radians(25), math.radians(155), L) if L > 1 else np.full(L, math.pi / 2)
    s = polar_nodes(th, 5.0 / np.sin(th))
    s["dist_mm_q2"][rng.random(L) < 0.05] = 0
    if L == 1:
        s["dist_mm_q2"][0] = 20000
    return s


def _one_cell_scan(L):
    """L equal returns at angle 0, 1.5 m in front of a sensor at (0.025, 3.025): the middle of cell ONE_CELL."""
    return nodes(np.zeros(L, np.int64), np.full(L, 6000, np.int64))


def _pass_field():
    f = random_field(1310, 1, PASS_GRID["height"], PASS_GRID["width"])
    f[0, ONE_CELL[1] - 4:ONE_CELL[1] + 5, ONE_CELL[0] - 4:ONE_CELL[0] + 5] = 0  # nothing else within the window
    f[0, ONE_CELL[1], ONE_CELL[0]] = 100
    return f


def passes_case():
    """Groups of ONE scan: the wall at every length that matters to the 2048-sample passes, a scan whose 4096
    samples all land in one cell of value 100, a scan with no kept sample, an empty scan."""
    rng = np.random.default_rng(1311)
    scans = [_wall_scan(L, rng) for L in PASS_LENS]
    scans.append(_one_cell_scan(4096))
    scans.append(nodes(np.arange(1000) * 60, np.zeros(1000, np.int64)))  # no return anywhere: E1 keeps nothing
    scans.append(np.zeros(0, abi.NODE_DTYPE))
    batch, lens = pad(scans, PASS_N)
    xs = [-3.0, -1.5, 0.0, 1.5, 3.0, 0.025, 0.5, 1.0]
    ys = [0.0] * 5 + [3.025, 0.0, 0.0]
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=PASS_SPEC, fields=_pass_field(),
                pose2d=rot_poses(np.zeros(len(scans)), xs, ys))


def weights_case():
    """ONE group of 8 one-cell scans: many workgroups add into the same candidates; and a second, empty group."""
    scans = [_one_cell_scan(4096) for _ in range(8)] + [np.zeros(0, abi.NODE_DTYPE)] * 3
    batch, lens = pad(scans, 4096)
    n = len(scans)
    return dict(batch=batch, lens=lens, group=8, p=Params.defaults(clip_enable=0), spec=PASS_SPEC, fields=_pass_field(),
                pose2d=rot_poses(np.zeros(n), [0.025] * n, [3.025] * n))


def passes_regime(oracle, case):
    want = case_want(oracle, case, "passes")
    n_lens = len(PASS_LENS)
    runs = 0
    for g in range(n_lens):
        x, y = case_points(oracle, case, g)
        assert 0 < want[g][1][4] == len(x) <= PASS_LENS[g] and want[g][1][0] > 0
        has, cx, cy = oo.cells_of(x, y, case["spec"])
        runs += int(((cx[1:] == cx[:-1]) & (cy[1:] == cy[:-1])).sum())
    assert runs >= 1000  # consecutive samples in one cell: the weight path
    vol, best, _ = want[n_lens]
    K, Ty, Tx = PASS_SPEC["rot_steps"], PASS_SPEC["shift_y"], PASS_SPEC["shift_x"]
    assert best[4] == 4096 and vol[K, Ty, Tx] == 100 * 4096 == best[5] == best[0]
    for g in (n_lens + 1, n_lens + 2):  # no kept sample; no sample
        assert not want[g][0].any() and tuple(want[g][1]) == (0, 0, 0, 0, 0, 0, mo.volume_size(PASS_SPEC), 0)
    return runs


def weights_regime(oracle, case):
    want = case_want(oracle, case, "weights")
    K, Ty, Tx = PASS_SPEC["rot_steps"], PASS_SPEC["shift_y"], PASS_SPEC["shift_x"]
    assert len(want) == 2 and want[0][1][4] == 8 * 4096 and want[0][0][K, Ty, Tx] == 100 * 8 * 4096
    assert not want[1][0].any() and tuple(want[1][1]) == (0, 0, 0, 0, 0, 0, mo.volume_size(PASS_SPEC), 0)


# ---- groups -----------------------------------------------------------------------------------------------------------------
GROUP_GRID = dict(origin_x=-6.4, origin_y=-6.4, resolution=0.05, width=256, height=256)
GROUP_SPEC = mo.spec(shift_x=3, shift_y=2, rot_steps=2, rot_step=0.01, **GROUP_GRID)


def groups_case(per_group=1):
    """B = 7 in groups of 3 (a ragged last group), random returns of 0.5 .. 7 m, poses, motion; scan 1 stands
    1e6 m away (its rotated points have no cell: CELL_RANGE for group 0, the other scans still count), scan 4
    has a NaN velocity (its points are NaN and ignored), scan 5 claims more samples than the stride holds."""
    rng = np.random.default_rng(1320)
    B, n = 7, 600
    scans = [polar_nodes(rng.uniform(0, 2 * math.pi, n), rng.uniform(0.5, 7.0, n)) for _ in range(B)]
    batch, lens = pad(scans, n)
    lens[5] = n + 7
    pose2d = rot_poses(np.linspace(0, 2, B), [0.5, 1.0e6, -0.5, 0.3, 0.0, -1.0, 0.8], [0.0, 0.0, 1.0, 0.2, 0.4, 0.0, -0.6])
    motion = np.tile(np.array([0.2, -0.1, 0.1, 0.1 / n], F32), (B, 1))
    motion[4, 0] = np.nan
    pivot = np.array([[0.1, 0.2], [-0.3, 0.0], [0.0, 0.5]], F32)
    return dict(batch=batch, lens=lens, group=3, p=Params.defaults(clip_enable=0), spec=GROUP_SPEC,
                fields=random_field(1321, 3 if per_group else 1, 256, 256), pose2d=pose2d, motion=motion, pivot=pivot)


def groups_regime(oracle, case, key):
    want = case_want(oracle, case, key)
    n = case["batch"].shape[1]
    assert len(want) == 3
    assert want[0][2] == abi.SCAN_CELL_RANGE and want[0][1][4] == 3 * n and want[0][1][0] > 0
    x, y = case_points(oracle, case, 1)
    assert np.isnan(x).sum() == n and want[1][1][4] == 2 * n
    assert want[1][2] == abi.SCAN_OUT_TRUNCATED and want[2][2] == 0 and want[2][1][4] == n
    return want


# ---- the full front end -----------------------------------------------------------------------------------------------------
def front_case(B=3):
    """E5 on, inverted, motion with time offsets and a pivot away from the origin, all at once: 3 scans of 4096
    samples (1 cm noise) with isolated returns that E5 removes, one group."""
    n = 4096
    batch = synth.make_batch(1330, B, n, noise_m=0.01, r0_range=(2.0, 5.5)).copy()
    for b in range(B):
        for i in (1000 + 37 * b, 3000 + 11 * b):
            batch[b]["dist_mm_q2"][i - 2:i + 3] = 0
            batch[b]["dist_mm_q2"][i] = 4000
            batch[b]["quality"][i] = 200
    rng = np.random.default_rng(1331)
    ang = 2 * math.pi * np.arange(B) / B
    pose2d = rot_poses(ang + 0.3, 0.6 * np.cos(ang), 0.6 * np.sin(ang))
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                       for _ in range(B)]).astype(F32)
    t0 = rng.uniform(-0.02, 0.02, B).astype(F32)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, inverted=1, ror_enable=1,
                        ror_radius=0.10, ror_min_neighbors=2)
    return dict(batch=batch, lens=np.full(B, n), group=B, p=p, spec=GROUP_SPEC, fields=random_field(1332, 1, 256, 256),
                pose2d=pose2d, motion=motion, t0=t0, pivot=np.array([[0.4, -0.3]], F32))


def front_regime(oracle, case):
    """E5 decides something: without it the oracle counts more points and the volume differs."""
    want = case_want(oracle, case, "front")
    p_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_off.ror_enable = 0
    off = case_want(oracle, case, None, p_off)
    assert off[0][1][4] > want[0][1][4] > 1000 and (off[0][0] != want[0][0]).any()
    return want
