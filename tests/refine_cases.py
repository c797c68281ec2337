"""The inputs of tests/test_gpu_refine.py and tests/test_refine_cpu.py (E25), each with a regime check made from the
oracle alone (tests/refine_oracle.py): the check asserts that the case exercises what it claims, so a green test
cannot be an empty one.  If a regime check fails, the input is what changes, never the check.  TEST INFRASTRUCTURE —
imported by tests/ only.

A device case is a dict as tests/pose_cases.py describes (batch, lens, group, p, spec, fields, poses, optionally
motion, pose2d, t0), with spec a tests/refine_oracle.spec.  A point case (the CPU tests and the host twins) is
(x, y, poses, spec, field) with the points already in the base frame."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi
from tests import match_cases as mc
from tests import refine_oracle as ro
from tests.occ_cases import nodes, pad, polar_nodes, rot_poses

F32 = np.float32
_CACHE = {}
P_PLAIN = dict(clip_enable=0)
W, H, RES = 64, 64, 0.05
GRID = dict(origin_x=-1.6, origin_y=-1.6, resolution=RES, width=W, height=H)
SPEC = ro.spec(min_points=3, **GRID)
LENGTHS = (1, 2, 127, 128, 129, 2047, 2048, 2049, 4097)
LAYOUT_P = (1, 2, 63, 64, 65, 1023, 1024, 1025)


def case_groups(case):
    return mc.case_groups(case)


def case_field(case, g):
    f = case["fields"]
    return f[g] if len(f) > 1 else f[0]


def case_poses(case, g):
    q = case["poses"]
    return q[g] if len(q) > 1 else q[0]


def case_points(oracle, case, g, p=None):
    return mc.case_points(oracle, case, g, p)


def case_want(oracle, case, key=None, p=None, iters=0):
    """Per group (poses_out, sums, step, result, status with the truncated bit), once per key.  iters = 0: the sums
    alone (poses_out and step None, result words 0 - 3 zero)."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    n = case["batch"].shape[1]
    out = []
    for g, sl in enumerate(case_groups(case)):
        x, y = case_points(oracle, case, g, p)
        if iters:
            got = ro.refine_points(x, y, case_poses(case, g), case["spec"], case_field(case, g), iters)
        else:
            sums, res, st = ro.sums_of(x, y, case_poses(case, g), case["spec"], case_field(case, g))
            got = (None, sums, None, res, st)
        status = got[4]
        if any(int(case["lens"][b]) > n for b in range(sl.start, sl.stop)):
            status |= abi.SCAN_OUT_TRUNCATED
        out.append(got[:4] + (status,))
    if key is not None:
        _CACHE[key] = out
    return out


# ---- fields -----------------------------------------------------------------------------------------------------------
def likelihood_field(walls, h, w, scale=18.0, top=127):
    """rint(top * exp(-D2 / scale)), D2 the squared distance in cells to the nearest wall cell; (h, w) int8."""
    yy, xx = np.mgrid[0:h, 0:w]
    wy, wx = np.nonzero(walls)
    d2 = np.full((h, w), 1 << 30, np.int64)
    for a, b in zip(wy, wx):
        np.minimum(d2, (yy - a) ** 2 + (xx - b) ** 2, out=d2)
    return np.rint(top * np.exp(-d2 / scale)).astype(np.int8)


def box_field(seed=2500):
    """(1, 64, 64): the likelihood field of a box of walls 12 cells inside the grid, with a sprinkle of unknown
    (negative) bytes."""
    key = ("box", seed)
    if key not in _CACHE:
        walls = np.zeros((H, W), bool)
        walls[12, 12:52] = walls[51, 12:52] = walls[12:52, 12] = walls[12:52, 51] = True
        f = likelihood_field(walls, H, W)
        rng = np.random.default_rng(seed)
        f[rng.random((H, W)) < 0.05] = -1
        f[rng.random((H, W)) < 0.02] = -128
        _CACHE[key] = f[None]
    return _CACHE[key]


def poses_near(P, seed, distinct=9, max_rot=0.05, max_shift=0.06):
    """(P, 4): pose 0 the identity, the others drawn from `distinct` small motions (the oracle computes equal poses
    once)."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-max_rot, max_rot, distinct)
    sh = rng.uniform(-max_shift, max_shift, (distinct, 2))
    th[0], sh[0] = 0.0, 0.0
    base = np.stack([np.cos(th), np.sin(th), sh[:, 0], sh[:, 1]], 1).astype(F32)
    pick = rng.integers(0, distinct, P)
    pick[0] = 0
    return base[pick]


def box_scan(n, rng, noise=0.01):
    """n returns from the origin onto the box's walls (1 m away per side, up to the noise)."""
    th = rng.uniform(0, 2 * math.pi, n)
    half = 0.975  # the wall cells' centres: cell 12 and cell 51 of 64 at 0.05 m around (-1.6, -1.6)
    r = half / np.maximum(np.abs(np.cos(th)), np.abs(np.sin(th))) + rng.normal(0, noise, n)
    return polar_nodes(th, r)


# ---- scan lengths, layouts, groups --------------------------------------------------------------------------------------
def length_case(n):
    """One scan of n samples of the box, three poses."""
    rng = np.random.default_rng(2510 + n)
    batch, lens = pad([box_scan(n, rng)], n)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=SPEC, fields=box_field(),
                poses=poses_near(3, 2511, 3)[None])


def length_regime(oracle, case):
    n = case["batch"].shape[1]
    want = case_want(oracle, case, f"len{n}", iters=1)
    _, sums, step, res, status = want[0]
    d = ro.from_words(sums[0])
    assert res[7] == n == d["n"] and status == 0 and d["dropped"] == 0 and d["sv"] > 0
    if n >= 127:
        assert res[0] == 3 and (step[:, 3] & ro.STEPPED).all() and d["stt"] > 0 and d["sxx"] > 0
    else:
        assert res[1] == 3  # too few points: min_points is 3 per pose only from 3 points on
    return want


def layout_case(P):
    rng = np.random.default_rng(2520)
    batch, lens = pad([box_scan(300, rng)], 300)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=SPEC, fields=box_field(),
                poses=poses_near(P, 2521 + P)[None])


def layout_regime(oracle, case):
    P = case_poses(case, 0).shape[0]
    want = case_want(oracle, case, f"layout{P}", iters=1)
    _, sums, step, res, status = want[0]
    assert status == 0 and res[7] == 300 and res[0] == P
    assert P < 3 or len(np.unique(sums, axis=0)) > 1
    return want


GROUPS_B, GROUPS_N, GROUPS_P = 3, 130, 5


def groups_case(poses_per_group, field_per_group):
    """B = 3 scans of 130 samples with group = 2: the last group is short; scan 1 claims more than the stride."""
    rng = np.random.default_rng(2530)
    scans = [box_scan(GROUPS_N, rng) for _ in range(GROUPS_B)]
    batch, lens = pad(scans, GROUPS_N)
    lens[1] = GROUPS_N + 7
    pose2d = rot_poses(rng.uniform(-0.1, 0.1, GROUPS_B), rng.uniform(-0.05, 0.05, GROUPS_B),
                       rng.uniform(-0.05, 0.05, GROUPS_B))
    L = 2 if poses_per_group else 1
    poses = np.stack([poses_near(GROUPS_P, 2531 + g, 5) for g in range(L)])
    fields = np.concatenate([box_field(2500), box_field(2501)]) if field_per_group else box_field()
    return dict(batch=batch, lens=lens, group=2, p=Params.defaults(**P_PLAIN), spec=SPEC, fields=fields, poses=poses,
                pose2d=pose2d)


def groups_regime(oracle, case, key):
    want = case_want(oracle, case, key, iters=1)
    assert len(want) == 2 and [int(w[3][7]) for w in want] == [2 * GROUPS_N, GROUPS_N]
    assert [w[4] for w in want] == [abi.SCAN_OUT_TRUNCATED, 0]
    assert want[0][1].tobytes() != want[1][1][:, :].tobytes()
    return want


# ---- the third limb ---------------------------------------------------------------------------------------------------------
LEVER = 8191.9  # cells
CORNER = (20, 20)  # the one cell of 127 in the limb field: a point just beyond its centre has Gx, Gy near -32512


def limb_field():
    f = np.zeros((1, H, W), np.int8)
    f[0, CORNER[1], CORNER[0]] = 127
    return f


def lever_pose(x0, y0, lx, ly):
    """The pose (a scale and a turn) that puts the point (x0, y0) at the lever (lx, ly) cells and a sixteenth of a
    cell beyond the centre of CORNER each way (a = b = 16 up to the rounding: |Gx| = |Gy| = 240 * 127), in float64 and
    rounded."""
    ax, ay = lx * RES, ly * RES
    d = x0 * x0 + y0 * y0
    c, s = (x0 * ax + y0 * ay) / d, (x0 * ay - y0 * ax) / d
    tx = GRID["origin_x"] + (CORNER[0] + 0.5625) * RES - ax
    ty = GRID["origin_y"] + (CORNER[1] + 0.5625) * RES - ay
    return np.array([c, s, tx, ty], F32)


def limb_case(oracle, kind):
    """single: one sample 2 m ahead at a lever of (8191.9, -8191.9) cells on the corner cell, so Gt^2 passes 2^64;
    mirror: the lever (-8191.9, 8191.9), so S Gx Gt is negative and its third limb all ones; many: 4097 such samples
    across chunks; deep: 3 x 32768 of them in one group, so S Gx Gt goes below -2^64."""
    n, B = dict(single=(1, 1), mirror=(1, 1), many=(4097, 1), deep=(32768, 3))[kind]
    scan = nodes(np.zeros(n, np.int64), np.full(n, 8000, np.int64))
    batch, lens = pad([scan] * B, n)
    case = dict(batch=batch, lens=lens, group=B, p=Params.defaults(**P_PLAIN), spec=ro.spec(min_points=3, **GRID),
                fields=limb_field())
    x, y = case_points(oracle, dict(case, poses=None), 0)
    sign = 1.0 if kind == "single" else -1.0
    pose = lever_pose(float(x[0]), float(y[0]), sign * LEVER, -sign * LEVER)
    return dict(case, poses=np.stack([pose, np.array([1, 0, 0, 0], F32)])[None])


def limb_regime(oracle, kind, case):
    want = case_want(oracle, case, f"limb_{kind}")
    sums, res, status = want[0][1], want[0][3], want[0][4]
    d = ro.from_words(sums[0])
    n = case["batch"].size
    assert d["n"] == n and d["dropped"] == 0 and status == 0
    assert d["stt"] >= n * 2 ** 64 and sums[0][20] != 0
    if kind == "single":
        assert d["sxt"] > 0
    else:
        assert d["sxt"] < 0 and sums[0][14] == 0xFFFFFFFF or d["sxt"] < -2 ** 64
    if kind == "deep":
        assert d["sxt"] < -2 ** 64 and sums[0][14] not in (0, 0xFFFFFFFF)
    return want


# ---- borders, limits -----------------------------------------------------------------------------------------------------------
def border_case():
    """Nine samples 1 m ahead; zero-matrix poses put them all at one position: the centres of cells -1 and width - 1
    in x (i0 = -1 and i0 = width - 1: one of the four bytes is outside) and the same in y, against a field of 100."""
    scan = nodes(np.zeros(9, np.int64), np.full(9, 4000, np.int64))
    batch, lens = pad([scan], 9)
    ox, oy = GRID["origin_x"], GRID["origin_y"]
    at = lambda i, j: (0, 0, ox + (i + 0.75) * RES, oy + (j + 0.75) * RES)  # noqa: E731  (a = b = 64)
    poses = np.array([at(-1, 30), at(W - 1, 30), at(30, -1), at(30, H - 1), at(-1, -1), at(W - 1, H - 1), at(-3, 30),
                      at(30, H + 2)], F32)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=SPEC,
                fields=np.full((1, H, W), 100, np.int8), poses=poses[None])


def border_regime(oracle, case):
    x, y = ro.finite_points(*case_points(oracle, case, 0))
    i0s, j0s = [], []
    for pose in case_poses(case, 0):
        _, t = ro.terms(x, y, pose, case["spec"], case_field(case, 0))
        i0s.append(int(t["i0"][0]))
        j0s.append(int(t["j0"][0]))
    assert i0s[:6] == [-1, W - 1, 30, 30, -1, W - 1] and j0s[:6] == [30, 30, -1, H - 1, -1, H - 1]
    want = case_want(oracle, case, "border")
    sv = [ro.from_words(w)["sv"] for w in want[0][1]]
    assert all(0 < v < 9 * 100 * 65536 for v in sv[:6]) and sv[6] == sv[7] == 0 and want[0][4] == 0
    return want


def limit_case():
    """Pose 0 the identity; a NaN entry in each place; a pose 2^21 cells away; a lever of 8192 cells."""
    rng = np.random.default_rng(2540)
    batch, lens = pad([box_scan(200, rng)], 200)
    nan = float("nan")
    far = float(2 ** 21 * RES)
    poses = np.array([(1, 0, 0, 0), (nan, 0, 0, 0), (1, nan, 0, 0), (1, 0, nan, 0), (1, 0, 0, nan), (1, 0, far, 0),
                      (1, 0, 0, -far), (9000, 0, 0, 0)], F32)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=SPEC, fields=box_field(),
                poses=poses[None])


def limit_regime(oracle, case):
    want = case_want(oracle, case, "limit", iters=1)
    out, sums, step, res, status = want[0]
    assert status == abi.SCAN_CELL_RANGE and res[7] == 200
    for q in range(1, 8):
        d = ro.from_words(sums[q])
        assert d["n"] == 0 and d["dropped"] == 200 and not sums[q][:27].any(), q
        assert step[q][3] == ro.FEW and out[q].tobytes() == case_poses(case, 0)[q].tobytes()
    assert step[0][3] & ro.STEPPED and tuple(res[:4]) == (1, 7, 0, int(bool(step[0][3] & 0x38)))
    return want


# ---- the full front end ------------------------------------------------------------------------------------------------------------
def front_case():
    """tests/match_cases.front_case (E5 on, inverted, motion with time offsets; 3 scans of 4096 samples, one group)
    on its 256 x 256 grid, five poses."""
    c = mc.front_case()
    s = ro.spec(min_points=3, **{k: c["spec"][k] for k in ("origin_x", "origin_y", "resolution", "width", "height")})
    return dict(batch=c["batch"], lens=c["lens"], group=c["group"], p=c["p"], spec=s, fields=c["fields"],
                motion=c["motion"], t0=c["t0"], pose2d=c["pose2d"], poses=poses_near(5, 2550, 5, 0.5, 1.0)[None])


def front_regime(oracle, case):
    want = case_want(oracle, case, "front", iters=1)
    p_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_off.ror_enable = 0
    off = case_want(oracle, case, None, p_off, iters=1)
    assert off[0][3][7] > want[0][3][7] > 1000 and off[0][1].tobytes() != want[0][1].tobytes()
    return want, off, p_off


# ---- the identity with E15 ------------------------------------------------------------------------------------------------------------
def identity_case(oracle):
    """Every point on a cell centre: samples at angle 0 and ranges that are whole cells, a mount at a cell centre and
    poses that shift by whole cells, on a grid whose origin and resolution are powers of two (every float32 operation
    of the front is exact), so a = b = 0 everywhere and S V / 65536 is E15's weight."""
    res = 0.0625
    s = ro.spec(origin_x=-2.0, origin_y=-2.0, resolution=res, width=64, height=64, target=127, min_points=3)
    r_cells = np.arange(1, 25)
    scan = nodes(np.zeros(len(r_cells), np.int64), (r_cells * res * 4000).astype(np.int64))
    batch, lens = pad([scan], len(scan))
    pose2d = np.array([[1, 0, -2.0 + 8.5 * res, 0, 1, -2.0 + 20.5 * res]], F32)
    poses = np.array([(1, 0, 0, 0), (1, 0, 3 * res, -2 * res), (0, 1, -30 * res, 0), (1, 0, 40 * res, 0)], F32)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=s,
                fields=mc.random_field(2560, 1, 64, 64), pose2d=pose2d, poses=poses[None])


def identity_regime(oracle, case):
    from tests import pose_oracle as po
    x, y = ro.finite_points(*case_points(oracle, case, 0))
    s = case["spec"]
    for pose in case_poses(case, 0):
        keep, t = ro.terms(x, y, pose, s, case_field(case, 0))
        assert keep.all() and not t["a"].any() and not t["b"].any()
    want = case_want(oracle, case, "identity")
    w, _, _ = po.score_points(x, y, case_poses(case, 0), po.spec(**{k: s[k] for k in po.DEFAULT}), case_field(case, 0))
    sv = [ro.from_words(v)["sv"] for v in want[0][1]]
    assert [v % 65536 for v in sv] == [0] * 4 and [v // 65536 for v in sv] == [int(v) for v in w] and max(sv) > 0
    assert len(set(sv)) > 2
    return want, w


# ---- the L-shaped room (convergence, CPU) ----------------------------------------------------------------------------------------------
ROOM_W = 200
ROOM_SPEC = ro.spec(origin_x=-5.0, origin_y=-5.0, resolution=0.05, width=ROOM_W, height=ROOM_W, target=127,
                    min_points=16, max_step_cells=4.0, max_rot=0.2)
# (the walls run through cell centres: a wall on a cell border would bias the field by half a cell)
ROOM_POLY = np.array([(-3.475, -3.475), (3.525, -3.475), (3.525, 0.525), (0.525, 0.525), (0.525, 3.525),
                      (-3.475, 3.525)], float)


def room_points(n=720, noise=0.005, seed=2570):
    """(x, y) float32 in the base frame (the base at (-1.0, -1.2), heading 0.2 rad): n returns from the walls of the
    L-shaped room with `noise` m of range noise; and the true pose (x, y, theta)."""
    true = (-1.0, -1.2, 0.2)
    rng = np.random.default_rng(seed)
    th = 2 * math.pi * np.arange(n) / n
    dx, dy = np.cos(th + true[2]), np.sin(th + true[2])
    best = np.full(n, np.inf)
    for a, b in zip(ROOM_POLY, np.roll(ROOM_POLY, -1, 0)):
        ex, ey = b - a
        den = dx * ey - dy * ex
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((a[0] - true[0]) * ey - (a[1] - true[1]) * ex) / den
            u = ((a[0] - true[0]) * dy - (a[1] - true[1]) * dx) / den
        hit = (np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1)
        best = np.where(hit & (t < best), t, best)
    r = best + rng.normal(0, noise, n)
    return (r * np.cos(th)).astype(F32), (r * np.sin(th)).astype(F32), true


def room_field():
    """(200, 200) int8: rint(127 exp(-D2 / 18)) of the room's walls, rasterised at a tenth of a cell."""
    if "lroom" not in _CACHE:
        walls = np.zeros((ROOM_W, ROOM_W), bool)
        for a, b in zip(ROOM_POLY, np.roll(ROOM_POLY, -1, 0)):
            for t in np.linspace(0, 1, int(np.hypot(*(b - a)) / 0.005) + 1):
                px, py = a + t * (b - a)
                cx, cy = int(math.floor((px + 5.0) / 0.05)), int(math.floor((py + 5.0) / 0.05))
                walls[min(cy, ROOM_W - 1), min(cx, ROOM_W - 1)] = True
        _CACHE["lroom"] = likelihood_field(walls, ROOM_W, ROOM_W)
    return _CACHE["lroom"]


def room_start(true, off_m, off_rad):
    x, y, th = true
    return np.array([math.cos(th + off_rad), math.sin(th + off_rad), x + off_m, y - off_m], F32)


def pose_error(pose, true):
    """(metres, radians) between a (c, s, x, y) pose and the true (x, y, theta)."""
    c, s, x, y = (float(v) for v in pose)
    dth = math.atan2(s, c) - true[2]
    return math.hypot(x - true[0], y - true[1]), abs(math.atan2(math.sin(dth), math.cos(dth)))


# ---- the chain (GPU) ----------------------------------------------------------------------------------------------------------------------
CHAIN_DISP = (2, -3, 4)
CHAIN_ITERS = 3


def chain_case(oracle):
    """tests/match_cases.room_case displaced by (k, j, i) = (2, -3, 4): E13's case, the mounts of its sensors in the
    base frame (the prior poses less the pivot: the base prior has no rotation), and E25's spec on the same grid with
    the target of the room's field (its table's top, 100)."""
    m = mc.room_case(oracle, CHAIN_DISP)
    mounts = m["pose2d"].copy()
    mounts[:, 2] = (m["pose2d"][:, 2] - m["pivot"][0][0]).astype(F32)
    mounts[:, 5] = (m["pose2d"][:, 5] - m["pivot"][0][1]).astype(F32)
    s = ro.spec(target=100, min_points=16, **mc.ROOM_GRID)
    return m, mounts, s
