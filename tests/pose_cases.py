"""The inputs of tests/test_gpu_pose.py (E15), each with a regime check made from the oracle alone
(tests/pose_oracle.py): the check asserts that the case exercises what it claims, so a green test cannot be an
empty one.  tests/test_pose_cpu.py runs every regime without a device.  If a regime check fails, the input is
what changes, never the check.  TEST INFRASTRUCTURE — imported by tests/ only.

A case is a dict: batch (B, n) nodes, lens, group, p, spec (tests/pose_oracle.spec), fields (F, H, W) int8 with
F = 1 (one map for every group) or F = the number of groups, poses (L, P, 4) float32 with L = 1 (one list for every
group) or L = the number of groups, and optionally motion, pose2d, t0."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi
from tests import inflate_oracle as io
from tests import map_oracle as mp
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import occ_oracle as oo
from tests import pose_oracle as po
from tests.occ_cases import nodes, pad, polar_nodes, rot_poses

F32 = np.float32
_CACHE = {}
FIELD_BYTES = np.array([-128, -1, 0, 1, 99, 100, 127], np.int8)  # every kind of byte the rule names
P_PLAIN = dict(clip_enable=0)


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


def case_want(oracle, case, key=None, p=None, writer=po.weight_bincount):
    """Per group (weights (P,) uint32, result (8,) uint32, status with the truncated bit), once per key."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    n = case["batch"].shape[1]
    out = []
    for g, sl in enumerate(case_groups(case)):
        x, y = case_points(oracle, case, g, p)
        w, res, status = po.score_points(x, y, case_poses(case, g), case["spec"], case_field(case, g), writer)
        if any(int(case["lens"][b]) > n for b in range(sl.start, sl.stop)):
            status |= abi.SCAN_OUT_TRUNCATED
        out.append((w, res, status))
    if key is not None:
        _CACHE[key] = out
    return out


def spec_of(s):
    """A pose spec from any spec dict that has the grid's five values."""
    return po.spec(**{k: s[k] for k in po.DEFAULT})


def poses_around(P, seed, centre, max_rot, max_shift):
    """(P, 4): pose 0 the identity, the others turn by up to max_rot [rad] about `centre` and shift by up to
    max_shift [m] per axis, made from (x, y, theta) doubles by the header's formula."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-max_rot, max_rot, P)
    sh = rng.uniform(-max_shift, max_shift, (P, 2))
    th[0], sh[0] = 0.0, 0.0
    cx, cy = centre
    x = cx - (np.cos(th) * cx - np.sin(th) * cy) + sh[:, 0]
    y = cy - (np.sin(th) * cx + np.cos(th) * cy) + sh[:, 1]
    x[0], y[0] = 0.0, 0.0
    return po.pose_list(np.stack([x, y, th], 1))


# ---- layouts ----------------------------------------------------------------------------------------------------------
# the list of the issue, plus 257 and 320: the two ends of the only `slices` value (3) that list does not reach
LAYOUT_P = (1, 63, 64, 65, 191, 192, 193, 257, 320, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, 3073)
EDGE_W, EDGE_H, EDGE_RES = 64, 40, 0.05


def _edge_base():
    """One scan of about 300 hand-placed returns on and around every border and corner of a 64 x 40 grid of 5 cm
    cells (tests/match_cases.edge_case), the field a pattern of the seven bytes."""
    if "edge" not in _CACHE:
        c = mc.edge_case(EDGE_W, EDGE_H, 0, 0, 0, 0.0)
        _CACHE["edge"] = dict(batch=c["batch"], lens=c["lens"], group=1, p=c["p"], spec=spec_of(c["spec"]),
                              fields=c["fields"], pose2d=c["pose2d"])
    return _CACHE["edge"]


def layout_case(P):
    centre = (EDGE_W * EDGE_RES / 2, EDGE_H * EDGE_RES / 2)
    return dict(_edge_base(), poses=poses_around(P, 1500 + P, centre, 0.4, 0.3)[None])


def layout_regime(oracle, case):
    """Each of the seven bytes is read at some pose, look-ups leave the grid on all four sides, every position
    has a cell, and the weights are not all equal (P > 1)."""
    s = case["spec"]
    W, H = s["width"], s["height"]
    x, y = po.finite_points(*case_points(oracle, case, 0))
    poses = case_poses(case, 0)
    assert len(x) >= 200 and (poses[0] == np.array([1, 0, 0, 0], F32)).all()
    seen = np.zeros(256, bool)
    sides = dict(left=False, right=False, below=False, above=False)
    field = case_field(case, 0)
    for pose in poses[:64]:
        has, cx, cy = po.posed_cells(x, y, pose, s)
        assert has.all()
        sides["left"] |= bool((cx < 0).any())
        sides["right"] |= bool((cx >= W).any())
        sides["below"] |= bool((cy < 0).any())
        sides["above"] |= bool((cy >= H).any())
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        seen[field[cy[ok], cx[ok]].view(np.uint8)] = True
    assert all(sides.values()), sides
    assert all(bool(seen[np.uint8(b)]) for b in FIELD_BYTES)
    w, res, status = case_want(oracle, case, f"layout{len(poses)}")[0]
    assert status == 0 and res[4] == len(x) and (len(poses) == 1 or len(np.unique(w)) > 1)
    return w


def layout_reach():
    """What the kernel's layout formula says LAYOUT_P reaches: (slices values, last-tile sizes of P > 1024,
    every slices value any P can have)."""
    every = sorted({po.layout(P)[1] for P in range(1, po.TILE + 1)})
    got = sorted({po.layout(P)[1] for P in LAYOUT_P})
    last = sorted({po.layout(P)[3] for P in LAYOUT_P if P > po.TILE})
    return got, last, every


# ---- the second pass ------------------------------------------------------------------------------------------------------
PASS_GRID = dict(origin_x=-6.4, origin_y=-6.4, resolution=0.05, width=256, height=256)
PASS_STRIDES = (18432, 32768)
PASS_P = (65, 1025)
PASS_FIRST = 16384  # samples of the first pass of every one of the 8 slices of a scan's passes


def pass_case(n, P):
    """One scan of n samples, every one a return 0.5 .. 7 m away at a random angle."""
    rng = np.random.default_rng(1510 + n)
    scan = polar_nodes(rng.uniform(0, 2 * math.pi, n), rng.uniform(0.5, 7.0, n))
    batch, lens = pad([scan], n)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=po.spec(**PASS_GRID),
                fields=mc.random_field(1511, 1, 256, 256), poses=poses_around(P, 1512 + P, (0.0, 0.0), 3.0, 1.0)[None])


def pass_regime(oracle, case):
    """The weights of the first 16384 samples alone differ from those of the whole scan, at every pose."""
    n = case["batch"].shape[1]
    P = case_poses(case, 0).shape[0]
    w, res, status = case_want(oracle, case, f"pass{n}_{P}")[0]
    head = dict(case, batch=case["batch"][:, :PASS_FIRST], lens=np.minimum(case["lens"], PASS_FIRST))
    wh, resh, _ = case_want(oracle, head, f"pass{n}_{P}_head")[0]
    assert n > PASS_FIRST and res[4] == n and resh[4] == PASS_FIRST and status == 0
    assert (wh < w).all()
    return w


# ---- poses at their limits ------------------------------------------------------------------------------------------------------
ZERO_CELL = (37, 11)  # where the all-zero matrix puts every point; pattern_field has 127 there (asserted)


def limit_poses():
    """name -> (c, s, tx, ty)."""
    nan, inf = float("nan"), float("inf")
    out = {"identity": (1, 0, 0, 0),
           "off_left": (1, 0, -10.0, 0), "off_right": (1, 0, 10.0, 0), "off_below": (1, 0, 0, -10.0),
           "off_above": (1, 0, 0, 10.0), "far": (1, 0, 1.0e7, 0), "scale2": (2, 0, -1.5, -1.0),
           "zero": (0, 0, (ZERO_CELL[0] + 0.5) * EDGE_RES, (ZERO_CELL[1] + 0.5) * EDGE_RES)}
    base = [0.8, 0.6, 0.1, -0.1]
    for i, nm in enumerate(("c", "s", "tx", "ty")):
        for bad, bn in ((nan, "nan"), (inf, "inf"), (-inf, "ninf")):
            v = list(base)
            v[i] = bad
            out[f"{bn}_{nm}"] = tuple(v)
    return out


def limit_case(only=None):
    names = sorted(limit_poses()) if only is None else list(only)
    poses = np.array([limit_poses()[k] for k in names], F32)
    return dict(_edge_base(), poses=poses[None], names=names)


def limit_regime(oracle, case):
    """Per pose, from the oracle: the four off-side poses and the far one weigh 0, only the far and the non-finite
    ones have positions without a cell, scale 2 and the identity weigh something, and the zero matrix weighs
    points x 127."""
    s = case["spec"]
    x, y = po.finite_points(*case_points(oracle, case, 0))
    field = case_field(case, 0)
    assert field[ZERO_CELL[1], ZERO_CELL[0]] == 127
    w, _, no_cell = po.weights_of(x, y, case_poses(case, 0), s, field)
    by = {k: (int(w[i]), bool(no_cell[i])) for i, k in enumerate(case["names"])}
    for k, (wt, nc) in by.items():
        if k.startswith("off_"):
            assert (wt, nc) == (0, False), k
        elif k == "far" or k.split("_")[0] in ("nan", "inf", "ninf"):
            assert (wt, nc) == (0, True), (k, wt, nc)
        elif k == "zero":
            assert (wt, nc) == (127 * len(x), False)
        else:
            assert wt > 0 and not nc, k
    return by


# ---- the largest list --------------------------------------------------------------------------------------------------------
BIG_P = po.MAX_POSES
BIG_DISTINCT = 64


def big_case():
    """P = 2^20 poses drawn from 64 distinct ones over a 16-sample scan."""
    base = _edge_base()
    rng = np.random.default_rng(1530)
    centre = (EDGE_W * EDGE_RES / 2, EDGE_H * EDGE_RES / 2)
    distinct = poses_around(BIG_DISTINCT, 1531, centre, 0.4, 0.3)
    pick = rng.integers(0, BIG_DISTINCT, BIG_P)
    pick[0] = 0
    return dict(base, batch=base["batch"][:, :16].copy(), lens=np.array([16]), poses=distinct[pick][None])


def big_regime(oracle, case):
    w, res, status = case_want(oracle, case, "big")[0]
    assert len(w) == BIG_P and res[4] == 16 and status == 0 and len(np.unique(w)) > 8 and res[2] > 1
    return res


# ---- groups ------------------------------------------------------------------------------------------------------------------------
GROUPS_B, GROUPS_G, GROUPS_N, GROUPS_P = 301, 101, 48, 70
GROUP_SPEC = po.spec(origin_x=-3.2, origin_y=-2.0, resolution=0.1, width=64, height=40)


def groups_case(poses_per_group, field_per_group):
    """301 scans of 48 samples in groups of 3 (the last group has one scan), rings of 0.3 .. 3 m around mounts
    within half a metre of the base; scan 100 claims more samples than the stride holds."""
    rng = np.random.default_rng(1540)
    B, n = GROUPS_B, GROUPS_N
    scans = [polar_nodes(rng.uniform(0, 2 * math.pi, n), rng.uniform(0.3, 3.0, n)) for _ in range(B)]
    batch, lens = pad(scans, n)
    lens[100] = n + 5
    pose2d = rot_poses(rng.uniform(-3, 3, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B))
    L = GROUPS_G if poses_per_group else 1
    poses = np.stack([poses_around(GROUPS_P, 1541 + g, (0.0, 0.0), 3.0, 0.5) for g in range(L)])
    fields = mc.random_field(1542, GROUPS_G if field_per_group else 1, 40, 64)
    return dict(batch=batch, lens=lens, group=3, p=Params.defaults(**P_PLAIN), spec=GROUP_SPEC, fields=fields,
                poses=poses, pose2d=pose2d)


def groups_regime(oracle, case, key):
    want = case_want(oracle, case, key)
    assert len(want) == GROUPS_G
    n = GROUPS_N
    assert [int(r[4]) for _, r, _ in want] == [3 * n] * (GROUPS_G - 1) + [n]
    assert [st for _, _, st in want] == [abi.SCAN_OUT_TRUNCATED if g == 33 else 0 for g in range(GROUPS_G)]
    assert all(r[0] > 0 for _, r, _ in want) and len({w.tobytes() for w, _, _ in want}) == GROUPS_G
    return want


# ---- the full front end -----------------------------------------------------------------------------------------------------------
def front_case(with_pose2d=True):
    """tests/match_cases.front_case (E5 on, inverted, motion with time offsets; 3 scans of 4096 samples, one
    group) with 65 poses anywhere on its 256 x 256 grid."""
    c = mc.front_case()
    case = dict(batch=c["batch"], lens=c["lens"], group=c["group"], p=c["p"], spec=spec_of(c["spec"]),
                fields=c["fields"], motion=c["motion"], t0=c["t0"], pose2d=c["pose2d"],
                poses=poses_around(65, 1550, (0.0, 0.0), 3.1, 1.5)[None])
    if not with_pose2d:
        del case["pose2d"]
    return case


def front_regime(oracle, case, key="front"):
    """E5 decides something: without it the oracle counts more points and the weights differ."""
    want = case_want(oracle, case, key)
    p_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_off.ror_enable = 0
    off = case_want(oracle, case, None, p_off)
    assert off[0][1][4] > want[0][1][4] > 1000 and (off[0][0] != want[0][0]).any() and want[0][2] == 0
    return want


# ---- the identities ------------------------------------------------------------------------------------------------------------------
def identity_a_case():
    """(E13 case with K = 64, Tx = Ty = 1 and no pivot, the E15 case on the same points and field whose list is
    the rotation table's 129 entries)."""
    m = mc.edge_case(EDGE_W, EDGE_H, 1, 1, 64, 0.02)
    m = dict(m, pivot=None)
    rot = mo.rotations(m["spec"])
    poses = np.zeros((len(rot), 4), F32)
    poses[:, :2] = rot
    e = dict(batch=m["batch"], lens=m["lens"], group=1, p=m["p"], spec=spec_of(m["spec"]), fields=m["fields"],
             pose2d=m["pose2d"], poses=poses[None])
    return m, e


def identity_a_regime(oracle):
    """The oracles agree with identity (a), and the 129 weights are not all equal."""
    m, e = identity_a_case()
    vol = mc.case_want(oracle, m, "pose_ida_match")[0][0]
    w = case_want(oracle, e, "pose_ida")[0][0]
    assert len(w) == 129 and w.tobytes() == np.ascontiguousarray(vol[:, 1, 1]).tobytes() and len(np.unique(w)) > 20
    return w


def identity_b_case():
    """The room of tests/match_cases.py (two sensors, 3000 returns, all within obstacle_max of their sensor,
    range_min 0) against a random field: (the E11 / E14 spec, the E15 case with the one pose (1, 0, 0, 0))."""
    batch, lens, pose2d = mc.room_scans()
    o = mc.room_occ_spec()
    e = dict(batch=batch, lens=lens, group=2, p=Params.defaults(**mc.ROOM_P), spec=spec_of(o),
             fields=mc.random_field(1560, 1, o["height"], o["width"]), pose2d=pose2d,
             poses=np.array([[[1, 0, 0, 0]]], F32))
    return o, e


def identity_b_want(oracle):
    """sum over cells of hits x max(field, 0), hits from the E14 oracle on a zeroed map."""
    o, e = identity_b_case()
    if "idb" not in _CACHE:
        counts, status = mp.map_group(oracle, list(e["batch"]), e["p"], o, None, e["pose2d"])
        assert status == 0 and o["range_min"] == 0
        r = oo.group_rays(oracle, list(e["batch"]), e["p"], o, None, e["pose2d"])
        assert r["ray"].all() and (r["d"] <= F32(o["obstacle_max"])).all() and not r["dropped"].any()
        _CACHE["idb"] = int((counts[:, :, 1] * po.field_values(e["fields"][0])).sum()), int(counts[:, :, 1].sum())
    return _CACHE["idb"]


def identity_b_regime(oracle):
    o, e = identity_b_case()
    total, hits = identity_b_want(oracle)
    w, res, status = case_want(oracle, e, "pose_idb")[0]
    assert hits == 2 * mc.ROOM_N == res[4] and int(w[0]) == total > 0 and status == 0
    return total


# ---- the result words ----------------------------------------------------------------------------------------------------------------
WORDS_N = 700      # equal returns in one cell
WORDS_CELL = (10, 10)
WORDS_SPEC = po.spec(**mc.TIE_GRID)  # 32 x 32 cells of 0.25 m, origin (0, 0)


def _words_base(n_points=WORDS_N):
    """n equal returns at angle 0, 2.5 m in front of a mount at (0.125, 2.625): the middle of cell (10, 10)."""
    scan = nodes(np.zeros(n_points, np.int64), np.full(n_points, 10000, np.int64))
    batch, lens = pad([scan], n_points)
    f = np.zeros((1, 32, 32), np.int8)
    f[0, 10, 10], f[0, 10, 12], f[0, 12, 10], f[0, 14, 14] = 127, 99, 99, -128
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN), spec=WORDS_SPEC, fields=f,
                pose2d=np.array([[1, 0, mc.TIE_SENSOR[0], 0, 1, mc.TIE_SENSOR[1]]], F32))


def words_cases():
    """name -> (case, expected (word 0, word 1, word 2, word 3), whether the sum needs its high word)."""
    A, B2, B3, C, U = (1, 0, 0, 0), (1, 0, 0.5, 0), (1, 0, 0, 0.5), (1, 0, 5.0, 0), (1, 0, 1.0, 1.0)
    n = WORDS_N
    out = {}
    ties = np.array([C, B2, A, U, A, B3, A, C], F32)  # the best weight at q = 2, 4 and 6
    out["ties"] = (dict(_words_base(), poses=ties[None]), (127 * n, 2, 3, 3), False)
    zeros = np.array([C, U, (1, 0, -9.0, 0), C, U], F32)  # empty cells, an unknown byte, off the grid
    out["zeros"] = (dict(_words_base(), poses=zeros[None]), (0, 0, 5, 5), False)
    rng = np.random.default_rng(1570)
    pick = rng.choice(3, 70000, p=[0.6, 0.3, 0.1])
    pick[:3] = (2, 1, 0)
    three = np.array([A, B2, C], F32)[pick]
    out["sum64"] = (dict(_words_base(), poses=three[None]),
                    (127 * n, 2, int((pick == 0).sum()), int((pick == 2).sum())), True)
    return out


def words_regime(oracle, name, case, expect, high):
    w, res, status = case_want(oracle, case, f"words_{name}")[0]
    total = sum(int(v) for v in w)
    assert tuple(int(v) for v in res[:4]) == expect and status == 0 and res[4] == WORDS_N, (name, res)
    assert (total >= 2 ** 32) == high and int(res[6]) + (int(res[7]) << 32) == total and res[5] == w[0]
    if name != "zeros":
        assert res[2] > 1 and res[1] > 0  # a tie, and the first of the equals is not pose 0
    return res


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
CHAIN_TRUE = (0.7, -0.4, 0.25)  # the base in the map's frame (x, y, theta)
CHAIN_P = 2048
CHAIN_AT = 777                  # where the true pose is planted in the list
CHAIN_RULE = mp.rule(min_observations=1, occupied_percent=0, mode=0)


def chain_mounts():
    """The room's sensors as mounts in the base frame: inverse(true pose) o (sensor pose in the map), in float64,
    then rounded."""
    _, _, pose2d = mc.room_scans()
    x0, y0, th = CHAIN_TRUE
    c, s = math.cos(th), math.sin(th)
    out = []
    for r00, r01, tx, r10, r11, ty in np.asarray(pose2d, np.float64):
        dx, dy = tx - x0, ty - y0
        out.append([c * r00 + s * r10, c * r01 + s * r11, c * dx + s * dy,
                    -s * r00 + c * r10, -s * r01 + c * r11, -s * dx + c * dy])
    return np.array(out, F32)


def chain_case(oracle):
    """The room's scans on their mounts against the field made of the room's own map, 2048 poses drawn around the
    true one (0.1 .. 0.5 m or 0.05 .. 0.3 rad away), which is planted at CHAIN_AT; pose 0 is a wrong odometry."""
    if "chain_case" in _CACHE:
        return _CACHE["chain_case"]
    batch, lens, pose2d = mc.room_scans()
    o = mc.room_occ_spec()
    counts, status = mp.map_group(oracle, list(batch), Params.defaults(**mc.ROOM_P), o, None, pose2d)
    assert status == 0
    grid, _ = mp.grid_of_counts(counts, CHAIN_RULE)
    field, _ = io.inflate(grid, mc.ROOM_TABLE, mc.ROOM_RC, 1)
    rng = np.random.default_rng(1580)
    ang = rng.uniform(0, 2 * math.pi, CHAIN_P)
    rad = rng.uniform(0.1, 0.5, CHAIN_P)
    dth = rng.uniform(0.05, 0.3, CHAIN_P) * rng.choice([-1, 1], CHAIN_P)
    xyt = np.stack([CHAIN_TRUE[0] + rad * np.cos(ang), CHAIN_TRUE[1] + rad * np.sin(ang), CHAIN_TRUE[2] + dth], 1)
    xyt[CHAIN_AT] = CHAIN_TRUE
    case = dict(batch=batch, lens=lens, group=2, p=Params.defaults(**mc.ROOM_P), spec=spec_of(o), fields=field[None],
                pose2d=chain_mounts(), poses=po.pose_list(xyt)[None], map_pose2d=pose2d, grid=grid)
    _CACHE["chain_case"] = case
    return case


def chain_regime(oracle, case):
    """From the oracle: the planted true pose is the best and the only best; the map's grid is E11's."""
    mc.room_field(oracle)
    assert case["grid"].tobytes() == mc._CACHE["room_field"][0][0].tobytes()
    w, res, status = case_want(oracle, case, "chain")[0]
    assert int(res[1]) == CHAIN_AT and int(res[2]) == 1 and status == 0 and res[4] == 2 * mc.ROOM_N
    assert res[5] < res[0]
    return res


# ---- the known answer -----------------------------------------------------------------------------------------------------------------------
def known_case():
    """A 5 x 5 field of 1 m cells written by hand, 9 returns anywhere, and poses (0, 0, tx, ty): every point lands
    in the one cell of (tx, ty), so the weight is 9 x that cell's byte clipped at 0."""
    f = np.array([[0, 1, 2, 3, 4],
                  [10, 11, 12, 13, 14],
                  [-1, -128, 100, 127, 99],
                  [30, 31, 32, 33, 34],
                  [40, 41, 42, 43, 44]], np.int8)
    cells = [(0, 0), (4, 0), (0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (2, 4), (4, 4), (5, 2), (-1, 0), (2, -1), (2, 5)]
    poses = np.array([(0, 0, cx + 0.5, cy + 0.5) for cx, cy in cells], F32)
    want = [9 * max(int(f[cy, cx]), 0) if 0 <= cx < 5 and 0 <= cy < 5 else 0 for cx, cy in cells]
    rng = np.random.default_rng(1590)
    scan = polar_nodes(rng.uniform(0, 2 * math.pi, 9), rng.uniform(0.5, 7.0, 9))
    batch, lens = pad([scan], 9)
    case = dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN),
                spec=po.spec(origin_x=0.0, origin_y=0.0, resolution=1.0, width=5, height=5), fields=f[None],
                poses=poses[None])
    return case, np.array(want, np.uint32)
