"""The inputs of tests/test_gpu_agree.py (E23), each with a regime check made from the oracle alone
(tests/agree_oracle.py): the check asserts that the case exercises what it claims, so a green test cannot be an empty
one.  tests/test_agree_cpu.py runs every regime without a device.  If a regime check fails, the input is what changes,
never the check.  TEST INFRASTRUCTURE — imported by tests/ only.

A case is a dict as in tests/pose_cases.py — batch (B, n_stride) nodes, lens, group, p, fields (F, H, W), poses
(L, P, 4), optionally motion, pose2d, t0 — with spec a tests/agree_oracle.spec."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi
from tests import agree_oracle as ao
from tests import match_cases as mc
from tests import pose_cases as pc
from tests import pose_oracle as po
from tests.occ_cases import pad, polar_nodes

F32 = np.float32
_CACHE = {}
P_PLAIN = dict(clip_enable=0)


def agree_spec(grid, **kw):
    return ao.spec(**{k: grid[k] for k in po.DEFAULT}, **kw)


def pose_case(case):
    """The same case for E15 (tests/pose_cases.case_want): the spec cut to its grid."""
    return dict(case, spec=ao.grid_of(case["spec"]))


def case_group_points(oracle, case, g, p=None):
    """(x, y, slot, sample index, scans of the group) of group g, the scans cut as the library reads them."""
    sl = pc.case_groups(case)[g]
    n = case["batch"].shape[1]
    scans = [case["batch"][b][:min(int(case["lens"][b]), n)] for b in range(sl.start, sl.stop)]
    pick = lambda a: None if a is None else a[sl]  # noqa: E731
    x, y, slot, idx = ao.group_xy(oracle, scans, p or case["p"], pick(case.get("motion")), pick(case.get("pose2d")),
                                  pick(case.get("t0")))
    return x, y, slot, idx, len(scans)


def case_want(oracle, case, key=None, p=None, writer="pairs"):
    """Per group (counts (scans, n_stride), mask (scans, words), weights (P,), result (8,), agree (8,), status with the
    truncated bit), once per key."""
    if key is not None and (key, writer) in _CACHE:
        return _CACHE[(key, writer)]
    n = case["batch"].shape[1]
    out = []
    for g, sl in enumerate(pc.case_groups(case)):
        x, y, slot, idx, ns = case_group_points(oracle, case, g, p)
        c, m, w, res, agr, status = ao.agree_points(x, y, slot, idx, ns, n, pc.case_poses(case, g), case["spec"],
                                                    pc.case_field(case, g), writer)
        if any(int(case["lens"][b]) > n for b in range(sl.start, sl.stop)):
            status |= abi.SCAN_OUT_TRUNCATED
        out.append((c, m, w, res, agr, status))
    if key is not None:
        _CACHE[(key, writer)] = out
    return out


def finite_bits(want_group):
    """The mask words of a group's scans (want_group[1]) as booleans (scans, n_stride): the samples kept by the rule."""
    c, m = want_group[0], want_group[1]
    bits = ((m[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(m), -1)[:, :c.shape[1]].astype(bool)
    return bits


# ---- person, lost ------------------------------------------------------------------------------------------------------
PERSON_AT = (700, 730)   # the samples of sensor 0 that a person 0.3 m in front of the wall returns
PERSON_P = 96
ROOM_AGREE = dict(agree_lo=60, keep_num=3, keep_den=10, err_num=9, err_den=10)


def _room_base(oracle):
    if "room" not in _CACHE:
        batch, lens, pose2d = mc.room_scans()
        batch = batch.copy()
        batch[0]["dist_mm_q2"][PERSON_AT[0]:PERSON_AT[1]] -= 1200  # 0.3 m nearer than the wall
        _CACHE["room"] = dict(batch=batch, lens=lens, group=2, p=Params.defaults(**mc.ROOM_P),
                              spec=agree_spec(mc.ROOM_GRID, **ROOM_AGREE), fields=mc.room_field(oracle), pose2d=pose2d)
    return _CACHE["room"]


def person_case(oracle):
    """The room's field, the room's scans with 30 returns of something the map does not hold, 96 poses within 3 cm and
    0.01 rad of the truth."""
    return dict(_room_base(oracle), poses=pc.poses_around(PERSON_P, 2300, (0.0, 0.0), 0.01, 0.03)[None])


def person_regime(oracle, case):
    """At least one finite sample is skipped (the person's, all of them), at least one is kept, the group does not
    fall back, and some pose's weight differs from E15's."""
    c, m, w, res, agr, status = case_want(oracle, case, "person")[0]
    e15 = pc.case_want(oracle, pose_case(case), "agree_person_e15")[0][0]
    F, K, back = int(agr[0]), int(agr[1]), int(agr[2])
    assert F == 2 * mc.ROOM_N and 0 < K < F and back == 0 and agr[3] == K and status == 0
    bits = finite_bits((c, m))
    assert not bits[0, PERSON_AT[0]:PERSON_AT[1]].any() and bits[1].sum() > 1000
    assert (w <= e15).all() and (w < e15).any()
    return w


def lost_case(oracle):
    """The same scans, 96 poses 1.5 .. 3 m and up to half a turn away from the truth."""
    rng = np.random.default_rng(2310)
    ang, rad = rng.uniform(0, 2 * math.pi, PERSON_P), rng.uniform(1.5, 3.0, PERSON_P)
    xyt = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-math.pi, math.pi, PERSON_P)], 1)
    return dict(_room_base(oracle), poses=po.pose_list(xyt)[None])


def lost_regime(oracle, case):
    """The group falls back — the weights are E15's — and the mask still has zero bits at finite samples."""
    c, m, w, res, agr, status = case_want(oracle, case, "lost")[0]
    e15 = pc.case_want(oracle, pose_case(case), "agree_lost_e15")[0]
    F, K = int(agr[0]), int(agr[1])
    assert F == 2 * mc.ROOM_N and K < F and agr[2] == 1 and agr[3] == F
    assert int(finite_bits((c, m)).sum()) == K
    assert w.tobytes() == e15[0].tobytes() and res.tobytes() == e15[1].tobytes()
    return w


# ---- stripes: counts made by hand -------------------------------------------------------------------------------------------
STRIPE_RES = 0.25


def stripe_case(rows, row_values, P, spec_kw, n_stride=None, group=1):
    """A field of len(row_values) rows and P columns of 0.25 m cells, row r holding row_values[r] (P bytes); P poses
    (1, 0, q * 0.25, 0), pose q moving every point q cells along x; scan b has one return in the middle of cell
    (0, r) for every r of rows[b] (a second return in one cell sits 3 cm beside the first).  So the look-up of a
    sample in row r at pose q is row_values[r][q], whatever else happens."""
    H = len(row_values)
    field = np.array(row_values, np.int8).reshape(1, H, P)
    scans = []
    for rr in rows:
        seen = {}
        xs, ys = [], []
        for r in rr:
            k = seen.get(r, 0)
            seen[r] = k + 1
            xs.append((0.5 + 0.12 * k) * STRIPE_RES)
            ys.append((r + 0.5) * STRIPE_RES)
        xs, ys = np.array(xs), np.array(ys)
        scans.append(polar_nodes(np.arctan2(ys, xs), np.hypot(xs, ys)))
    n = max(len(s) for s in scans)
    batch, lens = pad(scans, n_stride or n + 2)
    poses = np.zeros((P, 4), F32)
    poses[:, 0] = 1.0
    poses[:, 2] = np.arange(P) * STRIPE_RES
    grid = dict(origin_x=0.0, origin_y=0.0, resolution=STRIPE_RES, width=P, height=H)
    return dict(batch=batch, lens=lens, group=group, p=Params.defaults(**P_PLAIN), spec=agree_spec(grid, **spec_kw),
                fields=field, poses=poses[None], rows=rows, row_values=row_values)


def stripe_regime(oracle, case):
    """Every sample lands where the construction says: its look-ups are its row's bytes, pose by pose."""
    s = ao.grid_of(case["spec"])
    poses = case["poses"][0]
    for g, rr in enumerate(case["rows"]):
        x, y, slot, idx, _ = case_group_points(oracle, case, g)
        assert len(x) == len(rr) and (idx == np.arange(len(rr))).all()
        for q in (0, len(poses) // 2, len(poses) - 1):
            has, cx, cy = po.posed_cells(x, y, poses[q], s)
            assert has.all() and (cx == q).all() and (cy == np.array(rr)).all()


EDGE_LO = 50
EDGE_CELLS = (32, 33, 64, 0, 31, 34, 1, 63, 48, 16)  # the cells of row r that hold agree_lo; the others hold one less
EDGE_ROWS = ((0, 1, 2, 5, 7, 8),                      # counts 32 (skipped), 33 (kept), 64, 34, 63, 48
             (1, 2, 5, 7, 8, 0, 3, 4, 6, 9),          # 5 of 10 skipped: 5 * 2 == 1 * 10, falls back
             (1, 2, 5, 7, 8, 8, 0, 3, 4, 6))          # 4 of 10 skipped: one short, does not


def edge_case():
    """P = 64, keep 1 / 2, err 1 / 2, three groups of one scan; agree_lo is a byte the field holds and so is
    agree_lo - 1."""
    values = [[EDGE_LO] * c + [EDGE_LO - 1] * (64 - c) for c in EDGE_CELLS]
    return stripe_case(EDGE_ROWS, values, 64, dict(agree_lo=EDGE_LO, keep_num=1, keep_den=2, err_num=1, err_den=2))


def edge_regime(oracle, case):
    stripe_regime(oracle, case)
    want = case_want(oracle, case, "edge")
    c0, m0, w0, _, a0, _ = want[0]
    assert c0[0, :6].tolist() == [32, 33, 64, 34, 63, 48] and int(m0[0, 0]) == 0b111110  # 32 skipped, 33 kept
    assert a0[:6].tolist() == [6, 5, 0, 5, 64, 32]
    # pose 40: rows 0, 1, 5 hold 49 there, rows 2, 7, 8 hold 50; without row 0
    assert int(w0[40]) == 2 * 49 + 3 * 50 and int(w0[0]) == 5 * 50
    a1, a2 = want[1][4], want[2][4]
    sp = case["spec"]
    assert (int(a1[0]) - int(a1[1])) * sp["err_den"] == sp["err_num"] * int(a1[0]) and a1[2] == 1 and a1[3] == 10
    assert a2[:4].tolist() == [10, 6, 0, 6]
    assert int(want[1][2][40]) == sum(50 if 40 < EDGE_CELLS[r] else 49 for r in EDGE_ROWS[1])  # all ten entered
    # `>` in place of `>=` at agree_lo: no look-up would agree at all
    assert max(max(v) for v in case["row_values"]) == EDGE_LO
    return want


def all_from_skipped_case():
    """P = 8, keep 1 / 2: sample 0 agrees at pose 0 only and is skipped; sample 1 agrees at poses 1 .. 7.  Pose 0's
    whole E15 weight is sample 0's."""
    values = [[90, 0, 0, 0, 0, 0, 0, 0], [0, 90, 90, 90, 90, 90, 90, 90]]
    return stripe_case(((0, 1),), values, 8, dict(agree_lo=60, keep_num=1, keep_den=2, err_num=9, err_den=10))


def all_from_skipped_regime(oracle, case):
    stripe_regime(oracle, case)
    c, m, w, res, agr, status = case_want(oracle, case, "all_from_skipped")[0]
    e15_w, e15_res, _ = pc.case_want(oracle, pose_case(case), "agree_afs_e15")[0]
    assert e15_w.tolist() == [90] * 8 and w.tolist() == [0] + [90] * 7 and agr[:4].tolist() == [2, 1, 0, 1]
    assert (int(e15_res[2]), int(e15_res[3])) == (8, 0) and (int(res[2]), int(res[3])) == (7, 1) and res[1] == 1
    return w


# ---- poses at their limits ---------------------------------------------------------------------------------------------------
LIMIT_AGREE = dict(agree_lo=1, keep_num=1, keep_den=10, err_num=99, err_den=100)


def limits_case():
    """tests/pose_cases.limit_case: 20 poses, 13 of them without a cell for any point (not finite, or 10^7 m away)."""
    c = pc.limit_case()
    return dict(c, spec=agree_spec(c["spec"], **LIMIT_AGREE))


def limits_regime(oracle, case):
    """RPLGPU_SCAN_CELL_RANGE is set; the poses without a cell weigh 0 and agree with nothing but stay in P: some
    sample is skipped that would be kept if P were the poses that have a cell."""
    c, m, w, res, agr, status = case_want(oracle, case, "limits")[0]
    names = case["names"]
    P = len(names)
    bad = [i for i, k in enumerate(names) if k == "far" or k.split("_")[0] in ("nan", "inf", "ninf")]
    assert status == abi.SCAN_CELL_RANGE and len(bad) == 13 and all(int(w[i]) == 0 for i in bad)
    with_cell = P - len(bad)
    assert int(agr[4]) <= with_cell and agr[2] == 0
    fin = np.isfinite(case_group_points(oracle, case, 0)[0])
    counts = c[0][:int(fin.sum())]
    s = case["spec"]
    moved = [int(v) for v in counts if ao.kept_by_rule(v, with_cell, s) and not ao.kept_by_rule(v, P, s)]
    assert len(moved) > 5 and 0 < int(agr[1]) < int(agr[0])
    return w


# ---- layouts of the pose list, sample counts, passes ------------------------------------------------------------------------------
LAYOUT_P = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
LAYOUT_AGREE = dict(agree_lo=99, keep_num=3, keep_den=10, err_num=9, err_den=10)


def layout_case(P):
    """tests/pose_cases.layout_case: about 300 returns around a 64 x 40 grid of the seven bytes, P poses around it."""
    c = pc.layout_case(P)
    return dict(c, spec=agree_spec(c["spec"], **LAYOUT_AGREE))


def layout_regime(oracle, case):
    """Samples are kept and skipped, the group does not fall back, the counts are not all equal."""
    P = case["poses"].shape[1]
    c, m, w, res, agr, status = case_want(oracle, case, f"layout{P}")[0]
    assert 0 < agr[1] < agr[0] and agr[2] == 0 and status == 0 and (P == 1 or agr[4] > agr[5])
    return agr


SAMPLE_N = (1, 2, 31, 32, 33, 2047, 2048, 2049, 4097)
SAMPLE_P = 65
SAMPLE_AGREE = dict(agree_lo=99, keep_num=2, keep_den=5, err_num=9, err_den=10)


def samples_case(n, n_stride=None, P=SAMPLE_P):
    """tests/pose_cases.pass_case: one scan of n returns 0.5 .. 7 m away over a random 256 x 256 field of the seven
    bytes (three of seven are >= 99), at a stride above n."""
    c = pc.pass_case(n, P)
    n_stride = n_stride or n + 3
    batch, lens = pad([c["batch"][0]], n_stride)
    return dict(c, batch=batch, lens=lens, spec=agree_spec(c["spec"], **SAMPLE_AGREE))


def samples_regime(oracle, case, key):
    """Every sample is finite; with n >= 31 samples are kept and skipped (3 / 7 against 2 / 5) and nothing falls
    back."""
    n = int(case["lens"][0])
    c, m, w, res, agr, status = case_want(oracle, case, key)[0]
    assert agr[0] == n and status == 0 and (c[0, n:] == 0).all()
    if n >= 31:
        assert 0 < agr[1] < n and agr[2] == 0
    return agr


PASS_STRIDE = 18432  # a slice of the scan's passes runs two of them (tests/pose_cases.PASS_STRIDES)


def pass_regime(oracle, case):
    """Samples beyond the first pass of every slice (16384) are kept and are skipped."""
    agr = samples_regime(oracle, case, "pass")
    c, m = case_want(oracle, case, "pass")[0][:2]
    bits = finite_bits((c, m))[0]
    assert bits[pc.PASS_FIRST:].any() and not bits[pc.PASS_FIRST:].all() and c[0, pc.PASS_FIRST:].max() > 0
    return agr


# ---- groups -------------------------------------------------------------------------------------------------------------------------
def groups_case(poses_per_group, field_per_group):
    """Two groups of one scan.  Group 0 is the person regime's kind (poses near the truth: no fallback), group 1 has
    the same scan rotated half a turn on its mount, which no pose explains: it falls back."""
    n = 600
    th = 2 * math.pi * np.arange(n) / n
    scan = polar_nodes(th, mc._ray_ranges((0.0, 0.0), th))
    bad = polar_nodes(th, 0.45 * mc._ray_ranges((0.0, 0.0), th + 1.0))
    batch, lens = pad([scan, bad], n + 8)
    near = pc.poses_around(70, 2341, (0.0, 0.0), 0.01, 0.03)
    near2 = pc.poses_around(70, 2342, (0.0, 0.0), 0.01, 0.03)
    field = _centre_field()
    fields = np.stack([field, field]) if field_per_group else field[None]
    if field_per_group:
        fields[1] = np.roll(fields[1], 1, axis=1)  # one cell to the right: another map, still the room
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(**P_PLAIN),
                spec=agree_spec(mc.ROOM_GRID, **ROOM_AGREE), fields=fields,
                poses=np.stack([near, near2]) if poses_per_group else near[None])


def _centre_field():
    """(H, W) int8: the room's walls as seen from (0, 0), rasterised by hand (a wall cell 100, its 8 neighbours 80)."""
    if "centre_field" not in _CACHE:
        g = mc.ROOM_GRID
        W, H = g["width"], g["height"]
        f = np.zeros((H, W), np.int8)
        th = 2 * math.pi * np.arange(20000) / 20000
        r = mc._ray_ranges((0.0, 0.0), th)
        cx = np.floor((r * np.cos(th) - g["origin_x"]) / g["resolution"]).astype(int)
        cy = np.floor((r * np.sin(th) - g["origin_y"]) / g["resolution"]).astype(int)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                f[cy + dy, cx + dx] = np.maximum(f[cy + dy, cx + dx], 80)
        f[cy, cx] = 100
        _CACHE["centre_field"] = f
    return _CACHE["centre_field"]


def groups_regime(oracle, case, key):
    want = case_want(oracle, case, key)
    a0, a1 = want[0][4], want[1][4]
    assert a0[2] == 0 and 0 < a0[1] <= a0[0] and a1[2] == 1 and a1[1] < a1[0] and a0[0] == a1[0] == 600
    return want


# ---- the full front end ----------------------------------------------------------------------------------------------------------
FRONT_AGREE = dict(agree_lo=99, keep_num=2, keep_den=5, err_num=9, err_den=10)


def front_case():
    """tests/pose_cases.front_case: E5 on, inverted, motion with time offsets, mount poses; 3 scans of 4096, 65 poses."""
    c = pc.front_case()
    return dict(c, spec=agree_spec(c["spec"], **FRONT_AGREE))


def front_regime(oracle, case):
    """E5 decides something (the oracle without it has more finite points), samples are kept and skipped."""
    want = case_want(oracle, case, "front")
    p_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_off.ror_enable = 0
    off = case_want(oracle, case, None, p_off)
    agr = want[0][4]
    assert off[0][4][0] > agr[0] > 1000 and 0 < agr[1] < agr[0] and agr[2] == 0
    return want


# ---- the identities ------------------------------------------------------------------------------------------------------------------
def identity2_case():
    """A field of bytes 0 and 1 only, agree_lo 1: every agreeing look-up adds exactly 1 to one weight."""
    c = layout_case(65)
    rng = np.random.default_rng(2350)
    f = rng.integers(0, 2, c["fields"].shape).astype(np.int8)
    return dict(c, fields=f, spec=dict(c["spec"], agree_lo=1, err_num=0))  # err_num 0: the weights are E15's


def identity3_case():
    """P = 1, agree_lo 1, keep_num 0, err_num above err_den."""
    c = layout_case(1)
    return dict(c, spec=dict(c["spec"], agree_lo=1, keep_num=0, keep_den=1, err_num=2, err_den=1))


def replaced_batch(case, want):
    """Identity (4): a copy of the batch in which every skipped sample (finite, mask bit 0) is a node E1 drops."""
    batch = case["batch"].copy()
    at = 0
    for g, sl in enumerate(pc.case_groups(case)):
        c, m = want[g][0], want[g][1]
        kept = finite_bits((c, m))
        for k, b in enumerate(range(sl.start, sl.stop)):
            fin = _finite_of_scan(case, b)
            drop = fin & ~kept[k]
            at += int(drop.sum())
            batch[b]["dist_mm_q2"][drop] = 0
    return batch, at


def _finite_of_scan(case, b):
    """Which samples of scan b are finite points, for the cases of identity (4): E5 off, every kept point finite."""
    n = case["batch"].shape[1]
    live = np.zeros(n, bool)
    m = min(int(case["lens"][b]), n)
    live[:m] = case["batch"][b]["dist_mm_q2"][:m] != 0
    return live
