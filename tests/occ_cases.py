"""The inputs of tests/test_gpu_occ.py (E11), each with a regime check made from the oracle alone
(tests/occ_oracle.py): the check asserts that the case exercises what it claims, so a green test cannot
be an empty one.  tests/test_occ_cpu.py runs every regime without a device.
TEST INFRASTRUCTURE — imported by tests/ only."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import occ_oracle as oo

F32 = np.float32
_CACHE = {}


def nodes(q14, dist, quality=200):
    nd = np.zeros(len(q14), abi.NODE_DTYPE)
    nd["angle_z_q14"], nd["dist_mm_q2"], nd["quality"] = q14, dist, quality
    return nd


def polar_nodes(theta, r):
    """Nodes for returns at angle theta [rad, any sign] and range r [m] in the sensor's own convention."""
    q = np.round(np.mod(np.asarray(theta, float), 2 * math.pi) / (2 * math.pi) * 65536).astype(np.int64) % 65536
    return nodes(q, np.round(np.asarray(r, float) * 4000.0).astype(np.int64))


def pad(scans, n):
    """Scans of different lengths as one (B, n) batch and their lengths."""
    out = np.zeros((len(scans), n), abi.NODE_DTYPE)
    for b, s in enumerate(scans):
        out[b, :len(s)] = s
    return out, np.array([len(s) for s in scans], np.int64)


def rot_poses(angles, tx, ty):
    a = np.asarray(angles, float)
    return np.stack([np.cos(a), -np.sin(a), np.asarray(tx, float), np.sin(a), np.cos(a), np.asarray(ty, float)],
                    1).astype(F32)


def case_groups(case):
    B = len(case["batch"])
    group = min(case["group"], B)
    return [slice(g * group, min(B, (g + 1) * group)) for g in range((B + group - 1) // group)]


def case_rays(oracle, case, g, p=None):
    """group_rays of group g of a case (the scans cut to min(len, n_stride), as the library reads them)."""
    sl = case_groups(case)[g]
    n = case["batch"].shape[1]
    scans = [case["batch"][b][:min(int(case["lens"][b]), n)] for b in range(sl.start, sl.stop)]
    pick = lambda a: None if a is None else a[sl]  # noqa: E731
    return oo.group_rays(oracle, scans, p or case["p"], case["spec"], pick(case.get("motion")),
                         pick(case.get("pose2d")), pick(case.get("t0")))


def case_want(oracle, case, key=None, p=None, prev=None):
    """Per group (grid, cells, status with the truncated bit) of a case, computed once per key."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    n = case["batch"].shape[1]
    out = []
    for g, sl in enumerate(case_groups(case)):
        grid, cells, status = oo.grid_of_rays(case_rays(oracle, case, g, p), case["spec"],
                                              None if prev is None else prev[g])
        if any(int(case["lens"][b]) > n for b in range(sl.start, sl.stop)):
            status |= abi.SCAN_OUT_TRUNCATED
        out.append((grid, cells, status))
    if key is not None:
        _CACHE[key] = out
    return out


# ---- small, exact ------------------------------------------------------------------------------------------
# Known answers of the Bresenham rule, worked out by hand from the rule in include/rplgpu_msg.h: end cell
# relative to the sensor cell -> every visited cell, in order (the last is the end cell).
KNOWN_RAYS = {
    (4, 1): [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1)],          # octants; step 3 of this one takes both branches
    (1, 4): [(0, 0), (0, 1), (0, 2), (1, 3), (1, 4)],
    (-1, 4): [(0, 0), (0, 1), (0, 2), (-1, 3), (-1, 4)],
    (-4, 1): [(0, 0), (-1, 0), (-2, 0), (-3, 1), (-4, 1)],
    (-4, -1): [(0, 0), (-1, 0), (-2, 0), (-3, -1), (-4, -1)],
    (-1, -4): [(0, 0), (0, -1), (0, -2), (-1, -3), (-1, -4)],
    (1, -4): [(0, 0), (0, -1), (0, -2), (1, -3), (1, -4)],
    (4, -1): [(0, 0), (1, 0), (2, 0), (3, -1), (4, -1)],
    (3, 0): [(0, 0), (1, 0), (2, 0), (3, 0)],                  # both axes
    (0, -3): [(0, 0), (0, -1), (0, -2), (0, -3)],
    (0, 0): [(0, 0)],                                          # zero length: marks the sensor cell, clears nothing
    (3, 3): [(0, 0), (1, 1), (2, 2), (3, 3)],                  # slope 1: both branches every step
    (5, 2): [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)],  # e2 = 2 and e2 = 4 take both branches
}
SMALL_SPEC = oo.spec(origin_x=1.0, origin_y=-1.0, resolution=0.25, width=16, height=16, range_min=0.0,
                     obstacle_max=10.0, raytrace_max=10.0)
SMALL_SENSOR = (8, 8)  # the known-answer rays start in the middle of this cell


def small_case(oracle):
    """One scan per group: 13 scans of ONE sample each (the known-answer rays, the node found by asking the
    oracle which of the four mirror images of the angle lands in the intended cell), then two scans of 24
    samples whose points sit exactly on cell borders (angle 0 is (cos, sin) = (1, 0) exactly, range 0.25 k m
    is exact): along +x from a sensor left of the grid, and the same turned by 90 degrees."""
    if "small_case" in _CACHE:
        return _CACHE["small_case"]
    res = 0.25
    sx, sy = 1.0 + (SMALL_SENSOR[0] + 0.5) * res, -1.0 + (SMALL_SENSOR[1] + 0.5) * res
    p = Params.defaults(clip_enable=0)
    scans, poses = [], []
    for (ddx, ddy) in KNOWN_RAYS:
        r = math.hypot(ddx * res, ddy * res) if (ddx, ddy) != (0, 0) else 0.05
        th = math.atan2(ddy, ddx)
        pose = np.array([[1, 0, sx, 0, 1, sy]], F32)
        found = None
        for cand in (th, -th, math.pi - th, math.pi + th):
            s = polar_nodes([cand], [r])
            ray = oo.group_rays(oracle, [s], p, SMALL_SPEC, None, pose)
            if (int(ray["x1"][0]), int(ray["y1"][0])) == (SMALL_SENSOR[0] + ddx, SMALL_SENSOR[1] + ddy):
                found = s
                break
        assert found is not None, (ddx, ddy)
        scans.append(found)
        poses.append(pose[0])
    k = np.arange(1, 25)
    border = nodes(np.zeros(24, np.int64), 1000 * k)
    scans += [border, border]
    poses += [np.array([1, 0, 0, 0, 1, 0], F32), np.array([0, -1, 2, 1, 0, 0], F32)]
    batch, lens = pad(scans, 32)
    case = dict(batch=batch, lens=lens, group=1, p=p, spec=SMALL_SPEC, pose2d=np.stack(poses))
    _CACHE["small_case"] = case
    return case


def small_regime(oracle, case):
    n_known = len(KNOWN_RAYS)
    for g, (dd, cells) in enumerate(KNOWN_RAYS.items()):
        r = case_rays(oracle, case, g)
        assert r["ray"].sum() == 1 and not r["dropped"].any() and bool(r["mark"][0])
        assert (int(r["x0"][0]), int(r["y0"][0])) == SMALL_SENSOR
        assert (int(r["x1"][0]) - SMALL_SENSOR[0], int(r["y1"][0]) - SMALL_SENSOR[1]) == dd == cells[-1]
    integral, signs = 0, set()
    for g in (n_known, n_known + 1):
        r = case_rays(oracle, case, g)
        s = case["spec"]
        u = ((r["x"] - F32(s["origin_x"])).astype(F32) / F32(s["resolution"])).astype(F32)
        v = ((r["y"] - F32(s["origin_y"])).astype(F32) / F32(s["resolution"])).astype(F32)
        fu, fv = oo.cell_floor(r["x"], r["y"], s)
        on = (u == fu) & (v == fv)
        integral += int(on.sum())
        signs |= set(np.sign(u[on]).astype(int).tolist()) | set(np.sign(v[on]).astype(int).tolist())
    assert integral >= 16 and {-1, 1} <= signs, (integral, signs)


def known_grid(dd):
    """The grid of one known-answer ray, from the hand-written cells."""
    g = np.full((16, 16), -1, np.int8)
    cells = KNOWN_RAYS[dd]
    for cx, cy in cells[:-1]:
        g[SMALL_SENSOR[1] + cy, SMALL_SENSOR[0] + cx] = 0
    cx, cy = cells[-1]
    g[SMALL_SENSOR[1] + cy, SMALL_SENSOR[0] + cx] = 100
    return g


# ---- grid edges --------------------------------------------------------------------------------------------
EDGE_SPEC = oo.spec(origin_x=-12.85, origin_y=-10.15, resolution=0.1, width=257, height=203, range_min=0.0,
                    obstacle_max=25.0, raytrace_max=30.0)


def edges_case():
    """Two groups of 3 sensors over a 257 x 203 grid (the width no multiple of 4 or 64): one in the middle,
    one 1 m inside the right edge, one 7 m outside it; rings of 4 .. 14 m, so rays leave the grid."""
    B, n = 6, 1500
    batch = synth.make_batch(1110, B, n, noise_m=0.01, r0_range=(4.0, 14.0))
    pose2d = rot_poses([0.0, 0.7, -2.0] * 2, [0.0, 11.8, 20.0] * 2, [0.0, 3.0, -1.0, 1.0, -9.0, 2.0])
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    return dict(batch=batch, lens=np.full(B, n), group=3, p=p, spec=EDGE_SPEC, pose2d=pose2d)


def edges_regime(oracle, case):
    W, H = case["spec"]["width"], case["spec"]["height"]
    for g in range(2):
        r = case_rays(oracle, case, g)
        live = r["ray"] & ~r["dropped"]
        in0 = (r["x0"] >= 0) & (r["x0"] < W) & (r["y0"] >= 0) & (r["y0"] < H)
        in1 = (r["x1"] >= 0) & (r["x1"] < W) & (r["y1"] >= 0) & (r["y1"] < H)
        moved = (r["x0"] != r["x1"]) | (r["y0"] != r["y1"])
        assert (live & in0 & ~in1 & moved).sum() >= 1   # in-grid clears (the sensor cell), out-of-grid end
        assert (live & (np.minimum(r["x0"], r["x1"]) >= W)).sum() >= 1  # the whole walk right of the grid
        assert (~in0[r["slot"] == 2]).all() and in0[r["slot"] == 0].all()


# ---- ranges ------------------------------------------------------------------------------------------------
RANGE_SPEC = oo.spec(origin_x=-20.0, origin_y=-20.0, resolution=0.1, width=400, height=400, range_min=1.0,
                     obstacle_max=5.0, raytrace_max=8.0)


def ranges_case():
    """Two sensors, returns of 0.3 .. 14 m in no order: below range_min, marking, clearing only, cut."""
    rng = np.random.default_rng(1120)
    n = 1200
    scans = [polar_nodes(rng.uniform(0, 2 * math.pi, n), rng.uniform(0.3, 14.0, n)) for _ in range(2)]
    batch, lens = pad(scans, n)
    pose2d = rot_poses([0.3, -1.0], [-2.0, 3.0], [1.0, -2.5])
    return dict(batch=batch, lens=lens, group=2, p=Params.defaults(clip_enable=0), spec=RANGE_SPEC, pose2d=pose2d)


def ranges_regime(oracle, case):
    s = case["spec"]
    r = case_rays(oracle, case, 0)
    d = r["d"]
    below = np.isfinite(d) & (d < F32(s["range_min"]))
    between = r["ray"] & (d > F32(s["obstacle_max"])) & (d <= F32(s["raytrace_max"]))
    assert below.sum() >= 50 and (~r["ray"][below]).all()
    assert between.sum() >= 50 and not r["mark"][between].any() and not r["cut"][between].any()
    assert r["cut"].sum() >= 50 and r["mark"].sum() >= 50
    grid = case_want(oracle, case, "ranges")[0][0]
    cut = np.flatnonzero(r["cut"] & ~r["dropped"])
    assert (grid[r["y1"][cut], r["x1"][cut]] == 0).sum() >= 1  # a cut ray's end cell is cleared, not marked


# ---- marks beat clears, history is kept ------------------------------------------------------------------------
WALL_SPEC = oo.spec(origin_x=-10.0, origin_y=-2.0, resolution=0.05, width=400, height=200, range_min=0.0,
                    obstacle_max=25.0, raytrace_max=30.0)


def wall_case():
    """Three sensors on the x axis face the wall y = 5: the beams that meet it at a shallow angle pass
    through cells that steeper beams of the other sensors end in."""
    scans, n = [], 1400
    for _ in range(3):
        th = np.linspace(math.radians(25), math.radians(155), n)
        scans.append(polar_nodes(th, 5.0 / np.sin(th)))
    batch, lens = pad(scans, n)
    pose2d = rot_poses([0.0, 0.0, 0.0], [-3.0, 0.0, 3.0], [0.0, 0.0, 0.0])
    return dict(batch=batch, lens=lens, group=3, p=Params.defaults(clip_enable=0), spec=WALL_SPEC, pose2d=pose2d)


def wall_prev(case):
    s = case["spec"]
    rng = np.random.default_rng(1130)
    return rng.choice(np.array([-1, 0, 100, 37], np.int8), size=(1, s["height"], s["width"]))


def wall_regime(oracle, case):
    s = case["spec"]
    W, H = s["width"], s["height"]
    r = case_rays(oracle, case, 0)
    clear, marked = oo.bits_vector(*oo.live_rays(r), W, H)
    assert (clear & marked).sum() >= 100, int((clear & marked).sum())
    prev = wall_prev(case)[0]
    untouched = ~clear & ~marked
    assert untouched.sum() >= 1000 and (prev[untouched] == 37).sum() >= 1
    return untouched


# ---- the full front end ------------------------------------------------------------------------------------------
FULL_N, FULL_B, FULL_GROUP = 8192, 20, 8


def full_case(inverted=0, B=FULL_B):
    """Groups of 8 scans of 8192 samples (the 1024-thread loop strides), 1 cm noise, motion, poses on a 0.6 m
    circle, time offsets, E5 on, the default grid; B = 20: the last group is short; scan 5 claims 9000
    samples of a stride of 8192.  Every scan carries isolated returns 1.5 m from its sensor that E5 removes."""
    n = FULL_N
    batch = synth.make_batch(1140, B, n, noise_m=0.01, r0_range=(3.0, 12.0)).copy()
    for b in range(B):
        for i in (1000 + 37 * b, 5000 + 11 * b):
            batch[b]["dist_mm_q2"][i - 2:i + 3] = 0
            batch[b]["dist_mm_q2"][i] = 6000
            batch[b]["quality"][i] = 200
    rng = np.random.default_rng(1141)
    ang = 2 * math.pi * (np.arange(B) % FULL_GROUP) / FULL_GROUP
    pose2d = rot_poses(ang + 0.3, 0.6 * np.cos(ang), 0.6 * np.sin(ang))
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                       for _ in range(B)]).astype(F32)
    t0 = np.random.default_rng(1142).uniform(-0.02, 0.02, FULL_B).astype(F32)[:B]
    lens = np.full(B, n)
    if B > 5:
        lens[5] = 9000
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, inverted=inverted, ror_enable=1,
                        ror_radius=0.10, ror_min_neighbors=2, voxel_enable=1, scan_processing=0)
    return dict(batch=batch, lens=lens, group=FULL_GROUP, p=p, spec=oo.spec(), pose2d=pose2d, motion=motion, t0=t0)


def full_regime(oracle, case, want):
    """E5 decides something: without it group 0's grid differs (a removed return would have marked a cell)."""
    p_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_off.ror_enable = 0
    off, _, _ = oo.grid_of_rays(case_rays(oracle, case, 0, p_off), case["spec"])
    assert (off != want[0][0]).sum() >= 1
    assert want[0][2] == abi.SCAN_OUT_TRUNCATED and want[1][2] == 0 and len(want) == 3


# ---- the cell range -----------------------------------------------------------------------------------------------
def cell_range_case():
    """Two groups of 3: scan 1 stands 1e6 m away (no sensor cell: its rays are dropped and set the bit), scan 4
    has a NaN velocity (its points are NaN: d is not finite, the points are ignored)."""
    B, n = 6, 1024
    batch = synth.make_batch(1150, B, n, noise_m=0.01, r0_range=(2.0, 8.0))
    pose2d = rot_poses(np.linspace(0, 2, B), [0.5, 1.0e6, -0.5, 0.3, 0.0, -1.0], [0.0, 0.0, 1.0, 0.2, 0.4, 0.0])
    motion = np.tile(np.array([0.2, -0.1, 0.1, 0.1 / n], F32), (B, 1))
    motion[4, 0] = np.nan
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    return dict(batch=batch, lens=np.full(B, n), group=3, p=p, spec=oo.spec(width=512, height=512, origin_x=-12.8,
                                                                           origin_y=-12.8), pose2d=pose2d, motion=motion)


def cell_range_regime(oracle, case):
    r0, r1 = case_rays(oracle, case, 0), case_rays(oracle, case, 1)
    assert r0["dropped"][r0["slot"] == 1].all() and (r0["slot"] == 1).sum() > 100
    assert not r0["dropped"][r0["slot"] != 1].any()
    bad = r1["slot"] == 1
    assert bad.sum() > 100 and np.isnan(r1["x"][bad]).all() and not r1["ray"][bad].any()
    assert r1["ray"][~bad].sum() > 1000


# ---- beyond the LDS window ---------------------------------------------------------------------------------------
WIN = 640  # k_occ_walk keeps a scan's clears in a WIN x WIN bit window in LDS, its corner WIN / 2 below the sensor cell
SLOT_KEYS = ("ray", "dropped", "x0", "y0", "x1", "y1", "cut", "mark")


def slot_rays(r, slot):
    """The rays of one scan of a group."""
    m = r["slot"] == slot
    return {k: r[k][m] for k in SLOT_KEYS}


def slot_bits(r, slot, W, H):
    """(cleared, marked) (H, W) bool by the rays of ONE scan of a group."""
    return oo.bits_vector(*oo.live_rays(slot_rays(r, slot)), W, H)


def sensor_cell(r, slot):
    i = int(np.flatnonzero(r["slot"] == slot)[0])
    return int(r["x0"][i]), int(r["y0"][i])


def in_window(x0, y0, W, H):
    """(H, W) bool: the grid cells inside the window of a scan whose sensor cell is (x0, y0)."""
    cx, cy = np.arange(W)[None, :], np.arange(H)[:, None]
    return (cx >= x0 - WIN // 2) & (cx < x0 + WIN // 2) & (cy >= y0 - WIN // 2) & (cy < y0 + WIN // 2)


FAR_SPEC = oo.spec(origin_x=-11.0, origin_y=-9.0, resolution=0.02, width=1101, height=899, range_min=0.0,
                   obstacle_max=9.0, raytrace_max=10.0)
FAR_SENSORS = ((550, 450), (1075, 875), (-450, 450))


def far_case():
    """One group of three sensors over 1101 x 899 cells of 2 cm, returns of 5 .. 14 m at random angles (whole and
    marking up to 9 m, whole and unmarked up to 10 m, cut at 500 cells beyond): a in the middle, its window
    inside the grid on all four sides; b 25 cells inside the top-right corner, its window over two grid edges;
    c 450 cells left of the grid, its window wholly off it."""
    rng = np.random.default_rng(1160)
    n = 1501
    scans = [polar_nodes(rng.uniform(0, 2 * math.pi, n), rng.uniform(5.0, 14.0, n)) for _ in range(3)]
    batch, lens = pad(scans, n)
    s = FAR_SPEC
    tx = [s["origin_x"] + (cx + 0.5) * s["resolution"] for cx, _ in FAR_SENSORS]
    ty = [s["origin_y"] + (cy + 0.5) * s["resolution"] for _, cy in FAR_SENSORS]
    return dict(batch=batch, lens=lens, group=3, p=Params.defaults(clip_enable=0), spec=s,
                pose2d=rot_poses([0.4, -1.1, 2.0], tx, ty))


def far_prev(case):
    s = case["spec"]
    rng = np.random.default_rng(1161)
    return rng.choice(np.array([-1, 0, 100, 37], np.int8), size=(1, s["height"], s["width"]))


def far_regime(oracle, case):
    s = case["spec"]
    W, H = s["width"], s["height"]
    r = case_rays(oracle, case, 0)
    assert not r["dropped"].any()
    assert r["cut"].sum() >= 100 and r["mark"].sum() >= 100 and (r["ray"] & ~r["cut"] & ~r["mark"]).sum() >= 100
    clear, win = [], []
    for slot, cell in enumerate(FAR_SENSORS):
        assert sensor_cell(r, slot) == cell
        clear.append(slot_bits(r, slot, W, H)[0])
        win.append(in_window(*cell, W, H))
    # a: at least 1000 clears beyond each side of its window, and cleared cells in the two columns and the two
    # rows on either side of every window border
    (x0, y0), ys, xs = FAR_SENSORS[0], *np.nonzero(clear[0])
    sides = dict(left=(xs < x0 - WIN // 2).sum(), right=(xs >= x0 + WIN // 2).sum(),
                 below=(ys < y0 - WIN // 2).sum(), above=(ys >= y0 + WIN // 2).sum())
    assert min(sides.values()) >= 1000 and (clear[0] & win[0]).sum() >= 1000, sides
    for d in (-WIN // 2 - 1, -WIN // 2, WIN // 2 - 1, WIN // 2):
        assert clear[0][:, x0 + d].any() and clear[0][y0 + d, :].any(), d
    # b: its window hangs over the right and the top edge; clears beyond it on the two other sides
    (x0, y0), ys, xs = FAR_SENSORS[1], *np.nonzero(clear[1])
    assert x0 + WIN // 2 > W and y0 + WIN // 2 > H
    assert (xs < x0 - WIN // 2).sum() >= 1000 and (ys < y0 - WIN // 2).sum() >= 1000
    # c: every in-grid clear is beyond its window
    assert clear[2].sum() >= 1000 and not (clear[2] & win[2]).any() and not win[2].any()
    assert (clear[2] & ~clear[0] & ~clear[1]).any()
    assert (clear[0] & win[0] & clear[1] & ~win[1]).any()
    return sides


# ---- the window flush: every byte alignment, tiny grids --------------------------------------------------------------
FLUSH_WIDTHS = (64, 61, 62, 63)
FLUSH_H = 40
FLUSH_SENSORS = ((8, 20), (21, 9), (34, 30), (47, 15))  # x0 mod 4 = 0, 1, 2, 3: so is the window corner x0 - 320


def flush_case(W):
    """Four sensors inside a W x 40 grid of 5 cm cells, their window corners at the four residues mod 4, returns
    of 0.3 .. 6 m (up to 120 cells) at random angles: rays clear columns 0 and W - 1 and leave on both sides.
    Run as one group of four and as four groups of one."""
    rng = np.random.default_rng(1170 + W)
    n = 600
    scans = [polar_nodes(rng.uniform(0, 2 * math.pi, n), rng.uniform(0.3, 6.0, n)) for _ in FLUSH_SENSORS]
    batch, lens = pad(scans, n)
    s = oo.spec(origin_x=0.0, origin_y=0.0, resolution=0.05, width=W, height=FLUSH_H)
    pose2d = rot_poses([0.0, 0.9, -0.5, 2.2], [(cx + 0.5) * 0.05 for cx, _ in FLUSH_SENSORS],
                       [(cy + 0.5) * 0.05 for _, cy in FLUSH_SENSORS])
    return dict(batch=batch, lens=lens, group=len(FLUSH_SENSORS), p=Params.defaults(clip_enable=0), spec=s,
                pose2d=pose2d)


def flush_regime(oracle, cases):
    """cases: {W: flush_case(W)}.  -> the set of (W mod 4, corner mod 4) pairs seen."""
    pairs, starts = set(), set()
    below, beyond = False, False
    for W, case in cases.items():
        r = case_rays(oracle, case, 0)
        assert not r["dropped"].any()
        for slot, cell in enumerate(FLUSH_SENSORS):
            assert sensor_cell(r, slot) == cell
            sr = slot_rays(r, slot)
            live = sr["ray"] & ~sr["dropped"]
            assert (live & (sr["x1"] < 0)).any() and (live & (sr["x1"] >= W)).any()  # leave on both sides
            grid = oo.compose(*slot_bits(r, slot, W, FLUSH_H))
            for col in (0, W - 1):  # cleared (and not marked over) in two consecutive rows
                z = grid[:, col] == 0
                assert (z[:-1] & z[1:]).any(), (W, slot, col)
            corner = cell[0] - WIN // 2
            pairs.add((W % 4, corner % 4))
            ys, xs = np.nonzero(grid == 0)
            nib = corner + 4 * ((xs - corner) // 4)  # first cell of the window nibble that holds the cell
            starts |= set(((ys * W + nib) & 3).tolist())
            below |= bool((nib < 0).any())
            beyond |= bool((nib + 3 >= W).any())
    assert pairs == {(a, b) for a in range(4) for b in range(4)} and starts == {0, 1, 2, 3}, (pairs, starts)
    assert below and beyond  # nibbles that begin left of column 0 and that end right of column W - 1
    return pairs


TINY_GRIDS = ((1, 1), (1, 3), (3, 1), (2, 2), (5, 3))


def tiny_case(W, H, outside):
    """One scan of returns at random angles over W x H cells of 25 cm: from a sensor in the middle cell of the
    grid 2 of 0.05 m (they end in the sensor cell), 6 of 0.2 .. 0.6 m and 16 of 0.5 .. 3 m (rays end inside and
    leave; few enough to leave cleared cells unmarked), or, 512 `outside`, of 2.5 .. 4 m from a sensor three cells
    left of and two below the grid's corner (at least 10 cells: every ray that meets the grid crosses it)."""
    rng = np.random.default_rng(1180 + 16 * W + 2 * H + int(outside))
    n = 512 if outside else 24
    rr = rng.uniform(2.5, 4.0, n) if outside else np.concatenate([np.full(2, 0.05), rng.uniform(0.2, 0.6, 6),
                                                                  rng.uniform(0.5, 3.0, 16)])
    scan = polar_nodes(rng.uniform(0, 2 * math.pi, n), rr)
    batch, lens = pad([scan], n)
    s = oo.spec(origin_x=0.0, origin_y=0.0, resolution=0.25, width=W, height=H)
    cx, cy = (-3, -2) if outside else (W // 2, H // 2)
    pose2d = rot_poses([0.3], [(cx + 0.5) * 0.25], [(cy + 0.5) * 0.25])
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=s, pose2d=pose2d,
                sensor=(cx, cy))


def tiny_regime(oracle, case):
    s = case["spec"]
    W, H = s["width"], s["height"]
    r = case_rays(oracle, case, 0)
    assert sensor_cell(r, 0) == case["sensor"] and not r["dropped"].any()
    live = r["ray"] & ~r["dropped"]
    inside = (0 <= case["sensor"][0] < W) and (0 <= case["sensor"][1] < H)
    clear, marked = oo.bits_vector(*oo.live_rays(r), W, H)
    assert clear.any() and marked.any() == inside
    in1 = (r["x1"] >= 0) & (r["x1"] < W) & (r["y1"] >= 0) & (r["y1"] < H)
    assert (live & ~in1).sum() >= 10  # rays that leave (or cross and leave) the grid
    return inside


# ---- rays near the step cap -----------------------------------------------------------------------------------------
LONG_RES = 0.005
LONG_FAR = 3950  # cells between a sensor and the near edge of its grid


def _long_scan(offsets, whole, marked_in, cut):
    """A fan of beams `offsets` angle units (2 pi / 65536) around angle 0, each at every range of the lists."""
    rr = list(whole) + list(marked_in) + list(cut)
    q = np.repeat(np.asarray(offsets, np.int64) % 65536, len(rr))
    return nodes(q, np.round(np.tile(np.asarray(rr, float), len(offsets)) * 4000.0).astype(np.int64))


def long_cases():
    """Three inputs at 5 mm cells with raytrace_max = obstacle_max = 40 m (8000 steps), at most 64 rays each:
    4096 x 8 cells with a sensor 3950 cells left and one 3950 cells right of the grid, beams along +x / -x;
    the same turned by 90 degrees (8 x 4096, +y / -y); 96 x 96 cells with a pair of diagonal beams through it.
    Ranges: 39.6 and 39.9 m (whole, marking, some end cells in the grid), 45 and 60 m (cut at 8000 steps)."""
    fan = (-4, -2, -1, 0, 1, 3)
    scan = _long_scan(fan, [39.9], [39.6, 39.7], [45.0, 60.0])  # 30 samples
    p = Params.defaults(clip_enable=0)
    kw = dict(resolution=LONG_RES, origin_x=0.0, origin_y=0.0, range_min=0.0, obstacle_max=40.0, raytrace_max=40.0)
    at = lambda c: (c + 0.5) * LONG_RES  # noqa: E731
    batch, lens = pad([scan, scan], 32)
    out = []
    lo, hi = -LONG_FAR, 4095 + LONG_FAR
    out.append(dict(batch=batch, lens=lens, group=2, p=p, spec=oo.spec(width=4096, height=8, **kw),
                    pose2d=np.array([[1, 0, at(lo), 0, 1, at(4)], [-1, 0, at(hi), 0, -1, at(3)]], F32)))
    out.append(dict(batch=batch, lens=lens, group=2, p=p, spec=oo.spec(width=8, height=4096, **kw),
                    pose2d=np.array([[0, -1, at(4), 1, 0, at(lo)], [0, 1, at(3), -1, 0, at(hi)]], F32)))
    diag = _long_scan((-40, -8, 0, 8, 40), [39.9], [20.0, 20.2], [45.0])  # the grid's middle is 20.1 m away
    batch, lens = pad([diag, diag], 32)
    out.append(dict(batch=batch, lens=lens, group=2, p=p, spec=oo.spec(width=96, height=96, **kw),
                    pose2d=rot_poses([math.pi / 4, -3 * math.pi / 4], [at(-2800), at(2895)], [at(-2800), at(2895)])))
    return out


def long_regime(oracle, cases):
    seen = dict(px=False, nx=False, py=False, ny=False, diag=False, marked_in=False, cut_in=False)
    for case in cases:
        s = case["spec"]
        W, H = s["width"], s["height"]
        assert oo.spec_valid(s) and case["lens"].max() <= 64
        r = case_rays(oracle, case, 0)
        assert not r["dropped"].any()  # no CELL_RANGE
        live = r["ray"] & ~r["dropped"]
        ddx, ddy = (r["x1"] - r["x0"])[live], (r["y1"] - r["y0"])[live]
        assert max(np.abs(ddx).max(), np.abs(ddy).max()) <= oo.MAX_STEPS
        seen["px"] |= bool((ddx >= 7900).any())
        seen["nx"] |= bool((ddx <= -7900).any())
        seen["py"] |= bool((ddy >= 7900).any())
        seen["ny"] |= bool((ddy <= -7900).any())
        seen["diag"] |= bool(((np.abs(ddx) >= 5000) & (np.abs(ddy) >= 5000)).any())
        in1 = (r["x1"] >= 0) & (r["x1"] < W) & (r["y1"] >= 0) & (r["y1"] < H)
        seen["marked_in"] |= bool((live & in1 & r["mark"] & ~r["cut"]).any())
        seen["cut_in"] |= bool((live & in1 & r["cut"]).any())
    assert all(seen.values()), seen


# ---- lengths ------------------------------------------------------------------------------------------------------
RAGGED_N = 4096
RAGGED_LENS = (0, 1, 129, 1501, 2047, 2048, 2049, 4096, 0, 700, 131)  # a group of 8, then one of 3
RAGGED_X = (-3.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5, -2.0, 0.25, 2.75)


def ragged_case():
    """wall_case's geometry (sensors on the x axis facing the wall y = 5, so runs of consecutive samples end in
    one cell) at every length that matters to the 2048-sample passes of k_occ_walk: empty, one sample, odd
    above one wave, one below / at / one above a pass, two passes; a second, short group that begins with an
    empty scan.  5 % of the samples have no return (E1 removes them); the LAST sample of every scan is a return
    1 m + 0.3 m * scan in front of its sensor, which no other ray ends in."""
    rng = np.random.default_rng(1190)
    scans = []
    for b, L in enumerate(RAGGED_LENS):
        th = np.linspace(math.radians(25), math.radians(155), L) if L > 1 else np.full(L, math.pi / 2)
        s = polar_nodes(th, 5.0 / np.sin(th))
        s["dist_mm_q2"][rng.random(L) < 0.05] = 0
        if L:
            s[-1] = polar_nodes([math.pi / 2], [1.0 + 0.3 * (b % 8)])[0]
        scans.append(s)
    batch, lens = pad(scans, RAGGED_N)
    pose2d = rot_poses(np.zeros(len(scans)), RAGGED_X, np.zeros(len(scans)))
    return dict(batch=batch, lens=lens, group=8, p=Params.defaults(clip_enable=0), spec=WALL_SPEC, pose2d=pose2d)


def ragged_regime(oracle, case):
    s = case["spec"]
    W, H = s["width"], s["height"]
    at128, at_odd, removed = 0, 0, 0
    for g, sl in enumerate(case_groups(case)):
        r = case_rays(oracle, case, g)
        assert not r["dropped"].any()
        live = r["ray"] & ~r["dropped"]
        word = np.stack([r["x1"], r["y1"], r["cut"], r["mark"]], 1)
        marks = live & r["mark"] & ~r["cut"]
        for slot, b in enumerate(range(sl.start, sl.stop)):
            L = int(case["lens"][b])
            m = np.flatnonzero(r["slot"] == slot)
            removed += L - len(m)
            if L == 0:
                assert len(m) == 0  # the empty scan contributes nothing
                continue
            idx = r["idx"][m]
            assert (np.diff(idx) > 0).all()
            # the ray of a sample equals the ray of the sample before it
            dup = (np.diff(idx) == 1) & live[m][1:] & live[m][:-1] & (word[m][1:] == word[m][:-1]).all(1)
            at = idx[1:][dup]
            at128 += int((at % 128 == 0).sum())
            at_odd += int((at % 2 == 1).sum())
            # the last sample: a live, marking ray into a cell of the grid that no other ray of the group marks
            last = m[-1]
            assert idx[-1] == L - 1 and marks[last]
            x1, y1 = int(r["x1"][last]), int(r["y1"][last])
            assert 0 <= x1 < W and 0 <= y1 < H
            assert (marks & (r["x1"] == x1) & (r["y1"] == y1)).sum() == 1, b
    assert at128 >= 1 and at_odd >= 1 and removed >= 100, (at128, at_odd, removed)
    return at128, at_odd


# ---- messages from more than one workgroup ----------------------------------------------------------------------------
MSG_GRIDS = ((300, 300), (2051, 2049))


def msg_kernel_constants():
    """(kChunk, the most workgroups per message) as csrc/rpl_occ.hip has them."""
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    src = (root / "rplidar_ros2_driver_amd" / "csrc" / "rpl_occ.hip").read_text()
    chunk = re.search(r"constexpr uint32_t kChunk = (\d+);", src)
    most = re.search(r"const uint32_t gx = min\(\(n_cells / 4u \+ kChunk - 1\) / kChunk, (\d+)u\);", src)
    assert chunk and most, "k_msg_occupancy's launch geometry moved: look at MSG_GRIDS again"
    return int(chunk.group(1)), int(most.group(1))
