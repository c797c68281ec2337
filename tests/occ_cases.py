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
