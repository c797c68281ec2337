"""Restatement of E11, the ray-cast occupancy grid of a group of scans (include/rplgpu_msg.h,
rplgpu_occupancy_grid_dev), and of the serialised nav_msgs/OccupancyGrid.  TEST INFRASTRUCTURE — imported
by tests/ only.

Points: tests/fused_oracle.group_points, the composition E8 and E9 use (E1 + E2 by the C oracle, E5 on the
scan's own points, E6 and the planar pose by oracle/fusion_oracle.py).  On top of it, in numpy float32, the
cell rule and the cut, and the all-integer Bresenham in two forms: vectorised over rays (one numpy step per
Bresenham step, rays masked out as they finish) and a per-ray pure-Python walk for small inputs."""
from __future__ import annotations

import struct

import numpy as np

from tests.fused_oracle import group_points

F32 = np.float32
CELL_LIMIT = F32(1048576.0)
MAX_DIM = 4096
MAX_STEPS = 8192
SCAN_CELL_RANGE = 0x2
DEFAULT = dict(origin_x=-25.6, origin_y=-25.6, resolution=0.05, width=1024, height=1024, range_min=0.0,
               obstacle_max=25.0, raytrace_max=30.0)


def spec(**kw) -> dict:
    d = dict(DEFAULT)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return d


def spec_valid(s: dict) -> bool:
    f = [F32(s[k]) for k in ("origin_x", "origin_y", "resolution", "range_min", "obstacle_max", "raytrace_max")]
    if not all(np.isfinite(v) for v in f):
        return False
    _, _, res, rmin, omax, tmax = f
    if not res > 0:
        return False
    if not (1 <= s["width"] <= MAX_DIM and 1 <= s["height"] <= MAX_DIM):
        return False
    if not (F32(0) <= rmin < omax <= tmax):
        return False
    return float(tmax) / float(res) <= MAX_STEPS


# ---- the cell rule ----------------------------------------------------------------------------------
def cell_floor(x, y, s):
    """(fu, fv) float32 of positions: u = (x - origin_x) / resolution, fu = floorf(u); all float32."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    with np.errstate(all="ignore"):
        fu = np.floor(((x - F32(s["origin_x"])).astype(F32) / F32(s["resolution"])).astype(F32))
        fv = np.floor(((y - F32(s["origin_y"])).astype(F32) / F32(s["resolution"])).astype(F32))
    return fu.astype(F32), fv.astype(F32)


def cells_of(x, y, s):
    """(has cell, cx, cy): no cell when fu or fv is NaN or has magnitude >= 1048576."""
    fu, fv = cell_floor(x, y, s)
    with np.errstate(invalid="ignore"):
        has = (np.abs(fu) < CELL_LIMIT) & (np.abs(fv) < CELL_LIMIT)
    cx = np.where(has, fu, 0).astype(np.int64)
    cy = np.where(has, fv, 0).astype(np.int64)
    return has, cx, cy


# ---- points -> rays ----------------------------------------------------------------------------------
def rays_of(x, y, sx, sy, s):
    """Per point (x, y) seen from (sx, sy), all float32 arrays of one length:
    dict(ray bool — the point is not ignored; dropped bool — a ray without a sensor or end cell;
         x0, y0, x1, y1 int64; cut bool; mark bool; d float32) with the cells valid where ray & ~dropped."""
    x, y, sx, sy = (np.asarray(v, F32) for v in (x, y, sx, sy))
    with np.errstate(all="ignore"):
        dx, dy = (x - sx).astype(F32), (y - sy).astype(F32)
        d = np.sqrt(((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)).astype(F32)
        ray = np.isfinite(d) & ~(d < F32(s["range_min"]))
        whole = d <= F32(s["raytrace_max"])
        t = (F32(s["raytrace_max"]) / d).astype(F32)
        ex = np.where(whole, x, (sx + (dx * t).astype(F32)).astype(F32)).astype(F32)
        ey = np.where(whole, y, (sy + (dy * t).astype(F32)).astype(F32)).astype(F32)
        mark = whole & (d <= F32(s["obstacle_max"]))
    has0, x0, y0 = cells_of(sx, sy, s)
    has1, x1, y1 = cells_of(ex, ey, s)
    dropped = ray & ~(has0 & has1)
    return dict(ray=ray, dropped=dropped, x0=x0, y0=y0, x1=x1, y1=y1, cut=ray & ~whole, mark=ray & mark, d=d)


def live_rays(r):
    """(x0, y0, x1, y1, cut, mark) of the rays that are walked, duplicates removed (the result is a set)."""
    m = r["ray"] & ~r["dropped"]
    a = np.stack([r["x0"][m], r["y0"][m], r["x1"][m], r["y1"][m], r["cut"][m].astype(np.int64),
                  r["mark"][m].astype(np.int64)], 1)
    a = np.unique(a, axis=0) if len(a) else a.reshape(0, 6)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4].astype(bool), a[:, 5].astype(bool)


# ---- the walk, per ray in pure Python -------------------------------------------------------------------
def walk_cells(x0, y0, x1, y1):
    """The cells the spec's Bresenham visits from (x0, y0) to (x1, y1), in order, both ends included."""
    x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
    ax, ay = abs(x1 - x0), abs(y1 - y0)
    stepx = (x1 > x0) - (x1 < x0)
    stepy = (y1 > y0) - (y1 < y0)
    err = ax - ay
    x, y = x0, y0
    out = [(x, y)]
    while (x, y) != (x1, y1):
        e2 = 2 * err
        if e2 > -ay:
            err -= ay
            x += stepx
        if e2 < ax:
            err += ax
            y += stepy
        out.append((x, y))
    return out


def bits_python(x0, y0, x1, y1, cut, mark, W, H):
    """(cleared (H, W) bool, marked (H, W) bool) by walk_cells, one ray at a time."""
    clear = np.zeros((H, W), bool)
    marked = np.zeros((H, W), bool)
    for i in range(len(x0)):
        cells = walk_cells(x0[i], y0[i], x1[i], y1[i])
        for cx, cy in (cells if cut[i] else cells[:-1]):
            if 0 <= cx < W and 0 <= cy < H:
                clear[cy, cx] = True
        cx, cy = cells[-1]
        if mark[i] and not cut[i] and 0 <= cx < W and 0 <= cy < H:
            marked[cy, cx] = True
    return clear, marked


# ---- the walk, vectorised over rays ----------------------------------------------------------------------
def bits_vector(x0, y0, x1, y1, cut, mark, W, H):
    """bits_python with one numpy step per Bresenham step over the rays still under way."""
    clear = np.zeros(H * W, bool)
    marked = np.zeros(H * W, bool)
    x0, y0, x1, y1 = (np.asarray(v, np.int64) for v in (x0, y0, x1, y1))
    cut, mark = np.asarray(cut, bool), np.asarray(mark, bool)

    def put(plane, cx, cy):
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        plane[cy[ok] * W + cx[ok]] = True

    put(clear, x1[cut], y1[cut])
    m = mark & ~cut
    put(marked, x1[m], y1[m])
    ax, ay = np.abs(x1 - x0), np.abs(y1 - y0)
    stepx, stepy = np.sign(x1 - x0), np.sign(y1 - y0)
    err = ax - ay
    x, y = x0.copy(), y0.copy()
    live = (x != x1) | (y != y1)
    x, y, x1, y1, ax, ay, stepx, stepy, err = (v[live] for v in (x, y, x1, y1, ax, ay, stepx, stepy, err))
    while len(x):
        put(clear, x, y)  # not the end cell: the ray is still under way
        e2 = 2 * err
        mx, my = e2 > -ay, e2 < ax
        err = err - np.where(mx, ay, 0) + np.where(my, ax, 0)
        x = x + np.where(mx, stepx, 0)
        y = y + np.where(my, stepy, 0)
        live = (x != x1) | (y != y1)
        if not live.all():
            x, y, x1, y1, ax, ay, stepx, stepy, err = (v[live] for v in (x, y, x1, y1, ax, ay, stepx, stepy, err))
    return clear.reshape(H, W), marked.reshape(H, W)


def compose(clear, marked, prev=None):
    """int8 (H, W): 100 where marked, 0 where cleared and not marked, else prev (or -1)."""
    out = np.full(clear.shape, -1, np.int8) if prev is None else np.array(prev, np.int8).reshape(clear.shape).copy()
    out[clear] = 0
    out[marked] = 100
    return out


def count_cells(grid):
    return (int((grid == 0).sum()), int((grid == 100).sum()), int((grid == -1).sum()))


# ---- a group ------------------------------------------------------------------------------------------
def sensor_xy(n_scans, pose2d):
    if pose2d is None:
        return np.zeros(n_scans, F32), np.zeros(n_scans, F32)
    p = np.asarray(pose2d, F32).reshape(n_scans, 6)
    return p[:, 2].copy(), p[:, 5].copy()


def group_rays(oracle, scans, p, s, motion=None, pose2d=None, t0=None):
    """rays_of for the points of a group (plus 'x', 'y', 'slot' of every point)."""
    x, y, _, slot, idx, _ = group_points(oracle, scans, p, motion, pose2d, t0)
    sx, sy = sensor_xy(len(scans), pose2d)
    r = rays_of(x, y, sx[slot] if len(slot) else np.zeros(0, F32), sy[slot] if len(slot) else np.zeros(0, F32), s)
    r.update(x=x, y=y, slot=slot, idx=idx)
    return r


def grid_of_rays(r, s, prev=None, python=False):
    """(grid int8 (H, W), (cells 0, 100, -1), status) of rays_of's result."""
    W, H = int(s["width"]), int(s["height"])
    f = bits_python if python else bits_vector
    clear, marked = f(*live_rays(r), W, H)
    grid = compose(clear, marked, prev)
    return grid, count_cells(grid), SCAN_CELL_RANGE if bool(r["dropped"].any()) else 0


def occupancy_group(oracle, scans, p, s, motion=None, pose2d=None, t0=None, prev=None):
    """The grid of ONE group: (grid int8 (H, W), (cells 0, 100, -1), status without the truncated bit)."""
    return grid_of_rays(group_rays(oracle, scans, p, s, motion, pose2d, t0), s, prev)


# ---- nav_msgs/OccupancyGrid, CDR little endian, from the message definition ------------------------------
#   std_msgs/Header header { builtin_interfaces/Time stamp { int32 sec, uint32 nanosec }, string frame_id }
#   nav_msgs/MapMetaData info { builtin_interfaces/Time map_load_time, float32 resolution, uint32 width,
#     uint32 height, geometry_msgs/Pose origin { Point position { float64 x y z },
#     Quaternion orientation { float64 x y z w } } }
#   int8[] data
# Plain CDR: a 4-byte encapsulation header 00 01 00 00, every primitive aligned to its size counted from the
# byte after it, string = uint32 length with the NUL, the bytes, the NUL; sequence = uint32 count, elements.
class _Cdr:
    def __init__(self):
        self.b = bytearray(b"\x00\x01\x00\x00")

    def align(self, n):
        while (len(self.b) - 4) % n:
            self.b.append(0)

    def put(self, fmt, v):
        self.align(struct.calcsize(fmt))
        self.b += struct.pack("<" + fmt, v)

    def string(self, text):
        raw = text.encode()
        self.put("I", len(raw) + 1)
        self.b += raw + b"\x00"


def occupancy_msg(frame_id, sec, nanosec, resolution, width, height, origin_x, origin_y, data, offsets=None):
    """The serialised message; `offsets` (a dict) receives the layout's byte offsets."""
    c = _Cdr()
    c.put("i", sec)
    c.put("I", nanosec)
    c.string(frame_id)
    off = {}
    c.align(4)
    off["map_load_time_off"] = len(c.b)
    c.put("i", sec)
    c.put("I", nanosec)
    off["resolution_off"] = len(c.b)
    c.put("f", float(F32(resolution)))
    c.put("I", width)
    c.put("I", height)
    c.align(8)
    off["origin_off"] = len(c.b)
    for v in (float(F32(origin_x)), float(F32(origin_y)), 0.0, 0.0, 0.0, 0.0, 1.0):
        c.put("d", v)
    off["data_len_off"] = len(c.b)
    data = np.ascontiguousarray(data, np.int8).reshape(-1)
    assert len(data) == width * height
    c.put("I", len(data))
    off["data_off"] = len(c.b)
    c.b += data.tobytes()
    off["total_len"] = len(c.b)
    if offsets is not None:
        offsets.update(off)
    return bytes(c.b)
