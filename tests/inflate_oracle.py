"""E12 restated in numpy from the rules in include/rplgpu_msg.h (rplgpu_inflate_grids_dev), twice: the
squared distance to the nearest lethal cell by brute force (every offset of the disc, the shifted lethal
mask) and by an exact integer separable transform (row distances, then a column minimum); the two writers
must agree (tests/test_inflate_cpu.py).  Plus the cost table by the header's formula.
TEST INFRASTRUCTURE — imported by tests/ only."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
MAX_CELLS = 64
NONE = np.int64(1 << 40)  # D2 of a cell without a lethal cell in reach


def reach(inflation_radius, resolution):
    """Rc: every float widened to double first."""
    return int(math.ceil(float(F32(inflation_radius)) / float(F32(resolution))))


def spec_valid(inscribed, inflation, scaling, inflate_unknown, resolution):
    v = [float(F32(x)) for x in (inscribed, inflation, scaling, resolution)]
    if not all(math.isfinite(x) for x in v):
        return False
    ins, inf, sc, res = v
    if ins < 0 or inf < 0 or sc < 0 or not res > 0 or inf < ins or inflate_unknown > 1:
        return False
    return math.ceil(inf / res) <= MAX_CELLS


def table_values(inscribed, inflation, scaling, resolution):
    """-> (table uint8 (Rc * Rc + 1,), raw float64: 98 exp(..) before truncation, NaN where the rule does
    not use it)."""
    rc = reach(inflation, resolution)
    res, ins, sc = float(F32(resolution)), float(F32(inscribed)), float(F32(scaling))
    k = np.arange(rc * rc + 1, dtype=np.float64)
    d = np.sqrt(k) * res
    raw = 98.0 * np.exp(-sc * (d - ins))
    inside = d <= ins
    table = np.where(inside, 99, np.trunc(np.where(inside, 0.0, raw))).astype(np.uint8)
    table[0] = 100
    raw = np.where(inside, np.nan, raw)
    raw[0] = np.nan
    return table, raw


def lethal(grid):
    return np.asarray(grid, np.int8) >= 100


def d2_brute(grid, rc):
    """For every offset of the disc, in any order: a cell whose neighbour at that offset is lethal is at
    most that far from a lethal cell."""
    L = lethal(grid)
    H, W = L.shape
    out = np.full((H, W), NONE, np.int64)
    for dy in range(-rc, rc + 1):
        if abs(dy) >= H:
            continue
        for dx in range(-rc, rc + 1):
            k = dx * dx + dy * dy
            if k > rc * rc or abs(dx) >= W:
                continue
            # cell (y, x) looks at (y + dy, x + dx)
            ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
            xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
            view = out[yd, xd]
            np.minimum(view, np.where(L[ys, xs], k, NONE), out=view)
    return out


def d2_separable(grid, rc):
    """Row pass: hx = distance to the nearest lethal cell of the same row; column pass: min over |dy| <= rc
    of hx^2 + dy^2, rows outside the grid hold nothing.  All integers."""
    L = lethal(grid)
    H, W = L.shape
    big = np.int64(1 << 20)
    x = np.arange(W, dtype=np.int64)
    left = np.maximum.accumulate(np.where(L, x, -big), axis=1)              # nearest lethal column <= x
    right = np.minimum.accumulate(np.where(L, x, big)[:, ::-1], axis=1)[:, ::-1]  # ... >= x
    hx = np.minimum(x - left, right - x)
    hx2 = np.where(hx <= rc, hx * hx, NONE)
    out = np.full((H, W), NONE, np.int64)
    for dy in range(-rc, rc + 1):
        if abs(dy) >= H:
            continue
        ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
        view = out[yd]
        np.minimum(view, hx2[ys] + dy * dy, out=view)
    return np.where(out <= rc * rc, out, NONE)


def combine(grid, d2, table, rc, inflate_unknown):
    """The per-cell rule -> (result int8, (cells == 100, == 99, 1 .. 98, == -1))."""
    v = np.asarray(grid, np.int8).astype(np.int64)
    table = np.asarray(table, np.uint8)
    assert len(table) == rc * rc + 1
    hit = d2 <= rc * rc
    cost = np.where(hit, table[np.where(hit, d2, 0)], 0).astype(np.int64)
    out = np.where(v >= 100, 100, np.where(v >= 0, np.maximum(v, cost),
                                           np.where((cost > 0) if inflate_unknown else (cost >= 99), cost, -1)))
    out = out.astype(np.int8)
    cells = (int((out == 100).sum()), int((out == 99).sum()), int(((out >= 1) & (out <= 98)).sum()),
             int((out == -1).sum()))
    return out, cells


def inflate(grid, table, rc, inflate_unknown, writer=d2_separable):
    return combine(grid, writer(grid, rc), table, rc, inflate_unknown)
