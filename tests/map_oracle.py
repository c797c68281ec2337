"""Restatement of E14 (include/rplgpu_msg.h): the persistent hit / miss count map of rplgpu_map_update_dev, the
cell rule of rplgpu_map_grid_dev and the pose composition of rplgpu_apply_match_dev.  TEST INFRASTRUCTURE —
imported by tests/ only.

Rays: tests/occ_oracle.group_rays, every ray undeduplicated (here equal rays each count).  Counts come from two
writers: a per-ray pure-Python walk (occ_oracle.walk_cells) into a dict, and the vectorised Bresenham with
np.add.at.  The rule runs in Python integers (no width to overflow), the apply step in numpy float32 with every
product rounded before the sum."""
from __future__ import annotations

import numpy as np

from tests import match_oracle as mo
from tests import occ_oracle as oo

F32 = np.float32
DEFAULT_RULE = dict(min_observations=2, occupied_percent=10, mode=0)
E11_RULE = dict(min_observations=1, occupied_percent=0, mode=0)  # "marks beat clears"


def rule(**kw) -> dict:
    d = dict(DEFAULT_RULE)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return d


def rule_valid(r: dict) -> bool:
    return r["min_observations"] >= 1 and 0 <= r["occupied_percent"] <= 100 and r["mode"] in (0, 1)


# ---- rays -----------------------------------------------------------------------------------------------------
def all_rays(r):
    """(x0, y0, x1, y1, cut, mark) of every ray that is walked, in sample order, duplicates kept."""
    m = r["ray"] & ~r["dropped"]
    return r["x0"][m], r["y0"][m], r["x1"][m], r["y1"][m], r["cut"][m], (r["mark"] & ~r["cut"])[m]


# ---- writer (a): per ray, pure Python, into a dict ----------------------------------------------------------------
def counts_python(x0, y0, x1, y1, cut, mark, W, H):
    """(H, W, 2) int64 (misses, hits) by occ_oracle.walk_cells, one ray at a time."""
    d = {}
    for i in range(len(x0)):
        cells = oo.walk_cells(x0[i], y0[i], x1[i], y1[i])
        for c in (cells if cut[i] else cells[:-1]):
            e = d.setdefault(c, [0, 0])
            e[0] += 1
        if mark[i] and not cut[i]:
            e = d.setdefault(cells[-1], [0, 0])
            e[1] += 1
    out = np.zeros((H, W, 2), np.int64)
    for (cx, cy), (m, h) in d.items():
        if 0 <= cx < W and 0 <= cy < H:
            out[cy, cx] = (m, h)
    return out


# ---- writer (b): vectorised over rays, np.add.at --------------------------------------------------------------------
def counts_vector(x0, y0, x1, y1, cut, mark, W, H):
    """The same counts with one numpy step per Bresenham step over the rays still under way."""
    miss = np.zeros(H * W, np.int64)
    hit = np.zeros(H * W, np.int64)
    x0, y0, x1, y1 = (np.asarray(v, np.int64) for v in (x0, y0, x1, y1))
    cut, mark = np.asarray(cut, bool), np.asarray(mark, bool)

    def put(plane, cx, cy):
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        np.add.at(plane, cy[ok] * W + cx[ok], 1)

    put(miss, x1[cut], y1[cut])
    m = mark & ~cut
    put(hit, x1[m], y1[m])
    ax, ay = np.abs(x1 - x0), np.abs(y1 - y0)
    stepx, stepy = np.sign(x1 - x0), np.sign(y1 - y0)
    err = ax - ay
    x, y = x0.copy(), y0.copy()
    live = (x != x1) | (y != y1)
    x, y, x1, y1, ax, ay, stepx, stepy, err = (v[live] for v in (x, y, x1, y1, ax, ay, stepx, stepy, err))
    while len(x):
        put(miss, x, y)  # not the end cell: the ray is still under way
        e2 = 2 * err
        mx, my = e2 > -ay, e2 < ax
        err = err - np.where(mx, ay, 0) + np.where(my, ax, 0)
        x = x + np.where(mx, stepx, 0)
        y = y + np.where(my, stepy, 0)
        live = (x != x1) | (y != y1)
        if not live.all():
            x, y, x1, y1, ax, ay, stepx, stepy, err = (v[live] for v in (x, y, x1, y1, ax, ay, stepx, stepy, err))
    return np.stack([miss, hit], 1).reshape(H, W, 2)


def counts_of_rays(r, s, python=False):
    """((H, W, 2) int64 counts, status without the truncated bit) of rays_of's result."""
    W, H = int(s["width"]), int(s["height"])
    f = counts_python if python else counts_vector
    return f(*all_rays(r), W, H), oo.SCAN_CELL_RANGE if bool(r["dropped"].any()) else 0


def map_group(oracle, scans, p, s, motion=None, pose2d=None, t0=None, python=False):
    """The counts ONE group of scans adds to a map: ((H, W, 2) int64, status without the truncated bit)."""
    return counts_of_rays(oo.group_rays(oracle, scans, p, s, motion, pose2d, t0), s, python)


def as_words(counts) -> np.ndarray:
    """The map as it lies in memory: (H, W, 2) uint32; the oracle's sums must fit."""
    counts = np.asarray(counts, np.int64)
    assert counts.min(initial=0) >= 0 and counts.max(initial=0) < 2 ** 32
    return counts.astype(np.uint32)


def run_lengths(r, slot):
    """Lengths of the runs of equal consecutive rays of ONE scan of a group, in sample order: two samples are in
    one run when their sample indices are consecutive and both have the same walked ray."""
    m = np.flatnonzero((r["slot"] == slot) & r["ray"] & ~r["dropped"])
    if len(m) == 0:
        return []
    word = np.stack([r["x1"][m], r["y1"][m], r["cut"][m].astype(np.int64), (r["mark"] & ~r["cut"])[m].astype(np.int64)], 1)
    idx = r["idx"][m]
    same = (np.diff(idx) == 1) & (word[1:] == word[:-1]).all(1)
    out, n = [], 1
    for sm in same:
        if sm:
            n += 1
        else:
            out.append(n)
            n = 1
    out.append(n)
    return out


# ---- the cell rule, Python integers --------------------------------------------------------------------------------
def rule_cell(h: int, m: int, r: dict, prev: int = -1) -> int:
    h, m = int(h), int(m)
    n = h + m
    if n < r["min_observations"]:
        return int(prev)
    if r["mode"] == 0:
        return 100 if (h > 0 and 100 * h >= r["occupied_percent"] * n) else 0
    return (200 * h + n) // (2 * n)


def grid_of_counts(counts, r, prev=None):
    """(grid int8 (H, W), (cells -1, 0, 100, other)) — the rule once per distinct (misses, hits, prev) triple."""
    counts = np.asarray(counts).astype(np.int64)
    H, W, _ = counts.shape
    pv = np.full((H, W), -1, np.int64) if prev is None else np.asarray(prev, np.int8).reshape(H, W).astype(np.int64)
    tri = np.stack([counts[..., 0].ravel(), counts[..., 1].ravel(), pv.ravel()], 1)
    uniq, inv = np.unique(tri, axis=0, return_inverse=True)
    vals = np.array([rule_cell(int(h), int(m), r, int(p)) for m, h, p in uniq], np.int64)
    assert ((vals >= -128) & (vals <= 127)).all()
    grid = vals[inv.ravel()].reshape(H, W).astype(np.int8)
    return grid, count_cells(grid)


def count_cells(grid):
    g = np.asarray(grid, np.int8)
    a, b, c = int((g == -1).sum()), int((g == 0).sum()), int((g == 100).sum())
    return a, b, c, int(g.size) - a - b - c


# ---- E13's result applied to the poses -----------------------------------------------------------------------------
def apply_match(best, s, pivot, pose_in, B, group, flags=0):
    """(pose_out (B, 6) float32, pivot_out (G, 2) float32).  best: (G, 8) words (any integer dtype; k, j, i are
    read as int32); s: a match_oracle spec; pivot: (G, 2) or None; pose_in: (B, 6) or None (identity)."""
    K = int(s["rot_steps"])
    rot = mo.rotations(s)
    res = F32(s["resolution"])
    group = min(group, B)
    G = (B + group - 1) // group
    words = (np.asarray(best, np.int64).reshape(G, 8) & 0xFFFFFFFF).astype(np.uint32)
    kji = words[:, 1:4].view(np.int32).reshape(G, 3)
    pv = np.zeros((G, 2), F32) if pivot is None else np.asarray(pivot, F32).reshape(G, 2)
    pin = np.tile(np.array([1, 0, 0, 0, 1, 0], F32), (B, 1)) if pose_in is None else np.asarray(pose_in, F32).reshape(B, 6)
    out = pin.copy()
    pout = pv.copy()
    for g in range(G):
        k, j, i = (int(v) for v in kji[g])
        keep = k < -K or k > K
        if (flags & 1) and (int(words[g, 6]) != 1 or int(words[g, 0]) == 0):
            keep = True
        if keep:
            continue
        c, sn = F32(rot[k + K, 0]), F32(rot[k + K, 1])
        px, py = F32(pv[g, 0]), F32(pv[g, 1])
        dx, dy = F32(F32(i) * res), F32(F32(j) * res)
        pout[g] = (F32(px + dx), F32(py + dy))
        sl = slice(g * group, min(B, (g + 1) * group))
        r00, r01, tx, r10, r11, ty = (pin[sl, q].astype(F32) for q in range(6))
        with np.errstate(all="ignore"):
            out[sl, 0] = ((c * r00).astype(F32) - (sn * r10).astype(F32)).astype(F32)
            out[sl, 1] = ((c * r01).astype(F32) - (sn * r11).astype(F32)).astype(F32)
            out[sl, 3] = ((sn * r00).astype(F32) + (c * r10).astype(F32)).astype(F32)
            out[sl, 4] = ((sn * r01).astype(F32) + (c * r11).astype(F32)).astype(F32)
            qx, qy = (tx - px).astype(F32), (ty - py).astype(F32)
            out[sl, 2] = ((((c * qx).astype(F32) - (sn * qy).astype(F32)).astype(F32) + px).astype(F32) + dx).astype(F32)
            out[sl, 5] = ((((sn * qx).astype(F32) + (c * qy).astype(F32)).astype(F32) + py).astype(F32) + dy).astype(F32)
    return out, pout
