"""The E19 oracle (include/rplgpu_msg.h, the E19 block): M poses, their cell indices and eight result words of one
group, by two writers that share no step (Philox itself is tests/motion_oracle.py's, which has two writers of its own).

(a) `poses_numpy`: the free cells by `flatnonzero`, the r-th of them by a gather, Philox in numpy uint64 arrays over
    all outputs at once, the float steps in numpy float32.
(b) `poses_python`: a plain loop that walks the cells in index order and counts the free ones, handing every output
    whose r equals the count its cell; Philox in Python integers; the float steps in Python doubles rounded to float32
    after every operation (a double holds the exact sum, difference and product of two float32 and rounds a quotient
    where the second rounding to 24 bits cannot differ from the single one).

Above PYTHON_CELLS cells or PYTHON_LIMIT outputs writer (a) alone.

A spec is a dict(origin_x, origin_y, resolution, width, height, free_lo, free_hi, flags); a noise spec is
motion_oracle's dict(seed, step, first)."""
import math
import struct

import numpy as np

from tests import motion_oracle as mo

F32 = np.float32
MASK = 0xFFFFFFFF
DRAW = 3                                # the draw index E18 leaves unused
CELL_LIMIT = 1048576.0
PYTHON_CELLS = 1 << 17
PYTHON_LIMIT = 4096
DEFAULT = dict(origin_x=-25.6, origin_y=-25.6, resolution=0.05, width=1024, height=1024, free_lo=0, free_hi=0, flags=0)


def free_mask(grid, spec):
    """the cells of a flat int8 grid (only its first width * height bytes) that are free"""
    cells = spec["width"] * spec["height"]
    v = np.asarray(grid).reshape(-1)[:cells].view(np.int8).astype(np.int64)
    return (v >= spec["free_lo"]) & (v <= spec["free_hi"])


# ---- writer (a): numpy --------------------------------------------------------------------------------------------------
def blocks_numpy(noise, g, M):
    """-> the four Philox words of outputs 0 .. M - 1 of group g as uint64 arrays"""
    seed, step = int(noise["seed"]), int(noise["step"])
    j = (np.arange(M, dtype=np.uint64) + np.uint64(int(noise["first"]))) & np.uint64(MASK)
    full = np.full(M, 1, np.uint64)
    return mo.philox_numpy(j, full * np.uint64((g << 2) | DRAW), full * np.uint64(step & MASK),
                           full * np.uint64(step >> 32), seed & MASK, seed >> 32)


def ranks_numpy(noise, g, M, F):
    return (blocks_numpy(noise, g, M)[0] * np.uint64(F)) >> np.uint64(32)


def poses_numpy(grid, spec, headings, M, noise, g=0):
    """-> (words (M, 4) uint32, cells (M,) uint32, F, none)"""
    width, cells = spec["width"], spec["width"] * spec["height"]
    free = np.flatnonzero(free_mask(grid, spec))
    none = len(free) == 0
    if none:
        free = np.arange(cells)
    F = len(free)
    p0, p1, p2, p3 = blocks_numpy(noise, g, M)
    cell = free[((p0 * np.uint64(F)) >> np.uint64(32)).astype(np.int64)]
    head = np.ascontiguousarray(headings, F32).reshape(-1, 2).view(np.uint32)
    k = ((p1 * np.uint64(len(head))) >> np.uint64(32)).astype(np.int64)
    cx, cy = cell % width, cell // width
    ox, oy, res = F32(spec["origin_x"]), F32(spec["origin_y"]), F32(spec["resolution"])
    if spec["flags"] & 1:
        fx = fy = np.full(M, 0.5, F32)
    else:
        fx = ((p2 >> np.uint64(24)).astype(F32) + F32(0.5)) * F32(1.0 / 256.0)
        fy = ((p3 >> np.uint64(24)).astype(F32) + F32(0.5)) * F32(1.0 / 256.0)
    x = ox + (cx.astype(F32) + fx) * res
    y = oy + (cy.astype(F32) + fy) * res
    words = np.zeros((M, 4), np.uint32)
    words[:, :2] = head[k]
    words[:, 2] = x.astype(F32).view(np.uint32)
    words[:, 3] = y.astype(F32).view(np.uint32)
    return words, cell.astype(np.uint32), F, none


def off_cell_numpy(words, cell, spec):
    """-> per output, whether the E11 CELL of (x, y) does not exist or is not the chosen cell"""
    ox, oy, res = F32(spec["origin_x"]), F32(spec["origin_y"]), F32(spec["resolution"])
    x, y = words[:, 2].copy().view(F32), words[:, 3].copy().view(F32)
    with np.errstate(all="ignore"):
        fu, fv = np.floor((x - ox) / res), np.floor((y - oy) / res)
        has = (np.abs(fu) < CELL_LIMIT) & (np.abs(fv) < CELL_LIMIT)
        bx = np.where(has, fu, -1).astype(np.int64)
        by = np.where(has, fv, -1).astype(np.int64)
    c = cell.astype(np.int64)
    return ~(has & (bx == c % spec["width"]) & (by == c // spec["width"]))


# ---- writer (b): a loop over the cells, Python integers and doubles ----------------------------------------------------
def _r(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def block_python(noise, g, j):
    seed, step = int(noise["seed"]), int(noise["step"])
    ctr = ((int(noise["first"]) + j) & MASK, (g << 2) | DRAW, step & MASK, step >> 32)
    return mo.philox_python(ctr, (seed & MASK, seed >> 32))


def _cell_python(x, y, ox, oy, res):
    fu, fv = math.floor(_r(_r(x - ox) / res)), math.floor(_r(_r(y - oy) / res))
    if not (abs(fu) < CELL_LIMIT and abs(fv) < CELL_LIMIT):
        return None
    return fu, fv


def poses_python(grid, spec, headings, M, noise, g=0):
    """-> (words (M, 4) uint32, cells (M,) uint32, F, none, off-cell outputs)"""
    width, cells = spec["width"], spec["width"] * spec["height"]
    lo, hi = spec["free_lo"], spec["free_hi"]
    raw = bytes(np.asarray(grid).reshape(-1)[:cells].view(np.uint8))
    is_free = [lo <= (b - 256 if b > 127 else b) <= hi for b in raw]
    F = sum(is_free)
    none = F == 0
    if none:
        F, is_free = cells, [True] * cells
    blocks = [block_python(noise, g, j) for j in range(M)]
    waiting = {}
    for j, p in enumerate(blocks):
        waiting.setdefault((p[0] * F) >> 32, []).append(j)
    cell = [None] * M
    count = 0
    for i in range(cells):                      # the walk: `count` free cells lie in front of cell i
        if is_free[i]:
            for j in waiting.get(count, ()):
                cell[j] = i
            count += 1
    head = np.ascontiguousarray(headings, F32).reshape(-1, 2).view(np.uint32)
    ox, oy, res = (float(F32(spec[k])) for k in ("origin_x", "origin_y", "resolution"))
    words = np.zeros((M, 4), np.uint32)
    off = 0
    for j, p in enumerate(blocks):
        k = (p[1] * len(head)) >> 32
        cy, cx = divmod(cell[j], width)
        if spec["flags"] & 1:
            fx = fy = 0.5
        else:
            fx, fy = _r(((p[2] >> 24) + 0.5) * (1.0 / 256.0)), _r(((p[3] >> 24) + 0.5) * (1.0 / 256.0))
        x = _r(ox + _r(_r(cx + fx) * res))
        y = _r(oy + _r(_r(cy + fy) * res))
        words[j] = [head[k, 0], head[k, 1], struct.unpack("<I", struct.pack("<f", x))[0],
                    struct.unpack("<I", struct.pack("<f", y))[0]]
        off += _cell_python(x, y, ox, oy, res) != (cx, cy)
    return words, np.array(cell, np.uint32), F, none, off


# ---- the result words ---------------------------------------------------------------------------------------------------
def seed(grid, spec, headings, M, noise=mo.DEFAULT, g=0, writer=None):
    """-> (pose words (M, 4) uint32, cell indices (M,) uint32, result (8,) uint32) of group g"""
    cells = spec["width"] * spec["height"]
    if writer is None:
        writer = poses_python if cells <= PYTHON_CELLS and M <= PYTHON_LIMIT else poses_numpy
    out = writer(grid, spec, headings, M, noise, g)
    words, cell, F, none = out[:4]
    off = int(out[4]) if len(out) > 4 else int(off_cell_numpy(words, cell, spec).sum())
    res = np.array([F, off, int(cell.min()), int(cell.max()), 0, 0, 0, (1 if none else 0) | (2 if off else 0)],
                   np.uint32)
    return words, cell, res


def headings(H):
    """the table of rplgpu_seed_headings through Python's math (the same libm)"""
    out = np.zeros((H, 2), F32)
    for k in range(H):
        a = 2.0 * math.pi * k / H
        out[k] = (1.0, 0.0) if k == 0 else (math.cos(a), math.sin(a))
    return out
