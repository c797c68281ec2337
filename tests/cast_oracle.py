"""E22 (include/rplgpu_msg.h, rplgpu_cast_ranges_dev) in numpy, two writers that share no step:

  writer 1  `cast_rays` / `weights_rays`: a ray at a time in Python scalars, cell by cell by the rule's five tests;
  writer 2  `cast_lockstep` / `weights_table`: every ray of a case at once, one numpy pass per visit number over the
            rays still walking, the terms by one vectorised table look-up.

Both take float32 arrays and round every float32 operation once (numpy does not fuse).  `cast_group` puts a group's
range words, weights, E15's result words and the eight cast counts together under either writer."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32 = np.float32
HIT, UNKNOWN, LEFT, NO_STOP = 0, 1, 2, 3
DROPPED = 0xFFFFFFFF
CELL_LIMIT = 1048576.0
MAX_DIM, MAX_STEPS, MAX_BEAMS, MAX_HALF = 4096, 8192, 16384, 4096
DEFAULT = dict(origin_x=-25.6, origin_y=-25.6, resolution=0.05, width=1024, height=1024, max_steps=240, hit_lo=100,
               unknown_stops=1, table_half=40)


def spec(**kw) -> dict:
    s = dict(DEFAULT)
    for k, v in kw.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return s


def spec_valid(s: dict) -> bool:
    f = [float(F32(s[k])) for k in ("origin_x", "origin_y", "resolution")]
    return (all(math.isfinite(v) for v in f) and f[2] > 0 and 1 <= s["width"] <= MAX_DIM
            and 1 <= s["height"] <= MAX_DIM and 1 <= s["max_steps"] <= MAX_STEPS and 1 <= s["hit_lo"] <= 127
            and s["unknown_stops"] in (0, 1) and 0 <= s["table_half"] <= MAX_HALF)


# ---- writer 1: a ray at a time -------------------------------------------------------------------------------------------
def _cell(x, y, s):
    with np.errstate(all="ignore"):
        fu = np.floor((F32(x) - F32(s["origin_x"])) / F32(s["resolution"]))
        fv = np.floor((F32(y) - F32(s["origin_y"])) / F32(s["resolution"]))
    if not (abs(fu) < CELL_LIMIT and abs(fv) < CELL_LIMIT):
        return None
    return int(fu), int(fv)


def _fused(a, b, c) -> np.float32:
    """a * b + c rounded ONCE (what a fused multiply-add gives; finite arguments): exact in fractions, then rounded"""
    return F32(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def ray(s, pose, beam, grid, fused=False):
    """One ray by the rule -> (range word, n at the stop); (DROPPED, 0) for a ray without a start or end cell.
    fused: NOT the rule — the composition as an FMA would round it, for the regime check of the case that tells the
    two apart."""
    c, sn, tx, ty = (F32(v) for v in pose)
    cb, sb = F32(beam[0]), F32(beam[1])
    with np.errstate(all="ignore"):
        dc = F32(c * cb) - F32(sn * sb)
        ds = F32(sn * cb) + F32(c * sb)
        if fused:
            dc, ds = _fused(c, cb, -F32(sn * sb)), _fused(sn, cb, F32(c * sb))
        rm = F32(s["max_steps"]) * F32(s["resolution"])
        ex = tx + F32(dc * rm)
        ey = ty + F32(ds * rm)
    a, b = _cell(tx, ty, s), _cell(ex, ey, s)
    if a is None or b is None:
        return DROPPED, 0
    (x0, y0), (x1, y1) = a, b
    ax, ay = abs(x1 - x0), abs(y1 - y0)
    stepx, stepy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
    err, x, y, n = ax - ay, x0, y0, 0
    W, H, N = s["width"], s["height"], s["max_steps"]
    while True:
        if not (0 <= x < W and 0 <= y < H):
            kind = LEFT
            break
        v = int(grid[y, x])
        if v >= s["hit_lo"]:
            kind = HIT
            break
        if v < 0 and s["unknown_stops"]:
            kind = UNKNOWN
            break
        if (x == x1 and y == y1) or n == N:
            kind = NO_STOP
            break
        e2 = 2 * err
        if e2 > -ay:
            err -= ay
            x += stepx
        if e2 < ax:
            err += ax
            y += stepy
        n += 1
    return ((x - x0) ** 2 + (y - y0) ** 2) | (kind << 28), n


def cast_rays(s, poses, beams, grid):
    P, A = len(poses), len(beams)
    words, steps = np.zeros((P, A), np.uint32), np.zeros((P, A), np.int64)
    for q in range(P):
        for a in range(A):
            words[q, a], steps[q, a] = ray(s, poses[q], beams[a], grid)
    return words, steps


def term(s, word, z, table) -> int:
    """The table term of one range word against the measured range z (not NaN, the ray not dropped)."""
    K = s["table_half"]
    with np.errstate(all="ignore"):
        mz = F32(z) / F32(s["resolution"])
        de = F32(np.inf) if (int(word) >> 28) == NO_STOP else np.sqrt(F32(int(word) & 0x0FFFFFFF))
        if mz == np.inf and de == np.inf:
            return int(table[2 * K + 1])
        d = float(np.floor(mz - de))
    return int(table[K + int(max(-K, min(K, d)))])


def weights_rays(s, words, z, table):
    out = np.zeros(len(words), np.uint32)
    for q in range(len(words)):
        out[q] = sum(term(s, words[q, a], z[a], table) for a in range(words.shape[1])
                     if not np.isnan(z[a]) and int(words[q, a]) != DROPPED)
    return out


# ---- writer 2: all rays in lock step --------------------------------------------------------------------------------------
def cast_lockstep(s, poses, beams, grid):
    poses, beams = np.asarray(poses, F32), np.asarray(beams, F32)
    P, A = len(poses), len(beams)
    ox, oy, res = F32(s["origin_x"]), F32(s["origin_y"]), F32(s["resolution"])
    W, H, N = s["width"], s["height"], s["max_steps"]
    with np.errstate(all="ignore"):
        c, sn, tx, ty = (np.repeat(poses[:, k], A) for k in range(4))
        cb, sb = np.tile(beams[:, 0], P), np.tile(beams[:, 1], P)
        dc, ds = c * cb - sn * sb, sn * cb + c * sb
        rm = F32(N) * res
        ex, ey = tx + dc * rm, ty + ds * rm
        f = [np.floor((v - o) / res) for v, o in ((tx, ox), (ty, oy), (ex, ox), (ey, oy))]
        ok = np.ones(P * A, bool)
        for v in f:
            ok &= np.abs(v) < CELL_LIMIT
    x0, y0, x1, y1 = (np.where(ok, v, 0).astype(np.int64) for v in f)
    ax, ay = np.abs(x1 - x0), np.abs(y1 - y0)
    sx, sy = np.sign(x1 - x0), np.sign(y1 - y0)
    err, x, y = ax - ay, x0.copy(), y0.copy()
    kind = np.full(P * A, -1, np.int64)
    steps = np.zeros(P * A, np.int64)
    live = ok.copy()
    for n in range(N + 1):
        i = np.flatnonzero(live)
        if not i.size:
            break
        xi, yi = x[i], y[i]
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        v = np.zeros(i.size, np.int64)
        v[inside] = grid[yi[inside], xi[inside]]
        k = np.full(i.size, -1, np.int64)
        k[((xi == x1[i]) & (yi == y1[i])) | (n == N)] = NO_STOP          # the weakest test first, overwritten below
        if s["unknown_stops"]:
            k[v < 0] = UNKNOWN
        k[v >= s["hit_lo"]] = HIT
        k[~inside] = LEFT
        stop = k >= 0
        kind[i[stop]], steps[i[stop]] = k[stop], n
        live[i[stop]] = False
        j = i[~stop]
        e2 = 2 * err[j]
        mx, my = e2 > -ay[j], e2 < ax[j]
        err[j] += np.where(my, ax[j], 0) - np.where(mx, ay[j], 0)
        x[j] += np.where(mx, sx[j], 0)
        y[j] += np.where(my, sy[j], 0)
    assert not live.any()
    d2 = (x - x0) ** 2 + (y - y0) ** 2
    words = np.where(ok, d2 | (kind << 28), DROPPED).astype(np.uint32)
    return words.reshape(P, A), np.where(ok, steps, 0).reshape(P, A)


def weights_table(s, words, z, table):
    K = s["table_half"]
    words, z, table = np.asarray(words, np.uint32), np.asarray(z, F32), np.asarray(table, np.uint8)
    with np.errstate(all="ignore"):
        mz = (z / F32(s["resolution"]))[None, :]
        de = np.where((words >> 28) == NO_STOP, F32(np.inf), np.sqrt((words & 0x0FFFFFFF).astype(F32))).astype(F32)
        both = np.isposinf(mz) & np.isposinf(de)
        skip = np.isnan(z)[None, :] | (words == DROPPED)
        d = np.floor(np.where(both | skip, F32(0), mz - de))
    idx = np.where(both, 2 * K + 1, K + np.clip(d, -K, K).astype(np.int64))
    t = np.where(skip, 0, table[idx].astype(np.int64))
    return t.sum(axis=1).astype(np.uint32)


# ---- the words of a group ---------------------------------------------------------------------------------------------------
def result_of(weights, beams_in) -> np.ndarray:
    """E15's RESULT rule on a group's weights, word 4 = beams_in."""
    w = np.asarray(weights, np.uint32)
    top, total = int(w.max()), int(w.astype(np.uint64).sum())
    return np.array([top, int(np.flatnonzero(w == top)[0]), int((w == top).sum()), int((w == 0).sum()), beams_in,
                     int(w[0]), total & 0xFFFFFFFF, total >> 32], np.uint32)


def counts_of(words, steps) -> np.ndarray:
    w = np.asarray(words, np.uint32).reshape(-1)
    live = w != DROPPED
    kinds = [int((live & ((w >> 28) == k)).sum()) for k in range(4)]
    hits = w[live & ((w >> 28) == HIT)] & 0x0FFFFFFF
    total = int(np.asarray(steps).sum())
    return np.array(kinds + [int((~live).sum()), int(hits.max()) if hits.size else 0, total & 0xFFFFFFFF,
                             total >> 32], np.uint32)


def beam_ranges(measured, first, step, A):
    return np.asarray(measured, F32)[first + step * np.arange(A)]


def cast_group(s, poses, beams, grid, measured=None, first=0, step=1, table=None, writer=2) -> dict:
    """One group -> dict(ranges (P, A), weights (P,) or None, result (8,) or None, cast (8,), steps (P, A))."""
    cast, weigh = (cast_rays, weights_rays) if writer == 1 else (cast_lockstep, weights_table)
    words, steps = cast(s, np.asarray(poses, F32), np.asarray(beams, F32), np.asarray(grid, np.int8))
    out = dict(ranges=words, steps=steps, cast=counts_of(words, steps), weights=None, result=None)
    if measured is not None:
        z = beam_ranges(measured, first, step, len(beams))
        out["weights"] = weigh(s, words, z, np.asarray(table, np.uint8))
        out["result"] = result_of(out["weights"], int((~np.isnan(z)).sum()))
    return out


def range_m(word, resolution) -> float:
    if int(word) == DROPPED:
        return math.nan
    if (int(word) >> 28) == NO_STOP:
        return math.inf
    return math.sqrt(int(word) & 0x0FFFFFFF) * float(F32(resolution))
