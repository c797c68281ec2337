"""Restatement of E24, the wide-window scan matcher (include/rplgpu_msg.h, rplgpu_match_wide_dev), in numpy, twice:
(1) exhaustive — E13's score volume over the whole wide window, then the tie rule as a plain lexicographic sort
(tests/match_oracle.best_of); (2) bound and refine — the pooled field, the bounds, the seeds, the list, E13's scores
of the listed blocks only.  The two writers must agree on every case's best words (tests/test_wide_cpu.py); writer 2
alone gives P, U, the work words and the unproven results.  TEST INFRASTRUCTURE — imported by tests/ only.

Points, rotations, the rotated cell and the tie rule are tests/match_oracle.py's."""
from __future__ import annotations

import numpy as np

from tests import match_oracle as mo

F32 = np.float32
S = 8                   # RPLGPU_WIDE_MATCH_BLOCK
MAX_SHIFT = 256
MAX_BLOCKS = 65536
UNPROVEN = 0x1
DEFAULT = dict(mo.DEFAULT, shift_x=64, shift_y=64, max_blocks=1024)


def spec(**kw) -> dict:
    d = dict(DEFAULT)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return d


def spec_valid(s: dict) -> bool:
    """E13's check with the wide limits, and the cap."""
    if s["shift_x"] > MAX_SHIFT or s["shift_y"] > MAX_SHIFT:
        return False
    if not 1 <= s["max_blocks"] <= MAX_BLOCKS:
        return False
    return mo.spec_valid(dict(s, shift_x=0, shift_y=0))


def scan_match_spec(s: dict) -> dict:
    """The E13 spec of the same grid and rotations (the shifts only where E13 takes them)."""
    return {k: s[k] for k in mo.DEFAULT}


def blocks_shape(s: dict):
    return 2 * int(s["rot_steps"]) + 1, (2 * int(s["shift_y"]) + S) // S, (2 * int(s["shift_x"]) + S) // S


def blocks_size(s: dict) -> int:
    a, b, c = blocks_shape(s)
    return a * b * c


def scratch_words(s: dict, G: int) -> int:
    return G * (272 + 65 * int(s["max_blocks"]))


# ---- the pooled field ------------------------------------------------------------------------------------------------
def pool(field) -> np.ndarray:
    """P as (H + 7, W + 7) int8: P(x, y) at [y + 7, x + 7], the maximum of max(byte, 0) over [x, x + 8) x [y, y + 8),
    0 outside the grid; the definition, cell by cell over the 64 offsets."""
    f = np.maximum(np.asarray(field, np.int8), 0)
    H, W = f.shape
    big = np.zeros((H + 2 * (S - 1), W + 2 * (S - 1)), np.int8)  # F(x, y) at [y + 7, x + 7]
    big[S - 1:S - 1 + H, S - 1:S - 1 + W] = f
    out = np.zeros((H + S - 1, W + S - 1), np.int8)
    for b in range(S):
        for a in range(S):
            np.maximum(out, big[b:b + H + S - 1, a:a + W + S - 1], out=out)
    return out


# ---- what both writers share: the rotated cells, counted -------------------------------------------------------------
def _pad(s):
    return 2 * int(s["shift_y"]) + S, 2 * int(s["shift_x"]) + S


def _padded(values, s):
    """An (H, W) array of bytes surrounded by zeros: value (x, y) at [y + pad_y, x + pad_x]; every look-up of every
    kept cell stays inside."""
    H, W = values.shape
    py, px = _pad(s)
    big = np.zeros((H + 2 * py, W + 2 * px), np.uint8)
    big[py:py + H, px:px + W] = values
    return big


def _cells(x, y, pivot, s, kk, rot):
    """(no cell anywhere, cx, cy, count) of rotation kk: the distinct rotated cells within reach of the window (of
    the bound's look-ups, which covers every candidate's), each with the number of points in it."""
    W, H, Ty, Tx = int(s["width"]), int(s["height"]), int(s["shift_y"]), int(s["shift_x"])
    has, cx, cy = mo.rotated_cells(x, y, pivot[0], pivot[1], rot[kk, 0], rot[kk, 1], s)
    near = has & (cx >= -Tx - (S - 1)) & (cx < W + Tx) & (cy >= -Ty - (S - 1)) & (cy < H + Ty)
    if not near.any():
        return bool((~has).any()), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    cells, cnt = np.unique(np.stack([cy[near], cx[near]], 1), axis=0, return_counts=True)
    return bool((~has).any()), cells[:, 1].astype(np.int64), cells[:, 0].astype(np.int64), cnt.astype(np.int64)


# ---- writer 1: exhaustive --------------------------------------------------------------------------------------------
def scores_exhaustive(x, y, pivot, s, field):
    """(volume (2K+1, 2Ty+1, 2Tx+1) uint32, any rotated position without a cell): E13's score of every candidate of
    the wide window, per distinct cell one window of the zero-surrounded field added whole."""
    K, Ty, Tx = int(s["rot_steps"]), int(s["shift_y"]), int(s["shift_x"])
    H, W = int(s["height"]), int(s["width"])
    big = _padded(mo.field_values(field).reshape(H, W), s)
    py, px = _pad(s)
    rot = mo.rotations(s)
    vol = np.zeros(mo.volume_shape(s), np.int64)
    no_cell = False
    for kk in range(2 * K + 1):
        nc, cx, cy, cnt = _cells(x, y, pivot, s, kk, rot)
        no_cell |= nc
        for ax, ay, c in zip(cx, cy, cnt):
            vol[kk] += c * big[ay + py - Ty:ay + py + Ty + 1, ax + px - Tx:ax + px + Tx + 1].astype(np.int64)
    assert vol.max(initial=0) < 2 ** 32
    return vol.astype(np.uint32), no_cell


def match_exhaustive(x, y, pivot, s, field):
    """(volume, best int64 (8,), status without the truncated bit): writer 1."""
    pivot = (0.0, 0.0) if pivot is None else pivot
    fx, fy = mo.finite_points(x, y)
    vol, no_cell = scores_exhaustive(fx, fy, pivot, s, field)
    return vol, mo.best_of(vol, s, len(fx)), mo.SCAN_CELL_RANGE if no_cell else 0


# ---- writer 2: bound and refine --------------------------------------------------------------------------------------
def block_candidates(s, v):
    """(k, j (8, 1), i (1, 8), in window (8, 8)) of the block with flat index v."""
    K, Ty, Tx = int(s["rot_steps"]), int(s["shift_y"]), int(s["shift_x"])
    _, nby, nbx = blocks_shape(s)
    kk, r = divmod(int(v), nby * nbx)
    bj, bi = divmod(r, nbx)
    j = (-Ty + bj * S + np.arange(S))[:, None]
    i = (-Tx + bi * S + np.arange(S))[None, :]
    return kk - K, j, i, (j <= Ty) & (i <= Tx)


def match_bound_refine(x, y, pivot, s, field):
    """Writer 2 -> dict(P (Hp, Wp) int8, U (2K+1, nby, nbx) uint32, work (8,), best int64 (8,), status, listed: the
    flat indices of the list, scores: {flat index: (8, 8) int64 scores of the block's candidates})."""
    pivot = (0.0, 0.0) if pivot is None else pivot
    x, y = mo.finite_points(x, y)
    K, Ty, Tx = int(s["rot_steps"]), int(s["shift_y"]), int(s["shift_x"])
    H, W = int(s["height"]), int(s["width"])
    cap = int(s["max_blocks"])
    rots, nby, nbx = blocks_shape(s)
    P = pool(np.asarray(field, np.int8).reshape(H, W))
    py, px = _pad(s)
    bigF = _padded(mo.field_values(field).reshape(H, W), s)
    bigP = np.zeros_like(bigF)  # P(x, y) at [y + py, x + px], 0 where P is not defined
    bigP[py - (S - 1):py + H, px - (S - 1):px + W] = P
    rot = mo.rotations(s)
    cells = []
    no_cell = False
    U = np.zeros((rots, nby, nbx), np.int64)
    for kk in range(rots):
        nc, cx, cy, cnt = _cells(x, y, pivot, s, kk, rot)
        no_cell |= nc
        cells.append((cx, cy, cnt))
        for ax, ay, c in zip(cx, cy, cnt):
            y0, x0 = ay + py - Ty, ax + px - Tx
            U[kk] += c * bigP[y0:y0 + S * nby:S, x0:x0 + S * nbx:S].astype(np.int64)
    assert U.max(initial=0) < 2 ** 32

    def block_scores(v):
        kr, j, i, inside = block_candidates(s, v)
        cx, cy, cnt = cells[kr + K]
        out = np.zeros((S, S), np.int64)
        for ax, ay, c in zip(cx, cy, cnt):
            y0, x0 = ay + py + int(j[0, 0]), ax + px + int(i[0, 0])
            out += c * bigF[y0:y0 + S, x0:x0 + S].astype(np.int64)
        return np.where(inside, out, -1)  # -1: not a candidate

    flat = U.ravel()
    seed_a = int(np.argmax(flat))  # (the first of the greatest)
    seed_b = (K * nby + Ty // S) * nbx + Tx // S
    seeds = [seed_a] if seed_a == seed_b else [seed_a, seed_b]
    scores = {v: block_scores(v) for v in seeds}
    b0 = max(int(scores[v].max()) for v in seeds)
    listed = np.flatnonzero(flat >= b0)
    n = len(listed)
    proven = n <= cap
    if proven:
        for v in listed:
            if int(v) not in scores:
                scores[int(v)] = block_scores(int(v))
    over = [int(v) for v in listed] if proven else seeds
    rows = []
    for v in over:
        kr, j, i, inside = block_candidates(s, v)
        jj, ii = np.broadcast_arrays(j, i)
        m = inside
        rows.append(np.stack([scores[v][m], np.full(m.sum(), kr), jj[m], ii[m]], 1))
    c = np.concatenate(rows)
    sc, k, j, i = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    w = np.lexsort((i, j, k, np.abs(k), i * i + j * j, -sc))[0]  # (the last key is the primary one)
    top = int(sc[w])
    zero = int(scores[seed_b][Ty % S, Tx % S])
    best = np.array([top, k[w], j[w], i[w], len(x), zero, int((sc == top).sum()), 0 if proven else UNPROVEN], np.int64)
    work = np.array([flat.size, int(flat[seed_a]), seed_a, b0, n, cap, 0, 0], np.int64)
    return dict(P=P, U=U.astype(np.uint32), work=work, best=best, status=mo.SCAN_CELL_RANGE if no_cell else 0,
                listed=listed, scores=scores, seeds=seeds)


def block_of(s, k, j, i) -> int:
    """The flat index of the block that holds candidate (k, j, i)."""
    K, Ty, Tx = int(s["rot_steps"]), int(s["shift_y"]), int(s["shift_x"])
    _, nby, nbx = blocks_shape(s)
    return ((k + K) * nby + (j + Ty) // S) * nbx + (i + Tx) // S
