"""Restatement of E13, correlative scan matching of a group of scans against a likelihood field
(include/rplgpu_msg.h, rplgpu_match_scans_dev), in numpy, twice: (a) per point and candidate, the plain gather;
(b) per rotation, a histogram of the rotated cells cross-correlated with the clipped field over the shift
window.  The two writers must agree (tests/test_match_cpu.py).  Plus the spec check, the rotation table by the
header's formula and the tie rule as a plain lexicographic sort.  TEST INFRASTRUCTURE — imported by tests/ only.

Points: tests/fused_oracle.group_points, the composition E8, E9 and E11 use; the cell rule: tests/occ_oracle.cells_of."""
from __future__ import annotations

import math

import numpy as np

from tests.fused_oracle import group_points
from tests.occ_oracle import cells_of

F32 = np.float32
MAX_DIM = 4096
MAX_SHIFT = 32
MAX_ROT = 64
SCAN_CELL_RANGE = 0x2
DEFAULT = dict(origin_x=-25.6, origin_y=-25.6, resolution=0.05, width=1024, height=1024, shift_x=6, shift_y=6,
               rot_steps=10, rot_step=float(F32(0.25 * math.pi / 180.0)))


def spec(**kw) -> dict:
    d = dict(DEFAULT)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return d


def spec_valid(s: dict) -> bool:
    f = [F32(s[k]) for k in ("origin_x", "origin_y", "resolution", "rot_step")]
    if not all(np.isfinite(v) for v in f):
        return False
    if not f[2] > 0:
        return False
    if not (1 <= s["width"] <= MAX_DIM and 1 <= s["height"] <= MAX_DIM):
        return False
    if s["shift_x"] > MAX_SHIFT or s["shift_y"] > MAX_SHIFT or s["rot_steps"] > MAX_ROT:
        return False
    K = int(s["rot_steps"])
    if K > 0 and (not f[3] > 0 or float(K) * float(f[3]) > math.pi / 2):
        return False
    return True


def rotations(s: dict) -> np.ndarray:
    """(2K + 1, 2) float32: (float)cos((double)k * (double)rot_step), (float)sin(the same), k = -K .. K."""
    K = int(s["rot_steps"])
    step = float(F32(s["rot_step"]))
    return np.array([[F32(math.cos(k * step)), F32(math.sin(k * step))] for k in range(-K, K + 1)], F32).reshape(-1, 2)


def volume_shape(s: dict):
    return 2 * int(s["rot_steps"]) + 1, 2 * int(s["shift_y"]) + 1, 2 * int(s["shift_x"]) + 1


def volume_size(s: dict) -> int:
    a, b, c = volume_shape(s)
    return a * b * c


def field_values(field) -> np.ndarray:
    """max((int8)byte, 0) as int64, (H, W)."""
    return np.maximum(np.asarray(field, np.int8).astype(np.int64), 0)


# ---- the candidate's rotation and cell -------------------------------------------------------------------------
def rotated_cells(x, y, px, py, c, sn, s):
    """(has cell, cx, cy) of the finite points (x, y) turned by (c, sn) about (px, py): float32, every product,
    then the difference (sum), then the sum with the pivot rounded."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    px, py, c, sn = F32(px), F32(py), F32(c), F32(sn)
    with np.errstate(all="ignore"):
        qx, qy = (x - px).astype(F32), (y - py).astype(F32)
        rx = (((c * qx).astype(F32) - (sn * qy).astype(F32)).astype(F32) + px).astype(F32)
        ry = (((sn * qx).astype(F32) + (c * qy).astype(F32)).astype(F32) + py).astype(F32)
    return cells_of(rx, ry, s)


def finite_points(x, y):
    m = np.isfinite(x) & np.isfinite(y)
    return np.asarray(x, F32)[m], np.asarray(y, F32)[m]


# ---- writer (a): per point and candidate, the plain gather -----------------------------------------------------
def scores_gather(x, y, pivot, s, field):
    """(volume (2K+1, 2Ty+1, 2Tx+1) uint32, any rotated position without a cell) of the finite points."""
    W, H = int(s["width"]), int(s["height"])
    K, Ty, Tx = int(s["rot_steps"]), int(s["shift_y"]), int(s["shift_x"])
    f = field_values(field).reshape(H, W)
    rot = rotations(s)
    vol = np.zeros(volume_shape(s), np.int64)
    no_cell = False
    for kk in range(2 * K + 1):
        has, cx, cy = rotated_cells(x, y, pivot[0], pivot[1], rot[kk, 0], rot[kk, 1], s)
        no_cell |= bool((~has).any())
        cx, cy = cx[has], cy[has]
        for j in range(-Ty, Ty + 1):
            for i in range(-Tx, Tx + 1):
                ax, ay = cx + i, cy + j
                ok = (ax >= 0) & (ax < W) & (ay >= 0) & (ay < H)
                vol[kk, j + Ty, i + Tx] = int(f[ay[ok], ax[ok]].sum())
    assert vol.max(initial=0) < 2 ** 32
    return vol.astype(np.uint32), no_cell


# ---- writer (b): per rotation, histogram x clipped field -------------------------------------------------------------
def scores_correlate(x, y, pivot, s, field):
    """The same volume: the rotated cells within reach of the grid counted into a histogram over
    [-Tx, W + Tx) x [-Ty, H + Ty), then for every shift the sum of histogram x field, the field clipped at 0 and
    surrounded by zeros."""
    W, H = int(s["width"]), int(s["height"])
    K, Ty, Tx = int(s["rot_steps"]), int(s["shift_y"]), int(s["shift_x"])
    big = np.zeros((H + 4 * Ty, W + 4 * Tx), np.int64)  # the field at [2Ty, 2Ty + H) x [2Tx, 2Tx + W)
    big[2 * Ty:2 * Ty + H, 2 * Tx:2 * Tx + W] = field_values(field).reshape(H, W)
    rot = rotations(s)
    vol = np.zeros(volume_shape(s), np.int64)
    no_cell = False
    for kk in range(2 * K + 1):
        has, cx, cy = rotated_cells(x, y, pivot[0], pivot[1], rot[kk, 0], rot[kk, 1], s)
        no_cell |= bool((~has).any())
        near = has & (cx >= -Tx) & (cx < W + Tx) & (cy >= -Ty) & (cy < H + Ty)
        hist = np.zeros((H + 2 * Ty, W + 2 * Tx), np.int64)  # cell (cx, cy) at [cy + Ty, cx + Tx]
        np.add.at(hist, (cy[near] + Ty, cx[near] + Tx), 1)
        ys, xs = np.nonzero(hist.any(1))[0], np.nonzero(hist.any(0))[0]
        if len(ys) == 0:
            continue
        y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1  # the histogram's bounding box
        h = hist[y0:y1, x0:x1]
        for j in range(-Ty, Ty + 1):
            for i in range(-Tx, Tx + 1):
                # histogram row r is cell row r - Ty, which candidate j reads at big row (r - Ty + j) + 2 Ty
                vol[kk, j + Ty, i + Tx] = int((h * big[y0 + Ty + j:y1 + Ty + j, x0 + Tx + i:x1 + Tx + i]).sum())
    assert vol.max(initial=0) < 2 ** 32
    return vol.astype(np.uint32), no_cell


# ---- the best candidate -----------------------------------------------------------------------------------------
def best_of(vol, s, n_finite):
    """The eight result words (int64; k, j, i signed) by a plain lexicographic sort over every candidate:
    largest score, then smallest i*i + j*j, |k|, k, j, i."""
    K, Ty, Tx = int(s["rot_steps"]), int(s["shift_y"]), int(s["shift_x"])
    vol = np.asarray(vol, np.uint32).reshape(volume_shape(s)).astype(np.int64)
    k, j, i = np.meshgrid(np.arange(-K, K + 1), np.arange(-Ty, Ty + 1), np.arange(-Tx, Tx + 1), indexing="ij")
    k, j, i, sc = k.ravel(), j.ravel(), i.ravel(), vol.ravel()
    order = np.lexsort((i, j, k, np.abs(k), i * i + j * j, -sc))  # (the last key is the primary one)
    w = order[0]
    top = int(sc[w])
    return np.array([top, k[w], j[w], i[w], n_finite, int(vol[K, Ty, Tx]), int((sc == top).sum()), 0], np.int64)


def best_words(best) -> np.ndarray:
    """The result as the eight uint32 words in memory (k, j, i two's complement)."""
    return (np.asarray(best, np.int64) & 0xFFFFFFFF).astype(np.uint32)


# ---- a group ---------------------------------------------------------------------------------------------------------
def match_points(x, y, pivot, s, field, writer=scores_correlate):
    """(volume uint32, best int64 (8,), status without the truncated bit) of a group's points."""
    pivot = (0.0, 0.0) if pivot is None else pivot
    fx, fy = finite_points(x, y)
    vol, no_cell = writer(fx, fy, pivot, s, field)
    return vol, best_of(vol, s, len(fx)), SCAN_CELL_RANGE if no_cell else 0


def match_group(oracle, scans, p, s, field, motion=None, pose2d=None, t0=None, pivot=None, writer=scores_correlate):
    x, y, _, _, _, _ = group_points(oracle, scans, p, motion, pose2d, t0)
    return match_points(x, y, pivot, s, field, writer)


# ---- a displaced prior ---------------------------------------------------------------------------------------------------
def displaced_poses(pose2d, pivot, s, k0, j0, i0):
    """pose2d (S, 6) displaced by (k0, j0, i0): translated by (i0, j0) * resolution, then turned by k0 * rot_step
    about the pivot (float64, then rounded).  The inverse of that motion is "turn by -k0 * rot_step about the
    pivot, then translate by (-i0, -j0) * resolution": candidate (-k0, -j0, -i0) of the search window."""
    a = k0 * float(F32(s["rot_step"]))
    c, sn = math.cos(a), math.sin(a)
    res = float(F32(s["resolution"]))
    px, py = (0.0, 0.0) if pivot is None else (float(pivot[0]), float(pivot[1]))
    out = []
    for r00, r01, tx, r10, r11, ty in np.asarray(pose2d, np.float64).reshape(-1, 6):
        qx, qy = tx + i0 * res - px, ty + j0 * res - py
        out.append([c * r00 - sn * r10, c * r01 - sn * r11, c * qx - sn * qy + px,
                    sn * r00 + c * r10, sn * r01 + c * r11, sn * qx + c * qy + py])
    return np.array(out, F32)
