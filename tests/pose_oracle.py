"""Restatement of E15, a list of arbitrary poses weighed against a likelihood field (include/rplgpu_msg.h,
rplgpu_score_poses_dev), in numpy, twice: (a) per pose, the plain gather of the field under every point; (b) per
pose, a bincount of the flat cell index dotted with the clipped field.  The two writers must agree
(tests/test_pose_cpu.py).  Both are pure functions of ONE pose, so equal poses are computed once.  Plus the spec
check, the pose list by the header's formula, the result words by a plain lexsort and Python integers, and the
kernel's layout formula.  TEST INFRASTRUCTURE — imported by tests/ only.

Points: tests/fused_oracle.group_points, the composition E8, E9, E11 and E13 use; the cell rule:
tests/occ_oracle.cells_of."""
from __future__ import annotations

import numpy as np

from tests.fused_oracle import group_points
from tests.occ_oracle import cells_of

F32 = np.float32
MAX_DIM = 4096
MAX_POSES = 1 << 20
SCAN_CELL_RANGE = 0x2
TILE = 1024  # poses per workgroup, threads per workgroup (csrc/rpl_front.hpp: kPoseTile = kBlock)
DEFAULT = dict(origin_x=-25.6, origin_y=-25.6, resolution=0.05, width=1024, height=1024)


def spec(**kw) -> dict:
    d = dict(DEFAULT)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return d


def spec_valid(s: dict) -> bool:
    f = [F32(s[k]) for k in ("origin_x", "origin_y", "resolution")]
    if not all(np.isfinite(v) for v in f):
        return False
    if not f[2] > 0:
        return False
    return 1 <= s["width"] <= MAX_DIM and 1 <= s["height"] <= MAX_DIM


def pose_list(xyt) -> np.ndarray:
    """(P, 4) float32 (cos, sin, x, y): cos and sin in fp64, rounded once; theta == 0 gives exactly (1, 0)."""
    xyt = np.asarray(xyt, np.float64).reshape(-1, 3)
    out = np.zeros((len(xyt), 4), F32)
    for q, (x, y, th) in enumerate(xyt):
        with np.errstate(all="ignore"):
            c, s = (1.0, 0.0) if th == 0 else (np.cos(np.float64(th)), np.sin(np.float64(th)))
            out[q] = F32(c), F32(s), F32(x), F32(y)
    return out


def layout(P: int, tile: int = TILE):
    """The kernel's layout formula (csrc/rpl_pose.hip, k_pose_score): (threads of one copy of the list, copies of
    the list in a workgroup, tiles, poses of the last tile)."""
    per = min((P + 63) & ~63, tile)
    slices = tile // per if P <= tile else 1
    tiles = (P + tile - 1) // tile
    return per, slices, tiles, P - (tiles - 1) * tile


def field_values(field) -> np.ndarray:
    """max((int8)byte, 0) as int64, (H, W)."""
    return np.maximum(np.asarray(field, np.int8).astype(np.int64), 0)


def finite_points(x, y):
    m = np.isfinite(x) & np.isfinite(y)
    return np.asarray(x, F32)[m], np.asarray(y, F32)[m]


def posed_cells(x, y, pose, s):
    """(has cell, cx, cy) of the finite points (x, y) at pose (c, sn, tx, ty): float32, every product, then the
    difference (sum), then the sum with the translation rounded."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    c, sn, tx, ty = (F32(v) for v in pose)
    with np.errstate(all="ignore"):
        rx = (((c * x).astype(F32) - (sn * y).astype(F32)).astype(F32) + tx).astype(F32)
        ry = (((sn * x).astype(F32) + (c * y).astype(F32)).astype(F32) + ty).astype(F32)
    return cells_of(rx, ry, s)


# ---- writer (a): per pose, the plain gather -----------------------------------------------------------------------
def weight_gather(x, y, pose, s, field):
    """(weight, any position without a cell) of the finite points at ONE pose."""
    W, H = int(s["width"]), int(s["height"])
    f = field_values(field).reshape(H, W)
    has, cx, cy = posed_cells(x, y, pose, s)
    cx, cy = cx[has], cy[has]
    ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    return int(f[cy[ok], cx[ok]].sum()), bool((~has).any())


# ---- writer (b): per pose, bincount of the flat cell index . clipped field ----------------------------------------------
def weight_bincount(x, y, pose, s, field):
    W, H = int(s["width"]), int(s["height"])
    has, cx, cy = posed_cells(x, y, pose, s)
    ok = has & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    hist = np.bincount((cy[ok] * W + cx[ok]).astype(np.int64), minlength=W * H)
    return int(np.dot(hist.astype(np.int64), field_values(field).reshape(-1))), bool((~has).any())


def weights_of(x, y, poses, s, field, writer=weight_bincount):
    """(weights (P,) uint32, status without the truncated bit, per-pose "some position has no cell" (P,) bool) of
    the finite points; poses that are equal bit for bit are computed once."""
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 4)
    uniq, inv = np.unique(poses.view(np.uint32), axis=0, return_inverse=True)
    got = [writer(x, y, u.view(F32), s, field) for u in uniq]
    out = np.array([g[0] for g in got], np.int64)[inv.reshape(-1)]
    no_cell = np.array([g[1] for g in got], bool)[inv.reshape(-1)]
    assert out.max(initial=0) < 2 ** 32
    return out.astype(np.uint32), SCAN_CELL_RANGE if no_cell.any() else 0, no_cell


# ---- the result words -------------------------------------------------------------------------------------------------
def result_of(weights, n_finite) -> np.ndarray:
    """The eight result words (uint32) by a plain lexicographic sort and Python integers."""
    w = [int(v) for v in np.asarray(weights, np.uint32)]
    q = np.arange(len(w))
    order = np.lexsort((q, -np.asarray(w, np.int64)))  # (the last key is the primary one)
    top = w[order[0]]
    total = sum(w)
    return np.array([top, int(order[0]), sum(1 for v in w if v == top), sum(1 for v in w if v == 0), int(n_finite),
                     w[0], total & 0xFFFFFFFF, total >> 32], np.uint64).astype(np.uint32)


# ---- a group ---------------------------------------------------------------------------------------------------------------
def score_points(x, y, poses, s, field, writer=weight_bincount):
    """(weights uint32 (P,), result uint32 (8,), status without the truncated bit) of a group's points."""
    fx, fy = finite_points(x, y)
    w, status, _ = weights_of(fx, fy, poses, s, field, writer)
    return w, result_of(w, len(fx)), status


def score_group(oracle, scans, p, s, poses, field, motion=None, pose2d=None, t0=None, writer=weight_bincount):
    x, y, _, _, _, _ = group_points(oracle, scans, p, motion, pose2d, t0)
    return score_points(x, y, poses, s, field, writer)
