"""Restatement of E23, the beams a pose list disagrees with left out of the weights (include/rplgpu_msg.h,
rplgpu_score_poses_agree_dev), in numpy, twice, with no step shared behind the points:
  (a) per pose: the plain gather of the field under every point, a boolean row "agrees" over the samples, the rows
      summed; the weights by a second gather over the samples that entered;
  (b) per sample: the flat cell index into the clipped field, a bincount over the agreeing (pose, sample) pairs; the
      weights as E15's (tests/pose_oracle.weight_bincount) minus the skipped samples' sums.
The decision, the agree words and the result words are Python integers.  The two writers must agree
(tests/test_agree_cpu.py).  TEST INFRASTRUCTURE — imported by tests/ only.

Points: tests/fused_oracle.group_points (with the scan slot and sample index); the cell rule:
tests/occ_oracle.cells_of through tests/pose_oracle.posed_cells."""
from __future__ import annotations

import numpy as np

from tests import pose_oracle as po
from tests.fused_oracle import group_points

F32 = np.float32
MAX_DEN = 1 << 20
DEFAULT = dict(po.DEFAULT, agree_lo=1, keep_num=3, keep_den=10, err_num=9, err_den=10)


def spec(**kw) -> dict:
    d = dict(DEFAULT)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return d


def grid_of(s) -> dict:
    return {k: s[k] for k in po.DEFAULT}


def spec_valid(s: dict) -> bool:
    if not po.spec_valid(grid_of(s)):
        return False
    if not 1 <= s["agree_lo"] <= 127:
        return False
    if not (1 <= s["keep_den"] <= MAX_DEN and 0 <= s["keep_num"] <= s["keep_den"]):
        return False
    return 1 <= s["err_den"] <= MAX_DEN and 0 <= s["err_num"] <= MAX_DEN


# ---- the decision, in Python integers ------------------------------------------------------------------------------------
def kept_by_rule(count: int, P: int, s) -> bool:
    return int(count) * int(s["keep_den"]) > int(s["keep_num"]) * int(P)


def falls_back(F: int, K: int, s) -> bool:
    return F > 0 and (F - K) * int(s["err_den"]) >= int(s["err_num"]) * F


def agree_words(counts, kept, back) -> np.ndarray:
    """The eight agree words from the finite samples' counts (Python ints) and their kept flags."""
    c = [int(v) for v in counts]
    F, K, total = len(c), sum(1 for k in kept if k), sum(c)
    return np.array([F, K, 1 if back else 0, F if back else K, max(c, default=0), min(c, default=0),
                     total & 0xFFFFFFFF, total >> 32], np.uint64).astype(np.uint32)


# ---- writer (a): per pose, a boolean row over the samples -------------------------------------------------------------------
def _gather(x, y, pose, s, fv):
    """(f (m,) int64, some position has no cell) of the finite points at ONE pose: the plain gather."""
    W, H = int(s["width"]), int(s["height"])
    has, cx, cy = po.posed_cells(x, y, pose, s)
    ok = has & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    f = np.zeros(len(x), np.int64)
    f[ok] = fv[cy[ok], cx[ok]]
    return f, bool((~has).any())


def writer_rows(x, y, poses, s, field):
    """-> (counts (m,) int, weights (P,) int, kept (m,) bool, back, no_cell) over the finite points."""
    g = grid_of(s)
    fv = po.field_values(field).reshape(int(s["height"]), int(s["width"]))
    P = len(poses)
    counts = np.zeros(len(x), np.int64)
    no_cell = False
    for pose in poses:
        f, nc = _gather(x, y, pose, g, fv)
        counts += (f >= s["agree_lo"])  # the pose's row
        no_cell |= nc
    kept = np.array([kept_by_rule(c, P, s) for c in counts], bool)
    back = falls_back(len(x), int(kept.sum()), s)
    entered = np.ones(len(x), bool) if back else kept
    weights = [int(_gather(x, y, pose, g, fv)[0][entered].sum()) for pose in poses]
    return counts, weights, kept, back, no_cell


# ---- writer (b): per sample, a bincount over the agreeing pairs; E15 minus the skipped ---------------------------------------
def writer_pairs(x, y, poses, s, field):
    g = grid_of(s)
    W, H = int(s["width"]), int(s["height"])
    flat = np.concatenate([po.field_values(field).reshape(-1), [0]])  # one more slot, 0: no cell, or outside
    P, m = len(poses), len(x)
    pairs, per_pose = [], []
    no_cell = False
    for pose in poses:
        has, cx, cy = po.posed_cells(x, y, pose, g)
        inside = has & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        at = np.where(inside, cy.astype(np.int64) * W + cx.astype(np.int64), W * H)
        per_pose.append(at)
        pairs.append(np.flatnonzero(flat[at] >= s["agree_lo"]))
        no_cell |= bool((~has).any())
    counts = np.bincount(np.concatenate(pairs) if pairs else np.zeros(0, np.int64), minlength=m)
    kept = np.array([kept_by_rule(c, P, s) for c in counts], bool)
    back = falls_back(m, int(kept.sum()), s)
    e15, _, _ = po.weights_of(x, y, poses, g, field, po.weight_bincount)
    skipped = np.flatnonzero(~kept)
    weights = []
    for q in range(P):
        w = int(e15[q])
        if not back:
            w -= int(flat[per_pose[q][skipped]].sum())
        weights.append(w)
    return counts, weights, kept, back, no_cell


WRITERS = dict(rows=writer_rows, pairs=writer_pairs)


# ---- a group --------------------------------------------------------------------------------------------------------------
def agree_points(x, y, slot, index, n_scans, n_stride, poses, s, field, writer="pairs"):
    """(counts (n_scans, n_stride) uint32, mask (n_scans, ceil(n_stride / 32)) uint32, weights (P,) uint32, result (8,)
    uint32, agree (8,) uint32, status without the truncated bit) of a group's points."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    slot, index = np.asarray(slot, np.int64), np.asarray(index, np.int64)
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 4)
    fin = np.isfinite(x) & np.isfinite(y)
    x, y, slot, index = x[fin], y[fin], slot[fin], index[fin]
    assert len(set(zip(slot.tolist(), index.tolist()))) == len(x) and (index < n_stride).all()
    c, w, kept, back, no_cell = WRITERS[writer](x, y, poses, s, field)
    counts = np.zeros((n_scans, n_stride), np.uint32)
    counts[slot, index] = c
    mask = np.zeros((n_scans, (n_stride + 31) // 32), np.uint32)
    for sl, i in zip(slot[kept], index[kept]):
        mask[sl, i >> 5] |= np.uint32(1 << (int(i) & 31))
    assert all(0 <= v < 2 ** 32 for v in w)
    weights = np.array(w, np.uint64).astype(np.uint32)
    return (counts, mask, weights, po.result_of(weights, len(x)), agree_words(c, kept, back),
            po.SCAN_CELL_RANGE if no_cell else 0)


def group_xy(oracle, scans, p, motion=None, pose2d=None, t0=None):
    """(x, y, slot, sample index) of every point of a group that E1 and E5 keep (finite or not)."""
    x, y, _, slot, idx, _ = group_points(oracle, scans, p, motion, pose2d, t0)
    return x, y, slot, idx
