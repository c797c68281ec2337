"""E17's rule (include/rplgpu_msg.h, the E17 block) written twice, with no summation step in common:
  (a) ``sums_python``: Python integers, pose by pose;
  (b) ``sums_limbs``: numpy int64 dot products over limbs — w in four bytes, a moment split at 24 bits — recombined by
      shifts in Python integers; every partial stays below 2^53 (2^8 * 2^24 * 2^20 = 2^52).
The quantisation is numpy float32 (one product, ``np.rint``: ties to even).  Above 4096 poses use (b) alone."""
import numpy as np

F32 = np.float32
WORDS = 72
TILE = 1024
OPEN_R2 = (1 << 64) - 1
OPEN_DOT = -(1 << 63)
DEFAULT = dict(xy_scale=1024.0, gate_r2=512 * 512, gate_dot=15 << 36)
OPEN = dict(xy_scale=1024.0, gate_r2=OPEN_R2, gate_dot=OPEN_DOT)


def tiles(P):
    return (P + TILE - 1) // TILE


def scratch_words(G, P):
    if G == 0 or G > 65535 or P == 0 or P > (1 << 20):
        return 0
    return G * 68 * tiles(P)


def quantise(poses, xy_scale):
    """poses (P, 4) float32 (c, s, x, y) -> (q (P, 4) int64 in the order X, Y, C, S; in_range (P,) bool)"""
    poses = np.asarray(poses, F32)
    with np.errstate(all="ignore"):
        t = np.stack([poses[:, 2] * F32(xy_scale), poses[:, 3] * F32(xy_scale), poses[:, 0] * F32(1048576.0),
                      poses[:, 1] * F32(1048576.0)], axis=1)
        assert t.dtype == F32
        inr = (np.abs(t) < F32(8388608.0)).all(axis=1)
        q = np.rint(np.where(inr[:, None], t, F32(0))).astype(np.int64)
    return q, inr, t


def gate_of(q, inr, qc, spec):
    """the poses in the gate around pose qc (bool)"""
    if not inr[qc]:
        return np.zeros(len(q), bool)
    d = q[:, :2] - q[qc, :2]                       # |d| <= 2^24: the squares fit int64
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]     # < 2^50
    dot = q[:, 2] * q[qc, 2] + q[:, 3] * q[qc, 3]  # |.| <= 2^47
    # both bounds clamped to +-2^62, far beyond what r2 and dot reach: the int64 comparisons decide as the integers do
    ok = (r2 <= min(spec["gate_r2"], 1 << 62)) & (dot >= min(max(spec["gate_dot"], -(1 << 62)), 1 << 62))
    return inr & ok


def sums_python(q, w, mask):
    s = [0] * 8
    for (X, Y, C, S), wi, m in zip(q.tolist(), w.tolist(), mask.tolist()):
        if m:
            for k, v in enumerate((1, X, Y, C, S, X * X, X * Y, Y * Y)):
                s[k] += wi * v
    return s


def sums_limbs(q, w, mask):
    w = np.where(mask, w, 0).astype(np.int64)
    b = [(w >> (8 * k)) & 0xFF for k in range(4)]
    X, Y, C, S = (q[:, k] for k in range(4))
    out = []
    for v in (np.ones(len(q), np.int64), X, Y, C, S, X * X, X * Y, Y * Y):
        lo, hi = v & 0xFFFFFF, v >> 24             # (an arithmetic shift: lo + 2^24 hi == v for either sign)
        out.append(sum((int(np.dot(b[k], lo)) + (int(np.dot(b[k], hi)) << 24)) << (8 * k) for k in range(4)))
    return out


def words_of(v):
    v &= (1 << 128) - 1
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(4)]


def value_of(words):
    v = sum(int(x) << (32 * j) for j, x in enumerate(words))
    return v - (1 << 128) if v >> 127 else v


def sums_of_result(res, k):
    return [value_of(res[8 + 32 * k + 4 * m:12 + 32 * k + 4 * m]) for m in range(8)]


def estimate(poses, w, spec, center=0, writer=None):
    """one group -> the 72 result words (uint32)"""
    P = len(poses)
    if writer is None:
        writer = sums_python if P <= 4096 else sums_limbs
    assert writer is sums_limbs or P <= 4096
    q, inr, _ = quantise(poses, spec["xy_scale"])
    w = np.ones(P, np.uint32) if w is None else np.asarray(w, np.uint32)
    qc = min(int(center), P - 1)
    gate = gate_of(q, inr, qc, spec)
    s0, s1 = writer(q, w, inr), writer(q, w, gate)
    res = [(0 if inr[qc] else 1) | (2 if not inr.all() else 0) | (4 if s0[0] == 0 else 0) | (8 if s1[0] == 0 else 0),
           qc, int(inr.sum()), int((inr & (w != 0)).sum()), int(gate.sum()), int((gate & (w != 0)).sum()), 0, 0]
    for s in (s0, s1):
        for v in s:
            res += words_of(v)
    return np.array(res, np.uint32)
