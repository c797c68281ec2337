"""The oracle of E20 (include/rplgpu_msg.h, the E20 block): a pose list binned in (x, y, heading) and marked in a bit
map, by two writers that share no step.

(a) ``writer_a``: numpy — the float32 steps in float32 arrays, the header's bisection vectorised over the poses, the
    map by ``np.bitwise_or.at``, K by the popcount of the map.
(b) ``writer_b``: a Python loop — doubles rounded to float32 after every operation, the angular order by quadrants
    and cross-multiplied tangents in Python integers, the heading bin by COUNTING the edges <= h (valid tables only),
    a set of bin ids, K its size.

``bin_poses`` runs (a), and (b) beside it up to 4096 poses on valid tables, and returns (a)'s answer once they
agree."""
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
NONE = 0xFFFFFFFF
B_LIMIT = 4096

Spec = namedtuple("Spec", "origin_x origin_y inv_size nx ny keep")


def spec(origin_x=-25.6, origin_y=-25.6, inv_size=2.0, nx=103, ny=103, keep=0):
    return Spec(float(F32(origin_x)), float(F32(origin_y)), float(F32(inv_size)), int(nx), int(ny), int(keep))


def map_words(s, T):
    return (s.nx * s.ny * T + 31) // 32


def table(T):
    """T evenly spaced edges (cos, sin)(2 pi k / T) as float32, entry 0 exactly (1, 0)"""
    a = 2.0 * np.pi * np.arange(T, dtype=np.float64) / T
    t = np.stack([np.cos(a), np.sin(a)], axis=1).astype(F32)
    t[0] = (1.0, 0.0)
    return t


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def a_quantise(cs):
    """(n, 2) float32 -> ((n, 2) int64, usable (n,) bool): in range and not (0, 0)"""
    cs = np.ascontiguousarray(cs, F32).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        t = cs * F32(1048576.0)
        inr = (np.abs(t) < F32(8388608.0)).all(axis=1)
        q = np.where(inr[:, None], np.rint(np.where(inr[:, None], t, F32(0))), 0).astype(np.int64)
    return q, inr & (q != 0).any(axis=1)


def a_half(q):
    return np.where((q[:, 1] > 0) | ((q[:, 1] == 0) & (q[:, 0] > 0)), 0, 1)


def a_le(a, a_ok, b):
    ha, hb = a_half(a), a_half(b)
    cross = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return a_ok & ((ha < hb) | ((ha == hb) & (cross >= 0)))


def a_heading_bins(hq, eq, e_ok):
    T = len(eq)
    lo = np.zeros(len(hq), np.int64)
    hi = np.full(len(hq), T, np.int64)
    for _ in range(10):
        act = hi - lo > 1
        mid = np.minimum((lo + hi) >> 1, T - 1)
        le = a_le(eq[mid], e_ok[mid], hq)
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid, hi)
    assert (hi - lo <= 1).all()
    return lo


def writer_a(s, poses, weights, edges, map_in=None):
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 4)
    P, T = len(poses), len(edges)
    words = map_words(s, T)
    before = np.zeros(words, np.uint32) if not s.keep else np.array(map_in, np.uint32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        fx = (poses[:, 2] - F32(s.origin_x)) * F32(s.inv_size)
        fy = (poses[:, 3] - F32(s.origin_y)) * F32(s.inv_size)
        pos_in = (fx >= F32(0)) & (fx < F32(s.nx)) & (fy >= F32(0)) & (fy < F32(s.ny))
    assert fx.dtype == F32
    bx = np.floor(np.where(pos_in, fx, F32(0))).astype(np.int64)
    by = np.floor(np.where(pos_in, fy, F32(0))).astype(np.int64)
    hq, h_ok = a_quantise(poses[:, :2])
    eq, e_ok = a_quantise(edges)
    kt = a_heading_bins(hq, eq, e_ok)
    skipped = np.zeros(P, bool) if weights is None else np.asarray(weights, np.uint32) == 0
    counted = ~skipped & pos_in & h_ok
    b = (kt * s.ny + by) * s.nx + bx
    bins = np.where(counted, b, NONE).astype(np.uint32)
    after = before.copy()
    bc = b[counted]
    np.bitwise_or.at(after, bc >> 5, (np.uint32(1) << (bc & 31).astype(np.uint32)))
    K = int(np.unpackbits(after.view(np.uint8)).sum()) - int(np.unpackbits(before.view(np.uint8)).sum())
    n_in, n_skip = int(counted.sum()), int(skipped.sum())
    n_out = P - n_in - n_skip
    res = np.array([K, n_in, n_out, n_skip, bc.min() if n_in else NONE, bc.max() if n_in else 0, 0,
                    (0 if n_in else 1) | (2 if n_out else 0) | (4 if s.keep else 0)], np.uint32)
    return after, bins, res


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def r32(v):
    """a double rounded to float32 once (overflow to an infinity)"""
    with np.errstate(over="ignore"):
        return float(F32(v))


def b_quantise(c, s):
    """-> (C, S) or None for an entry that is out of range or (0, 0)"""
    tc, ts = r32(float(c) * 1048576.0), r32(float(s) * 1048576.0)
    if math.isnan(tc) or math.isnan(ts) or not (abs(tc) < 8388608.0 and abs(ts) < 8388608.0):
        return None
    q = (round(tc), round(ts))          # Python rounds halves to even
    return None if q == (0, 0) else q


def b_turned(q):
    """the quadrant of q counted from the positive x axis, and q turned back by it into [0, 90) degrees"""
    C, S = q
    if C > 0 and S >= 0:
        return 0, (C, S)
    if C <= 0 and S > 0:
        return 1, (S, -C)
    if C < 0 and S <= 0:
        return 2, (-C, -S)
    return 3, (-S, C)


def b_le(a, b):
    """the angle of a in [0, 360) <= the angle of b, by quadrants and then tangents cross-multiplied"""
    qa, (ca, sa) = b_turned(a)
    qb, (cb, sb) = b_turned(b)
    if qa != qb:
        return qa < qb
    return sa * cb <= sb * ca           # ca, cb > 0


def valid_table(edges):
    e = [b_quantise(c, s) for c, s in np.asarray(edges, F32).reshape(-1, 2)]
    if not e or e[0] != (1 << 20, 0) or any(q is None for q in e):
        return False
    return all(not b_le(e[k], e[k - 1]) for k in range(1, len(e)))


def writer_b(s, poses, weights, edges, map_in=None):
    T = len(edges)
    assert valid_table(edges)
    e = [b_quantise(c, v) for c, v in np.asarray(edges, F32).reshape(-1, 2)]
    old = set()
    if s.keep:
        for w, word in enumerate(np.asarray(map_in, np.uint32).tolist()):
            old.update(32 * w + i for i in range(32) if word >> i & 1)
    seen, bins = set(), []
    n_in = n_out = n_skip = 0
    for i, (c, v, x, y) in enumerate(np.asarray(poses, F32).reshape(-1, 4).tolist()):
        if weights is not None and int(weights[i]) == 0:
            n_skip += 1
            bins.append(NONE)
            continue
        fx = r32(r32(x - s.origin_x) * s.inv_size)
        fy = r32(r32(y - s.origin_y) * s.inv_size)
        h = b_quantise(c, v)
        if not (0.0 <= fx < s.nx and 0.0 <= fy < s.ny) or h is None:      # (a NaN fails the chain)
            n_out += 1
            bins.append(NONE)
            continue
        kt = sum(1 for q in e if b_le(q, h)) - 1
        b = (kt * s.ny + math.floor(fy)) * s.nx + math.floor(fx)
        n_in += 1
        seen.add(b)
        bins.append(b)
    words = np.zeros(map_words(s, T), np.uint32)
    for b in seen | old:
        words[b >> 5] |= np.uint32(1 << (b & 31))
    res = np.array([len(seen - old), n_in, n_out, n_skip, min(seen) if seen else NONE, max(seen) if seen else 0, 0,
                    (0 if n_in else 1) | (2 if n_out else 0) | (4 if s.keep else 0)], np.uint32)
    return words, np.array(bins, np.uint32), res


def bin_poses(s, poses, weights, edges, map_in=None, both=None):
    """-> (map, bins, result) of ONE group; writer (b) beside (a) where the module's header says so (``both``
    overrides)"""
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 4)
    got = writer_a(s, poses, weights, edges, map_in)
    if both is None:
        both = len(poses) <= B_LIMIT and valid_table(edges)
    if both:
        other = writer_b(s, poses, weights, edges, map_in)
        for k, (x, y) in enumerate(zip(got, other)):
            assert x.tobytes() == y.tobytes(), f"the two writers differ in output {k}"
    return got
