"""Restatement of E9, the merged LaserScan of a group of scans (include/rplgpu_msg.h,
rplgpu_merge_scans_dev).  TEST INFRASTRUCTURE — imported by tests/ only.

Points: the C oracle's E1 + E2 cloud (oracle_lib.scan_to_cloud), E5 by oracle_lib.ror_mask on that cloud,
E6 and the planar pose by oracle/fusion_oracle.py — the composition test_gpu_msg.py's E8 oracle uses.
On top of it, in numpy, the E9 bin rule and the reduction.  Edges use math.cos / math.sin (the C
library the product's host code calls), never np.cos, whose SIMD paths may differ by an ulp."""
from __future__ import annotations

import math

import numpy as np

MAX_BEAMS = 16384
F32 = np.float32


def spec_inc(angle_min, angle_max, count):
    """inc of the spec, or None when the spec is refused."""
    vals = [float(F32(v)) for v in (angle_min, angle_max)]
    amin, amax = vals
    return float(F32((amax - amin) / float(count))) if count else None


def spec_valid(angle_min, angle_max, count, range_min, range_max, scan_time=0.1) -> bool:
    f = [float(F32(v)) for v in (angle_min, angle_max, range_min, range_max, scan_time)]
    if not all(math.isfinite(v) for v in f):
        return False
    amin, amax, rmin, rmax, _ = f
    if count == 0 or count > MAX_BEAMS:
        return False
    inc = float(F32((amax - amin) / float(count)))
    if not inc > 0.0 or inc > float(F32(math.pi / 2)):
        return False
    if amax - amin > 2.0 * math.pi * (1.0 + 2.0 ** -20):
        return False
    return 0.0 <= rmin < rmax


def edges(angle_min, count, inc) -> np.ndarray:
    """(count + 1, 2) float32: e_k = ((float)cos(phi_k), (float)sin(phi_k)), phi_k in fp64."""
    amin = float(F32(angle_min))
    out = np.empty((count + 1, 2), np.float32)
    for k in range(count + 1):
        phi = amin + float(k) * float(inc)
        out[k, 0] = math.cos(phi)
        out[k, 1] = math.sin(phi)
    return out


def _sides(E, x, y):
    """(n, count + 1) bool: cross_k >= 0, exact products of float32 values in fp64, one rounding."""
    ex = E[:, 0].astype(np.float64)[None, :]
    ey = E[:, 1].astype(np.float64)[None, :]
    return (ex * y.astype(np.float64)[:, None] - ey * x.astype(np.float64)[:, None]) >= 0.0


def bin_rule(E, x, y, chunk: int = 2048) -> np.ndarray:
    """The rule by brute force: the smallest k in [0, count) with cross_k >= 0 and cross_k+1 < 0,
    else -1."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    out = np.full(len(x), -1, np.int64)
    for a in range(0, len(x), chunk):
        s = _sides(E, x[a:a + chunk], y[a:a + chunk])
        t = s[:, :-1] & ~s[:, 1:]
        has = t.any(axis=1)
        out[a:a + chunk] = np.where(has, np.argmax(t, axis=1), -1)
    return out


def _monotone(E) -> bool:
    e = E.astype(np.float64)
    return bool(np.all(e[:-1, 0] * e[1:, 1] - e[:-1, 1] * e[1:, 0] > 0.0))


def bin_fast(E, x, y, angle_min, inc) -> np.ndarray:
    """bin_rule, fast: an fp64 atan2 guess, the exact tests at guess - 1 .. guess + 2, bin 0 re-tested
    for a point found in the last bin (the wrap sliver), brute force for whatever the window leaves
    open and for every point of a spec whose rounded edges do not turn monotonically."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    count = len(E) - 1
    if len(x) == 0:
        return np.zeros(0, np.int64)
    if not _monotone(E):
        return bin_rule(E, x, y)
    th = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    rel = np.mod(th - float(F32(angle_min)), 2.0 * math.pi)
    g = np.clip(np.floor(rel / float(inc)).astype(np.int64), 0, count - 1)
    xd, yd = x.astype(np.float64), y.astype(np.float64)

    def side(k):
        kk = np.clip(k, 0, count)
        return E[kk, 0].astype(np.float64) * yd - E[kk, 1].astype(np.float64) * xd >= 0.0

    out = np.full(len(x), -1, np.int64)
    for d in (-1, 0, 1):  # candidates k = g + d
        k = g + d
        ok = (k >= 0) & (k < count) & (out < 0)
        hit = ok & side(k) & ~side(k + 1)
        out[hit] = k[hit]
    last = out == count - 1
    if count > 1 and last.any():
        zero = side(np.zeros(len(x), np.int64)) & ~side(np.ones(len(x), np.int64))
        out[last & zero] = 0
    # open points: outside every beam, or the guess was off by more than one step — the rule decides
    rest = np.flatnonzero(out < 0)
    if len(rest):
        out[rest] = bin_rule(E, x[rest], y[rest])
    return out


# (the points of a group — E1, E2, E5 on the scan's own points, E6, pose — are the fused grid's too:
# tests/fused_oracle.py holds the one composition)
from tests.fused_oracle import group_points  # noqa: E402,F401


def reduce_beams(count, k, r2, slot, idx, intens):
    """Per beam the smallest r2, ties to the smallest (slot, index): (ranges, intensities, beams hit)."""
    ranges = np.full(count, np.inf, np.float32)
    out_i = np.zeros(count, np.float32)
    m = k >= 0
    if not m.any():
        return ranges, out_i, 0
    k, r2, slot, idx, intens = k[m], r2[m], slot[m], idx[m], intens[m]
    order = np.lexsort((idx, slot, r2, k))
    ks = k[order]
    first = np.ones(len(ks), bool)
    first[1:] = ks[1:] != ks[:-1]
    win = order[first]
    ranges[k[win]] = np.sqrt(r2[win]).astype(np.float32)
    out_i[k[win]] = intens[win]
    return ranges, out_i, int(first.sum())


def merge_group(oracle, scans, p, spec, motion=None, pose2d=None, t0=None, fast=True):
    """The merged scan of one group: spec = dict(angle_min, angle_max, count, range_min, range_max)."""
    count = int(spec["count"])
    inc = spec_inc(spec["angle_min"], spec["angle_max"], count)
    E = edges(spec["angle_min"], count, inc)
    x, y, r2, slot, idx, intens = group_points(oracle, scans, p, motion, pose2d, t0)
    r = np.sqrt(r2).astype(np.float32)
    gate = (r >= F32(spec["range_min"])) & (r <= F32(spec["range_max"]))
    k = np.full(len(x), -1, np.int64)
    if gate.any():
        sel = np.flatnonzero(gate)
        k[sel] = bin_fast(E, x[sel], y[sel], spec["angle_min"], inc) if fast else bin_rule(E, x[sel], y[sel])
    return reduce_beams(count, k, r2, slot, idx, intens)
