"""Inputs for E17's tests (tests/test_estimate_cpu.py, tests/test_gpu_estimate.py), each with a regime check made
from tests/estimate_oracle.py alone: what the case is meant to reach is asserted on the oracle's numbers, never on
the code under test.  A case: ``poses`` (L, P, 4) float32 (L = 1: one list serves every group), ``w`` (G, P) uint32
or None (every weight 1), ``spec`` (xy_scale, gate_r2, gate_dot), ``center`` (G,) uint32 or None (pose 0)."""
import functools

import numpy as np

from tests import estimate_oracle as eo

F32 = np.float32
U32_MAX = 0xFFFFFFFF
EDGE_P = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4096]
TOP = 8388607.5 / 1024.0     # x whose product with 1024 is 2^23 - 0.5: rounds (ties to even) to 2^23, in range


def spec_of(s):
    from rplidar_ros2_driver_amd import abi
    return abi.PoseEstimate(s["xy_scale"], s["gate_r2"], s["gate_dot"])


def case_of(poses, w, spec, center):
    poses = np.ascontiguousarray(poses, F32)
    if poses.ndim == 2:
        poses = poses[None]
    G = len(w) if w is not None else (len(center) if center is not None else len(poses))
    return dict(poses=poses, w=None if w is None else np.ascontiguousarray(w, np.uint32), spec=dict(spec), G=G,
                center=None if center is None else np.ascontiguousarray(center, np.uint32))


def group_inputs(case, g):
    """-> (poses (P, 4), w (P,) or None, centre word) of group g"""
    poses = case["poses"][g if len(case["poses"]) > 1 else 0]
    return poses, None if case["w"] is None else case["w"][g], 0 if case["center"] is None else int(case["center"][g])


_WANT = {}


def want(case, key=None, writer=None):
    """the oracle's (G, 72) words; cached under `key` for the default writer (a reference is computed once)"""
    if key is not None and writer is None and key in _WANT:
        return _WANT[key]
    out = np.stack([eo.estimate(*group_inputs(case, g)[:2], case["spec"], group_inputs(case, g)[2], writer=writer)
                    for g in range(case["G"])])
    if key is not None and writer is None:
        _WANT[key] = out
    return out


def cloud(rng, P, spread=4000, near=0.5):
    """P poses on the quantum lattice: a share `near` within 200 quanta and 0.1 rad of (0, 0, heading 0.3), the others
    anywhere within `spread` quanta and at any heading"""
    close = rng.random(P) < near
    X = np.where(close, rng.integers(-200, 201, P), rng.integers(-spread, spread + 1, P))
    Y = np.where(close, rng.integers(-200, 201, P), rng.integers(-spread, spread + 1, P))
    th = np.where(close, 0.3 + rng.uniform(-0.1, 0.1, P), rng.uniform(-np.pi, np.pi, P))
    return np.stack([np.cos(th), np.sin(th), X / 1024.0, Y / 1024.0], axis=1).astype(F32), close


# ---- tile edges: every centre of the issue as a group of one call ----------------------------------------------------------------
def edge_case(P):
    rng = np.random.default_rng(1700 + P)
    poses, close = cloud(rng, P)
    centers = sorted({min(c, P - 1) for c in (0, 1023, 1024, P - 1)})
    for c in centers:                       # a centre is a near pose; its neighbour in the list a far one
        poses[c] = [np.cos(0.3), np.sin(0.3), 0.0, 0.0]
        if P > 1:
            far = c + 1 if c + 1 < P and c + 1 not in centers else c - 1
            if far not in centers:
                poses[far] = [-1.0, 0.0, 3.0, 3.0]
    if P == 2:                              # both poses are centres: apart, each alone in its gate
        poses[1] = [-1.0, 0.0, 3.0, 3.0]
    w = rng.integers(0, 1 << 32, (len(centers), P), dtype=np.uint64).astype(np.uint32)
    w[:, rng.random(P) < 0.1] = 0
    if P == 2:
        w[:] = np.maximum(w, 1)
    for g, c in enumerate(centers):
        w[g, c] = max(int(w[g, c]), 1)
    return case_of(poses, w, eo.DEFAULT, np.array(centers, np.uint32))


def edge_regime(case, res):
    P = case["poses"].shape[1]
    for g in range(case["G"]):
        r = res[g]
        assert r[1] == case["center"][g] and r[0] & 0xD == 0                   # both sets have weight
        assert (r[4] < r[2] and r[8:40].tobytes() != r[40:72].tobytes()) or P == 1   # and differ (P = 1 cannot)


# ---- quantisation ------------------------------------------------------------------------------------------------------------
def quant_case(xy_scale):
    rng = np.random.default_rng(1701)
    sc = F32(xy_scale)
    rows = []
    base = np.array([0.5, -0.25, 1.0, -2.0], F32)

    def put(k, v):
        p = base.copy()
        p[k] = v
        rows.append(p)

    ties = [0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 1000.5, 1001.5, -1000.5, -1001.5, 4194303.5, -4194304.5]
    for t in ties:                                                  # k + 0.5, even and odd k, both signs
        for k in (2, 3):
            put(k, F32(t) / F32(1024.0))                             # (exact for 1024; rounds for another scale)
        for k in (0, 1):
            put(k, F32(t) / F32(1048576.0))
    for sgn in (1.0, -1.0):
        for k in (2, 3):
            put(k, F32(sgn * TOP))                                   # -> +-2^23, in range
            put(k, F32(sgn * 8192.0))                                # -> the product is +-2^23: out
            put(k, np.nextafter(F32(sgn * 8192.0), F32(0)))
        for k in (0, 1):
            put(k, np.nextafter(F32(sgn * 8.0), F32(0)))             # |c| just under 8: 2^23 - 0.5 -> 2^23, in range
            put(k, F32(sgn * 8.0))                                   # at 8: out
    for k in range(4):
        for v in (-0.0, 1e-45, -1e-45, 1e-39, np.nan, np.inf, -np.inf, 3.0e38, -3.0e38):
            put(k, F32(v))
    nan_payload = np.array([0x7FA00001, 0xFFC12345], np.uint32).view(F32)
    for k in range(4):
        put(k, nan_payload[k % 2])
    for v in (0.0015, 0.0025, -0.0035, 1.2345678, -7.654321, 8388.607, 8388.608, -8388.6075, 8191.9995, 8000.0005):
        put(2, F32(v))                                               # the product with 1000 rounds
        put(3, F32(-v))
    poses = np.array(rows, F32)
    poses = np.concatenate([base[None], poses])                      # the centre: an ordinary pose
    w = rng.integers(1, 1 << 32, (1, len(poses)), dtype=np.uint64).astype(np.uint32)
    return case_of(poses, w, dict(eo.OPEN, xy_scale=float(sc)), None)


def quant_regime(case):
    q, inr, t = eo.quantise(case["poses"][0], case["spec"]["xy_scale"])
    tt = t[inr].astype(np.float64)
    half = np.abs(tt - np.floor(tt) - 0.5) == 0
    fl = np.floor(tt[half]).astype(np.int64)
    assert ((fl % 2 == 0) & (fl >= 0)).any() and ((fl % 2 == 1) & (fl >= 0)).any()      # ties, even and odd, both signs
    assert ((fl % 2 == 0) & (fl < 0)).any() and ((fl % 2 == 1) & (fl < 0)).any()
    assert (q[inr] == 1 << 23).any() and (q[inr] == -(1 << 23)).any()                     # the ends of the range
    with np.errstate(all="ignore"):
        out = t[~inr]
        assert np.isnan(out).any(0).all() and np.isposinf(out).any(0).all() and np.isneginf(out).any(0).all()
        assert (np.abs(out) == F32(8388608.0)).any(0).all()                               # at the limit, every entry
    assert inr[0] and inr.sum() > 50 and (~inr).sum() > 20
    if case["spec"]["xy_scale"] != 1024.0:   # some product is not exact: the float32 rounding is part of the rule
        exact = case["poses"][0][inr, 2].astype(np.float64) * case["spec"]["xy_scale"]
        assert (exact != t[inr, 0].astype(np.float64)).any()


# ---- gate borders ------------------------------------------------------------------------------------------------------------
GATE_KINDS = ["borders", "r2_zero", "open", "centre_out", "centre_word"]


def _lattice(X, Y, C, S):
    return [C / 1048576.0, S / 1048576.0, X / 1024.0, Y / 1024.0]


def gate_case(kind):
    rng = np.random.default_rng(1702)
    cx, cy = 100, -50
    rows = [_lattice(cx, cy, 1 << 20, 0)]                                        # pose 0: the centre
    spec = dict(xy_scale=1024.0, gate_r2=25, gate_dot=1000 << 20)
    for dx, dy in [(3, 4), (-4, 3), (5, 0), (0, -5), (5, 1), (-1, 5), (4, 4), (0, 0), (1, 0), (3, 3), (6, 0)]:
        rows.append(_lattice(cx + dx, cy + dy, 1 << 20, 0))                      # r2 = 25 in, 26 and beyond out
    for C, S in [(1000, 0), (999, 0), (1000, 77), (999, 900000), (1001, 0), (-1000, 0), (0, 1 << 20)]:
        rows.append(_lattice(cx, cy, C, S))                                      # dot = gate_dot in, one below out
    poses = np.array(rows, F32)
    center = None
    if kind == "r2_zero":
        spec["gate_r2"] = 0
    elif kind == "open":
        spec = dict(eo.OPEN)
    elif kind == "centre_out":                                                   # the open gate, and still empty
        spec = dict(eo.OPEN)
        poses[0, 2] = np.nan
    elif kind == "centre_word":                                                  # a word >= P: the last pose
        center = np.array([U32_MAX], np.uint32)
        poses = np.concatenate([poses, np.array([_lattice(cx, cy, 1 << 20, 0)], F32)])
    w = rng.integers(1, 1 << 32, (1, len(poses)), dtype=np.uint64).astype(np.uint32)
    return case_of(poses, w, spec, center)


def gate_regime(case, kind, res):
    r = res[0]
    q, inr, _ = eo.quantise(case["poses"][0], 1024.0)
    if kind in ("borders", "centre_word"):
        qc = int(r[1])
        d = q[:, :2] - q[qc, :2]
        r2 = (d * d).sum(1)
        dot = q[:, 2] * q[qc, 2] + q[:, 3] * q[qc, 3]
        assert (r2 == 25).sum() >= 4 and (r2 == 26).sum() >= 2                   # at the border and one beyond
        assert (dot == 1000 << 20).sum() >= 1 and (dot == (1000 << 20) - (1 << 20)).sum() >= 1
        gate = eo.gate_of(q, inr, qc, case["spec"])
        assert gate[r2 == 25].any() and not gate[r2 == 26].any() and gate[(dot == 1000 << 20) & (r2 == 0)].all()
        assert not gate[dot < 1000 << 20].any() and 2 <= r[4] < r[2]
    if kind == "centre_word":
        assert r[1] == case["poses"].shape[1] - 1 and case["center"][0] >= case["poses"].shape[1]
    if kind == "r2_zero":
        assert 2 <= r[4] < 10
    if kind == "open":
        assert r[8:40].tobytes() == r[40:72].tobytes() and r[4] == r[2] and r[5] == r[3]
    if kind == "centre_out":
        assert r[0] == 1 | 2 | 8 and r[4] == 0 and r[5] == 0 and not r[40:72].any() and r[2] == len(q) - 1


# ---- extremes ----------------------------------------------------------------------------------------------------------------
def extreme_case(P, cancel=False):
    poses = np.zeros((P, 4), F32)
    poses[:, 0] = 1.0
    poses[:, 2] = TOP
    poses[:, 3] = -TOP
    if cancel:                               # mixed signs: the first moments of x cancel, those of y do not
        poses[1::2, 2] = -TOP
        poses = poses[:P - (P % 2)]
    w = np.full((1, len(poses)), U32_MAX, np.uint32)
    return case_of(poses, w, eo.OPEN, None)


def extreme_regime(case, res, cancel=False):
    P = case["poses"].shape[1]
    s = eo.sums_of_result(res[0], 0)
    assert s[0] == P * U32_MAX and s[5] == P * U32_MAX << 46 and s[5] > 1 << 64      # some sum exceeds 2^64
    assert s[2] == -(P * U32_MAX << 23) and res[0][8 + 8 + 2] >> 31 and res[0][8 + 8 + 3] == U32_MAX   # negative
    assert s[1] == (0 if cancel else P * U32_MAX << 23) and (s[6] == 0 if cancel else s[6] == -s[5])
    assert res[0][0] == 0 and res[0][8:40].tobytes() == res[0][40:72].tobytes()


# ---- groups ------------------------------------------------------------------------------------------------------------------
def groups_case(ppg, G=101, P=1100):
    rng = np.random.default_rng(1703 + ppg)
    L = G if ppg else 1
    poses = np.stack([cloud(rng, P)[0] for _ in range(L)])
    center = rng.integers(0, P + 50, G).astype(np.uint32)          # (some words beyond the list)
    for g in range(G):
        poses[g if ppg else 0][min(int(center[g]), P - 1)] = [np.cos(0.3), np.sin(0.3), 0.0, 0.0]
    w = rng.integers(0, 1 << 32, (G, P), dtype=np.uint64).astype(np.uint32)
    w[rng.random((G, P)) < 0.05] = 0
    dead = min(7, G - 1)
    w[dead] = 0                                                    # a group without weight
    poses[dead if ppg else 0][5] = [np.nan, 0, 0, 0]
    return case_of(poses, w, eo.DEFAULT, center)


def groups_regime(case, res):
    P = case["poses"].shape[1]
    assert (case["center"] >= P).any() and len({bytes(r) for r in res}) == case["G"]
    assert res[7][0] & 0xC == 0xC and res[7][3] == 0 and (res[:, 0] & 2).any() and (res[:7, 0] & 0xD == 0).all()
    assert ((res[:, 4] >= 2) & (res[:, 4] < res[:, 2])).sum() >= case["G"] - 1


@functools.lru_cache(None)
def big_case():
    return extreme_case(1 << 20)
