"""Inputs for E22 (tests/cast_oracle.py, rplgpu_cast_ranges_dev): seeded grids, pose lists, beam tables, measured scans
and byte tables, each case with a REGIME that the oracle's own answer must satisfy before anything is compared with it
(`regime`), so that a case cannot quietly stop exercising what it is there for.

A case is a dict: spec, G, lists (1 or G arrays (P, 4)), grids (1 or G arrays (height, width) int8), beams (A, 2),
measured ((G, stride) float32 or None), first, step, table ((2K + 2,) uint8 or None), ranges (bool: range words wanted),
regime (dict)."""
from __future__ import annotations

import numpy as np

from tests import cast_oracle as co

F32 = np.float32
_WANT = {}


def fan(A: int, phase: float = 0.5) -> np.ndarray:
    """A beam directions evenly over the circle, (A, 2) float32."""
    a = 2.0 * np.pi * (np.arange(A) + phase) / A
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(F32)


def room(rng, W: int, H: int, walls=(100,), blobs: int = 6, unknown: int = 3) -> np.ndarray:
    """Free cells, walls along the left and the bottom edge only (so that rays also LEAVE), a few blocks whose bytes
    are drawn from `walls`, a few patches of unknown."""
    g = np.zeros((H, W), np.int8)
    if W >= 3 and H >= 3:
        g[0, :] = walls[0]
        g[:, 0] = walls[0]
        for k in range(blobs):
            w, h = int(rng.integers(1, max(2, W // 6))), int(rng.integers(1, max(2, H // 6)))
            x, y = int(rng.integers(1, W - w + 1)), int(rng.integers(1, H - h + 1))
            g[y:y + h, x:x + w] = walls[k % len(walls)]
        for _ in range(unknown):
            w, h = int(rng.integers(1, max(2, W // 5))), int(rng.integers(1, max(2, H // 5)))
            x, y = int(rng.integers(1, W - w + 1)), int(rng.integers(1, H - h + 1))
            g[y:y + h, x:x + w] = -1
    return g


def poses_in(rng, s, P: int, margin: float = 0.0, scale=(1.0,)) -> np.ndarray:
    """P poses over the grid's extent (grown by `margin` of it on every side), any heading; (c, s) scaled by an entry of
    `scale` in turn (any matrix [c -s; s c] is defined: a small scale puts the end cell inside the grid)."""
    w, h = s["width"] * s["resolution"], s["height"] * s["resolution"]
    x = s["origin_x"] + rng.uniform(-margin * w, (1 + margin) * w, P)
    y = s["origin_y"] + rng.uniform(-margin * h, (1 + margin) * h, P)
    th = rng.uniform(-np.pi, np.pi, P)
    k = np.array(scale)[np.arange(P) % len(scale)]
    return np.stack([k * np.cos(th), k * np.sin(th), x, y], axis=1).astype(F32)


def byte_table(K: int, zeros: bool = False) -> np.ndarray:
    """2K + 2 bytes: a peak at 0 falling off to a floor (or to 0 with `zeros`), the last entry 77."""
    j = np.arange(-K, K + 1)
    t = np.maximum(np.round(250.0 * np.exp(-0.5 * (j / 3.0) ** 2)), 0 if zeros else 3)
    t[j < -8] = 0 if zeros else 9                                   # (short readings: another floor)
    if zeros:
        t[np.abs(j) > 2] = 0
    return np.concatenate([t, [77]]).astype(np.uint8)


def scan_of(rng, s, pose, beams, grid, first, step, pad, nan_every=0, inf_every=0) -> np.ndarray:
    """A measured scan as the pose `pose` would see it (the oracle's lock-step ranges in metres, with noise of a few
    cells), laid out at first + a * step; the entries between are NaN; some beams +inf or NaN."""
    A = len(beams)
    words, _ = co.cast_lockstep(s, pose[None, :], beams, grid)
    z = np.array([co.range_m(w, s["resolution"]) for w in words[0]])
    z = np.where(np.isfinite(z), np.maximum(z + rng.normal(0.0, 2.5 * s["resolution"], A), 0.0), np.inf)
    if inf_every:
        z[::inf_every] = np.inf
    if nan_every:
        z[1::nan_every] = np.nan
    out = np.full(first + (A - 1) * step + 1 + pad, np.nan, F32)
    out[first + step * np.arange(A)] = z.astype(F32)
    return out


def make(seed, W, H, P, A, N=240, G=1, own_lists=False, own_grids=False, meas=True, step=1, first=0, hit_lo=100,
         unknown_stops=1, K=40, ranges=True, res=0.05, origin=(-1.0, -0.7), walls=(100,), margin=0.0, scale=(1.0,),
         zeros=False, nan_every=0, inf_every=0, extra=None, regime=None, empty=False, beams=None) -> dict:
    rng = np.random.default_rng(seed)
    s = co.spec(origin_x=origin[0], origin_y=origin[1], resolution=res, width=W, height=H, max_steps=N, hit_lo=hit_lo,
                unknown_stops=unknown_stops, table_half=K)
    grids = [np.zeros((H, W), np.int8) if empty else room(rng, W, H, walls) for _ in range(G if own_grids else 1)]
    lists = []
    for _ in range(G if own_lists else 1):
        p = poses_in(rng, s, P, margin, scale)
        if extra is not None:
            p[len(p) - len(extra):] = extra
        lists.append(p)
    beams = fan(A) if beams is None else np.array(beams, F32)
    case = dict(spec=s, G=G, lists=lists, grids=grids, beams=beams, measured=None, first=first, step=step, table=None,
                ranges=ranges, regime=regime or {})
    if meas:
        case["table"] = byte_table(K, zeros)
        case["measured"] = np.stack([scan_of(rng, s, lists[g % len(lists)][0], beams, grids[g % len(grids)], first, step,
                                             3, nan_every, inf_every) for g in range(G)])
    return case


def want(case, name, writer=2):
    """The oracle's answer, one dict per group (cast_oracle.cast_group), computed once per (name, writer)."""
    key = (name, writer)
    if key not in _WANT:
        out = []
        for g in range(case["G"]):
            out.append(co.cast_group(case["spec"], case["lists"][g % len(case["lists"])], case["beams"],
                                     case["grids"][g % len(case["grids"])],
                                     None if case["measured"] is None else case["measured"][g], case["first"],
                                     case["step"], case["table"], writer))
        _WANT[key] = out
    return _WANT[key]


def regime(case, want_):
    """The case's REGIME on the oracle's answer alone: kinds (the kinds that occur, exactly), dropped (True: at least one
    dropped ray, False: none), zero_w (weights of 0 occur), far (a walk of at least that many steps occurs)."""
    r = case["regime"]
    cast = np.sum([w["cast"].astype(np.int64) for w in want_], axis=0)
    rays = case["G"] * len(case["lists"][0]) * len(case["beams"])
    assert int(cast[:5].sum()) == rays
    if "kinds" in r:
        assert {k for k in range(4) if cast[k]} == set(r["kinds"]), cast[:5].tolist()
    if "dropped" in r:
        assert (cast[4] > 0) == r["dropped"], cast[:5].tolist()
    if r.get("zero_w"):
        assert any((w["weights"] == 0).any() for w in want_) and any((w["weights"] != 0).any() for w in want_)
    if r.get("fused"):                                           # an FMA in the composition would be seen
        s, grid, beam = case["spec"], case["grids"][0], case["beams"][0]
        other = [co.ray(s, p, beam, grid, fused=True)[0] for p in case["lists"][0]]
        differ = sum(int(a) != int(b) for a, b in zip(other, want_[0]["ranges"][:, 0]))
        assert 3 <= differ <= len(other) - 3, differ
    if "far" in r:
        assert max(int(w["steps"].max()) for w in want_) >= r["far"]
    if case["measured"] is not None and not r.get("zero_w"):
        assert all(int(w["result"][0]) > 0 for w in want_)
    if case["G"] > 1 and (len(case["lists"]) > 1 or len(case["grids"]) > 1 or case["measured"] is not None):
        assert len({w["ranges"].tobytes() + (w["weights"].tobytes() if w["weights"] is not None else b"")
                    for w in want_}) == case["G"]                  # the groups differ


def fused_case() -> dict:
    """Tells the rule's composition (each product rounded, then the difference) from a fused multiply-add: one pose
    heading and one beam whose composition points along +y, so that dc is nothing but rounding (0 by the rule, the
    products' rounding error when fused); 64 poses in column 4 whose tx are float32 values 8 ulps apart next to the edge
    towards which the fused dc points.  For the nearest of them a fused dc puts the end cell into the next column, the
    walk changes column half way up, and that column is a wall: HIT against a ray that runs up column 4."""
    s = co.spec(origin_x=0.0, origin_y=0.0, resolution=1.0, width=9, height=2100, max_steps=8192, table_half=1)
    rng = np.random.default_rng(77)
    rm, best = F32(8192.0), None
    for _ in range(400):
        th = rng.uniform(0.3, 1.2)
        pose = np.array([0.5 * np.cos(th), 0.5 * np.sin(th)], F32)
        beam = np.array([[np.cos(np.pi / 2 - th), np.sin(np.pi / 2 - th)]], F32)
        plain = F32(F32(pose[0] * beam[0, 0]) - F32(pose[1] * beam[0, 1])) * rm
        fused = co._fused(pose[0], beam[0, 0], -F32(pose[1] * beam[0, 1])) * rm
        if plain == 0 and (best is None or abs(float(fused)) > abs(float(best[2]))):
            best = (pose, beam, fused)
    pose, beam, fused = best
    up = float(fused) > 0
    grid = np.zeros((2100, 9), np.int8)
    grid[:, 5 if up else 3] = 100
    tx = np.nextafter(F32(5.0), F32(0.0)) if up else F32(4.0)
    poses = np.zeros((64, 4), F32)
    poses[:, 0], poses[:, 1], poses[:, 3] = pose[0], pose[1], 0.5
    for k in range(64):
        poses[k, 2] = tx
        for _ in range(8):
            tx = np.nextafter(tx, F32(4.5))
    z = np.full(4, 300.0, F32)
    return dict(spec=s, G=1, lists=[poses], grids=[grid], beams=beam, measured=z[None, :], first=0, step=1,
                table=np.array([1, 200, 3, 77], np.uint8), ranges=True, regime=dict(fused=True, dropped=False))


ALL = (co.HIT, co.UNKNOWN, co.LEFT, co.NO_STOP)
NAN = float("nan")
# poses that have no start cell (NaN, a position beyond 2^20 cells, Inf), no end cell (a huge scale), and the zero
# matrix (end cell = start cell)
ODD = np.array([[NAN, 0.0, 0.0, 0.0], [1.0, 0.0, 1e9, 0.0], [1.0, 0.0, 0.0, float("inf")], [1e30, 1e30, 0.0, 0.0],
                [0.0, 0.0, 0.3, 0.3]], F32)

CASES = {
    # the smallest grid: every ray starts in its only cell (free) or outside it
    "p1": lambda: make(1, 1, 1, 1, 64, N=1, K=0, origin=(0.0, 0.0), extra=np.array([[1, 0, 0.02, 0.03]], F32),
                       regime=dict(kinds=(co.LEFT,), dropped=False)),
    "p63": lambda: make(2, 37, 29, 63, 2, N=2, K=1, margin=0.1,
                        regime=dict(kinds=ALL, dropped=False)),
    "p64": lambda: make(3, 37, 29, 64, 63, K=40, scale=(1.0, 0.02), nan_every=5, inf_every=7,
                        regime=dict(kinds=ALL, dropped=False)),
    "p65": lambda: make(4, 130, 67, 65, 65, hit_lo=1, unknown_stops=0, step=7, first=2, walls=(100, 1, 50),
                        scale=(1.0, 0.1), regime=dict(kinds=(co.HIT, co.LEFT, co.NO_STOP), dropped=False)),
    "p1023": lambda: make(5, 130, 67, 1023, 1, hit_lo=127, walls=(127, 126, 100), scale=(1.0, 0.2), zeros=True,
                          regime=dict(kinds=ALL, dropped=False, zero_w=True)),
    "p1024": lambda: make(6, 4096, 3, 1024, 2, ranges=False, origin=(-100.0, 0.0), scale=(1.0, 0.05),
                          regime=dict(kinds=ALL, dropped=False)),
    "p1025": lambda: make(7, 3, 4096, 1025, 2, meas=False, origin=(0.0, -100.0), scale=(1.0, 0.05),
                          regime=dict(kinds=ALL, dropped=False)),
    "p2049": lambda: make(8, 640, 640, 2049, 3, K=4096, origin=(-16.0, -16.0), regime=dict(kinds=ALL, dropped=False)),
    "a360": lambda: make(9, 640, 640, 5, 360, K=40, origin=(-16.0, -16.0), step=7, inf_every=9,
                         regime=dict(kinds=ALL, dropped=False)),
    # N = 8192 on a few rays of a grid 4096 cells long: walks of thousands of steps, D2 above 2^23
    "long": lambda: make(10, 4096, 3, 4, 4, N=8192, origin=(0.0, 0.0), empty=True, K=1,
                         beams=[(1, 0), (-1, 0), (1, 1e-5), (0, 1)],
                         extra=np.array([[1, 0, 0.01, 0.07], [-1, 0, 204.79, 0.07]], F32),
                         regime=dict(kinds=(co.LEFT,), dropped=False, far=4096)),
    "empty": lambda: make(11, 640, 640, 300, 7, N=30, origin=(-16.0, -16.0), empty=True, margin=-0.1,
                          regime=dict(kinds=(co.NO_STOP,), dropped=False)),
    "odd": lambda: make(12, 37, 29, 40, 9, extra=ODD, nan_every=4, regime=dict(dropped=True)),
    "zeros": lambda: make(13, 130, 67, 200, 5, zeros=True, K=4, regime=dict(zero_w=True, dropped=False)),
    "groups_own": lambda: make(14, 37, 29, 130, 7, G=3, own_lists=True, own_grids=True, scale=(1.0, 0.05),
                               regime=dict(kinds=ALL, dropped=False)),
    "groups_shared": lambda: make(15, 37, 29, 130, 7, G=3, scale=(1.0, 0.05), step=7,
                                  regime=dict(kinds=ALL, dropped=False)),
    "groups_ranges": lambda: make(16, 37, 29, 70, 3, G=3, own_lists=True, meas=False, scale=(1.0, 0.05),
                                  regime=dict(kinds=ALL, dropped=False)),
    "hit1": lambda: make(17, 37, 29, 100, 4, hit_lo=1, walls=(1, 100), regime=dict(dropped=False)),
    "fused": fused_case,
    "hit127": lambda: make(18, 37, 29, 100, 4, hit_lo=127, walls=(126, 127), unknown_stops=0,
                           regime=dict(kinds=(co.HIT, co.LEFT), dropped=False)),
}
_BUILT = {}


def case(name: str) -> dict:
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]
