"""Inputs of the E27 tests (tests/test_rollout_cpu.py, tests/test_gpu_rollout.py) and, per family, a ``*_regime``
function that asserts from tests/rollout_oracle.py ALONE that the inputs are in the regime their name claims (blocked
exactly at step T, only the last footprint point blocks, a tie that spans two tiles, ...).  Nothing here loads the
library.  A case is a dict: name, spec, start (4,), delta (K, 4) arcs or (K, T, 4) per step, footprint (F, 2), grid
(H, W) int8, potential (H, W) uint32 or None.  No grid is larger than 130 x 70."""
import functools
import math

import numpy as np

from tests import rollout_oracle as ro

U = ro.UNREACHED
TILE, CHUNK = ro.TILE, 32   # candidates a workgroup takes; steps a pass over its LDS takes
W, H, RES = 128, 64, 0.1
ORIGIN = (-2.0, -3.2)       # x in [-2, 10.8), y in [-3.2, 3.2)
MAX_CAP = 0xFFFF0000


def base_spec(**kw):
    return ro.spec(**dict(dict(origin_x=ORIGIN[0], origin_y=ORIGIN[1], resolution=RES, width=W, height=H), **kw))


def centre_of(cx, cy):
    """The middle of cell (cx, cy) of the base grid."""
    return ORIGIN[0] + (cx + 0.5) * RES, ORIGIN[1] + (cy + 0.5) * RES


def pose(x, y, th=0.0):
    return np.array([math.cos(th), math.sin(th), x, y], np.float32)


def arc_deltas(v, w, dt):
    """The deltas of constant (v, w) held for dt, in fp64, rounded once (this file's own formula)."""
    out = np.zeros((len(v), 4), np.float32)
    for i, (vi, wi) in enumerate(zip(v, w)):
        th = wi * dt
        if abs(th) < 1e-9:
            out[i] = [1.0, 0.0, vi * dt, 0.0]
        else:
            out[i] = [math.cos(th), math.sin(th), vi * math.sin(th) / wi, vi * (1.0 - math.cos(th)) / wi]
    return out


def free_grid(value=0):
    return np.full((H, W), value, np.int8)


def rough_grid(seed):
    """Costs 0 .. 60 everywhere, a few lethal blocks and an unknown patch."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 61, (H, W)).astype(np.int8)
    for _ in range(6):
        x, y = int(rng.integers(20, W - 8)), int(rng.integers(0, H - 8))
        g[y:y + int(rng.integers(2, 8)), x:x + int(rng.integers(2, 8))] = 100
    g[5:12, 60:70] = -1
    return g


def slope_field(grid, goal=(120, 32), lethal=99):
    """A field-like potential: 50 per cell of Chebyshev distance plus 7 per cell of the other axis; UNREACHED on
    lethal cells (not a solution of E26's equation: E27 reads any words)."""
    cy, cx = np.mgrid[0:grid.shape[0], 0:grid.shape[1]]
    dx, dy = np.abs(cx - goal[0]), np.abs(cy - goal[1])
    d = (50 * np.maximum(dx, dy) + 7 * np.minimum(dx, dy)).astype(np.uint32)
    d[grid >= lethal] = U
    return d


def ring(F, radius=0.25):
    """F footprint points on a circle; F = 1 is the centre."""
    if F == 1:
        return np.zeros((1, 2), np.float32)
    a = np.arange(F) * (2.0 * math.pi / F)
    return np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1).astype(np.float32)


_WANT = {}


def want(c):
    """(out, end_poses, result) of a case by the vectorised writer, computed once per name and shared."""
    if c["name"] not in _WANT:
        _WANT[c["name"]] = ro.sweep(c["spec"], c["start"], c["delta"], c["footprint"], c["grid"], c["potential"])
    return _WANT[c["name"]]


def case(name, spec, start, delta, footprint, grid, potential=None):
    return dict(name=name, spec=spec, start=np.asarray(start, np.float32), delta=np.asarray(delta, np.float32),
                footprint=np.asarray(footprint, np.float32).reshape(-1, 2), grid=grid, potential=potential)


# ---- shapes at the kernel's edges ----------------------------------------------------------------------------------------------
# (K, T, F, per_step): K = 1, tile - 1, tile, tile + 1, 3 tiles + 5; T = 1, 2, one chunk - 1 / + 0 / + 1, two chunks +
# 1, 256; F = 1, 2, 63, 64
SHAPES = [(1, 1, 1, 0), (TILE - 1, 2, 2, 1), (TILE, CHUNK - 1, 63, 0), (TILE + 1, CHUNK, 64, 1),
          (3 * TILE + 5, CHUNK + 1, 2, 1), (3 * TILE + 5, CHUNK, 1, 0), (5, 256, 1, 0), (TILE + 1, 256, 2, 1),
          (2 * TILE, 2 * CHUNK + 1, 3, 1), (TILE + 1, CHUNK + 1, 64, 0)]


@functools.lru_cache(maxsize=None)
def shape_case(K, T, F, per_step, seed=0):
    rng = np.random.default_rng(1000 * K + 10 * T + F + per_step + 7919 * seed)
    grid = rough_grid(seed + 3)
    dist = 9.0                                   # metres an unblocked candidate covers: most of the grid's length
    v = rng.uniform(0.3, 1.0, K) * dist
    w = rng.uniform(-1.0, 1.0, K) * 0.8
    arcs = arc_deltas(v, w, 1.0 / T)
    if per_step:
        noise = rng.normal(0.0, 0.02, (K, T, 4)).astype(np.float32) * np.float32(1.0 / math.sqrt(T))
        delta = arcs[:, None, :] + noise
    else:
        delta = arcs
    s = base_spec(steps=T, min_steps=max(1, 7 * T // 8), a_end=3, a_min=2, a_sum=5, a_max=11)
    start = pose(*centre_of(6, 30 + seed), 0.05 * seed)
    return case(f"shape_{K}_{T}_{F}_{per_step}_{seed}", s, start, delta, ring(F), grid, slope_field(grid))


def shapes_regime():
    """Over the shapes: blocked and unblocked candidates, blocks in the first, a middle and the last chunk, admissible
    and inadmissible ones, END_UNREACHED absent and present somewhere."""
    seen = set()
    for sh in SHAPES:
        c = shape_case(*sh)
        out, _, res = want(c)
        T = c["spec"]["steps"]
        assert out.shape == (sh[0], 8) and (out[:, 0] <= T).all()
        for n, fl in out[:, :2]:
            seen.add("blocked" if fl & ro.BLOCKED else "free")
            seen.add("adm" if fl & ro.ADMISSIBLE else "inadm")
            if fl & ro.BLOCKED and T > CHUNK:
                seen.add("first_chunk" if n < CHUNK else "last_chunk" if n >= (T - 1) // CHUNK * CHUNK else "mid_chunk")
        assert res[0] == (out[:, 1] & ro.ADMISSIBLE != 0).sum()
    assert seen >= {"blocked", "free", "adm", "inadm", "first_chunk", "mid_chunk", "last_chunk"}, seen


def group_cases(K=TILE + 3, T=CHUNK + 2, F=5, per_step=1, G=3):
    """G cases of one shape and spec (the groups of one call)."""
    return [shape_case(K, T, F, per_step, seed=g) for g in range(G)]


# ---- blocking -------------------------------------------------------------------------------------------------------------------
def _line(T, cells_per_step=1.0, K=1):
    """K equal candidates that move cells_per_step cells along +x per step."""
    return np.tile(np.array([[1.0, 0.0, cells_per_step * RES, 0.0]], np.float32), (K, 1))


@functools.lru_cache(maxsize=None)
def blocking_cases():
    out = {}
    T = 8
    s = base_spec(steps=T)
    wall = free_grid(10)
    wall[:, 20] = 100
    # the start in cell (19, 30): pose 1 is in the wall
    out["at_step_1"] = case("block_at_step_1", s, pose(*centre_of(19, 30)), _line(T), ring(1), wall)
    # the start in cell (12, 30): pose T is the first in the wall
    out["at_step_T"] = case("block_at_step_T", s, pose(*centre_of(12, 30)), _line(T), ring(1), wall)
    # five points, the last 0.52 m ahead: it alone reaches the wall, at pose 3 (cell 20 = 12 + 3 + 5)
    fp = np.array([[0, 0], [-0.1, 0.1], [-0.1, -0.1], [0.0, -0.2], [0.52, 0.0]], np.float32)
    out["last_point"] = case("block_last_point", s, pose(*centre_of(12, 30)), _line(T), fp, wall)
    out["last_point_without"] = case("block_last_point_without", s, pose(*centre_of(12, 30)), _line(T), fp[:-1], wall)
    # off each edge: three steps inside, then cell -1 or cell = width / height
    for name, (cx, cy, th) in dict(east=(W - 4, 30, 0.0), west=(3, 30, math.pi), north=(40, H - 4, math.pi / 2),
                                   south=(40, 3, -math.pi / 2)).items():
        st = np.array([round(math.cos(th)), round(math.sin(th)), *centre_of(cx, cy)], np.float32)
        out["edge_" + name] = case("block_edge_" + name, s, st, _line(T), ring(1), free_grid(7))
    # values that are not finite: a NaN start; an Inf in a delta's dx (candidate 1) and in its dc (candidate 2: Inf *
    # 0 makes NaN in the pose); candidate 0 is sound
    nan_start = pose(*centre_of(30, 30))
    nan_start[2] = np.nan
    out["nan_start"] = case("block_nan_start", s, nan_start, _line(T, K=2), ring(2), free_grid(7))
    d = _line(T, K=3)
    d[1, 2] = np.inf
    d[2, 0] = np.inf
    out["inf_delta"] = case("block_inf_delta", s, pose(*centre_of(30, 30)), d, ring(2), free_grid(7))
    # a per-step sequence that goes off range at step 5 only, by a magnitude (2^21 cells), and would be back at step 6
    seq = np.tile(_line(T)[:, None, :], (1, T, 1))
    seq[0, 4, 2] = 3.0e5
    seq[0, 5, 2] = -3.0e5
    out["far_step"] = case("block_far_step", s, pose(*centre_of(30, 30)), seq, ring(1), free_grid(7))
    # unknown cells ahead (cells 16 .. 18 of the row): a value below lethal is a cost, a value at lethal blocks
    unk = free_grid(5)
    unk[:, 16:19] = -1
    out["unknown_below"] = case("block_unknown_below", base_spec(steps=T, unknown_value=30, lethal=31),
                                pose(*centre_of(12, 30)), _line(T), ring(1), unk)
    out["unknown_at"] = case("block_unknown_at", base_spec(steps=T, unknown_value=31, lethal=31),
                             pose(*centre_of(12, 30)), _line(T), ring(1), unk)
    # lethal 1: any cost blocks; lethal 100: 99 is a cost, 100 blocks
    ramp = free_grid(0)
    ramp[:, 15] = 1
    out["lethal_1"] = case("block_lethal_1", base_spec(steps=T, lethal=1, unknown_value=0), pose(*centre_of(12, 30)),
                           _line(T), ring(1), ramp)
    top = free_grid(0)
    top[:, 15] = 99
    top[:, 18] = 100
    out["lethal_100"] = case("block_lethal_100", base_spec(steps=T, lethal=100), pose(*centre_of(12, 30)), _line(T),
                             ring(1), top)
    # min_steps 4 of 8 with the wall at pose 7 (candidate 0: admissible and BLOCKED) and at pose 3 (candidate 1, three
    # times the speed: blocked before min_steps)
    thick = free_grid(10)
    thick[:, 20:23] = 100
    d = np.concatenate([_line(T), _line(T, 3.0)])
    out["min_steps"] = case("block_min_steps", base_spec(steps=T, min_steps=4), pose(*centre_of(13, 30)), d, ring(1),
                            thick)
    return out


def blocking_regime():
    c = blocking_cases()
    o = lambda name: want(c[name])  # noqa: E731
    out, ends, res = o("at_step_1")
    assert out[0, :4].tolist() == [0, ro.BLOCKED, 0, 0] and ends[0].tobytes() == c["at_step_1"]["start"].tobytes()
    assert res.tolist() == [0, ro.NONE, 0xFFFFFFFF, 0xFFFFFFFF, 0, 1, 0, 1]
    out, _, _ = o("at_step_T")
    assert out[0, :4].tolist() == [7, ro.BLOCKED, 70, 10]          # blocked exactly at step T = 8
    out, _, _ = o("last_point")
    assert out[0, :2].tolist() == [2, ro.BLOCKED]                  # only point F - 1 blocks:
    assert o("last_point_without")[0][0, :2].tolist() == [7, ro.BLOCKED]
    for name in ("east", "west", "north", "south"):
        out, _, _ = o("edge_" + name)
        assert out[0, :4].tolist() == [3, ro.BLOCKED, 21, 7], name  # no CELL_RANGE: the cell exists, outside the grid
    out, ends, res = o("nan_start")
    assert (out[:, 0] == 0).all() and (out[:, 1] == ro.BLOCKED | ro.CELL_RANGE).all() and res[6] == 2
    assert ends.tobytes() == np.tile(c["nan_start"]["start"], (2, 1)).tobytes()
    out, ends, res = o("inf_delta")
    assert out[0, :2].tolist() == [8, ro.ADMISSIBLE] and (out[1:, 0] == 0).all()
    assert (out[1:, 1] == ro.BLOCKED | ro.CELL_RANGE).all() and res[5] == 2 and res[6] == 2
    out, ends, _ = o("far_step")
    assert out[0, :2].tolist() == [4, ro.BLOCKED | ro.CELL_RANGE]
    out, _, _ = o("unknown_below")
    assert out[0, :4].tolist() == [8, ro.ADMISSIBLE, 5 * 5 + 3 * 30, 30]
    assert o("unknown_at")[0][0, :4].tolist() == [3, ro.BLOCKED, 15, 5]
    assert o("lethal_1")[0][0, :4].tolist() == [2, ro.BLOCKED, 0, 0]
    assert o("lethal_100")[0][0, :4].tolist() == [5, ro.BLOCKED, 99, 99]
    out, _, res = o("min_steps")
    assert out[0, :2].tolist() == [6, ro.BLOCKED | ro.ADMISSIBLE] and out[1, :2].tolist() == [2, ro.BLOCKED]
    assert res[:2].tolist() == [1, 0]


# ---- D and the score ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field_cases():
    out = {}
    T = 8
    grid = free_grid(4)
    # the row of the walk: D falls to 5 at pose 4 (cell 16) and rises again
    dip = np.full((H, W), 9000, np.uint32)
    dip[30, 12:24] = [900, 800, 700, 600, 5, 650, 640, 630, 620, 610, 600, 590]
    s = base_spec(steps=T, a_end=2, a_min=3, a_sum=1, a_max=1)
    out["d_min_middle"] = case("field_d_min_middle", s, pose(*centre_of(12, 30)), _line(T), ring(1), grid, dip)
    # the last pose's cell is unreached, the one before is not
    hole = dip.copy()
    hole[30, 20] = U
    out["end_unreached"] = case("field_end_unreached", s, pose(*centre_of(12, 30)), _line(T), ring(1), grid, hole)
    # two points 0.5 m ahead and no (0, 0): the centre starts west of the grid (cells -4 .. 3) while the points are inside
    fp = np.array([[0.5, 0.03], [0.5, -0.03]], np.float32)
    st = pose(ORIGIN[0] - 3.5 * RES, centre_of(0, 30)[1])
    out["centre_outside"] = case("field_centre_outside", s, st, _line(T), fp, grid, dip)
    out["centre_outside_short"] = case("field_centre_outside_short", base_spec(steps=3), st, _line(3), fp, grid, dip)
    out["no_potential"] = case("field_no_potential", s, pose(*centre_of(12, 30)), _line(T), ring(1), grid, None)
    # all four scales at 65535 and D near RPLGPU_NAV_MAX_CAP: the score needs its high word
    high = np.full((H, W), MAX_CAP - 3, np.uint32)
    high[30, 20] = MAX_CAP
    big = base_spec(steps=T, a_end=65535, a_min=65535, a_sum=65535, a_max=65535)
    out["big_score"] = case("field_big_score", big, pose(*centre_of(12, 30)), _line(T, K=2), ring(1), free_grid(98),
                            high)
    return out


def field_regime():
    c = field_cases()
    o = lambda name: want(c[name])  # noqa: E731
    out, _, _ = o("d_min_middle")
    assert out[0].tolist() == [8, ro.ADMISSIBLE, 32, 4, 620, 5, 2 * 620 + 3 * 5 + 32 + 4, 0]
    out, _, res = o("end_unreached")
    assert out[0].tolist() == [8, ro.END_UNREACHED, 32, 4, U, 5, 0xFFFFFFFF, 0xFFFFFFFF] and res[7] == 1
    out, _, _ = o("centre_outside")
    assert out[0, :2].tolist() == [8, ro.ADMISSIBLE] and out[0, 4] == 9000   # poses 1 .. 3 have no D, 4 .. 8 do
    out, _, _ = o("centre_outside_short")
    assert out[0].tolist() == [3, ro.END_UNREACHED, 12, 4, U, U, 0xFFFFFFFF, 0xFFFFFFFF]
    out, _, _ = o("no_potential")
    assert out[0].tolist() == [8, ro.ADMISSIBLE, 32, 4, 0, 0, 32 + 4, 0]
    out, _, res = o("big_score")
    score = 65535 * (MAX_CAP + (MAX_CAP - 3) + 8 * 98 + 98)
    assert score >> 32 and score < 1 << 50
    assert out[0, 6:].tolist() == [score & 0xFFFFFFFF, score >> 32] and res[1:5].tolist() == [0, *out[0, 6:], 2]


# ---- ties and admissibility --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_case(K, winners, name, T=4):
    """K candidates along +x at speeds that cost more the higher k is, except the winners, which are equal and best."""
    grid = free_grid(0)
    grid[:, 40:] = np.minimum(np.arange(W - 40), 90).astype(np.int8)[None, :]   # dearer the further east
    d = _line(T, K=K)
    d[:, 2] = (0.8 + 0.0004 * np.arange(K)).astype(np.float32)   # further and dearer than the winners, every one
    for k in winners:
        d[k, 2] = 0.3
    pot = slope_field(grid, goal=(20, 30))     # the goal is behind: the further a candidate gets, the worse
    return case(name, base_spec(steps=T, a_end=1, a_sum=1), pose(*centre_of(24, 30)), d, ring(1), grid, pot)


def tie_cases():
    far = 256 * TILE   # the closing workgroup's second round over the tiles
    return dict(lanes=tie_case(TILE, (3, 17), "tie_lanes"), tiles=tie_case(3 * TILE + 5, (TILE - 1, TILE, 3 * TILE + 4),
                                                                            "tie_tiles"),
                waves=tie_case(far + 40, (40, 70 * TILE + 1, far + 3), "tie_waves", T=1))


def tie_regime():
    for name, c in tie_cases().items():
        out, _, res = want(c)
        K = len(out)
        winners = [k for k in range(K) if c["delta"][k, 2] == np.float32(0.3)]
        assert len(winners) >= 2 and (out[:, 1] == ro.ADMISSIBLE).all(), name
        score = out[:, 6].astype(np.uint64) + (out[:, 7].astype(np.uint64) << np.uint64(32))
        others = np.delete(score, winners)
        assert (score[winners] == score[winners[0]]).all() and (others > score[winners[0]]).all(), name
        assert res.tolist() == [K, winners[0], int(score[winners[0]]), 0, len(winners), 0, 0, 0], name
    c = tie_cases()
    assert [k // TILE for k in (TILE - 1, TILE, 3 * TILE + 4)] == [0, 1, 3]   # this tie spans three tiles
    assert len(c["waves"]["delta"]) > 256 * TILE                                # ... and this one two rounds of the close


@functools.lru_cache(maxsize=None)
def none_admissible_case():
    wall = free_grid(3)
    wall[:, 30:34] = 100
    K = TILE + 2
    d = _line(8, K=K)
    d[:, 2] = np.linspace(0.1, 0.3, K).astype(np.float32)
    return case("none_admissible", base_spec(steps=8), pose(*centre_of(20, 30)), d, ring(2), wall, slope_field(wall))


def none_regime():
    out, _, res = want(none_admissible_case())
    assert (out[:, 1] & ro.BLOCKED != 0).all() and len(set(out[:, 0])) > 1
    assert res.tolist() == [0, ro.NONE, 0xFFFFFFFF, 0xFFFFFFFF, 0, len(out), 0, 1]


# ---- the E16 identity -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def identity_case(K=TILE + 8, T=5):
    rng = np.random.default_rng(16)
    d = arc_deltas(rng.uniform(-0.3, 0.8, K), rng.uniform(-1.5, 1.5, K), 0.2)
    d[3] *= np.float32(1.7)                   # (c, s) need not be a rotation: nothing renormalises
    return case("identity", base_spec(steps=T), pose(4.0, 0.1, 0.3), d, ring(1), free_grid(1))


def identity_regime():
    out, _, _ = want(identity_case())
    assert (out[:, :2] == [5, ro.ADMISSIBLE]).all()   # never blocked: the end pose is pose_T


def all_small_cases():
    """Every case a scalar walk is affordable for (the CPU test runs both writers and the host twin over these)."""
    out = [shape_case(*sh) for sh in SHAPES] + group_cases()
    out += list(blocking_cases().values()) + list(field_cases().values())
    t = tie_cases()
    return out + [t["lanes"], t["tiles"], none_admissible_case()]
