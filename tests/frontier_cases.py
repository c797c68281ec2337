"""The inputs of the E29 tests (tests/test_frontier_cpu.py, tests/test_gpu_frontier.py) and, per family, the check that
each case is in the regime its name claims — from tests/frontier_oracle.py alone, so a case that drifted out of its
regime fails without the library.  A case is a dictionary: name, grid (H, W) int8, potential (H, W) uint32 or None,
spec, comp_cap, row_cap.  ``want`` is the scalar writer's answer, computed once per case."""
import numpy as np

from tests import frontier_oracle as fo

TILE = fo.TILE
U = fo.UNREACHED
UNKNOWN, FREE, WALL = -1, 0, 100
SIZES = [(1, 1), (1, 7), (7, 1), (4096, 3), (3, 4096), (131, 70), (64, 64), (65, 65)]
_wants = {}


def case(name, grid, potential=None, comp_cap=None, row_cap=4, **spec_kw):
    grid = np.ascontiguousarray(grid, np.int8)
    H, W = grid.shape
    s = fo.spec(width=W, height=H, **dict(dict(min_size=1), **spec_kw))
    if potential is not None:
        potential = np.ascontiguousarray(potential, np.uint32)
    return dict(name=name, grid=grid, potential=potential, spec=s, comp_cap=comp_cap or W * H, row_cap=row_cap)


def want(c):
    key = (c["name"], c["comp_cap"], c["row_cap"], tuple(sorted(c["spec"].items())))
    if key not in _wants:
        _wants[key] = fo.frontiers_walk(c["grid"], c["potential"], c["spec"], c["comp_cap"], c["row_cap"], 0x5A5A5A5A)
    return _wants[key]


def _tile_of(cell, W):
    return (cell % W) // TILE, (cell // W) // TILE


# ---- sizes: random maps of every byte class -------------------------------------------------------------------------------------
def size_case(W, H, seed=0, lethal=99, with_potential=True):
    rng = np.random.default_rng(1000 * W + H + seed)
    coarse = rng.integers(0, 3, (-(-H // 5), -(-W // 5)))
    cls = np.kron(coarse, np.ones((5, 5), int))[:H, :W]
    noise = rng.random((H, W)) < 0.05
    cls = np.where(noise, rng.integers(0, 3, (H, W)), cls)
    values = np.array([[-128, -1, -1], [0, lethal - 1, 1], [lethal, 100, 127]], np.int16)
    grid = values[cls, rng.integers(0, 3, (H, W))].astype(np.int8)
    pot = None
    if with_potential:
        pot = rng.integers(0, 40, (H, W)).astype(np.uint32)
        pot[rng.random((H, W)) < 0.05] = U
        pot[rng.random((H, W)) < 0.02] = 0xFFFFFFFE
    return case(f"size{W}x{H}s{seed}l{lethal}{'' if with_potential else 'nopot'}", grid, pot, lethal=lethal)


def sizes_regime():
    for W, H in SIZES:
        c = size_case(W, H)
        w = want(c)
        assert c["grid"].shape == (H, W) and w["result"][2] == len(w["comps"])
        if W * H > 100:
            assert w["result"][1] > 10 and w["result"][2] > 3 and (c["grid"] == 127).any() and (c["grid"] == -128).any()
            assert (c["grid"] == 98).any() and (c["grid"] == 99).any()
    w = want(size_case(131, 70))
    tiles = {_tile_of(int(c), 131) for c in np.flatnonzero(w["labels"].reshape(-1) != fo.NO_LABEL)}
    assert tiles == {(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)}  # the ragged last tiles hold frontier cells too


# ---- seams ------------------------------------------------------------------------------------------------------------------
def seam_cases():
    out = {}
    g = np.full((64, 128), UNKNOWN, np.int8)
    g[10, 60:70] = FREE
    out["vertical"] = case("seam_vertical", g)
    out["horizontal"] = case("seam_horizontal", g.T.copy())
    g = np.full((128, 128), UNKNOWN, np.int8)
    for i in range(60, 68):
        g[i, i] = FREE
    out["diagonal"] = case("seam_diagonal", g)
    g = np.full((128, 128), UNKNOWN, np.int8)
    for i in range(60, 68):
        g[127 - i, i] = FREE
    out["antidiagonal"] = case("seam_antidiagonal", g)
    # the pair (63, 11) - (64, 10): the second cell is north-east of the first and lies on a tile's FIRST column, in no
    # tile's last row — only the last column's test of its NE neighbour meets it
    g = np.full((64, 128), UNKNOWN, np.int8)
    for i in range(4):
        g[12 - i, 62 + i] = FREE
    out["ne"] = case("seam_ne", g)
    # a component whose least index lies in the LAST tile it touches (tile (1, 0) of a 2 x 2 grid of tiles): a hook
    g = np.full((128, 128), UNKNOWN, np.int8)
    g[70, 10:100] = FREE
    g[5:71, 99] = FREE
    out["hook"] = case("seam_hook", g)
    return out


def seams_regime():
    cs = seam_cases()
    for name in ("vertical", "horizontal", "diagonal", "antidiagonal", "ne", "hook"):
        w = want(cs[name])
        assert w["result"][2] == 1 and w["result"][1] == w["comps"][0][1] == (cs[name]["grid"] == FREE).sum(), name
    d = cs["diagonal"]["grid"]
    assert d[63, 63] == FREE and d[64, 64] == FREE and d[63, 64] != FREE and d[64, 63] != FREE
    a = cs["antidiagonal"]["grid"]
    assert a[63, 64] == FREE and a[64, 63] == FREE and a[63, 63] != FREE and a[64, 64] != FREE
    e = cs["ne"]["grid"]
    assert e[11, 63] == FREE and e[10, 64] == FREE and e[10, 63] != FREE and e[11, 64] != FREE
    w = want(cs["hook"])
    assert _tile_of(int(w["comps"][0][0]), 128) == (1, 0)
    assert {_tile_of(int(c), 128) for c in np.flatnonzero(w["labels"].reshape(-1) != fo.NO_LABEL)} == \
        {(0, 1), (1, 1), (1, 0)}


# ---- the longest chains ---------------------------------------------------------------------------------------------------------
def serpentine_case():
    """A one-cell-wide corridor of free cells in unknown space inside one tile: 32 teeth joined at alternating ends."""
    g = np.full((64, 64), UNKNOWN, np.int8)
    for i in range(32):
        g[1:63, 2 * i] = FREE
        if i < 31:
            g[63 if i % 2 == 0 else 0, 2 * i:2 * i + 3] = FREE
    return case("serpentine", g)


def spiral_case():
    """A square spiral over 3 x 3 tiles, arms four cells apart, from the centre outwards to its outer end at (0, 0)."""
    n = 192
    g = np.full((n, n), UNKNOWN, np.int8)
    x0, y0, x1, y1 = 0, 0, n - 1, n - 1
    g[0, 0] = FREE
    while x1 - x0 > 8:
        g[y0:y1 + 1, x0] = FREE          # down the left side
        g[y1, x0:x1 + 1] = FREE          # along the bottom
        g[y0 + 4:y1 + 1, x1] = FREE      # up the right side
        g[y0 + 4, x0 + 4:x1 + 1] = FREE  # back along the top, one arm in
        x0, y0, x1, y1 = x0 + 4, y0 + 4, x1 - 4, y1 - 4
    return case("spiral", g)


def chains_regime():
    w = want(serpentine_case())
    # every corridor cell but (0, 63), whose neighbours are corridor cells and the outside, which is not unknown
    assert w["result"][2] == 1 and w["result"][1] == 32 * 62 + 31 * 3 - 1 == w["comps"][0][1]
    c = spiral_case()
    w = want(c)
    assert w["result"][2] == 1 and w["comps"][0][0] == 0 and w["result"][1] > 5000
    assert {_tile_of(int(i), 192) for i in np.flatnonzero(w["labels"].reshape(-1) != fo.NO_LABEL)} == \
        {(x, y) for x in range(3) for y in range(3)}
    # the spiral is ONE corridor: no cell has more than two corridor neighbours among its four edge neighbours but at
    # the joints, and the cell (0, 0), its least index, is an end of it
    assert c["grid"][0, 1] != FREE and c["grid"][1, 0] == FREE


# ---- nothing to find, and many to find ------------------------------------------------------------------------------------------
def empty_cases():
    return dict(no_unknown=case("no_unknown", np.zeros((70, 131), np.int8)),
                no_free=case("no_free", np.full((70, 131), UNKNOWN, np.int8)),
                walls=case("walls", np.where(np.indices((70, 131)).sum(0) % 2, WALL, UNKNOWN).astype(np.int8)))


def lattice_case(min_size=1, comp_cap=None, row_cap=4, W=131, H=70):
    g = np.full((H, W), UNKNOWN, np.int8)
    g[::3, ::3] = FREE
    return case(f"lattice{min_size}", g, comp_cap=comp_cap, row_cap=row_cap, min_size=min_size)


LATTICE_N = 44 * 24


def counts_regime():
    for c in empty_cases().values():
        w = want(c)
        assert w["result"].tolist()[:6] == [fo.NONE | fo.NO_KEPT, 0, 0, 0, 0, fo.NO_LABEL] and w["n_goal"] == 0
    w = want(lattice_case(1))
    assert w["result"][1] == w["result"][2] == w["result"][3] == LATTICE_N == -(-131 // 3) * -(-70 // 3)
    assert w["result"][13] == 1 and w["result"][4] == 0 and w["result"][14] == 4
    w = want(lattice_case(2))
    assert w["result"][3] == 0 and w["result"][4] == LATTICE_N and w["result"][0] == fo.NO_KEPT and w["goal"] is None
    for cap, bound in ((LATTICE_N - 1, True), (LATTICE_N, False), (LATTICE_N + 1, False)):
        w = want(lattice_case(1, comp_cap=cap))
        assert bool(w["result"][0] & fo.BOUND) == bound and w["result"][1] == w["result"][2] == LATTICE_N
        assert (w["result"][3] == 0 and w["result"][14] == 0 and w["n_goal"] == 0) if bound else w["n_goal"] == 1
    for row_cap, written in ((0, 0), (LATTICE_N - 1, LATTICE_N - 1), (LATTICE_N + 1, LATTICE_N)):
        assert want(lattice_case(1, row_cap=row_cap))["result"][14] == written


# ---- the potential, the cost --------------------------------------------------------------------------------------------------
def _bar(W=140, H=9):
    g = np.full((H, W), UNKNOWN, np.int8)
    g[4, 3:W - 3] = FREE
    return g


def potential_cases():
    out = {}
    g = _bar()
    d = np.full(g.shape, 1000, np.uint32)
    out["none"] = case("pot_none", g, None)
    d1 = d.copy()
    d1[4, 63] = U  # a free cell next to unknown that the robot cannot reach: no frontier cell, and it SPLITS the bar
    out["split"] = case("pot_split", g, d1)
    d2 = d.copy()
    d2[4, 100], d2[4, 20] = 7, 7  # two cells share Dmin: the smaller index is the component's cell
    out["equal"] = case("pot_equal", g, d2)
    d3 = np.full(g.shape, 0xFFFFFFFE, np.uint32)
    out["huge"] = case("pot_huge", g, d3)
    d4 = d3.copy()
    d4[4, 130] = 0
    out["zero"] = case("pot_zero", g, d4)
    return out


def potential_regime():
    cs = potential_cases()
    n = 140 - 6
    w = want(cs["none"])
    assert w["comps"].tolist() == [[4 * 140 + 3, n, sum(range(3, 137)), 0, 4 * n, 0, 0, 4 * 140 + 3]]
    w = want(cs["split"])
    assert w["result"][2] == 2 and w["result"][1] == n - 1 and w["comps"][1][0] == 4 * 140 + 64
    assert w["labels"][4, 63] == fo.NO_LABEL
    w = want(cs["equal"])
    assert w["comps"][0][6] == 7 and w["comps"][0][7] == 4 * 140 + 20
    w = want(cs["huge"])
    assert w["comps"][0][6] == 0xFFFFFFFE and w["comps"][0][7] == 4 * 140 + 3
    w = want(cs["zero"])
    assert w["comps"][0][6] == 0 and w["comps"][0][7] == 4 * 140 + 130 == w["goal"]


def cost_cases():
    """Three bars, top to bottom: 20 cells at D 50, 60 cells at D 50, 30 cells at D 10."""
    g = np.full((20, 140), UNKNOWN, np.int8)
    d = np.full(g.shape, 9999, np.uint32)
    for y, (x0, n, dist) in {3: (70, 20, 50), 9: (10, 60, 50), 15: (60, 30, 10)}.items():
        g[y, x0:x0 + n] = FREE
        d[y, x0 + n // 2] = dist
    mk = lambda name, **kw: case("cost_" + name, g, d, **kw)  # noqa: E731
    return dict(default=mk("default", dist_weight=1, size_weight=0), size_only=mk("size_only", dist_weight=0, size_weight=65535),
                dist_only=mk("dist_only", dist_weight=65535, size_weight=0), kept_one=mk("kept_one", min_size=31),
                tie=mk("tie", dist_weight=3, size_weight=4),
                all_tie=mk("all_tie", dist_weight=0, size_weight=0), mixed=mk("mixed", dist_weight=1, size_weight=2),
                big=mk("big", dist_weight=65535, size_weight=65535))


def cost_regime():
    cs = cost_cases()
    labels = [3 * 140 + 70, 9 * 140 + 10, 15 * 140 + 60]
    assert want(cs["default"])["comps"][:, 0].tolist() == labels
    best = {k: int(want(c)["result"][5]) for k, c in cs.items()}
    assert best["default"] == labels[2] and best["size_only"] == labels[1] and best["dist_only"] == labels[2]
    assert best["kept_one"] == labels[1] and want(cs["kept_one"])["result"][3] == 1  # (only the 60-cell bar is kept)
    assert 3 * 50 - 4 * 60 == 3 * 10 - 4 * 30 < 3 * 50 - 4 * 20 and best["tie"] == labels[1]  # a tie: the smaller label
    assert best["all_tie"] == labels[0]                                     # every cost 0: the smallest label
    assert 50 - 2 * 60 < 10 - 2 * 30 < 50 - 2 * 20 and best["mixed"] == labels[1]
    assert best["big"] == labels[2]                                         # 65535 (10 - 30) is the least
    # a cost tie between two kept components of different labels, decided by the label alone
    w = want(dict(cs["default"], spec=dict(cs["default"]["spec"], dist_weight=1, size_weight=0, min_size=1)))
    top, mid = w["comps"][0], w["comps"][1]
    assert top[6] == mid[6] == 50 and top[0] < mid[0]


# ---- a room with a doorway into unknown space (the chain) ---------------------------------------------------------------------
def room_case(n=256):
    """A walled room of free cells, the rest unknown; a doorway in its east wall opens on a short known corridor that
    ends in unknown space, and a window of unknown cells is left INSIDE the room.  (0 / 100 / -1: an occupancy grid.)"""
    g = np.full((n, n), UNKNOWN, np.int8)
    g[40:200, 40:180] = WALL
    g[41:199, 41:179] = FREE
    g[100:110, 179] = FREE          # the doorway
    g[100:110, 180:215] = FREE      # the corridor beyond it, its far end open to unknown
    g[99, 180:215] = WALL
    g[110, 180:215] = WALL
    g[60:64, 60:64] = UNKNOWN       # a patch nobody has seen yet, inside the room
    return case("room", g, min_size=4)


def all_cases():
    out = [size_case(W, H) for W, H in SIZES] + [size_case(131, 70, seed=s) for s in (1, 2)]
    out += [size_case(65, 65, lethal=1), size_case(65, 65, lethal=100), size_case(131, 70, with_potential=False)]
    out += list(seam_cases().values()) + [serpentine_case(), spiral_case()] + list(empty_cases().values())
    out += [lattice_case(1), lattice_case(2), lattice_case(1, comp_cap=LATTICE_N - 1), lattice_case(1, comp_cap=LATTICE_N),
            lattice_case(1, row_cap=0), lattice_case(1, row_cap=LATTICE_N + 1)]
    out += list(potential_cases().values()) + list(cost_cases().values()) + [room_case()]
    return out
