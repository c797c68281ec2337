"""The inputs of tests/test_gpu_inflate.py (E12), each with a regime check made from the oracle alone
(tests/inflate_oracle.py): the check asserts that the case exercises what it claims, so a green test cannot
be an empty one.  tests/test_inflate_cpu.py runs every regime, and both oracle writers on every case,
without a device.  A case is dict(grids (G, H, W) int8, rc, table uint8 (rc * rc + 1,)); the tables of the
named specs come from the library's own rplgpu_inflation_table (tests/test_inflate_cpu.py holds that one to
the numpy table), so no exp enters a GPU comparison.
TEST INFRASTRUCTURE — imported by tests/ only."""
from __future__ import annotations

import numpy as np

from rplidar_ros2_driver_amd import abi
from tests import inflate_oracle as io

TILE = 64  # the kernel's output tile (csrc/rpl_inflate.hip): where the cases put their cells, nothing else
_CACHE = {}

# resolution / inscribed / inflation / scaling, by the reach they give
SPECS = {
    0: (0.05, 0.0, 0.0, 3.0),
    1: (0.05, 0.05, 0.05, 3.0),
    2: (1.0, 1.0, 2.0, 1.0),
    4: (0.1, 0.0, 0.35, 10.0),
    5: (0.05, 0.175, 0.25, 3.0),
    12: (0.05, 0.22, 0.55, 3.0),
    64: (0.05, 0.3, 3.2, 1.0),
}


def inflation(rc, inflate_unknown=0):
    _, ins, inf, sc = SPECS[rc]
    return abi.Inflation(ins, inf, sc, inflate_unknown)


def lib_table(rc):
    """The library's table of SPECS[rc] (host only)."""
    if ("table", rc) not in _CACHE:
        table, got = abi.inflation_table(inflation(rc), SPECS[rc][0])
        assert got == rc and len(table) == rc * rc + 1
        _CACHE[("table", rc)] = table
    return _CACHE[("table", rc)]


def case(grids, rc, table=None):
    grids = np.ascontiguousarray(grids, np.int8)
    if grids.ndim == 2:
        grids = grids[None]
    return dict(grids=grids, rc=rc, table=lib_table(rc) if table is None else np.asarray(table, np.uint8))


def want(c, inflate_unknown, key=None):
    """Per grid (result, cells) of a case by the separable writer, computed once per key."""
    k = None if key is None else ("want", key, inflate_unknown)
    if k is not None and k in _CACHE:
        return _CACHE[k]
    out = [io.inflate(g, c["table"], c["rc"], inflate_unknown) for g in c["grids"]]
    if k is not None:
        _CACHE[k] = out
    return out


# ---- tiny grids: the window is larger than the grid ------------------------------------------------------------
TINY_SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5)]  # (height, width)


def tiny_cases(rc):
    """Every tiny shape without and with one lethal cell (101: any value >= 100 is lethal), the other cells
    free, unknown and history values; one call per grid."""
    rng = np.random.default_rng(1200 + rc)
    out = []
    for H, W in TINY_SHAPES:
        for hot in (False, True):
            g = rng.choice(np.array([-1, 0, 37, 99], np.int8), size=(H, W))
            if hot:
                g[H // 2, W - 1] = 101
            out.append(case(g, rc))
    return out


def tiny_regime(rc):
    cs = tiny_cases(rc)
    assert sum(int(io.lethal(c["grids"]).any()) for c in cs) == len(TINY_SHAPES)
    assert all(TILE + 2 * rc > max(c["grids"].shape[1:]) for c in cs)
    if rc >= 1:  # some cell of some tiny grid takes a cost
        assert any((want(c, 1)[0][0] != want(case(c["grids"], 0), 1)[0][0]).any() for c in cs)


# ---- 131 x 67: tile edges and corners, the grid's corners, history and unknown cells -------------------------
EW, EH = 131, 67
CORNER = (TILE, TILE)  # (x, y): the first cell of tile (1, 1)
EDGE_LETHAL = [(0, 0), (EW - 1, 0), (0, EH - 1), (EW - 1, EH - 1),        # the grid's corners
               (TILE - 1, 20), (TILE, 30), (2 * TILE - 1, 40), (2 * TILE, 50),  # either side of x = 64 and x = 128
               (20, TILE - 1), (40, TILE), (100, TILE - 1), (110, TILE),  # either side of y = 64
               CORNER,
               (TILE - 5, 5), (TILE + 4, 45), (50, TILE - 5)]  # the outermost halo column / row of a tile at rc 5


def edges_grid():
    """Free cells; a band of unknown cells right of the tile corner; history values 1 .. 99 around (20, 63);
    values 101 and 127 (lethal too)."""
    if "edges" in _CACHE:
        return _CACHE["edges"]
    rng = np.random.default_rng(1210)
    g = np.zeros((EH, EW), np.int8)
    g[:, 65:80] = -1
    g[55:EH, 12:29] = rng.integers(1, 100, size=(EH - 55, 17))
    for x, y in EDGE_LETHAL:
        g[y, x] = 100
    g[10, 100], g[12, 90] = 101, 127
    _CACHE["edges"] = g
    return g


def edges_case(rc):
    return case(edges_grid(), rc)


def edges_regime():
    g = edges_grid()
    cx, cy = CORNER
    c5, c64 = edges_case(5), edges_case(64)
    d2 = io.d2_separable(g, 5)
    # (3, 4) and (4, 3) reach across the tile corner, (4, 4) does not
    assert d2[cy - 4, cx - 3] == 25 and d2[cy - 3, cx - 4] == 25 and d2[cy - 4, cx - 4] == io.NONE
    w5 = want(c5, 0, "edges5")[0][0]
    assert w5[cy - 4, cx - 3] == c5["table"][25] > 0 and w5[cy - 3, cx - 4] == c5["table"][25] and w5[cy - 4, cx - 4] == 0
    lone = g.copy()
    lone[cy, cx] = 0  # without the corner cell the three are out of every reach: the cost came across the corner
    assert (io.d2_separable(lone, 5)[cy - 4:cy - 2, cx - 4:cx - 2] == io.NONE).all()
    # every lethal cell next to a tile edge gives a cost to a cell of the tile beyond that edge
    for x, y in EDGE_LETHAL[4:12]:
        for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            if 0 <= nx < EW and 0 <= ny < EH and (nx // TILE, ny // TILE) != (x // TILE, y // TILE):
                assert d2[ny, nx] == 1 and w5[ny, nx] == 99, (x, y)
    # a lethal cell in the outermost column (row) of a tile's halo gives a cost to the tile's first column (row)
    for (x, y), (nx, ny) in zip(EDGE_LETHAL[13:], ((TILE, 5), (TILE - 1, 45), (50, TILE))):
        assert d2[ny, nx] == 25 and w5[ny, nx] == c5["table"][25], (x, y)
        lone = g.copy()
        lone[y, x] = 0
        assert io.d2_separable(lone, 5)[ny, nx] == io.NONE
    # at least one unknown cell flips between the two flag values, one stays unknown, one is inscribed in both
    u0, u1 = w5, want(c5, 1, "edges5")[0][0]
    unk = g < 0
    assert ((u0 == -1) & (u1 > 0) & unk).sum() >= 1 and ((u0 == 99) & (u1 == 99) & unk).sum() >= 1
    assert ((u1 == -1) & unk).sum() >= 1
    # history values above and below their cost
    hist = (g >= 1) & (g <= 99)
    cost = io.combine(np.zeros_like(g), d2, c5["table"], 5, 0)[0]
    assert (hist & (g > cost) & (cost > 0)).sum() >= 1 and (hist & (g < cost)).sum() >= 1
    assert (u0[g > 100] == 100).all() and (g > 100).sum() == 2
    # rc 64: the window of every tile is higher than the grid, every cell is within reach of a lethal cell, some
    # only of one that is more than half a tile away
    w64 = io.d2_separable(g, 64)
    assert (w64 != io.NONE).all() and w64.max() > (TILE // 2) ** 2 and (want(c64, 0, "edges64")[0][0] != w5).any()


# ---- uniform grids and a disc cut by the border ---------------------------------------------------------------
UW, UH = 70, 66


def uniform_cases():
    lone = np.zeros((UH, UW), np.int8)
    lone[2, 1] = 100
    return {"free": case(np.zeros((UH, UW), np.int8), 5), "unknown": case(np.full((UH, UW), -1, np.int8), 5),
            "lethal": case(np.full((UH, UW), 100, np.int8), 5), "cut_disc": case(lone, 5)}


def uniform_regime():
    cs = uniform_cases()
    for name, cells in (("free", (0, 0, 0, 0)), ("unknown", (0, 0, 0, UW * UH)), ("lethal", (UW * UH, 0, 0, 0))):
        assert want(cs[name], 0)[0][1] == cells, name
    out, cells = want(cs["cut_disc"], 0)[0]
    full = int((io.d2_separable(np.pad(cs["cut_disc"]["grids"][0], 8), 5) != io.NONE).sum())
    assert 1 < (out > 0).sum() < full  # the border cuts the disc


# ---- three grids in one call, width a multiple of 4, one of them empty --------------------------------------------
BW, BH = 140, 70


def batch_case():
    """Grid 0: a cluster in the middle of tile (0, 0), every other tile's window is empty; grid 1: no lethal
    cell at all (history and unknown cells only); grid 2: lethal cells sprinkled everywhere."""
    if "batch" in _CACHE:
        return _CACHE["batch"]
    rng = np.random.default_rng(1220)
    g = rng.choice(np.array([-1, 0, 0, 0, 45], np.int8), size=(3, BH, BW))
    g[0, 28:33, 30:34] = 100
    g[2][rng.random((BH, BW)) < 0.004] = 100
    _CACHE["batch"] = case(g, 12)
    return _CACHE["batch"]


def batch_regime():
    c = batch_case()
    g, rc = c["grids"], c["rc"]
    assert BW % 4 == 0 and BW % TILE and BH % TILE
    L0 = np.argwhere(io.lethal(g[0]))
    assert len(L0) and (L0 + rc < TILE).all() and not io.lethal(g[1]).any()  # no other tile's window sees them
    assert len(np.argwhere(io.lethal(g[2]))) >= 20
    res = want(c, 0, "batch")
    assert res[1][1][0] == 0 and res[1][1][3] == (g[1] < 0).sum() and res[0][1][0] == 20


# ---- a table the caller made: a step function ---------------------------------------------------------------------
STEP_TABLE = np.array([100] + [70] * 4 + [20] * 5, np.uint8)  # rc 3: 70 up to distance 2, 20 up to 3


def step_case():
    return case(edges_grid(), 3, STEP_TABLE)


def step_regime():
    c = step_case()
    assert (np.diff(c["table"].astype(int)) <= 0).all()
    out = want(c, 0, "step")[0][0]
    free = edges_grid() == 0
    assert set(np.unique(out[free]).tolist()) == {0, 20, 70}
    assert (out != want(case(edges_grid(), 3, np.array([100] + [99] * 9, np.uint8)), 0)[0][0]).any()


# ---- the chain: E11's grid of an existing input, 1024 x 1024, the defaults ------------------------------------------
def chain_case(occ_grid):
    """occ_grid: group 0 of tests/occ_cases.py full_case(0), by the E11 oracle or by the device."""
    return case(occ_grid, 12)


def chain_regime(c):
    g = c["grids"][0]
    assert g.shape == (1024, 1024) and set(np.unique(g).tolist()) == {-1, 0, 100}
    L = io.lethal(g)
    tiles = L.reshape(16, TILE, 16, TILE).any(axis=(1, 3))
    assert tiles.sum() >= 8 and (~tiles).sum() >= 100  # working tiles beside tiles that leave early
    out, cells = want(c, 0, "chain")[0]
    assert cells[1] > 0 and cells[2] > 0 and cells[3] > 0 and cells[0] == L.sum()
