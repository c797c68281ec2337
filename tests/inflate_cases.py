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


# ==== tests across the window =======================================================================================
# Every grid above holds many lethal cells, so a wrong distance to a far one hides behind a nearer one.  The cases
# below put single cells where one code path of k_inflate alone decides a byte.
def linear_table(rc):
    """table[0] = 100, table[k] = max(1, 98 - floor(97 sqrt(k) / rc)): non-increasing, 1 .. 98, and far from flat
    far out (the library's table at rc 64 is nearly flat there).  Made here and handed to the oracle and the device
    as the same bytes, so no sqrt enters a comparison."""
    k = np.arange(1, rc * rc + 1, dtype=np.float64)
    far = np.maximum(1.0, 98.0 - np.floor(97.0 * np.sqrt(k) / max(rc, 1)))
    return np.concatenate(([100.0], far)).astype(np.uint8)


# ---- one lethal cell per grid, rc 64: every byte within 64 cells is table[D2] of that cell ----------------------------
LONE_H = 192
LONE_WIDTHS = (192, 189, 190, 191)  # both kernel instances, every width mod 4
LONE_SHIFTS = {192: (0, 7), 189: (3, 11), 190: (5, 13), 191: (1, 9)}  # x number i goes with y number i + shift
LONE_127 = 4  # the grid whose lethal cell holds 127


def lone_axis(n):
    return [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 159, 160, n - 1]


def lone_cells(W):
    xs, ys = lone_axis(W), lone_axis(LONE_H)
    return [(xs[i], ys[(i + s) % len(ys)]) for s in LONE_SHIFTS[W] for i in range(len(xs))]


def lone_case(W):
    if ("lone", W) not in _CACHE:
        cells = lone_cells(W)
        g = np.zeros((len(cells), LONE_H, W), np.int8)
        for i, (x, y) in enumerate(cells):
            g[i, y, x] = 127 if i == LONE_127 else 100
        _CACHE[("lone", W)] = case(g, 64, linear_table(64))
    return _CACHE[("lone", W)]


def lone_regime():
    if "lone_regime" in _CACHE:
        return
    sides, cuts = set(), set()
    for W in LONE_WIDTHS:
        c, cells = lone_case(W), lone_cells(W)
        assert len(cells) <= 64 and (io.lethal(c["grids"]).sum(axis=(1, 2)) == 1).all() and not (c["grids"] < 0).any()
        assert c["grids"][LONE_127].max() == 127
        for axis, n in ((0, W), (1, LONE_H)):  # every x goes with two different y, every y with two different x
            for v in lone_axis(n):
                assert len({p[1 - axis] for p in cells if p[axis] == v}) >= 2, (W, axis, v)
        words = set()
        yy, xx = np.mgrid[0:LONE_H, 0:W]
        for (x, y), (out, cnt) in zip(cells, want(c, 0, ("lone", W))):
            assert len(np.unique(out)) >= 60 and cnt[0] == 1
            other = (out > 0) & ((xx // TILE != x // TILE) | (yy // TILE != y // TILE))
            allowed = []
            for name, sgn in (("left", -1), ("right", 1)):
                if any(0 <= x + sgn * d < W and (x + sgn * d) // TILE != x // TILE for d in range(33, 65)):
                    assert (other & (sgn * (xx - x) > 32)).any(), (W, x, y, name)
                    allowed.append(name)
            assert allowed, (W, x, y)
            sides.update(allowed)
            cuts.add(min(x, y) < 64 or x > W - 65 or y > LONE_H - 65)
            # the 32-bit word of the mask row that holds the cell, for every tile column whose tiles it reaches
            words.update((x - tx0 + TILE) >> 5 for tx0 in range(0, W, TILE) if max(tx0 - x, x - tx0 - 63) <= 64)
        assert words == set(range(6)), (W, words)
    assert sides == {"left", "right"} and cuts == {False, True}
    _CACHE["lone_regime"] = True


# ---- the lanes-per-row switch of the stage pass: window rows of 57 .. 63 and 122 .. 127 cells ---------------------------
STAGE_NARROW = (57, 58, 59, 60, 61, 62, 63)  # one tile column, rc 3: the 16 | 32 lane switch is at 60 | 61
STAGE_NARROW_H = 40
STAGE_NARROW_ROWS = (2, 9, 16, 23, 30, 37)
STAGE_WIDE = (122, 123, 124, 125, 126, 127)  # two tile columns, rc 64: the 32 | 64 lane switch is at 124 | 125
STAGE_H = 70
STAGE_ROWS = (3, 12, 21, 30, 39, 48, 57, 66)  # y mod 4 = 3 0 1 2 3 0 1 2
STAGE_INNER = ((200, 30), (200, 31), (199, 30), (199, 31))  # (W, rc): the interior tile's window row is 64 + 2 rc long


def stage_narrow_case(W):
    g = np.zeros((STAGE_NARROW_H, W), np.int8)
    for y in STAGE_NARROW_ROWS:
        g[y, W - 1] = g[y, 0] = 100
    return case(g, 3, STEP_TABLE)


def stage_wide_case(W):
    g = np.zeros((STAGE_H, W), np.int8)
    for y in STAGE_ROWS[:4]:
        g[y, W - 1] = 100  # the last window column of both tiles
    for y in STAGE_ROWS[4:]:
        g[y, 0] = 100      # the first
    return case(g, 64, linear_table(64))


def stage_inner_case(W, rc):
    g = np.zeros((STAGE_H, W), np.int8)
    for y in STAGE_ROWS:
        g[y, 2 * TILE - 1 + rc] = g[y, TILE - rc] = 100  # the last and the first window column of tile (1, 0)
    return case(g, rc, linear_table(rc))


def stage_cases():
    if "stage" in _CACHE:
        return _CACHE["stage"]
    out = {f"narrow{W}": stage_narrow_case(W) for W in STAGE_NARROW}
    out.update({f"wide{W}": stage_wide_case(W) for W in STAGE_WIDE})
    out.update({f"inner{W}_rc{rc}": stage_inner_case(W, rc) for W, rc in STAGE_INNER})
    _CACHE["stage"] = out
    return out


def _only_source(c, src, dst, k):
    """dst takes table[k] and only because of the lethal cell src: without src its distance is another one."""
    g, rc = c["grids"][0], c["rc"]
    assert io.lethal(g)[src[1], src[0]] and io.d2_separable(g, rc)[dst[1], dst[0]] == k
    assert io.inflate(g, c["table"], rc, 0)[0][dst[1], dst[0]] == c["table"][k] > 0
    lone = g.copy()
    lone[src[1], src[0]] = 0
    assert io.d2_separable(lone, rc)[dst[1], dst[0]] > k


def _phases(W, x0, rows):
    return {(y * W + x0) & 3 for y in rows}


def stage_regime():
    if "stage_regime" in _CACHE:
        return
    _stage_regime()
    _CACHE["stage_regime"] = True


def _stage_regime():
    for W in STAGE_NARROW:
        c = stage_narrow_case(W)
        assert c["grids"].shape[1:] == (STAGE_NARROW_H, W) and W <= TILE  # the window row is the grid row
        assert all(b - a > 2 * c["rc"] for a, b in zip(STAGE_NARROW_ROWS, STAGE_NARROW_ROWS[1:]))
        assert _phases(W, 0, STAGE_NARROW_ROWS) == _phases(W, 0, range(STAGE_NARROW_H))
        for y in STAGE_NARROW_ROWS:
            _only_source(c, (W - 1, y), (W - 2, y), 1)
            _only_source(c, (0, y), (1, y), 1)
    assert {(W + 3) // 4 + 1 for W in STAGE_NARROW} == {16, 17}
    for W in STAGE_WIDE:
        c = stage_wide_case(W)
        assert TILE < W <= 2 * TILE and c["rc"] == 64  # both tiles' window rows are the grid row
        assert _phases(W, 0, STAGE_ROWS[:4]) == _phases(W, 0, STAGE_ROWS[4:]) == _phases(W, 0, range(STAGE_H))
        for y in STAGE_ROWS[:4]:
            _only_source(c, (W - 1, y), (W - 2, y), 1)
        for y in STAGE_ROWS[4:]:
            _only_source(c, (0, y), (1, y), 1)
    assert {(W + 3) // 4 + 1 for W in STAGE_WIDE} == {32, 33}
    # a row of W cells that starts at byte a of a word touches (a + W + 3) // 4 words: 17 only at W 62 (a 3) and
    # W 63 (a >= 2), 33 only at W 126 (a 3) and W 127 (a >= 2), and an even width has no row with a 3, so W 63 and
    # W 127 are where a lane too few drops a word; they hold a lethal cell in that word
    assert any((y * 63 & 3) >= 2 for y in STAGE_NARROW_ROWS) and any((y * 127 & 3) >= 2 for y in STAGE_ROWS[:4])
    for W, rc in STAGE_INNER:
        c = stage_inner_case(W, rc)
        xa, xb = TILE - rc, 2 * TILE + rc
        assert 0 < xa and xb < W and xb - xa == TILE + 2 * rc and c["grids"].shape[1:] == (STAGE_H, W)
        assert _phases(W, xa, STAGE_ROWS) == _phases(W, xa, range(STAGE_H))
        for y in STAGE_ROWS:
            _only_source(c, (xb - 1, y), (2 * TILE - 1, y), rc * rc)
            _only_source(c, (xa, y), (TILE, y), rc * rc)
    assert {(TILE + 2 * rc + 3) // 4 + 1 for _, rc in STAGE_INNER} == {32, 33}
    assert any(((y * 199 + TILE - 31) & 3) == 3 for y in STAGE_ROWS)  # 126 cells from byte 3: 33 words


# ---- reaches that put the halo edge at, next to and across a mask word boundary ----------------------------------------
REACH_RCS = (2, 7, 30, 31, 32, 33, 63)
REACH_SHAPES = ((200, 136), (197, 131))  # (W, H): 4 x 3 tiles, an interior tile, both kernel instances
REACH_UNKNOWN = (-1, -2, -77, -128)
REACH_LETHAL = {2: 700, 7: 110, 30: 9, 31: 9, 32: 8, 33: 8, 63: 2}  # sprinkled lethal cells per grid, see reach_regime


def reach_word(W):
    """(x, y) of the first cell of the planted output word: in tile (1, 1), at a multiple of 4 of the flat array."""
    y = TILE + 6
    return TILE + 4 + (-(y * W + TILE + 4)) % 4, y


def reach_case(rc, W, H):
    """History values 1 .. 99 and the four unknown bytes among free cells; REACH_LETHAL[rc] lethal cells sprinkled
    with a fixed seed, so few that many cells take their cost from another tile's cell and from far away (at rc 2
    half of them within rc of a tile edge: a disc of 13 cells seldom crosses one by chance).  From rc 7 on, two
    planted cells around the word at reach_word, r = rc - 1: A r rows above the word's first cell and B r - 2
    columns right of its last cell on its own row, no sprinkled cell within reach of the word.  Its D2 are
    then r^2 (from A, row r), r^2, (r - 1)^2, (r - 2)^2 (from B, row 0): the second pair is done long before
    row r, the first cell is not."""
    if ("reach", rc, W) not in _CACHE:
        rng = np.random.default_rng(1240 + 1000 * rc + W)
        kind = rng.random((H, W))
        g = np.zeros((H, W), np.int8)
        g[kind < 0.15] = rng.integers(1, 100, size=int((kind < 0.15).sum()))
        g[kind > 0.85] = rng.choice(np.array(REACH_UNKNOWN, np.int8), size=int((kind > 0.85).sum()))
        yy, xx = np.mgrid[0:H, 0:W]
        ok = np.ones((H, W), bool)
        n = REACH_LETHAL[rc]
        if rc >= 7:
            xw, yw = reach_word(W)
            r = rc - 1
            ok = (xx < xw - rc) | (xx > xw + 3 + rc) | (np.abs(yy - yw) > rc)
            g[yw - r, xw] = g[yw, xw + 3 + r - 2] = 100
        else:
            band = ((xx % TILE < rc) | (xx % TILE >= TILE - rc) | (yy % TILE < rc) | (yy % TILE >= TILE - rc))
            g.reshape(-1)[rng.choice(np.flatnonzero(band), size=n // 2, replace=False)] = 100
            n -= n // 2
        g.reshape(-1)[rng.choice(np.flatnonzero(ok), size=n, replace=False)] = 100
        _CACHE[("reach", rc, W)] = case(g, rc, linear_table(rc))
    return _CACHE[("reach", rc, W)]


def reach_cases():
    return {f"rc{rc}_{W}x{H}": reach_case(rc, W, H) for rc in REACH_RCS for W, H in REACH_SHAPES}


def d2_rows(grid, rc):
    """-> (D2, the smallest |dy| of a row that gives it): the column minimum of d2_separable, rows taken in
    the order y, y -+ 1, y -+ 2, ..."""
    L = io.lethal(grid)
    H, W = L.shape
    hx2 = np.stack([io.d2_separable(L[y:y + 1].astype(np.int8) * 100, rc)[0] for y in range(H)])  # dy = 0 alone
    out = np.full((H, W), io.NONE, np.int64)
    first = np.full((H, W), -1, np.int64)
    for d in range(0, rc + 1):
        for dy in {d, -d}:
            if abs(dy) >= H:
                continue
            ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
            cand = hx2[ys] + dy * dy
            better = (cand < out[yd]) & (cand <= rc * rc)
            out[yd][better] = cand[better]
            first[yd][better] = d
    return out, first


def reach_regime(rc, W, H):
    if ("reach_regime", rc, W) in _CACHE:
        return
    _reach_regime(rc, W, H)
    _CACHE[("reach_regime", rc, W)] = True


def _reach_regime(rc, W, H):
    c = reach_case(rc, W, H)
    g, table = c["grids"][0], c["table"]
    assert g.shape == (H, W) and (W + TILE - 1) // TILE == 4 and (H + TILE - 1) // TILE == 3
    assert ((g >= 1) & (g <= 99)).sum() > 1000 and len(np.unique(g[(g >= 1) & (g <= 99)])) == 99
    d2 = io.d2_separable(g, rc)
    costed = (d2 > 0) & (d2 <= rc * rc)
    # the share of costed cells whose nearest lethal cell is in another tile: no cell of their own tile is as near
    same = np.full((H, W), io.NONE, np.int64)
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            same[ty:ty + TILE, tx:tx + TILE] = io.d2_separable(g[ty:ty + TILE, tx:tx + TILE], rc)
    across = costed & (same > d2)
    far = costed & (d2 > (rc - 1) ** 2)
    print(f"rc {rc} {W} x {H}: {int(costed.sum())} costed cells, {across.sum() / costed.sum():.3f} from another tile, "
          f"{far.sum() / costed.sum():.3f} from more than rc - 1 away, {int((d2 == io.NONE).sum())} without a cost")
    assert across.sum() >= 0.05 * costed.sum() and far.sum() >= 0.01 * costed.sum()
    # every unknown byte under a cost and under none; what comes out for both flags (the table has no 99)
    assert table[1:].max() <= 98 and table.min() >= 1
    out0, out1 = want(c, 0, ("reach", rc, W))[0][0], want(c, 1, ("reach", rc, W))[0][0]
    for u in REACH_UNKNOWN:
        under, bare = (g == u) & costed, (g == u) & (d2 == io.NONE)
        assert under.sum() >= 1 and bare.sum() >= 1, u
        assert (out0[g == u] == -1).all() and (out1[bare] == -1).all()
        assert (out1[under] == table[d2[under]]).all() and (out1[under] > 0).all()
    # an output word (four cells of one tile row, at a multiple of 4 of the flat array) whose D2 differ by more than
    # 2 rc and whose largest comes from a row more than rc / 2 away; in one of them the other pair of the word
    # is done before that row, which is where an early stop on less than the largest of the four stops too soon.
    # Not at rc 2: four D2 within reach are 0 .. 4 and cannot differ by more than 2 rc = 4.
    if rc < 7:
        return
    d2r, first = d2_rows(g, rc)
    assert np.array_equal(d2r, d2)
    xw, yw = reach_word(W)
    r = rc - 1
    assert (yw * W + xw) % 4 == 0 and xw // TILE == (xw + 3) // TILE == 1 and yw // TILE == 1
    assert d2[yw, xw:xw + 4].tolist() == [r * r, r * r, (r - 1) ** 2, (r - 2) ** 2] and first[yw, xw] == r > rc / 2
    assert (first[yw, xw + 1:xw + 4] == 0).all() and r * r - (r - 2) ** 2 > 2 * rc
    assert table[r * r] != table[(r + 1) ** 2]  # what the first cell keeps from B if the walk stops before row r
    spread = stops = 0
    flat_d2, flat_first = d2.reshape(-1), first.reshape(-1)
    for f in range(0, W * H - 3, 4):
        y, x = divmod(f, W)
        if x + 3 >= W or x // TILE != (x + 3) // TILE:
            continue
        q, fr = flat_d2[f:f + 4], flat_first[f:f + 4]
        if (q > rc * rc).any() or q.max() - q.min() <= 2 * rc:
            continue
        e = int(np.argmax(q))
        if 2 * fr[e] <= rc:
            continue
        spread += 1
        pair = q[2:] if e < 2 else q[:2]
        stops += int(pair.max() <= (fr[e] - 1) ** 2)
    print(f"  {spread} words with a spread above 2 rc from a far row, {stops} where the other pair is done before it")
    assert spread >= 1 and stops >= 1


# ---- the 99 and 1 .. 98 counters at full tiles: a checkerboard, rc 1 -------------------------------------------------
COUNT_TABLES = {"99": np.array([100, 99], np.uint8), "50": np.array([100, 50], np.uint8)}
COUNT_WIDTHS = (128, 127)


def count_case(W, name):
    yy, xx = np.mgrid[0:128, 0:W]
    return case(np.where((xx + yy) & 1, 0, 100), 1, COUNT_TABLES[name])


def count_regime():
    if "count_regime" in _CACHE:
        return
    _count_regime()
    _CACHE["count_regime"] = True


def _count_regime():
    for W in COUNT_WIDTHS:
        n = 128 * W // 2
        assert want(count_case(W, "99"), 0)[0][1] == (n, n, 0, 0) and want(count_case(W, "50"), 1)[0][1] == (n, 0, n, 0)
    assert 128 * 128 // 2 == 8192 and 128 % TILE == 0  # whole tiles: every free cell of every wave is counted


# ---- extreme shapes ----------------------------------------------------------------------------------------------------
SHAPES = {"4096x65": (4096, 65, 12), "65x4096": (65, 4096, 12), "4093x67": (4093, 67, 31)}  # (W, H, rc)
MANY_G, MANY_W, MANY_H = 300, 5, 3


def shape_case(name):
    """A sparse lattice of lethal cells, one in every corner and one in the last tile of the last tile row."""
    if ("shape", name) not in _CACHE:
        W, H, rc = SHAPES[name]
        g = np.zeros((H, W), np.int8)
        g[7::53, 11::97] = 100
        g[0, 0] = g[0, W - 1] = g[H - 1, 0] = g[H - 1, W - 1] = 100
        g[H - 1 - (H - 1) % TILE, W - 1 - (W - 1) % TILE] = 100  # the first cell of the last tile
        _CACHE[("shape", name)] = case(g, rc, None if rc == 12 else linear_table(rc))
    return _CACHE[("shape", name)]


def many_case():
    """300 grids of 5 x 3 in one call, every third one without a lethal cell."""
    if "many" not in _CACHE:
        rng = np.random.default_rng(1260)
        g = rng.choice(np.array([-1, 0, 0, 0, 45], np.int8), size=(MANY_G, MANY_H, MANY_W))
        for i in range(MANY_G):
            if i % 3:
                g[i, i % MANY_H, (i // 3) % MANY_W] = 100
        _CACHE["many"] = case(g, 2)
    return _CACHE["many"]


def shape_regime():
    if "shape_regime" in _CACHE:
        return
    _shape_regime()
    _CACHE["shape_regime"] = True


def _shape_regime():
    assert abi.MAX_OCC_DIM == 4096 and {s[0] for s in SHAPES.values()} >= {4096, 4093, 65}
    for name, (W, H, rc) in SHAPES.items():
        c = shape_case(name)
        L = io.lethal(c["grids"][0])
        assert L.shape == (H, W) and L[0, 0] and L[0, W - 1] and L[H - 1, 0] and L[H - 1, W - 1]
        assert L[(H - 1) // TILE * TILE, (W - 1) // TILE * TILE] and max(W, H) > 3 * TILE and 30 <= L.sum() < W * H // 500
        out = want(c, 0, ("shape", name))[0][0]
        assert out[H - 1, W - 2] == c["table"][1] and out[H - 2, 0] == c["table"][1]
    assert SHAPES["4093x67"][0] % 4 and SHAPES["4093x67"][0] > 3 * TILE  # more than 3 tiles across, odd width
    c = many_case()
    n = io.lethal(c["grids"]).sum(axis=(1, 2))
    assert c["grids"].shape == (MANY_G, MANY_H, MANY_W) and (n[::3] == 0).all() and (n[1::3] == 1).all() and (n[2::3] == 1).all()
    cells = [w[1] for w in want(c, 0, "many")]
    assert len(set(cells)) > 20  # the counts tell the grids apart
