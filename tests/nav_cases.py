"""The inputs of E26's tests and what makes each of them a test: every builder returns a case (a spec, a grid, the
goals) and every ``*_regime`` asserts, from tests/nav_oracle.py alone, that the case is in the regime its name claims
— a reachable cell three tiles from the goal, a diagonal refused only by the corner rule, a cap that cuts and keeps.
``want`` is the heap writer's field of a case, computed once per name."""
import numpy as np

from tests import nav_oracle as no

TILE = 64  # the relaxation's tile (csrc/rpl_nav.hip): where the cases put their walls, doors and goals
U = no.UNREACHED
_CACHE = {}
BYTES = np.array([0, 30, 98, 99, 100, -1], np.int8)


def case(name, grid, goals, **spec):
    grid = np.ascontiguousarray(grid, np.int8)
    H, W = grid.shape
    return dict(name=name, grid=grid, goals=[int(g) for g in goals], spec=no.spec(width=W, height=H, **spec))


def want(c):
    """The field of a case by the heap writer, once per name."""
    if c["name"] not in _CACHE:
        _CACHE[c["name"]] = no.field_heap(c["grid"], c["goals"], c["spec"])
    return _CACHE[c["name"]]


def cell(c, x, y):
    return y * c["spec"]["width"] + x


def random_grid(seed, W, H, free=0.8):
    """Mostly free cells, the rest drawn from every kind of byte."""
    rng = np.random.default_rng(seed)
    g = BYTES[rng.integers(0, len(BYTES), (H, W))]
    g[rng.random((H, W)) < free] = 0
    return g


# ---- sizes: below, at and above a tile, a row, a column, a grid of several tiles with ragged edges -----------------------
SIZES = ((1, 1), (1, 65), (65, 1), (63, 63), (64, 64), (65, 65), (129, 67))  # (width, height)


def size_case(W, H):
    g = random_grid(100 * W + H, W, H)
    goal = (W // 3, H // 2)
    g[goal[1], goal[0]] = 0
    if H == 1 or W == 1:
        g[:] = np.where(g >= 99, 30, g)  # a row or column keeps no wall: every cell stays in reach
        g[g < 0] = 0
    return case(f"size{W}x{H}", g, [goal[1] * W + goal[0]])


def sizes_regime():
    for W, H in SIZES:
        c = size_case(W, H)
        D = want(c)
        reached = D != U
        assert reached.sum() >= max(1, W * H // 2), (W, H)
        if W > TILE:  # the last tile column is ragged and reached
            assert reached[:, TILE * (W // TILE):].any()
        if W * H > 1 and W > 1 and H > 1:
            assert (~reached).any()  # and walls are in the way somewhere


# ---- goals: the corners of a tile and of the grid, on a wall, doubled, out of range, none -----------------------------------
GW, GH = 129, 67


def goals_grid():
    g = random_grid(7, GW, GH, free=0.9)
    g[10, 10] = 100  # a goal will sit on this wall
    g[9:12, 9] = 0
    return g


def goal_cases():
    g = goals_grid()
    at = lambda x, y: y * GW + x  # noqa: E731
    tile = [at(0, 0), at(63, 0), at(0, 63), at(63, 63), at(64, 0), at(127, 63), at(64, 64), at(128, 66), at(0, 66),
            at(128, 0)]
    return {
        "corners": case("goal_corners", g, tile),
        "wall": case("goal_wall", g, [at(10, 10)]),
        "double": case("goal_double", g, [at(40, 40), at(40, 40), at(100, 5), at(40, 40)]),
        "outside": case("goal_outside", g, [GW * GH, at(70, 30), 0xFFFFFFFF, GW * GH + 5]),
        "only_outside": case("goal_only_outside", g, [GW * GH]),
        "none": case("goal_none", g, []),
        "many": case("goal_many", g, [at(x % GW, (7 * x) % GH) for x in range(1100)]),
    }


def goals_regime():
    cs = goal_cases()
    D = want(cs["corners"])
    assert all(D.reshape(-1)[c] == 0 for c in cs["corners"]["goals"])
    D = want(cs["wall"])
    assert cs["wall"]["grid"][10, 10] == 100 and D[10, 10] == 0 and D[10, 9] == 250  # a goal on a wall is a goal
    assert no.goals_taken(cs["outside"]["goals"], GW * GH) == ([30 * GW + 70], 3)
    assert (want(cs["none"]) == U).all() and (want(cs["only_outside"]) == U).all()
    taken, ignored = no.goals_taken(cs["many"]["goals"], GW * GH)
    assert len(taken) == 1024 and ignored == 76  # the goals beyond the first 1024 are ignored
    late = cs["many"]["goals"][1050]
    assert late not in taken and want(cs["many"]).reshape(-1)[late] != 0


# ---- a goal on a tile's border that is the only cell its neighbours can read --------------------------------------------
def border_goal_cases():
    """The goal's own tile changes nothing when it runs (its only passable cell is the goal, already 0), so the tiles
    across the border are in reach only if placing the goal itself made them dirty."""
    row = np.zeros((1, 130), np.int8)
    row[0, 62] = 100
    row_west = np.zeros((1, 130), np.int8)
    row_west[0, 65] = 100
    col = np.zeros((130, 1), np.int8)
    col[62, 0] = 100
    door = np.zeros((70, 130), np.int8)
    door[:, :64] = 100  # tile column 0 is wall but for the door in its last column
    door[30, 63] = 0
    wall = door.copy()
    wall[30, 63] = 100  # the goal on the wall itself
    corner = np.zeros((130, 130), np.int8)
    corner[:64, :64] = 100
    corner[63, 63] = 0
    return {
        "row": case("border_row", row, [63]),                    # east of the goal: tile 1
        "row_west": case("border_row_west", row_west, [64]),     # west of the goal: tile 0
        "col": case("border_col", col, [63]),
        "door": case("border_door", door, [30 * 130 + 63]),
        "wall": case("border_wall", wall, [30 * 130 + 63]),
        "corner": case("border_corner", corner, [63 * 130 + 63]),  # the tiles east, south and south-east
    }


def border_goals_regime():
    cs = border_goal_cases()
    for name, c in cs.items():
        D = want(c)
        g = c["goals"][0]
        gx, gy = g % c["spec"]["width"], g // c["spec"]["width"]
        ty, tx = gy // TILE, gx // TILE
        own = D[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
        if name in ("row", "col", "row_west"):
            # in its own tile the goal's side of the lethal cell: nothing on the border towards the other tile changes
            assert D[gy, gx] == 0
        else:
            assert (own != U).sum() == 1  # the goal alone
        other = D.copy()
        other[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = U
        assert (other != U).sum() >= 60, name  # and the answer reaches into the tiles across the border
    assert want(cs["row"])[0, 64] == 250 and want(cs["row"])[0, 61] == U
    assert want(cs["row_west"])[0, 63] == 250 and want(cs["row_west"])[0, 66] == U
    D = want(cs["corner"])
    assert D[63, 64] == 250 and D[64, 63] == 250 and D[64, 64] == 350


# ---- walls on tile borders with a door one cell wide at a tile corner ------------------------------------------------------
def doors_case():
    """130 x 130: a wall down column 64 with its door at (64, 63), a wall along row 64 with doors at (63, 64) and
    (127, 64).  The goal is in the top-left room; the bottom-right room is reached through three doors."""
    g = np.zeros((130, 130), np.int8)
    g[:, 64] = 100
    g[64, :] = 100
    g[63, 64] = 0
    g[64, 63] = 0
    g[64, 127] = 0
    return case("doors", g, [5 * 130 + 5])


def doors_regime():
    c = doors_case()
    D = want(c)
    assert D[20, 20] != U and D[20, 100] != U and D[100, 20] != U and D[100, 100] != U  # all four rooms
    assert D[100, 100] > D[20, 100] and D[100, 100] > D[64, 127] > D[63, 127]           # the last through (127, 64)
    shut = c["grid"].copy()
    shut[64, 127] = 100
    assert no.field_heap(shut, c["goals"], c["spec"])[100, 100] == U                    # and through nothing else


# ---- the corner rule where the diagonal crosses a tile corner -------------------------------------------------------------
def corner_case(blocked):
    """130 x 130, open, the goal at (64, 64), the first cell of tile (1, 1).  The step from (63, 63) to it passes
    between (64, 63) and (63, 64), which lie in two more tiles: for tile (0, 0) the neighbour is the halo's corner
    word and the two cells are halo edge cells.  blocked: '', 'x' ((64, 63) lethal), 'y' ((63, 64)), 'xy'."""
    g = np.zeros((130, 130), np.int8)
    if "x" in blocked:
        g[63, 64] = 100
    if "y" in blocked:
        g[64, 63] = 100
    return case(f"corner_{blocked or 'open'}", g, [64 * 130 + 64])


def corner_regime():
    assert want(corner_case(""))[63, 63] == 350                    # the diagonal: 7 * 50
    for b in ("x", "y"):
        c = corner_case(b)
        D = want(c)
        assert D[63, 63] == 500                                    # refused: around, 5 * 50 twice
        assert c["grid"][63, 63] == 0 and D[64, 64] == 0            # ... by the corner rule alone
    assert want(corner_case("xy"))[63, 63] > 500


# ---- unknown cells, lethal 100 against 99, factor 0 -----------------------------------------------------------------------
def cost_cases():
    g = random_grid(11, 100, 70, free=0.6)
    g[30:40, 20:60] = -1  # a lake of unknown cells between the goal and the far side
    g[35, 5] = 0
    goal = [35 * 100 + 5]
    return {
        "unknown_shut": case("unknown_shut", g, goal),
        "unknown_open": case("unknown_open", g, goal, unknown_cost=200),
        "lethal100": case("lethal100", g, goal, lethal=100),
        "factor0": case("factor0", g, goal, factor=0),
        "dear": case("dear", g, goal, neutral=255, factor=16, unknown_cost=2047, lethal=100),
    }


def costs_regime():
    cs = cost_cases()
    shut, opened = want(cs["unknown_shut"]), want(cs["unknown_open"])
    lake = cs["unknown_shut"]["grid"] < 0
    assert (shut[lake] == U).all() and (opened[lake] != U).any() and (opened <= shut).all()
    g = cs["lethal100"]["grid"]
    assert (g == 99).any() and (want(cs["lethal100"])[g == 99] != U).any() and (shut[g == 99] == U).all()
    flat = want(cs["factor0"])
    assert (flat[flat != U] % 50 == 0).all() and (flat != shut).any()
    dear = want(cs["dear"])  # the greatest weights the check lets through: 255 + 16 * 99 and 2047
    assert int(dear[dear != U].max()) > 5 * int(shut[shut != U].max()) // 2


# ---- the cap, inside a tile and exactly on a tile border --------------------------------------------------------------------
def cap_case(last_x):
    """130 x 70, open, every cell of column 0 a goal: D = 250 x.  cap = 250 last_x keeps columns 0 .. last_x."""
    g = np.zeros((70, 130), np.int8)
    return case(f"cap{last_x}", g, [y * 130 for y in range(70)], cap=250 * last_x)


def cap_regime():
    for last_x in (40, 63, 64):
        D = want(cap_case(last_x))
        assert (D[:, :last_x + 1] == 250 * np.arange(last_x + 1)).all() and (D[:, last_x + 1:] == U).all()
    rnd = cost_cases()["unknown_open"]
    c = case("cap_random", rnd["grid"], rnd["goals"], unknown_cost=200, cap=9000)
    D, full = want(c), want(rnd)
    assert ((D == U) & (full != U)).any() and (D != U).sum() > 100       # it cuts some and keeps some
    assert (D[D != U] == full[D != U]).all() and (full[D == U] > 9000).all()  # and cutting is consistent
    return c


# ---- the serpentine -------------------------------------------------------------------------------------------------------
def serpentine_case():
    """130 x 130: walls along every fourth row with a gap of three cells at alternating ends, so the corridors, three
    cells high, cross the tile borders at x = 64 and x = 128 once in every four rows; the goal in the first corner."""
    g = np.zeros((130, 130), np.int8)
    for i, y in enumerate(range(3, 130, 4)):
        g[y, :] = 100
        if i % 2 == 0:
            g[y, 127:] = 0
        else:
            g[y, :3] = 0
    return case("serpentine", g, [0])


def serpentine_regime():
    c = serpentine_case()
    D = want(c)
    assert (D[c["grid"] == 0] != U).all()
    far = int(D[129, 129 if (len(range(3, 130, 4)) % 2 == 0) else 0])
    assert int(D[D != U].max()) >= 30 * 120 * 250 and far != U  # some thirty corridors of a hundred cells and more
    rows = [int(D[y, 64]) for y in range(1, 130, 4)]
    assert rows == sorted(rows)  # every corridor crosses the border x = 64 later than the one above


# ---- the corridor: more tiles from the goal than rounds -------------------------------------------------------------------
def corridor_case(rounds):
    g = np.zeros((3, 330), np.int8)
    return case("corridor", g, [330], rounds=rounds)


def corridor_regime():
    D = want(corridor_case(2))
    assert D[1, 329] == 250 * 329 and (D != U).all() and -(-330 // TILE) == 6


# ---- three grids in one call ----------------------------------------------------------------------------------------------
def batch_cases():
    """Three 65 x 70 grids that share a spec: random walls, the doors' corner, an empty grid without a goal in range."""
    W, H = 65, 70
    a = random_grid(21, W, H)
    a[5, 5] = 0
    b = np.zeros((H, W), np.int8)
    b[:, 63] = 100
    b[64, 63] = 0
    c = random_grid(23, W, H, free=0.5)
    return [case("batch0", a, [5 * W + 5, 69 * W + 64]), case("batch1", b, [0, W * H + 1]),
            case("batch2", c, [W * H])]


def batch_regime():
    cs = batch_cases()
    assert (want(cs[0]) != U).sum() > 1000 and want(cs[1])[10, 64] != U and (want(cs[2]) == U).all()
    assert len({c["spec"]["rounds"] for c in cs}) == 1


# ---- path starts ------------------------------------------------------------------------------------------------------------
def path_starts(c, S, seed=3):
    """S starts over a case: the goal, a wall or unreached cell, out of range, then random cells."""
    W, H = c["spec"]["width"], c["spec"]["height"]
    D = want(c)
    rng = np.random.default_rng(seed)
    unreached = np.flatnonzero(D.reshape(-1) == U)
    fixed = [c["goals"][0], int(unreached[0]) if len(unreached) else W * H, W * H, 0xFFFFFFFF]
    rest = rng.integers(0, W * H, max(S - len(fixed), 0)).tolist()
    return (fixed + rest)[:S] if S >= len(fixed) else [int(np.argmax(np.where(D == U, 0, D)))][:S]


ALL_FIELDS = ("sizes", "goals", "border_goals", "doors", "corner", "costs", "cap", "serpentine", "corridor", "batch")


def all_cases():
    """Every case of this file, for the tests that hold the writers and the host twin to one another."""
    out = [size_case(W, H) for W, H in SIZES] + list(goal_cases().values()) + list(border_goal_cases().values())
    out += [doors_case()]
    out += [corner_case(b) for b in ("", "x", "y", "xy")] + list(cost_cases().values())
    out += [cap_case(x) for x in (40, 63, 64)] + [cap_regime(), serpentine_case(), corridor_case(2)] + batch_cases()
    return out
