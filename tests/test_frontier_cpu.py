"""E29 without a device: the symbols and constants against the header, the check and the defaults of
rplgpu_frontiers_t, the scratch size, an answer known by hand, the two writers of tests/frontier_oracle.py against each
other on every case of tests/frontier_cases.py, and the host twin rplgpu_frontiers_host (ctypes) against the oracle,
with its refusals."""
import pathlib
import re

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import frontier_cases as fc
from tests import frontier_oracle as fo

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "rplgpu_msg.h"
FILL = 0x5A5A5A5A


def _host(c, **kw):
    a = dict(comp_cap=c["comp_cap"], row_cap=c["row_cap"], row_fill=FILL, goal_fill=FILL)
    a.update(kw)
    return abi.frontiers_host(fo.struct_of(c["spec"]), c["grid"], c["potential"], **a)


def _same(got, want, name):
    assert got["result"].tolist() == want["result"].tolist(), (name, got["result"], want["result"])
    assert got["labels"].tobytes() == want["labels"].tobytes(), name
    assert got["rows"].tobytes() == want["rows"].tobytes(), name
    assert int(got["n_goal"][0]) == want["n_goal"], name
    assert int(got["goal"][0]) == (FILL if want["goal"] is None else want["goal"]), name


def test_symbols_and_constants_against_the_header():
    text = HEADER.read_text()
    for name in ("rplgpu_default_frontiers", "rplgpu_frontiers_check", "rplgpu_frontiers_scratch_words",
                 "rplgpu_frontiers_host", "rplgpu_frontiers_dev", "rplgpu_frontiers"):
        assert re.search(r"\b%s\(" % name, text) and name in abi.ABI_SYMBOLS and hasattr(abi.load_library(), name)
    define = lambda n: int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u" % n, text).group(1), 0)  # noqa: E731
    assert define("RPLGPU_FRONTIER_WORDS") == abi.FRONTIER_WORDS == 16
    assert define("RPLGPU_FRONTIER_ROW_WORDS") == abi.FRONTIER_ROW_WORDS == 8
    assert define("RPLGPU_FRONTIER_MAX_COMPS") == abi.FRONTIER_MAX_COMPS == fo.MAX_COMPS == 1 << 20
    assert define("RPLGPU_FRONTIER_NO_LABEL") == abi.FRONTIER_NO_LABEL == fo.NO_LABEL
    flags = [define("RPLGPU_FRONTIER_" + n) for n in ("NONE", "NO_KEPT", "BOUND", "LOOP")]
    assert flags == [abi.FRONTIER_NONE, abi.FRONTIER_NO_KEPT, abi.FRONTIER_BOUND, abi.FRONTIER_LOOP] == [1, 2, 4, 8]
    assert [fo.NONE, fo.NO_KEPT, fo.BOUND, fo.LOOP] == flags and fo.UNREACHED == abi.NAV_UNREACHED
    fields = re.search(r"typedef struct rplgpu_frontiers \{(.*?)\} rplgpu_frontiers_t;", text, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [n for n, _ in abi.Frontiers._fields_] == list(fo.spec())


def test_default_and_check():
    d = abi.Frontiers.defaults()
    assert (d.width, d.height, d.lethal, d.min_size, d.dist_weight, d.size_weight) == (1024, 1024, 99, 8, 1, 0)
    assert d.check() == abi.OK and abi.load_library().rplgpu_frontiers_check(None) == abi.ERR_INVALID_ARG
    abi.load_library().rplgpu_default_frontiers(None)
    good = fo.spec(width=65, height=3)
    for kw in [dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(lethal=0), dict(lethal=101),
               dict(min_size=0), dict(dist_weight=65536), dict(size_weight=65536), dict(size_weight=0xFFFFFFFF)]:
        s = dict(good, **kw)
        assert not fo.spec_valid(s) and fo.struct_of(s).check() == abi.ERR_INVALID_ARG, kw
        with pytest.raises(abi.RplGpuError):
            abi.frontiers_check(fo.struct_of(s))
    for kw in [dict(width=1, height=1), dict(width=4096, height=4096), dict(lethal=1), dict(lethal=100),
               dict(min_size=1), dict(min_size=0xFFFFFFFF), dict(dist_weight=0, size_weight=0),
               dict(dist_weight=65535, size_weight=65535)]:
        s = dict(good, **kw)
        assert fo.spec_valid(s) and fo.struct_of(s).check() == abi.OK, kw
    abi.frontiers_check(fo.struct_of(good))


def test_scratch_words():
    s = fo.spec(width=129, height=67)  # 8643 cells: 9 counts -> 12, the planes 8644 each
    for G, cap in ((1, 1), (2, 7), (3, 4096), (100, 1 << 20)):
        words = abi.frontiers_scratch_words(fo.struct_of(s), G, cap)
        assert words == fo.scratch_words(s, G, cap) == G * (16 + 12 + 2 * 8644 + 8 * cap)
    assert abi.frontiers_scratch_words(fo.struct_of(fo.spec(width=1, height=1)), 1, 1) == 16 + 4 + 8 + 8
    big = fo.spec(width=4096, height=4096)  # G x tiles at most RPLGPU_NAV_MAX_TILES = 2^23
    assert abi.frontiers_scratch_words(fo.struct_of(big), 2048, 1) == fo.scratch_words(big, 2048, 1) > 0
    for G, cap in ((2049, 1), (65535, 1), (0, 1), (65536, 1), (1, 0), (1, (1 << 20) + 1)):
        assert abi.frontiers_scratch_words(fo.struct_of(big), G, cap) == fo.scratch_words(big, G, cap) == 0
    assert abi.frontiers_scratch_words(fo.struct_of(dict(s, lethal=0)), 1, 1) == 0


def test_known_answer_by_hand():
    """6 x 5, lethal 99, min_size 2; '?' unknown, '.' free, '#' 100; cell index = 6 y + x:

        y 0   . . ? . # .      the unknown cells are (2,0) and (5,3)
        y 1   . . . . # .      frontier cells beside (2,0): (1,0) = 1, (3,0) = 3, (2,1) = 8
        y 2   . . . . # .      frontier cells beside (5,3): (5,2) = 17, (4,3) = 22, (5,4) = 29        F = 6
        y 3   # # # . . ?      {1, 3, 8}: 1 - 8 and 3 - 8 are diagonal neighbours (1 and 3 are not neighbours)
        y 4   . . # . . .      {17, 22, 29}: 17 - 22 and 22 - 29 are diagonal neighbours                N = 2

    label 1: n 3, sum cx 1 + 3 + 2 = 6, sum cy 0 + 0 + 1 = 1; label 17: n 3, sum cx 5 + 4 + 5 = 14, sum cy 2 + 3 + 4 = 9.
    D = 10 x + y + 1: label 1 holds 11, 31, 22 -> Dmin 11 at cell 1; label 17 holds 53, 44, 55 -> Dmin 44 at cell 22.
    Both are kept (n 3 >= 2), BEST by dist_weight 1 is label 1 at cost 11; rows {label, n, sum cx (2), sum cy (2),
    Dmin, cell} = {1, 3, 6, 0, 1, 0, 11, 1} and {17, 3, 14, 0, 9, 0, 44, 22}; the goal is cell 1."""
    text = ["..?.#.", "....#.", "....#.", "###..?", "..#..."]
    grid = np.array([[{".": 0, "?": -1, "#": 100}[ch] for ch in row] for row in text], np.int8)
    pot = np.array([[10 * x + y + 1 for x in range(6)] for y in range(5)], np.uint32)
    s = fo.spec(width=6, height=5, min_size=2)
    rows = [[1, 3, 6, 0, 1, 0, 11, 1], [17, 3, 14, 0, 9, 0, 44, 22]]
    result = [0, 6, 2, 2, 0, 1, 3, 11, 1, 6, 0, 1, 0, 3, 2, 0]
    labels = np.full(30, fo.NO_LABEL, np.uint32)
    labels[[1, 3, 8]] = 1
    labels[[17, 22, 29]] = 17
    for writer in (fo.frontiers_walk, fo.frontiers_arrays):
        w = writer(grid, pot, s, 16, 4, FILL)
        assert w["comps"].tolist() == rows and w["result"].tolist() == result and w["goal"] == 1
        assert w["labels"].reshape(-1).tolist() == labels.tolist()
        assert w["rows"][:2].tolist() == rows and (w["rows"][2:] == FILL).all()
    got = abi.frontiers_host(fo.struct_of(s), grid, pot, comp_cap=16, row_cap=4, row_fill=FILL, goal_fill=FILL)
    assert got["result"].tolist() == result and got["rows"][:2].tolist() == rows and (got["rows"][2:] == FILL).all()
    assert got["labels"].reshape(-1).tolist() == labels.tolist() and got["goal"][0] == 1 and got["n_goal"][0] == 1
    # min_size 4 drops both: six dropped cells, no BEST, the goal word untouched
    got = abi.frontiers_host(fo.struct_of(dict(s, min_size=4)), grid, pot, comp_cap=16, row_cap=4, goal_fill=FILL)
    assert got["result"].tolist() == [fo.NO_KEPT, 6, 2, 0, 6, fo.NO_LABEL, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0]
    assert got["goal"][0] == FILL and got["n_goal"][0] == 0
    # comp_cap 1 < N: the bound
    got = abi.frontiers_host(fo.struct_of(s), grid, pot, comp_cap=1, row_cap=4, row_fill=FILL, goal_fill=FILL)
    assert got["result"].tolist() == [fo.BOUND | fo.NO_KEPT, 6, 2, 0, 0, fo.NO_LABEL, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert (got["rows"] == FILL).all() and got["labels"].reshape(-1).tolist() == labels.tolist()


def test_regimes():
    """The oracle alone: passes without the library."""
    fc.sizes_regime()
    fc.seams_regime()
    fc.chains_regime()
    fc.counts_regime()
    fc.potential_regime()
    fc.cost_regime()
    w = fc.want(fc.room_case())
    assert w["result"][3] >= 2 and w["result"][0] == 0  # the corridor's far end and the unseen patch


@pytest.mark.parametrize("c", fc.all_cases(), ids=lambda c: f"{c['name']}-{c['comp_cap']}-{c['row_cap']}")
def test_writers_and_host_twin(c):
    walk = fc.want(c)
    arrays = fo.frontiers_arrays(c["grid"], c["potential"], c["spec"], c["comp_cap"], c["row_cap"], FILL)
    assert fo.same(walk, arrays), c["name"]
    _same(_host(c), walk, c["name"])
    if c["potential"] is not None:  # without labels, rows and goal outputs the result words are the same
        got = abi.frontiers_host(fo.struct_of(c["spec"]), c["grid"], c["potential"], comp_cap=c["comp_cap"],
                                 row_cap=0, labels=False)
        want = walk["result"].copy()
        want[14] = 0
        assert got["result"].tolist() == want.tolist()


def test_host_twin_refusals_write_nothing():
    lib = abi.load_library()
    c = fc.seam_cases()["vertical"]
    grid = c["grid"]
    labels = np.full(grid.size, FILL, np.uint32)
    rows = np.full(32, FILL, np.uint32)
    goal, n_goal, result = (np.full(n, FILL, np.uint32) for n in (1, 1, 16))

    def call(spec=None, grid_p=grid.ctypes.data, comp_cap=16, rows_p=rows.ctypes.data, row_cap=4,
             goal_p=goal.ctypes.data, n_p=n_goal.ctypes.data, result_p=result.ctypes.data):
        import ctypes as C
        s = fo.struct_of(spec or c["spec"])
        return lib.rplgpu_frontiers_host(C.byref(s), grid_p, 0, comp_cap, labels.ctypes.data, rows_p, row_cap, goal_p,
                                         n_p, result_p)

    for kw in [dict(spec=dict(c["spec"], lethal=0)), dict(spec=dict(c["spec"], min_size=0)), dict(grid_p=0),
               dict(comp_cap=0), dict(comp_cap=(1 << 20) + 1), dict(rows_p=0), dict(goal_p=0), dict(n_p=0),
               dict(result_p=0)]:
        assert call(**kw) == abi.ERR_INVALID_ARG, kw
    for a in (labels, rows, goal, n_goal, result):
        assert (a == FILL).all()
    assert call() == abi.OK and result[2] == 1 and n_goal[0] == 1
    assert call(rows_p=0, row_cap=0) == abi.OK and call(goal_p=0, n_p=0) == abi.OK
