"""E26 without a device: the check and the defaults of rplgpu_nav_field_t, answers known by hand, the two writers of
tests/nav_oracle.py against each other on every case of tests/nav_cases.py, and the host twins rplgpu_nav_field_host
and rplgpu_nav_path_host (ctypes) against the oracle, with the properties a path has by the rules."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import nav_cases as nc
from tests import nav_oracle as no

U = no.UNREACHED


def test_default_and_check():
    d = abi.NavField.defaults()
    assert (d.width, d.height, d.lethal, d.neutral, d.factor, d.unknown_cost, d.cap, d.rounds) == \
        (1024, 1024, 99, 50, 2, 0, abi.NAV_MAX_CAP, 66)
    assert d.check() == abi.OK and abi.load_library().rplgpu_nav_field_check(None) == abi.ERR_INVALID_ARG
    abi.load_library().rplgpu_default_nav_field(None)
    good = no.spec(width=65, height=3)
    refused = [dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(lethal=0), dict(lethal=101),
               dict(neutral=0), dict(neutral=256), dict(factor=17), dict(unknown_cost=2048), dict(cap=0xFFFF0001),
               dict(cap=0xFFFFFFFF), dict(rounds=0), dict(rounds=4097)]
    for kw in refused:
        s = dict(good, **kw)
        assert not no.spec_valid(s) and no.struct_of(s).check() == abi.ERR_INVALID_ARG, kw
        with pytest.raises(abi.RplGpuError):
            abi.nav_field_check(no.struct_of(s))
    edges = [dict(width=1, height=1), dict(width=4096, height=4096), dict(lethal=1), dict(lethal=100),
             dict(neutral=1), dict(neutral=255, factor=16, lethal=100), dict(factor=0), dict(unknown_cost=2047),
             dict(cap=0), dict(cap=0xFFFF0000), dict(rounds=1), dict(rounds=4096)]
    for kw in edges:
        s = dict(good, **kw)
        assert no.spec_valid(s) and no.struct_of(s).check() == abi.OK, kw
    # the ranges keep neutral + factor (lethal - 1) at or below 255 + 16 * 99 = 1839: inside RPLGPU_NAV_MAX_COST
    assert 255 + 16 * 99 <= abi.NAV_MAX_COST


def test_default_rounds_and_scratch_words():
    assert abi.NAV_TILE == no.TILE == nc.TILE == 64
    last = 0
    for n in (1, 63, 64, 65, 128, 129, 1024, 4095, 4096):
        r = abi.nav_field_default_rounds(n, n)
        assert r == no.default_rounds(n, n) == 4 * -(-n // 64) + 2 and r >= last
        last = r
        assert abi.nav_field_default_rounds(n, 1) == 2 * (-(-n // 64) + 1) + 2
    assert abi.nav_field_default_rounds(0, 5) == 0 and abi.nav_field_default_rounds(5, 4097) == 0
    s = no.spec(width=129, height=67)
    words = [abi.nav_field_scratch_words(no.struct_of(s), G) for G in (1, 2, 3, 100)]
    assert words == [2 * 3 * 2 * G for G in (1, 2, 3, 100)]
    assert abi.nav_field_scratch_words(no.struct_of(no.spec(width=64, height=64)), 1) == 2
    big = no.struct_of(no.spec(width=4096, height=4096))  # G x tiles at most RPLGPU_NAV_MAX_TILES = 2^23
    assert abi.NAV_MAX_TILES == 1 << 23 and abi.nav_field_scratch_words(big, 2048) == 2 << 23
    assert abi.nav_field_scratch_words(big, 2049) == 0 and abi.nav_field_scratch_words(big, 65535) == 0
    assert abi.nav_field_scratch_words(no.struct_of(s), 0) == 0
    assert abi.nav_field_scratch_words(no.struct_of(dict(s, lethal=0)), 1) == 0


def test_known_answers_by_hand():
    s = no.spec(width=3, height=3)
    open3 = np.zeros((3, 3), np.int8)
    want = np.array([[350, 250, 350], [250, 0, 250], [350, 250, 350]], np.uint32)
    for writer in (no.field_heap, no.field_graph):
        assert (writer(open3, [4], s) == want).all()
    pot, res = abi.nav_field_host(no.struct_of(s), open3, [4])
    assert (pot == want).all() and res.tolist() == [0, 0, 1, 0, 9, 350, 0, 0]
    # a two-cell diagonal gap: (0, 0) and (1, 1) free, (1, 0) and (0, 1) lethal — no corner cutting
    gap = np.array([[0, 100], [100, 0]], np.int8)
    s2 = no.spec(width=2, height=2)
    for writer in (no.field_heap, no.field_graph):
        assert writer(gap, [3], s2).tolist() == [[U, U], [U, 0]]
    assert abi.nav_field_host(no.struct_of(s2), gap, [3])[0].tolist() == [[U, U], [U, 0]]
    one_side = np.array([[0, 0], [100, 0]], np.int8)  # one of the two is enough to refuse the diagonal
    assert no.field_heap(one_side, [3], s2).tolist() == [[500, 250], [U, 0]]
    # weights: 50 + 2 v, v = 30 -> 110: leaving a dear cell costs its own weight
    row = np.array([[0, 30, 0]], np.int8)
    s3 = no.spec(width=3, height=1)
    assert no.field_heap(row, [0], s3).tolist() == [[0, 550, 800]]
    assert no.field_heap(row, [0], dict(s3, cap=799)).tolist() == [[0, 550, U]]
    assert no.field_heap(np.array([[0, -1, 0]], np.int8), [0], dict(s3, unknown_cost=7)).tolist() == [[0, 35, 285]]


def test_regimes():
    for name in nc.ALL_FIELDS:
        getattr(nc, name + "_regime")()


def test_writers_agree_and_the_host_twin_with_them():
    for c in nc.all_cases():
        a, b = nc.want(c), no.field_graph(c["grid"], c["goals"], c["spec"])
        assert a.tobytes() == b.tobytes(), c["name"]
        pot, res = abi.nav_field_host(no.struct_of(c["spec"]), c["grid"], c["goals"])
        assert pot.tobytes() == a.tobytes(), c["name"]
        assert res.tolist() == [0, 0] + no.result_words(a, c["goals"]) + [0, 0], c["name"]


def test_host_twin_refusals_write_nothing():
    lib = abi.load_library()
    s = no.struct_of(no.spec(width=3, height=3))
    grid, goals = np.zeros(9, np.int8), np.array([4], np.uint32)
    pot, res = np.full(9, 77, np.uint32), np.full(8, 77, np.uint32)
    bad = no.struct_of(no.spec(width=3, height=3, lethal=0))
    import ctypes as C
    for args in ((C.byref(bad), grid.ctypes.data, goals.ctypes.data, 1, pot.ctypes.data, res.ctypes.data),
                 (C.byref(s), 0, goals.ctypes.data, 1, pot.ctypes.data, res.ctypes.data),
                 (C.byref(s), grid.ctypes.data, 0, 1, pot.ctypes.data, res.ctypes.data),
                 (C.byref(s), grid.ctypes.data, goals.ctypes.data, 1, 0, res.ctypes.data)):
        assert lib.rplgpu_nav_field_host(*args) == abi.ERR_INVALID_ARG
    path, info = np.full(4, 77, np.uint32), np.full(4, 77, np.uint32)
    for args in ((C.byref(bad), grid.ctypes.data, pot.ctypes.data, 0, path.ctypes.data, 4, info.ctypes.data),
                 (C.byref(s), grid.ctypes.data, pot.ctypes.data, 0, path.ctypes.data, 0, info.ctypes.data),
                 (C.byref(s), grid.ctypes.data, pot.ctypes.data, 0, 0, 4, info.ctypes.data),
                 (C.byref(s), grid.ctypes.data, pot.ctypes.data, 0, path.ctypes.data, 4, 0)):
        assert lib.rplgpu_nav_path_host(*args) == abi.ERR_INVALID_ARG
    assert (pot == 77).all() and (res == 77).all() and (path == 77).all() and (info == 77).all()
    assert lib.rplgpu_nav_field_host(C.byref(s), grid.ctypes.data, 0, 0, pot.ctypes.data, 0) == abi.OK  # no goal, no result
    assert (pot == U).all()


@pytest.mark.parametrize("name", ["unknown_open", "doors", "serpentine", "goal_many", "cap_random"])
def test_paths_host_twin_and_properties(name):
    c = {x["name"]: x for x in nc.all_cases()}[name]
    field = nc.want(c)
    s, W = c["spec"], c["spec"]["width"]
    starts = nc.path_starts(c, 40, seed=5) + [int(np.argmax(np.where(field == U, 0, field)))]
    seen = 0
    for st in starts:
        cells, info = no.path(c["grid"], field, s, st, 8000)
        path, hinfo = abi.nav_path_host(no.struct_of(s), c["grid"], field, st, 8000, path_fill=77)
        assert hinfo.tolist() == info and path[:len(cells)].tolist() == cells and (path[len(cells):] == 77).all()
        seen |= info[1]
        if info[1] != no.REACHED:
            assert info[0] == 0
            continue
        assert cells[0] == st and field.reshape(-1)[cells[-1]] == 0 and info[3] == cells[-1]
        assert no.path_cost(c["grid"], s, cells) == info[2] == field.reshape(-1)[st]  # every step allowed, the cost D
        d = [int(field.reshape(-1)[x]) for x in cells]
        assert all(a > b for a, b in zip(d, d[1:]))  # D falls strictly
        w = no.weights(c["grid"], s)
        for a, b in zip(cells, cells[1:]):  # the tie rule: no allowed step of a lower number satisfies the equality
            taken = [i for i, (dx, dy, _) in enumerate(no.STEPS) if (dx, dy) == (b % W - a % W, b // W - a // W)][0]
            for k in no.allowed_steps(c["grid"], s, a % W, a // W, w):
                if k >= taken:
                    break
                dn = int(field[a // W + no.STEPS[k][1], a % W + no.STEPS[k][0]])
                assert dn == U or dn + no.STEPS[k][2] * int(w[a // W, a % W]) != int(field.reshape(-1)[a])
        if len(cells) > 2:  # cut short: TRUNCATED, the same cells, nothing behind them
            path, hinfo = abi.nav_path_host(no.struct_of(s), c["grid"], field, st, len(cells) - 1, path_fill=77)
            assert hinfo.tolist() == [len(cells) - 1, no.TRUNCATED, info[2], cells[-2]] and path.tolist() == cells[:-1]
    assert seen & no.REACHED and seen & no.NO_START and (seen & no.PATH_UNREACHED or (field != U).all())


def test_tie_rule_by_hand_and_a_broken_potential():
    s = no.spec(width=3, height=3)
    grid = np.zeros((3, 3), np.int8)
    field = no.field_heap(grid, [1, 3], s)  # (1, 0) and (0, 1): from (1, 1) step 1 (-1, 0) and step 3 (0, -1) tie
    assert field[1, 1] == 250
    cells, info = no.path(grid, field, s, 4, 9)
    assert cells == [4, 3] and info == [2, no.REACHED, 250, 3]  # step 1 before step 3
    path, hinfo = abi.nav_path_host(no.struct_of(s), grid, field, 4, 9)
    assert path[:2].tolist() == [4, 3] and hinfo.tolist() == info
    broken = field.copy()
    broken[1, 1] = 251
    cells, info = no.path(grid, broken, s, 4, 9)
    assert cells == [4] and info == [1, no.BROKEN, 251, 4]
    assert abi.nav_path_host(no.struct_of(s), grid, broken, 4, 9)[1].tolist() == info
