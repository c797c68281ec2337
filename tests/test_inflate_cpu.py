"""E12 without a device: rplgpu_inflation_check and rplgpu_inflation_table of include/rplgpu_msg.h against
tests/inflate_oracle.py, hand-written known answers, the oracle's two writers against each other on every
input of tests/test_gpu_inflate.py, and the regime of every such input."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import inflate_cases as ic
from tests import inflate_oracle as io

SYMBOLS = ("rplgpu_default_inflation", "rplgpu_inflation_check", "rplgpu_inflation_table",
           "rplgpu_inflate_grids_dev", "rplgpu_inflate_grid")


def test_symbols_and_struct():
    lib = abi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in abi.ABI_SYMBOLS
    assert C.sizeof(abi.Inflation) == 16 and abi.MAX_INFLATION_CELLS == 64 == io.MAX_CELLS
    assert lib.rplgpu_abi_version() == 1


def test_defaults():
    f = abi.Inflation.defaults()
    assert (np.float32(f.inscribed_radius), np.float32(f.inflation_radius), np.float32(f.cost_scaling_factor),
            f.inflate_unknown) == (np.float32(0.22), np.float32(0.55), np.float32(3.0), 0)
    abi.inflation_check(f, 0.05)
    table, rc = abi.inflation_table(f, 0.05)
    assert rc == 12 == io.reach(0.55, 0.05) and len(table) == 145  # 12, not 11: (double)0.55f / (double)0.05f > 11
    assert float(np.float32(0.55)) / float(np.float32(0.05)) > 11.0
    assert abi.load_library().rplgpu_inflation_check(None, 0.05) == abi.ERR_INVALID_ARG


BAD = [
    (dict(inscribed_radius=float("nan")), 0.05), (dict(inflation_radius=float("inf")), 0.05),
    (dict(cost_scaling_factor=float("nan")), 0.05), ({}, float("nan")), ({}, float("inf")),
    (dict(inscribed_radius=-0.1), 0.05), (dict(inflation_radius=-0.5, inscribed_radius=-1.0), 0.05),
    (dict(cost_scaling_factor=-1.0), 0.05), ({}, 0.0), ({}, -0.05),
    (dict(inflation_radius=0.2), 0.05),  # below the inscribed radius
    (dict(inflate_unknown=2), 0.05),
    (dict(inflation_radius=3.25), 0.05),  # Rc = 65
    (dict(inflation_radius=3.2001), 0.05),
]


@pytest.mark.parametrize("kw,res", BAD)
def test_check_refuses(kw, res):
    f = abi.Inflation.defaults(**kw)
    assert not io.spec_valid(f.inscribed_radius, f.inflation_radius, f.cost_scaling_factor, f.inflate_unknown, res)
    with pytest.raises(abi.RplGpuError) as e:
        abi.inflation_check(f, res)
    assert e.value.code == abi.ERR_INVALID_ARG
    with pytest.raises(abi.RplGpuError) as e:
        abi.inflation_table(f, res)
    assert e.value.code == abi.ERR_INVALID_ARG


GOOD = [
    ({}, 0.05, 12), (dict(inflation_radius=3.2, inscribed_radius=0.3), 0.05, 64),
    (dict(inscribed_radius=0.0, inflation_radius=0.0), 0.05, 0), (dict(inflation_radius=0.22), 0.05, 5),
    (dict(cost_scaling_factor=0.0, inflate_unknown=1), 0.05, 12), (dict(inflation_radius=0.6), 0.05, 13),
]


@pytest.mark.parametrize("kw,res,rc", GOOD)
def test_check_accepts(kw, res, rc):
    f = abi.Inflation.defaults(**kw)
    assert io.spec_valid(f.inscribed_radius, f.inflation_radius, f.cost_scaling_factor, f.inflate_unknown, res)
    abi.inflation_check(f, res)
    assert abi.inflation_table(f, res)[1] == rc == io.reach(f.inflation_radius, res)


@pytest.mark.parametrize("rc", [12, 64, 4, 5, 0])
def test_table_equals_numpy(rc):
    res, ins, inf, sc = ic.SPECS[rc]
    want, raw = io.table_values(ins, inf, sc, res)
    used = raw[~np.isnan(raw)]
    # equality of truncated values is only owed where 98 exp(..) is not within libm-versus-numpy distance
    # (about 1e-14) of an integer: asserted, not assumed
    margin = float(np.min(np.abs(used - np.round(used)))) if len(used) else 1.0
    print(f"rc {rc}: {len(want)} entries, smallest distance to an integer {margin:.3g}")
    assert margin >= 1e-9
    got = ic.lib_table(rc)
    assert len(got) == rc * rc + 1 == len(want) and got[0] == 100
    assert got.tobytes() == want.tobytes()
    assert (np.diff(got.astype(int)) <= 0).all() and got[1:].max(initial=0) <= 99


def test_table_capacity():
    lib = abi.load_library()
    f = abi.Inflation.defaults()
    buf = np.full(200, 7, np.uint8)
    reach = np.zeros(1, np.uint32)
    assert lib.rplgpu_inflation_table(C.byref(f), 0.05, buf.ctypes.data, 144, reach.ctypes.data) == abi.ERR_CAPACITY
    assert reach[0] == 12 and (buf == 7).all()
    assert lib.rplgpu_inflation_table(C.byref(f), 0.05, buf.ctypes.data, 145, None) == abi.OK
    assert buf[0] == 100 and (buf[145:] == 7).all()
    assert lib.rplgpu_inflation_table(C.byref(f), 0.05, None, 145, None) == abi.ERR_INVALID_ARG


def test_known_table_entries():
    """Worked out by hand from the header's formula."""
    t2 = ic.lib_table(2)  # resolution 1, inscribed 1, scaling 1: 98 exp(-(sqrt k - 1))
    assert t2.tolist() == [100, 99, int(98 * math.exp(1 - math.sqrt(2))), int(98 * math.exp(1 - math.sqrt(3))), 36]
    assert t2.tolist() == [100, 99, 64, 47, 36]
    t5 = ic.lib_table(5)  # 0.05 m cells, inscribed 0.175 m = 3.5 cells: sqrt(12) cells are inside, sqrt(13) are not
    assert t5[12] == 99 and t5[13] == int(98 * math.exp(-3 * (math.sqrt(13) * 0.05 - 0.175))) == 96
    assert t5[25] == 78  # 98 exp(-3 * 0.075) = 78.25
    assert ic.lib_table(0).tolist() == [100] and ic.lib_table(1).tolist() == [100, 99]


@pytest.mark.parametrize("writer", [io.d2_brute, io.d2_separable])
def test_single_lethal_cell_rc2(writer):
    g = np.zeros((9, 9), np.int8)
    g[4, 4] = 100
    out, cells = io.inflate(g, ic.lib_table(2), 2, 0, writer)
    hood = [[0, 0, 36, 0, 0],
            [0, 64, 99, 64, 0],
            [36, 99, 100, 99, 36],
            [0, 64, 99, 64, 0],
            [0, 0, 36, 0, 0]]
    assert out[2:7, 2:7].tolist() == hood
    rest = out.copy()
    rest[2:7, 2:7] = 0
    assert not rest.any() and cells == (1, 4, 8, 0)


@pytest.mark.parametrize("writer", [io.d2_brute, io.d2_separable])
def test_three_four_five(writer):
    g = np.full((12, 12), -1, np.int8)
    g[2, 3] = 100
    d2 = writer(g, 5)
    assert d2[2 + 4, 3 + 3] == 25 and d2[2 + 3, 3 + 4] == 25 and d2[2 + 4, 3 + 4] == io.NONE and d2[2, 3] == 0
    t = ic.lib_table(5)
    for flag, far in ((0, -1), (1, 78)):
        out, _ = io.combine(g, d2, t, 5, flag)
        assert out[6, 6] == far and out[5, 7] == far and out[6, 7] == -1 and out[2, 3] == 100 and out[2, 6] == 99


def _all_cases():
    out = [(f"tiny{rc}_{i}", c) for rc in (0, 1, 64) for i, c in enumerate(ic.tiny_cases(rc))]
    out += [("edges5", ic.edges_case(5)), ("edges64", ic.edges_case(64)), ("batch", ic.batch_case()),
            ("step", ic.step_case())]
    out += [(f"uniform_{k}", c) for k, c in ic.uniform_cases().items()]
    return out


def test_writers_agree_on_every_case():
    for name, c in _all_cases():
        for g in c["grids"]:
            a, b = io.d2_brute(g, c["rc"]), io.d2_separable(g, c["rc"])
            assert np.array_equal(a, b), name


def test_regimes():
    for rc in (0, 1, 64):
        ic.tiny_regime(rc)
    ic.edges_regime()
    ic.uniform_regime()
    ic.batch_regime()
    ic.step_regime()


def test_linear_table():
    for rc in sorted({64, 3} | set(ic.REACH_RCS) | {rc for _, rc in ic.STAGE_INNER} | {s[2] for s in ic.SHAPES.values()}):
        t = ic.linear_table(rc)
        assert t.dtype == np.uint8 and len(t) == rc * rc + 1 and t[0] == 100
        assert (np.diff(t.astype(int)) <= 0).all() and 1 <= t[1:].min() and t[1:].max() <= 98 and t[-1] == 1
        for k in (1, 2, rc * rc // 2, rc * rc - 1, rc * rc):  # the formula, in integers: floor(97 sqrt(k) / rc) = n
            n = 98 - int(t[k])
            assert n * n * rc * rc <= 97 * 97 * k and (t[k] == 1 or (n + 1) ** 2 * rc * rc > 97 * 97 * k), (rc, k)
    assert len(set(ic.linear_table(64).tolist())) == 98
    assert ic.linear_table(0).tolist() == [100] and ic.linear_table(1).tolist() == [100, 1]


def test_regimes_across_the_window():
    ic.lone_regime()
    ic.stage_regime()
    ic.count_regime()
    ic.shape_regime()


@pytest.mark.parametrize("W,H", ic.REACH_SHAPES)
@pytest.mark.parametrize("rc", ic.REACH_RCS)
def test_reach_regime(rc, W, H):
    ic.reach_regime(rc, W, H)


def _window_cases():
    """(name, case, grids to run the brute writer on): every grid below rc 63, at most 8 grids in all at rc 63 / 64
    (the brute writer takes over a second per 192 x 192 grid there)."""
    out = [(f"lone{W}", ic.lone_case(W), (7 * i,)) for i, W in enumerate(ic.LONE_WIDTHS)]
    for name, c in ic.stage_cases().items():
        out.append((name, c, (0,) if c["rc"] < 63 or name in ("wide124", "wide127") else ()))
    for name, c in ic.reach_cases().items():
        out.append((name, c, (0,) if c["rc"] < 63 or name.endswith("197x131") else ()))
    out += [(f"count{W}_{t}", ic.count_case(W, t), (0,)) for W in ic.COUNT_WIDTHS for t in ic.COUNT_TABLES]
    out += [(name, ic.shape_case(name), (0,)) for name in ic.SHAPES]
    out.append(("many", ic.many_case(), range(ic.MANY_G)))
    return out


def test_writers_agree_across_the_window():
    slow = 0
    for name, c, which in _window_cases():
        slow += len(which) if c["rc"] >= 63 else 0
        for i in which:
            g = c["grids"][i]
            assert np.array_equal(io.d2_brute(g, c["rc"]), io.d2_separable(g, c["rc"])), (name, i)
    assert 1 <= slow <= 8


def test_chain_input_and_writers(oracle):
    from tests import occ_cases as oc
    occ = oc.case_want(oracle, oc.full_case(0), "full0")[0][0]
    c = ic.chain_case(occ)
    ic.chain_regime(c)
    assert np.array_equal(io.d2_brute(occ, 12), io.d2_separable(occ, 12))
