"""The cases of tests/match_path_cases.py without a device: every regime check, the oracle's two writers against
each other where both are cheap, and that the window layouts cover what they claim."""
import numpy as np
import pytest

from tests import match_cases as mc
from tests import match_oracle as mo
from tests import match_path_cases as mp


def _writers_agree(oracle, case, key):
    a = mc.case_want(oracle, case, key)
    b = mc.case_want(oracle, case, None, writer=mo.scores_gather)
    assert len(a) == len(b)
    for (va, ba, sa), (vb, bb, sb) in zip(a, b):
        assert np.array_equal(va, vb) and np.array_equal(ba, bb) and sa == sb


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", sorted(mp.LONG_LENS))
def test_long_scans_need_their_second_pass(oracle, stride):
    case = mp.long_case(stride)
    mp.long_regime(oracle, case, mp.long_key(stride))
    _writers_agree(oracle, case, mp.long_key(stride))


def test_long_scans_wide_window(oracle):
    case = mp.long_case(32768, wide=True)
    assert mp.layout_of(16, 16)[0] > 1024
    mp.long_regime(oracle, case, mp.long_key(32768, True))


def test_long_front_end(oracle):
    mp.long_front_regime(oracle, mp.long_front_case())


# ---- B ------------------------------------------------------------------------------------------------------------------
def test_layouts_cover_the_kernel():
    """Every `per` from 64 to 1024, every number of copies, both sides of 1024 candidates, 1 to 5 candidates per
    thread, rows of 65 and of 1, Tx != Ty on the wide path."""
    lay = {t: mp.layout_of(*t) for t in mp.LAYOUTS}
    assert len(set(mp.LAYOUTS)) == len(mp.LAYOUTS)
    assert {v[1] for v in lay.values()} == set(range(64, 1025, 64))
    assert {v[2] for v in lay.values() if v[0] <= 1024} == {1, 2, 3, 4, 5, 8, 16}
    assert {v[3] for v in lay.values()} == {1, 2, 3, 4, 5}
    ncs = sorted(v[0] for v in lay.values())
    assert 1023 in ncs and 1089 in ncs and not any(1023 < n < 1089 for n in ncs)
    assert lay[(32, 31)] == (4095, 1024, 1, 4) and lay[(7, 7)] == (225, 256, 4, 1) and lay[(8, 8)][1:3] == (320, 3)
    assert lay[(11, 10)] == (483, 512, 2, 1) and lay[(11, 11)] == (529, 576, 1, 1) and lay[(32, 7)][0] == 975
    assert (32, 0) in lay and (0, 32) in lay and lay[(32, 0)][0] == 65
    assert any(t[0] != t[1] and v[0] > 1024 for t, v in lay.items())
    for t, (nc, per, slices, owned) in lay.items():
        assert per % 64 == 0 and (nc > 1024 or (nc <= per and slices * per <= 1024 < (slices + 1) * per))
        assert (owned - 1) * 1024 < nc <= owned * 1024


@pytest.mark.parametrize("t", mp.LAYOUTS, ids=[mp.layout_name(t) for t in mp.LAYOUTS])
def test_layout_cases(oracle, t):
    case = mp.layout_case(t)
    mp.layout_regime(oracle, t, case)
    if mp.layout_of(*t)[0] <= 1100:
        _writers_agree(oracle, case, f"layout_{mp.layout_name(t)}")


# ---- C ------------------------------------------------------------------------------------------------------------------
def test_run_palette():
    """The hand-made cells: four distinct ones in a row, two cells apart, each with its own positive byte."""
    f = mp.run_field()[0]
    cells = [mp.cell_of_dist(d) for d in (mp.D_A, mp.D_A2, mp.D_B, mp.D_C)]
    assert cells == [(10, 10), (12, 10), (6, 10), (8, 10)]
    assert len({int(f[cy, cx]) for cx, cy in cells}) == 4 and f.min() >= 1


def test_run_sweep(oracle):
    case = mp.sweep_case()
    assert case["batch"].shape == (65, 2048)
    mp.sweep_regime(oracle, case)
    _writers_agree(oracle, case, "run_sweep")


def test_run_boundaries(oracle):
    case = mp.boundary_case()
    assert case["lengths"] == list(range(2, 131))
    mp.boundary_regime(oracle, case, "run_boundary")
    _writers_agree(oracle, case, "run_boundary")
    k1 = mp.boundary_case(mp.RUN_SPEC_K1, (63, 64, 65, 130))
    mp.boundary_regime(oracle, k1, "run_boundary_k1")


def test_run_across_two_passes(oracle):
    case = mp.two_pass_run_case()
    mp.boundary_regime(oracle, case, "run_two_pass", (mp.TWO_PASS,))


def test_run_broken(oracle):
    case = mp.broken_case()
    mp.broken_regime(oracle, case)
    _writers_agree(oracle, case, "run_broken")


# ---- D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mp.KEY_NAMES)
def test_key_cases(oracle, name):
    case, expect, equals = mp.key_cases()[name]
    mp.key_regime(oracle, name, case, expect, equals)
    if not name.startswith("full_volume"):
        _writers_agree(oracle, case, f"key_{name}")


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mp.BIG))
def test_big_grids(oracle, name):
    mp.big_regime(oracle, name, mp.big_case(name))


# ---- F ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_group", [0, 1])
def test_many_groups(oracle, per_group):
    case = mp.many_case(per_group)
    want = mp.many_regime(oracle, case, f"many{per_group}")
    _writers_agree(oracle, case, f"many{per_group}")
    if per_group:
        shared = mc.case_want(oracle, mp.many_case(0), "many0")
        assert sum(1 for a, b in zip(shared, want) if (a[0] != b[0]).any()) >= 300
