"""E13 without a device: the new symbols, the host-only functions of include/rplgpu_msg.h (spec check, rotation
table, volume size) against tests/match_oracle.py, the oracle's two writers against each other on every case of
tests/match_cases.py, every regime check, and known answers worked out by hand."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import match_cases as mc
from tests import match_oracle as mo

F32 = np.float32


def _struct(s):
    return abi.ScanMatch(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["shift_x"],
                         s["shift_y"], s["rot_steps"], s["rot_step"])


def test_symbols_and_struct():
    lib = abi.load_library()
    for name in ("rplgpu_default_scan_match", "rplgpu_scan_match_check", "rplgpu_scan_match_rotations",
                 "rplgpu_scan_match_volume", "rplgpu_match_scans_dev", "rplgpu_match_scans"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(abi.ScanMatch) == 36
    d = abi.ScanMatch.defaults()
    want = mo.spec()
    for k, v in want.items():
        assert getattr(d, k) == (F32(v) if isinstance(v, float) else v), k
    assert d.rot_step == F32(0.25 * math.pi / 180.0)
    assert abi.ScanMatch.defaults(shift_x=9).shift_x == 9
    with pytest.raises(AttributeError):
        abi.ScanMatch.defaults(shift=1)


HALF_PI_STEP = float(np.nextafter(F32(math.pi / 2 / 64), F32(0)))  # 64 steps of it stay within pi / 2
SPECS = [
    (dict(), True),
    (dict(resolution=0.0), False), (dict(resolution=-0.05), False), (dict(resolution=float("nan")), False),
    (dict(origin_x=float("inf")), False), (dict(origin_y=float("nan")), False), (dict(rot_step=float("inf")), False),
    (dict(width=0), False), (dict(height=0), False),
    (dict(width=4096, height=4096), True), (dict(width=4097), False), (dict(height=4097), False),
    (dict(shift_x=32, shift_y=32), True), (dict(shift_x=33), False), (dict(shift_y=33), False),
    (dict(shift_x=0, shift_y=0), True),
    (dict(rot_steps=64, rot_step=0.02), True), (dict(rot_steps=65, rot_step=0.01), False),
    (dict(rot_steps=0, rot_step=0.0), True), (dict(rot_steps=0, rot_step=-1.0), True),
    (dict(rot_steps=1, rot_step=0.0), False), (dict(rot_steps=1, rot_step=-0.01), False),
    (dict(rot_steps=1, rot_step=float(F32(math.pi / 2))), float(F32(math.pi / 2)) <= math.pi / 2),
    (dict(rot_steps=1, rot_step=float(np.nextafter(F32(math.pi / 2), F32(4)))), False),
    (dict(rot_steps=64, rot_step=HALF_PI_STEP), True),
    (dict(rot_steps=64, rot_step=float(np.nextafter(F32(math.pi / 2 / 64), F32(1)))), False),
    (dict(rot_steps=2, rot_step=1.0), False),
]


@pytest.mark.parametrize("kw,ok", SPECS, ids=[str(i) for i in range(len(SPECS))])
def test_spec_check_matches_the_oracle(kw, ok):
    s = mo.spec(**kw)
    assert mo.spec_valid(s) == ok, s
    lib = abi.load_library()
    m = _struct(s)
    assert (lib.rplgpu_scan_match_check(C.byref(m)) == abi.OK) == ok
    assert abi.scan_match_volume(m) == (mo.volume_size(s) if ok else 0)
    if ok:
        abi.scan_match_check(m)
    else:
        with pytest.raises(abi.RplGpuError) as e:
            abi.scan_match_check(m)
        assert e.value.code == abi.ERR_INVALID_ARG
        with pytest.raises(abi.RplGpuError):
            abi.scan_match_rotations(m)
    assert lib.rplgpu_scan_match_check(None) == abi.ERR_INVALID_ARG


@pytest.mark.parametrize("K", [0, 1, 64])
@pytest.mark.parametrize("step", [float(F32(0.25 * math.pi / 180.0)), 0.02, 1.0e-4, HALF_PI_STEP])
def test_rotation_table_bit_for_bit(K, step):
    s = mo.spec(rot_steps=K, rot_step=step)
    got = abi.scan_match_rotations(_struct(s))
    want = mo.rotations(s)
    assert got.shape == want.shape == (2 * K + 1, 2) and got.tobytes() == want.tobytes()
    assert got[K].tobytes() == np.array([1.0, 0.0], F32).tobytes()  # entry k = 0 is exactly (1, 0)
    assert (got[::-1, 0] == got[:, 0]).all() and (got[::-1, 1] == -got[:, 1]).all()
    assert abi.load_library().rplgpu_scan_match_rotations(C.byref(_struct(s)), None) == abi.ERR_INVALID_ARG


def test_volume_size():
    assert abi.scan_match_volume(abi.ScanMatch.defaults()) == 21 * 13 * 13
    assert abi.scan_match_volume(_struct(mo.spec(shift_x=32, shift_y=32, rot_steps=64, rot_step=0.02))) == 129 * 65 * 65
    assert abi.scan_match_volume(_struct(mo.spec(shift_x=7, shift_y=2, rot_steps=0))) == 15 * 5


# ---- known answers by hand ------------------------------------------------------------------------------------------
def test_one_point_one_cell():
    """One point in cell (10, 10), one field cell of 100 at (12, 9): the volume is a single 100 at the shift that
    brings the point there, i = 2, j = -1."""
    s = mo.spec(origin_x=0.0, origin_y=0.0, resolution=0.25, width=32, height=32, shift_x=3, shift_y=3, rot_steps=0,
                rot_step=0.0)
    field = np.zeros((32, 32), np.int8)
    field[9, 12] = 100
    x, y = np.array([2.625], F32), np.array([2.625], F32)
    for writer in (mo.scores_gather, mo.scores_correlate):
        vol, best, status = mo.match_points(x, y, None, s, field, writer)
        want = np.zeros((1, 7, 7), np.uint32)
        want[0, -1 + 3, 2 + 3] = 100
        assert np.array_equal(vol, want) and status == 0
        assert tuple(best) == (100, 0, -1, 2, 1, 0, 1, 0)


def test_bytes_and_borders_by_hand():
    """A point in the corner cell (0, 0) of a 2 x 2 field [[127, -128], [-1, 7]] with T 1: only the four shifts
    that stay inside read a byte, negative bytes give 0; a NaN point is ignored, a point 1e9 m away has no cell."""
    s = mo.spec(origin_x=0.0, origin_y=0.0, resolution=1.0, width=2, height=2, shift_x=1, shift_y=1, rot_steps=0,
                rot_step=0.0)
    field = np.array([[127, -128], [-1, 7]], np.int8)
    x, y = np.array([0.5, np.nan, 1.0e9], F32), np.array([0.5, 0.5, 0.5], F32)
    for writer in (mo.scores_gather, mo.scores_correlate):
        vol, best, status = mo.match_points(x, y, None, s, field, writer)
        assert vol.tolist() == [[[0, 0, 0], [0, 127, 0], [0, 0, 7]]]
        assert status == mo.SCAN_CELL_RANGE and tuple(best) == (127, 0, 0, 0, 2, 127, 1, 0)


def test_rotation_by_hand():
    """A quarter turn about (1, 1) takes the point (3, 1) to (1, 3) and (1, -1): K 1 with a step of pi / 2."""
    s = mo.spec(origin_x=-4.0, origin_y=-4.0, resolution=1.0, width=8, height=8, shift_x=0, shift_y=0, rot_steps=1,
                rot_step=float(F32(math.pi / 2)))
    if not mo.spec_valid(s):  # (float)(pi / 2) rounds above pi / 2: one ulp less
        s["rot_step"] = float(np.nextafter(F32(math.pi / 2), F32(0)))
    field = np.zeros((8, 8), np.int8)
    field[4 + 3, 4 + 1], field[4 - 1, 4 + 1], field[4 + 1, 4 + 3] = 30, 20, 10  # (x, y) = (1, 3), (1, -1), (3, 1)
    field[4 - 2, 4 + 1] = 20  # whichever side of the cell border the rounded rotation lands on
    x, y = np.array([3.25], F32), np.array([1.25], F32)
    vol, best, _ = mo.match_points(x, y, (1.25, 1.25), s, field, mo.scores_gather)
    assert vol.ravel().tolist() == [20, 10, 30] and tuple(best[:4]) == (30, 1, 0, 0)


def test_tie_rule_by_hand():
    s = mo.spec(shift_x=2, shift_y=2, rot_steps=2, rot_step=0.1)
    vol = np.zeros(mo.volume_shape(s), np.uint32)
    assert tuple(mo.best_of(vol, s, 0)) == (0, 0, 0, 0, 0, 0, 125, 0)
    vol[2 + 1, 2, 2] = vol[2 - 1, 2, 2] = vol[2 + 0, 2, 2 + 1] = 9   # k = +-1 at no shift beat k = 0 at i = 1
    assert tuple(mo.best_of(vol, s, 3)[:4]) == (9, -1, 0, 0)
    vol[:] = 0
    vol[2 + 2, 2, 2] = vol[2 - 1, 2 + 1, 2] = 9                       # i*i + j*j before |k|
    assert tuple(mo.best_of(vol, s, 3)[:4]) == (9, 2, 0, 0)
    vol[:] = 0
    vol[2, 2 + 1, 2 - 2] = vol[2, 2 - 1, 2 + 2] = vol[2, 2 - 1, 2 - 2] = vol[2, 2 + 2, 2 - 1] = 9
    assert tuple(mo.best_of(vol, s, 3)[:4]) == (9, 0, -1, -2) and mo.best_of(vol, s, 3)[6] == 4
    assert mo.best_words([5, -1, -2, 3, 0, 0, 1, 0]).tolist() == [5, 0xFFFFFFFF, 0xFFFFFFFE, 3, 0, 0, 1, 0]


# ---- the cases: regimes, and the two writers ----------------------------------------------------------------------------
def _writers_agree(oracle, case, key):
    a = mc.case_want(oracle, case, key)
    b = mc.case_want(oracle, case, None, writer=mo.scores_gather)
    assert len(a) == len(b)
    for (va, ba, sa), (vb, bb, sb) in zip(a, b):
        assert np.array_equal(va, vb) and np.array_equal(ba, bb) and sa == sb


@pytest.mark.parametrize("disp", mc.ROOM_DISPLACEMENTS, ids=[str(d) for d in mc.ROOM_DISPLACEMENTS])
def test_room_recovers_the_displacement(oracle, disp):
    case = mc.room_case(oracle, disp)
    mc.room_regime(oracle, case)
    _writers_agree(oracle, case, f"room{disp}")


def test_displacement_inverse_is_a_candidate():
    """displaced_poses followed by candidate (-k0, -j0, -i0) is the identity on the poses (to float32 rounding)."""
    _, _, pose2d = mc.room_scans()
    s, pv = mc.ROOM_SPEC, mc.ROOM_PIVOT[0].astype(float)
    for k0, j0, i0 in mc.ROOM_DISPLACEMENTS:
        d = mo.displaced_poses(pose2d, pv, s, k0, j0, i0).astype(float)
        a = -k0 * float(F32(s["rot_step"]))
        c, sn = math.cos(a), math.sin(a)
        for got, want in zip(d, pose2d.astype(float)):
            qx, qy = got[2] - pv[0], got[5] - pv[1]
            tx = c * qx - sn * qy + pv[0] - i0 * 0.05
            ty = sn * qx + c * qy + pv[1] - j0 * 0.05
            assert abs(tx - want[2]) < 1e-5 and abs(ty - want[5]) < 1e-5
            assert abs(c * got[0] - sn * got[3] - want[0]) < 1e-6


@pytest.mark.parametrize("name", sorted(mc.tie_cases()))
def test_tie_cases(oracle, name):
    case, expect, equals = mc.tie_cases()[name]
    mc.tie_regime(oracle, name, case, expect, equals)
    _writers_agree(oracle, case, f"tie_{name}")


@pytest.mark.parametrize("name", sorted(mc.edge_cases()))
def test_edge_cases(oracle, name):
    case = mc.edge_cases()[name]
    mc.edge_regime(oracle, name, case)
    _writers_agree(oracle, case, f"edge_{name}")


def test_passes_and_weights(oracle):
    case = mc.passes_case()
    mc.passes_regime(oracle, case)
    _writers_agree(oracle, case, "passes")
    case = mc.weights_case()
    mc.weights_regime(oracle, case)
    _writers_agree(oracle, case, "weights")


@pytest.mark.parametrize("per_group", [0, 1])
def test_groups(oracle, per_group):
    case = mc.groups_case(per_group)
    want = mc.groups_regime(oracle, case, f"groups{per_group}")
    _writers_agree(oracle, case, f"groups{per_group}")
    if per_group:  # different fields per group give different volumes than one shared field
        shared = mc.case_want(oracle, mc.groups_case(0), "groups0")
        assert np.array_equal(shared[0][0], want[0][0]) and (shared[1][0] != want[1][0]).any()


def test_front_end(oracle):
    case = mc.front_case()
    mc.front_regime(oracle, case)
    _writers_agree(oracle, case, "front")
