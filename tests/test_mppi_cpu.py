"""E28 without a device: the symbols, the check and the defaults of rplgpu_mppi_t, the answer known by hand, the two
writers of tests/mppi_oracle.py against each other and against the host twins rplgpu_mppi_update_host and
rplgpu_mppi_spread_host (ctypes) on every case of tests/mppi_cases.py, the spread's identity with E16's move through
rplgpu_resample_host, rplgpu_mppi_table's known answers and the host twins' refusals."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import mppi_cases as mc
from tests import mppi_oracle as mo

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["rplgpu_default_mppi", "rplgpu_mppi_check", "rplgpu_mppi_scratch_words", "rplgpu_mppi_table",
           "rplgpu_mppi_update_host", "rplgpu_mppi_update_dev", "rplgpu_mppi_update", "rplgpu_mppi_spread_host",
           "rplgpu_mppi_spread_dev", "rplgpu_mppi_spread"]


def _abi():
    from rplidar_ros2_driver_amd import abi
    return abi


def _host(c):
    return _abi().mppi_update_host(mo.struct_of(c["spec"]), c["out"], c["rres"], c["delta"], c["table"], c["nominal"])


def _all_cases():
    cases = [mc.shape_case(*sh) for sh in mc.SHAPES if sh[0] <= 300]
    cases += list(mc.group_cases(1)) + list(mc.group_cases(0))
    cases += [c for n, c in mc.weight_cases().items() if n != "big_sums"] + list(mc.range_cases().values())
    return cases


def test_regimes_from_the_oracle_alone():
    """Passes without the library: every case is in the regime it was built for."""
    assert mc.shapes_regime() and mc.weight_regime() and mc.range_regime() and mc.spread_regime()


def test_symbols_are_declared_and_exported():
    abi = _abi()
    hdr = (ROOT / "include" / "rplgpu_msg.h").read_text()
    declared = set(re.findall(r"\b(rplgpu_[a-z_0-9]+)\s*\(", hdr))
    lib = abi.load_library()
    for name in SYMBOLS:
        assert name in declared and name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    for name, value in dict(MAX_SHIFT=49, MAX_TABLE=65536, MAX_SPREAD_SHIFT=256, PER_LANE=8, MAX_BLOCKS=1 << 23,
                            NO_WEIGHT=1, OFF_RANGE=2, EMPTY_STEP=4).items():
        m = re.search(rf"#define RPLGPU_MPPI_{name}\s+(0x[0-9A-Fa-f]+|\d+)u", hdr)
        assert m and int(m.group(1), 0) == value == getattr(abi, "MPPI_" + name), name
    assert (mo.MAX_SHIFT, mo.MAX_TABLE, mo.PER_LANE, mo.ADMISSIBLE) == (49, 65536, 8, abi.ROLLOUT_ADMISSIBLE)
    assert C.sizeof(abi.Mppi) == 20


def test_default_and_check():
    abi = _abi()
    d = abi.Mppi.defaults()
    assert {k: getattr(d, k) for k in mo.DEFAULT} == mo.DEFAULT and d.check() == abi.OK
    lib = abi.load_library()
    assert lib.rplgpu_mppi_check(None) == abi.ERR_INVALID_ARG
    lib.rplgpu_default_mppi(None)
    good = mo.spec(steps=9)
    for kw in [dict(xy_scale=0.0), dict(xy_scale=-1.0), dict(xy_scale=math.inf), dict(xy_scale=math.nan),
               dict(shift=50), dict(table_len=0), dict(table_len=65537), dict(steps=0), dict(steps=257),
               dict(delta_per_step=2)]:
        s = dict(good, **kw)
        assert not mo.spec_valid(s) and mo.struct_of(s).check() == abi.ERR_INVALID_ARG, kw
        with pytest.raises(abi.RplGpuError):
            abi.mppi_check(mo.struct_of(s))
    for kw in [dict(xy_scale=1e-30), dict(xy_scale=3e38), dict(shift=0), dict(shift=49), dict(table_len=1),
               dict(table_len=65536), dict(steps=1), dict(steps=256), dict(delta_per_step=0)]:
        s = dict(good, **kw)
        assert mo.spec_valid(s) and mo.struct_of(s).check() == abi.OK, kw
    # the sums' bound: 2^20 candidates of weight 65535 and a magnitude of 2^23
    assert (1 << 20) * 65535 * (1 << 23) < 1 << 59 and (1 << 20) * 65535 ** 2 < 1 << 52


def test_scratch_words():
    abi = _abi()
    for G, K, T_e in [(1, 1, 1), (1, 2048, 56), (3, 257, 65), (1, 40, 256), (65535, 1, 1), (2, 1 << 20, 16),
                      (1, 1 << 20, 1), (64, 1024, 32)]:
        assert abi.mppi_scratch_words(G, K, T_e) == mo.scratch_words(G, K, T_e) > 0, (G, K, T_e)
        assert abi.mppi_scratch_words(G, K, T_e) % 4 == 0
    assert abi.mppi_scratch_words(1, 2048, 56) == 8 * 8 + 12 * 64 * 56
    for G, K, T_e in [(0, 5, 1), (65536, 5, 1), (5, 0, 1), (5, (1 << 20) + 1, 1), (1, 5, 0), (1, 5, 257),
                      (1, (1 << 16) + 1, 256), (65535, 1 << 16, 256), (65535, 1 << 20, 1)]:
        assert abi.mppi_scratch_words(G, K, T_e) == mo.scratch_words(G, K, T_e) == 0, (G, K, T_e)


def test_answer_by_hand():
    """Two candidates with deltas (0, 1, 1, 0) and (0, -1, 2, 0), weights 3 and 1, xy_scale 1024: W = 4, sum w H = 2^21,
    sum w X = 5120; the new delta is (float 0.6, float 0.8, 1.25, 0)."""
    s = mo.spec(steps=1, table_len=2, shift=0)
    out, rres = mc.scored([10, 11], [True, True])
    delta = np.array([[[0, 1, 1, 0]], [[0, -1, 2, 0]]], np.float32)
    table = np.array([3, 1], np.uint16)
    want_sums = [4, 0, 1 << 21, 0, 5120, 0, 0, 0]
    want_new = np.array([0.6, 0.8, 1.25, 0.0], np.float32)
    for got in (mo.update_walk(s, out, rres, delta, table), mo.update_sweep(s, out, rres, delta, table),
                _abi().mppi_update_host(mo.struct_of(s), out, rres, delta, table)):
        w, sums, nout, res = got
        assert w.tolist() == [3, 1] and sums[0].tolist() == want_sums and nout[0].tobytes() == want_new.tobytes()
        assert res.tolist() == [2, 0, 4, 0, 10, 0, 0, 0]


@pytest.mark.parametrize("i", range(len(_all_cases())))
def test_writers_and_host_twin_agree(i):
    c = _all_cases()[i]
    a = mo.update_walk(c["spec"], c["out"], c["rres"], c["delta"], c["table"], c["nominal"])
    assert mo.equal(a, mc.want(c)), c["name"]
    assert mo.equal(_host(c), mc.want(c)), c["name"]


def test_large_cases_host_twin_and_walk():
    for c in (mc.shape_case(3000, 12, 0), mc.shape_case(1100, 5, 1), mc.weight_cases()["big_sums"]):
        assert mo.equal(_host(c), mc.want(c)), c["name"]
    c = mc.weight_cases()["big_sums"]
    assert mo.equal(mo.update_walk(c["spec"], c["out"], c["rres"], c["delta"], c["table"], None), mc.want(c))


def test_host_twin_in_place_nominal():
    abi = _abi()
    c = mc.range_cases()["empty_step_odd_nominal"]
    lib = abi.load_library()
    a = abi._mppi_update_args(mo.struct_of(c["spec"]), c["out"], c["rres"], c["delta"], c["table"], c["nominal"].copy())
    args = list(a[0])
    args[8] = args[4]   # nominal_out = nominal
    assert lib.rplgpu_mppi_update_host(C.byref(mo.struct_of(c["spec"])), *args) == abi.OK
    assert a[2][4].tobytes() == mc.want(c)[2].tobytes()


@pytest.mark.parametrize("name", [s[0] for s in mc.SPREADS])
def test_spread_writers_and_host_twin_agree(name):
    c = mc.spread_case(name)
    want = mc.spread_want(name)
    assert mo.spread_walk(c["nominal"], c["noise"], c["shift"], c["keep_first"]).tobytes() == want.tobytes()
    assert _abi().mppi_spread_host(c["nominal"], c["noise"], c["shift"], c["keep_first"]).tobytes() == want.tobytes()


def test_spread_identity_with_e16_move():
    """Without keep_first, step t of all candidates — the host twin's and the oracle's — equals rplgpu_resample_host
    with P = 1, the nominal step as the pose, weight 1, M = K, n_delta = M."""
    abi = _abi()
    for name in ("shift_0", "shift_1", "shift_beyond"):
        c, want = mc.spread_case(name), mc.spread_want(name)
        got = abi.mppi_spread_host(c["nominal"], c["noise"], c["shift"], 0)
        K, T = c["noise"].shape[:2]
        for t in range(T):
            pose = c["nominal"][min(t + c["shift"], len(c["nominal"]) - 1)]
            moved, _, _ = abi.resample_host(np.ones(1, np.uint32), pose[None, :], K, 0,
                                            np.ascontiguousarray(c["noise"][:, t]))
            assert moved.tobytes() == got[:, t].tobytes() == want[:, t].tobytes(), (name, t)


def test_table_known_answers():
    abi = _abi()
    t = abi.mppi_table(300.0, 4, 64)
    assert t[0] == 65535 and (np.diff(t.astype(np.int64)) <= 0).all() and t.tobytes() == mc.table_of(300.0, 4, 64).tobytes()
    assert abi.mppi_table(1e-300, 0, 3).tolist() == [65535, 0, 0]       # entry 0 whatever the temperature
    far = abi.mppi_table(1.0, 49, 65536)
    assert far[0] == 65535 and not far[1:].any()                          # 0 in the far tail
    assert abi.mppi_table(1.0, 0, 13)[12] == math.floor(65535 * math.exp(-12.0) + 0.5) == 0
    assert abi.mppi_table(1.0, 0, 12)[11] == 1
    assert abi.mppi_table(1e300, 0, 5).tolist() == [65535] * 5
    for bad in [(0.0, 0, 4), (-1.0, 0, 4), (math.nan, 0, 4), (math.inf, 0, 4), (1.0, 50, 4), (1.0, 0, 0),
                (1.0, 0, 65537)]:
        with pytest.raises(abi.RplGpuError):
            abi.mppi_table(*bad)
    assert abi.load_library().rplgpu_mppi_table(1.0, 0, 4, None) == abi.ERR_INVALID_ARG


def test_host_twins_refuse():
    abi = _abi()
    lib = abi.load_library()
    c = mc.group_cases()[0]
    a = abi._mppi_update_args(mo.struct_of(c["spec"]), c["out"], c["rres"], c["delta"], c["table"], c["nominal"])
    before = [x.copy() for x in a[1]]

    def call(spec=None, **kw):
        args = list(a[0])
        for i, v in kw.items():
            args[int(i[1:])] = v
        return lib.rplgpu_mppi_update_host(C.byref(mo.struct_of(spec or c["spec"])), *args)

    assert call() == abi.OK and mo.equal(a[1], mc.want(c))
    for x, b in zip(a[1], before):
        x[...] = b
    for i in (0, 1, 2, 3, 6, 7, 8, 9):
        assert call(**{f"a{i}": 0}) == abi.ERR_INVALID_ARG, i
    assert call(a5=0) == call(a5=(1 << 20) + 1) == abi.ERR_INVALID_ARG
    assert call(spec=dict(c["spec"], steps=256), a5=(1 << 16) + 1) == abi.ERR_INVALID_ARG
    assert call(spec=dict(c["spec"], shift=50)) == call(spec=dict(c["spec"], xy_scale=0.0)) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_mppi_update_host(None, *a[0]) == abi.ERR_INVALID_ARG
    assert all(x.tobytes() == b.tobytes() for x, b in zip(a[1], before))       # nothing written
    s = mc.spread_case("shift_1")
    sa, out, _ = abi._mppi_spread_args(s["nominal"], s["noise"], 1, 0)
    for kw in [{0: 0}, {2: 0}, {7: 0}, {1: 0}, {1: 257}, {3: 0}, {3: (1 << 20) + 1}, {4: 0}, {4: 257}, {5: 257}]:
        args = list(sa)
        for i, v in kw.items():
            args[i] = v
        assert lib.rplgpu_mppi_spread_host(*args) == abi.ERR_INVALID_ARG, kw
    assert not out.any()
