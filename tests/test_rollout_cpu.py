"""E27 without a device: the symbols, the check and the defaults of rplgpu_rollout_t, an answer known by hand, the two
writers of tests/rollout_oracle.py against each other and against the host twin rplgpu_rollout_host (ctypes) on every
case of tests/rollout_cases.py, the identity with E16's move through rplgpu_resample_host, rplgpu_rollout_deltas'
known answers and the host twin's refusals."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import rollout_cases as rc
from tests import rollout_oracle as ro

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["rplgpu_default_rollout", "rplgpu_rollout_check", "rplgpu_rollout_scratch_words", "rplgpu_rollout_deltas",
           "rplgpu_rollout_host", "rplgpu_rollout_dev", "rplgpu_rollout"]


def _host(c):
    return abi.rollout_host(ro.struct_of(c["spec"]), c["start"], c["delta"], c["footprint"], c["grid"], c["potential"])


def test_symbols_are_declared_and_exported():
    hdr = (ROOT / "include" / "rplgpu_msg.h").read_text()
    declared = set(re.findall(r"\b(rplgpu_[a-z_0-9]+)\s*\(", hdr))
    lib = abi.load_library()
    for name in SYMBOLS:
        assert name in declared and name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.rplgpu_abi_version() == 1
    for name, value in dict(MAX_STEPS=256, MAX_FOOTPRINT=64, MAX_WEIGHT=65535, NONE=0xFFFFFFFF, TILE=32,
                            MAX_TILES=1 << 23, BLOCKED=1, CELL_RANGE=2, END_UNREACHED=4, ADMISSIBLE=8).items():
        m = re.search(rf"#define RPLGPU_ROLLOUT_{name}\s+(0x[0-9A-Fa-f]+|\d+)u", hdr)
        assert m and int(m.group(1), 0) == value == getattr(abi, "ROLLOUT_" + name), name
    assert (ro.TILE, ro.MAX_STEPS, ro.MAX_FOOTPRINT, ro.MAX_WEIGHT) == (32, 256, 64, 65535)
    assert C.sizeof(abi.Rollout) == 52


def test_default_and_check():
    d = abi.Rollout.defaults()
    got = {k: getattr(d, k) for k in ro.DEFAULT}
    want = dict(ro.DEFAULT, origin_x=float(np.float32(-25.6)), origin_y=float(np.float32(-25.6)),
                resolution=float(np.float32(0.05)))
    assert got == want and d.check() == abi.OK
    lib = abi.load_library()
    assert lib.rplgpu_rollout_check(None) == abi.ERR_INVALID_ARG
    lib.rplgpu_default_rollout(None)
    good = rc.base_spec(steps=9, min_steps=4)
    refused = [dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(lethal=0), dict(lethal=101),
               dict(unknown_value=101), dict(steps=0), dict(steps=257), dict(min_steps=0), dict(min_steps=10),
               dict(a_end=65536), dict(a_min=65536), dict(a_sum=65536), dict(a_max=1 << 31), dict(resolution=0.0),
               dict(resolution=-0.1), dict(resolution=math.inf), dict(resolution=math.nan), dict(origin_x=math.inf),
               dict(origin_y=math.nan)]
    for kw in refused:
        s = dict(good, **kw)
        assert not ro.spec_valid(s) and ro.struct_of(s).check() == abi.ERR_INVALID_ARG, kw
        with pytest.raises(abi.RplGpuError):
            abi.rollout_check(ro.struct_of(s))
    edges = [dict(width=1, height=1), dict(width=4096, height=4096), dict(lethal=1), dict(lethal=100),
             dict(unknown_value=0), dict(unknown_value=100), dict(steps=1, min_steps=1), dict(steps=256, min_steps=256),
             dict(min_steps=1), dict(min_steps=9), dict(a_end=0, a_min=0, a_sum=0, a_max=0),
             dict(a_end=65535, a_min=65535, a_sum=65535, a_max=65535)]
    for kw in edges:
        s = dict(good, **kw)
        assert ro.spec_valid(s) and ro.struct_of(s).check() == abi.OK, kw
    # the score's bound: four scales at their limit, D at the field's cap, 256 poses of cost 99
    assert 65535 * (2 * 0xFFFF0000 + 256 * 99 + 99) < 1 << 50


def test_scratch_words():
    for G, K in [(1, 1), (1, 31), (1, 32), (1, 33), (3, 101), (65535, 1), (8, 1 << 20), (256, 1 << 20)]:
        assert abi.rollout_scratch_words(G, K) == ro.scratch_words(G, K) == 8 * -(-K // 32) * G, (G, K)
    for G, K in [(0, 5), (65536, 5), (5, 0), (5, (1 << 20) + 1), (257, 1 << 20), (65535, 4097)]:
        assert abi.rollout_scratch_words(G, K) == ro.scratch_words(G, K) == 0, (G, K)


def test_three_unit_steps_into_a_wall_by_hand():
    """A 6 x 1 grid of 1 m cells with the costs 0 10 20 30 | 100, the start in cell 0, one cell a step, five steps:
    poses 1 - 3 count, pose 4 is in the wall."""
    s = ro.spec(origin_x=0.0, origin_y=0.0, resolution=1.0, width=6, height=1, steps=5, min_steps=3, a_end=2, a_min=0,
                a_sum=3, a_max=7)
    grid = np.array([[0, 10, 20, 30, 100, 0]], np.int8)
    pot = np.array([[500, 400, 300, 200, 100, 0]], np.uint32)
    start, delta, fp = [1, 0, 0.5, 0.5], [[1, 0, 1, 0]], [[0, 0]]
    want_out = [3, ro.BLOCKED | ro.ADMISSIBLE, 60, 30, 200, 200, 2 * 200 + 3 * 60 + 7 * 30, 0]
    for writer in (ro.walk, ro.sweep, lambda *a: abi.rollout_host(ro.struct_of(a[0]), *a[1:])):
        out, ends, res = writer(s, start, delta, fp, grid, pot)
        assert out[0].tolist() == want_out
        assert ends[0].tolist() == [1.0, 0.0, 3.5, 0.5]
        assert res.tolist() == [1, 0, want_out[6], 0, 1, 1, 0, 0]
    out, _, res = abi.rollout_host(ro.struct_of(dict(s, min_steps=4)), start, delta, fp, grid, pot)
    assert out[0].tolist() == [3, ro.BLOCKED, 60, 30, 200, 200, 0xFFFFFFFF, 0xFFFFFFFF]
    assert res.tolist() == [0, ro.NONE, 0xFFFFFFFF, 0xFFFFFFFF, 0, 1, 0, 1]


def test_regimes():
    """By the oracle alone: passes without the library."""
    for regime in (rc.shapes_regime, rc.blocking_regime, rc.field_regime, rc.tie_regime, rc.none_regime,
                   rc.identity_regime):
        regime()


def test_writers_and_host_twin_agree_on_every_case():
    cases = rc.all_small_cases() + [rc.identity_case()]
    assert len({c["name"] for c in cases}) == len(cases) > 30
    for c in cases:
        a = ro.walk(c["spec"], c["start"], c["delta"], c["footprint"], c["grid"], c["potential"])
        b = rc.want(c)
        h = _host(c)
        for name, x, y, z in zip(("out", "end_poses", "result"), a, b, h):
            assert x.tobytes() == y.tobytes(), (c["name"], name, "walk != sweep")
            assert z.tobytes() == y.tobytes(), (c["name"], name, "host twin != sweep")
    big = rc.tie_cases()["waves"]   # (the scalar walk would take a minute)
    assert ro.equal(_host(big), rc.want(big))


def test_identity_with_e16_move():
    """d_end_poses of (T, one delta a candidate) = T chained moves of rplgpu_resample_host with P = 1, weight 1,
    M = K, n_delta = M."""
    c = rc.identity_case()
    K, T = len(c["delta"]), c["spec"]["steps"]
    poses, _, _ = abi.resample_host(np.ones(1, np.uint32), c["start"].reshape(1, 4), K, 0, c["delta"])
    for _ in range(T - 1):
        # (K weights of 1 with u = 0: output j descends from pose j)
        poses, anc, _ = abi.resample_host(np.ones(K, np.uint32), poses, K, 0, c["delta"])
        assert anc.tolist() == list(range(K))
    out, ends, _ = _host(c)
    assert (out[:, 0] == T).all() and ends.tobytes() == poses.tobytes() == rc.want(c)[1].tobytes()


def test_rollout_deltas_known_answers():
    d = abi.rollout_deltas([[0.5, -0.25, 0.0], [1.0, 0.0, math.pi / 2], [0.0, 2.0, math.pi / 2], [3.0, 1.0, 1e-12],
                            [1.0, 0.5, -0.7]], 1.0)
    assert d[0].tobytes() == np.array([1.0, 0.0, 0.5, -0.25], np.float32).tobytes()   # w = 0: exactly
    # a quarter turn at radius v / w = 2 / pi: the base ends at (r, r), heading 90 degrees
    r = 2.0 / math.pi
    assert d[1].tolist() == [np.float32(math.cos(math.pi / 2)), 1.0, np.float32(r), np.float32(r)]
    assert d[2].tolist() == [np.float32(math.cos(math.pi / 2)), 1.0, np.float32(-2 * r), np.float32(2 * r)]
    assert d[3].tolist() == [1.0, np.float32(1e-12), 3.0, 1.0]                         # |th| < 1e-9: the straight line
    th = -0.7
    want = [math.cos(th), math.sin(th), (math.sin(th) - 0.5 * (1 - math.cos(th))) / th,
            ((1 - math.cos(th)) + 0.5 * math.sin(th)) / th]
    assert np.allclose(d[4], want, rtol=0, atol=1e-7)
    half = abi.rollout_deltas([[2.0, 0.0, math.pi]], 0.5)
    assert half.tobytes() == d[1:2].tobytes()
    lib = abi.load_library()
    buf = np.zeros(4, np.float32)
    v = np.zeros(3, np.float64)
    assert lib.rplgpu_rollout_deltas(None, 1, 1.0, buf.ctypes.data) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_rollout_deltas(v.ctypes.data, 1, 1.0, None) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_rollout_deltas(v.ctypes.data, 0, 1.0, buf.ctypes.data) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_rollout_deltas(v.ctypes.data, (1 << 20) + 1, 1.0, buf.ctypes.data) == abi.ERR_INVALID_ARG


def test_host_twin_refusals_write_nothing():
    lib = abi.load_library()
    c = rc.blocking_cases()["at_step_T"]
    spec = ro.struct_of(c["spec"])
    out = np.full(8, 0x5A5A5A5A, np.uint32)
    ends = np.full(4, 7.0, np.float32)
    res = np.full(8, 0x5A5A5A5A, np.uint32)
    a = dict(spec=C.byref(spec), start=c["start"].ctypes.data, delta=c["delta"].ctypes.data, per_step=0,
             fp=c["footprint"].ctypes.data, F=1, grid=c["grid"].ctypes.data, pot=0, K=1, out=out.ctypes.data,
             ends=ends.ctypes.data, res=res.ctypes.data)
    bad_spec = ro.struct_of(dict(c["spec"], lethal=0))
    long_spec = ro.struct_of(dict(c["spec"], steps=256, min_steps=256))
    for kw in [dict(spec=None), dict(spec=C.byref(bad_spec)), dict(start=0), dict(delta=0), dict(fp=0), dict(grid=0),
               dict(out=0), dict(res=0), dict(K=0), dict(K=(1 << 20) + 1), dict(F=0), dict(F=65), dict(per_step=2),
               dict(spec=C.byref(long_spec), K=(1 << 16) + 1)]:
        b = dict(a, **kw)
        rc_ = lib.rplgpu_rollout_host(b["spec"], b["start"], b["delta"], b["per_step"], b["fp"], b["F"], b["grid"],
                                      b["pot"], b["K"], b["out"], b["ends"], b["res"])
        assert rc_ == abi.ERR_INVALID_ARG, kw
    assert (out == 0x5A5A5A5A).all() and (res == 0x5A5A5A5A).all() and (ends == 7.0).all()
    assert lib.rplgpu_rollout_host(a["spec"], a["start"], a["delta"], 0, a["fp"], 1, a["grid"], 0, 1, a["out"], 0,
                                   a["res"]) == abi.OK          # the end poses are optional
    assert out.tolist() == rc.want(c)[0][0].tolist() and (ends == 7.0).all()
