"""E18 without a device: the new symbols, the struct's layout and the defaults; Philox4x32-10's known answers and
their Z; rplgpu_sample_motion_host (the rule in plain C++) against both writers of tests/motion_oracle.py on every case
of tests/motion_cases.py and on random lists, the writers against each other; the moments of Z; rplgpu_motion_odometry
against the same expressions through Python's math; and the refusals of the host functions."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import motion_cases as mc
from tests import motion_oracle as mo

F32 = np.float32
KNOWN = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8", 120177),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd", -61960),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1", 63541),
)


def _host(case, g):
    L = len(case["odom"])
    delta, res = abi.sample_motion_host(case["odom"][g if L > 1 else 0], case["M"], mc.spec_of(case["spec"]), g)
    assert delta.dtype == F32 and delta.shape == (case["M"], 4) and res.dtype == np.uint32
    return delta.view(np.uint32), res


def _all_three(case, key=None, groups=None):
    """the host function, the first writer (up to PYTHON_LIMIT outputs) and the second writer: the same words; -> the
    oracle's triple"""
    a = mc.want(case, key)
    b = mc.want(case, None, writer=mo.deltas_numpy)
    for k in range(3):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    for g in range(case["G"]) if groups is None else groups:
        words, res = _host(case, g)
        assert words.tobytes() == a[0][g].tobytes(), g
        assert res.tobytes() == a[1][g].tobytes(), (g, res, a[1][g])
    return a


# ---- symbols, the struct, the defaults ----------------------------------------------------------------------------------
def test_symbols_struct_and_defaults():
    s = abi.MotionNoise.defaults()
    lib = abi.load_library()
    for name in ("rplgpu_default_motion_noise", "rplgpu_sample_motion_dev", "rplgpu_sample_motion_host",
                 "rplgpu_sample_motion", "rplgpu_philox4x32", "rplgpu_motion_odometry"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    for fn in ("sample_motion_dev", "sample_motion"):
        assert callable(getattr(abi.RplGpu, fn))
    assert (s.seed, s.step, s.first) == (0, 0, 0) == tuple(mo.DEFAULT.values())
    assert C.sizeof(abi.MotionNoise) == 24
    assert (abi.MotionNoise.seed.offset, abi.MotionNoise.step.offset, abi.MotionNoise.first.offset) == (0, 8, 16)
    s = abi.MotionNoise.defaults(seed=(1 << 64) - 1, step=1 << 63, first=(1 << 32) - 1)
    assert (s.seed, s.step, s.first) == ((1 << 64) - 1, 1 << 63, (1 << 32) - 1)
    assert lib.rplgpu_abi_version() == 1


# ---- the generator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,text,z", KNOWN)
def test_philox_known_answers(ctr, key, text, z):
    want = [int(t, 16) for t in text.split()]
    got = abi.philox4x32(ctr, key)
    assert got.dtype == np.uint32 and got.tolist() == want
    assert list(mo.philox_python(ctr, key)) == want
    assert [int(v[0]) for v in mo.philox_numpy(*([c] for c in ctr), *key)] == want
    assert mo.z_of_words(got) == z
    # ... and Z through the host function: with r = (1, 0), trans 0 and kt = 1 output 0's dx is Z of draw 1, whose
    # counter is (first, (g << 2) | 1, step low word, step high word) under the key (seed low word, seed high word)
    spec = abi.MotionNoise.defaults(seed=key[0] | key[1] << 32, step=ctr[2] | ctr[3] << 32, first=ctr[0])
    delta, res = abi.sample_motion_host(np.array([1, 0, 0, 1, 0, 0, 1, 0], F32), 1, spec, 5)
    w = mo.philox_python((ctr[0], 5 << 2 | 1, ctr[2], ctr[3]), key)
    assert delta[0, 2] == mo.z_of_words(w) and delta[0].tolist()[:2] == [1.0, 0.0]


def test_philox_against_the_writers_on_random_blocks():
    rng = np.random.default_rng(18)
    ctr = rng.integers(0, 1 << 32, (200, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (200, 2), dtype=np.uint64)
    for c, k in zip(ctr, key):
        want = list(mo.philox_python(c, k))
        assert abi.philox4x32(c.astype(np.uint32), k.astype(np.uint32)).tolist() == want
        assert [int(v[0]) for v in mo.philox_numpy(*([int(x)] for x in c), int(k[0]), int(k[1]))] == want
    # the output may be written over the counter
    buf = np.zeros(4, np.uint32)
    zero = np.zeros(2, np.uint32)
    assert abi.load_library().rplgpu_philox4x32(buf.ctypes.data, zero.ctypes.data, buf.ctypes.data) == abi.OK
    assert buf.tolist() == [int(t, 16) for t in KNOWN[0][2].split()]
    # Z is symmetric, bounded and exact as a float32; its variance is that of eight uniform 16-bit integers
    assert mo.z_of_words([0, 0, 0, 0]) == -262140 and mo.z_of_words([0xFFFFFFFF] * 4) == 262140
    assert mo.z_of_words([0xFFFF0000] * 4) == 0
    assert float(F32(262140)) == 262140.0 and float(F32(-262139)) == -262139.0
    assert 8 * ((1 << 32) - 1) == 12 * mo.Z_VAR


# ---- every case: host function and both writers -------------------------------------------------------------------------
@pytest.mark.parametrize("M", mc.EDGE_M)
def test_edge_cases(M):
    case = mc.edge_case(M)
    mc.edge_regime(case, _all_three(case, f"edge{M}"))


def test_largest_list():
    case = mc.big_case()
    a = mc.want(case, "big")                                   # (the numpy writer alone at this size)
    mc.big_regime(case, a)
    words, res = _host(case, 0)
    assert words.tobytes() == a[0][0].tobytes() and res.tobytes() == a[1][0].tobytes()


def test_wrap_of_the_first_counter_word():
    case = mc.wrap_case()
    mc.wrap_regime(case, _all_three(case, "wrap"))


def test_a_piece_of_a_list():
    whole, piece = mc.piece_cases()
    a, b = mc.want(whole, "whole"), _all_three(piece, "piece")
    assert b[0][0].tobytes() == a[0][0, 1000:2000].tobytes() and (b[2][0] == a[2][0, 1000:2000]).all()
    assert b[0][0].tobytes() != a[0][0, :1000].tobytes()
    words, _ = _host(whole, 0)
    assert words.tobytes() == a[0][0].tobytes()


@pytest.mark.parametrize("kind", mc.COUNTER_KINDS)
def test_counter_cases(kind):
    case = mc.counter_case(kind)
    mc.counter_regime(kind, _all_three(case, f"counter_{kind}"))


@pytest.mark.parametrize("ppg", [0, 1])
def test_groups_cases(ppg):
    case = mc.groups_case(ppg)
    mc.groups_regime(case, _all_three(case, f"groups{ppg}", groups=[0, 1, 7, 50, 100]))


@pytest.mark.parametrize("which", [0, 2])
def test_z_through_the_floats(which):
    case = mc.z_case(which)
    a = _all_three(case, f"z{which}")
    mc.z_regime(case, which, a)
    _, res = _host(case, 0)
    zs = a[2][0]
    assert int(res[1]) == int(np.abs(zs).max()) and mo.sum_z(res) == int(zs.sum())
    assert mo.sum_z2(res) == int((zs * zs).sum())


def test_float_cases():
    for name, case, regime in (("zero", mc.zero_scale_case(), mc.zero_scale_regime),
                               ("denormal", mc.denormal_case(), mc.denormal_regime),
                               ("huge", mc.huge_case(), mc.huge_regime),
                               ("special", mc.special_case(), mc.special_regime),
                               ("ordinary", mc.ordinary_case(), mc.ordinary_regime)):
        regime(case, _all_three(case, name))


def test_writers_on_random_lists():
    rng = np.random.default_rng(1810)
    for _ in range(60):
        case = mc.random_case(rng)
        _all_three(case)


# ---- moments ------------------------------------------------------------------------------------------------------------
def _moments(seed, g, step):
    M = 65536
    spec = abi.MotionNoise.defaults(seed=seed, step=step)
    _, res = abi.sample_motion_host(mc.ordinary_odom(), M, spec, g)
    zs = mo.z_numpy(dict(seed=seed, step=step, first=0), g, M)
    assert mo.sum_z(res) == int(zs.sum()) and mo.sum_z2(res) == int((zs * zs).sum())
    assert int(res[1]) == int(np.abs(zs).max())
    n = 3 * M
    s, s2 = mo.sum_z(res), mo.sum_z2(res)
    print(f"sum Z {s}, sum Z^2 {s2}, max |Z| {int(res[1])}: {s / n / (mc.SIGMA_Z / math.sqrt(n)):.2f} and "
          f"{(s2 / n - mo.Z_VAR) / math.sqrt(mo.Z2_VAR / n):.2f} standard errors")
    assert abs(s / n) <= 4 * mc.SIGMA_Z / math.sqrt(n)
    assert abs(s2 / n - mo.Z_VAR) <= 4 * math.sqrt(1.51673e19 / n)  # (the figure is mo.Z2_VAR)
    return s, s2, int(res[1])


def test_moments():
    assert _moments(2 << 32 | 1, 0, 0) == (-25886380, 559287488632600, 220864)   # key (1, 2)
    _moments(0x9ABCDEF0 << 32 | 0x12345678, 3, 7)


# ---- the odometry helper ------------------------------------------------------------------------------------------------
def test_motion_odometry():
    alpha = [0.2, 0.1, 0.3, 0.05]
    cases = [(0.3, 0.1, 0.2), (0.0, 0.0, 0.0), (0.005, 0.002, 0.4), (0.00999, 0.0, -0.1), (0.01, 0.0, 0.1),
             (-0.5, 0.0, 0.0), (-0.5, 0.02, 0.05), (0.2, 0.0, math.pi - 0.01), (0.2, 0.1, -math.pi + 0.01),
             (0.1, -0.3, 3.5), (0.1, 0.3, -3.5), (1e3, -2e3, 100.0), (0.0, 0.25, math.pi / 2)]
    for dx, dy, dth in cases:
        got = abi.motion_odometry(dx, dy, dth, alpha)
        want = mo.odometry(dx, dy, dth, alpha)
        assert got.dtype == F32 and got.tobytes() == want.tobytes(), (dx, dy, dth, got, want)
    # below 0.01 m the heading of the motion is not used: rot1 is exactly (1, 0) and rot2 the whole turn
    got = abi.motion_odometry(0.005, 0.002, 0.4, alpha)
    assert got[0] == 1.0 and got[1] == 0.0 and got[3] == F32(math.cos(0.4)) and got[4] == F32(math.sin(0.4))
    # backward: rot1 is about pi, the translation is positive and the rotation noise is that of a small turn
    back, fwd = abi.motion_odometry(-0.5, 0.02, 0.05, alpha), abi.motion_odometry(0.5, 0.02, 0.05, alpha)
    assert back[0] < -0.99 and back[2] > 0 and abs(back[5] / fwd[5] - 1) < 0.05 and abs(back[6] / fwd[6] - 1) < 0.05
    # across +-pi: d = dtheta - rot1 is folded by atan2(sin, cos)
    got = abi.motion_odometry(0.1, 0.3, -3.5, alpha)
    assert abs(math.atan2(got[4], got[3]) - (-3.5 - math.atan2(0.3, 0.1) + 2 * math.pi)) < 1e-6
    # no noise asked for, none given; at rest nothing moves
    assert abi.motion_odometry(0.3, 0.1, 0.2, [0, 0, 0, 0])[5:].tolist() == [0, 0, 0]
    assert abi.motion_odometry(0.0, 0.0, 0.0, alpha).tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    # the scales are sigma over sigma_Z: 10000 draws of the translation have the asked deviation within 5 %
    od = abi.motion_odometry(1.0, 0.0, 0.0, [0, 0, 0.04, 0])
    delta, _ = abi.sample_motion_host(od, 10000, abi.MotionNoise.defaults(seed=1))
    assert abs(delta[:, 2].astype(np.float64).std() / 0.2 - 1) < 0.05 and abs(delta[:, 2].mean() - 1) < 0.01
    od = abi.motion_odometry(1.0, 0.0, 0.0, [0, 0.01, 0, 0])              # 0.1 rad on rot1 and on rot2
    delta, _ = abi.sample_motion_host(od, 10000, abi.MotionNoise.defaults(seed=2))
    head = np.arctan2(delta[:, 1].astype(np.float64), delta[:, 0])
    assert abs(head.std() / math.sqrt(0.02) - 1) < 0.05


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_host_function_refusals():
    lib = abi.load_library()
    bad = abi.ERR_INVALID_ARG
    od = mc.ordinary_odom()
    delta = np.full(24, 7.0, F32)
    res = np.full(12, 77, np.uint32)
    good = abi.MotionNoise.defaults()

    def call(od_=od.ctypes.data, g=0, M=2, spec=good, delta_=delta.ctypes.data, res_=res.ctypes.data):
        return lib.rplgpu_sample_motion_host(od_, g, M, C.byref(spec) if spec is not None else None, delta_, res_)

    assert call(od_=0) == bad and call(spec=None) == bad and call(delta_=0) == bad and call(res_=0) == bad
    assert call(M=0) == bad and call(M=abi.MAX_POSES + 1) == bad and call(g=65535) == bad
    assert (delta == 7.0).all() and (res == 77).all()
    assert call(g=65534) == abi.OK and (delta[8:] == 7.0).all() and (res[8:] == 77).all() and res[6] == 0
    with pytest.raises(abi.RplGpuError) as e:
        abi.sample_motion_host(od, 0)
    assert e.value.code == bad
    lib.rplgpu_default_motion_noise(None)                                   # (ignored)
    out = np.full(4, 9, np.uint32)
    ctr, key = np.zeros(4, np.uint32), np.zeros(2, np.uint32)
    assert lib.rplgpu_philox4x32(0, key.ctypes.data, out.ctypes.data) == bad
    assert lib.rplgpu_philox4x32(ctr.ctypes.data, 0, out.ctypes.data) == bad
    assert lib.rplgpu_philox4x32(ctr.ctypes.data, key.ctypes.data, 0) == bad
    assert (out == 9).all()
    alpha = np.zeros(4)
    o8 = np.full(8, 5.0, F32)
    assert lib.rplgpu_motion_odometry(1.0, 0.0, 0.0, 0, o8.ctypes.data) == bad
    assert lib.rplgpu_motion_odometry(1.0, 0.0, 0.0, alpha.ctypes.data, 0) == bad
    assert (o8 == 5.0).all()
    assert lib.rplgpu_motion_odometry(1.0, 0.0, 0.0, alpha.ctypes.data, o8.ctypes.data) == abi.OK and o8[2] == 1.0
