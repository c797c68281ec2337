"""E17 without a device: the new symbols and the scratch formula, rplgpu_estimate_host (the rule in plain C++ with
__int128) against both writers of tests/estimate_oracle.py on every case of tests/estimate_cases.py, the writers
against each other, answers worked out by hand, rplgpu_estimate_pose against fractions.Fraction on the same
integers, and the refusals of the host functions."""
import math
from fractions import Fraction

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import estimate_cases as ec
from tests import estimate_oracle as eo

F32 = np.float32
U32_MAX = 0xFFFFFFFF
WRITERS = (eo.sums_python, eo.sums_limbs)


def _host(case, g=0):
    poses, w, c = ec.group_inputs(case, g)
    return abi.estimate_host(poses, w, ec.spec_of(case["spec"]), c)


def _all_three(case, key=None, groups=None):
    """the host function, the first writer and the second writer: the same 72 words; -> the words"""
    a = ec.want(case, key)
    b = ec.want(case, None, writer=eo.sums_limbs)
    assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape == (case["G"], 72) and a.tobytes() == b.tobytes()
    for g in range(case["G"]) if groups is None else groups:
        got = _host(case, g)
        assert got.dtype == np.uint32 and got.tobytes() == a[g].tobytes(), (g, got, a[g])
    return a


# ---- symbols, the defaults, the scratch formula ------------------------------------------------------------------------------
def test_symbols_defaults_and_scratch_words():
    lib = abi.load_library()
    for name in ("rplgpu_default_pose_estimate", "rplgpu_pose_estimate_check", "rplgpu_estimate_scratch_words",
                 "rplgpu_estimate_poses_dev", "rplgpu_estimate_host", "rplgpu_estimate_poses", "rplgpu_estimate_pose"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    for fn in ("estimate_poses_dev", "estimate_poses"):
        assert callable(getattr(abi.RplGpu, fn))
    s = abi.PoseEstimate.defaults()
    assert (s.xy_scale, s.gate_r2, s.gate_dot) == (1024.0, 512 * 512, 15 << 36) == tuple(eo.DEFAULT.values())
    assert abi.ESTIMATE_WORDS == eo.WORDS == 72
    import ctypes
    assert ctypes.sizeof(abi.PoseEstimate) == 24 and abi.PoseEstimate.gate_r2.offset == 8
    for G, P in [(1, 1), (1, 1024), (1, 1025), (7, 4096), (101, 1100), (65535, 3), (1, 1 << 20), (3, (1 << 20) - 1)]:
        n = abi.estimate_scratch_words(G, P)
        assert n == eo.scratch_words(G, P) and n % 2 == 0 and n >= G * 68 * eo.tiles(P)
    for G, P in [(0, 5), (5, 0), (1, (1 << 20) + 1), (0, 0), (65536, 5)]:
        assert abi.estimate_scratch_words(G, P) == 0 == eo.scratch_words(G, P)
    assert abi.estimate_scratch_words(65535, 1 << 20) == 65535 * 68 * 1024 > 1 << 30  # needs 64 bits of bytes


# ---- every case: host function and both writers ------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ec.EDGE_P)
def test_edge_cases(P):
    case = ec.edge_case(P)
    ec.edge_regime(case, _all_three(case, f"edge{P}"))


@pytest.mark.parametrize("xy_scale", [1024.0, 1000.0])
def test_quantisation_cases(xy_scale):
    case = ec.quant_case(xy_scale)
    ec.quant_regime(case)
    _all_three(case, f"quant{xy_scale}")


@pytest.mark.parametrize("kind", ec.GATE_KINDS)
def test_gate_cases(kind):
    case = ec.gate_case(kind)
    ec.gate_regime(case, kind, _all_three(case, f"gate_{kind}"))


@pytest.mark.parametrize("cancel", [False, True])
def test_extreme_cases(cancel):
    case = ec.extreme_case(2049, cancel)
    ec.extreme_regime(case, _all_three(case, f"extreme{cancel}"), cancel)


def test_largest_list():
    case = ec.big_case()
    res = ec.want(case, "big")                                   # (the limb writer alone at this size)
    ec.extreme_regime(case, res)
    assert _host(case).tobytes() == res[0].tobytes()


def test_weights_null_is_every_weight_one():
    case = ec.edge_case(1025)
    ones = dict(case, w=np.ones_like(case["w"]))
    null = dict(case, w=None)
    a = _all_three(null, "null1025")
    assert a.tobytes() == _all_three(ones).tobytes() and (a[:, 2] == a[:, 3]).all() and (a[:, 4] == a[:, 5]).all()
    assert a.tobytes() != ec.want(case, "edge1025").tobytes()


@pytest.mark.parametrize("ppg", [0, 1])
def test_groups_cases(ppg):
    case = ec.groups_case(ppg)
    ec.groups_regime(case, _all_three(case, f"groups{ppg}", groups=[0, 7, 8, 50, 100]))


def test_writers_on_random_lists():
    rng = np.random.default_rng(1710)
    for _ in range(60):
        P = int(rng.integers(1, 300))
        poses, _ = ec.cloud(rng, P, spread=int(rng.choice([50, 4000, 8000000])))
        w = rng.integers(0, 1 << int(rng.integers(1, 33)), P, dtype=np.uint64).astype(np.uint32)
        spec = dict(xy_scale=float(rng.choice([1024.0, 1000.0, 0.37])), gate_r2=int(rng.integers(0, 1 << 24)),
                    gate_dot=int(rng.integers(-(1 << 40), 1 << 40)))
        c = int(rng.integers(0, P + 3))
        a, b = (eo.estimate(poses, w, spec, c, writer=wr) for wr in WRITERS)
        assert a.tobytes() == b.tobytes()
        assert abi.estimate_host(poses, w, ec.spec_of(spec), c).tobytes() == a.tobytes()


# ---- answers by hand -----------------------------------------------------------------------------------------------------------
def _words(v):
    return eo.words_of(v)


def test_known_answers():
    # two poses, w = (1, 3), heading 0 (C = 2^20, S = 0): X = (1024, -2048), Y = (512, 512); the open gate
    poses = np.array([[1, 0, 1.0, 0.5], [1, 0, -2.0, 0.5]], F32)
    w = np.array([1, 3], np.uint32)
    sums = [4, 1024 - 3 * 2048, 4 * 512, 4 << 20, 0, 1024 ** 2 + 3 * 2048 ** 2, 1024 * 512 - 3 * 2048 * 512,
            4 * 512 ** 2]
    words = [0, 0, 2, 2, 2, 2, 0, 0] + 2 * [x for v in sums for x in _words(v)]
    spec = abi.PoseEstimate.open_gate()
    res = abi.estimate_host(poses, w, spec)
    assert res.tolist() == words
    for wr in WRITERS:
        assert eo.estimate(poses, w, eo.OPEN, writer=wr).tolist() == words
    # ... the default gate (0.5 m) around pose 0 holds pose 0 alone: 3 m apart
    res = abi.estimate_host(poses, w)
    own = [1, 1024, 512, 1 << 20, 0, 1024 ** 2, 1024 * 512, 512 ** 2]
    assert res.tolist() == [0, 0, 2, 2, 1, 1, 0, 0] + [x for v in sums + own for x in _words(v)]
    # a negative sum: the high words are all ones (sum wX = -5120 = 0xFFFFEC00 below 2^32)
    assert res[12:16].tolist() == [0xFFFFEC00, U32_MAX, U32_MAX, U32_MAX] and eo.value_of(res[12:16]) == -5120
    # a sum that cancels to 0: w = (3, 1) at X = (-1024, 3072); the mean is 0 although no pose is there
    poses = np.array([[1, 0, -1.0, 0.0], [1, 0, 3.0, 0.0]], F32)
    res = abi.estimate_host(poses, np.array([3, 1], np.uint32), spec)
    assert res[12:16].tolist() == [0, 0, 0, 0] and eo.value_of(res[28:32]) == 3 * 1024 ** 2 + 3072 ** 2
    # weight 0 everywhere: counted as in range, not as alive; both W flags
    res = abi.estimate_host(poses, np.zeros(2, np.uint32), spec)
    assert res[:8].tolist() == [4 | 8, 0, 2, 0, 2, 0, 0, 0] and not res[8:].any()
    # ties go to even: 0.5, 1.5, 2.5, -0.5, -1.5, -2.5 quanta -> 0, 2, 2, -0, -2, -2
    poses = np.array([[1, 0, t / 1024.0, 0] for t in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5)], F32)
    got = [eo.sums_of_result(abi.estimate_host(poses[k:k + 1], None, spec), 0)[1] for k in range(6)]
    assert got == [0, 2, 2, 0, -2, -2]


# ---- the fp64 helper against exact rationals -----------------------------------------------------------------------------------
def _sin_cos(x, terms=40):
    """sine and cosine of a Fraction by their series (|x| <= 4: the remainder is below 4^80 / 80!, about 1e-71)"""
    s = c = Fraction(0)
    term = Fraction(1)
    for n in range(2 * terms):
        if n % 2 == 0:
            c += term if n % 4 == 0 else -term
        else:
            s += term if n % 4 == 1 else -term
        term = term * x / (n + 1)
    return s, c


def _pose_check(res, xy_scale, k):
    out = abi.estimate_pose(res, xy_scale, k)
    W, sx, sy, sc, ss, sxx, sxy, syy = eo.sums_of_result(res, k)
    scale = Fraction(float(F32(xy_scale)))
    mx, my = Fraction(sx, W) / scale, Fraction(sy, W) / scale
    rel, tiny = Fraction(1, 1 << 49), Fraction(1, 1 << 48)
    worst = {}
    for name, got, true in (("mean x", out[0], mx), ("mean y", out[1], my)):
        err = abs(Fraction(got) - true)
        worst[name] = float(err / abs(true)) if true else float(err)
        assert err <= rel * abs(true), (name, got, float(true))
    for name, got, s2, prod in (("cov xx", out[3], sxx, mx * mx), ("cov xy", out[4], sxy, mx * my),
                                ("cov yy", out[5], syy, my * my)):
        first = Fraction(s2, W) / scale ** 2
        bound = tiny * (abs(first) + abs(prod))
        err = abs(Fraction(got) - (first - prod))
        worst[name] = float(err / bound) if bound else float(err)
        assert err <= bound, (name, got, float(first - prod), float(err), float(bound))
    norm2 = sc * sc + ss * ss
    if norm2:
        # theta against atan2(ss, sc): sin(theta - true) = (sin(theta) sc' - cos(theta) ss') with the unit vector
        # (sc', ss'); |sin(e)| >= |e| (1 - e^2 / 6), and cos(e) > 0 rules the opposite direction out
        s, c = _sin_cos(Fraction(out[2]))
        cross, dot = s * sc - c * ss, c * sc + s * ss
        assert dot > 0 and cross * cross <= (tiny * tiny) * norm2 * Fraction(999, 1000), (out[2], sc, ss)
        worst["theta"] = math.sqrt(float(cross * cross / norm2))
        r_true2 = Fraction(norm2, W * W << 40)                      # R^2, exact
        r2 = Fraction(out[6]) ** 2                                  # |R - true| <= rel * true, on the squares
        assert out[6] > 0 and r_true2 * (1 - rel) ** 2 <= r2 <= r_true2 * (1 + rel) ** 2, (out[6], float(r_true2))
        worst["R"] = abs(float(r2 / r_true2) - 1.0) / 2
    assert out[7] == W
    return worst


def test_estimate_pose_within_its_bounds():
    worst = {}
    cases = [(ec.edge_case(P), 1024.0) for P in (1, 2, 65, 1025, 4096)] + [(ec.quant_case(1000.0), 1000.0),
                                                                         (ec.extreme_case(2049), 1024.0),
                                                                         (ec.extreme_case(2049, True), 1024.0),
                                                                         (ec.groups_case(0, G=9), 1024.0)]
    for case, scale in cases:
        for g in range(case["G"]):
            res = _host(case, g)
            for k in (0, 1):
                if not res[0] & (4 << k):
                    for name, v in _pose_check(res, scale, k).items():
                        worst[name] = max(worst.get(name, 0.0), v)
    print("worst errors (means: relative; covariances: share of the bound; theta: radians):", worst)
    # by hand: w = (1, 3) at x = (1, -2), y = 0.5, heading 0 -> mean (-1.25, 0.5), cov xx = 13/4 - 25/16, R = 1
    res = abi.estimate_host(np.array([[1, 0, 1.0, 0.5], [1, 0, -2.0, 0.5]], F32), np.array([1, 3], np.uint32),
                            abi.PoseEstimate.open_gate())
    assert abi.estimate_pose(res, 1024.0, 0).tolist() == [-1.25, 0.5, 0.0, 13 / 4 - 25 / 16, 0.0, 0.0, 1.0, 4.0]
    # headings +-90 degrees with equal weight cancel: R = 0, theta = atan2(0, 0) = 0
    res = abi.estimate_host(np.array([[0, 1, 0, 0], [0, -1, 0, 0]], F32), None, abi.PoseEstimate.open_gate())
    out = abi.estimate_pose(res, 1024.0, 0)
    assert out[6] == 0.0 and out[2] == 0.0 and out[7] == 2.0


def test_estimate_pose_refusals():
    lib = abi.load_library()
    res = abi.estimate_host(np.array([[1, 0, 1.0, 0.5]], F32), np.array([0], np.uint32))
    out = np.full(8, 7.0)
    bad = abi.ERR_INVALID_ARG
    assert res[0] == 4 | 8
    assert lib.rplgpu_estimate_pose(res.ctypes.data, 1024.0, 0, out.ctypes.data) == bad     # W = 0
    assert lib.rplgpu_estimate_pose(res.ctypes.data, 1024.0, 1, out.ctypes.data) == bad
    res = abi.estimate_host(np.array([[1, 0, 1.0, 0.5]], F32))
    assert lib.rplgpu_estimate_pose(res.ctypes.data, 1024.0, 2, out.ctypes.data) == bad     # no such set
    assert lib.rplgpu_estimate_pose(0, 1024.0, 0, out.ctypes.data) == bad
    assert lib.rplgpu_estimate_pose(res.ctypes.data, 1024.0, 0, 0) == bad
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.rplgpu_estimate_pose(res.ctypes.data, scale, 0, out.ctypes.data) == bad
    assert (out == 7.0).all()
    assert lib.rplgpu_estimate_pose(res.ctypes.data, 1024.0, 0, out.ctypes.data) == abi.OK and out[0] == 1.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_spec_check_and_host_function_refusals():
    lib = abi.load_library()
    bad = abi.ERR_INVALID_ARG
    assert lib.rplgpu_pose_estimate_check(None) == bad
    abi.pose_estimate_check(abi.PoseEstimate.defaults())
    abi.pose_estimate_check(abi.PoseEstimate.open_gate(xy_scale=1e-30))
    for v in (0.0, -0.0, -1024.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(abi.RplGpuError) as e:
            abi.pose_estimate_check(abi.PoseEstimate.defaults(xy_scale=v))
        assert e.value.code == bad
    poses = np.array([[1, 0, 1.0, 0.5], [1, 0, -2.0, 0.5]], F32)
    res = np.full(80, 77, np.uint32)
    good = abi.PoseEstimate.defaults()
    import ctypes as C

    def call(poses_=poses.ctypes.data, P=2, w=0, spec=good, res_=res.ctypes.data):
        return lib.rplgpu_estimate_host(poses_, P, w, C.byref(spec) if spec is not None else None, 0, res_)

    assert call(poses_=0) == bad and call(res_=0) == bad and call(spec=None) == bad
    assert call(P=0) == bad and call(P=abi.MAX_POSES + 1) == bad
    assert call(spec=abi.PoseEstimate.defaults(xy_scale=0.0)) == bad
    assert call(spec=abi.PoseEstimate.defaults(xy_scale=float("nan"))) == bad
    assert (res == 77).all()
    assert call() == abi.OK and res[2] == 2 and (res[72:] == 77).all()
    with pytest.raises(abi.RplGpuError) as e:
        abi.estimate_host(np.zeros((0, 4), F32))
    assert e.value.code == bad
