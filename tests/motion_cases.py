"""The inputs of the E18 tests (tests/test_motion_cpu.py without a device, tests/test_gpu_motion.py on it) and, for
every case, a regime check made from tests/motion_oracle.py alone: that the case is in the situation it is named for.

A case: dict(odom (L, 8) float32 — L = G lists, or 1 shared by every group —, G, M, spec dict(seed, step, first))."""
import math

import numpy as np

from rplidar_ros2_driver_amd import abi
from tests import motion_oracle as mo

F32 = np.float32
EDGE_M = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4096)
BIG_M = 1 << 20
SIGMA_Z = math.sqrt(mo.Z_VAR)
_CACHE = {}


def spec_of(spec):
    return abi.MotionNoise.defaults(**spec)


def ordinary_odom(rot1=0.3, trans=0.25, rot2=-0.2, s_rot=0.05, s_trans=0.02):
    """an increment with noise of s_rot radians and s_trans metres (one sigma), made without the library"""
    return np.array([math.cos(rot1), math.sin(rot1), trans, math.cos(rot2), math.sin(rot2),
                     s_rot / (2 * SIGMA_Z), s_trans / SIGMA_Z, 0.7 * s_rot / (2 * SIGMA_Z)], F32)


def want(case, key=None, writer=None):
    """-> (words (G, M, 4) uint32, results (G, 8) uint32, Z (G, M, 3) int64); computed once per key"""
    if key is not None and writer is None and key in _CACHE:
        return _CACHE[key]
    G, M = case["G"], case["M"]
    L = len(case["odom"])
    parts = [mo.sample(case["odom"][g if L > 1 else 0], M, case["spec"], g, writer=writer) for g in range(G)]
    out = tuple(np.stack([p[k] for p in parts]) for k in range(3))
    if key is not None and writer is None:
        _CACHE[key] = out
    return out


def floats_of(words):
    return np.ascontiguousarray(words).view(F32)


# ---- tile edges -------------------------------------------------------------------------------------------------------
def edge_case(M):
    """two groups with a list each, a seed with bits in both words and a step"""
    odom = np.stack([ordinary_odom(), ordinary_odom(-2.9, 0.4, 3.0, 0.02, 0.05)])
    return dict(odom=odom, G=2, M=M, spec=dict(seed=0x0123456789ABCDEF, step=5, first=0))


def edge_regime(case, want_):
    words, res, zs = want_
    M = case["M"]
    assert words.shape == (2, M, 4) and (res[:, 0] == 0).all() and (res[:, 7] == 0).all()
    assert words[0].tobytes() != words[1].tobytes()
    assert words[0, -1].tobytes() != words[0, 0].tobytes() or M == 1
    assert (zs[0] != zs[1]).any()
    for g in range(2):
        assert int(res[g, 1]) == int(np.abs(zs[g]).max()) > 0
        assert mo.sum_z(res[g]) == int(zs[g].sum()) and mo.sum_z2(res[g]) == int((zs[g] * zs[g]).sum())


def big_case():
    return dict(odom=ordinary_odom()[None], G=1, M=BIG_M, spec=dict(seed=0xFEDCBA9876543210, step=1 << 40, first=7))


def big_regime(case, want_):
    words, res, zs = want_
    n = 3 * BIG_M
    assert res[0, 0] == 0 and mo.sum_z2(res[0]) >= 1 << 32 and res[0, 5] > 0
    assert abs(mo.sum_z(res[0]) / n) <= 4 * SIGMA_Z / math.sqrt(n)
    assert abs(mo.sum_z2(res[0]) / n - mo.Z_VAR) <= 4 * math.sqrt(mo.Z2_VAR / n)
    assert words[0, -1].tobytes() != words[0, 0].tobytes()


# ---- counters ---------------------------------------------------------------------------------------------------------
def wrap_case():
    """first = 2^32 - 3: outputs 3 .. are counters 0 .. of the next 2^32"""
    return dict(odom=ordinary_odom()[None], G=1, M=70, spec=dict(seed=11, step=0, first=(1 << 32) - 3))


def wrap_regime(case, want_):
    zs = want_[2]
    again = mo.z_numpy(dict(case["spec"], first=0), 0, 67)
    assert (zs[0, 3:] == again).all() and (zs[0, :3] != again[:3]).any()
    assert mo.z_python(case["spec"], 0, 3, 1) == mo.z_python(dict(case["spec"], first=0), 0, 0, 1)


def piece_cases():
    """first = 1000 with M = 1000 is outputs 1000 .. 1999 of a call with M = 5000"""
    spec = dict(seed=0xDEADBEEF00000001, step=3, first=0)
    whole = dict(odom=ordinary_odom()[None], G=1, M=5000, spec=spec)
    piece = dict(whole, M=1000, spec=dict(spec, first=1000))
    return whole, piece


def counter_case(kind):
    base = dict(odom=ordinary_odom()[None], G=3, M=130, spec=dict(seed=0x1111111122222222, step=9, first=4))
    if kind == "step_hi":
        base["spec"] = dict(base["spec"], step=(0xABCDEF01 << 32) | 9)
    elif kind == "seed_high_bits":
        base["spec"] = dict(base["spec"], seed=0xFFFFFFFF80000000)
    elif kind == "seed_low_word_only":
        base["spec"] = dict(base["spec"], seed=0x80000001)
    return base


COUNTER_KINDS = ("plain", "step_hi", "seed_high_bits", "seed_low_word_only")


def counter_regime(kind, want_):
    """every word of the counter and of the key matters: each kind's draws differ from the plain case's, the three
    draws of an output differ and so do the groups"""
    zs = want_[2]
    assert (zs[0] != zs[1]).any() and (zs[1] != zs[2]).any()
    assert (zs[:, :, 0] != zs[:, :, 1]).any() and (zs[:, :, 1] != zs[:, :, 2]).any()
    if kind != "plain":
        assert (zs != want(counter_case("plain"), "counter_plain")[2]).any()


def groups_case(ppg, G=101, M=70):
    rng = np.random.default_rng(18)
    L = G if ppg else 1
    odom = np.stack([ordinary_odom(rng.uniform(-3, 3), rng.uniform(0, 1), rng.uniform(-3, 3)) for _ in range(L)])
    return dict(odom=odom, G=G, M=M, spec=dict(seed=0x5555AAAA3333CCCC, step=2, first=0))


def groups_regime(case, want_):
    words = want_[0]
    lists = {words[g].tobytes() for g in range(case["G"])}
    assert len(lists) == case["G"]                           # no two groups' lists are equal


# ---- Z through the floats ---------------------------------------------------------------------------------------------
def z_case(which):
    """r1 = r2 = (1, 0), trans 0, kt = 1, one rotation scale 2^-40 and the other 0: dx = Z_1 and ds * 2^39 = Z_0 (or
    Z_2) exactly — t = Z 2^-40 is exact, q = t^2 < 2^-44 vanishes against 1, so nc = 1 and ns = 2 t"""
    k = F32(2.0 ** -40)
    odom = np.array([1, 0, 0, 1, 0, k if which == 0 else 0, 1, k if which == 2 else 0], F32)
    return dict(odom=odom[None], G=1, M=1500, spec=dict(seed=0x13579BDF02468ACE, step=77, first=0))


def z_regime(case, which, want_):
    words, res, zs = want_
    f = floats_of(words)[0]
    assert (f[:, 2].astype(np.int64) == zs[0, :, 1]).all() and (f[:, 2] == zs[0, :, 1].astype(F32)).all()
    assert (f[:, 1].astype(np.float64) * 2.0 ** 39 == zs[0, :, which]).all()
    assert (f[:, 0] == 1.0).all() and res[0, 0] == 0
    assert len(np.unique(zs[0])) > 1000


# ---- floats -----------------------------------------------------------------------------------------------------------
def zero_scale_case():
    """all scales 0, no entry of r1, r2 or trans equal to 0"""
    o = ordinary_odom()
    o[5:] = 0
    return dict(odom=o[None], G=1, M=1100, spec=dict(seed=3, step=3, first=3))


def zero_scale_regime(case, want_):
    words = want_[0]
    assert (case["odom"][0, :5] != 0).all() and (words[0] == words[0, 0]).all() and want_[1][0, 0] == 0
    assert len(np.unique(want_[2][0])) > 1000                # (the draws themselves vary)


def denormal_case():
    """scales that make every t = Z k denormal: 2^-149, 2^-147 and 2^-145 against |Z| < 2^18.  With r1 = r2 = (1, 0)
    and trans 0 the denormals reach the output: ds = 2 t_0 + 2 t_2 and dx = Z_1 kt; a device that flushed them would
    store zeros"""
    odom = np.zeros((3, 8), F32)
    odom[:, 0] = odom[:, 3] = 1
    for g, e in enumerate((-149, -147, -145)):
        odom[g, 5:] = F32(2.0 ** e)
    return dict(odom=odom, G=3, M=300, spec=dict(seed=99, step=1, first=0))


def denormal_regime(case, want_):
    words, res, zs = want_
    f = floats_of(words)
    tiny = np.finfo(F32).tiny
    for g in range(3):
        t = zs[g].astype(np.float64) * float(case["odom"][g, 5])
        assert (np.abs(t) < tiny).all() and (t != 0).sum() > 880
        sub = (np.abs(f[g]) < tiny) & (f[g] != 0)
        assert sub[:, 1].sum() > 280 and sub[:, 2].sum() > 280 and (f[g][:, 0] == 1).all()
        assert (f[g][:, 2].astype(np.float64) == t[:, 1]).all()      # dx is t_1 itself
    assert (res[:, 0] == 0).all() and words[0].tobytes() != words[2].tobytes()


def huge_case():
    """scales of 3e38: t overflows, Inf / Inf and Inf - Inf make NaN"""
    odom = np.stack([ordinary_odom() for _ in range(3)])
    odom[0, 5] = 3e38
    odom[1, 6] = 3e38
    odom[2, 5:] = 3e38
    return dict(odom=odom, G=3, M=200, spec=dict(seed=5, step=0, first=0))


def huge_regime(case, want_):
    words, res, _ = want_
    f = floats_of(words)
    assert (res[[0, 2], 0] > 0).all() and (res[[0, 2], 7] == 1).all()
    assert (words[np.isnan(f)] == mo.QNAN).all() and np.isnan(f).any()
    assert np.isinf(f[1]).any() and res[1, 0] == 0 == res[1, 7]  # an infinite translation is kept and is no NaN
    for g in range(3):
        assert res[g, 0] == np.isnan(f[g]).any(axis=1).sum()


SPECIAL = (float("nan"), float("inf"), float("-inf"), -0.0)


def special_case():
    """odometry entries NaN, +-Inf and -0, one entry at a time: group 8 e + v has entry e replaced by value v"""
    rows = []
    for e in range(8):
        for v in SPECIAL:
            o = ordinary_odom()
            o[e] = v
            rows.append(o)
    return dict(odom=np.stack(rows), G=32, M=66, spec=dict(seed=8, step=8, first=8))


def special_regime(case, want_):
    words, res, _ = want_
    f = floats_of(words)
    assert (words[np.isnan(f)] == mo.QNAN).all()
    assert (res[0::4, 0] == 66).all()                         # a NaN entry reaches every output
    assert (res[3::4, 0] == 0).all()                          # -0 makes none
    assert (res[:, 7] == (res[:, 0] != 0)).all()
    signs = words[3::4] >> 31
    assert signs.any() and np.isinf(f).any()


def ordinary_case():
    return dict(odom=ordinary_odom()[None], G=1, M=5000, spec=dict(seed=0x2026, step=20, first=0))


def ordinary_regime(case, want_):
    words, res, _ = want_
    f = floats_of(words)[0].astype(np.float64)
    assert len({w.tobytes() for w in words[0]}) > 0.99 * case["M"]
    worst = np.abs(f[:, 0] ** 2 + f[:, 1] ** 2 - 1).max()
    assert worst < 1e-6, worst
    assert res[0, 0] == 0
    # the noise has the size it was asked for: 0.25 m ahead with 0.02 m, headings within a few sigma
    assert abs(np.hypot(f[:, 2], f[:, 3]).mean() - 0.25) < 0.002 and 0.015 < np.hypot(f[:, 2], f[:, 3]).std() < 0.025
    return worst


def random_case(rng):
    o = ordinary_odom(rng.uniform(-3, 3), rng.uniform(-1, 1), rng.uniform(-3, 3))
    for e in (5, 6, 7):
        o[e] = rng.choice([0.0, 2.0 ** -40, 3e38, o[e], -o[e], 1e-3])
    return dict(odom=o[None], G=1, M=int(rng.integers(1, 200)),
                spec=dict(seed=int(rng.integers(0, 1 << 63)) * 2 + 1, step=int(rng.integers(0, 1 << 63)),
                          first=int(rng.integers(0, 1 << 32))))
