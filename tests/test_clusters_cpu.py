"""E21 without a device: the spec check and the scratch size, the oracle's two writers against each other and the
library's own rplgpu_cluster_poses_host against them byte for byte on every case of tests/clusters_cases.py, set 1 of the
result against rplgpu_estimate_host on BEST's poses, both sets of a two-mode list as poses, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import clusters_cases as cc
from tests import clusters_oracle as co
from tests import estimate_oracle as eo

NONE = co.NONE
GUARD_WORD = 0x5A5A5A5A


def spec_of(c, **kw):
    d = dict(nx=c["nx"], ny=c["ny"], xy_scale=c["xy_scale"], flags=c["wrap"])
    d.update(kw)
    return abi.PoseClusters(d["nx"], d["ny"], d["xy_scale"], d["flags"])


def twin(c, g, cap, clusters_in=None):
    poses = c["groups"][0]["poses"] if c["shared"] else g["poses"]
    return abi.cluster_poses_host(poses, g["map"], g["bins"], c["T"], g["weights"], spec_of(c), cap, clusters_in)


def test_spec_check_and_scratch_size():
    s = abi.PoseClusters.defaults()
    assert (s.nx, s.ny, s.xy_scale, s.flags) == (103, 103, 1024.0, 1) and s.check(72) == abi.OK
    bad = abi.ERR_INVALID_ARG
    for kw, T in ((dict(nx=0), 1), (dict(ny=0), 1), (dict(nx=65537), 1), (dict(ny=65537), 1), (dict(), 0), (dict(), 1025),
                  (dict(nx=65536, ny=1025), 1), (dict(xy_scale=0.0), 1), (dict(xy_scale=-1.0), 1),
                  (dict(xy_scale=float("nan")), 1), (dict(xy_scale=float("inf")), 1), (dict(flags=2), 1)):
        assert abi.PoseClusters.defaults(**kw).check(T) == bad, (kw, T)
    assert abi.PoseClusters.defaults(nx=65536, ny=1024).check(1) == abi.OK                # exactly RPLGPU_MAX_POSE_BINS
    assert abi.PoseClusters.defaults(nx=1, ny=1, flags=0).check(1024) == abi.OK
    assert abi.load_library().rplgpu_pose_clusters_check(None, 1) == bad
    for a in ((0, 1, 4, 4, 4), (65536, 1, 4, 4, 4), (1, 0, 4, 4, 4), (1, abi.MAX_POSES + 1, 4, 4, 4), (1, 1, 0, 4, 4),
              (1, 1, 4, 65537, 4), (1, 1, 4, 4, 0), (1, 1, 4, 4, 1025), (1, 1, 65536, 1025, 1)):
        assert abi.cluster_scratch_words(*a) == 0, a
    one, three = abi.cluster_scratch_words(1, 1000, 103, 103, 72), abi.cluster_scratch_words(3, 1000, 103, 103, 72)
    assert one > 0 and one % 2 == 0 and three == 3 * one
    # what the head of rpl_clusters.hip says: hdr, bbase, rbase, wpre, five parts of KC, tabW, pord, E17's tiles
    even = lambda v: (v + 1) & ~1
    words, kc = (103 * 103 * 72 + 31) // 32, 103 * 103 * 72
    assert one == 16 + even((words + 1023) // 1024) + even((kc + 1023) // 1024) + even(words) + 7 * even(kc) + 1000 + 68
    assert abi.cluster_scratch_words(1, 1, 65536, 1024, 1) < 2 ** 24                       # KC stops at 2^20 bins


@pytest.mark.parametrize("name", cc.NAMES)
def test_regime_and_writers_agree(name):
    cc.check_regime(name)                                          # (want() has run both writers against each other)
    c, w = cc.get(name), cc.want(name)
    if name != "large":
        return
    other = co.writer_b(c["groups"][0], c["nx"], c["ny"], c["T"], c["wrap"], c["xy_scale"])   # beyond 4096 poses, once
    for x, y in zip(w[0], other):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", cc.NAMES)
def test_host_twin_matches_the_oracle(name):
    c, w = cc.get(name), cc.want(name)
    for g, (labels, table, res) in zip(c["groups"], w):
        cap = len(table) + 2
        guard = np.full((cap, 4), GUARD_WORD, np.uint32)
        got = twin(c, g, cap, guard)
        print(name, "result", got[2][:8].tolist(), got[2][72:].tolist(), "want", res[:8].tolist(), res[72:].tolist())
        assert got[0].tobytes() == labels.tobytes()
        assert got[1][:len(table)].tobytes() == table.tobytes() and (got[1][len(table):] == GUARD_WORD).all()
        assert got[2].tobytes() == res.tobytes()


@pytest.mark.parametrize("name", ["edge1025", "blocks", "comb", "strays", "heavy_few", "big_w", "out_of_range", "five",
                                  "groups0", "two_modes", "large"])
def test_set_1_is_e17_on_the_poses_of_best(name):
    """independent of both writers: E17's own host twin, every pose of the sub-list admitted"""
    c, w = cc.get(name), cc.want(name)
    for g, (labels, table, res) in zip(c["groups"], w):
        for k, pick in ((0, labels != NONE), (1, labels == res[1])):
            q, inr, _ = eo.quantise(g["poses"], c["xy_scale"])
            pick = pick & inr
            assert pick.any()
            sub_w = None if g["weights"] is None else g["weights"][pick]
            e17 = abi.estimate_host(g["poses"][pick], sub_w,
                                    abi.PoseEstimate(c["xy_scale"], eo.OPEN_R2, eo.OPEN_DOT), 0)
            assert res[8 + 32 * k:40 + 32 * k].tobytes() == e17[8:40].tobytes(), (name, k)
            assert res[2 + 2 * k:4 + 2 * k].tolist() == e17[2:4].tolist()


def test_both_sets_of_a_two_mode_list_as_poses():
    c, w = cc.get("two_modes"), cc.want("two_modes")
    g = c["groups"][0]
    got = twin(c, g, 8)
    assert got[2].tobytes() == w[0][2].tobytes()
    heavy, light = cc.MODES                                        # 60 % of the poses are drawn around MODES[0]
    best = abi.estimate_pose(got[2][:72], c["xy_scale"], 1)
    whole = abi.estimate_pose(got[2][:72], c["xy_scale"], 0)
    print("set 1", best[:3].tolist(), "set 0", whole[:3].tolist())
    assert abs(best[0] - heavy[0]) < 0.5 and abs(best[1] - heavy[1]) < 0.5           # within one bin of 0.5 m
    assert abs((best[2] - heavy[2] + np.pi) % (2 * np.pi) - np.pi) < 2 * np.pi / c["T"]
    # SECOND's mean by E17 with a gate at one of its poses, as the header advises: here simply the sub-list
    second = g["poses"][w[0][0] == got[2][72]]
    e17 = abi.estimate_host(second, None, abi.PoseEstimate(c["xy_scale"], eo.OPEN_R2, eo.OPEN_DOT), 0)
    other = abi.estimate_pose(e17, c["xy_scale"], 0)
    assert abs(other[0] - light[0]) < 0.5 and abs(other[1] - light[1]) < 0.5
    mix = [0.6 * a + 0.4 * b for a, b in zip(heavy, light)]        # the whole list's mean lies between the modes
    assert abs(whole[0] - mix[0]) < 0.5 and abs(whole[1] - mix[1]) < 0.5 and abs(whole[0] - heavy[0]) > 2.0


def test_table_caps_and_optional_outputs():
    c, (labels, table, res) = cc.get("five"), cc.want("five")[0]
    g = c["groups"][0]
    for cap in (0, 1, 3, 5, 8):
        guard = np.full((cap, 4), GUARD_WORD, np.uint32)
        got = twin(c, g, cap, guard)
        n = min(cap, 5)
        assert got[1][:n].tobytes() == table[:n].tobytes() and (got[1][n:] == GUARD_WORD).all(), cap
        assert got[0].tobytes() == labels.tobytes() and got[2].tobytes() == res.tobytes()
    lib = abi.load_library()
    out = np.full(81, GUARD_WORD, np.uint32)
    s = spec_of(c)
    assert lib.rplgpu_cluster_poses_host(C.byref(s), g["poses"].ctypes.data, len(g["poses"]), g["weights"].ctypes.data,
                                         c["T"], g["map"].ctypes.data, g["bins"].ctypes.data, None, None, 7,
                                         out.ctypes.data) == abi.OK
    assert out[:80].tobytes() == res.tobytes() and out[80] == GUARD_WORD


def test_refusals_write_nothing():
    c = cc.get("five")
    g = c["groups"][0]
    lib = abi.load_library()
    P = len(g["poses"])
    labels = np.full(P + 1, GUARD_WORD, np.uint32)
    table = np.full((5, 4), GUARD_WORD, np.uint32)
    out = np.full(81, GUARD_WORD, np.uint32)
    good = dict(s=spec_of(c), poses=g["poses"].ctypes.data, P=P, w=g["weights"].ctypes.data, T=c["T"],
                m=g["map"].ctypes.data, b=g["bins"].ctypes.data, res=out.ctypes.data)

    def call(fn, h=(), **kw):
        a = dict(good)
        a.update(kw)
        return fn(*h, C.byref(a["s"]) if a["s"] is not None else None, a["poses"], a["P"], a["w"], a["T"], a["m"], a["b"],
                  labels.ctypes.data, table.ctypes.data, 5, a["res"])

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(s=None), dict(s=spec_of(c, nx=0)), dict(s=spec_of(c, flags=2)), dict(s=spec_of(c, xy_scale=0.0)),
               dict(T=0), dict(T=1025), dict(poses=0), dict(P=0), dict(P=abi.MAX_POSES + 1), dict(m=0), dict(b=0),
               dict(res=0)):
        assert call(lib.rplgpu_cluster_poses_host, **kw) == bad, kw
        assert call(lib.rplgpu_cluster_poses, h=(None,), **kw) == bad, kw          # the door without a handle
    assert call(lib.rplgpu_cluster_poses, h=(None,)) == bad
    assert lib.rplgpu_cluster_poses_dev(None, C.byref(good["s"]), 16, 4 * P, 0, 0, 0, 1, P, c["T"], 16, 2, 16, P, 0, 0, 0,
                                        0, 0, 16, 16) == bad
    assert (labels == GUARD_WORD).all() and (table == GUARD_WORD).all() and (out == GUARD_WORD).all()
    assert call(lib.rplgpu_cluster_poses_host) == abi.OK
    assert out[:80].tobytes() == cc.want("five")[0][2].tobytes() and out[80] == labels[P] == GUARD_WORD
