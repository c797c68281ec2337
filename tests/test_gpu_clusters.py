"""E21 on the device: rplgpu_cluster_poses_dev against tests/clusters_oracle.py byte for byte — the 80 result words, the
labels and the table rows of every group, flag bit 5 clear, the guard words around every output, and the unchanged
poses, weights, maps and bin ids.  The inputs and their regime checks live in tests/clusters_cases.py."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import bins_oracle as bo
from tests import clusters_cases as cc
from tests import clusters_oracle as co
from tests import resample_oracle as ro
from tests import test_gpu_bins as tb

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD_WORD = 0x5A5A5A5A
PAD = 5                                # guard entries behind every group's list
FRONT = 4                              # guard words in front of every output (a multiple of 4: alignment)
NONE = co.NONE


def spec_of(c, **kw):
    d = dict(nx=c["nx"], ny=c["ny"], xy_scale=c["xy_scale"], flags=c["wrap"])
    d.update(kw)
    return abi.PoseClusters(d["nx"], d["ny"], d["xy_scale"], d["flags"])


def _up(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda:0"))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _full(k):
    import torch
    return torch.full((k,), GUARD_WORD, dtype=torch.int32, device=torch.device("cuda:0"))


def _buffers(c, cap, pad=PAD, labels=True, table=True):
    """Device copies of a case's lists, weights, maps and bin ids (each group's followed by guard entries) and the
    guarded outputs: FRONT guard words in front of the labels, the table and the result, guards behind every group's."""
    G, L = len(c["groups"]), 1 if c["shared"] else len(c["groups"])
    P, T = len(c["groups"][0]["poses"]), c["T"]
    words = co.map_words(c["nx"], c["ny"], T)
    mstride = words + (words & 1) + 2
    h_p = np.full((L, P + pad, 4), 123.0, F32)
    for g in range(L):
        h_p[g, :P] = c["groups"][g]["poses"]
    h_w = None
    if any(g["weights"] is not None for g in c["groups"]):
        h_w = np.full((G, P + pad), 1, np.uint32)                  # (no weights for one group of several: all 1)
        for g in range(G):
            if c["groups"][g]["weights"] is not None:
                h_w[g, :P] = c["groups"][g]["weights"]
    h_m = np.full((G, mstride), GUARD_WORD, np.uint32)
    h_b = np.full((G, P + pad), GUARD_WORD, np.uint32)
    for g in range(G):
        h_m[g, :words] = c["groups"][g]["map"]
        h_b[g, :P] = c["groups"][g]["bins"]
    scratch = abi.cluster_scratch_words(G, P, c["nx"], c["ny"], T)
    assert scratch > 0
    return dict(G=G, P=P, T=T, L=L, cap=cap, spec=spec_of(c), h_p=h_p, d_p=_up(h_p.view(np.uint32)),
                pstride=4 * (P + pad), ppg=1 if L > 1 else 0, h_w=h_w, d_w=_up(h_w) if h_w is not None else None,
                wstride=P + pad, h_m=h_m, d_m=_up(h_m), mstride=mstride, h_b=h_b, d_b=_up(h_b), bstride=P + pad,
                d_l=_full(FRONT + G * (P + pad)) if labels else None, lstride=P + pad,
                d_t=_full(FRONT + G * (4 * cap + 4)) if table else None, tstride=4 * cap + 4,
                d_r=_full(FRONT + 80 * G + 8), d_s=_full(scratch + 2), scratch=scratch)


def _call(gpu, b, **kw):
    a = dict(spec=b["spec"], poses=b["d_p"].data_ptr(), pstride=b["pstride"], ppg=b["ppg"],
             w=b["d_w"].data_ptr() if b["d_w"] is not None else 0, wstride=b["wstride"], G=b["G"], P=b["P"], T=b["T"],
             map=b["d_m"].data_ptr(), mstride=b["mstride"], bins=b["d_b"].data_ptr(), bstride=b["bstride"],
             labels=b["d_l"].data_ptr() + 4 * FRONT if b["d_l"] is not None else 0, lstride=b["lstride"],
             table=b["d_t"].data_ptr() + 4 * FRONT if b["d_t"] is not None else 0, tstride=b["tstride"], cap=b["cap"],
             res=b["d_r"].data_ptr() + 4 * FRONT, scratch=b["d_s"].data_ptr())
    a.update(kw)
    gpu.cluster_poses_dev(a["spec"], a["poses"], a["pstride"], a["ppg"], a["w"], a["wstride"], a["G"], a["P"], a["T"],
                          a["map"], a["mstride"], a["bins"], a["bstride"], a["labels"], a["lstride"], a["table"],
                          a["tstride"], a["cap"], a["res"], a["scratch"])


def _inputs_unchanged(b):
    assert _u32(b["d_p"]).tobytes() == b["h_p"].tobytes()
    assert _u32(b["d_m"]).tobytes() == b["h_m"].tobytes() and _u32(b["d_b"]).tobytes() == b["h_b"].tobytes()
    if b["d_w"] is not None:
        assert _u32(b["d_w"]).tobytes() == b["h_w"].tobytes()


def _read(b):
    """-> (labels (G, P) or None, the table's words (G, 4 cap) or None, results (G, 80)), the guards checked"""
    G, P, cap = b["G"], b["P"], b["cap"]
    _inputs_unchanged(b)
    assert (_u32(b["d_s"])[b["scratch"]:] == GUARD_WORD).all()      # nothing behind the scratch the size function gives
    res = _u32(b["d_r"])
    assert (res[:FRONT] == GUARD_WORD).all() and (res[FRONT + 80 * G:] == GUARD_WORD).all()
    labels = table = None
    if b["d_l"] is not None:
        v = _u32(b["d_l"])
        assert (v[:FRONT] == GUARD_WORD).all()
        v = v[FRONT:].reshape(G, b["lstride"])
        assert (v[:, P:] == GUARD_WORD).all()
        labels = v[:, :P]
    if b["d_t"] is not None:
        v = _u32(b["d_t"])
        assert (v[:FRONT] == GUARD_WORD).all()
        v = v[FRONT:].reshape(G, b["tstride"])
        assert (v[:, 4 * cap:] == GUARD_WORD).all()
        table = v[:, :4 * cap]
    return labels, table, res[FRONT:FRONT + 80 * G].reshape(G, 80)


def _run(gpu, c, cap, **kw):
    b = _buffers(c, cap, **kw)
    _call(gpu, b)
    gpu.synchronize()
    return _read(b)


def _check(got, want_, cap):
    labels, table, res = got
    assert len(res) == len(want_)
    for g, (wl, wt, wr) in enumerate(want_):
        print(f"group {g}: result {res[g][:8].tolist()} {res[g][72:].tolist()} want {wr[:8].tolist()} {wr[72:].tolist()}")
        if labels is not None and labels[g].tobytes() != wl.tobytes():
            bad = np.flatnonzero(labels[g] != wl)
            print(f"group {g}: {len(bad)} of {len(wl)} labels differ, first {int(bad[0])}: {int(labels[g][bad[0]])} "
                  f"want {int(wl[bad[0]])}")
        assert not int(res[g][0]) & 32 or int(wr[0]) & 32, "flag bit 5: a loop bound was hit"
        assert labels is None or labels[g].tobytes() == wl.tobytes(), g
        if table is not None:
            n = min(cap, len(wt))
            assert table[g][:4 * n].tobytes() == wt[:n].tobytes(), g
            assert (table[g][4 * n:] == GUARD_WORD).all(), g        # rows beyond min(N_c, cap) are not written
        assert res[g].tobytes() == wr.tobytes(), g


@pytest.mark.parametrize("name", cc.NAMES)
def test_cases(gpu, name):
    cc.check_regime(name)
    want_ = cc.want(name)
    cap = min(max(len(w[1]) for w in want_) + 2, 4096)
    _check(_run(gpu, cc.get(name), cap), want_, cap)


@pytest.mark.parametrize("name", ["blocks", "spiral", "large"])
def test_twice_is_the_same(gpu, name):
    c = cc.get(name)
    a, b = _run(gpu, c, 64), _run(gpu, c, 64)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    _check(a, cc.want(name), 64)


@pytest.mark.parametrize("cap", [0, 1, 3, 5, 8])
def test_table_caps(gpu, cap):
    _check(_run(gpu, cc.get("five"), cap), cc.want("five"), cap)


def test_without_optional_outputs(gpu):
    c, want_ = cc.get("groups0"), cc.want("groups0")
    got = _run(gpu, c, 4, labels=False)
    assert got[0] is None
    _check(got, want_, 4)
    got = _run(gpu, c, 4, table=False)
    assert got[1] is None
    _check(got, want_, 4)
    b = _buffers(c, 4)
    _call(gpu, b, cap=0, tstride=0)                                # a table pointer with cap 0: nothing is written
    gpu.synchronize()
    assert (_u32(b["d_t"]) == GUARD_WORD).all()
    _check((_read(b)[0], None, _read(b)[2]), want_, 0)


@pytest.mark.parametrize("name", cc.NAMES)
def test_host_buffers_every_case(gpu, name):
    """every case through the door rplgpu_cluster_poses, one call per group (the door takes one group; a shared list is
    group 0's): labels, the table with its untouched rows and the 80 words against the oracle and the host twin"""
    c, want_ = cc.get(name), cc.want(name)
    for g, (wl, wt, wr) in zip(c["groups"], want_):
        poses = c["groups"][0]["poses"] if c["shared"] else g["poses"]
        cap = min(len(wt) + 1, 4096)
        n = min(cap, len(wt))
        guard = np.full((cap, 4), GUARD_WORD, np.uint32)
        got = gpu.cluster_poses(poses, g["map"], g["bins"], c["T"], g["weights"], spec_of(c), cap, guard)
        twin = abi.cluster_poses_host(poses, g["map"], g["bins"], c["T"], g["weights"], spec_of(c), cap, guard)
        print(name, "result", got[2][:8].tolist(), got[2][72:].tolist(), "want", wr[:8].tolist(), wr[72:].tolist())
        assert not int(got[2][0]) & 32 or int(wr[0]) & 32, "flag bit 5: a loop bound was hit"
        for k, w in enumerate((wl, np.concatenate([wt[:n], guard[n:]]), wr)):
            assert got[k].tobytes() == twin[k].tobytes() == w.tobytes(), (name, k)
    g = c["groups"][0]                                              # and without the optional outputs
    lib, out = abi.load_library(), np.full(81, GUARD_WORD, np.uint32)
    s, w = spec_of(c), g["weights"]
    assert lib.rplgpu_cluster_poses(gpu._h, C.byref(s), g["poses"].ctypes.data, len(g["poses"]),
                                    w.ctypes.data if w is not None else None, c["T"], g["map"].ctypes.data,
                                    g["bins"].ctypes.data, None, None, 3, out.ctypes.data) == abi.OK
    assert out[:80].tobytes() == want_[0][2].tobytes() and out[80] == GUARD_WORD


def test_host_buffers_refusals(gpu):
    c = cc.get("five")
    g = c["groups"][0]
    lib = abi.load_library()
    P = len(g["poses"])
    labels, table, out = (np.full(n, GUARD_WORD, np.uint32) for n in (P + 1, 20, 81))
    good = dict(h=gpu._h, s=spec_of(c), poses=g["poses"].ctypes.data, P=P, T=c["T"], m=g["map"].ctypes.data,
                b=g["bins"].ctypes.data, res=out.ctypes.data)

    def door(**kw):
        a = dict(good)
        a.update(kw)
        return lib.rplgpu_cluster_poses(a["h"], C.byref(a["s"]) if a["s"] is not None else None, a["poses"], a["P"],
                                        g["weights"].ctypes.data, a["T"], a["m"], a["b"], labels.ctypes.data,
                                        table.ctypes.data, 5, a["res"])

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(h=None), dict(s=None), dict(s=spec_of(c, ny=0)), dict(s=spec_of(c, flags=3)), dict(poses=0),
               dict(P=0), dict(P=abi.MAX_POSES + 1), dict(T=0), dict(T=1025), dict(m=0), dict(b=0), dict(res=0)):
        assert door(**kw) == bad, kw
    assert (labels == GUARD_WORD).all() and (table == GUARD_WORD).all() and (out == GUARD_WORD).all()
    wl, wt, wr = cc.want("five")[0]
    assert door() == abi.OK and labels[:P].tobytes() == wl.tobytes() and table.tobytes() == wt.tobytes()
    assert out[:80].tobytes() == wr.tobytes() and out[80] == labels[P] == GUARD_WORD


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu):
    import torch
    c = cc.get("groups0")
    b = _buffers(c, 4)
    P = b["P"]
    words = co.map_words(c["nx"], c["ny"], c["T"])
    host = np.zeros(64, np.uint32)
    hp = host.ctypes.data + (-host.ctypes.data % 16)
    refused = []

    def call(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            _call(gpu, b, **kw)
        refused.append(kw)
        return e.value.code

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(nx=0), dict(ny=65537), dict(xy_scale=float("nan")), dict(xy_scale=0.0), dict(flags=2)):
        assert call(spec=spec_of(c, **kw)) == bad, kw
    assert call(T=0) == bad and call(T=1025) == bad
    assert call(spec=spec_of(c, nx=65536, ny=1025), T=1) == bad     # above RPLGPU_MAX_POSE_BINS
    assert call(G=0) == bad and call(G=65536) == bad
    assert call(P=0) == bad and call(P=abi.MAX_POSES + 1, pstride=1 << 23, wstride=1 << 21, bstride=1 << 21,
                                     lstride=1 << 21) == bad
    for k in ("poses", "map", "bins", "res", "scratch"):            # required pointers
        assert call(**{k: 0}) == bad, k
    names = dict(poses="d_p", w="d_w", map="d_m", bins="d_b", labels="d_l", table="d_t", res="d_r", scratch="d_s")
    for k, step in (("poses", 4), ("poses", 8), ("w", 2), ("map", 4), ("bins", 1), ("labels", 2), ("table", 1),
                    ("res", 2), ("scratch", 4)):                    # alignment
        assert call(**{k: b[names[k]].data_ptr() + step}) == bad, (k, step)
    assert call(pstride=4 * P - 4) == bad and call(pstride=4 * P + 2) == bad and call(pstride=0) == bad
    assert call(wstride=P - 1) == bad and call(bstride=P - 1) == bad and call(lstride=P - 1) == bad
    assert call(tstride=4 * b["cap"] - 1) == bad
    assert call(mstride=words + (words & 1) - 2) == bad and call(mstride=b["mstride"] + 1) == bad and call(mstride=0) == bad
    # an output that shares bytes with an input or with another output
    assert call(labels=b["d_b"].data_ptr()) == bad and call(res=b["d_m"].data_ptr()) == bad
    assert call(table=b["d_r"].data_ptr() + 4 * FRONT) == bad and call(scratch=b["d_p"].data_ptr()) == bad
    assert call(labels=b["d_s"].data_ptr() + 64) == bad
    for k in ("poses", "w", "map", "bins", "labels", "table", "res", "scratch"):       # plain host memory
        assert call(**{k: hp}) == bad, k
    lib = abi.load_library()
    assert lib.rplgpu_cluster_poses_dev(None, C.byref(b["spec"]), b["d_p"].data_ptr(), b["pstride"], 1, 0, 0, b["G"], P,
                                        b["T"], b["d_m"].data_ptr(), b["mstride"], b["d_b"].data_ptr(), b["bstride"], 0,
                                        0, 0, 0, 0, b["d_r"].data_ptr(), b["d_s"].data_ptr()) == bad
    assert lib.rplgpu_cluster_poses_dev(gpu._h, None, b["d_p"].data_ptr(), b["pstride"], 1, 0, 0, b["G"], P,
                                        b["T"], b["d_m"].data_ptr(), b["mstride"], b["d_b"].data_ptr(), b["bstride"], 0,
                                        0, 0, 0, 0, b["d_r"].data_ptr(), b["d_s"].data_ptr()) == bad
    assert len(refused) >= 40
    gpu.synchronize()
    torch.cuda.synchronize()
    for k in ("d_l", "d_t", "d_r", "d_s"):                          # nothing was queued
        assert (_u32(b[k]) == GUARD_WORD).all(), k
    _inputs_unchanged(b)
    _call(gpu, b)                                                   # then a good call on the same buffers
    gpu.synchronize()
    _check(_read(b), cc.want("groups0"), 4)


# ---- chains: one stream, nothing read in between --------------------------------------------------------------------------
def _chain_cluster(gpu, s, T, d_poses, pstride, d_w, wstride, P, d_m, mstride, d_b, bstride, cap):
    d_l, d_t, d_r = _full(P + PAD), _full(4 * cap + 4), _full(80 + 8)
    scratch = abi.cluster_scratch_words(1, P, s.nx, s.ny, T)
    d_s = _full(scratch + 2)
    gpu.cluster_poses_dev(abi.PoseClusters(s.nx, s.ny, 1024.0, 1), d_poses, pstride, 0, d_w, wstride, 1, P, T, d_m,
                          mstride, d_b, bstride, d_l.data_ptr(), P + PAD, d_t.data_ptr(), 4 * cap + 4, cap,
                          d_r.data_ptr(), d_s.data_ptr())
    return d_l, d_t, d_r, d_s


def _chain_check(out, P, cap, want_):
    d_l, d_t, d_r, _ = out
    wl, wt, wr = want_
    n = min(cap, len(wt))
    assert (_u32(d_l)[P:] == GUARD_WORD).all() and (_u32(d_t)[4 * n:] == GUARD_WORD).all()
    assert (_u32(d_r)[80:] == GUARD_WORD).all()
    assert _u32(d_l)[:P].tobytes() == wl.tobytes() and _u32(d_t)[:4 * n].tobytes() == wt[:n].tobytes()
    print("result", _u32(d_r)[:8].tolist(), "want", wr[:8].tolist())
    assert _u32(d_r)[:80].tobytes() == wr.tobytes()


def test_chain_bins_then_clusters(gpu):
    """(1) E20 -> E21 on one stream: the map and the bin ids never leave the device"""
    c = cc.get("two_modes")
    g = c["groups"][0]
    s, T, P = bo.spec(0.0, 0.0, 2.0, c["nx"], c["ny"]), c["T"], len(g["poses"])
    rng = np.random.default_rng(71)
    w = (rng.integers(0, 3, P) * rng.integers(1, 1000, P)).astype(np.uint32)        # a third of the poses skipped
    bmap, bins, r20 = bo.bin_poses(s, g["poses"], w, bo.table(T))
    want_ = co.cluster(dict(poses=g["poses"], weights=w, map=bmap, bins=bins), s.nx, s.ny, T, 1)
    assert int(want_[2][77]) == int(r20[3]) > P // 4 and int(want_[2][6]) >= 2 and int(want_[2][76]) == 0    # the regime
    words = bo.map_words(s, T)
    d_p, d_w, d_e = _up(g["poses"].view(np.uint32)), _up(w), _up(bo.table(T).view(np.uint32))
    d_m, d_b, d_r20 = _full(words + (words & 1) + 2), _full(P + PAD), _full(16)
    gpu.bin_poses_dev(tb.spec_of(s), d_p.data_ptr(), 4 * P, 0, d_w.data_ptr(), P, 1, P, d_e.data_ptr(), T,
                      d_m.data_ptr(), words + (words & 1), d_b.data_ptr(), P + PAD, d_r20.data_ptr())
    out = _chain_cluster(gpu, s, T, d_p.data_ptr(), 4 * P, d_w.data_ptr(), P, P, d_m.data_ptr(), words + (words & 1),
                         d_b.data_ptr(), P + PAD, 8)
    gpu.synchronize()  # nothing was read until here
    assert _u32(d_m)[:words].tobytes() == bmap.tobytes() and _u32(d_b)[:P].tobytes() == bins.tobytes()
    assert _u32(d_r20)[:8].tobytes() == r20.tobytes()
    _chain_check(out, P, 8, want_)


def test_chain_score_bins_clusters_resample(gpu, oracle):
    """(2) score (E15) -> bin (E20) -> cluster (E21) -> resample (E16) on one stream: the cluster result is the oracle's
    on E15's weights, and what E16 produces is what it produces without the calls in between"""
    import torch
    a = tb.score_chain(oracle)
    P, T, bs = tb.sc.CHAIN_P, a["T"], a["bs"]
    bmap, bins, r20 = a["want"]
    want_ = co.cluster(dict(poses=a["poses"], weights=a["w"], map=bmap, bins=bins), bs.nx, bs.ny, T, 1)
    u = 0x2345678
    moved, anc, r16 = ro.resample(a["w"], a["poses"], P, u)
    assert int(want_[2][77]) == int(r20[3]) > 0 and int(want_[2][6]) >= 1 and not int(want_[2][0]) & 4      # the regime
    d = tb._score_setup(a["case"])
    h_p = np.full((P + PAD, 4), 123.0, F32)
    h_p[:P] = a["poses"]
    d_p, d_e, d_u = _up(h_p.view(np.uint32)), _up(bo.table(T).view(np.uint32)), _up(np.array([u], np.uint32))
    d_w, d_b, d_r15, d_r20, d_r16 = _full(P + PAD), _full(P + PAD), _full(16), _full(16), _full(16)
    d_out, d_anc = _full(4 * (P + PAD)), _full(P + PAD)
    words = bo.map_words(bs, T)
    d_m = _full(words + (words & 1) + 2)
    d_scr = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=torch.device("cuda:0"))
    tb._score(gpu, d, d_p.data_ptr(), P, 4 * (P + PAD), d_w, d_r15)
    gpu.bin_poses_dev(tb.spec_of(bs), d_p.data_ptr(), 4 * (P + PAD), 0, d_w.data_ptr(), P + PAD, 1, P, d_e.data_ptr(), T,
                      d_m.data_ptr(), words + (words & 1), d_b.data_ptr(), P + PAD, d_r20.data_ptr())
    out = _chain_cluster(gpu, bs, T, d_p.data_ptr(), 4 * (P + PAD), d_w.data_ptr(), P + PAD, P, d_m.data_ptr(),
                         words + (words & 1), d_b.data_ptr(), P + PAD, 8)
    gpu.resample_poses_dev(d_w.data_ptr(), P + PAD, d_p.data_ptr(), 4 * (P + PAD), 0, 1, P, P, d_u.data_ptr(), 0, 0, 0, 0,
                           d_out.data_ptr(), 4 * (P + PAD), d_anc.data_ptr(), P + PAD, d_r16.data_ptr(),
                           d_scr.data_ptr())
    gpu.synchronize()  # nothing was read until here
    assert _u32(d_p).tobytes() == h_p.tobytes()
    assert _u32(d_w)[:P].tobytes() == a["w"].tobytes() and _u32(d_r15)[:8].tobytes() == a["r15"].tobytes()
    assert _u32(d_m)[:words].tobytes() == bmap.tobytes() and _u32(d_b)[:P].tobytes() == bins.tobytes()
    _chain_check(out, P, 8, want_)
    assert _u32(d_out)[:4 * P].tobytes() == np.ascontiguousarray(moved).view(np.uint32).tobytes()
    assert _u32(d_anc)[:P].tobytes() == anc.astype(np.uint32).tobytes() and _u32(d_r16)[:8].tobytes() == r16.tobytes()
    for t, k in ((d_w, P), (d_b, P), (d_out, 4 * P), (d_anc, P), (d_r15, 8), (d_r20, 8), (d_r16, 8), (d_m, words)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
