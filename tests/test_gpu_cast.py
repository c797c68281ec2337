"""E22 on the device: rplgpu_cast_ranges_dev against tests/cast_oracle.py byte for byte — the range words, the weights,
E15's result words and the eight cast counts of every group, the guard words behind every group's outputs and behind the
result blocks, and the unchanged grids, byte table, beam table, measured scans and poses; every case once through the
device call and once through the host-buffer door.  The inputs and their regime checks live in tests/cast_cases.py."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi, synth
from tests import cast_cases as cc
from tests import cast_oracle as co
from tests import estimate_oracle as eo
from tests import filter_oracle as fo
from tests import pose_oracle as po
from tests import resample_oracle as ro
from tests import seed_cases as sc

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD_WORD = 0x5A5A5A5A
PAD = 5                                # guard entries behind every group's list


def spec_of(s):
    return abi.RangeCast(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["max_steps"],
                         s["hit_lo"], s["unknown_stops"], s["table_half"])


def _up(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda:0"))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _full(k):
    import torch
    return torch.full((k,), GUARD_WORD, dtype=torch.int32, device=torch.device("cuda:0"))


def _buffers(case, pad=PAD, ranges=None, weights=None):
    """Device copies of a case's lists (each followed by guard poses), grids (guard bytes behind each), beam table,
    byte table and measured scans (guard entries behind them), and the guarded outputs."""
    s, G = case["spec"], case["G"]
    L, Lg, P, A = len(case["lists"]), len(case["grids"]), len(case["lists"][0]), len(case["beams"])
    ranges = case["ranges"] if ranges is None else ranges
    weights = (case["measured"] is not None) if weights is None else weights
    cells = s["width"] * s["height"]
    gstride = ((cells + 3) & ~3) + 4 * pad
    h_p = np.full((L, P + pad, 4), 123.0, F32)
    h_g = np.full((Lg, gstride), 100, np.int8)
    for g in range(L):
        h_p[g, :P] = case["lists"][g]
    for g in range(Lg):
        h_g[g, :cells] = case["grids"][g].reshape(-1)
    h_b = np.full((A + 2, 2), 123.0, F32)
    h_b[:A] = case["beams"]
    b = dict(G=G, P=P, A=A, spec=spec_of(s), h_p=h_p, d_p=_up(h_p.view(np.uint32)), pstride=4 * (P + pad),
             ppg=1 if L > 1 else 0, h_g=h_g, d_g=_up(h_g), gstride=gstride, gpg=1 if Lg > 1 else 0, h_b=h_b,
             d_b=_up(h_b.view(np.uint32)), d_c=_full(8 * G + 8), rstride=P * A + pad, wstride=P + pad,
             d_r=_full(G * (P * A + pad)) if ranges else None, h_z=None, d_z=None, h_t=None, d_t=None, d_w=None,
             d_res=None, mstride=0, first=case["first"], step=case["step"])
    if weights:
        b["h_z"] = np.ascontiguousarray(case["measured"], F32)
        b["mstride"] = b["h_z"].shape[1]
        b["h_t"] = np.concatenate([case["table"], np.full(6, 200, np.uint8)])
        b["d_z"], b["d_t"] = _up(b["h_z"].view(np.uint32)), _up(b["h_t"])
        b["d_w"], b["d_res"] = _full(G * (P + pad)), _full(8 * G + 8)
    return b


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _call(gpu, b, **kw):
    a = dict(spec=b["spec"], poses=_ptr(b["d_p"]), pstride=b["pstride"], ppg=b["ppg"], G=b["G"], P=b["P"],
             beams=_ptr(b["d_b"]), A=b["A"], grid=_ptr(b["d_g"]), gstride=b["gstride"], gpg=b["gpg"], z=_ptr(b["d_z"]),
             mstride=b["mstride"], first=b["first"], step=b["step"], table=_ptr(b["d_t"]), ranges=_ptr(b["d_r"]),
             rstride=b["rstride"], w=_ptr(b["d_w"]), wstride=b["wstride"], res=_ptr(b["d_res"]), cast=_ptr(b["d_c"]))
    a.update(kw)
    gpu.cast_ranges_dev(a["spec"], a["poses"], a["pstride"], a["ppg"], a["G"], a["P"], a["beams"], a["A"], a["grid"],
                        a["gstride"], a["gpg"], a["z"], a["mstride"], a["first"], a["step"], a["table"], a["ranges"],
                        a["rstride"], a["w"], a["wstride"], a["res"], a["cast"])


def _inputs_unchanged(b):
    assert _u32(b["d_p"]).tobytes() == b["h_p"].tobytes()
    assert _u32(b["d_b"]).tobytes() == b["h_b"].tobytes()
    assert b["d_g"].cpu().numpy().tobytes() == b["h_g"].tobytes()
    if b["d_z"] is not None:
        assert _u32(b["d_z"]).tobytes() == b["h_z"].tobytes()
        assert b["d_t"].cpu().numpy().tobytes() == b["h_t"].tobytes()


def _read(b):
    """-> (ranges (G, P * A) or None, weights (G, P) or None, result (G, 8) or None, cast (G, 8)), guards checked"""
    G, P, A = b["G"], b["P"], b["A"]
    _inputs_unchanged(b)
    cast = _u32(b["d_c"])
    assert (cast[8 * G:] == GUARD_WORD).all()
    r = w = res = None
    if b["d_r"] is not None:
        r = _u32(b["d_r"]).reshape(G, b["rstride"])
        assert (r[:, P * A:] == GUARD_WORD).all()
        r = r[:, :P * A]
    if b["d_w"] is not None:
        w = _u32(b["d_w"]).reshape(G, b["wstride"])
        assert (w[:, P:] == GUARD_WORD).all()
        w = w[:, :P]
        res = _u32(b["d_res"])
        assert (res[8 * G:] == GUARD_WORD).all()
        res = res[:8 * G].reshape(G, 8)
    return r, w, res, cast[:8 * G].reshape(G, 8)


def _run(gpu, case, **kw):
    b = _buffers(case, **kw)
    _call(gpu, b)
    gpu.synchronize()
    return _read(b)


def _check(got, want_):
    r, w, res, cast = got
    assert len(cast) == len(want_)
    for g, o in enumerate(want_):
        print(f"group {g}: cast {cast[g].tolist()} want {o['cast'].tolist()}")
        if r is not None and r[g].tobytes() != o["ranges"].tobytes():
            bad = np.flatnonzero(r[g] != o["ranges"].reshape(-1))
            print(f"group {g}: {len(bad)} of {r[g].size} range words differ, first {int(bad[0])}: "
                  f"{int(r[g][bad[0]]):08x} want {int(o['ranges'].reshape(-1)[bad[0]]):08x}")
        if w is not None:
            print(f"group {g}: result {res[g].tolist()} want {o['result'].tolist()}")
        assert r is None or r[g].tobytes() == o["ranges"].tobytes(), g
        assert cast[g].tobytes() == o["cast"].tobytes(), g
        if w is not None:
            assert w[g].tobytes() == o["weights"].tobytes(), g
            assert res[g].tobytes() == o["result"].tobytes(), g


# ---- every case, both ways ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_cases(gpu, name):
    case = cc.case(name)
    want_ = cc.want(case, name)
    cc.regime(case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_cases_through_the_door(gpu, name):
    case = cc.case(name)
    want_ = cc.want(case, name)
    for g in range(case["G"]):
        z = None if case["measured"] is None else case["measured"][g]
        r, w, res, cast = gpu.cast_ranges(case["lists"][g % len(case["lists"])], case["beams"],
                                          case["grids"][g % len(case["grids"])], spec_of(case["spec"]), z, case["table"],
                                          case["first"], case["step"], want_ranges=case["ranges"])
        o = want_[g]
        assert cast.tobytes() == o["cast"].tobytes(), g
        assert (r is None and not case["ranges"]) or r.tobytes() == o["ranges"].tobytes(), g
        if z is not None:
            assert w.tobytes() == o["weights"].tobytes() and res.tobytes() == o["result"].tobytes(), g
        else:
            assert w is None and res is None


@pytest.mark.parametrize("mode", ["ranges", "weights", "both"])
@pytest.mark.parametrize("name", ["p64", "groups_own"])
def test_ranges_only_weights_only_both(gpu, name, mode):
    case = cc.case(name)
    want_ = cc.want(case, name)
    r, w, res, cast = got = _run(gpu, case, ranges=mode != "weights", weights=mode != "ranges")
    assert (r is None) == (mode == "weights") and (w is None) == (mode == "ranges")
    _check(got, want_)


def test_larger_strides_and_offset_pointers(gpu):
    """strides larger than needed, and result / cast / weight / range pointers that are only 4-byte aligned"""
    case = cc.case("groups_shared")
    want_ = cc.want(case, "groups_shared")
    _check(_run(gpu, case, pad=PAD + 58), want_)
    b = _buffers(case)
    _call(gpu, b, res=b["d_res"].data_ptr() + 4, cast=b["d_c"].data_ptr() + 4, w=b["d_w"].data_ptr() + 4,
          ranges=b["d_r"].data_ptr() + 4, wstride=b["wstride"], rstride=b["rstride"])
    gpu.synchronize()
    G, P, A = b["G"], b["P"], b["A"]
    for t, block, words in ((b["d_res"], "result", 8 * G), (b["d_c"], "cast", 8 * G)):
        v = _u32(t)
        assert v[0] == GUARD_WORD and (v[1 + words:] == GUARD_WORD).all()
        assert v[1:1 + words].tobytes() == b"".join(o[block].tobytes() for o in want_)
    w, r = _u32(b["d_w"]), _u32(b["d_r"])
    for g, o in enumerate(want_):
        assert w[1 + g * b["wstride"]:][:P].tobytes() == o["weights"].tobytes()
        assert r[1 + g * b["rstride"]:][:P * A].tobytes() == o["ranges"].tobytes()
    assert w[0] == GUARD_WORD == r[0]


# ---- the identities, on the device ---------------------------------------------------------------------------------------
def test_identity_1_a_pose_heading_is_a_beam_direction(gpu):
    case = cc.case("p64")
    poses = case["lists"][0]
    plain = poses.copy()
    plain[:, 0], plain[:, 1] = 1.0, 0.0
    a = dict(case, lists=[poses], beams=np.array([[1, 0]], F32), measured=None, table=None)
    b = dict(case, lists=[plain], beams=np.ascontiguousarray(poses[:, :2]), measured=None, table=None)
    ra, rb = _run(gpu, a)[0][0], _run(gpu, b)[0][0].reshape(len(poses), len(poses))
    assert ra.tobytes() == np.diagonal(rb).tobytes() and len({int(v) >> 28 for v in ra}) >= 3


def test_identities_2_and_4_weights_and_result_from_the_returned_words(gpu):
    for name in ("p65", "a360", "odd"):
        case = cc.case(name)
        r, w, res, _ = _run(gpu, case)
        for g in range(case["G"]):
            z = co.beam_ranges(case["measured"][g], case["first"], case["step"], len(case["beams"]))
            words = r[g].reshape(len(w[g]), -1)
            assert co.weights_rays(case["spec"], words, z, case["table"]).tobytes() == w[g].tobytes(), name
            assert po.result_of(w[g], int((~np.isnan(z)).sum())).tobytes() == res[g].tobytes(), name


def test_identity_3_a_list_in_two_pieces(gpu):
    case = cc.case("p2049")
    want_ = cc.want(case, "p2049")[0]
    P, A, k = len(case["lists"][0]), len(case["beams"]), 1031
    b = _buffers(case)
    c1 = _full(16)
    _call(gpu, b, P=k)
    gpu.synchronize()
    head = [_u32(b["d_res"])[:8].copy(), _u32(b["d_c"])[:8].astype(np.int64)]
    _call(gpu, b, P=P - k, poses=b["d_p"].data_ptr() + 16 * k, ranges=b["d_r"].data_ptr() + 4 * k * A,
          w=b["d_w"].data_ptr() + 4 * k, cast=c1.data_ptr())
    gpu.synchronize()
    assert _u32(b["d_r"])[:P * A].tobytes() == want_["ranges"].tobytes() and (_u32(b["d_r"])[P * A:] == GUARD_WORD).all()
    assert _u32(b["d_w"])[:P].tobytes() == want_["weights"].tobytes() and (_u32(b["d_w"])[P:] == GUARD_WORD).all()
    c0, c1 = head[1], _u32(c1)[:8].astype(np.int64)
    whole = want_["cast"].astype(np.int64)
    assert (c0[:5] + c1[:5]).tolist() == whole[:5].tolist() and max(c0[5], c1[5]) == whole[5]
    assert (c0[6] | c0[7] << 32) + (c1[6] | c1[7] << 32) == whole[6] | whole[7] << 32
    assert head[0].tobytes() == po.result_of(want_["weights"][:k], int(want_["result"][4])).tobytes()
    assert _u32(b["d_res"])[:8].tobytes() == po.result_of(want_["weights"][k:], int(want_["result"][4])).tobytes()


# ---- chains on one stream ----------------------------------------------------------------------------------------------------
def _seed_chain(oracle):
    """the CPU side of the first chain: E14's and E19's oracles (tests/seed_cases.py), then E22's and E17's on them"""
    a = sc.init_chain(oracle)
    P, s0 = sc.CHAIN_P, a["case"]["spec"]
    W, H = s0["width"], s0["height"]
    s = co.spec(**{k: s0[k] for k in ("origin_x", "origin_y", "resolution", "width", "height")}, max_steps=60, hit_lo=100,
                unknown_stops=1, table_half=10)
    grid = np.asarray(a["grid"], np.int8).reshape(H, W)
    poses = np.ascontiguousarray(a["words"]).view(F32).reshape(P, 4)
    beams, table = cc.fan(24), cc.byte_table(10)
    z = cc.scan_of(np.random.default_rng(5), s, poses[7], beams, grid, 0, 1, 3, nan_every=6, inf_every=0)
    o = co.cast_group(s, poses, beams, grid, z, 0, 1, table)
    est = eo.estimate(poses, o["weights"], eo.DEFAULT, int(o["result"][1]))
    kinds = {int(v) >> 28 for v in o["ranges"].reshape(-1)}
    assert {co.HIT, co.UNKNOWN} <= kinds and len(np.unique(o["weights"])) > 10 and int(o["cast"][4]) == 0   # the regime
    return dict(a=a, s=s, grid=grid, poses=poses, beams=beams, table=table, z=z, o=o, est=est)


def test_chain_map_seed_cast_estimate(gpu, oracle):
    """map_grid (E14) -> seed over its 0-cells (E19) -> cast against a scan (E22) -> estimate around E22's best pose
    (E17), all queued before anything is read"""
    import torch
    c = _seed_chain(oracle)
    a, s, grid, poses, beams, table, z, o, est = (c[k] for k in ("a", "s", "grid", "poses", "beams", "table", "z", "o", "est"))
    P, W, H = sc.CHAIN_P, s["width"], s["height"]
    gstride = (W * H + 3) & ~3
    d_counts, d_grid, d_kinds = _up(a["counts"].reshape(-1)), _full(gstride // 4 + 1), _full(5)
    d_head, d_beams, d_table, d_z = _up(a["table"].view(np.uint32)), _up(beams.view(np.uint32)), _up(table), _up(z.view(np.uint32))
    d_out, d_w, d_rng = _full(4 * (P + PAD)), _full(P + PAD), _full(P * 24 + PAD)
    d_r19, d_res, d_cast, d_est = _full(16), _full(16), _full(16), _full(eo.WORDS + 8)
    d_scr19 = _full(abi.seed_scratch_words(1, W, H))
    d_scr17 = torch.zeros(abi.estimate_scratch_words(1, P), dtype=torch.int32, device=torch.device("cuda:0"))
    gpu.map_grid_dev(d_counts.data_ptr(), W, H, abi.MapRule(**a["rule"]), 0, d_grid.data_ptr(), gstride,
                     d_kinds.data_ptr())
    gpu.seed_poses_dev(sc.spec_of(a["sspec"]), d_grid.data_ptr(), gstride, 0, d_head.data_ptr(), sc.CHAIN_H, 1, P,
                       sc.noise_of(a["noise"]), d_out.data_ptr(), 4 * (P + PAD), 0, 0, d_r19.data_ptr(),
                       d_scr19.data_ptr())
    gpu.cast_ranges_dev(spec_of(s), d_out.data_ptr(), 4 * (P + PAD), 0, 1, P, d_beams.data_ptr(), 24, d_grid.data_ptr(),
                        gstride, 0, d_z.data_ptr(), len(z), 0, 1, d_table.data_ptr(), d_rng.data_ptr(), P * 24 + PAD,
                        d_w.data_ptr(), P + PAD, d_res.data_ptr(), d_cast.data_ptr())
    gpu.estimate_poses_dev(d_out.data_ptr(), 4 * (P + PAD), 0, d_w.data_ptr(), P + PAD, 1, P,
                           abi.PoseEstimate.defaults(), d_res.data_ptr() + 4, 8, d_est.data_ptr(), d_scr17.data_ptr())
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_out, 4 * P), (d_w, P), (d_rng, P * 24), (d_r19, 8), (d_res, 8), (d_cast, 8), (d_est, eo.WORDS)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert d_grid.cpu().numpy().view(np.int8)[:W * H].tobytes() == grid.tobytes()
    assert _u32(d_out)[:4 * P].tobytes() == a["words"].tobytes()
    assert _u32(d_rng)[:P * 24].tobytes() == o["ranges"].tobytes() and _u32(d_w)[:P].tobytes() == o["weights"].tobytes()
    assert _u32(d_res)[:8].tobytes() == o["result"].tobytes() and _u32(d_cast)[:8].tobytes() == o["cast"].tobytes()
    assert _u32(d_est)[:eo.WORDS].tobytes() == est.tobytes()


def test_chain_merge_filter_cast_resample_cast(gpu):
    """merge_scans (E9) -> filter (E10) -> cast against the filtered scan, every 7th beam (E22) -> resample by the weights
    (E16) -> cast the new list (E22), all queued before anything is read; the filtered scan and the list in between are
    read at the end and the oracles chained on them"""
    import torch
    dev = torch.device("cuda:0")
    S, n, count, A, P = 2, 4000, 360, 51, 700
    batch = synth.make_batch(2026 + 22, S, n, noise_m=0.01, r0_range=(0.4, 1.6))
    pose2d = np.array([[1, 0, 0.05, 0, 1, 0.0], [0, -1, -0.05, 1, 0, 0.02]], F32)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    merge = abi.ScanMerge(-math.pi, math.pi, count, 0.0, 40.0, 0.1)
    f = fo.flt()
    case = cc.make(22, 130, 67, P, A, K=40, origin=(-3.2, -1.7), scale=(1.0, 0.2))
    s, grid, poses, table = case["spec"], case["grids"][0], case["lists"][0], case["table"]
    beams = abi.cast_beams(merge, 2, 7, A)
    gstride = (130 * 67 + 3) & ~3
    h_grid = np.zeros(gstride, np.int8)
    h_grid[:130 * 67] = grid.reshape(-1)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(S, n * 8)).to(dev)
    d_len = torch.full((S,), n, dtype=torch.int32, device=dev)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_r, d_i, d_ro, d_io = (torch.zeros(count, dtype=torch.float32, device=dev) for _ in range(4))
    d_hit = torch.zeros(1, dtype=torch.int32, device=dev)
    d_grid, d_beams, d_table, d_p = _up(h_grid), _up(beams.view(np.uint32)), _up(table), _up(poses.view(np.uint32))
    d_u = _up(np.array([0x9E3779B9], np.uint32))
    d_w1, d_w2, d_out = _full(P + PAD), _full(P + PAD), _full(4 * (P + PAD))
    d_rng = _full(P * A + PAD)
    d_res1, d_res2, d_c1, d_c2, d_r16 = _full(16), _full(16), _full(16), _full(16), _full(16)
    d_scr16 = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=dev)
    gpu.merge_scans_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), merge, d_r.data_ptr(),
                        d_i.data_ptr(), d_hit.data_ptr(), 0)
    gpu.filter_merged_scans_dev(d_r.data_ptr(), d_i.data_ptr(), 1, merge, abi.ScanFilter(**{k: f[k] for k, _ in
                                abi.ScanFilter._fields_}), d_ro.data_ptr(), d_io.data_ptr(), 0)
    gpu.cast_ranges_dev(spec_of(s), d_p.data_ptr(), 4 * P, 0, 1, P, d_beams.data_ptr(), A, d_grid.data_ptr(), gstride, 0,
                        d_ro.data_ptr(), count, 2, 7, d_table.data_ptr(), 0, 0, d_w1.data_ptr(), P + PAD,
                        d_res1.data_ptr(), d_c1.data_ptr())
    gpu.resample_poses_dev(d_w1.data_ptr(), P + PAD, d_p.data_ptr(), 4 * P, 0, 1, P, P, d_u.data_ptr(), 0, 0, 0, 0,
                           d_out.data_ptr(), 4 * (P + PAD), 0, 0, d_r16.data_ptr(), d_scr16.data_ptr())
    gpu.cast_ranges_dev(spec_of(s), d_out.data_ptr(), 4 * (P + PAD), 0, 1, P, d_beams.data_ptr(), A, d_grid.data_ptr(),
                        gstride, 0, d_ro.data_ptr(), count, 2, 7, d_table.data_ptr(), d_rng.data_ptr(), P * A + PAD,
                        d_w2.data_ptr(), P + PAD, d_res2.data_ptr(), d_c2.data_ptr())
    gpu.synchronize()  # nothing was read until here
    merged, z = d_r.cpu().numpy(), d_ro.cpu().numpy()
    want_z, n_sh, n_sp = fo.filter_scan(merged, abi.scan_merge_edges(merge)[1], f)
    assert z.view(np.uint32).tobytes() == np.ascontiguousarray(want_z, F32).view(np.uint32).tobytes()
    used = co.beam_ranges(z, 2, 7, A)
    assert np.isfinite(used).sum() > A // 2 and n_sh + n_sp > 0                                   # the regime
    o1 = co.cast_group(s, poses, beams, grid, z, 2, 7, table)
    moved, _, r16 = ro.resample(o1["weights"], poses, P, 0x9E3779B9, None)
    moved = np.ascontiguousarray(moved, F32)
    o2 = co.cast_group(s, moved, beams, grid, z, 2, 7, table)
    assert len(np.unique(o1["weights"])) > 10 and moved.tobytes() != poses.tobytes()
    for t, k in ((d_w1, P), (d_w2, P), (d_out, 4 * P), (d_rng, P * A), (d_res1, 8), (d_res2, 8), (d_c1, 8), (d_c2, 8),
                 (d_r16, 8)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert _u32(d_w1)[:P].tobytes() == o1["weights"].tobytes() and _u32(d_res1)[:8].tobytes() == o1["result"].tobytes()
    assert _u32(d_c1)[:8].tobytes() == o1["cast"].tobytes() and _u32(d_r16)[:8].tobytes() == r16.tobytes()
    assert _u32(d_out)[:4 * P].tobytes() == moved.view(np.uint32).tobytes()
    assert _u32(d_rng)[:P * A].tobytes() == o2["ranges"].tobytes() and _u32(d_w2)[:P].tobytes() == o2["weights"].tobytes()
    assert _u32(d_res2)[:8].tobytes() == o2["result"].tobytes() and _u32(d_c2)[:8].tobytes() == o2["cast"].tobytes()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_door_refusals_change_nothing(gpu):
    lib = abi.load_library()
    case = cc.case("p63")
    s, poses, beams, grid = spec_of(case["spec"]), case["lists"][0], case["beams"], case["grids"][0]
    z, table = case["measured"][0], case["table"]
    out = [np.full(n, GUARD_WORD, np.uint32) for n in (len(poses) * len(beams) + 1, len(poses) + 1, 9, 9)]

    def door(h=gpu._h, spec=s, poses_=poses.ctypes.data, P=len(poses), beams_=beams.ctypes.data, A=len(beams),
             grid_=grid.ctypes.data, z_=z.ctypes.data, n=len(z), first=0, step=1, table_=table.ctypes.data,
             r_=out[0].ctypes.data, w_=out[1].ctypes.data, res_=out[2].ctypes.data, cast_=out[3].ctypes.data):
        return lib.rplgpu_cast_ranges(h, C.byref(spec) if spec is not None else None, poses_, P, beams_, A, grid_, z_, n,
                                      first, step, table_, r_, w_, res_, cast_)

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(h=None), dict(spec=None), dict(spec=abi.RangeCast.defaults(max_steps=0)), dict(poses_=None),
               dict(beams_=None), dict(grid_=None), dict(cast_=None), dict(P=0), dict(P=abi.MAX_POSES + 1), dict(A=0),
               dict(A=16385), dict(r_=None, z_=None), dict(table_=None), dict(w_=None), dict(res_=None), dict(n=0),
               dict(first=len(z)), dict(step=len(z))):
        assert door(**kw) == bad, kw
    assert all((o == GUARD_WORD).all() for o in out)
    o = cc.want(case, "p63")[0]
    assert door() == abi.OK and out[0][:-1].tobytes() == o["ranges"].tobytes() and out[1][:-1].tobytes() == o["weights"].tobytes()
    assert out[2][:8].tobytes() == o["result"].tobytes() and out[3][:8].tobytes() == o["cast"].tobytes()
    assert all(v[-1] == GUARD_WORD for v in out)


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu):
    import torch
    case = cc.case("groups_own")
    b = _buffers(case)
    P, A = b["P"], b["A"]
    host = np.zeros(64, np.uint32)
    hp = host.ctypes.data + (-host.ctypes.data % 16)
    refused = []

    def call(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            _call(gpu, b, **kw)
        refused.append(kw)
        return e.value.code

    bad = abi.ERR_INVALID_ARG
    for field, value in (("origin_x", math.nan), ("origin_y", math.inf), ("resolution", 0.0), ("resolution", -1.0),
                         ("width", 0), ("height", 4097), ("max_steps", 0), ("max_steps", 8193), ("hit_lo", 0),
                         ("hit_lo", 128), ("unknown_stops", 2), ("table_half", 4097)):          # the spec check
        assert call(spec=spec_of(dict(case["spec"], **{field: value}))) == bad, field
    assert call(G=0) == bad and call(G=65536) == bad
    assert call(P=0) == bad and call(P=abi.MAX_POSES + 1, pstride=1 << 23, wstride=1 << 21, rstride=1 << 30) == bad
    assert call(A=0) == bad and call(A=16385, rstride=1 << 30, mstride=1 << 20) == bad
    assert call(P=1 << 20, A=257, pstride=1 << 22, wstride=1 << 20, rstride=1 << 30, mstride=1 << 20) == bad   # P A > 2^28
    for k in ("poses", "beams", "grid", "cast", "table", "w", "res"):          # required pointers (three with d_measured)
        assert call(**{k: 0}) == bad, k
    assert call(ranges=0, z=0) == bad                                          # neither output
    names = dict(poses="d_p", beams="d_b", grid="d_g", z="d_z", ranges="d_r", w="d_w", res="d_res", cast="d_c")
    for k, step in (("poses", 4), ("poses", 8), ("beams", 4), ("grid", 1), ("grid", 2), ("z", 2), ("ranges", 1),
                    ("ranges", 2), ("w", 2), ("res", 1), ("cast", 2)):         # alignment
        assert call(**{k: b[names[k]].data_ptr() + step}) == bad, (k, step)
    assert call(pstride=4 * P - 4) == bad and call(pstride=4 * P + 2) == bad and call(pstride=0) == bad
    cells = case["spec"]["width"] * case["spec"]["height"]
    assert call(gstride=((cells + 3) & ~3) - 4) == bad and call(gstride=b["gstride"] + 2) == bad and call(gstride=0) == bad
    assert call(rstride=P * A - 1) == bad and call(wstride=P - 1) == bad
    assert call(first=b["mstride"] - (A - 1) * b["step"]) == bad and call(step=b["mstride"]) == bad and call(mstride=0) == bad
    for k in ("poses", "beams", "grid", "z", "table", "ranges", "w", "res", "cast"):   # plain host memory
        assert call(**{k: hp}) == bad, k
    lib = abi.load_library()
    args = (b["d_p"].data_ptr(), b["pstride"], 1, b["G"], P, b["d_b"].data_ptr(), A, b["d_g"].data_ptr(), b["gstride"],
            1, 0, 0, 0, 1, 0, b["d_r"].data_ptr(), b["rstride"], 0, 0, 0, b["d_c"].data_ptr())
    assert lib.rplgpu_cast_ranges_dev(None, C.byref(b["spec"]), *args) == bad
    assert lib.rplgpu_cast_ranges_dev(gpu._h, None, *args) == bad
    assert len(refused) >= 50
    gpu.synchronize()
    torch.cuda.synchronize()
    for k in ("d_r", "d_w", "d_res", "d_c"):                                   # nothing was queued
        assert (_u32(b[k]) == GUARD_WORD).all(), k
    _inputs_unchanged(b)
    _call(gpu, b)                                                              # then a good call on the same buffers
    gpu.synchronize()
    _check(_read(b), cc.want(case, "groups_own"))
    # without d_measured the weight, result and table arguments are ignored: NULL, misaligned or host memory
    b2 = _buffers(case, weights=False)
    _call(gpu, b2, w=hp + 1, res=3, table=hp, wstride=0, mstride=0, first=99, step=99)
    gpu.synchronize()
    _check(_read(b2), cc.want(case, "groups_own"))
