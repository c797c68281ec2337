"""E18 on the device: rplgpu_sample_motion_dev against tests/motion_oracle.py byte for byte — the M deltas and the eight
result words of every group, the guard words behind every group's deltas and behind the result words, and the unchanged
odometry.  The inputs and their regime checks live in tests/motion_cases.py."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import estimate_oracle as eo
from tests import motion_cases as mc
from tests import motion_oracle as mo
from tests import pose_cases as pc
from tests import pose_oracle as po
from tests import resample_oracle as ro

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD_WORD = 0x5A5A5A5A
PAD = 5  # guard deltas behind every group's list


def _up(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda:0"))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _buffers(case, pad=PAD):
    """Device copies of a case's odometry (followed by eight guard floats) and guarded outputs."""
    import torch
    dev = torch.device("cuda:0")
    G, M = case["G"], case["M"]
    L = len(case["odom"])
    h_o = np.full((L + 1, 8), 123.0, F32)
    h_o[:L] = case["odom"]
    b = dict(G=G, M=M, spec=mc.spec_of(case["spec"]), h_o=h_o, d_o=_up(h_o), opg=1 if L > 1 else 0,
             dstride=4 * (M + pad))
    b["d_delta"] = torch.full((G * 4 * (M + pad),), GUARD_WORD, dtype=torch.int32, device=dev)
    b["d_res"] = torch.full((8 * G + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    return b


def _call(gpu, b, **kw):
    a = dict(odom=b["d_o"].data_ptr(), opg=b["opg"], G=b["G"], M=b["M"], spec=b["spec"],
             delta=b["d_delta"].data_ptr(), dstride=b["dstride"], res=b["d_res"].data_ptr())
    a.update(kw)
    gpu.sample_motion_dev(a["odom"], a["opg"], a["G"], a["M"], a["spec"], a["delta"], a["dstride"], a["res"])


def _outputs_untouched(b):
    for k in ("d_delta", "d_res"):
        assert (_u32(b[k]) == GUARD_WORD).all(), k


def _run(gpu, case, **kw):
    """-> (delta words (G, M, 4), result (G, 8)); guards and the odometry checked"""
    b = _buffers(case, **kw)
    _call(gpu, b)
    gpu.synchronize()
    G, M = b["G"], b["M"]
    assert b["d_o"].cpu().numpy().tobytes() == b["h_o"].tobytes()
    res = _u32(b["d_res"])
    assert (res[8 * G:] == GUARD_WORD).all()
    delta = _u32(b["d_delta"]).reshape(G, b["dstride"])
    assert (delta[:, 4 * M:] == GUARD_WORD).all()
    return delta[:, :4 * M].reshape(G, M, 4), res[:8 * G].reshape(G, 8)


def _check(got, want_):
    words, res = got
    assert words.shape == want_[0].shape and res.shape == want_[1].shape
    for g in range(len(res)):
        if words[g].tobytes() != want_[0][g].tobytes():
            bad = np.flatnonzero((words[g] != want_[0][g]).any(axis=1))
            j = int(bad[0])
            print(f"group {g}: {len(bad)} of {len(words[g])} outputs differ, first {j}: "
                  f"{[hex(v) for v in words[g][j]]} want {[hex(v) for v in want_[0][g][j]]}, Z {want_[2][g][j]}")
        if res[g].tobytes() != want_[1][g].tobytes():
            print(f"group {g}: result {res[g].tolist()} want {want_[1][g].tolist()}")
        assert words[g].tobytes() == want_[0][g].tobytes(), g
        assert res[g].tobytes() == want_[1][g].tobytes(), g


# ---- tile edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", mc.EDGE_M)
def test_tile_edges(gpu, M):
    case = mc.edge_case(M)
    want_ = mc.want(case, f"edge{M}")
    mc.edge_regime(case, want_)
    _check(_run(gpu, case), want_)


def test_largest_list(gpu):
    case = mc.big_case()
    want_ = mc.want(case, "big")
    mc.big_regime(case, want_)
    _check(_run(gpu, case), want_)


# ---- counters ---------------------------------------------------------------------------------------------------------
def test_wrap_of_the_first_counter_word(gpu):
    case = mc.wrap_case()
    want_ = mc.want(case, "wrap")
    mc.wrap_regime(case, want_)
    _check(_run(gpu, case), want_)


def test_a_piece_of_a_list(gpu):
    whole, piece = mc.piece_cases()
    a, b = mc.want(whole, "whole"), mc.want(piece, "piece")
    assert b[0][0].tobytes() == a[0][0, 1000:2000].tobytes() != a[0][0, :1000].tobytes()
    got_whole, got_piece = _run(gpu, whole), _run(gpu, piece)
    _check(got_whole, a)
    _check(got_piece, b)
    assert got_piece[0][0].tobytes() == got_whole[0][0, 1000:2000].tobytes()


@pytest.mark.parametrize("kind", mc.COUNTER_KINDS)
def test_counters(gpu, kind):
    case = mc.counter_case(kind)
    want_ = mc.want(case, f"counter_{kind}")
    mc.counter_regime(kind, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("ppg", [0, 1])
def test_groups(gpu, ppg):
    case = mc.groups_case(ppg)
    want_ = mc.want(case, f"groups{ppg}")
    mc.groups_regime(case, want_)
    _check(_run(gpu, case, pad=PAD + 59 * ppg), want_)        # a stride larger than needed, twice


# ---- Z through the floats ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 2])
def test_z_through_the_floats(gpu, which):
    case = mc.z_case(which)
    want_ = mc.want(case, f"z{which}")
    mc.z_regime(case, which, want_)
    words, res = _run(gpu, case)
    f = mc.floats_of(words)[0]
    # against the integer writer, draw by draw, and against result words 1 - 5
    z1 = [mo.z_python(case["spec"], 0, j, 1) for j in range(case["M"])]
    zw = [mo.z_python(case["spec"], 0, j, which) for j in range(case["M"])]
    zo = [mo.z_python(case["spec"], 0, j, 2 - which) for j in range(case["M"])]
    assert f[:, 2].astype(np.int64).tolist() == z1
    assert (f[:, 1].astype(np.float64) * 2.0 ** 39).tolist() == zw
    allz = z1 + zw + zo
    assert int(res[0, 1]) == max(abs(z) for z in allz)
    assert mo.sum_z(res[0]) == sum(allz) and mo.sum_z2(res[0]) == sum(z * z for z in allz)
    _check((words, res), want_)


# ---- floats -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zero", "denormal", "huge", "special", "ordinary"])
def test_floats(gpu, name):
    case, regime = dict(zero=(mc.zero_scale_case, mc.zero_scale_regime), denormal=(mc.denormal_case, mc.denormal_regime),
                        huge=(mc.huge_case, mc.huge_regime), special=(mc.special_case, mc.special_regime),
                        ordinary=(mc.ordinary_case, mc.ordinary_regime))[name]
    case = case()
    want_ = mc.want(case, name)
    regime(case, want_)
    _check(_run(gpu, case), want_)


def test_zero_scales_through_the_move_are_one_delta(gpu):
    """E18 with every scale 0 writes M equal deltas: E16 with n_delta = M on that list is E16 with n_delta = 1 and the
    one delta — two kernels held to each other, and both to E16's oracle"""
    import torch
    dev = torch.device("cuda:0")
    case = mc.zero_scale_case()
    M = case["M"]
    P = 700
    want_ = mc.want(case, "zero")
    rng = np.random.default_rng(16)
    th = rng.uniform(-3, 3, P)
    poses = np.stack([np.cos(th), np.sin(th), rng.uniform(-5, 5, P), rng.uniform(-5, 5, P)], 1).astype(F32)
    w = rng.integers(0, 1000, P).astype(np.uint32)
    u = 0x12345678
    one = mc.floats_of(want_[0])[0, :1]
    out_want, _, r16_want = ro.resample(w, poses, M, u, one)
    assert out_want.tobytes() != poses[ro.ancestors_search(w, M, u)].tobytes()     # the delta moves
    b = _buffers(case, pad=0)
    d_p, d_w, d_u = _up(poses), _up(w), _up(np.array([u], np.uint32))
    d_out = torch.full((2, 4 * M + 8), GUARD_WORD, dtype=torch.int32, device=dev)
    d_r16 = torch.full((2, 8), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=dev)
    _call(gpu, b)
    for k, n_delta in enumerate((M, 1)):
        gpu.resample_poses_dev(d_w.data_ptr(), P, d_p.data_ptr(), 4 * P, 0, 1, P, M, d_u.data_ptr(),
                               b["d_delta"].data_ptr(), n_delta, 4 * M, 1, d_out[k].data_ptr(), 4 * M, 0, 0,
                               d_r16[k].data_ptr(), d_scr.data_ptr())
    gpu.synchronize()
    out = _u32(d_out)
    assert (out[:, 4 * M:] == GUARD_WORD).all()
    assert out[0, :4 * M].tobytes() == out[1, :4 * M].tobytes() == out_want.tobytes()
    assert _u32(d_r16)[0].tobytes() == _u32(d_r16)[1].tobytes() == r16_want.tobytes()
    assert _u32(b["d_delta"]).tobytes() == want_[0][0].tobytes()


# ---- the chain, between the real kernels ------------------------------------------------------------------------------
def test_chain_sample_resample_score_estimate(gpu, oracle):
    """sample (E18) -> resample and move with n_delta = M (E16) -> score (E15) -> estimate around E15's best pose
    (E17), all queued before anything is read, each against its own oracle"""
    import torch
    dev = torch.device("cuda:0")
    P = M = 2049
    case = pc.layout_case(P)
    w1 = pc.case_want(oracle, case, f"layout{P}")[0][0]         # the weights of the list: what a previous score left
    poses = case["poses"][0]
    sig = mc.SIGMA_Z
    odom = np.array([1, 0, 0.02, 1, 0, 0.01 / (2 * sig), 0.01 / sig, 0.01 / (2 * sig)], F32)
    mcase = dict(odom=odom[None], G=1, M=M, spec=dict(seed=0xC0FFEE, step=41, first=0))
    d_words, d_res_want, _ = mc.want(mcase, "chain")
    delta = mc.floats_of(d_words)[0]
    u = 0x9E3779B9
    moved, anc, r16_want = ro.resample(w1, poses, M, u, delta)
    x, y = pc.case_points(oracle, case, 0)
    w2, r15_want, _ = po.score_points(x, y, moved, case["spec"], pc.case_field(case, 0), po.weight_bincount)
    best = int(r15_want[1])
    est_want = eo.estimate(moved, w2, eo.DEFAULT, best)
    # the regime, all from the oracles: the noise moved every output its own way, the moved list still sees the
    # field, its best pose is not pose 0 and the gate holds some poses and not all
    assert len({d.tobytes() for d in d_words[0]}) > 0.99 * M and d_res_want[0, 0] == 0
    assert moved.tobytes() != ro.move(poses[anc], delta[:1]).tobytes()
    assert int(r15_want[0]) > 0 and best != 0 and 2 <= est_want[4] < M and est_want[0] == 0
    s = case["spec"]
    spec = abi.PoseScore(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"])
    B, n = case["batch"].shape
    d_nodes = _up(np.ascontiguousarray(case["batch"]).view(np.uint8).reshape(B, n * 8))
    d_lens = _up(np.asarray(case["lens"], np.int32))
    d_pose2d = _up(case["pose2d"])
    cells = s["width"] * s["height"]
    fstride = (cells + 3) & ~3
    h_field = np.zeros(fstride, np.int8)
    h_field[:cells] = case["fields"][0].reshape(-1)
    d_field = _up(h_field)
    d_poses, d_w1, d_u, d_odom = _up(poses), _up(w1), _up(np.array([u], np.uint32)), _up(odom)
    full = lambda k: torch.full((k,), GUARD_WORD, dtype=torch.int32, device=dev)  # noqa: E731
    d_delta, d_out, d_w2 = full(4 * (M + PAD)), full(4 * (M + PAD)), full(M + PAD)
    d_r18, d_r16, d_r15, d_est = full(16), full(16), full(16), full(eo.WORDS + 8)
    d_scr16 = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=dev)
    d_scr17 = torch.zeros(abi.estimate_scratch_words(1, M), dtype=torch.int32, device=dev)

    gpu.sample_motion_dev(d_odom.data_ptr(), 0, 1, M, mc.spec_of(mcase["spec"]), d_delta.data_ptr(), 4 * (M + PAD),
                          d_r18.data_ptr())
    gpu.resample_poses_dev(d_w1.data_ptr(), P, d_poses.data_ptr(), 4 * P, 0, 1, P, M, d_u.data_ptr(),
                           d_delta.data_ptr(), M, 4 * (M + PAD), 1, d_out.data_ptr(), 4 * (M + PAD), 0, 0,
                           d_r16.data_ptr(), d_scr16.data_ptr())
    gpu.score_poses_dev(d_nodes.data_ptr(), n, d_lens.data_ptr(), B, case["group"], case["p"], 0,
                        d_pose2d.data_ptr(), spec, d_out.data_ptr(), M, 4 * (M + PAD), 0, d_field.data_ptr(), fstride,
                        0, d_w2.data_ptr(), M + PAD, d_r15.data_ptr(), 0)
    gpu.estimate_poses_dev(d_out.data_ptr(), 4 * (M + PAD), 0, d_w2.data_ptr(), M + PAD, 1, M,
                           abi.PoseEstimate.defaults(), d_r15.data_ptr() + 4, 8, d_est.data_ptr(), d_scr17.data_ptr())
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_delta, 4 * M), (d_out, 4 * M), (d_w2, M), (d_r18, 8), (d_r16, 8), (d_r15, 8), (d_est, eo.WORDS)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert _u32(d_delta)[:4 * M].tobytes() == d_words[0].tobytes()
    assert _u32(d_r18)[:8].tobytes() == d_res_want[0].tobytes()
    assert _u32(d_out)[:4 * M].tobytes() == moved.tobytes() and _u32(d_r16)[:8].tobytes() == r16_want.tobytes()
    assert _u32(d_w2)[:M].tobytes() == w2.tobytes() and _u32(d_r15)[:8].tobytes() == r15_want.tobytes()
    assert _u32(d_est)[:eo.WORDS].tobytes() == est_want.tobytes()
    assert d_odom.cpu().numpy().tobytes() == odom.tobytes() and d_poses.cpu().numpy().tobytes() == poses.tobytes()


# ---- the door, refusals -----------------------------------------------------------------------------------------------
def test_host_buffers_one_group(gpu):
    for case, key in ((mc.edge_case(1025), "edge1025"), (mc.huge_case(), "huge"), (mc.z_case(0), "z0"),
                      (mc.wrap_case(), "wrap")):
        delta, res = gpu.sample_motion(case["odom"][0], case["M"], mc.spec_of(case["spec"]))
        want_ = mc.want(case, key)
        assert delta.view(np.uint32).tobytes() == want_[0][0].tobytes() and res.tobytes() == want_[1][0].tobytes()
    lib = abi.load_library()
    od = mc.ordinary_odom()
    delta = np.full(24, 7.0, F32)
    res = np.full(12, GUARD_WORD, np.uint32)
    good = abi.MotionNoise.defaults(seed=4)

    def door(od_=od.ctypes.data, M=2, spec=good, delta_=delta.ctypes.data, res_=res.ctypes.data, h=gpu._h):
        return lib.rplgpu_sample_motion(h, od_, M, C.byref(spec) if spec is not None else None, delta_, res_)

    bad = abi.ERR_INVALID_ARG
    assert door(od_=0) == bad and door(spec=None) == bad and door(delta_=0) == bad and door(res_=0) == bad
    assert door(h=None) == bad and door(M=0) == bad and door(M=abi.MAX_POSES + 1) == bad
    assert (delta == 7.0).all() and (res == GUARD_WORD).all()
    words, want_res, _ = mo.sample(od, 2, dict(seed=4, step=0, first=0))
    assert door() == abi.OK and delta[:8].view(np.uint32).tobytes() == words.tobytes()
    assert res[:8].tobytes() == want_res.tobytes() and (delta[8:] == 7.0).all() and (res[8:] == GUARD_WORD).all()


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu):
    import torch
    case = mc.groups_case(1, G=3, M=1100)
    b = _buffers(case)
    G, M = b["G"], b["M"]
    host = np.zeros(64, np.uint32)
    hp = host.ctypes.data + (-host.ctypes.data % 16)

    def call(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            _call(gpu, b, **kw)
        return e.value.code

    bad = abi.ERR_INVALID_ARG
    assert call(G=0) == bad and call(G=65536) == bad
    assert call(M=0) == bad and call(M=abi.MAX_POSES + 1, dstride=1 << 23) == bad
    for k in ("odom", "delta", "res"):                                    # required pointers
        assert call(**{k: 0}) == bad, k
    for k, step in (("odom", 4), ("odom", 8), ("delta", 4), ("delta", 8), ("res", 1), ("res", 2)):  # alignment
        t = b[dict(odom="d_o", delta="d_delta", res="d_res")[k]]
        assert call(**{k: t.data_ptr() + step}) == bad, (k, step)
    assert call(dstride=4 * M - 4) == bad and call(dstride=4 * M + 2) == bad and call(dstride=0) == bad
    for k in ("odom", "delta", "res"):                                    # plain host memory, pointer by pointer
        assert call(**{k: hp}) == bad, k
    lib = abi.load_library()
    args = (b["d_o"].data_ptr(), 1, G, M)
    tail = (b["d_delta"].data_ptr(), b["dstride"], b["d_res"].data_ptr())
    assert lib.rplgpu_sample_motion_dev(None, *args, C.byref(b["spec"]), *tail) == bad
    assert lib.rplgpu_sample_motion_dev(gpu._h, *args, None, *tail) == bad            # a NULL spec
    gpu.synchronize()
    torch.cuda.synchronize()
    _outputs_untouched(b)
    assert b["d_o"].cpu().numpy().tobytes() == b["h_o"].tobytes()
    _check(_run(gpu, case), mc.want(case))                                # then a good call on the case
    # a result pointer that is only 4-byte aligned is allowed: the 64-bit sums are two words each
    b2 = _buffers(case)
    _call(gpu, b2, res=b2["d_res"].data_ptr() + 4)
    gpu.synchronize()
    res = _u32(b2["d_res"])
    assert res[0] == GUARD_WORD and res[1 + 8 * G:].tolist() == [GUARD_WORD] * 7
    assert res[1:1 + 8 * G].tobytes() == mc.want(case)[1].tobytes()
