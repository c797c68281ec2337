"""E17 on the device: rplgpu_estimate_poses_dev against tests/estimate_oracle.py byte for byte — the 72 result words
of every group, the guard words behind the result words and behind the scratch, and the unchanged poses, weights and
centre words.  The inputs and their regime checks live in tests/estimate_cases.py."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import estimate_cases as ec
from tests import estimate_oracle as eo
from tests import pose_cases as pc
from tests import resample_oracle as ro

pytestmark = pytest.mark.gpu
F32 = np.float32
U32_MAX = 0xFFFFFFFF
GUARD_WORD = 0x5A5A5A5A
PAD = 5  # guard words (or poses) behind every group's part of an array
W = eo.WORDS


def _up(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda:0"))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _buffers(case, pad=PAD, cstride=1):
    """Device copies of a case's inputs (every group's part followed by `pad` guard entries; the centre words
    `cstride` apart, at word 1 of each stretch as in E15's result) and guarded outputs."""
    import torch
    dev = torch.device("cuda:0")
    L, P, _ = case["poses"].shape
    G = case["G"]
    b = dict(G=G, P=P, spec=ec.spec_of(case["spec"]))
    h_p = np.full((L, 4 * (P + pad)), 123.0, F32)
    h_p[:, :4 * P] = case["poses"].reshape(L, 4 * P)
    b.update(h_p=h_p, d_p=_up(h_p), pstride=4 * (P + pad), ppg=1 if L > 1 else 0)
    b.update(h_w=None, d_w=None, wstride=0, h_c=None, d_c=None, cstride=0, c_off=0)
    if case["w"] is not None:
        h_w = np.full((G, P + pad), GUARD_WORD, np.uint32)
        h_w[:, :P] = case["w"]
        b.update(h_w=h_w, d_w=_up(h_w), wstride=P + pad)
    if case["center"] is not None:
        h_c = np.full((G, cstride), GUARD_WORD, np.uint32)
        off = 1 if cstride > 1 else 0
        h_c[:, off] = case["center"]
        b.update(h_c=h_c, d_c=_up(h_c), cstride=cstride, c_off=off)
    words = abi.estimate_scratch_words(G, P)
    b["words"] = words
    b["d_res"] = torch.full((W * G + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    b["d_scr"] = torch.full((words + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    return b


def _call(gpu, b, **kw):
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    a = dict(poses=ptr(b["d_p"]), pstride=b["pstride"], ppg=b["ppg"], w=ptr(b["d_w"]), wstride=b["wstride"],
             G=b["G"], P=b["P"], spec=b["spec"], center=ptr(b["d_c"]) + 4 * b["c_off"] if b["d_c"] is not None else 0,
             cstride=b["cstride"], res=ptr(b["d_res"]), scr=ptr(b["d_scr"]))
    a.update(kw)
    gpu.estimate_poses_dev(a["poses"], a["pstride"], a["ppg"], a["w"], a["wstride"], a["G"], a["P"], a["spec"],
                           a["center"], a["cstride"], a["res"], a["scr"])


def _inputs_unchanged(b):
    assert b["d_p"].cpu().numpy().tobytes() == b["h_p"].tobytes()
    if b["d_w"] is not None:
        assert _u32(b["d_w"]).tobytes() == b["h_w"].tobytes()
    if b["d_c"] is not None:
        assert _u32(b["d_c"]).tobytes() == b["h_c"].tobytes()


def _outputs_untouched(b):
    for k in ("d_res", "d_scr"):
        assert (_u32(b[k]) == GUARD_WORD).all(), k


def _run(gpu, case, **kw):
    """-> result (G, 72) uint32; guards and inputs checked"""
    b = _buffers(case, **kw)
    _call(gpu, b)
    gpu.synchronize()
    _inputs_unchanged(b)
    res = _u32(b["d_res"])
    assert (res[W * b["G"]:] == GUARD_WORD).all()
    assert (_u32(b["d_scr"])[b["words"]:] == GUARD_WORD).all()
    return res[:W * b["G"]].reshape(b["G"], W)


def _check(got, want_):
    assert got.shape == want_.shape
    for g in range(len(want_)):
        if got[g].tobytes() != want_[g].tobytes():
            bad = np.flatnonzero(got[g] != want_[g])
            print(f"group {g}: words {bad.tolist()} differ; head {got[g][:8].tolist()} want {want_[g][:8].tolist()}")
            for m in sorted({(int(k) - 8) // 4 for k in bad if k >= 8}):
                print(f"  sum {m % 8} of set {m // 8}: {eo.value_of(got[g][8 + 4 * m:12 + 4 * m])} want "
                      f"{eo.value_of(want_[g][8 + 4 * m:12 + 4 * m])}")
        assert got[g].tobytes() == want_[g].tobytes(), g


# ---- tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ec.EDGE_P)
def test_tile_edges(gpu, P):
    case = ec.edge_case(P)
    want_ = ec.want(case, f"edge{P}")
    ec.edge_regime(case, want_)
    _check(_run(gpu, case), want_)


# ---- quantisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xy_scale", [1024.0, 1000.0])
def test_quantisation(gpu, xy_scale):
    case = ec.quant_case(xy_scale)
    ec.quant_regime(case)
    _check(_run(gpu, case), ec.want(case, f"quant{xy_scale}"))


# ---- gate borders -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ec.GATE_KINDS)
def test_gate_borders(gpu, kind):
    case = ec.gate_case(kind)
    want_ = ec.want(case, f"gate_{kind}")
    ec.gate_regime(case, kind, want_)
    _check(_run(gpu, case), want_)


# ---- extremes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cancel", [False, True])
def test_every_weight_and_coordinate_at_its_maximum(gpu, cancel):
    case = ec.extreme_case(2049, cancel)
    want_ = ec.want(case, f"extreme{cancel}")
    ec.extreme_regime(case, want_, cancel)
    _check(_run(gpu, case), want_)


def test_largest_list(gpu):
    case = ec.big_case()
    want_ = ec.want(case, "big")
    ec.extreme_regime(case, want_)
    assert eo.tiles(case["poses"].shape[1]) == 1024
    _check(_run(gpu, case), want_)


# ---- weights NULL -----------------------------------------------------------------------------------------------------------
def test_weights_null(gpu):
    case = dict(ec.edge_case(1025), w=None)
    want_ = ec.want(case, "null1025")
    assert want_.tobytes() == ec.want(dict(case, w=np.ones((case["G"], 1025), np.uint32))).tobytes()
    assert (want_[:, 8] == want_[:, 2]).all()                     # W is the number of poses in range
    _check(_run(gpu, case), want_)


# ---- groups -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppg,cstride", [(0, 1), (1, 8)])
def test_groups(gpu, ppg, cstride):
    case = ec.groups_case(ppg)
    want_ = ec.want(case, f"groups{ppg}")
    ec.groups_regime(case, want_)
    _check(_run(gpu, case, pad=PAD + 59 * ppg, cstride=cstride), want_)  # strides larger than needed, twice


def test_center_null_and_one_shared_word(gpu):
    case = ec.groups_case(0)
    null = dict(case, center=None)
    want0 = ec.want(null, "groups_c0")
    assert (want0[:, 1] == 0).all() and want0.tobytes() != ec.want(case, "groups0").tobytes()
    _check(_run(gpu, null), want0)
    one = dict(ec.edge_case(1025), center=np.array([1024], np.uint32))     # G = 1: center_stride 0 is allowed
    one["w"], one["G"] = one["w"][:1], 1
    b = _buffers(one)
    _call(gpu, b, cstride=0)
    gpu.synchronize()
    _check(_u32(b["d_res"])[:W].reshape(1, W), ec.want(one))


# ---- identities between real kernels ----------------------------------------------------------------------------------------
def test_resampled_with_equal_weights_is_the_list_itself(gpu):
    """with equal weights and M = P, E16 copies the list (a[j] = j): E17 of its output with NULL weights is E17 of
    the input with w = 1; and E16's S is E17's W of set 0 on the weighted list"""
    import torch
    dev = torch.device("cuda:0")
    P = 2049
    case = ec.edge_case(P)
    poses = case["poses"][0]
    d_p = _up(poses)
    h_w = np.full(P, 77, np.uint32)
    d_w = _up(h_w)
    d_out = torch.full((4 * P + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_r16 = torch.full((8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr16 = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=dev)
    d_res = torch.full((3 * W + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr = torch.full((abi.estimate_scratch_words(1, P) + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    spec = abi.PoseEstimate.defaults()
    gpu.resample_poses_dev(d_w.data_ptr(), P, d_p.data_ptr(), 4 * P, 0, 1, P, P, 0, 0, 0, 0, 0, d_out.data_ptr(),
                           4 * P, 0, 0, d_r16.data_ptr(), d_scr16.data_ptr())
    gpu.estimate_poses_dev(d_out.data_ptr(), 4 * P, 0, 0, 0, 1, P, spec, 0, 0, d_res.data_ptr(), d_scr.data_ptr())
    gpu.estimate_poses_dev(d_p.data_ptr(), 4 * P, 0, 0, 0, 1, P, spec, 0, 0, d_res.data_ptr() + 4 * W,
                           d_scr.data_ptr())
    gpu.estimate_poses_dev(d_p.data_ptr(), 4 * P, 0, d_w.data_ptr(), P, 1, P, spec, 0, 0,
                           d_res.data_ptr() + 8 * W, d_scr.data_ptr())
    gpu.synchronize()
    res = _u32(d_res)
    assert (res[3 * W:] == GUARD_WORD).all() and (_u32(d_scr)[-8:] == GUARD_WORD).all()
    res = res[:3 * W].reshape(3, W)
    assert _u32(d_out)[:4 * P].tobytes() == poses.tobytes()
    want1 = eo.estimate(poses, None, eo.DEFAULT)
    assert res[0].tobytes() == res[1].tobytes() == want1.tobytes()
    r16 = _u32(d_r16)
    assert want1[0] & 2 == 0 and eo.value_of(res[2][8:12]) == 77 * P == int(r16[0]) | int(r16[1]) << 32
    assert res[2].tobytes() == eo.estimate(poses, h_w, eo.DEFAULT).tobytes()
    assert poses.tobytes() == d_p.cpu().numpy().tobytes() and _u32(d_w).tobytes() == h_w.tobytes()


# ---- the chain, between the real kernels ------------------------------------------------------------------------------------
def test_chain_score_estimate_resample_estimate(gpu, oracle):
    """score -> estimate (the centre is E15's result word 1) -> resample -> estimate (NULL weights), all queued before
    anything is read"""
    import torch
    dev = torch.device("cuda:0")
    P = M = 2049
    case = pc.layout_case(P)
    w1_want, r15_want, _ = pc.case_want(oracle, case, f"layout{P}")[0]
    poses = case["poses"][0]
    best = int(r15_want[1])
    u = 0x9E3779B9
    a_want = ro.ancestors_search(w1_want, M, u)
    want1 = eo.estimate(poses, w1_want, eo.DEFAULT, best)
    want2 = eo.estimate(poses[a_want], None, eo.DEFAULT, 0)
    # the regime, all from the oracles: the best pose is the centre and not pose 0, the gate holds some poses and
    # not all, the sets differ, and resampling changed the list
    assert best == int(np.argmax(w1_want)) != 0 and want1[1] == best and want1[0] == 0
    assert 2 <= want1[4] < P and want1[8:40].tobytes() != want1[40:72].tobytes()
    assert 2 <= want2[4] < M and want2.tobytes() != want1.tobytes() and len(np.unique(a_want)) < P
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
    d_poses = _up(poses)
    d_w1 = torch.full((P + PAD,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_r15 = torch.full((8 + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_r16 = torch.full((8 + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_u = _up(np.array([u], np.uint32))
    d_out = torch.full((4 * (M + PAD),), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr16 = torch.full((abi.resample_scratch_words(1, P) + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    words = abi.estimate_scratch_words(1, P)
    d_scr = torch.full((words + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((2 * W + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    est = abi.PoseEstimate.defaults()

    gpu.score_poses_dev(d_nodes.data_ptr(), n, d_lens.data_ptr(), B, case["group"], case["p"], 0,
                        d_pose2d.data_ptr(), spec, d_poses.data_ptr(), P, 4 * P, 0, d_field.data_ptr(), fstride, 0,
                        d_w1.data_ptr(), P + PAD, d_r15.data_ptr(), 0)
    gpu.estimate_poses_dev(d_poses.data_ptr(), 4 * P, 0, d_w1.data_ptr(), P + PAD, 1, P, est, d_r15.data_ptr() + 4, 8,
                           d_res.data_ptr(), d_scr.data_ptr())
    gpu.resample_poses_dev(d_w1.data_ptr(), P + PAD, d_poses.data_ptr(), 4 * P, 0, 1, P, M, d_u.data_ptr(), 0, 0, 0,
                           0, d_out.data_ptr(), 4 * (M + PAD), 0, 0, d_r16.data_ptr(), d_scr16.data_ptr())
    gpu.estimate_poses_dev(d_out.data_ptr(), 4 * (M + PAD), 0, 0, 0, 1, M, est, 0, 0, d_res.data_ptr() + 4 * W,
                           d_scr.data_ptr())
    gpu.synchronize()  # nothing was read until here
    w1, res, r15, r16 = _u32(d_w1), _u32(d_res), _u32(d_r15), _u32(d_r16)
    assert (w1[P:] == GUARD_WORD).all() and (res[2 * W:] == GUARD_WORD).all() and (r15[8:] == GUARD_WORD).all()
    assert (r16[8:] == GUARD_WORD).all() and (_u32(d_scr)[words:] == GUARD_WORD).all()
    assert (_u32(d_out)[4 * M:] == GUARD_WORD).all()
    assert w1[:P].tobytes() == w1_want.tobytes() and r15[:8].tobytes() == r15_want.tobytes()
    assert _u32(d_out)[:4 * M].tobytes() == poses[a_want].tobytes()
    _check(res[:2 * W].reshape(2, W), np.stack([want1, want2]))
    # W of set 0 is E15's words 6, 7 and E16's S on a list that is in range
    total = eo.value_of(res[8:12])
    assert total == int(r15[6]) | int(r15[7]) << 32 == int(r16[0]) | int(r16[1]) << 32
    assert d_poses.cpu().numpy().tobytes() == poses.tobytes()


# ---- the door, refusals -----------------------------------------------------------------------------------------------------
def test_host_buffers_one_group(gpu):
    for case, g in ((ec.edge_case(1025), 1), (ec.quant_case(1000.0), 0), (dict(ec.edge_case(65), w=None), 0),
                    (ec.gate_case("centre_word"), 0)):
        poses, w, c = ec.group_inputs(case, g)
        res = gpu.estimate_poses(poses, w, ec.spec_of(case["spec"]), c)
        assert res.tobytes() == ec.want(case)[g].tobytes()
    lib = abi.load_library()
    import ctypes as C
    poses = np.array([[1, 0, 1.0, 0.5], [1, 0, -2.0, 0.5]], F32)
    res = np.full(80, GUARD_WORD, np.uint32)
    good = abi.PoseEstimate.defaults()

    def door(poses_=poses.ctypes.data, P=2, spec=good, res_=res.ctypes.data, h=gpu._h):
        return lib.rplgpu_estimate_poses(h, poses_, P, 0, C.byref(spec) if spec is not None else None, 0, res_)

    bad = abi.ERR_INVALID_ARG
    assert door(poses_=0) == bad and door(res_=0) == bad and door(spec=None) == bad and door(h=None) == bad
    assert door(P=0) == bad and door(P=abi.MAX_POSES + 1) == bad
    assert door(spec=abi.PoseEstimate.defaults(xy_scale=0.0)) == bad
    assert door(spec=abi.PoseEstimate.defaults(xy_scale=float("inf"))) == bad
    assert (res == GUARD_WORD).all()
    assert door() == abi.OK and res[:72].tobytes() == eo.estimate(poses, None, eo.DEFAULT).tobytes()
    assert (res[72:] == GUARD_WORD).all()


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu):
    import torch
    case = ec.groups_case(1, G=3, P=1100)
    b = _buffers(case, cstride=8)
    G, P = b["G"], b["P"]
    host = np.zeros(64, np.uint32)
    hp = host.ctypes.data + (-host.ctypes.data % 16)

    def call(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            _call(gpu, b, **kw)
        return e.value.code

    bad = abi.ERR_INVALID_ARG
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert call(spec=abi.PoseEstimate.defaults(xy_scale=v)) == bad
    assert call(G=0) == bad and call(G=65536) == bad
    assert call(P=0) == bad and call(P=abi.MAX_POSES + 1, wstride=1 << 21, pstride=1 << 23) == bad
    for k in ("poses", "res", "scr"):                                     # required pointers
        assert call(**{k: 0}) == bad, k
    for k, step in (("poses", 4), ("poses", 8), ("w", 2), ("center", 2), ("res", 1), ("res", 2), ("scr", 4),
                    ("scr", 2)):                                          # alignment
        t = b[dict(poses="d_p", w="d_w", center="d_c", res="d_res", scr="d_scr")[k]]
        assert call(**{k: t.data_ptr() + step}) == bad, (k, step)
    assert call(wstride=P - 1) == bad
    assert call(pstride=4 * P - 4) == bad and call(pstride=4 * P + 2) == bad
    assert call(cstride=0) == bad                                         # one word for three groups
    for k in ("poses", "w", "center", "res", "scr"):                      # plain host memory, pointer by pointer
        assert call(**{k: hp}) == bad, k
    import ctypes as C
    assert abi.load_library().rplgpu_estimate_poses_dev(
        None, b["d_p"].data_ptr(), b["pstride"], 1, 0, 0, G, P, C.byref(b["spec"]), 0, 0, b["d_res"].data_ptr(),
        b["d_scr"].data_ptr()) == bad
    assert abi.load_library().rplgpu_estimate_poses_dev(
        gpu._h, b["d_p"].data_ptr(), b["pstride"], 1, 0, 0, G, P, None, 0, 0, b["d_res"].data_ptr(),
        b["d_scr"].data_ptr()) == bad
    gpu.synchronize()
    torch.cuda.synchronize()
    _outputs_untouched(b)
    _inputs_unchanged(b)
    _check(_run(gpu, case, cstride=8), ec.want(case))                     # then a good call on the case
