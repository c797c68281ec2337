"""E15 on the device: rplgpu_score_poses_dev against tests/pose_oracle.py byte for byte — weights, d_result,
d_status, the guard words behind every group's weights, behind the result words and the status words, and the
unchanged field and pose list.  The inputs and their regime checks live in tests/pose_cases.py; every input is one
the rule defines a result for."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, RplGpu, abi
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import pose_cases as pc
from tests import pose_oracle as po

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 0x5A
GUARD_WORD = 0x5A5A5A5A
PAD = 5  # guard words behind every group's weights


def _struct(s):
    return abi.PoseScore(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"])


def _upload(case):
    import torch
    dev = torch.device("cuda:0")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    batch = case["batch"]
    B, n = batch.shape
    return dict(nodes=up(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)),
                lens=up(np.asarray(case["lens"], np.int32)), motion=up(case.get("motion")),
                pose2d=up(case.get("pose2d")), t0=up(case.get("t0")))


def _field_buffer(case):
    """(host (F, stride) uint8 with four guard bytes behind every field, stride)."""
    s = case["spec"]
    cells = s["width"] * s["height"]
    stride = ((cells + 3) & ~3) + 4
    f = np.asarray(case["fields"], np.int8)
    host = np.full((len(f), stride), GUARD, np.uint8)
    host[:, :cells] = f.reshape(len(f), cells).view(np.uint8)
    return host, stride


def _pose_buffer(case):
    """(host (L, stride) float32 with four guard floats behind every list, stride in floats)."""
    q = np.asarray(case["poses"], F32)
    L, P, _ = q.shape
    stride = 4 * P + 4
    host = np.full((L, stride), 123.0, F32)
    host[:, :4 * P] = q.reshape(L, 4 * P)
    return host, stride


def _run(gpu, case, p=None, status=True, d_field=None, field_stride=None, pad=PAD):
    """-> (weights (G, P) uint32, result (G, 8) uint32, status (G,)).  The guard words behind the weights, the
    results and the status words, the field and the pose list are checked here.  status False: NULL goes in for
    d_status.  d_field: a device field to use instead of the case's (the chain test)."""
    import torch
    dev = torch.device("cuda:0")
    s = case["spec"]
    B, n = case["batch"].shape
    G = len(pc.case_groups(case))
    P = case["poses"].shape[1]
    stride = P + pad
    d = _upload(case)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    host_field = None
    if d_field is None:
        host_field, field_stride = _field_buffer(case)
        d_field_t = torch.from_numpy(host_field.reshape(-1)).to(dev)
        d_field = d_field_t.data_ptr()
    host_poses, pose_stride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    d_w = torch.full((G * stride,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((G * 8 + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_st = torch.full((G + 2,), 99, dtype=torch.int32, device=dev)
    gpu.set_scan_time_offsets_dev(ptr(d["t0"]))
    try:
        gpu.score_poses_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, case["group"], p or case["p"],
                            ptr(d["motion"]), ptr(d["pose2d"]), _struct(s), d_poses.data_ptr(), P, pose_stride,
                            1 if len(case["poses"]) > 1 else 0, d_field, field_stride,
                            1 if len(case["fields"]) > 1 else 0, d_w.data_ptr(), stride, d_res.data_ptr(),
                            d_st.data_ptr() if status else 0)
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    if host_field is not None:
        assert d_field_t.cpu().numpy().tobytes() == host_field.tobytes()  # the field is only read
    assert d_poses.cpu().numpy().tobytes() == host_poses.tobytes()        # and so is the pose list
    raw = d_w.cpu().numpy().view(np.uint32).reshape(G, stride)
    res = d_res.cpu().numpy().view(np.uint32)
    st = d_st.cpu().numpy().astype(np.int64)
    assert (raw[:, P:] == GUARD_WORD).all() and (res[8 * G:] == GUARD_WORD).all() and (st[G:] == 99).all()
    if not status:
        assert (st == 99).all()
    return raw[:, :P], res[:8 * G].reshape(G, 8), st[:G]


def _check(got, want, has_status=True):
    weights, res, status = got
    assert len(weights) == len(want)
    for g, (ww, wr, ws) in enumerate(want):
        diff = np.flatnonzero(weights[g] != ww)
        if g < 4 or len(diff):
            print(f"group {g}: result {res[g].tolist()} want {wr.tolist()}, status {status[g]} want {ws}, "
                  f"{len(diff)} of {ww.size} weights differ")
        assert len(diff) == 0, (g, diff[:8], weights[g][diff[:8]], ww[diff[:8]])
        assert res[g].tobytes() == wr.tobytes(), (g, res[g], wr)
        assert not has_status or status[g] == ws, g


# ---- layouts, passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", pc.LAYOUT_P)
def test_layouts(gpu, oracle, P):
    case = pc.layout_case(P)
    pc.layout_regime(oracle, case)
    _check(_run(gpu, case), pc.case_want(oracle, case, f"layout{P}"))


@pytest.mark.parametrize("n", pc.PASS_STRIDES)
@pytest.mark.parametrize("P", pc.PASS_P)
def test_second_pass(gpu, oracle, n, P):
    if n * P > 5 * 10 ** 7:
        raise AssertionError("the case is larger than the suite allows")
    case = pc.pass_case(n, P)
    pc.pass_regime(oracle, case)
    _check(_run(gpu, case), pc.case_want(oracle, case, f"pass{n}_{P}"))


# ---- poses at their limits, the largest list -------------------------------------------------------------------------------
def test_poses_at_their_limits(gpu, oracle):
    case = pc.limit_case()
    by = pc.limit_regime(oracle, case)
    want = pc.case_want(oracle, case, "limits")
    assert want[0][2] == abi.SCAN_CELL_RANGE
    got = _run(gpu, case)
    _check(got, want)
    names = case["names"]
    assert got[0][0][names.index("zero")] == 127 * want[0][1][4] == by["zero"][0]  # the known answer
    # without the far and the non-finite poses no status bit is set
    finite = pc.limit_case([k for k in names if k.startswith("off_") or k in ("identity", "zero", "scale2")])
    wf = pc.case_want(oracle, finite, "limits_finite3")
    assert wf[0][2] == 0
    _check(_run(gpu, finite), wf)
    # and each of them sets it alone
    for k in ("far", "nan_c", "inf_s", "ninf_tx", "nan_ty"):
        one = pc.limit_case(["identity", k])
        w1 = pc.case_want(oracle, one, f"limits_{k}")
        assert w1[0][2] == abi.SCAN_CELL_RANGE and w1[0][0][1] == 0 and w1[0][0][0] > 0
        _check(_run(gpu, one), w1)


def test_known_answer(gpu, oracle):
    case, want = pc.known_case()
    got = _run(gpu, case)
    assert got[0][0].tobytes() == want.tobytes()
    _check(got, pc.case_want(oracle, case, "known"))


def test_largest_list_and_one_more(gpu, oracle):
    import torch
    case = pc.big_case()
    pc.big_regime(oracle, case)
    _check(_run(gpu, case), pc.case_want(oracle, case, "big"))
    # P + 1: refused, nothing written
    dev = torch.device("cuda:0")
    P = pc.BIG_P + 1
    d = _upload(case)
    host_field, fstride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    d_poses = torch.zeros(4 * P, dtype=torch.float32, device=dev)
    d_w = torch.full((P,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((8,), GUARD_WORD, dtype=torch.int32, device=dev)
    with pytest.raises(abi.RplGpuError) as e:
        gpu.score_poses_dev(d["nodes"].data_ptr(), 16, d["lens"].data_ptr(), 1, 1, case["p"], 0,
                            d["pose2d"].data_ptr(), _struct(case["spec"]), d_poses.data_ptr(), P, 4 * P, 0,
                            d_field.data_ptr(), fstride, 0, d_w.data_ptr(), P, d_res.data_ptr(), 0)
    assert e.value.code == abi.ERR_INVALID_ARG
    gpu.synchronize()
    assert (d_w.cpu().numpy().view(np.uint32) == GUARD_WORD).all()
    assert (d_res.cpu().numpy().view(np.uint32) == GUARD_WORD).all()


# ---- groups ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppg,fpg", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_groups(gpu, oracle, ppg, fpg):
    case = pc.groups_case(ppg, fpg)
    want = pc.groups_regime(oracle, case, f"groups{ppg}{fpg}")
    _check(_run(gpu, case, pad=PAD + 59 * ppg), want)  # weight_stride > P, twice


# ---- the front end --------------------------------------------------------------------------------------------------------------
def test_full_front_end(gpu, oracle):
    case = pc.front_case()
    want = pc.front_regime(oracle, case)
    _check(_run(gpu, case), want)
    _check(_run(gpu, case, status=False), want, has_status=False)  # d_status left out
    bare = pc.front_case(with_pose2d=False)                         # d_pose2d left out: identity mounts
    _check(_run(gpu, bare), pc.front_regime(oracle, bare, "front_nopose"))


def test_ieee_divide_instance(gpu, oracle):
    """A handle whose fast divides are refused (as tests/test_gpu_ieee_div.py arranges): the same bytes."""
    import torch

    from tests.conftest import _shared_stream
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    case = pc.front_case()
    want = pc.case_want(oracle, case, "front")
    h = RplGpu(device=0, max_samples_per_scan=32768, max_batch=64)
    try:
        h.set_stream(_shared_stream().cuda_stream)
        assert lib.rplgpu_debug_force_ieee_div(h._h, 7) == abi.OK
        got = _run(h, case)
        torch.cuda.synchronize()
    finally:
        h.close()
    _check(got, want)
    fast = _run(gpu, case)
    assert fast[0].tobytes() == got[0].tobytes() and fast[1].tobytes() == got[1].tobytes()


# ---- the identities, between the real kernels --------------------------------------------------------------------------------
def test_identity_a_with_the_scan_matcher(gpu, oracle):
    """weights[k + K] == score[k][0][0]: E13's kernel and this one on the same points and field, K = 64."""
    import torch
    dev = torch.device("cuda:0")
    pc.identity_a_regime(oracle)
    m, e = pc.identity_a_case()
    got = _run(gpu, e)
    _check(got, pc.case_want(oracle, e, "pose_ida"))
    s = m["spec"]
    B, n = m["batch"].shape
    volume = mo.volume_size(s)
    d = _upload(m)
    host_field, fstride = _field_buffer(m)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    d_scores = torch.full((volume,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_best = torch.full((8,), GUARD_WORD, dtype=torch.int32, device=dev)
    ms = abi.ScanMatch(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["shift_x"],
                       s["shift_y"], s["rot_steps"], s["rot_step"])
    gpu.match_scans_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, 1, m["p"], 0, d["pose2d"].data_ptr(), 0,
                        ms, d_field.data_ptr(), fstride, 0, d_scores.data_ptr(), volume, d_best.data_ptr(), 0)
    gpu.synchronize()
    vol = d_scores.cpu().numpy().view(np.uint32).reshape(mo.volume_shape(s))
    assert abi.scan_match_rotations(ms).tobytes() == e["poses"][0][:, :2].tobytes()
    assert got[0][0].tobytes() == np.ascontiguousarray(vol[:, 1, 1]).tobytes()
    assert got[1][0][4] == d_best.cpu().numpy().view(np.uint32)[4]


def test_identity_b_with_the_map(gpu, oracle):
    """weight of (1, 0, 0, 0) == sum of hits x max(field, 0): E14's kernel on a zeroed map and this one."""
    import torch
    dev = torch.device("cuda:0")
    total = pc.identity_b_regime(oracle)
    o, e = pc.identity_b_case()
    got = _run(gpu, e)
    _check(got, pc.case_want(oracle, e, "pose_idb"))
    B, n = e["batch"].shape
    W, H = o["width"], o["height"]
    d = _upload(e)
    d_counts = torch.zeros(2 * W * H, dtype=torch.int32, device=dev)
    grid = abi.OccGrid(o["origin_x"], o["origin_y"], o["resolution"], W, H, o["range_min"], o["obstacle_max"],
                       o["raytrace_max"])
    gpu.map_update_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, B, e["p"], 0, d["pose2d"].data_ptr(), grid,
                       d_counts.data_ptr())
    gpu.synchronize()
    hits = d_counts.cpu().numpy().view(np.uint32).reshape(H, W, 2)[:, :, 1].astype(np.int64)
    assert int((hits * po.field_values(e["fields"][0])).sum()) == int(got[0][0][0]) == total


# ---- the result words ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.words_cases()))
def test_result_words(gpu, oracle, name):
    case, expect, high = pc.words_cases()[name]
    pc.words_regime(oracle, name, case, expect, high)
    got = _run(gpu, case)
    _check(got, pc.case_want(oracle, case, f"words_{name}"))
    assert tuple(int(v) for v in got[1][0][:4]) == expect and (got[1][0][7] != 0) == high


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def test_chain_on_the_device(gpu, oracle):
    """E14 -> its grid -> E12 with a table -> E15, all queued before anything is read: the map of the room made at
    the true poses, as a likelihood field, weighs 2048 poses of the base and the planted true one wins alone."""
    import torch
    dev = torch.device("cuda:0")
    case = pc.chain_case(oracle)
    pc.chain_regime(oracle, case)
    want = pc.case_want(oracle, case, "chain")
    s = case["spec"]
    B, n = case["batch"].shape
    W, H = s["width"], s["height"]
    P = pc.CHAIN_P
    stride = W * H
    o = mc.room_occ_spec()
    d = _upload(case)
    d_map_pose = torch.from_numpy(case["map_pose2d"]).to(dev)
    d_counts = torch.zeros(2 * stride, dtype=torch.int32, device=dev)
    d_grid = torch.full((stride,), GUARD, dtype=torch.uint8, device=dev)
    d_field = torch.full((stride,), GUARD, dtype=torch.uint8, device=dev)
    d_table = torch.from_numpy(mc.ROOM_TABLE).to(dev)
    d_poses = torch.from_numpy(case["poses"][0].reshape(-1)).to(dev)
    d_w = torch.full((P + PAD,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((16,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_st = torch.full((2,), 99, dtype=torch.int32, device=dev)
    grid = abi.OccGrid(o["origin_x"], o["origin_y"], o["resolution"], W, H, o["range_min"], o["obstacle_max"],
                       o["raytrace_max"])
    rule = abi.MapRule(**pc.CHAIN_RULE)
    gpu.map_update_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, B, case["p"], 0, d_map_pose.data_ptr(),
                       grid, d_counts.data_ptr())
    gpu.map_grid_dev(d_counts.data_ptr(), W, H, rule, 0, d_grid.data_ptr(), stride)
    gpu.inflate_grids_dev(d_grid.data_ptr(), stride, d_field.data_ptr(), stride, 1, W, H, d_table.data_ptr(),
                          mc.ROOM_RC, 1)
    gpu.score_poses_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, B, case["p"], 0, d["pose2d"].data_ptr(),
                        _struct(s), d_poses.data_ptr(), P, 4 * P, 0, d_field.data_ptr(), stride, 0, d_w.data_ptr(),
                        P + PAD, d_res.data_ptr(), d_st.data_ptr())
    gpu.synchronize()  # nothing was read until here
    assert d_field.cpu().numpy().view(np.int8).tobytes() == case["fields"][0].tobytes()
    raw = d_w.cpu().numpy().view(np.uint32)
    res = d_res.cpu().numpy().view(np.uint32)
    assert (raw[P:] == GUARD_WORD).all() and (res[8:] == GUARD_WORD).all()
    _check((raw[None, :P], res[None, :8], d_st.cpu().numpy()[:1].astype(np.int64)), want)
    assert res[1] == pc.CHAIN_AT and res[2] == 1 and d_st.cpu().numpy()[1] == 99


# ---- the door, refusals --------------------------------------------------------------------------------------------------------------
def test_host_buffers_one_group(gpu, oracle):
    case = pc.front_case()
    w, res, status = pc.case_want(oracle, case, "front")[0]
    weights, words, st = gpu.score_poses(case["batch"], case["lens"], case["p"], _struct(case["spec"]),
                                         case["poses"][0], case["fields"][0], motion=case["motion"],
                                         pose2d=case["pose2d"], t0=case["t0"])
    assert weights.tobytes() == w.tobytes() and words.tobytes() == res.tobytes() and st == status
    none, words2, _ = gpu.score_poses(case["batch"], case["lens"], case["p"], _struct(case["spec"]),
                                      case["poses"][0], case["fields"][0], motion=case["motion"],
                                      pose2d=case["pose2d"], t0=case["t0"], want_weights=False)
    assert none is None and words2.tobytes() == words.tobytes()
    lib = abi.load_library()
    out = np.full(8, GUARD_WORD, np.uint32)
    lens = np.ascontiguousarray(case["lens"], np.uint32)
    poses = np.ascontiguousarray(case["poses"][0])
    field = np.ascontiguousarray(case["fields"][0])

    def door(P=65, spec=None, n_scans=3, result=out.ctypes.data):
        sp = _struct(dict(case["spec"], **(spec or {})))
        return lib.rplgpu_score_poses(gpu._h, case["batch"].ctypes.data, 4096, lens.ctypes.data, n_scans,
                                      C.byref(case["p"]), 0, 0, 0, C.byref(sp), poses.ctypes.data, P,
                                      field.ctypes.data, 0, result, 0)

    assert door(P=0) == abi.ERR_INVALID_ARG and door(P=abi.MAX_POSES + 1) == abi.ERR_INVALID_ARG
    assert door(spec=dict(width=0)) == abi.ERR_INVALID_ARG and door(result=0) == abi.ERR_INVALID_ARG
    assert door(n_scans=0) == abi.ERR_INVALID_ARG and door(n_scans=gpu.max_batch + 1) == abi.ERR_CAPACITY
    assert (out == GUARD_WORD).all()
    assert door() == abi.OK and out[4] > 0


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    case = pc.layout_case(65)
    s = case["spec"]
    B, n = case["batch"].shape
    P = 65
    cells = s["width"] * s["height"]
    d = _upload(case)
    host_field, fstride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pstride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    d_w = torch.full((P + PAD,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_t0 = torch.zeros(B, dtype=torch.float32, device=dev)
    d_st = torch.full((2,), 99, dtype=torch.int32, device=dev)
    host = np.zeros(4 * P + 8, np.uint32)
    lib = abi.load_library()

    def call(**kw):
        a = dict(nodes=d["nodes"].data_ptr(), n=n, B=B, group=1, spec=_struct(s), poses=d_poses.data_ptr(), P=P,
                 pstride=pstride, field=d_field.data_ptr(), fstride=fstride, w=d_w.data_ptr(), wstride=P + PAD,
                 res=d_res.data_ptr(), p=case["p"], motion=0, status=0)
        a.update(kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.score_poses_dev(a["nodes"], a["n"], d["lens"].data_ptr(), a["B"], a["group"], a["p"], a["motion"],
                                d["pose2d"].data_ptr(), a["spec"], a["poses"], a["P"], a["pstride"], 0, a["field"],
                                a["fstride"], 0, a["w"], a["wstride"], a["res"], a["status"])
        return e.value.code

    def raw(p_ref, s_ref):
        """The C entry point with a NULL p or s (the binding always passes a struct)."""
        return lib.rplgpu_score_poses_dev(gpu._h, d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, 1, p_ref, 0,
                                          d["pose2d"].data_ptr(), s_ref, d_poses.data_ptr(), P, pstride, 0,
                                          d_field.data_ptr(), fstride, 0, d_w.data_ptr(), P + PAD,
                                          d_res.data_ptr(), 0)

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(resolution=0.0), dict(width=0), dict(height=4097), dict(origin_x=float("nan")),
               dict(resolution=float("inf"))):
        assert call(spec=_struct(dict(s, **kw))) == bad, kw
    assert call(P=0) == bad
    assert call(P=abi.MAX_POSES + 1, pstride=4 * (abi.MAX_POSES + 1), wstride=abi.MAX_POSES + 1) == bad
    assert call(pstride=4 * P - 4) == bad           # below 4 P
    assert call(pstride=4 * P + 2) == bad           # not a multiple of 4
    assert call(poses=d_poses.data_ptr() + 4) == bad    # not 16-byte aligned
    assert call(poses=d_poses.data_ptr() + 8) == bad
    assert call(poses=0) == bad
    assert call(fstride=cells - 4) == bad           # below width * height
    assert call(fstride=fstride + 2) == bad         # not a multiple of 4
    assert call(field=d_field.data_ptr() + 1) == bad
    assert call(field=0) == bad
    assert call(w=0) == bad
    assert call(res=0) == bad
    assert call(w=d_w.data_ptr() + 2) == bad
    assert call(res=d_res.data_ptr() + 1) == bad
    assert call(wstride=P - 1) == bad
    assert call(w=host.ctypes.data) == bad          # plain host memory, pointer by pointer
    assert call(res=host.ctypes.data) == bad
    assert call(field=host.ctypes.data) == bad
    assert call(poses=host.ctypes.data + (-host.ctypes.data % 16)) == bad
    assert call(status=host.ctypes.data) == bad
    assert call(motion=host.ctypes.data) == bad
    assert call(status=d_st.data_ptr() + 2) == bad  # a misaligned d_status
    assert raw(None, C.byref(_struct(s))) == bad and raw(C.byref(case["p"]), None) == bad
    assert call(group=0) == bad
    assert call(nodes=0) == bad
    assert call(n=0) == bad
    assert call(B=gpu.max_batch + 1) == abi.ERR_CAPACITY
    assert call(p=Params.defaults(clip_enable=0, ror_enable=1, ror_radius=0.0)) == bad
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        assert call() == bad  # offsets set, d_motion NULL
    finally:
        gpu.set_scan_time_offsets_dev(0)
    # group x n_stride above 2^24: 513 scans claimed at a stride of 32768 (refused before anything is read)
    assert call(n=32768, B=513, group=513) == bad
    gpu.synchronize()
    assert (d_w.cpu().numpy().view(np.uint32) == GUARD_WORD).all()
    assert (d_res.cpu().numpy().view(np.uint32) == GUARD_WORD).all() and (d_st.cpu().numpy() == 99).all()
    assert d_field.cpu().numpy().tobytes() == host_field.tobytes()
    assert d_poses.cpu().numpy().tobytes() == host_poses.tobytes()
    _check(_run(gpu, case), pc.case_want(oracle, case, "layout65"))  # the handle still works
