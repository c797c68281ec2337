"""E23 on the device: rplgpu_score_poses_agree_dev against tests/agree_oracle.py byte for byte — counts, mask, weights,
d_result, d_agree, d_status, the guard words behind every one of them, and the unchanged field and pose list.  The
inputs and their regime checks live in tests/agree_cases.py; every input is one the rule defines a result for."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, RplGpu, abi
from tests import agree_cases as ac
from tests import estimate_oracle as eo
from tests import pose_cases as pc
from tests import resample_oracle as ro

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 0x5A
GUARD_WORD = 0x5A5A5A5A
PAD = 5  # guard words behind every group's weights, every scan's counts and every scan's mask words


def _struct(s):
    return abi.BeamAgree(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["agree_lo"],
                         s["keep_num"], s["keep_den"], s["err_num"], s["err_den"])


def _pose_struct(s):
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
    s = case["spec"]
    cells = s["width"] * s["height"]
    stride = ((cells + 3) & ~3) + 4
    f = np.asarray(case["fields"], np.int8)
    host = np.full((len(f), stride), GUARD, np.uint8)
    host[:, :cells] = f.reshape(len(f), cells).view(np.uint8)
    return host, stride


def _pose_buffer(case):
    q = np.asarray(case["poses"], F32)
    L, P, _ = q.shape
    stride = 4 * P + 4
    host = np.full((L, stride), 123.0, F32)
    host[:, :4 * P] = q.reshape(L, 4 * P)
    return host, stride


class _Outputs:
    """The call's outputs on the device, every one with guard words behind each row."""

    def __init__(self, B, n, G, P, pad=PAD):
        import torch
        dev = torch.device("cuda:0")
        full = lambda k: torch.full((k,), GUARD_WORD, dtype=torch.int32, device=dev)  # noqa: E731
        self.B, self.n, self.G, self.P = B, n, G, P
        self.words = (n + 31) // 32
        self.wstride, self.cstride, self.mstride = P + pad, n + pad, self.words + pad
        self.w, self.res, self.agree = full(G * self.wstride), full(G * 8 + 8), full(G * 8 + 8)
        self.counts, self.mask = full(B * self.cstride), full(B * self.mstride)
        self.st = torch.full((G + 2,), 99, dtype=torch.int32, device=dev)

    def untouched(self):
        return all((t.cpu().numpy().view(np.uint32) == GUARD_WORD).all()
                   for t in (self.w, self.res, self.agree, self.counts, self.mask)) and \
            (self.st.cpu().numpy() == 99).all()

    def read(self, status=True):
        """-> (counts (B, n), mask (B, words), weights (G, P), result (G, 8), agree (G, 8), status (G,)); the guard
        words are checked here."""
        u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        G, P = self.G, self.P
        w = u(self.w).reshape(G, self.wstride)
        c = u(self.counts).reshape(self.B, self.cstride)
        m = u(self.mask).reshape(self.B, self.mstride)
        res, agr, st = u(self.res), u(self.agree), self.st.cpu().numpy().astype(np.int64)
        assert (w[:, P:] == GUARD_WORD).all() and (c[:, self.n:] == GUARD_WORD).all()
        assert (m[:, self.words:] == GUARD_WORD).all()
        assert (res[8 * G:] == GUARD_WORD).all() and (agr[8 * G:] == GUARD_WORD).all() and (st[G:] == 99).all()
        if not status:
            assert (st == 99).all()
        return c[:, :self.n], m[:, :self.words], w[:, :P], res[:8 * G].reshape(G, 8), agr[:8 * G].reshape(G, 8), st[:G]


def _run(gpu, case, p=None, status=True, pad=PAD, spec=None, batch=None):
    import torch
    dev = torch.device("cuda:0")
    if batch is not None:
        case = dict(case, batch=batch)
    s = spec or case["spec"]
    B, n = case["batch"].shape
    G = len(pc.case_groups(case))
    P = case["poses"].shape[1]
    d = _upload(case)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    host_field, field_stride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pose_stride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    out = _Outputs(B, n, G, P, pad)
    gpu.set_scan_time_offsets_dev(ptr(d["t0"]))
    try:
        gpu.score_poses_agree_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, case["group"], p or case["p"],
                                  ptr(d["motion"]), ptr(d["pose2d"]), _struct(s), d_poses.data_ptr(), P, pose_stride,
                                  1 if len(case["poses"]) > 1 else 0, d_field.data_ptr(), field_stride,
                                  1 if len(case["fields"]) > 1 else 0, out.w.data_ptr(), out.wstride,
                                  out.res.data_ptr(), out.st.data_ptr() if status else 0, out.counts.data_ptr(),
                                  out.cstride, out.mask.data_ptr(), out.mstride, out.agree.data_ptr())
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    assert d_field.cpu().numpy().tobytes() == host_field.tobytes()  # the field is only read
    assert d_poses.cpu().numpy().tobytes() == host_poses.tobytes()  # and so is the pose list
    return out.read(status)


def _run_e15(gpu, case, batch=None):
    """rplgpu_score_poses_dev itself on the same inputs -> (weights (G, P), result (G, 8))."""
    import torch
    dev = torch.device("cuda:0")
    if batch is not None:
        case = dict(case, batch=batch)
    B, n = case["batch"].shape
    G = len(pc.case_groups(case))
    P = case["poses"].shape[1]
    d = _upload(case)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    host_field, field_stride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pose_stride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    d_w = torch.zeros(G * P, dtype=torch.int32, device=dev)
    d_res = torch.zeros(G * 8, dtype=torch.int32, device=dev)
    gpu.set_scan_time_offsets_dev(ptr(d["t0"]))
    try:
        gpu.score_poses_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, case["group"], case["p"],
                            ptr(d["motion"]), ptr(d["pose2d"]), _pose_struct(case["spec"]), d_poses.data_ptr(), P,
                            pose_stride, 1 if len(case["poses"]) > 1 else 0, d_field.data_ptr(), field_stride,
                            1 if len(case["fields"]) > 1 else 0, d_w.data_ptr(), P, d_res.data_ptr(), 0)
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    return d_w.cpu().numpy().view(np.uint32).reshape(G, P), d_res.cpu().numpy().view(np.uint32).reshape(G, 8)


def _check(got, want, case, has_status=True):
    counts, mask, weights, res, agr, status = got
    assert len(weights) == len(want)
    for g, sl in enumerate(pc.case_groups(case)):
        wc, wm, ww, wr, wa, ws = want[g]
        print(f"group {g}: agree {agr[g].tolist()} want {wa.tolist()}, result {res[g].tolist()} want {wr.tolist()}, "
              f"status {status[g]} want {ws}") if g < 4 else None
        diff = np.argwhere(counts[sl] != wc)
        assert len(diff) == 0, (g, "counts", diff[:8], counts[sl][tuple(diff[:8].T)], wc[tuple(diff[:8].T)])
        diff = np.argwhere(mask[sl] != wm)
        assert len(diff) == 0, (g, "mask", diff[:8], mask[sl][tuple(diff[:8].T)], wm[tuple(diff[:8].T)])
        assert agr[g].tobytes() == wa.tobytes(), (g, agr[g], wa)
        diff = np.flatnonzero(weights[g] != ww)
        assert len(diff) == 0, (g, "weights", diff[:8], weights[g][diff[:8]], ww[diff[:8]])
        assert res[g].tobytes() == wr.tobytes(), (g, res[g], wr)
        assert not has_status or status[g] == ws, g


# ---- the pose list's layouts, sample counts, a second pass -------------------------------------------------------------------
@pytest.mark.parametrize("P", ac.LAYOUT_P)
def test_layouts(gpu, oracle, P):
    case = ac.layout_case(P)
    ac.layout_regime(oracle, case)
    _check(_run(gpu, case), ac.case_want(oracle, case, f"layout{P}"), case)


@pytest.mark.parametrize("n", ac.SAMPLE_N)
def test_sample_counts(gpu, oracle, n):
    case = ac.samples_case(n)
    ac.samples_regime(oracle, case, f"n{n}")
    _check(_run(gpu, case), ac.case_want(oracle, case, f"n{n}"), case)


def test_second_pass(gpu, oracle):
    case = ac.samples_case(ac.PASS_STRIDE, n_stride=ac.PASS_STRIDE)
    ac.pass_regime(oracle, case)
    _check(_run(gpu, case), ac.case_want(oracle, case, "pass"), case)


# ---- the named cases ----------------------------------------------------------------------------------------------------------
def test_person(gpu, oracle):
    case = ac.person_case(oracle)
    ac.person_regime(oracle, case)
    _check(_run(gpu, case), ac.case_want(oracle, case, "person"), case)


def test_lost(gpu, oracle):
    case = ac.lost_case(oracle)
    ac.lost_regime(oracle, case)
    _check(_run(gpu, case), ac.case_want(oracle, case, "lost"), case)


def test_edge(gpu, oracle):
    case = ac.edge_case()
    _check(_run(gpu, case), ac.edge_regime(oracle, case), case)


def test_all_from_skipped(gpu, oracle):
    case = ac.all_from_skipped_case()
    ac.all_from_skipped_regime(oracle, case)
    _check(_run(gpu, case), ac.case_want(oracle, case, "all_from_skipped"), case)


def test_limits(gpu, oracle):
    case = ac.limits_case()
    ac.limits_regime(oracle, case)
    want = ac.case_want(oracle, case, "limits")
    assert want[0][5] == abi.SCAN_CELL_RANGE
    _check(_run(gpu, case), want, case)


# ---- groups, the front end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppg,fpg", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_groups(gpu, oracle, ppg, fpg):
    case = ac.groups_case(ppg, fpg)
    want = ac.groups_regime(oracle, case, f"groups{ppg}{fpg}")
    _check(_run(gpu, case, pad=PAD + 59 * ppg), want, case)


def test_full_front_end(gpu, oracle):
    case = ac.front_case()
    want = ac.front_regime(oracle, case)
    _check(_run(gpu, case), want, case)
    _check(_run(gpu, case, status=False), want, case, has_status=False)  # d_status left out


def test_ieee_divide_instance(gpu, oracle):
    """A handle whose fast divides are refused (as tests/test_gpu_ieee_div.py arranges): the same bytes."""
    import torch

    from tests.conftest import _shared_stream
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    case = ac.front_case()
    want = ac.case_want(oracle, case, "front")
    h = RplGpu(device=0, max_samples_per_scan=32768, max_batch=64)
    try:
        h.set_stream(_shared_stream().cuda_stream)
        assert lib.rplgpu_debug_force_ieee_div(h._h, 7) == abi.OK
        got = _run(h, case)
        torch.cuda.synchronize()
    finally:
        h.close()
    _check(got, want, case)


# ---- the identities, against rplgpu_score_poses_dev itself ------------------------------------------------------------------------
def test_identity_1_stage_off(gpu, oracle):
    """err_num = 0: weights and d_result are E15's, byte for byte; the mask is still the rule's."""
    case = ac.person_case(oracle)
    off = dict(case["spec"], err_num=0)
    got = _run(gpu, case, spec=off)
    w15, r15 = _run_e15(gpu, case)
    assert got[2].tobytes() == w15.tobytes() and got[3].tobytes() == r15.tobytes() and got[4][0][2] == 1
    assert got[1].tobytes() == np.concatenate([w[1] for w in ac.case_want(oracle, case, "person")]).tobytes()


def test_identity_2_counts_sum(gpu, oracle):
    case = ac.identity2_case()
    got = _run(gpu, case)
    w15, r15 = _run_e15(gpu, case)
    assert got[4][0][6:].tobytes() == r15[0][6:].tobytes() and r15[0][6] > 0
    _check(got, ac.case_want(oracle, case, "identity2"), case)


def test_identity_4_skipped_samples_dropped(gpu, oracle):
    """E5 off, no fallback: the weights are E15's on the batch whose skipped samples are nodes E1 drops."""
    for case, key in ((ac.person_case(oracle), "person"), (ac.layout_case(1025), "layout1025")):
        want = ac.case_want(oracle, case, key)
        assert case["p"].ror_enable == 0 and all(w[4][2] == 0 for w in want)
        batch, dropped = ac.replaced_batch(case, want)
        assert dropped > 0
        got = _run(gpu, case)
        w15, r15 = _run_e15(gpu, case, batch=batch)
        assert got[2].tobytes() == w15.tobytes()
        assert np.delete(got[3], 4, axis=1).tobytes() == np.delete(r15, 4, axis=1).tobytes()  # word 4: finite points
        assert (got[3][:, 4] == r15[:, 4] + dropped).all() or len(want) > 1


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def test_chain_on_the_device(gpu, oracle):
    """score_poses_agree -> resample -> score_poses_agree -> estimate on one stream, nothing read in between, against
    the oracles' chain."""
    import torch
    dev = torch.device("cuda:0")
    case = ac.person_case(oracle)
    s = case["spec"]
    B, n = case["batch"].shape
    P = case["poses"].shape[1]
    want1 = ac.case_want(oracle, case, "person")[0]
    u = 0x9E3779B9
    poses2, _, _ = ro.resample(want1[2], case["poses"][0], P, u, None)
    case2 = dict(case, poses=np.asarray(poses2, F32)[None])
    want2 = ac.case_want(oracle, case2, "person_chain2")[0]
    es = dict(eo.DEFAULT)
    want_est = eo.estimate(case2["poses"][0], want2[2], es, int(want2[3][1]))
    d = _upload(case)
    host_field, fstride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    d_p1 = torch.from_numpy(np.ascontiguousarray(case["poses"][0]).reshape(-1)).to(dev)
    d_p2 = torch.zeros(4 * P, dtype=torch.float32, device=dev)
    d_u = torch.from_numpy(np.array([u], np.uint32).view(np.int32)).to(dev)
    o1, o2 = _Outputs(B, n, 1, P), _Outputs(B, n, 1, P)
    d_rs = torch.zeros(8, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(int(abi.resample_scratch_words(1, P)) + 2, dtype=torch.int32, device=dev)
    d_est = torch.zeros(abi.ESTIMATE_WORDS, dtype=torch.int32, device=dev)
    d_escr = torch.zeros(int(abi.estimate_scratch_words(1, P)) + 2, dtype=torch.int32, device=dev)

    def score(d_poses, o):
        gpu.score_poses_agree_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, case["group"], case["p"], 0,
                                  d["pose2d"].data_ptr(), _struct(s), d_poses.data_ptr(), P, 4 * P, 0,
                                  d_field.data_ptr(), fstride, 0, o.w.data_ptr(), o.wstride, o.res.data_ptr(),
                                  o.st.data_ptr(), o.counts.data_ptr(), o.cstride, o.mask.data_ptr(), o.mstride,
                                  o.agree.data_ptr())

    score(d_p1, o1)
    gpu.resample_poses_dev(o1.w.data_ptr(), o1.wstride, d_p1.data_ptr(), 4 * P, 0, 1, P, P, d_u.data_ptr(), 0, 1, 0, 0,
                           d_p2.data_ptr(), 4 * P, 0, 0, d_rs.data_ptr(), d_scr.data_ptr())
    score(d_p2, o2)
    gpu.estimate_poses_dev(d_p2.data_ptr(), 4 * P, 0, o2.w.data_ptr(), o2.wstride, 1, P,
                           abi.PoseEstimate(es["xy_scale"], es["gate_r2"], es["gate_dot"]), o2.res.data_ptr() + 4, 8,
                           d_est.data_ptr(), d_escr.data_ptr())
    gpu.synchronize()  # nothing was read until here
    _check(o1.read(), [want1], case)
    assert d_p2.cpu().numpy().tobytes() == case2["poses"][0].tobytes()
    _check(o2.read(), [want2], case2)
    assert d_est.cpu().numpy().view(np.uint32).tobytes() == np.asarray(want_est, np.uint32).tobytes()


# ---- the door, refusals ------------------------------------------------------------------------------------------------------------
def test_host_buffers_one_group(gpu, oracle):
    case = ac.front_case()
    dev_got = _run(gpu, case)
    w, res, st, counts, mask, agree = gpu.score_poses_agree(
        case["batch"], case["lens"], case["p"], _struct(case["spec"]), case["poses"][0], case["fields"][0],
        motion=case["motion"], pose2d=case["pose2d"], t0=case["t0"])
    assert counts.tobytes() == dev_got[0].tobytes() and mask.tobytes() == dev_got[1].tobytes()
    assert w.tobytes() == dev_got[2][0].tobytes() and res.tobytes() == dev_got[3][0].tobytes()
    assert agree.tobytes() == dev_got[4][0].tobytes() and st == dev_got[5][0]
    lib = abi.load_library()
    out = np.full(16, GUARD_WORD, np.uint32)
    lens = np.ascontiguousarray(case["lens"], np.uint32)
    poses = np.ascontiguousarray(case["poses"][0])
    field = np.ascontiguousarray(case["fields"][0])

    def door(P=65, spec=None, n_scans=3, result=out.ctypes.data, agree_at=out.ctypes.data + 32):
        sp = _struct(dict(case["spec"], **(spec or {})))
        return lib.rplgpu_score_poses_agree(gpu._h, case["batch"].ctypes.data, 4096, lens.ctypes.data, n_scans,
                                            C.byref(case["p"]), 0, 0, 0, C.byref(sp), poses.ctypes.data, P,
                                            field.ctypes.data, 0, result, 0, 0, 0, agree_at)

    bad = abi.ERR_INVALID_ARG
    assert door(P=0) == bad and door(P=abi.MAX_POSES + 1) == bad and door(spec=dict(width=0)) == bad
    assert door(spec=dict(agree_lo=0)) == bad and door(spec=dict(keep_den=0)) == bad and door(result=0) == bad
    assert door(agree_at=0) == bad and door(n_scans=0) == bad and door(n_scans=gpu.max_batch + 1) == abi.ERR_CAPACITY
    assert (out == GUARD_WORD).all()
    assert door() == abi.OK and out[4] > 0 and out[8] == out[4]  # F twice: result word 4 and agree word 0


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    case = ac.layout_case(65)
    s = case["spec"]
    B, n = case["batch"].shape
    P = 65
    cells = s["width"] * s["height"]
    d = _upload(case)
    host_field, fstride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pstride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    o = _Outputs(B, n, 1, P)
    d_t0 = torch.zeros(B, dtype=torch.float32, device=dev)
    host = np.zeros(4 * P + 8, np.uint32)
    lib = abi.load_library()

    def call(**kw):
        a = dict(nodes=d["nodes"].data_ptr(), n=n, B=B, group=1, spec=_struct(s), poses=d_poses.data_ptr(), P=P,
                 pstride=pstride, field=d_field.data_ptr(), fstride=fstride, w=o.w.data_ptr(), wstride=o.wstride,
                 res=o.res.data_ptr(), p=case["p"], motion=0, status=0, counts=o.counts.data_ptr(),
                 cstride=o.cstride, mask=o.mask.data_ptr(), mstride=o.mstride, agree=o.agree.data_ptr())
        a.update(kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.score_poses_agree_dev(a["nodes"], a["n"], d["lens"].data_ptr(), a["B"], a["group"], a["p"],
                                      a["motion"], d["pose2d"].data_ptr(), a["spec"], a["poses"], a["P"],
                                      a["pstride"], 0, a["field"], a["fstride"], 0, a["w"], a["wstride"], a["res"],
                                      a["status"], a["counts"], a["cstride"], a["mask"], a["mstride"], a["agree"])
        return e.value.code

    def raw(p_ref, s_ref):
        """The C entry point with a NULL p or s (the binding always passes a struct)."""
        return lib.rplgpu_score_poses_agree_dev(
            gpu._h, d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, 1, p_ref, 0, d["pose2d"].data_ptr(), s_ref,
            d_poses.data_ptr(), P, pstride, 0, d_field.data_ptr(), fstride, 0, o.w.data_ptr(), o.wstride,
            o.res.data_ptr(), 0, o.counts.data_ptr(), o.cstride, o.mask.data_ptr(), o.mstride, o.agree.data_ptr())

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(resolution=0.0), dict(width=0), dict(height=4097), dict(origin_x=float("nan")), dict(agree_lo=0),
               dict(agree_lo=128), dict(keep_den=0), dict(keep_num=11, keep_den=10), dict(err_den=0),
               dict(err_num=(1 << 20) + 1), dict(keep_den=(1 << 20) + 1)):
        assert call(spec=_struct(dict(s, **kw))) == bad, kw
    assert call(P=0) == bad
    assert call(P=abi.MAX_POSES + 1, pstride=4 * (abi.MAX_POSES + 1), wstride=abi.MAX_POSES + 1) == bad
    assert call(pstride=4 * P - 4) == bad and call(pstride=4 * P + 2) == bad
    assert call(poses=d_poses.data_ptr() + 4) == bad and call(poses=0) == bad
    assert call(fstride=cells - 4) == bad and call(fstride=fstride + 2) == bad
    assert call(field=d_field.data_ptr() + 1) == bad and call(field=0) == bad
    assert call(w=0) == bad and call(res=0) == bad and call(w=o.w.data_ptr() + 2) == bad
    assert call(res=o.res.data_ptr() + 1) == bad and call(wstride=P - 1) == bad
    # the new outputs: required, aligned, device memory, strides that hold a scan
    assert call(counts=0) == bad and call(mask=0) == bad and call(agree=0) == bad
    assert call(counts=o.counts.data_ptr() + 2) == bad and call(mask=o.mask.data_ptr() + 1) == bad
    assert call(agree=o.agree.data_ptr() + 3) == bad
    assert call(cstride=n - 1) == bad and call(mstride=(n + 31) // 32 - 1) == bad
    assert call(counts=host.ctypes.data) == bad and call(mask=host.ctypes.data) == bad
    assert call(agree=host.ctypes.data) == bad
    assert call(w=host.ctypes.data) == bad and call(status=host.ctypes.data) == bad
    assert call(motion=host.ctypes.data) == bad and call(status=o.st.data_ptr() + 2) == bad
    assert raw(None, C.byref(_struct(s))) == bad and raw(C.byref(case["p"]), None) == bad
    assert call(group=0) == bad and call(nodes=0) == bad and call(n=0) == bad
    assert call(B=gpu.max_batch + 1) == abi.ERR_CAPACITY
    assert call(p=Params.defaults(clip_enable=0, ror_enable=1, ror_radius=0.0)) == bad
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        assert call() == bad  # offsets set, d_motion NULL
    finally:
        gpu.set_scan_time_offsets_dev(0)
    # group x n_stride above 2^24: 513 scans claimed at a stride of 32768 (refused before anything is read)
    assert call(n=32768, B=513, group=513, cstride=32768, mstride=1024) == bad
    gpu.synchronize()
    assert o.untouched()
    assert d_field.cpu().numpy().tobytes() == host_field.tobytes()
    assert d_poses.cpu().numpy().tobytes() == host_poses.tobytes()
    _check(_run(gpu, case), ac.case_want(oracle, case, "layout65"), case)  # the handle still works
