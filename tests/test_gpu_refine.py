"""E25 on the device: rplgpu_refine_sums_dev, rplgpu_refine_step_dev, rplgpu_refine_poses_dev and the two joints
against tests/refine_oracle.py byte for byte — sums, stepped poses, step words, d_result, d_status, the guard words
behind every output and behind the declared scratch, and the unchanged field and input poses.  The inputs and their
regime checks live in tests/refine_cases.py; the grid is 64 x 64 unless a case says otherwise."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi
from tests import map_oracle as mp
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import refine_cases as rc
from tests import refine_oracle as ro

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 0x5A
GUARD_WORD = 0x5A5A5A5A
PAD = 4  # guard words behind every group's part of an output (the strides stay multiples of 4)


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


class _Buffers:
    """The outputs of a call, every one filled with guard words and a guard behind every group's part."""

    def __init__(self, G, P):
        import torch
        dev = torch.device("cuda:0")
        full = lambda n: torch.full((n,), GUARD_WORD, dtype=torch.int32, device=dev)  # noqa: E731
        self.G, self.P = G, P
        self.sums_stride, self.out_stride, self.step_stride = 32 * P + PAD, 4 * P + PAD, 4 * P + PAD
        self.scratch_words = abi.refine_scratch_words(G, P)
        self.sums, self.out, self.step = full(G * self.sums_stride), full(G * self.out_stride), full(G * self.step_stride)
        self.scratch, self.res, self.st = full(self.scratch_words + 16), full(8 * G + 8), full(G + 2)

    def read(self, status=True, stepped=True):
        """-> (out (G, P, 4) f32, sums (G, P, 32), step (G, P, 4), res (G, 8), st (G,)); the guards are checked."""
        G, P = self.G, self.P
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        sums, out, step = (u32(t).reshape(G, -1) for t in (self.sums, self.out, self.step))
        res, st, scr = u32(self.res), u32(self.st), u32(self.scratch)
        assert (sums[:, 32 * P:] == GUARD_WORD).all() and (res[8 * G:] == GUARD_WORD).all()
        assert (scr[self.scratch_words:] == GUARD_WORD).all()
        assert (st[G:] == GUARD_WORD).all() and (status or (st == GUARD_WORD).all())
        assert (out[:, 4 * P:] == GUARD_WORD).all() and (step[:, 4 * P:] == GUARD_WORD).all()
        if not stepped:
            assert (out == GUARD_WORD).all() and (step == GUARD_WORD).all()
        return (out[:, :4 * P].reshape(G, P, 4).view(F32), sums[:, :32 * P].reshape(G, P, 32),
                step[:, :4 * P].reshape(G, P, 4), res[:8 * G].reshape(G, 8), st[:G])

    def untouched(self):
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        return all((u32(t) == GUARD_WORD).all() for t in (self.sums, self.out, self.step, self.scratch, self.res, self.st))


def _run(gpu, case, mode="poses", iters=1, p=None, status=True):
    """mode: 'sums' (rplgpu_refine_sums_dev), 'poses' (rplgpu_refine_poses_dev with iters), 'apart' (the sums, then
    rplgpu_refine_step_dev).  -> what _Buffers.read returns; the field and the input poses are checked unchanged."""
    import torch
    dev = torch.device("cuda:0")
    B, n = case["batch"].shape
    G = len(rc.case_groups(case))
    P = case["poses"].shape[1]
    d = _upload(case)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    host_field, field_stride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pose_stride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    b = _Buffers(G, P)
    spec = ro.struct_of(case["spec"])
    ppg, fpg = (1 if len(case["poses"]) > 1 else 0), (1 if len(case["fields"]) > 1 else 0)
    front = (d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, case["group"], p or case["p"], ptr(d["motion"]),
             ptr(d["pose2d"]), spec, d_poses.data_ptr(), P, pose_stride, ppg, d_field.data_ptr(), field_stride, fpg)
    st = b.st.data_ptr() if status else 0
    gpu.set_scan_time_offsets_dev(ptr(d["t0"]))
    try:
        if mode == "poses":
            gpu.refine_poses_dev(*front, iters, b.out.data_ptr(), b.out_stride, b.sums.data_ptr(), b.sums_stride,
                                 b.step.data_ptr(), b.step_stride, b.scratch.data_ptr(), b.res.data_ptr(), st)
        else:
            gpu.refine_sums_dev(*front, b.sums.data_ptr(), b.sums_stride, b.scratch.data_ptr(), b.res.data_ptr(), st)
            if mode == "apart":
                gpu.refine_step_dev(b.sums.data_ptr(), b.sums_stride, spec, d_poses.data_ptr(), pose_stride, ppg, G, P,
                                    b.out.data_ptr(), b.out_stride, b.step.data_ptr(), b.step_stride, b.res.data_ptr())
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    assert d_field.cpu().numpy().tobytes() == host_field.tobytes()  # the field is only read
    assert d_poses.cpu().numpy().tobytes() == host_poses.tobytes()  # and so is the pose list
    return b.read(status, mode != "sums")


def _check(got, want, stepped=True, has_status=True):
    out, sums, step, res, status = got
    assert len(sums) == len(want)
    for g, (wo, ws, wstep, wr, wst) in enumerate(want):
        bad = np.flatnonzero((sums[g] != ws).any(1))
        print(f"group {g}: result {res[g].tolist()} want {wr.tolist()}, status {status[g]} want {wst}, "
              f"{len(bad)} of {len(ws)} poses' sums differ")
        assert len(bad) == 0, (g, bad[:4], sums[g][bad[:2]], ws[bad[:2]])
        if stepped:
            assert out[g].tobytes() == wo.tobytes(), (g, out[g][:4], wo[:4])
            assert step[g].tobytes() == wstep.tobytes(), (g, step[g][:4], wstep[:4])
            assert res[g].tobytes() == wr.tobytes(), (g, res[g], wr)
        else:
            assert res[g][4:].tobytes() == wr[4:].tobytes() and not res[g][:4].any(), (g, res[g], wr)
        assert not has_status or status[g] == wst, g


# ---- scan lengths, layouts, groups ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.LENGTHS)
def test_scan_lengths(gpu, oracle, n):
    case = rc.length_case(n)
    _check(_run(gpu, case), rc.length_regime(oracle, case))


@pytest.mark.parametrize("P", rc.LAYOUT_P)
def test_layouts(gpu, oracle, P):
    case = rc.layout_case(P)
    _check(_run(gpu, case), rc.layout_regime(oracle, case))


@pytest.mark.parametrize("ppg,fpg", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_groups(gpu, oracle, ppg, fpg):
    case = rc.groups_case(ppg, fpg)
    _check(_run(gpu, case), rc.groups_regime(oracle, case, f"groups{ppg}{fpg}"))


# ---- the third limb, the borders, the limits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "mirror", "many", "deep"])
def test_third_limb(gpu, oracle, kind):
    case = rc.limb_case(oracle, kind)
    _check(_run(gpu, case, "sums"), rc.limb_regime(oracle, kind, case), stepped=False)


def test_borders(gpu, oracle):
    case = rc.border_case()
    _check(_run(gpu, case, "sums"), rc.border_regime(oracle, case), stepped=False)


def test_poses_at_their_limits(gpu, oracle):
    case = rc.limit_case()
    want = rc.limit_regime(oracle, case)
    got = _run(gpu, case)
    _check(got, want)
    assert got[0][0][1:].tobytes() == case["poses"][0][1:].tobytes()  # not stepped: bit for bit, NaN payloads too
    only = dict(case, poses=case["poses"][:, :1])
    _check(_run(gpu, only), rc.case_want(oracle, only, "limit_identity", iters=1))
    assert rc.case_want(oracle, only, "limit_identity", iters=1)[0][4] == 0  # without them no status bit


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def test_full_front_end(gpu, oracle):
    case = rc.front_case()
    want, off, p_off = rc.front_regime(oracle, case)
    _check(_run(gpu, case), want)
    _check(_run(gpu, case, p=p_off), off)
    _check(_run(gpu, case, status=False), want, has_status=False)


# ---- rounds ---------------------------------------------------------------------------------------------------------------------------
def test_one_round_is_sums_then_step(gpu, oracle):
    case = rc.groups_case(1, 1)
    want = rc.groups_regime(oracle, case, "groups11")
    a, b = _run(gpu, case, "poses", 1), _run(gpu, case, "apart")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    _check(b, want)


@pytest.mark.parametrize("name", ["groups", "length"])
def test_four_rounds(gpu, oracle, name):
    case = rc.groups_case(0, 1) if name == "groups" else rc.length_case(2049)
    want = rc.case_want(oracle, case, f"four_{name}", iters=4)
    one = rc.case_want(oracle, case, f"one_{name}", iters=1)
    assert want[0][0].tobytes() != one[0][0].tobytes() and want[0][1].tobytes() != one[0][1].tobytes()
    _check(_run(gpu, case, "poses", 4), want)


def test_in_place(gpu, oracle):
    """d_poses_out == d_poses with every group its own list: the rounds step the list where it lies."""
    import torch
    dev = torch.device("cuda:0")
    case = rc.groups_case(1, 0)
    want = rc.case_want(oracle, case, "in_place", iters=3)
    B, n = case["batch"].shape
    G, P = 2, rc.GROUPS_P
    d = _upload(case)
    host_field, field_stride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pose_stride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    b = _Buffers(G, P)
    gpu.refine_poses_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, case["group"], case["p"], 0,
                         d["pose2d"].data_ptr(), ro.struct_of(case["spec"]), d_poses.data_ptr(), P, pose_stride, 1,
                         d_field.data_ptr(), field_stride, 0, 3, d_poses.data_ptr(), pose_stride,
                         b.sums.data_ptr(), b.sums_stride, b.step.data_ptr(), b.step_stride, b.scratch.data_ptr(),
                         b.res.data_ptr(), b.st.data_ptr())
    gpu.synchronize()
    got = d_poses.cpu().numpy().reshape(G, pose_stride)
    assert (got[:, 4 * P:] == 123.0).all()
    for g in range(G):
        assert got[g, :4 * P].tobytes() == want[g][0].tobytes(), g
    sums = b.sums.cpu().numpy().view(np.uint32).reshape(G, -1)[:, :32 * P]
    assert all(sums[g].tobytes() == want[g][1].tobytes() for g in range(G))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    case = rc.groups_case(1, 1)
    B, n = case["batch"].shape
    G, P = 2, rc.GROUPS_P
    d = _upload(case)
    host_field, fstride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pstride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    b = _Buffers(G, P)
    good = dict(nodes=d["nodes"].data_ptr(), n=n, lens=d["lens"].data_ptr(), B=B, group=2, p=case["p"], motion=0,
                pose2d=d["pose2d"].data_ptr(), spec=ro.struct_of(case["spec"]), poses=d_poses.data_ptr(), P=P,
                pstride=pstride, ppg=1, field=d_field.data_ptr(), fstride=fstride, fpg=1, iters=2,
                out=b.out.data_ptr(), ostride=b.out_stride, sums=b.sums.data_ptr(), sstride=b.sums_stride,
                step=b.step.data_ptr(), tstride=b.step_stride, scratch=b.scratch.data_ptr(), res=b.res.data_ptr(),
                st=b.st.data_ptr())
    bad = [dict(P=0), dict(P=abi.MAX_POSES + 1), dict(group=0), dict(poses=0), dict(field=0), dict(sums=0),
           dict(scratch=0), dict(res=0), dict(out=0), dict(poses=good["poses"] + 4), dict(pstride=4 * P - 4),
           dict(pstride=4 * P + 2), dict(fstride=64 * 64 - 4), dict(fstride=64 * 64 + 2), dict(field=good["field"] + 1),
           dict(sstride=32 * P - 4), dict(sstride=32 * P + 2), dict(sums=good["sums"] + 4),
           dict(scratch=good["scratch"] + 4), dict(res=good["res"] + 2), dict(st=good["st"] + 1),
           dict(ostride=4 * P - 4), dict(out=good["out"] + 4), dict(tstride=4 * P - 4), dict(step=good["step"] + 4),
           dict(iters=0), dict(iters=abi.REFINE_MAX_ITERS + 1), dict(spec=ro.struct_of(ro.spec(target=0, **rc.GRID))),
           dict(spec=ro.struct_of(ro.spec(min_points=2, **rc.GRID))), dict(out=good["poses"] + 16, ostride=pstride),
           dict(out=good["poses"], ostride=pstride + 4), dict(out=good["poses"], ostride=pstride, ppg=0)]
    order = ("nodes", "n", "lens", "B", "group", "p", "motion", "pose2d", "spec", "poses", "P", "pstride", "ppg", "field",
             "fstride", "fpg", "iters", "out", "ostride", "sums", "sstride", "step", "tstride", "scratch", "res", "st")
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.refine_poses_dev(*[a[k] for k in order])
        assert e.value.code == abi.ERR_INVALID_ARG, kw
    sums_order = order[:16] + ("sums", "sstride", "scratch", "res", "st")
    for kw in (dict(P=0), dict(scratch=0), dict(sums=good["sums"] + 8), dict(sstride=32 * P - 4)):
        a = dict(good, **kw)
        with pytest.raises(abi.RplGpuError):
            gpu.refine_sums_dev(*[a[k] for k in sums_order])
    step_order = ("sums", "sstride", "spec", "poses", "pstride", "ppg", "G", "P", "out", "ostride", "step", "tstride", "res")
    for kw in (dict(G=0), dict(G=65536), dict(P=0), dict(out=0), dict(sums=0), dict(res=0), dict(ostride=4 * P - 4),
               dict(out=good["poses"] + 16, ostride=pstride)):
        a = dict(good, G=G)
        a.update(kw)
        with pytest.raises(abi.RplGpuError):
            gpu.refine_step_dev(*[a[k] for k in step_order])
    with pytest.raises(abi.RplGpuError):  # the joints
        gpu.match_poses_dev(b.res.data_ptr(), abi.ScanMatch(-1.6, -1.6, 0.05, 64, 64, 1, 1, 1, 0.01), 0, 0, 0,
                            b.out.data_ptr(), 4)
    with pytest.raises(abi.RplGpuError):
        gpu.match_poses_dev(b.res.data_ptr(), abi.ScanMatch(-1.6, -1.6, 0.05, 64, 64, 1, 1, 1, 0.01), 0, 0, 1,
                            b.out.data_ptr(), 2)
    with pytest.raises(abi.RplGpuError):
        gpu.compose_poses_dev(d_poses.data_ptr(), pstride, 1, 0, 0, 0, 0, B, 2, b.out.data_ptr())
    with pytest.raises(abi.RplGpuError):
        gpu.compose_poses_dev(d_poses.data_ptr(), pstride, 1, P, 0, 0, 0, B, 0, b.out.data_ptr())
    gpu.synchronize()
    assert b.untouched()
    assert d_poses.cpu().numpy().tobytes() == host_poses.tobytes()


# ---- the identity with E15 ----------------------------------------------------------------------------------------------------------------
def test_cell_centres_give_e15_weights(gpu, oracle):
    """Independent kernels held to each other: every point on a cell centre and target 127, so S V / 65536 is
    rplgpu_score_poses_dev's weight of the same pose."""
    import torch
    dev = torch.device("cuda:0")
    case = rc.identity_case(oracle)
    want, weights = rc.identity_regime(oracle, case)
    got = _run(gpu, case, "sums")
    _check(got, want, stepped=False)
    s = case["spec"]
    B, n = case["batch"].shape
    P = case["poses"].shape[1]
    d = _upload(case)
    host_field, fstride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    host_poses, pstride = _pose_buffer(case)
    d_poses = torch.from_numpy(host_poses.reshape(-1)).to(dev)
    d_w = torch.zeros(P, dtype=torch.int32, device=dev)
    d_res = torch.zeros(8, dtype=torch.int32, device=dev)
    gpu.score_poses_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, 1, case["p"], 0, d["pose2d"].data_ptr(),
                        abi.PoseScore(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"]),
                        d_poses.data_ptr(), P, pstride, 0, d_field.data_ptr(), fstride, 0, d_w.data_ptr(), P,
                        d_res.data_ptr(), 0)
    gpu.synchronize()
    w = d_w.cpu().numpy().view(np.uint32)
    sv = [int(v[10]) | (int(v[11]) << 32) for v in got[1][0]]
    assert [v >> 16 for v in sv] == [int(v) for v in w] == [int(v) for v in weights] and not any(v & 0xFFFF for v in sv)


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------
def test_chain_match_refine_map(gpu, oracle):
    """rplgpu_match_scans_dev -> rplgpu_match_poses_dev -> rplgpu_refine_poses_dev -> rplgpu_compose_poses_dev ->
    rplgpu_map_update_dev on one stream with no read in between, against the oracles chained the same way."""
    import torch
    dev = torch.device("cuda:0")
    m, mounts, s = rc.chain_case(oracle)
    ms, o = m["spec"], mc.room_occ_spec()
    B, n = m["batch"].shape
    W, H = s["width"], s["height"]
    # the oracles, chained
    _, best, _ = mc.case_want(oracle, m, "refine_chain_match")[0]
    best = np.asarray(best, np.int64).astype(np.uint32)
    pose0 = ro.match_pose(best, mo.rotations(ms), ms["rot_steps"], ms["resolution"], m["pivot"][0], None)
    base = dict(batch=m["batch"], lens=m["lens"], group=2, p=m["p"], spec=s, fields=m["fields"], pose2d=mounts,
                poses=pose0[None, None])
    wo, wsums, wstep, wres, wst = rc.case_want(oracle, base, "refine_chain", iters=rc.CHAIN_ITERS)[0]
    assert wres[0] == 1 and wst == 0 and wo[0].tobytes() != pose0.tobytes() and int(best[1]) != 0
    wpose2d = np.stack([ro.compose_pose(wo[int(wres[4])], mounts[b]) for b in range(B)])
    wcounts, wmst = mp.map_group(oracle, list(m["batch"]), m["p"], o, None, wpose2d)
    # the device
    d = _upload(m)
    d_pivot = torch.from_numpy(np.ascontiguousarray(m["pivot"], F32)).to(dev)
    d_mounts = torch.from_numpy(mounts).to(dev)
    host_field, fstride = _field_buffer(dict(spec=s, fields=m["fields"]))
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    vol = mo.volume_size(ms)
    d_scores = torch.zeros(vol, dtype=torch.int32, device=dev)
    d_best = torch.zeros(8, dtype=torch.int32, device=dev)
    d_list = torch.full((8,), 7.0, dtype=torch.float32, device=dev)
    d_pose2d_out = torch.full((6 * B + 6,), 7.0, dtype=torch.float32, device=dev)
    d_counts = torch.zeros(2 * W * H, dtype=torch.int32, device=dev)
    d_mst = torch.zeros(1, dtype=torch.int32, device=dev)
    b = _Buffers(1, 1)
    match = abi.ScanMatch(ms["origin_x"], ms["origin_y"], ms["resolution"], ms["width"], ms["height"], ms["shift_x"],
                          ms["shift_y"], ms["rot_steps"], ms["rot_step"])
    grid = abi.OccGrid(o["origin_x"], o["origin_y"], o["resolution"], W, H, o["range_min"], o["obstacle_max"],
                       o["raytrace_max"])
    front = (d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, 2, m["p"], 0)
    gpu.match_scans_dev(*front, d["pose2d"].data_ptr(), d_pivot.data_ptr(), match, d_field.data_ptr(), fstride, 0,
                        d_scores.data_ptr(), vol, d_best.data_ptr(), 0)
    gpu.match_poses_dev(d_best.data_ptr(), match, d_pivot.data_ptr(), 0, 1, d_list.data_ptr(), 4)
    gpu.refine_poses_dev(*front, d_mounts.data_ptr(), ro.struct_of(s), d_list.data_ptr(), 1, 4, 1, d_field.data_ptr(),
                         fstride, 0, rc.CHAIN_ITERS, b.out.data_ptr(), b.out_stride, b.sums.data_ptr(), b.sums_stride,
                         b.step.data_ptr(), b.step_stride, b.scratch.data_ptr(), b.res.data_ptr(), b.st.data_ptr())
    gpu.compose_poses_dev(b.out.data_ptr(), b.out_stride, 1, 1, b.res.data_ptr(), 0, d_mounts.data_ptr(), B, 2,
                          d_pose2d_out.data_ptr())
    gpu.map_update_dev(*front, d_pose2d_out.data_ptr(), grid, d_counts.data_ptr(), d_mst.data_ptr())
    gpu.synchronize()
    assert d_best.cpu().numpy().view(np.uint32).tobytes() == best.tobytes()
    lst = d_list.cpu().numpy()
    assert lst[:4].tobytes() == pose0.tobytes() and (lst[4:] == 7.0).all()
    _check(b.read(), [(wo, wsums, wstep, wres, wst)])
    p2 = d_pose2d_out.cpu().numpy()
    assert p2[:6 * B].tobytes() == wpose2d.tobytes() and (p2[6 * B:] == 7.0).all()
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == mp.as_words(wcounts).tobytes()
    assert int(d_mst.cpu().numpy()[0]) == wmst
    # the joints' other branches: a constant q, a q beyond the list and a k outside the table keep what they were given
    gpu.compose_poses_dev(b.out.data_ptr(), b.out_stride, 1, 1, 0, 5, d_mounts.data_ptr(), B, 2, d_pose2d_out.data_ptr())
    bad = torch.from_numpy(np.array([1, ms["rot_steps"] + 1, 0, 0, 0, 0, 1, 0], np.int32)).to(dev)
    d_prior = torch.from_numpy(np.array([0.6, 0.8, 1.5, -2.5], F32)).to(dev)
    gpu.match_poses_dev(bad.data_ptr(), match, d_pivot.data_ptr(), d_prior.data_ptr(), 1, d_list.data_ptr(), 4)
    gpu.synchronize()
    assert d_pose2d_out.cpu().numpy()[:6 * B].tobytes() == mounts.tobytes()
    assert d_list.cpu().numpy()[:4].tobytes() == d_prior.cpu().numpy().tobytes()
    prior = np.array([0.6, 0.8, 1.5, -2.5], F32)
    gpu.match_poses_dev(d_best.data_ptr(), match, d_pivot.data_ptr(), d_prior.data_ptr(), 1, d_list.data_ptr(), 4)
    gpu.synchronize()
    want = ro.match_pose(best, mo.rotations(ms), ms["rot_steps"], ms["resolution"], m["pivot"][0], prior)
    assert d_list.cpu().numpy()[:4].tobytes() == want.tobytes()


# ---- the door -----------------------------------------------------------------------------------------------------------------------------------
def test_host_door(gpu, oracle):
    case = rc.groups_case(0, 0)
    one = dict(case, batch=case["batch"][:2], lens=case["lens"][:2], pose2d=case["pose2d"][:2])
    wo, wsums, wstep, wres, wst = rc.case_want(oracle, one, "door", iters=2)[0]
    out, sums, step, res, status = gpu.refine_poses(one["batch"], one["lens"], one["p"], ro.struct_of(one["spec"]),
                                                    one["poses"][0], one["fields"][0], 2, pose2d=one["pose2d"])
    assert out.tobytes() == wo.tobytes() and sums.tobytes() == wsums.tobytes() and step.tobytes() == wstep.tobytes()
    assert res.tobytes() == wres.tobytes() and status == wst
