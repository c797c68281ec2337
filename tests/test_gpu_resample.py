"""E16 on the device: rplgpu_resample_poses_dev against tests/resample_oracle.py byte for byte — the new list, the
ancestors, d_result, the guard words behind every group's outputs, behind the result words and behind the scratch,
and the unchanged weights, poses, deltas and random words.  The inputs and their regime checks live in
tests/resample_cases.py."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import pose_cases as pc
from tests import resample_cases as rc
from tests import resample_oracle as ro

pytestmark = pytest.mark.gpu
F32 = np.float32
U32_MAX = 0xFFFFFFFF
GUARD_WORD = 0x5A5A5A5A
PAD = 5  # guard words (or poses) behind every group's part of an array


def _buffers(case, pad=PAD, ancestors=True, with_u=True):
    """Device copies of a case's inputs (every group's part followed by `pad` guard entries) and guarded outputs."""
    import torch
    dev = torch.device("cuda:0")
    G, P = case["w"].shape
    M = case["M"]
    b = dict(G=G, P=P, M=M)
    h_w = np.full((G, P + pad), GUARD_WORD, np.uint32)
    h_w[:, :P] = case["w"]
    L = len(case["poses"])
    h_p = np.full((L, 4 * (P + pad)), 123.0, F32)
    h_p[:, :4 * P] = case["poses"].reshape(L, 4 * P)
    b.update(h_w=h_w, h_p=h_p, wstride=P + pad, pstride=4 * (P + pad), ppg=1 if L > 1 else 0)
    up = lambda a: torch.from_numpy(a.reshape(-1).view(np.int32 if a.dtype == np.uint32 else a.dtype)).to(dev)  # noqa: E731
    b["d_w"], b["d_p"] = up(h_w), up(h_p)
    b["h_u"] = b["d_u"] = None
    if case["u"] is not None and with_u:
        b["h_u"] = np.ascontiguousarray(case["u"], np.uint32)
        b["d_u"] = up(b["h_u"])
    b["h_d"] = b["d_d"] = None
    b.update(n_delta=0, dstride=0, dpg=0)
    if case["delta"] is not None:
        Ld, nd, _ = case["delta"].shape
        h_d = np.full((Ld, 4 * (nd + pad)), 321.0, F32)
        h_d[:, :4 * nd] = case["delta"].reshape(Ld, 4 * nd)
        b.update(h_d=h_d, d_d=up(h_d), n_delta=nd, dstride=4 * (nd + pad), dpg=1 if Ld > 1 else 0)
    words = abi.resample_scratch_words(G, P)
    b.update(ostride=4 * (M + pad), astride=M + pad, words=words)
    b["d_out"] = torch.full((G * b["ostride"],), GUARD_WORD, dtype=torch.int32, device=dev)
    b["d_anc"] = torch.full((G * b["astride"],), GUARD_WORD, dtype=torch.int32, device=dev) if ancestors else None
    b["d_res"] = torch.full((8 * G + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    b["d_scr"] = torch.full((words + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    return b


def _call(gpu, b, **kw):
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    a = dict(w=ptr(b["d_w"]), wstride=b["wstride"], poses=ptr(b["d_p"]), pstride=b["pstride"], ppg=b["ppg"],
             G=b["G"], P=b["P"], M=b["M"], u=ptr(b["d_u"]), delta=ptr(b["d_d"]), n_delta=b["n_delta"],
             dstride=b["dstride"], dpg=b["dpg"], out=ptr(b["d_out"]), ostride=b["ostride"], anc=ptr(b["d_anc"]),
             astride=b["astride"], res=ptr(b["d_res"]), scr=ptr(b["d_scr"]))
    a.update(kw)
    gpu.resample_poses_dev(a["w"], a["wstride"], a["poses"], a["pstride"], a["ppg"], a["G"], a["P"], a["M"], a["u"],
                           a["delta"], a["n_delta"], a["dstride"], a["dpg"], a["out"], a["ostride"], a["anc"],
                           a["astride"], a["res"], a["scr"])


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _inputs_unchanged(b):
    assert _u32(b["d_w"]).tobytes() == b["h_w"].tobytes()
    assert b["d_p"].cpu().numpy().tobytes() == b["h_p"].tobytes()
    if b["d_u"] is not None:
        assert _u32(b["d_u"]).tobytes() == b["h_u"].tobytes()
    if b["d_d"] is not None:
        assert b["d_d"].cpu().numpy().tobytes() == b["h_d"].tobytes()


def _outputs_untouched(b):
    for k in ("d_out", "d_anc", "d_res", "d_scr"):
        assert b[k] is None or (_u32(b[k]) == GUARD_WORD).all(), k


def _run(gpu, case, **kw):
    """-> (out (G, M, 4) float32, ancestors (G, M) uint32 or None, result (G, 8) uint32); guards and inputs checked."""
    b = _buffers(case, **kw)
    _call(gpu, b)
    gpu.synchronize()
    _inputs_unchanged(b)
    G, M = b["G"], b["M"]
    out = _u32(b["d_out"]).reshape(G, b["ostride"])
    res = _u32(b["d_res"])
    assert (out[:, 4 * M:] == GUARD_WORD).all() and (res[8 * G:] == GUARD_WORD).all()
    assert (_u32(b["d_scr"])[b["words"]:] == GUARD_WORD).all()
    anc = None
    if b["d_anc"] is not None:
        anc = _u32(b["d_anc"]).reshape(G, b["astride"])
        assert (anc[:, M:] == GUARD_WORD).all()
        anc = anc[:, :M]
    return np.ascontiguousarray(out[:, :4 * M]).view(F32).reshape(G, M, 4), anc, res[:8 * G].reshape(G, 8)


def _check(got, want_):
    out, anc, res = got
    assert len(out) == len(want_)
    for g, (wo, wa, wr) in enumerate(want_):
        bad = np.flatnonzero(anc[g] != wa) if anc is not None else []
        rows = np.flatnonzero((out[g].view(np.uint32) != wo.view(np.uint32)).any(1))
        if g < 3 or len(bad) or len(rows) or res[g].tobytes() != wr.tobytes():
            print(f"group {g}: result {res[g].tolist()} want {wr.tolist()}, {len(bad)} ancestors and {len(rows)} "
                  f"poses of {len(wa)} differ")
        assert len(bad) == 0, (g, bad[:8], anc[g][bad[:8]], wa[bad[:8]])
        assert len(rows) == 0, (g, rows[:8], out[g][rows[:4]], wo[rows[:4]])
        assert res[g].tobytes() == wr.tobytes(), (g, res[g], wr)


# ---- tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", rc.EDGE_P)
def test_tile_edges(gpu, P):
    for M in rc.edge_ms(P):
        case = rc.edge_case(P, M)
        rc.edge_regime(case)
        _check(_run(gpu, case), rc.want(case, f"edge{P}_{M}"))


# ---- dead stretches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.DEAD_KINDS)
def test_dead_stretches(gpu, kind):
    case = rc.dead_case(kind)
    rc.dead_regime(case, kind)
    _check(_run(gpu, case), rc.want(case, f"dead_{kind}"))


# ---- extremes -------------------------------------------------------------------------------------------------------------------
def test_every_weight_at_its_maximum(gpu):
    case = rc.allmax_case()
    rc.allmax_regime(case)
    _check(_run(gpu, case), rc.want(case, "allmax"))


def test_sum_below_the_number_of_outputs(gpu):
    case = rc.small_case()
    rc.small_regime(case)
    _check(_run(gpu, case), rc.want(case, "small"))


@pytest.mark.parametrize("u", [0, U32_MAX])
def test_ends_of_u(gpu, u):
    rc.u_regime()
    _check(_run(gpu, rc.u_case(u)), rc.want(rc.u_case(u), "u0" if u == 0 else "umax"))


def test_one_workgroup_walks_every_output(gpu):
    case = rc.walk_case()
    rc.walk_regime(case)
    _check(_run(gpu, case), rc.want(case, "walk"))


def test_largest_list(gpu):
    case = rc.big_case()
    rc.big_regime(case)
    _check(_run(gpu, case), rc.want(case, "big"))


# ---- S = 0 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", rc.ZERO_M)
def test_every_pose_dead(gpu, M):
    case = rc.zero_case(M)
    rc.zero_regime(case)
    _check(_run(gpu, case), rc.want(case))
    small = rc.zero_case(5, P=3)
    _check(_run(gpu, small), rc.want(small))


# ---- the move ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_delta,G,per_group,special", [
    (0, 1, 0, False), (1, 1, 0, False), (rc.MOVE_M, 1, 0, False), (0, 1, 0, True), (1, 1, 0, True),
    (rc.MOVE_M, 1, 0, True), (1, 3, 0, True), (1, 3, 1, True), (rc.MOVE_M, 3, 0, False), (rc.MOVE_M, 3, 1, True)])
def test_move(gpu, n_delta, G, per_group, special):
    case = rc.move_case(n_delta, G, per_group, special)
    rc.move_regime(case, special)
    _check(_run(gpu, case), rc.want(case))


def test_identity_delta_is_not_the_bit_copy(gpu):
    case = rc.minus_zero_case()
    moved = _run(gpu, case)
    copied = _run(gpu, dict(case, delta=None))
    _check(moved, rc.want(case))
    _check(copied, rc.want(dict(case, delta=None)))
    rc.minus_zero_check(moved[0][0], copied[0][0])


# ---- groups -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppg", [0, 1])
def test_groups(gpu, ppg):
    case = rc.groups_case(ppg)
    rc.groups_regime(case)
    want_ = rc.want(case, f"groups{len(case['poses'])}")
    _check(_run(gpu, case, pad=PAD + 59 * ppg), want_)  # strides larger than needed, twice


def test_optional_pointers_left_out(gpu):
    case = rc.groups_case(0)
    want_ = rc.want(case, "groups1")
    out, anc, res = _run(gpu, case, ancestors=False)          # d_ancestors NULL: the same list and words
    assert anc is None
    _check((out, None, res), want_)
    no_u = dict(case, u=None)                                 # d_u NULL: u = 0 in every group
    want0 = rc.want(no_u, "groups_u0")
    assert any(a[1].tobytes() != b[1].tobytes() for a, b in zip(want_, want0))
    _check(_run(gpu, case, with_u=False), want0)


# ---- the result words -------------------------------------------------------------------------------------------------------------
def test_result_words(gpu):
    case = rc.words_case()
    rc.words_regime(case)
    got = _run(gpu, case)
    _check(got, rc.want(case, "words"))
    assert got[2][0][4] >= 3 and got[2][0][5] == 105


def test_result_words_across_the_scan_kernels_waves(gpu):
    case = rc.words_wide_case()
    rc.words_wide_regime(case)
    _check(_run(gpu, case), rc.want(case, "words_wide"))


# ---- the chain with E15, between the real kernels ---------------------------------------------------------------------------------
def test_chain_score_resample_score(gpu, oracle):
    """score -> resample (no delta) -> score on the same points and field, all queued before anything is read: the
    second call's weight j is the first call's weight a[j]."""
    import torch
    dev = torch.device("cuda:0")
    P = M = 2049
    case = pc.layout_case(P)
    w1_want = pc.case_want(oracle, case, f"layout{P}")[0][0]
    u = 0x9E3779B9
    a_want = ro.ancestors_search(w1_want, M, u)
    k = np.bincount(a_want, minlength=P)
    assert len(np.unique(a_want)) >= 2 and ((k == 0) & (w1_want > 0)).any() and k.max() >= 2  # the regime
    s = case["spec"]
    spec = abi.PoseScore(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"])
    B, n = case["batch"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_nodes = up(np.ascontiguousarray(case["batch"]).view(np.uint8).reshape(B, n * 8))
    d_lens = up(np.asarray(case["lens"], np.int32))
    d_pose2d = up(case["pose2d"])
    cells = s["width"] * s["height"]
    fstride = (cells + 3) & ~3
    h_field = np.zeros(fstride, np.int8)
    h_field[:cells] = case["fields"][0].reshape(-1)
    d_field = up(h_field)
    d_poses = up(case["poses"][0].reshape(-1))
    d_w1 = torch.full((P + PAD,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_w2 = torch.full((M + PAD,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((24 + 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_u = up(np.array([u], np.uint32).view(np.int32))
    d_out = torch.full((4 * (M + PAD),), GUARD_WORD, dtype=torch.int32, device=dev)
    d_anc = torch.full((M + PAD,), GUARD_WORD, dtype=torch.int32, device=dev)
    words = abi.resample_scratch_words(1, P)
    d_scr = torch.full((words + 8,), GUARD_WORD, dtype=torch.int32, device=dev)

    def score(d_list, count, d_w, d_r):
        gpu.score_poses_dev(d_nodes.data_ptr(), n, d_lens.data_ptr(), B, case["group"], case["p"], 0,
                            d_pose2d.data_ptr(), spec, d_list, count, 4 * count, 0, d_field.data_ptr(), fstride, 0,
                            d_w, count + PAD, d_r, 0)

    score(d_poses.data_ptr(), P, d_w1.data_ptr(), d_res.data_ptr())
    gpu.resample_poses_dev(d_w1.data_ptr(), P + PAD, d_poses.data_ptr(), 4 * P, 0, 1, P, M, d_u.data_ptr(), 0, 0, 0,
                           0, d_out.data_ptr(), 4 * (M + PAD), d_anc.data_ptr(), M + PAD,
                           d_res.data_ptr() + 32, d_scr.data_ptr())
    score(d_out.data_ptr(), M, d_w2.data_ptr(), d_res.data_ptr() + 64)
    gpu.synchronize()  # nothing was read until here
    w1, w2, anc = _u32(d_w1), _u32(d_w2), _u32(d_anc)
    assert (w1[P:] == GUARD_WORD).all() and (w2[M:] == GUARD_WORD).all() and (anc[M:] == GUARD_WORD).all()
    assert (_u32(d_res)[24:] == GUARD_WORD).all() and (_u32(d_out)[4 * M:] == GUARD_WORD).all()
    assert w1[:P].tobytes() == w1_want.tobytes() and anc[:M].tobytes() == a_want.tobytes()
    assert w2[:M].tobytes() == w1[:P][anc[:M]].tobytes()
    res = _u32(d_res)[:24].reshape(3, 8)
    assert res[1].tobytes() == ro.result_of(w1_want, M, a_want).tobytes()
    assert (int(res[1][0]) | int(res[1][1]) << 32) == (int(res[0][6]) | int(res[0][7]) << 32)  # E15's sum is E16's S
    assert _u32(d_out)[:4 * M].tobytes() == case["poses"][0][a_want].tobytes()


# ---- the door, refusals --------------------------------------------------------------------------------------------------------------
def test_host_buffers_one_group(gpu):
    for case in (rc.edge_case(1025, 1026), rc.move_case(1, 1, 0, True), rc.move_case(rc.MOVE_M, 1, 0, False),
                 rc.zero_case(700)):
        w, poses, M, u, d = rc.group_inputs(case, 0)
        wo, wa, wr = rc.want(case)[0]
        out, anc, res = gpu.resample_poses(w, poses, M, u, d)
        assert out.tobytes() == wo.tobytes() and anc.tobytes() == wa.tobytes() and res.tobytes() == wr.tobytes()
    lib = abi.load_library()
    w = np.array([1, 2, 3], np.uint32)
    buf = np.full(64, 7.0, F32)
    res = np.full(8, GUARD_WORD, np.uint32)
    at = lambda k: buf.ctypes.data + 4 * k  # noqa: E731

    def door(weights=w.ctypes.data, P=3, M=4, poses=None, dl=0, n_delta=0, out=None, res_=res.ctypes.data):
        return lib.rplgpu_resample_poses(gpu._h, weights, P, M, 5, at(0) if poses is None else poses, dl, n_delta,
                                         at(32) if out is None else out, 0, res_)

    bad = abi.ERR_INVALID_ARG
    assert door(weights=0) == bad and door(poses=0) == bad and door(out=0) == bad and door(res_=0) == bad
    assert door(P=0) == bad and door(M=0) == bad and door(P=abi.MAX_POSES + 1) == bad
    assert door(M=abi.MAX_POSES + 1) == bad and door(dl=at(60), n_delta=2) == bad and door(out=at(8)) == bad
    assert (buf == 7.0).all() and (res == GUARD_WORD).all()
    assert door() == abi.OK and res[0] == 6 and (buf[48:] == 7.0).all()


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu):
    import torch
    case = rc.move_case(rc.MOVE_M, 3, 1, False)
    b = _buffers(case)
    G, P, M = b["G"], b["P"], b["M"]
    host = np.zeros(64, np.uint32)
    hp = host.ctypes.data + (-host.ctypes.data % 16)

    def call(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            _call(gpu, b, **kw)
        return e.value.code

    bad = abi.ERR_INVALID_ARG
    assert call(G=0) == bad and call(G=65536) == bad
    assert call(P=0) == bad and call(M=0) == bad
    assert call(P=abi.MAX_POSES + 1, wstride=1 << 21, pstride=1 << 23) == bad
    assert call(M=abi.MAX_POSES + 1, ostride=1 << 23, astride=1 << 21, n_delta=abi.MAX_POSES + 1, dstride=1 << 23) == bad
    for k in ("w", "poses", "out", "res", "scr"):                         # required pointers
        assert call(**{k: 0}) == bad, k
    for k, step in (("w", 2), ("poses", 4), ("poses", 8), ("out", 4), ("out", 8), ("res", 1), ("scr", 4), ("u", 2),
                    ("delta", 4), ("delta", 8), ("anc", 2)):              # alignment
        t = b[dict(w="d_w", poses="d_p", out="d_out", res="d_res", scr="d_scr", u="d_u", delta="d_d", anc="d_anc")[k]]
        assert call(**{k: t.data_ptr() + step}) == bad, (k, step)
    assert call(wstride=P - 1) == bad
    assert call(pstride=4 * P - 4) == bad and call(pstride=4 * P + 2) == bad
    assert call(ostride=4 * M - 4) == bad and call(ostride=4 * M + 2) == bad
    assert call(astride=M - 1) == bad
    assert call(dstride=4 * M - 4) == bad and call(dstride=4 * M + 2) == bad
    assert call(n_delta=0) == bad and call(n_delta=2) == bad and call(n_delta=M - 1) == bad
    # the overlap: the new list inside the old one, at its last pose, and the old one inside the new one's range
    assert call(out=b["d_p"].data_ptr()) == bad
    assert call(out=b["d_p"].data_ptr() + 4 * ((G - 1) * b["pstride"] + 4 * P - 4), ostride=4 * M) == bad
    assert call(poses=b["d_out"].data_ptr() + 4 * ((G - 1) * b["ostride"] + 4 * M - 4), ppg=0) == bad
    for k in ("w", "poses", "out", "res", "scr", "u", "delta", "anc"):   # plain host memory, pointer by pointer
        assert call(**{k: hp}) == bad, k
    assert abi.load_library().rplgpu_resample_poses_dev(
        None, b["d_w"].data_ptr(), b["wstride"], b["d_p"].data_ptr(), b["pstride"], 1, G, P, M, 0, 0, 0, 0, 0,
        b["d_out"].data_ptr(), b["ostride"], 0, 0, b["d_res"].data_ptr(), b["d_scr"].data_ptr()) == bad
    gpu.synchronize()
    torch.cuda.synchronize()
    _outputs_untouched(b)
    _inputs_unchanged(b)
    # adjacent is no overlap: the new list right behind the old one (one buffer), then a good call on the case
    _check(_run(gpu, case), rc.want(case))
