"""E19 on the device: rplgpu_seed_poses_dev against tests/seed_oracle.py byte for byte — the M poses, the cell indices
and the eight result words of every group, the guard words behind every group's outputs and behind the result words,
and the unchanged grid and heading table.  The inputs and their regime checks live in tests/seed_cases.py."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi
from tests import estimate_oracle as eo
from tests import match_cases as mtc
from tests import motion_cases as mc
from tests import seed_cases as sc
from tests import seed_oracle as so

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD_WORD = 0x5A5A5A5A
GUARD_BYTE = 0                         # the stride padding of a grid looks free under (0, 0) and must not count
PAD = 5                                # guard poses behind every group's list


def _up(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda:0"))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _full(k):
    import torch
    return torch.full((k,), GUARD_WORD, dtype=torch.int32, device=torch.device("cuda:0"))


def _buffers(case, pad=PAD, cells=True):
    """Device copies of a case's grids (each followed by free-looking padding up to its stride) and heading table
    (followed by two guard entries), guarded outputs and the scratch."""
    import torch
    dev = torch.device("cuda:0")
    G, M, s = case["G"], case["M"], case["spec"]
    L = len(case["grids"])
    n = s["width"] * s["height"]
    gstride = ((n + 3) & ~3) + 8
    pad_byte = s["free_lo"] if not s["free_lo"] <= GUARD_BYTE <= s["free_hi"] else GUARD_BYTE
    h_g = np.full((L, gstride), pad_byte, np.int8)
    h_g[:, :n] = case["grids"]
    H = len(case["headings"])
    h_t = np.full((H + 2, 2), 123.0, F32)
    h_t[:H] = case["headings"]
    b = dict(G=G, M=M, H=H, spec=sc.spec_of(s), noise=sc.noise_of(case["noise"]), h_g=h_g, d_g=_up(h_g), gstride=gstride,
             gpg=1 if L > 1 else 0, h_t=h_t, d_t=_up(h_t.view(np.uint32)), ostride=4 * (M + pad), cstride=M + pad)
    b["d_out"] = _full(G * 4 * (M + pad))
    b["d_cells"] = _full(G * (M + pad)) if cells else None
    b["d_res"] = _full(8 * G + 8)
    words = abi.seed_scratch_words(L, s["width"], s["height"])
    assert words > 0
    b["d_scr"] = torch.full((words + 2,), GUARD_WORD, dtype=torch.int32, device=dev)   # (whatever it held before)
    return b


def _call(gpu, b, **kw):
    a = dict(spec=b["spec"], grid=b["d_g"].data_ptr(), gstride=b["gstride"], gpg=b["gpg"], head=b["d_t"].data_ptr(),
             H=b["H"], G=b["G"], M=b["M"], noise=b["noise"], out=b["d_out"].data_ptr(), ostride=b["ostride"],
             cells=b["d_cells"].data_ptr() if b["d_cells"] is not None else 0, cstride=b["cstride"],
             res=b["d_res"].data_ptr(), scr=b["d_scr"].data_ptr())
    a.update(kw)
    gpu.seed_poses_dev(a["spec"], a["grid"], a["gstride"], a["gpg"], a["head"], a["H"], a["G"], a["M"], a["noise"],
                       a["out"], a["ostride"], a["cells"], a["cstride"], a["res"], a["scr"])


def _outputs_untouched(b):
    for k in ("d_out", "d_cells", "d_res"):
        assert (_u32(b[k]) == GUARD_WORD).all(), k


def _inputs_unchanged(b):
    assert b["d_g"].cpu().numpy().tobytes() == b["h_g"].tobytes()
    assert _u32(b["d_t"]).tobytes() == b["h_t"].tobytes()


def _read(b):
    G, M = b["G"], b["M"]
    _inputs_unchanged(b)
    res = _u32(b["d_res"])
    assert (res[8 * G:] == GUARD_WORD).all()
    assert (_u32(b["d_scr"])[-2:] == GUARD_WORD).all()
    out = _u32(b["d_out"]).reshape(G, b["ostride"])
    assert (out[:, 4 * M:] == GUARD_WORD).all()
    cells = None
    if b["d_cells"] is not None:
        cells = _u32(b["d_cells"]).reshape(G, b["cstride"])
        assert (cells[:, M:] == GUARD_WORD).all()
        cells = cells[:, :M]
    return out[:, :4 * M].reshape(G, M, 4), cells, res[:8 * G].reshape(G, 8)


def _run(gpu, case, **kw):
    """-> (pose words (G, M, 4), cells (G, M) or None, result (G, 8)); guards and the inputs checked"""
    b = _buffers(case, **kw)
    _call(gpu, b)
    gpu.synchronize()
    return _read(b)


def _check(got, want_):
    words, cells, res = got
    assert words.shape == want_[0].shape and res.shape == want_[2].shape
    for g in range(len(res)):
        if res[g].tobytes() != want_[2][g].tobytes():
            print(f"group {g}: result {res[g].tolist()} want {want_[2][g].tolist()}")
        if cells is not None and cells[g].tobytes() != want_[1][g].tobytes():
            bad = np.flatnonzero(cells[g] != want_[1][g])
            print(f"group {g}: {len(bad)} of {len(cells[g])} cells differ, first {int(bad[0])}: "
                  f"{int(cells[g][bad[0]])} want {int(want_[1][g][bad[0]])}")
        if words[g].tobytes() != want_[0][g].tobytes():
            bad = np.flatnonzero((words[g] != want_[0][g]).any(axis=1))
            j = int(bad[0])
            print(f"group {g}: {len(bad)} of {len(words[g])} outputs differ, first {j}: "
                  f"{[hex(v) for v in words[g][j]]} want {[hex(v) for v in want_[0][g][j]]}")
        assert cells is None or cells[g].tobytes() == want_[1][g].tobytes(), g
        assert words[g].tobytes() == want_[0][g].tobytes(), g
        assert res[g].tobytes() == want_[2][g].tobytes(), g


# ---- grid sizes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", sc.SIZES)
def test_grid_sizes(gpu, width, height):
    case = sc.size_case(width, height)
    want_ = sc.want(case, f"size{width}x{height}")
    sc.size_regime(case, want_)
    _check(_run(gpu, case), want_)


def test_default_grid_and_largest_list(gpu):
    case = sc.default_case()
    want_ = sc.want(case, "default")
    sc.default_regime(case, want_)
    _check(_run(gpu, case), want_)


def test_largest_grid_sparse(gpu):
    case = sc.sparse_case()
    want_ = sc.want(case, "sparse")
    sc.sparse_regime(case, want_)
    _check(_run(gpu, case), want_)


# ---- free-cell patterns, byte values ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.PATTERNS)
def test_patterns(gpu, name):
    case = sc.pattern_case(name)
    want_ = sc.want(case, f"pattern_{name}")
    sc.pattern_regime(name, case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("lo,hi", sc.RANGES)
def test_byte_values(gpu, lo, hi):
    case = sc.bytes_case(lo, hi)
    want_ = sc.want(case, f"bytes{lo}_{hi}")
    sc.bytes_regime(case, want_)
    _check(_run(gpu, case), want_)


# ---- M, groups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", sc.EDGE_M)
def test_tile_edges(gpu, M):
    case = sc.edge_case(M)
    want_ = sc.want(case, f"edge{M}")
    sc.edge_regime(case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("gpg", [0, 1])
def test_groups(gpu, gpg):
    case = sc.groups_case(gpg)
    want_ = sc.want(case, f"groups{gpg}")
    sc.groups_regime(case, want_)
    _check(_run(gpu, case, pad=PAD + 59 * gpg), want_)        # a stride larger than needed, twice


def test_without_cell_indices(gpu):
    case = sc.groups_case(1)
    got = _run(gpu, case, cells=False)
    assert got[1] is None
    _check(got, sc.want(case, "groups1"))


# ---- headings, counters, pieces, flags, the round trip ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one", "most", "bits"])
def test_headings(gpu, kind):
    case = sc.headings_case(kind)
    want_ = sc.want(case, f"headings_{kind}")
    sc.headings_regime(kind, case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("kind", sc.COUNTER_KINDS)
def test_counters(gpu, kind):
    case = sc.counter_case(kind)
    want_ = sc.want(case, f"counter_{kind}")
    sc.counter_regime(kind, want_)
    _check(_run(gpu, case), want_)


def test_a_list_in_three_pieces(gpu):
    """three calls with first = 0, 1000 and 1001 into one list equal one call"""
    whole, pieces, cuts = sc.piece_cases()
    want_ = sc.want(whole, "whole")
    one = _run(gpu, whole)
    _check(one, want_)
    b = _buffers(whole)
    for piece, lo in zip(pieces, cuts):
        _call(gpu, b, M=piece["M"], noise=sc.noise_of(piece["noise"]), out=b["d_out"].data_ptr() + 16 * lo,
              cells=b["d_cells"].data_ptr() + 4 * lo)
    gpu.synchronize()
    words, cells, res = _read(b)
    assert words.tobytes() == one[0].tobytes() == want_[0].tobytes() and cells.tobytes() == want_[1].tobytes()
    assert res.tobytes() == sc.want(pieces[-1])[2].tobytes()     # the result words are those of the last call


def test_cell_centres(gpu):
    case = sc.centres_case()
    want_ = sc.want(case, "centres")
    sc.centres_regime(case, want_)
    _check(_run(gpu, case), want_)


def test_the_round_trip_counts(gpu):
    near, far = sc._small(), sc.far_case()
    a, b = sc.want(near, "small"), sc.want(far, "far")
    sc.small_regime(near, a)
    sc.far_regime(far, b)
    _check(_run(gpu, near), a)
    _check(_run(gpu, far), b)


# ---- identities with independent kernels, chains ------------------------------------------------------------------------
def test_free_cells_as_e11_counts_them(gpu):
    """E11 writes a grid and counts its 0-cells (d_cells word 0); E19 on that grid with (0, 0) reports the same F,
    with nothing read in between — and the list is the oracle's over the grid E11 wrote"""
    batch, lens, pose2d = mtc.room_scans()
    B, n = batch.shape
    o = mtc.room_occ_spec()
    W, H = o["width"], o["height"]
    stride = (W * H + 3) & ~3
    M = 3000
    spec = dict(so.DEFAULT, **{k: o[k] for k in ("origin_x", "origin_y", "resolution", "width", "height")})
    noise = dict(seed=11, step=19, first=0)
    d_nodes = _up(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8))
    d_len, d_pose = _up(np.asarray(lens, np.int32)), _up(pose2d)
    d_grid = _full(stride // 4 + 1)
    d_count = _full(4)
    d_head = _up(sc.table(64).view(np.uint32))
    d_out, d_cells, d_res = _full(4 * M + 4), _full(M + 1), _full(9)
    d_scr = _full(abi.seed_scratch_words(1, W, H))
    grid = abi.OccGrid(o["origin_x"], o["origin_y"], o["resolution"], W, H, o["range_min"], o["obstacle_max"],
                       o["raytrace_max"])
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, B, Params.defaults(**mtc.ROOM_P), 0,
                           d_pose.data_ptr(), grid, 0, d_grid.data_ptr(), stride, d_count.data_ptr())
    gpu.seed_poses_dev(sc.spec_of(spec), d_grid.data_ptr(), stride, 0, d_head.data_ptr(), 64, 1, M, sc.noise_of(noise),
                       d_out.data_ptr(), 4 * M, d_cells.data_ptr(), M, d_res.data_ptr(), d_scr.data_ptr())
    gpu.synchronize()
    h_grid = d_grid.cpu().numpy().view(np.int8)[:W * H]
    zeros = int(_u32(d_count)[0])
    assert zeros == int((h_grid == 0).sum()) > 100 and _u32(d_res)[0] == zeros
    want_ = so.seed(h_grid, spec, sc.table(64), M, noise)
    assert _u32(d_out)[:4 * M].tobytes() == want_[0].tobytes() and _u32(d_cells)[:M].tobytes() == want_[1].tobytes()
    assert _u32(d_res)[:8].tobytes() == want_[2].tobytes()
    assert _u32(d_out)[4 * M:].tolist() == [GUARD_WORD] * 4 and _u32(d_res)[8] == GUARD_WORD
    assert (h_grid[want_[1]] == 0).all()


def _score_setup(oracle, case):
    """E15's layout case: its scans, field and spec on the device"""
    s = case["spec"]
    B, n = case["batch"].shape
    cells = s["width"] * s["height"]
    fstride = (cells + 3) & ~3
    h_field = np.zeros(fstride, np.int8)
    h_field[:cells] = case["fields"][0].reshape(-1)
    return dict(case=case, B=B, n=n, fstride=fstride,
                spec=abi.PoseScore(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"]),
                d_nodes=_up(np.ascontiguousarray(case["batch"]).view(np.uint8).reshape(B, n * 8)),
                d_lens=_up(np.asarray(case["lens"], np.int32)), d_pose2d=_up(case["pose2d"]), d_field=_up(h_field))


def _score(gpu, d, d_poses, P, pstride, d_w, d_r15):
    case = d["case"]
    gpu.score_poses_dev(d["d_nodes"].data_ptr(), d["n"], d["d_lens"].data_ptr(), d["B"], case["group"], case["p"], 0,
                        d["d_pose2d"].data_ptr(), d["spec"], d_poses, P, pstride, 0, d["d_field"].data_ptr(),
                        d["fstride"], 0, d_w.data_ptr(), P + PAD, d_r15.data_ptr(), 0)


def test_chain_map_seed_score_estimate(gpu, oracle):
    """initialise: map_grid (E14) -> seed over its 0-cells (E19) -> score (E15) -> estimate around E15's best pose
    (E17), all queued before anything is read, each against its own oracle (chained in tests/seed_cases.py); E19's F
    is E14's count of 0-cells"""
    import torch
    a = sc.init_chain(oracle)
    P = sc.CHAIN_P
    d = _score_setup(oracle, a["case"])
    s = a["case"]["spec"]
    W, H = s["width"], s["height"]
    gstride = (W * H + 3) & ~3
    d_counts = _up(a["counts"].reshape(-1))
    d_grid, d_kinds = _full(gstride // 4 + 1), _full(5)
    d_table = _up(a["table"].view(np.uint32))
    d_out, d_cells, d_w = _full(4 * (P + PAD)), _full(P + PAD), _full(P + PAD)
    d_r19, d_r15, d_est = _full(16), _full(16), _full(eo.WORDS + 8)
    d_scr19 = _full(abi.seed_scratch_words(1, W, H))
    d_scr17 = torch.zeros(abi.estimate_scratch_words(1, P), dtype=torch.int32, device=torch.device("cuda:0"))

    gpu.map_grid_dev(d_counts.data_ptr(), W, H, abi.MapRule(**a["rule"]), 0, d_grid.data_ptr(), gstride,
                     d_kinds.data_ptr())
    gpu.seed_poses_dev(sc.spec_of(a["sspec"]), d_grid.data_ptr(), gstride, 0, d_table.data_ptr(), sc.CHAIN_H, 1, P,
                       sc.noise_of(a["noise"]), d_out.data_ptr(), 4 * (P + PAD), d_cells.data_ptr(), P + PAD,
                       d_r19.data_ptr(), d_scr19.data_ptr())
    _score(gpu, d, d_out.data_ptr(), P, 4 * (P + PAD), d_w, d_r15)
    gpu.estimate_poses_dev(d_out.data_ptr(), 4 * (P + PAD), 0, d_w.data_ptr(), P + PAD, 1, P,
                           abi.PoseEstimate.defaults(), d_r15.data_ptr() + 4, 8, d_est.data_ptr(), d_scr17.data_ptr())
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_out, 4 * P), (d_cells, P), (d_w, P), (d_r19, 8), (d_r15, 8), (d_est, eo.WORDS), (d_kinds, 4)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert d_grid.cpu().numpy().view(np.int8)[:W * H].tobytes() == a["grid"].tobytes()
    assert tuple(int(v) for v in _u32(d_kinds)[:4]) == tuple(a["kinds"]) and _u32(d_r19)[0] == _u32(d_kinds)[1]
    assert _u32(d_out)[:4 * P].tobytes() == a["words"].tobytes() and _u32(d_cells)[:P].tobytes() == a["cells"].tobytes()
    assert _u32(d_r19)[:8].tobytes() == a["r19"].tobytes()
    assert _u32(d_w)[:P].tobytes() == a["w"].tobytes() and _u32(d_r15)[:8].tobytes() == a["r15"].tobytes()
    assert _u32(d_est)[:eo.WORDS].tobytes() == a["est"].tobytes()


def test_chain_sample_resample_inject_score(gpu, oracle):
    """inject: sample (E18) -> resample and move (E16) -> seed into the last M' slots of E16's list (E19, first =
    M - M') -> score (E15), under ONE seed and step and with nothing read in between: the first M - M' outputs are
    E16's bytes (moved by E18's deltas), the rest E19's — the two streams do not meet"""
    import torch
    c = sc.inject_chain(oracle)
    P = M = sc.CHAIN_P
    Mi = sc.CHAIN_INJECT
    d = _score_setup(oracle, c["case"])
    s = c["case"]["spec"]
    W, H = s["width"], s["height"]
    gstride = (W * H + 3) & ~3
    h_grid = np.zeros(gstride, np.int8)
    h_grid[:W * H] = c["grid"]
    d_grid, d_table = _up(h_grid), _up(c["table"].view(np.uint32))
    d_poses, d_w1, d_u, d_odom = _up(c["poses"]), _up(c["w1"]), _up(np.array([c["u"]], np.uint32)), _up(c["odom"])
    d_delta, d_out, d_w2 = _full(4 * (M + PAD)), _full(4 * (M + PAD)), _full(M + PAD)
    d_r18, d_r16, d_r19, d_r15 = _full(16), _full(16), _full(16), _full(16)
    d_scr16 = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=torch.device("cuda:0"))
    d_scr19 = _full(abi.seed_scratch_words(1, W, H))

    gpu.sample_motion_dev(d_odom.data_ptr(), 0, 1, M, mc.spec_of(c["noise"]), d_delta.data_ptr(), 4 * (M + PAD),
                          d_r18.data_ptr())
    gpu.resample_poses_dev(d_w1.data_ptr(), P, d_poses.data_ptr(), 4 * P, 0, 1, P, M, d_u.data_ptr(),
                           d_delta.data_ptr(), M, 4 * (M + PAD), 1, d_out.data_ptr(), 4 * (M + PAD), 0, 0,
                           d_r16.data_ptr(), d_scr16.data_ptr())
    gpu.seed_poses_dev(sc.spec_of(c["sspec"]), d_grid.data_ptr(), gstride, 0, d_table.data_ptr(), sc.CHAIN_H, 1, Mi,
                       sc.noise_of(c["inoise"]), d_out.data_ptr() + 16 * (M - Mi), 4 * Mi, 0, 0, d_r19.data_ptr(),
                       d_scr19.data_ptr())
    _score(gpu, d, d_out.data_ptr(), M, 4 * (M + PAD), d_w2, d_r15)
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_delta, 4 * M), (d_out, 4 * M), (d_w2, M), (d_r18, 8), (d_r16, 8), (d_r19, 8), (d_r15, 8)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert _u32(d_delta)[:4 * M].tobytes() == c["d_words"][0].tobytes()
    assert _u32(d_r18)[:8].tobytes() == c["r18"][0].tobytes()
    assert _u32(d_r16)[:8].tobytes() == c["r16"].tobytes() and _u32(d_r19)[:8].tobytes() == c["r19"].tobytes()
    got = _u32(d_out)[:4 * M].reshape(M, 4)
    assert got[:M - Mi].tobytes() == c["final"][:M - Mi].tobytes()         # E16's bytes
    assert got[M - Mi:].tobytes() == c["iwords"].tobytes()                 # E19's
    assert _u32(d_w2)[:M].tobytes() == c["w2"].tobytes() and _u32(d_r15)[:8].tobytes() == c["r15"].tobytes()
    assert d_grid.cpu().numpy().tobytes() == h_grid.tobytes()


# ---- the door, refusals -----------------------------------------------------------------------------------------------
def test_host_buffers_one_group(gpu):
    for case in (sc.size_case(67, 61), sc.pattern_case("none_free"), sc.far_case(), sc.counter_case("wrap"),
                 sc.headings_case("bits")):
        one = dict(case, M=min(case["M"], 3000))
        spec, noise = sc.spec_of(one["spec"]), sc.noise_of(one["noise"])
        poses, cells, res = gpu.seed_poses(one["grids"][0], one["headings"], one["M"], spec, noise)
        twin = abi.seed_poses_host(one["grids"][0], one["headings"], one["M"], spec, noise)
        want_ = sc.want(one)
        assert poses.view(np.uint32).tobytes() == twin[0].view(np.uint32).tobytes() == want_[0][0].tobytes()
        assert cells.tobytes() == twin[1].tobytes() == want_[1][0].tobytes()
        assert res.tobytes() == twin[2].tobytes() == want_[2][0].tobytes()
    lib = abi.load_library()
    grid = np.zeros(15, np.int8)
    head = sc.table(4)
    poses = np.full(24, 7.0, F32)
    cells = np.full(6, GUARD_WORD, np.uint32)
    res = np.full(12, GUARD_WORD, np.uint32)
    good, noise = sc.spec_of(sc.grid_spec(5, 3)), abi.MotionNoise.defaults(seed=4)

    def door(spec=good, grid_=grid.ctypes.data, head_=head.ctypes.data, H=4, M=2, noise_=noise,
             poses_=poses.ctypes.data, cells_=cells.ctypes.data, res_=res.ctypes.data, h=gpu._h):
        return lib.rplgpu_seed_poses(h, C.byref(spec) if spec is not None else None, grid_, head_, H, M,
                                     C.byref(noise_) if noise_ is not None else None, poses_, cells_, res_)

    bad = abi.ERR_INVALID_ARG
    assert door(spec=None) == bad and door(spec=sc.spec_of(sc.grid_spec(5, 3, free_lo=1))) == bad
    assert door(grid_=0) == bad and door(head_=0) == bad and door(noise_=None) == bad and door(poses_=0) == bad
    assert door(res_=0) == bad and door(h=None) == bad and door(M=0) == bad and door(M=abi.MAX_POSES + 1) == bad
    assert door(H=0) == bad and door(H=65537) == bad
    assert (poses == 7.0).all() and (cells == GUARD_WORD).all() and (res == GUARD_WORD).all()
    want_ = so.seed(grid, sc.grid_spec(5, 3), head, 2, dict(seed=4, step=0, first=0))
    assert door() == abi.OK and poses[:8].view(np.uint32).tobytes() == want_[0].tobytes()
    assert cells[:2].tobytes() == want_[1].tobytes() and res[:8].tobytes() == want_[2].tobytes()
    assert (poses[8:] == 7.0).all() and (cells[2:] == GUARD_WORD).all() and (res[8:] == GUARD_WORD).all()
    assert door(cells_=0) == abi.OK


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu):
    import torch
    case = sc.groups_case(1)
    b = _buffers(case)
    M = b["M"]
    n = case["spec"]["width"] * case["spec"]["height"]
    host = np.zeros(64, np.uint32)
    hp = host.ctypes.data + (-host.ctypes.data % 16)

    def call(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            _call(gpu, b, **kw)
        return e.value.code

    bad = abi.ERR_INVALID_ARG
    s = case["spec"]
    for field, value in (("origin_x", float("nan")), ("resolution", 0.0), ("width", 0), ("height", 4097),
                         ("free_lo", -129), ("free_hi", 128), ("free_lo", 1), ("flags", 2)):   # the spec check
        assert call(spec=sc.spec_of(dict(s, **{field: value}))) == bad, field
    assert call(G=0) == bad and call(G=65536) == bad
    assert call(M=0) == bad and call(M=abi.MAX_POSES + 1, ostride=1 << 23, cstride=1 << 21) == bad
    assert call(H=0) == bad and call(H=65537) == bad
    for k in ("grid", "head", "out", "res", "scr"):                       # required pointers
        assert call(**{k: 0}) == bad, k
    names = dict(grid="d_g", head="d_t", out="d_out", cells="d_cells", res="d_res", scr="d_scr")
    for k, step in (("grid", 1), ("grid", 2), ("head", 4), ("out", 4), ("out", 8), ("cells", 2), ("res", 1),
                    ("res", 2), ("scr", 4)):                              # alignment
        assert call(**{k: b[names[k]].data_ptr() + step}) == bad, (k, step)
    assert call(gstride=((n + 3) & ~3) - 4) == bad and call(gstride=b["gstride"] + 2) == bad and call(gstride=0) == bad
    assert call(ostride=4 * M - 4) == bad and call(ostride=4 * M + 2) == bad and call(ostride=0) == bad
    assert call(cstride=M - 1) == bad
    for k in ("grid", "head", "out", "cells", "res", "scr"):              # plain host memory, pointer by pointer
        assert call(**{k: hp}) == bad, k
    lib = abi.load_library()

    def raw(h=gpu._h, spec=b["spec"], noise=b["noise"]):
        return lib.rplgpu_seed_poses_dev(h, C.byref(spec) if spec is not None else None, b["d_g"].data_ptr(),
                                         b["gstride"], 1, b["d_t"].data_ptr(), b["H"], b["G"], M,
                                         C.byref(noise) if noise is not None else None, b["d_out"].data_ptr(),
                                         b["ostride"], b["d_cells"].data_ptr(), b["cstride"], b["d_res"].data_ptr(),
                                         b["d_scr"].data_ptr())

    assert raw(h=None) == bad and raw(spec=None) == bad and raw(noise=None) == bad
    gpu.synchronize()
    torch.cuda.synchronize()
    _outputs_untouched(b)
    assert (_u32(b["d_scr"]) == GUARD_WORD).all()                         # nothing was queued
    _inputs_unchanged(b)
    _check(_run(gpu, case), sc.want(case, "groups1"))                     # then a good call on the case
    # result and cell pointers that are only 4-byte aligned are allowed; a cell_stride below M without d_cells_out too
    b2 = _buffers(case)
    _call(gpu, b2, res=b2["d_res"].data_ptr() + 4, cells=0, cstride=0)
    gpu.synchronize()
    res = _u32(b2["d_res"])
    assert res[0] == GUARD_WORD and res[1 + 8 * b2["G"]:].tolist() == [GUARD_WORD] * 7
    assert res[1:1 + 8 * b2["G"]].tobytes() == sc.want(case, "groups1")[2].tobytes()
    assert (_u32(b2["d_cells"]) == GUARD_WORD).all()
