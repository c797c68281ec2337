"""E20 on the device: rplgpu_bin_poses_dev against tests/bins_oracle.py byte for byte — the bit map, the bin ids and the
eight result words of every group, the guard words behind every group's map, bin ids and result words, and the
unchanged poses, weights and edge table.  The inputs and their regime checks live in tests/bins_cases.py."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import bins_cases as bc
from tests import bins_oracle as bo
from tests import motion_cases as mc
from tests import resample_oracle as ro
from tests import seed_cases as sc
from tests import seed_oracle as so

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD_WORD = 0x5A5A5A5A
PAD = 5                                # guard entries behind every group's list
NONE = bo.NONE


def spec_of(s):
    return abi.PoseBins(s.origin_x, s.origin_y, s.inv_size, s.nx, s.ny, s.keep)


def _up(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda:0"))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _full(k):
    import torch
    return torch.full((k,), GUARD_WORD, dtype=torch.int32, device=torch.device("cuda:0"))


def _buffers(case, pad=PAD, bins=True, map_pad=2):
    """Device copies of a case's lists (each followed by guard poses), weights and edge table (followed by two guard
    entries), the guarded maps (under KEEP: the case's maps, guards behind them), bin ids and result words."""
    s, G = case["spec"], bc.groups(case)
    L, P, T = len(case["lists"]), len(case["lists"][0]), len(case["edges"])
    words = bo.map_words(s, T)
    mstride = words + (words & 1) + map_pad
    h_p = np.full((L, P + pad, 4), 123.0, F32)
    for g in range(L):
        h_p[g, :P] = case["lists"][g]
    h_w = None
    if any(w is not None for w in case["weights"]):
        h_w = np.full((G, P + pad), 3, np.uint32)                  # (no weights for one group of several: all count)
        for g in range(G):
            if case["weights"][g] is not None:
                h_w[g, :P] = case["weights"][g]
    h_e = np.full((T + 2, 2), 123.0, F32)
    h_e[:T] = case["edges"]
    h_m = np.full((G, mstride), GUARD_WORD, np.uint32)
    if s.keep:
        for g in range(G):
            h_m[g, :words] = case["maps"][g]
    b = dict(G=G, P=P, T=T, L=L, words=words, spec=spec_of(s), h_p=h_p, d_p=_up(h_p.view(np.uint32)),
             pstride=4 * (P + pad), ppg=1 if L > 1 else 0, h_w=h_w, d_w=_up(h_w) if h_w is not None else None,
             wstride=P + pad, h_e=h_e, d_e=_up(h_e.view(np.uint32)), d_m=_up(h_m), mstride=mstride,
             d_b=_full(G * (P + pad)) if bins else None, bstride=P + pad, d_r=_full(8 * G + 8))
    return b


def _call(gpu, b, **kw):
    a = dict(spec=b["spec"], poses=b["d_p"].data_ptr(), pstride=b["pstride"], ppg=b["ppg"],
             w=b["d_w"].data_ptr() if b["d_w"] is not None else 0, wstride=b["wstride"], G=b["G"], P=b["P"],
             edges=b["d_e"].data_ptr(), T=b["T"], map=b["d_m"].data_ptr(), mstride=b["mstride"],
             bins=b["d_b"].data_ptr() if b["d_b"] is not None else 0, bstride=b["bstride"], res=b["d_r"].data_ptr())
    a.update(kw)
    gpu.bin_poses_dev(a["spec"], a["poses"], a["pstride"], a["ppg"], a["w"], a["wstride"], a["G"], a["P"], a["edges"],
                      a["T"], a["map"], a["mstride"], a["bins"], a["bstride"], a["res"])


def _inputs_unchanged(b):
    assert _u32(b["d_p"]).tobytes() == b["h_p"].tobytes()
    assert _u32(b["d_e"]).tobytes() == b["h_e"].tobytes()
    if b["d_w"] is not None:
        assert _u32(b["d_w"]).tobytes() == b["h_w"].tobytes()


def _read(b):
    G, P, words = b["G"], b["P"], b["words"]
    _inputs_unchanged(b)
    res = _u32(b["d_r"])
    assert (res[8 * G:] == GUARD_WORD).all()
    m = _u32(b["d_m"]).reshape(G, b["mstride"])
    assert (m[:, words:] == GUARD_WORD).all()                      # (the padding word of an odd count among them)
    bins = None
    if b["d_b"] is not None:
        bins = _u32(b["d_b"]).reshape(G, b["bstride"])
        assert (bins[:, P:] == GUARD_WORD).all()
        bins = bins[:, :P]
    return m[:, :words], bins, res[:8 * G].reshape(G, 8)


def _run(gpu, case, **kw):
    b = _buffers(case, **kw)
    _call(gpu, b)
    gpu.synchronize()
    return _read(b)


def _check(got, want_):
    m, bins, res = got
    assert len(res) == len(want_)
    for g, (wm, wb, wr) in enumerate(want_):
        print(f"group {g}: result {res[g].tolist()} want {wr.tolist()}")
        if bins is not None and bins[g].tobytes() != wb.tobytes():
            bad = np.flatnonzero(bins[g] != wb)
            print(f"group {g}: {len(bad)} of {len(wb)} bin ids differ, first {int(bad[0])}: {int(bins[g][bad[0]])} "
                  f"want {int(wb[bad[0]])}")
        if m[g].tobytes() != wm.tobytes():
            bad = np.flatnonzero(m[g] != wm)
            print(f"group {g}: {len(bad)} of {len(wm)} map words differ, first {int(bad[0])}: {int(m[g][bad[0]]):08x} "
                  f"want {int(wm[bad[0]]):08x}")
        assert bins is None or bins[g].tobytes() == wb.tobytes(), g
        assert m[g].tobytes() == wm.tobytes(), g
        assert res[g].tobytes() == wr.tobytes(), g


# ---- P, NB --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", bc.EDGE_P)
def test_tile_edges(gpu, P):
    case = bc.edge_case(P)
    want_ = bc.want(case, f"edge{P}")
    bc.edge_regime(case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("NB", bc.NB_SIZES)
def test_map_sizes(gpu, NB):
    case = bc.nb_case(NB)
    want_ = bc.want(case, f"nb{NB}")
    bc.nb_regime(case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("name", ["two_bins", "one_bin", "one_word", "own_bin", "positions", "positions_far", "headings",
                                  "keep", "large"])
def test_cases(gpu, name):
    case = getattr(bc, name + "_case")()
    want_ = bc.want(case, name)
    getattr(bc, name + "_regime")(case, want_)
    _check(_run(gpu, case), want_)


def test_widest_map(gpu):
    case = bc.widest_case()
    want_ = bc.want(case, "widest", both=False)
    bc.widest_regime(case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("T", bc.T_SIZES)
def test_heading_tables(gpu, T):
    case = bc.t_case(T)
    want_ = bc.want(case, f"t{T}")
    bc.t_regime(case, want_)
    _check(_run(gpu, case), want_)


def test_table_that_is_not_valid(gpu):
    case = bc.t_case(36, valid=False)
    want_ = bc.want(case, "t36_broken")
    bc.t_regime(case, want_, valid=False)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("kind", ["none", "zero", "mixed"])
def test_weights(gpu, kind):
    case = bc.weights_case(kind)
    want_ = bc.want(case, f"weights_{kind}")
    bc.weights_regime(kind, case, want_)
    _check(_run(gpu, case), want_)


@pytest.mark.parametrize("shared", [0, 1])
def test_groups(gpu, shared):
    case = bc.groups_case(shared)
    want_ = bc.want(case, f"groups{shared}")
    bc.groups_regime(case, want_)
    _check(_run(gpu, case, pad=PAD + 59 * shared, map_pad=2 + 6 * shared), want_)      # strides larger than needed


def test_without_bin_ids(gpu):
    case = bc.groups_case(0)
    got = _run(gpu, case, bins=False)
    assert got[1] is None
    _check(got, bc.want(case, "groups0"))


# ---- KEEP ---------------------------------------------------------------------------------------------------------------
def test_three_pieces_equal_one_call(gpu):
    case = bc.weights_case("mixed")
    want_ = bc.want(case, "weights_mixed")
    b = _buffers(case)
    cuts = [0, 1025, 1026, 1500]
    d_r = _full(3 * 8 + 8)
    for i in range(3):
        lo, n = cuts[i], cuts[i + 1] - cuts[i]
        _call(gpu, b, spec=spec_of(case["spec"]._replace(keep=int(i > 0))), poses=b["d_p"].data_ptr() + 16 * lo,
              w=b["d_w"].data_ptr() + 4 * lo, P=n, bins=b["d_b"].data_ptr() + 4 * lo, res=d_r.data_ptr() + 32 * i)
    gpu.synchronize()  # nothing was read until here
    m, bins, _ = _read(b)
    r = _u32(d_r)
    assert (r[24:] == GUARD_WORD).all() and (_u32(b["d_r"]) == GUARD_WORD).all()
    r = r[:24].reshape(3, 8)
    wm, wb, wr = want_[0]
    assert m[0].tobytes() == wm.tobytes() and bins[0].tobytes() == wb.tobytes()
    assert int(r[:, 0].sum()) == int(wr[0]) and r[:, 1:4].sum(axis=0).tolist() == wr[1:4].tolist()
    assert r[:, 7].tolist() == [int(r[0, 7]) & 3, 4 | int(r[1, 7]) & 3, 4 | int(r[2, 7]) & 3]
    assert int(r[:, 4].min()) == int(wr[4]) and int(r[:, 5].max()) == int(wr[5])
    for i in range(3):                                             # each piece against the oracle chained on the CPU
        part = slice(cuts[i], cuts[i + 1])
        prev = bo.bin_poses(case["spec"], case["lists"][0][:cuts[i]], case["weights"][0][:cuts[i]], case["edges"])[0] \
            if i else None
        want_i = bo.bin_poses(case["spec"]._replace(keep=int(i > 0)), case["lists"][0][part],
                              case["weights"][0][part], case["edges"], prev)
        assert r[i].tobytes() == want_i[2].tobytes(), i


# ---- chains: each stage against its oracle chained on the CPU, one stream, nothing read in between --------------------------
def test_chain_resample_then_bins_counts_the_distinct_ancestors(gpu):
    """(i) P poses in pairwise distinct bins -> E16 without a delta (copies, bit for bit) -> E20 without weights: K is
    E16's count of distinct ancestors"""
    import torch
    rng = np.random.default_rng(61)
    s, T, P = bo.spec(-8.0, -8.0, 2.0, 32, 32), 4, 3000
    poses = bc.centres(s, T, rng.permutation(32 * 32 * T)[:P], rng)
    w = (rng.integers(0, 4, P) * rng.integers(1, 1000, P)).astype(np.uint32)
    u = 0x1234567
    out, anc, r16 = ro.resample(w, poses, P, u)
    want_ = bo.bin_poses(s, out, None, bo.table(T))
    assert len(set(bo.bin_poses(s, poses, None, bo.table(T))[1].tolist())) == P       # the regime: distinct bins
    assert int(want_[2][0]) == int(r16[6]) == len(np.unique(anc)) and 100 < int(r16[6]) < P
    d_p, d_w, d_u, d_e = _up(poses.view(np.uint32)), _up(w), _up(np.array([u], np.uint32)), _up(bo.table(T).view(np.uint32))
    d_out, d_r16, d_r20 = _full(4 * (P + PAD)), _full(16), _full(16)
    words = bo.map_words(s, T)
    d_m, d_b = _full(words + 2), _full(P + PAD)
    d_scr = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=torch.device("cuda:0"))
    gpu.resample_poses_dev(d_w.data_ptr(), P, d_p.data_ptr(), 4 * P, 0, 1, P, P, d_u.data_ptr(), 0, 0, 0, 0,
                           d_out.data_ptr(), 4 * (P + PAD), 0, 0, d_r16.data_ptr(), d_scr.data_ptr())
    gpu.bin_poses_dev(spec_of(s), d_out.data_ptr(), 4 * (P + PAD), 0, 0, 0, 1, P, d_e.data_ptr(), T, d_m.data_ptr(),
                      words + 2, d_b.data_ptr(), P + PAD, d_r20.data_ptr())
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_out, 4 * P), (d_r16, 8), (d_r20, 8), (d_m, words), (d_b, P)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert _u32(d_out)[:4 * P].tobytes() == out.view(np.uint32).tobytes() and _u32(d_r16)[:8].tobytes() == r16.tobytes()
    assert _u32(d_m)[:words].tobytes() == want_[0].tobytes() and _u32(d_b)[:P].tobytes() == want_[1].tobytes()
    assert _u32(d_r20)[:8].tobytes() == want_[2].tobytes() and _u32(d_r20)[0] == _u32(d_r16)[6]


def _score_setup(case):
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


def score_chain(oracle):
    """(ii)'s inputs and the oracles' answers: E15's layout list with every third pose carried 5 m off the field (no
    point of it meets a cell of the field: weight 0), bins of 0.5 m that hold the whole list"""
    P = sc.CHAIN_P
    case = sc.pc.layout_case(P)
    s = case["spec"]
    poses = np.array(case["poses"][0], F32).reshape(P, 4)
    poses[::3, 2] += F32(5.0)
    x, y = sc.pc.case_points(oracle, case, 0)
    w, r15, _ = sc.po.score_points(x, y, poses, s, sc.pc.case_field(case, 0), sc.po.weight_bincount)
    bs = bo.spec(-4.0, -4.0, 2.0, 32, 24)
    T = 36
    want_ = bo.bin_poses(bs, poses, w, bo.table(T))
    # the regime: the list is wholly in range, E15 gave some poses the weight 0 and not all, and E20 skips exactly those
    assert int(want_[2][2]) == 0 and P > int(r15[3]) >= (P + 2) // 3 and int(want_[2][3]) == int(r15[3])
    assert int(want_[2][0]) > 4 and (want_[1][w == 0] == NONE).all() and (want_[1][w != 0] != NONE).all()
    return dict(case=case, poses=poses, w=w, r15=r15, bs=bs, T=T, want=want_)


def test_chain_score_then_bins_skips_the_dead_poses(gpu, oracle):
    """(ii) score (E15) -> E20 with E15's weights on a list wholly in range: the skipped poses are E15's poses of
    weight 0"""
    a = score_chain(oracle)
    P, T, bs, want_ = sc.CHAIN_P, a["T"], a["bs"], a["want"]
    d = _score_setup(a["case"])
    h_p = np.full((P + PAD, 4), 123.0, F32)
    h_p[:P] = a["poses"]
    d_p, d_e = _up(h_p.view(np.uint32)), _up(bo.table(T).view(np.uint32))
    d_w, d_b, d_r15, d_r20 = _full(P + PAD), _full(P + PAD), _full(16), _full(16)
    words = bo.map_words(bs, T)
    d_m = _full(words + (words & 1) + 2)
    _score(gpu, d, d_p.data_ptr(), P, 4 * (P + PAD), d_w, d_r15)
    gpu.bin_poses_dev(spec_of(bs), d_p.data_ptr(), 4 * (P + PAD), 0, d_w.data_ptr(), P + PAD, 1, P, d_e.data_ptr(), T,
                      d_m.data_ptr(), words + (words & 1), d_b.data_ptr(), P + PAD, d_r20.data_ptr())
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_w, P), (d_b, P), (d_r15, 8), (d_r20, 8), (d_m, words)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert _u32(d_p).tobytes() == h_p.tobytes()
    assert _u32(d_w)[:P].tobytes() == a["w"].tobytes() and _u32(d_r15)[:8].tobytes() == a["r15"].tobytes()
    assert _u32(d_m)[:words].tobytes() == want_[0].tobytes() and _u32(d_b)[:P].tobytes() == want_[1].tobytes()
    assert _u32(d_r20)[:8].tobytes() == want_[2].tobytes() and _u32(d_r20)[3] == _u32(d_r15)[3]


def test_chain_seed_then_bins_counts_the_cell_heading_pairs(gpu):
    """(iii) E19 with cell centres on a grid of resolution 0.5 at origin 0 and 36 headings -> E20 with the same table
    as edges and the cells as bins: a pose's bin is (heading, cell), K the number of distinct pairs"""
    W, Hh, H, M = 13, 9, 36, 3000
    rng = np.random.default_rng(62)
    grid = rng.choice(np.array([0, 100], np.int8), W * Hh)
    sspec = dict(so.DEFAULT, origin_x=0.0, origin_y=0.0, resolution=0.5, width=W, height=Hh, flags=1)
    noise = dict(seed=77, step=3, first=0)
    table = sc.table(H)
    words_, cells, r19 = so.seed(grid, sspec, table, M, noise)
    poses = np.ascontiguousarray(words_).view(F32).reshape(M, 4)
    index = {tuple(e.view(np.uint32).tolist()): k for k, e in enumerate(table)}
    heading = np.array([index[tuple(v)] for v in np.ascontiguousarray(words_).reshape(M, 4)[:, :2].tolist()])
    pairs = heading * (W * Hh) + cells.astype(np.int64)
    bs = bo.spec(0.0, 0.0, 2.0, W, Hh)
    want_ = bo.bin_poses(bs, poses, None, table)
    assert len(index) == H and want_[1].tolist() == pairs.tolist()                     # the regime: bins = cells
    assert int(want_[2][0]) == len(set(pairs.tolist())) > 500 and int(want_[2][1]) == M
    gstride = (W * Hh + 3) & ~3
    h_grid = np.full(gstride, 100, np.int8)
    h_grid[:W * Hh] = grid
    d_grid, d_table = _up(h_grid), _up(table.view(np.uint32))
    d_out, d_cells, d_b = _full(4 * (M + PAD)), _full(M + PAD), _full(M + PAD)
    d_r19, d_r20 = _full(16), _full(16)
    d_scr = _full(abi.seed_scratch_words(1, W, Hh))
    nw = bo.map_words(bs, H)
    d_m = _full(nw + (nw & 1) + 2)
    gpu.seed_poses_dev(sc.spec_of(sspec), d_grid.data_ptr(), gstride, 0, d_table.data_ptr(), H, 1, M,
                       sc.noise_of(noise), d_out.data_ptr(), 4 * (M + PAD), d_cells.data_ptr(), M + PAD,
                       d_r19.data_ptr(), d_scr.data_ptr())
    gpu.bin_poses_dev(spec_of(bs), d_out.data_ptr(), 4 * (M + PAD), 0, 0, 0, 1, M, d_table.data_ptr(), H,
                      d_m.data_ptr(), nw + (nw & 1), d_b.data_ptr(), M + PAD, d_r20.data_ptr())
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_out, 4 * M), (d_cells, M), (d_b, M), (d_r19, 8), (d_r20, 8), (d_m, nw)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert _u32(d_out)[:4 * M].tobytes() == words_.tobytes() and _u32(d_cells)[:M].tobytes() == cells.tobytes()
    assert _u32(d_r19)[:8].tobytes() == r19.tobytes()
    assert _u32(d_m)[:nw].tobytes() == want_[0].tobytes() and _u32(d_b)[:M].tobytes() == want_[1].tobytes()
    assert _u32(d_r20)[:8].tobytes() == want_[2].tobytes()


def test_chain_sample_resample_bins_score(gpu, oracle):
    """(iv) sample (E18) -> resample and move (E16) -> bin (E20) -> score (E15): the bins of the moved list, counted
    between the move and the next sensor update"""
    import torch
    c = sc.inject_chain(oracle)
    P = M = sc.CHAIN_P
    d = _score_setup(c["case"])
    s = c["case"]["spec"]
    moved, _, r16 = ro.resample(c["w1"], c["poses"], M, c["u"], mc.floats_of(c["d_words"])[0])
    moved = np.ascontiguousarray(moved)
    T = 36
    bs = bo.spec(-4.0, -4.0, 2.0, 32, 24)
    want_ = bo.bin_poses(bs, moved, None, bo.table(T))
    x, y = sc.pc.case_points(oracle, c["case"], 0)
    w2, r15, _ = sc.po.score_points(x, y, moved, s, sc.pc.case_field(c["case"], 0), sc.po.weight_bincount)
    assert r16.tobytes() == c["r16"].tobytes() and 3 < int(want_[2][0]) < M and int(want_[2][1]) > M // 2   # the regime
    d_poses, d_w1, d_u, d_odom = _up(c["poses"]), _up(c["w1"]), _up(np.array([c["u"]], np.uint32)), _up(c["odom"])
    d_e = _up(bo.table(T).view(np.uint32))
    d_delta, d_out, d_w2, d_b = _full(4 * (M + PAD)), _full(4 * (M + PAD)), _full(M + PAD), _full(M + PAD)
    d_r18, d_r16, d_r20, d_r15 = _full(16), _full(16), _full(16), _full(16)
    d_scr16 = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=torch.device("cuda:0"))
    nw = bo.map_words(bs, T)
    d_m = _full(nw + (nw & 1) + 2)
    gpu.sample_motion_dev(d_odom.data_ptr(), 0, 1, M, mc.spec_of(c["noise"]), d_delta.data_ptr(), 4 * (M + PAD),
                          d_r18.data_ptr())
    gpu.resample_poses_dev(d_w1.data_ptr(), P, d_poses.data_ptr(), 4 * P, 0, 1, P, M, d_u.data_ptr(),
                           d_delta.data_ptr(), M, 4 * (M + PAD), 1, d_out.data_ptr(), 4 * (M + PAD), 0, 0,
                           d_r16.data_ptr(), d_scr16.data_ptr())
    gpu.bin_poses_dev(spec_of(bs), d_out.data_ptr(), 4 * (M + PAD), 0, 0, 0, 1, M, d_e.data_ptr(), T, d_m.data_ptr(),
                      nw + (nw & 1), d_b.data_ptr(), M + PAD, d_r20.data_ptr())
    _score(gpu, d, d_out.data_ptr(), M, 4 * (M + PAD), d_w2, d_r15)
    gpu.synchronize()  # nothing was read until here
    for t, k in ((d_delta, 4 * M), (d_out, 4 * M), (d_w2, M), (d_b, M), (d_r18, 8), (d_r16, 8), (d_r20, 8), (d_r15, 8),
                 (d_m, nw)):
        assert (_u32(t)[k:] == GUARD_WORD).all()
    assert _u32(d_delta)[:4 * M].tobytes() == c["d_words"][0].tobytes()
    assert _u32(d_r18)[:8].tobytes() == c["r18"][0].tobytes() and _u32(d_r16)[:8].tobytes() == r16.tobytes()
    assert _u32(d_out)[:4 * M].tobytes() == moved.view(np.uint32).tobytes()
    assert _u32(d_m)[:nw].tobytes() == want_[0].tobytes() and _u32(d_b)[:M].tobytes() == want_[1].tobytes()
    assert _u32(d_r20)[:8].tobytes() == want_[2].tobytes()
    assert _u32(d_w2)[:M].tobytes() == w2.tobytes() and _u32(d_r15)[:8].tobytes() == r15.tobytes()
    assert abi.kld_samples(int(_u32(d_r20)[0])) >= 500                      # what the host would pass to E16 as M


# ---- the door, refusals -------------------------------------------------------------------------------------------------
def test_host_buffers_one_group(gpu):
    for name, case in (("positions", bc.positions_case()), ("headings", bc.headings_case()), ("keep", bc.keep_case()),
                       ("weights_mixed", bc.weights_case("mixed")), ("nb33", bc.nb_case(33))):
        wm, wb, wr = bc.want(case, name)[0]
        got = gpu.bin_poses(case["lists"][0], case["edges"], case["weights"][0], spec_of(case["spec"]),
                            case["maps"][0] if case.get("maps") else None)
        twin = abi.bin_poses_host(case["lists"][0], case["edges"], case["weights"][0], spec_of(case["spec"]),
                                  case["maps"][0] if case.get("maps") else None)
        for k, w in enumerate((wm, wb, wr)):
            assert got[k].tobytes() == twin[k].tobytes() == w.tobytes(), (name, k)
    lib = abi.load_library()
    case = bc.nb_case(33)
    s, poses, edges = spec_of(case["spec"]), case["lists"][0], case["edges"]
    m = np.full(3, GUARD_WORD, np.uint32)
    bins = np.full(len(poses) + 1, GUARD_WORD, np.uint32)
    res = np.full(9, GUARD_WORD, np.uint32)
    bad_spec = spec_of(case["spec"]._replace(nx=0))

    def door(h=gpu._h, spec=s, poses_=poses.ctypes.data, P=len(poses), edges_=edges.ctypes.data, T=1, m_=m.ctypes.data,
             bins_=bins.ctypes.data, res_=res.ctypes.data):
        return lib.rplgpu_bin_poses(h, C.byref(spec) if spec is not None else None, poses_, P, None, edges_, T, m_,
                                    bins_, res_)

    bad = abi.ERR_INVALID_ARG
    assert door(h=None) == bad and door(spec=None) == bad and door(spec=bad_spec) == bad and door(poses_=0) == bad
    assert door(P=0) == bad and door(P=abi.MAX_POSES + 1) == bad and door(edges_=0) == bad and door(T=0) == bad
    assert door(T=1025) == bad and door(m_=0) == bad and door(res_=0) == bad
    assert (m == GUARD_WORD).all() and (bins == GUARD_WORD).all() and (res == GUARD_WORD).all()
    wm, wb, wr = bc.want(case, "nb33")[0]
    assert door() == abi.OK and m[:2].tobytes() == wm.tobytes() and bins[:-1].tobytes() == wb.tobytes()
    assert res[:8].tobytes() == wr.tobytes() and m[2] == bins[-1] == res[8] == GUARD_WORD
    assert door(bins_=0) == abi.OK


def test_bad_arguments_leave_outputs_and_a_working_handle(gpu):
    import torch
    case = bc.groups_case(0)
    b = _buffers(case)
    P, words = b["P"], b["words"]
    host = np.zeros(64, np.uint32)
    hp = host.ctypes.data + (-host.ctypes.data % 16)
    refused = []

    def call(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            _call(gpu, b, **kw)
        refused.append(kw)
        return e.value.code

    bad = abi.ERR_INVALID_ARG
    s = case["spec"]
    for field, value in (("origin_x", float("nan")), ("origin_y", float("inf")), ("inv_size", 0.0), ("inv_size", -1.0),
                         ("nx", 0), ("ny", 65537), ("keep", 2)):           # the spec check
        assert call(spec=spec_of(s._replace(**{field: value}))) == bad, field
    assert call(T=0) == bad and call(T=1025) == bad
    assert call(spec=spec_of(s._replace(nx=65536, ny=1025)), T=1) == bad   # above RPLGPU_MAX_POSE_BINS
    assert call(G=0) == bad and call(G=65536) == bad
    assert call(P=0) == bad and call(P=abi.MAX_POSES + 1, pstride=1 << 23, wstride=1 << 21, bstride=1 << 21) == bad
    for k in ("poses", "edges", "map", "res"):                             # required pointers
        assert call(**{k: 0}) == bad, k
    names = dict(poses="d_p", w="d_w", edges="d_e", map="d_m", bins="d_b", res="d_r")
    for k, step in (("poses", 4), ("poses", 8), ("w", 2), ("edges", 4), ("map", 4), ("bins", 1), ("bins", 2),
                    ("res", 1), ("res", 2)):                               # alignment
        assert call(**{k: b[names[k]].data_ptr() + step}) == bad, (k, step)
    assert call(pstride=4 * P - 4) == bad and call(pstride=4 * P + 2) == bad and call(pstride=0) == bad
    assert call(wstride=P - 1) == bad and call(bstride=P - 1) == bad
    assert call(mstride=words + (words & 1) - 2) == bad and call(mstride=b["mstride"] + 1) == bad and call(mstride=0) == bad
    for k in ("poses", "w", "edges", "map", "bins", "res"):                # plain host memory, pointer by pointer
        assert call(**{k: hp}) == bad, k
    lib = abi.load_library()
    assert lib.rplgpu_bin_poses_dev(None, C.byref(b["spec"]), b["d_p"].data_ptr(), b["pstride"], 1, 0, 0, b["G"], P,
                                    b["d_e"].data_ptr(), b["T"], b["d_m"].data_ptr(), b["mstride"], 0, 0,
                                    b["d_r"].data_ptr()) == bad
    assert lib.rplgpu_bin_poses_dev(gpu._h, None, b["d_p"].data_ptr(), b["pstride"], 1, 0, 0, b["G"], P,
                                    b["d_e"].data_ptr(), b["T"], b["d_m"].data_ptr(), b["mstride"], 0, 0,
                                    b["d_r"].data_ptr()) == bad
    assert len(refused) >= 30
    gpu.synchronize()
    torch.cuda.synchronize()
    for k in ("d_m", "d_b", "d_r"):                                        # nothing was queued
        assert (_u32(b[k]) == GUARD_WORD).all(), k
    _inputs_unchanged(b)
    _check(_run(gpu, case), bc.want(case, "groups0"))                      # then a good call on the case
    # result, weight and bin pointers that are only 4-byte aligned are allowed; a bin_stride below P without d_bins_out
    b2 = _buffers(case)
    _call(gpu, b2, res=b2["d_r"].data_ptr() + 4, bins=0, bstride=0)
    gpu.synchronize()
    res = _u32(b2["d_r"])
    want_ = bc.want(case, "groups0")
    assert res[0] == GUARD_WORD and res[1 + 8 * b2["G"]:].tolist() == [GUARD_WORD] * 7
    assert res[1:1 + 8 * b2["G"]].tobytes() == b"".join(w[2].tobytes() for w in want_)
    assert (_u32(b2["d_b"]) == GUARD_WORD).all()
