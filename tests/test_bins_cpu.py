"""E20 without a device: the new symbols, the struct's layout and the defaults; one refusal per clause of both checks;
rplgpu_heading_edges_check on valid and on broken tables; rplgpu_kld_samples' known answers; rplgpu_bin_poses_host
(the rule in plain C++) against both writers of tests/bins_oracle.py on every case of tests/bins_cases.py and on
random inputs; the two forms of the heading bin; a list counted in pieces under KEEP; and the refusals of the host
functions."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import bins_cases as bc
from tests import bins_oracle as bo

F32 = np.float32
NONE = bo.NONE


def spec_of(s):
    return abi.PoseBins(s.origin_x, s.origin_y, s.inv_size, s.nx, s.ny, s.keep)


def _host(case, g):
    poses = case["lists"][g if len(case["lists"]) > 1 else 0]
    m = case["maps"][g] if case.get("maps") else None
    return abi.bin_poses_host(poses, case["edges"], case["weights"][g], spec_of(case["spec"]), m)


def _against_oracle(case, name, both=None):
    w = bc.want(case, name, both=both)
    for g in range(bc.groups(case)):
        got = _host(case, g)
        for k in (2, 1, 0):
            assert got[k].dtype == np.uint32 and got[k].tobytes() == w[g][k].tobytes(), (name, g, k, got[2], w[g][2])
        assert int(got[2][1]) + int(got[2][2]) + int(got[2][3]) == len(got[1])       # words 1 + 2 + 3 = P
    return w


# ---- symbols, the struct, the defaults ----------------------------------------------------------------------------------
def test_symbols_struct_and_defaults():
    s = abi.PoseBins.defaults()
    lib = abi.load_library()
    for name in ("rplgpu_default_pose_bins", "rplgpu_pose_bins_check", "rplgpu_bin_map_words",
                 "rplgpu_heading_edges_check", "rplgpu_bin_poses_dev", "rplgpu_bin_poses_host", "rplgpu_bin_poses",
                 "rplgpu_kld_samples"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    for fn in ("bin_poses_dev", "bin_poses"):
        assert callable(getattr(abi.RplGpu, fn))
    assert (s.origin_x, s.origin_y, s.inv_size) == (F32(-25.6), F32(-25.6), F32(2.0))
    assert (s.nx, s.ny, s.flags) == (103, 103, 0)
    d = bo.spec()
    assert (s.origin_x, s.origin_y, s.inv_size, s.nx, s.ny, s.flags) == tuple(d)
    assert s.origin_x + s.nx / s.inv_size >= 25.6                   # E11's default grid (1024 cells of 0.05 m) is inside
    assert C.sizeof(abi.PoseBins) == 24
    assert [getattr(abi.PoseBins, f).offset for f, _ in abi.PoseBins._fields_] == [0, 4, 8, 12, 16, 20]
    assert s.check(36) == abi.OK and s.check(1) == abi.OK and s.check(1024) == abi.OK
    assert abi.MAX_POSE_BINS == 1 << 26 and abi.MAX_HEADING_BINS == 1024
    lib.rplgpu_default_pose_bins(None)                              # (ignored)
    assert lib.rplgpu_abi_version() == 1


@pytest.mark.parametrize("field,value,T", [
    ("origin_x", math.nan, 36), ("origin_y", math.inf, 36), ("inv_size", math.nan, 36), ("inv_size", -math.inf, 36),
    ("inv_size", math.inf, 36), ("inv_size", 0.0, 36), ("inv_size", -2.0, 36), ("nx", 0, 1), ("ny", 0, 1),
    ("nx", 65537, 1), ("ny", 65537, 1), ("nx", 103, 0), ("nx", 103, 1025), ("flags", 2, 36), ("flags", 3, 36),
])
def test_check_refuses(field, value, T):
    s = abi.PoseBins.defaults(nx=1, ny=1) if field in ("nx", "ny") and value > 65536 else abi.PoseBins.defaults()
    setattr(s, field, value)
    assert s.check(T) == abi.ERR_INVALID_ARG
    assert abi.load_library().rplgpu_pose_bins_check(None, 36) == abi.ERR_INVALID_ARG


def test_check_bin_limit_and_map_words():
    ok = [(65536, 1024, 1), (1, 65536, 1024), (256, 256, 1024), (8192, 8192, 1), (1, 1, 1)]
    for nx, ny, T in ok:
        assert abi.PoseBins.defaults(nx=nx, ny=ny).check(T) == abi.OK, (nx, ny, T)
        words = (nx * ny * T + 31) // 32
        assert abi.bin_map_words(nx, ny, T) == words + (words & 1)
    for nx, ny, T in [(65536, 1025, 1), (8192, 8193, 1), (256, 257, 1024), (65536, 65536, 1), (65536, 65536, 1024)]:
        assert abi.PoseBins.defaults(nx=nx, ny=ny).check(T) == abi.ERR_INVALID_ARG, (nx, ny, T)
        assert abi.bin_map_words(nx, ny, T) == 0
    assert abi.bin_map_words(0, 1, 1) == abi.bin_map_words(1, 0, 1) == abi.bin_map_words(1, 1, 0) == 0
    assert abi.bin_map_words(1, 1, 1025) == 0 and abi.bin_map_words(65537, 1, 1) == 0
    assert abi.bin_map_words(103, 103, 36) == 11936 and abi.bin_map_words(3, 11, 1) == 2
    assert abi.bin_map_words(33, 1, 1) == 2 and abi.bin_map_words(65, 1, 1) == 4 and abi.bin_map_words(1, 1, 1) == 2


# ---- the heading tables -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 36, 72, 360, 1000, 1024])
def test_library_tables_are_valid_and_the_two_forms_agree(T):
    t = abi.seed_headings(T)
    assert abi.heading_edges_check(t) == abi.OK and bo.valid_table(t)
    assert abi.heading_edges_check(bo.table(T)) == abi.OK and bo.valid_table(bo.table(T))
    rng = np.random.default_rng(T)
    n = 20000 if T in (7, 36, 1024) else 2000
    a = rng.uniform(0, 2 * np.pi, n)
    h = np.concatenate([np.stack([np.cos(a), np.sin(a)], axis=1).astype(F32), t, t * F32(0.5), -t])
    hq, ok = bo.a_quantise(h)
    eq, e_ok = bo.a_quantise(t)
    assert ok.all() and e_ok.all()
    bisected = bo.a_heading_bins(hq, eq, e_ok)
    # (the number of edges <= h) - 1, by writer (a)'s order over the whole table at once ...
    counted = np.zeros(len(hq), np.int64)
    for k in range(T):
        counted += bo.a_le(np.broadcast_to(eq[k], hq.shape), np.ones(len(hq), bool), hq)
    assert (bisected == counted - 1).all()
    assert (bisected[n:n + T] == np.arange(T)).all()                # a heading on an edge: the bin that starts there
    # ... and by writer (b)'s order on a part of them
    e = [bo.b_quantise(c, s) for c, s in t]
    for i in list(range(0, n, max(n // 40, 1))) + list(range(n, len(h), max(T // 20, 1))):
        assert sum(1 for q in e if bo.b_le(q, tuple(hq[i].tolist()))) - 1 == bisected[i], i


def test_broken_tables():
    t = abi.seed_headings(36)
    off = t.copy()
    off[0] = t[1]
    swapped = t.copy()
    swapped[[4, 9]] = swapped[[9, 4]]
    repeated = t.copy()
    repeated[12] = repeated[11]
    nan = t.copy()
    nan[20, 1] = np.nan
    almost = t.copy()
    almost[0] = (1.0, 2.0 ** -20)                                   # entry 0 one quantisation step off
    short = t.copy()
    short[0] = (0.5, 0.0)                                           # the right direction, not (2^20, 0)
    zero = t.copy()
    zero[7] = (0.0, 0.0)
    for name, bad in dict(off=off, swapped=swapped, repeated=repeated, nan=nan, almost=almost, short=short,
                          zero=zero).items():
        assert abi.heading_edges_check(bad) == abi.ERR_INVALID_ARG, name
        assert not bo.valid_table(bad), name
    lib = abi.load_library()
    assert lib.rplgpu_heading_edges_check(None, 36) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_heading_edges_check(t.ctypes.data, 0) == abi.ERR_INVALID_ARG
    big = abi.seed_headings(1025)
    assert lib.rplgpu_heading_edges_check(big.ctypes.data, 1025) == abi.ERR_INVALID_ARG


def test_a_valid_table_need_not_close_the_circle():
    big = abi.seed_headings(1025)
    assert abi.heading_edges_check(big[:1024]) == abi.OK and abi.heading_edges_check(big[:1]) == abi.OK


# ---- rplgpu_kld_samples -------------------------------------------------------------------------------------------------
def _kld(k, eps, z):
    b = 2.0 / (9.0 * (k - 1))
    x = 1.0 - b + math.sqrt(b) * z
    return math.ceil((k - 1) / (2.0 * eps) * x * x * x)


def test_kld_samples():
    for k, n in [(2, 527), (10, 1363), (100, 7332), (1000, 56923)]:
        assert abi.kld_samples(k, 0.01, 3.0, 1, 10 ** 9) == n == _kld(k, 0.01, 3.0)
    for k in (0, 1):
        assert abi.kld_samples(k, 0.01, 3.0, 500, 100000) == 100000
    assert abi.kld_samples(2, 0.01, 3.0, 600, 100000) == 600          # clamped from below
    assert abi.kld_samples(2, 0.01, 3.0, 500, 100000) == 527
    assert abi.kld_samples(1000, 0.01, 3.0, 500, 5000) == 5000        # and from above
    assert abi.kld_samples(1 << 26, 0.01, 3.0, 500, 100000) == 100000
    assert _kld(1 << 26, 0.001, 3.0) > 2 ** 32                        # beyond a uint32: the clamp, no wrap
    assert abi.kld_samples(1 << 26, 0.001, 3.0, 500, 2 ** 32 - 1) == 2 ** 32 - 1
    for k in (3, 17, 361, 5000, 381924):
        for eps, z in [(0.01, 3.0), (0.05, 2.326), (0.02, 0.99)]:
            assert abi.kld_samples(k, eps, z, 1, 2 ** 32 - 1) == min(_kld(k, eps, z), 2 ** 32 - 1)
    assert abi.kld_samples(50) == min(max(_kld(50, 0.01, 3.0), 500), 100000)       # AMCL's limits by default


# ---- the host twin against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", bc.EDGE_P)
def test_host_tile_edges(P):
    case = bc.edge_case(P)
    bc.edge_regime(case, _against_oracle(case, f"edge{P}"))


@pytest.mark.parametrize("NB", bc.NB_SIZES)
def test_host_map_sizes(NB):
    case = bc.nb_case(NB)
    bc.nb_regime(case, _against_oracle(case, f"nb{NB}"))


@pytest.mark.parametrize("name", ["two_bins", "one_bin", "one_word", "own_bin", "positions", "positions_far", "headings",
                                  "keep", "large"])
def test_host_cases(name):
    case = getattr(bc, name + "_case")()
    w = bc.want(case, name)
    getattr(bc, name + "_regime")(case, w)
    _against_oracle(case, name)


def test_host_widest_map():
    case = bc.widest_case()
    w = bc.want(case, "widest", both=False)
    bc.widest_regime(case, w)
    _against_oracle(case, "widest", both=False)
    # writer (b) on a part of the list (counting 1024 edges per pose is slow): the same bins
    part = slice(0, 192)
    other = bo.writer_b(case["spec"], case["lists"][0][part], None, case["edges"])
    assert other[1].tobytes() == w[0][1][part].tobytes()


@pytest.mark.parametrize("T", bc.T_SIZES)
def test_host_heading_tables(T):
    case = bc.t_case(T)
    w = bc.want(case, f"t{T}")
    bc.t_regime(case, w)
    _against_oracle(case, f"t{T}")


def test_host_table_that_is_not_valid():
    case = bc.t_case(36, valid=False)
    w = bc.want(case, "t36_broken")
    bc.t_regime(case, w, valid=False)
    assert abi.heading_edges_check(case["edges"]) == abi.ERR_INVALID_ARG
    _against_oracle(case, "t36_broken")
    good = bc.want(bc.t_case(36), "t36")
    assert good[0][1].tobytes() != w[0][1].tobytes()                # the bisection does land elsewhere


@pytest.mark.parametrize("kind", ["none", "zero", "mixed"])
def test_host_weights(kind):
    case = bc.weights_case(kind)
    w = bc.want(case, f"weights_{kind}")
    bc.weights_regime(kind, case, w)
    _against_oracle(case, f"weights_{kind}")


@pytest.mark.parametrize("shared", [0, 1])
def test_host_groups(shared):
    case = bc.groups_case(shared)
    bc.groups_regime(case, _against_oracle(case, f"groups{shared}"))


@pytest.mark.parametrize("seed", range(80))
def test_host_random(seed):
    case = bc.random_case(seed)
    assert len(case["lists"][0]) <= bo.B_LIMIT and bo.valid_table(case["edges"])     # both writers
    _against_oracle(case, f"random{seed}")


def test_random_inputs_reach_every_outcome():
    tot = np.zeros(8, np.int64)
    keeps = 0
    for seed in range(80):
        case = bc.random_case(seed)
        res = bc.want(case, f"random{seed}")[0][2]
        tot += res
        keeps += case["spec"].keep
        if case["spec"].keep:
            occupied = len(set(bc.want(case, f"random{seed}")[0][1].tolist()) - {NONE})
            assert int(res[0]) <= occupied
    assert tot[1] > 3000 and tot[2] > 1000 and tot[3] > 1000 and 20 < keeps < 60


# ---- properties -----------------------------------------------------------------------------------------------------------
def test_pieces_with_keep():
    case = bc.weights_case("mixed")
    s, poses, w, edges = case["spec"], case["lists"][0], case["weights"][0], case["edges"]
    whole = abi.bin_poses_host(poses, edges, w, spec_of(s))
    cuts = [0, 1, 700, 1500]
    m, ks, counts = None, [], np.zeros(3, np.int64)
    bins = []
    for i in range(3):
        part = slice(cuts[i], cuts[i + 1])
        m, b, res = abi.bin_poses_host(poses[part], edges, w[part], spec_of(s._replace(keep=int(i > 0))), m)
        assert int(res[7]) & 4 == (4 if i else 0)
        ks.append(int(res[0]))
        counts += res[1:4]
        bins.append(b)
    assert m.tobytes() == whole[0].tobytes() and sum(ks) == int(whole[2][0]) and ks[2] < int(whole[2][0])
    assert counts.tolist() == whole[2][1:4].tolist() and np.concatenate(bins).tobytes() == whole[1].tobytes()
    # the same list again under KEEP: nothing new, the map as it was
    again = abi.bin_poses_host(poses, edges, w, spec_of(s._replace(keep=1)), whole[0])
    assert int(again[2][0]) == 0 and again[0].tobytes() == whole[0].tobytes()
    assert again[2][1:6].tolist() == whole[2][1:6].tolist()


def test_keep_counts_new_bits_only_and_leaves_the_rest_of_the_map():
    case = bc.keep_case()
    w = bc.want(case, "keep")
    bc.keep_regime(case, w)
    got = _host(case, 0)
    fresh = abi.bin_poses_host(case["lists"][0], case["edges"], None, spec_of(case["spec"]._replace(keep=0)))
    assert int(got[2][0]) < int(fresh[2][0]) and (got[0] == (fresh[0] | case["maps"][0])).all()
    assert int(got[2][0]) == int(np.unpackbits((fresh[0] & ~case["maps"][0]).view(np.uint8)).sum())


def test_host_leaves_words_behind_the_map_and_the_list():
    case = bc.nb_case(33)
    s, poses = spec_of(case["spec"]), case["lists"][0]
    lib = abi.load_library()
    m = np.full(4, 0xDEADBEEF, np.uint32)
    bins = np.full(len(poses) + 2, 0xDEADBEEF, np.uint32)
    res = np.full(10, 0xDEADBEEF, np.uint32)
    assert lib.rplgpu_bin_poses_host(C.byref(s), poses.ctypes.data, len(poses), None, case["edges"].ctypes.data, 1,
                                     m.ctypes.data, bins.ctypes.data, res.ctypes.data) == abi.OK
    assert m[:2].tolist() == [0xFFFFFFFF, 1] and (m[2:] == 0xDEADBEEF).all()
    assert (bins[-2:] == 0xDEADBEEF).all() and (res[8:] == 0xDEADBEEF).all() and int(res[0]) == 33


def test_host_refusals():
    lib = abi.load_library()
    case = bc.nb_case(33)
    s, poses, edges = spec_of(case["spec"]), case["lists"][0], case["edges"]
    m = np.full(2, 0xDEADBEEF, np.uint32)
    res = np.full(8, 0xDEADBEEF, np.uint32)
    bad_spec = spec_of(case["spec"])
    bad_spec.inv_size = 0.0
    P = len(poses)
    args = dict(s=C.byref(s), poses=poses.ctypes.data, P=P, edges=edges.ctypes.data, T=1, m=m.ctypes.data,
                res=res.ctypes.data)
    for change in (dict(s=None), dict(s=C.byref(bad_spec)), dict(poses=None), dict(P=0), dict(P=abi.MAX_POSES + 1),
                   dict(edges=None), dict(T=0), dict(T=1025), dict(m=None), dict(res=None)):
        a = dict(args, **change)
        assert lib.rplgpu_bin_poses_host(a["s"], a["poses"], a["P"], None, a["edges"], a["T"], a["m"], None,
                                         a["res"]) == abi.ERR_INVALID_ARG, change
        assert (m == 0xDEADBEEF).all() and (res == 0xDEADBEEF).all()
    assert lib.rplgpu_bin_poses_host(args["s"], args["poses"], P, None, args["edges"], 1, args["m"], None,
                                     args["res"]) == abi.OK
    assert int(res[0]) == 33
    # the door without a handle
    assert lib.rplgpu_bin_poses(None, C.byref(s), poses.ctypes.data, P, None, edges.ctypes.data, 1, m.ctypes.data, None,
                                res.ctypes.data) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_bin_poses_dev(None, C.byref(s), 16, 4 * P, 0, None, 0, 1, P, 8, 1, 8, 2, None, 0,
                                    4) == abi.ERR_INVALID_ARG
