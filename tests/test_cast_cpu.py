"""E22 without a device: the two oracle writers of tests/cast_oracle.py against each other on every case of
tests/cast_cases.py (each under its regime check), the library's host twin rplgpu_cast_ranges_host against both, the
spec check's table of refusals, known answers worked out by hand, the four identities of the header and the table
index rule at its edges."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import cast_cases as cc
from tests import cast_oracle as co
from tests import pose_oracle as po

F32 = np.float32
GUARD_WORD = 0x5A5A5A5A


def spec_of(s):
    return abi.RangeCast(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["max_steps"],
                         s["hit_lo"], s["unknown_stops"], s["table_half"])


def twin(case, g=0, **kw):
    a = dict(measured=None if case["measured"] is None else case["measured"][g], table=case["table"],
             meas_first=case["first"], meas_step=case["step"])
    a.update(kw)
    return abi.cast_ranges_host(case["lists"][g % len(case["lists"])], case["beams"],
                                case["grids"][g % len(case["grids"])], spec_of(case["spec"]), **a)


def same(got, want_):
    ranges, weights, result, cast = got
    assert ranges.tobytes() == want_["ranges"].tobytes()
    assert cast.tobytes() == want_["cast"].tobytes(), (cast.tolist(), want_["cast"].tolist())
    if want_["weights"] is not None:
        assert weights.tobytes() == want_["weights"].tobytes()
        assert result.tobytes() == want_["result"].tobytes(), (result.tolist(), want_["result"].tolist())
    else:
        assert weights is None and result is None


# ---- the writers, the twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_writers_agree_and_the_twin_with_them(name):
    case = cc.case(name)
    a, b = cc.want(case, name, 1), cc.want(case, name, 2)
    cc.regime(case, b)
    for g in range(case["G"]):
        for k in ("ranges", "steps", "cast", "weights", "result"):
            assert (a[g][k] is None and b[g][k] is None) or a[g][k].tobytes() == b[g][k].tobytes(), (g, k)
        same(twin(case, g), b[g])


def test_twin_ranges_only_and_weights_only():
    case = cc.case("p64")
    w = cc.want(case, "p64")[0]
    r, wt, res, cast = twin(case, measured=None, table=None)
    assert r.tobytes() == w["ranges"].tobytes() and wt is None and res is None and cast.tobytes() == w["cast"].tobytes()
    r, wt, res, cast = twin(case, want_ranges=False)
    assert r is None and wt.tobytes() == w["weights"].tobytes() and res.tobytes() == w["result"].tobytes()
    assert cast.tobytes() == w["cast"].tobytes()


# ---- the spec check, the helpers, the twin's refusals ---------------------------------------------------------------------
REFUSED = [("origin_x", math.nan), ("origin_x", math.inf), ("origin_y", -math.inf), ("origin_y", math.nan),
           ("resolution", math.nan), ("resolution", math.inf), ("resolution", 0.0), ("resolution", -0.05),
           ("width", 0), ("width", 4097), ("height", 0), ("height", 4097), ("max_steps", 0), ("max_steps", 8193),
           ("hit_lo", 0), ("hit_lo", -1), ("hit_lo", 128), ("unknown_stops", 2), ("table_half", 4097)]
ALLOWED = [("width", 4096), ("height", 1), ("max_steps", 1), ("max_steps", 8192), ("hit_lo", 1), ("hit_lo", 127),
           ("unknown_stops", 0), ("table_half", 0), ("table_half", 4096), ("resolution", 1e-6), ("origin_x", 1e30)]


def test_defaults_and_spec_check():
    d = abi.RangeCast.defaults()
    assert {k: getattr(d, k) for k, _ in d._fields_} == {k: (float(F32(v)) if isinstance(v, float) else v)
                                                          for k, v in co.DEFAULT.items()}
    assert d.check() == abi.OK and co.spec_valid(co.DEFAULT)
    assert abi.load_library().rplgpu_range_cast_check(None) == abi.ERR_INVALID_ARG
    for field, value in REFUSED:
        assert abi.RangeCast.defaults(**{field: value}).check() == abi.ERR_INVALID_ARG, (field, value)
        assert not co.spec_valid(co.spec(**{field: value})), (field, value)
    for field, value in ALLOWED:
        assert abi.RangeCast.defaults(**{field: value}).check() == abi.OK, (field, value)
        assert co.spec_valid(co.spec(**{field: value})), (field, value)


def test_cast_beams_are_the_centres_of_the_merged_beams():
    m = abi.ScanMerge(-math.pi, math.pi, 360, 0.1, 30.0, 0.1)
    inc = float(F32((float(F32(math.pi)) - float(F32(-math.pi))) / 360.0))
    got = abi.cast_beams(m, 3, 7, 51)
    k = 3 + 7 * np.arange(51)
    phi = float(F32(-math.pi)) + (k + 0.5) * inc
    assert np.abs(got[:, 0].astype(np.float64) - np.cos(phi)).max() < 1e-7       # (one fp64 rounding of libm apart)
    assert np.abs(got[:, 1].astype(np.float64) - np.sin(phi)).max() < 1e-7
    assert abi.cast_beams(m, 359, 1, 1).shape == (1, 2) and abi.cast_beams(m, 0, 1, 360).shape == (360, 2)
    for first, step, A in ((360, 1, 1), (0, 1, 361), (3, 7, 52), (0, 0, 0), (0, 1, 16385)):
        with pytest.raises(abi.RplGpuError):
            abi.cast_beams(m, first, step, A)
    with pytest.raises(abi.RplGpuError):
        abi.cast_beams(abi.ScanMerge(0.0, 1.0, 0, 0.1, 30.0, 0.1), 0, 1, 1)
    assert abi.load_library().rplgpu_cast_beams(C.byref(m), 0, 1, 1, None) == abi.ERR_INVALID_ARG


def test_cast_range_m():
    assert abi.cast_range_m(16 | co.HIT << 28, 0.05) == 4.0 * float(F32(0.05))
    assert abi.cast_range_m(2 | co.UNKNOWN << 28, 1.0) == math.sqrt(2.0) and abi.cast_range_m(co.LEFT << 28, 1.0) == 0.0
    assert abi.cast_range_m(9 | co.NO_STOP << 28, 1.0) == math.inf and math.isnan(abi.cast_range_m(co.DROPPED, 1.0))
    for w in (0, 5 | co.LEFT << 28, 1 << 27, co.NO_STOP << 28, co.DROPPED):
        a, b = abi.cast_range_m(w, 0.05), co.range_m(w, 0.05)
        assert a == b or (math.isnan(a) and math.isnan(b))


def test_twin_refusals_write_nothing():
    lib = abi.load_library()
    s = abi.RangeCast.defaults(width=4, height=4, table_half=1)
    poses, beams = np.array([[1, 0, -25.5, -25.5]], F32), np.array([[1, 0]], F32)
    grid, z, table = np.zeros((4, 4), np.int8), np.array([1.0, 2.0], F32), np.array([1, 2, 3, 4], np.uint8)
    out = [np.full(4, GUARD_WORD, np.uint32) for _ in range(4)]            # ranges, weights, result, cast

    def call(spec=s, poses_=poses.ctypes.data, P=1, beams_=beams.ctypes.data, A=1, grid_=grid.ctypes.data,
             z_=z.ctypes.data, n=2, first=0, step=1, table_=table.ctypes.data, ranges_=out[0].ctypes.data,
             w_=out[1].ctypes.data, res_=None, cast_=None):
        res = np.full(9, GUARD_WORD, np.uint32) if res_ is None else res_
        cast = np.full(9, GUARD_WORD, np.uint32)
        rc = lib.rplgpu_cast_ranges_host(C.byref(spec) if spec is not None else None, poses_, P, beams_, A, grid_, z_,
                                         n, first, step, table_, ranges_, w_, res.ctypes.data,
                                         cast.ctypes.data if cast_ != 0 else None)
        return rc, res, cast

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(spec=None), dict(spec=abi.RangeCast.defaults(width=0)), dict(poses_=None), dict(beams_=None),
               dict(grid_=None), dict(cast_=0), dict(P=0), dict(P=abi.MAX_POSES + 1), dict(A=0), dict(A=16385),
               dict(P=1 << 20, A=257), dict(ranges_=None, z_=None), dict(table_=None), dict(w_=None),
               dict(first=2), dict(first=1, step=1, A=2), dict(n=0)):
        rc, res, cast = call(**kw)
        assert rc == bad, kw
        assert (res == GUARD_WORD).all() and (cast == GUARD_WORD).all(), kw
    assert all((o == GUARD_WORD).all() for o in out)
    rc, res, cast = call()
    assert rc == abi.OK and res[8] == GUARD_WORD == cast[8] and out[0][1] == GUARD_WORD == out[1][1]
    assert int(cast[:5].sum()) == 1 and int(res[4]) == 1


# ---- known answers: a 9 x 9 grid of 1 m cells at the origin, poses at cell centres ---------------------------------------
def board(marks=(), ring=False):
    g = np.zeros((9, 9), np.int8)
    if ring:
        g[0, :] = g[8, :] = g[:, 0] = g[:, 8] = 100
    for x, y, v in marks:
        g[y, x] = v
    return g


def answer(grid, pose, beam, N, **kw):
    """(kind, D2, n) of one ray: the twin and both writers, which must agree."""
    s = co.spec(origin_x=0.0, origin_y=0.0, resolution=1.0, width=grid.shape[1], height=grid.shape[0], max_steps=N, **kw)
    poses, beams = np.array([pose], F32), np.array([beam], F32)
    r, _, _, cast = abi.cast_ranges_host(poses, beams, grid, spec_of(s))
    a, b = co.cast_group(s, poses, beams, grid, writer=1), co.cast_group(s, poses, beams, grid, writer=2)
    assert r.tobytes() == a["ranges"].tobytes() == b["ranges"].tobytes()
    assert cast.tobytes() == a["cast"].tobytes() == b["cast"].tobytes()
    w = int(r[0, 0])
    if w == co.DROPPED:
        return "dropped"
    n = int(cast[6])
    assert int(cast[w >> 28]) == 1 and int(cast[5]) == ((w & 0x0FFFFFFF) if (w >> 28) == co.HIT else 0)
    return w >> 28, w & 0x0FFFFFFF, n


C44 = (1.0, 0.0, 4.5, 4.5)


@pytest.mark.parametrize("beam", [(1, 0), (-1, 0), (0, 1), (0, -1)])
def test_axis_rays(beam):
    assert answer(board(ring=True), C44, beam, 20) == (co.HIT, 16, 4)
    assert answer(board(), C44, beam, 20) == (co.LEFT, 25, 5)
    assert answer(board(), C44, beam, 3) == (co.NO_STOP, 9, 3)


@pytest.mark.parametrize("sx", [1, -1])
@pytest.mark.parametrize("sy", [1, -1])
@pytest.mark.parametrize("swap", [0, 1])
def test_eight_octants(sx, sy, swap):
    """(4, 4) -> (8, 6) visits (5, 4), (6, 5), (7, 5), (8, 6) (ax 4, ay 2, err 2, 0, 2, 0, 2); mirrored into every
    octant the walk is the mirror image"""
    def m(dx, dy):
        dx, dy = (dy, dx) if swap else (dx, dy)
        return 4 + sx * dx, 4 + sy * dy
    beam = (sx * 0.5, sy * 1.0) if swap else (sx * 1.0, sy * 0.5)
    assert answer(board(), C44, beam, 4) == (co.NO_STOP, 20, 4)
    for n, (dx, dy) in enumerate([(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]):
        x, y = m(dx, dy)
        assert answer(board([(x, y, 100)]), C44, beam, 4) == (co.HIT, dx * dx + dy * dy, n)
    for dx, dy in [(1, 1), (2, 0), (3, 2), (4, 1), (2, 2)]:                  # cells beside the walk stop nothing
        x, y = m(dx, dy)
        assert answer(board([(x, y, 100)]), C44, beam, 4) == (co.NO_STOP, 20, 4)


def test_exact_diagonal_and_a_wall_met_at_a_corner():
    assert answer(board([(6, 6, 100)]), C44, (1, 1), 3) == (co.HIT, 8, 2)
    assert answer(board(), C44, (1, 1), 3) == (co.NO_STOP, 18, 3)
    # a wall one cell thick whose cells touch only at a corner lets the diagonal through: no cell of the walk is a wall
    assert answer(board([(5, 4, 100), (4, 5, 100), (6, 5, 100), (5, 6, 100)]), C44, (1, 1), 3) == (co.NO_STOP, 18, 3)
    assert answer(board([(5, 4, 100), (4, 5, 100), (5, 5, -1)]), C44, (1, 1), 3) == (co.UNKNOWN, 2, 1)
    assert answer(board([(5, 5, -1)]), C44, (1, 1), 3, unknown_stops=0) == (co.NO_STOP, 18, 3)


def test_start_cells_and_the_bounds_of_the_walk():
    assert answer(board(), (1, 0, -0.5, 4.5), (1, 0), 20) == (co.LEFT, 0, 0)         # starts outside: no way back in
    assert answer(board(), (1, 0, 4.5, 9.5), (0, -1), 20) == (co.LEFT, 0, 0)
    assert answer(board([(4, 4, 100)]), C44, (1, 0), 20) == (co.HIT, 0, 0)           # starts on an obstacle
    assert answer(board([(4, 4, -1)]), C44, (1, 0), 20) == (co.UNKNOWN, 0, 0)
    assert answer(board([(4, 4, 99)]), C44, (1, 0), 20) == (co.LEFT, 25, 5)          # (99 < hit_lo)
    assert answer(board([(4, 4, 99)]), C44, (1, 0), 20, hit_lo=99) == (co.HIT, 0, 0)
    assert answer(board(), C44, (1, 0), 1) == (co.NO_STOP, 1, 1)                     # N = 1
    assert answer(board([(5, 4, 100)]), C44, (1, 0), 1) == (co.HIT, 1, 1)
    assert answer(board([(6, 4, 100)]), C44, (1, 0), 1) == (co.NO_STOP, 1, 1)
    assert answer(board(), C44, (0.5, 0), 4) == (co.NO_STOP, 4, 2)                   # the end cell before N
    assert answer(board([(7, 4, 100)]), C44, (0.5, 0), 4) == (co.NO_STOP, 4, 2)
    assert answer(board(), C44, (0, 0), 4) == (co.NO_STOP, 0, 0)                     # the zero matrix
    assert answer(board(), (math.nan, 0, 4.5, 4.5), (1, 0), 4) == "dropped"
    assert answer(board(), (1, 0, 4.5, 2e6), (1, 0), 4) == "dropped"
    assert answer(board(), (1e7, 0, 4.5, 4.5), (1, 0), 4) == "dropped"               # no end cell


# ---- the index rule at its edges ------------------------------------------------------------------------------------------
TABLE3 = np.array([10, 11, 12, 13, 14, 15, 16, 99], np.uint8)                        # K = 3


def weight(grid, N, z, beam=(1, 0)):
    s = co.spec(origin_x=0.0, origin_y=0.0, resolution=1.0, width=9, height=9, max_steps=N, table_half=3)
    poses, beams, z = np.array([C44], F32), np.array([beam], F32), np.array([z], F32)
    _, w, res, _ = abi.cast_ranges_host(poses, beams, grid, spec_of(s), z, TABLE3)
    for writer in (1, 2):
        o = co.cast_group(s, poses, beams, grid, z, 0, 1, TABLE3, writer)
        assert w.tobytes() == o["weights"].tobytes() and res.tobytes() == o["result"].tobytes(), writer
    return int(w[0]), int(res[4])


def test_table_index_rule():
    hit = board(ring=True)                                                           # HIT at 4 cells
    assert weight(hit, 20, 4.0) == (13, 1) and weight(hit, 20, 4.99) == (13, 1)
    assert weight(hit, 20, 3.5) == (12, 1)                                           # floorf(-0.5) = -1, not 0
    assert weight(hit, 20, 3.0) == (12, 1) and weight(hit, 20, 2.99) == (11, 1)
    assert weight(hit, 20, 1.0) == (10, 1) and weight(hit, 20, 0.5) == (10, 1)       # d = -K exactly, then beyond
    assert weight(hit, 20, 0.0) == (10, 1) and weight(hit, 20, -5.0) == (10, 1)
    assert weight(hit, 20, 6.99) == (15, 1) and weight(hit, 20, 7.0) == (16, 1)      # d = +K exactly
    assert weight(hit, 20, 7.5) == (16, 1) and weight(hit, 20, 1e30) == (16, 1)
    assert weight(hit, 20, math.inf) == (16, 1)                                      # z = +inf against a HIT
    assert weight(hit, 20, -math.inf) == (10, 1)
    assert weight(hit, 20, math.nan) == (0, 0)                                       # the beam is skipped
    free = board()
    assert weight(free, 3, math.inf) == (99, 1)                                      # both infinite
    assert weight(free, 3, 2.0) == (10, 1) and weight(free, 3, 1e30) == (10, 1)      # NONE against a return
    assert weight(free, 20, 5.5) == (13, 1)                                          # LEFT has a range (5 cells)
    assert weight(board([(4, 4, 100)]), 20, 0.5) == (13, 1)                          # D2 = 0
    assert weight(hit, 20, 5.0, (math.nan, 0)) == (0, 1)                             # a dropped ray: skipped, the beam counts


# ---- the identities ---------------------------------------------------------------------------------------------------------
def test_identity_1_a_pose_heading_is_a_beam_direction():
    case = cc.case("p64")
    s, poses, grid = case["spec"], case["lists"][0], case["grids"][0]
    ahead = np.array([[1, 0]], F32)
    plain = poses.copy()
    plain[:, 0], plain[:, 1] = 1.0, 0.0
    for cast in (lambda p, b: abi.cast_ranges_host(p, b, grid, spec_of(s))[0], lambda p, b: co.cast_lockstep(s, p, b, grid)[0]):
        a = cast(poses, ahead)[:, 0]
        b = np.diagonal(cast(plain, np.ascontiguousarray(poses[:, :2])))
        assert a.tobytes() == b.tobytes() and len({int(v) >> 28 for v in a}) >= 3


def test_identity_2_the_weights_follow_from_the_range_words():
    for name in ("p64", "p65", "a360", "odd"):
        case = cc.case(name)
        r, w, _, _ = twin(case)
        z = co.beam_ranges(case["measured"][0], case["first"], case["step"], len(case["beams"]))
        assert co.weights_rays(case["spec"], r, z, case["table"]).tobytes() == w.tobytes(), name
        assert co.weights_table(case["spec"], r, z, case["table"]).tobytes() == w.tobytes(), name


def test_identity_3_a_list_in_two_pieces():
    case = cc.case("p65")
    r, w, _, cast = twin(case)
    k = 23
    parts = [abi.cast_ranges_host(case["lists"][0][a:b], case["beams"], case["grids"][0], spec_of(case["spec"]),
                                  case["measured"][0], case["table"], case["first"], case["step"])
             for a, b in ((0, k), (k, len(r)))]
    assert np.concatenate([p[0] for p in parts]).tobytes() == r.tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == w.tobytes()
    c0, c1 = (p[3].astype(np.int64) for p in parts)
    total = (c0[6] | c0[7] << 32) + (c1[6] | c1[7] << 32)
    assert (c0[:5] + c1[:5]).tolist() == cast[:5].tolist() and max(c0[5], c1[5]) == cast[5]
    assert total == int(cast[6]) | int(cast[7]) << 32


def test_identity_4_the_result_words_are_e15s_on_the_weights():
    for name in ("p64", "p1023", "zeros", "odd"):
        case = cc.case(name)
        _, w, res, _ = twin(case)
        z = co.beam_ranges(case["measured"][0], case["first"], case["step"], len(case["beams"]))
        assert res.tobytes() == po.result_of(w, int((~np.isnan(z)).sum())).tobytes(), name
