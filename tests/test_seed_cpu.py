"""E19 without a device: the new symbols, the struct's layout and the defaults; the spec check's refusals; the heading
helper's known answers; the draw's exact property from the formula; rplgpu_seed_poses_host (the rule in plain C++)
against both writers of tests/seed_oracle.py on every case of tests/seed_cases.py and on random inputs, the writers
against each other; a list made in pieces; the scratch size; and the refusals of the host functions."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import motion_oracle as mo
from tests import seed_cases as sc
from tests import seed_oracle as so

F32 = np.float32


def _host(case, g):
    L = len(case["grids"])
    poses, cells, res = abi.seed_poses_host(case["grids"][g if L > 1 else 0], case["headings"], case["M"],
                                            sc.spec_of(case["spec"]), sc.noise_of(case["noise"]), g)
    assert poses.dtype == F32 and poses.shape == (case["M"], 4) and cells.dtype == res.dtype == np.uint32
    return poses.view(np.uint32), cells, res


def _all_three(case, key=None, both=True):
    """the host function, the default writer and (with `both`) the numpy writer: the same words; -> the oracle's
    triple"""
    a = sc.want(case, key)
    if both:
        b = sc.want(case, None, writer=so.poses_numpy)
        for k in range(3):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (k, a[2], b[2])
    for g in range(case["G"]):
        words, cells, res = _host(case, g)
        assert cells.tobytes() == a[1][g].tobytes(), g
        assert words.tobytes() == a[0][g].tobytes(), g
        assert res.tobytes() == a[2][g].tobytes(), (g, res, a[2][g])
    return a


# ---- symbols, the struct, the defaults ----------------------------------------------------------------------------------
def test_symbols_struct_and_defaults():
    s = abi.PoseSeed.defaults()
    lib = abi.load_library()
    for name in ("rplgpu_default_pose_seed", "rplgpu_pose_seed_check", "rplgpu_seed_scratch_words",
                 "rplgpu_seed_headings", "rplgpu_seed_poses_dev", "rplgpu_seed_poses_host", "rplgpu_seed_poses"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    for fn in ("seed_poses_dev", "seed_poses"):
        assert callable(getattr(abi.RplGpu, fn))
    d = so.DEFAULT
    assert (s.width, s.height, s.free_lo, s.free_hi, s.flags) == (1024, 1024, 0, 0, 0)
    assert (s.width, s.height, s.free_lo, s.free_hi, s.flags) == tuple(d[k] for k in ("width", "height", "free_lo",
                                                                                      "free_hi", "flags"))
    assert (s.origin_x, s.origin_y, s.resolution) == (F32(-25.6), F32(-25.6), F32(0.05))
    p = abi.PoseScore()
    lib.rplgpu_default_pose_score(C.byref(p))                     # E15's default grid is the same grid
    assert (p.origin_x, p.origin_y, p.resolution, p.width, p.height) == (s.origin_x, s.origin_y, s.resolution, s.width,
                                                                         s.height)
    assert C.sizeof(abi.PoseSeed) == 32
    assert [getattr(abi.PoseSeed, f).offset for f, _ in abi.PoseSeed._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert s.check() == abi.OK
    lib.rplgpu_default_pose_seed(None)                            # (ignored)
    assert lib.rplgpu_abi_version() == 1


@pytest.mark.parametrize("field,value", [
    ("origin_x", math.nan), ("origin_y", math.inf), ("resolution", -math.inf), ("resolution", math.nan),
    ("resolution", 0.0), ("resolution", -0.05),
    ("width", 0), ("width", abi.MAX_OCC_DIM + 1), ("height", 0), ("height", abi.MAX_OCC_DIM + 1),
    ("free_lo", -129), ("free_lo", 128), ("free_hi", -129), ("free_hi", 128), ("flags", 2), ("flags", 1 << 31)])
def test_spec_check_refusals(field, value):
    assert abi.PoseSeed.defaults(**{field: value}).check() == abi.ERR_INVALID_ARG


def test_spec_check_limits():
    lib = abi.load_library()
    assert lib.rplgpu_pose_seed_check(None) == abi.ERR_INVALID_ARG
    assert abi.PoseSeed.defaults(free_lo=1, free_hi=0).check() == abi.ERR_INVALID_ARG          # free_lo > free_hi
    for ok in (dict(free_lo=-128, free_hi=127), dict(free_lo=127, free_hi=127), dict(free_lo=-128, free_hi=-128),
               dict(width=abi.MAX_OCC_DIM, height=1), dict(width=1, height=abi.MAX_OCC_DIM), dict(flags=1),
               dict(resolution=1e-30), dict(origin_x=-3e38, origin_y=3e38)):
        assert abi.PoseSeed.defaults(**ok).check() == abi.OK, ok


# ---- the heading helper -------------------------------------------------------------------------------------------------
def test_seed_headings_known_answers():
    assert abi.seed_headings(1).tolist() == [[1.0, 0.0]]
    h4 = abi.seed_headings(4)
    assert h4.dtype == F32 and h4.shape == (4, 2)
    assert h4[0].tolist() == [1.0, 0.0] and h4[0].view(np.uint32).tolist() == [0x3F800000, 0]
    assert h4[1, 1] == 1.0 and h4[2, 0] == -1.0 and h4[3, 1] == -1.0
    assert h4[1, 0] == F32(math.cos(math.pi / 2)) and abs(h4[1, 0]) < 1e-16 and abs(h4[2, 1]) < 1e-15
    for H in (1, 2, 3, 4, 7, 360, 65536):
        got = abi.seed_headings(H)
        assert got.tobytes() == so.headings(H).tobytes() and got[0].tolist() == [1.0, 0.0], H
        assert np.abs(np.hypot(got[:, 0].astype(np.float64), got[:, 1]) - 1).max() < 1e-7
    lib = abi.load_library()
    buf = np.full(8, 9.0, F32)
    assert lib.rplgpu_seed_headings(0, buf.ctypes.data) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_seed_headings(65537, buf.ctypes.data) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_seed_headings(4, None) == abi.ERR_INVALID_ARG and (buf == 9.0).all()
    assert lib.rplgpu_seed_headings(2, buf.ctypes.data) == abi.OK and (buf[4:] == 9.0).all() and buf[2] == -1.0


# ---- the draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3, 7, 15, 1000, 4087, (1 << 24) - 1, 1 << 24])
def test_the_draw_is_uniform_to_one_part_in_2_32(F):
    """r = (p0 * F) >> 32 over all 2^32 values of p0: r = i exactly for ceil(i 2^32 / F) <= p0 < ceil((i + 1) 2^32 / F),
    so cell i is hit floor or ceil of 2^32 / F times, every value below F is hit and none above — arithmetic on the
    formula, not a sample.  The edges are checked against the formula itself."""
    edge = lambda i: -((-i << 32) // F)                                  # ceil(i 2^32 / F)  # noqa: E731
    lo, hi = (1 << 32) // F, -((-1 << 32) // F)
    picks = range(F) if F <= 4087 else [0, 1, 2, F // 3, F // 2, F - 3, F - 2, F - 1]
    total = 0
    for i in picks:
        a, b = edge(i), edge(i + 1)
        assert (a * F) >> 32 == i and ((b - 1) * F) >> 32 == i           # the first and the last p0 of cell i
        assert a == 0 or ((a - 1) * F) >> 32 == i - 1
        assert b - a in (lo, hi)
        total += b - a
    assert edge(0) == 0 and edge(F) == 1 << 32 and (((1 << 32) - 1) * F) >> 32 == F - 1
    if F <= 4087:
        assert total == 1 << 32
    # ... and the library and both writers use that formula: the cells of a one-row grid of F free cells are the ranks
    if F <= 4096:
        M = 300
        noise = dict(seed=F, step=1, first=0)
        grid = np.zeros(F, np.int8)
        _, cells, res = abi.seed_poses_host(grid, sc.table(), M, sc.spec_of(sc.grid_spec(F, 1)), sc.noise_of(noise))
        want = [(mo.philox_python((j, 3, 1, 0), (F, 0))[0] * F) >> 32 for j in range(M)]
        assert cells.tolist() == want and res[0] == F and so.ranks_numpy(noise, 0, M, F).tolist() == want


def test_the_draw_uses_index_3_and_every_word():
    """output 0's counter is (first, (g << 2) | 3, step low, step high) under the key (seed low, seed high); p0 picks
    the cell, p1 the heading, the top bytes of p2 and p3 the jitter"""
    noise = dict(seed=(0x299F31D0 << 32) | 0xA4093822, step=(0x03707344 << 32) | 0x13198A2E, first=0x243F6A88)
    g = 0x85A308D3 >> 2 & 0xFFFF
    p = mo.philox_python((0x243F6A88, (g << 2) | 3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    spec = dict(sc.grid_spec(64, 32), origin_x=0.0, origin_y=0.0, resolution=1.0)
    H = 1000
    poses, cells, res = abi.seed_poses_host(np.zeros(2048, np.int8), so.headings(H), 1, sc.spec_of(spec),
                                            sc.noise_of(noise), g)
    r = (p[0] * 2048) >> 32
    assert cells[0] == r and poses[0, :2].tobytes() == so.headings(H)[(p[1] * H) >> 32].tobytes()
    assert poses[0, 2] == r % 64 + ((p[2] >> 24) + 0.5) / 256 and poses[0, 3] == r // 64 + ((p[3] >> 24) + 0.5) / 256
    assert res.tolist() == [2048, 0, r, r, 0, 0, 0, 0]


# ---- every case: host function and both writers -------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", sc.SIZES)
def test_size_cases(width, height):
    case = sc.size_case(width, height)
    sc.size_regime(case, _all_three(case, f"size{width}x{height}"))


def test_default_grid_and_largest_list():
    case = sc.default_case()
    a = sc.want(case, "default")                                 # (the numpy writer alone at this size)
    sc.default_regime(case, a)
    words, cells, res = _host(case, 0)
    assert words.tobytes() == a[0][0].tobytes() and cells.tobytes() == a[1][0].tobytes()
    assert res.tobytes() == a[2][0].tobytes()


def test_largest_grid_sparse():
    case = sc.sparse_case()
    a = sc.want(case, "sparse")
    sc.sparse_regime(case, a)
    words, cells, res = _host(case, 0)
    assert words.tobytes() == a[0][0].tobytes() and cells.tobytes() == a[1][0].tobytes()
    assert res.tobytes() == a[2][0].tobytes()


@pytest.mark.parametrize("name", sc.PATTERNS)
def test_pattern_cases(name):
    case = sc.pattern_case(name)
    both = case["M"] <= so.PYTHON_LIMIT
    sc.pattern_regime(name, case, _all_three(case, f"pattern_{name}", both=both))
    if not both:                                                 # the loop writer on the first outputs
        short = dict(case, M=500)
        _all_three(short)


@pytest.mark.parametrize("lo,hi", sc.RANGES)
def test_byte_values(lo, hi):
    case = sc.bytes_case(lo, hi)
    sc.bytes_regime(case, _all_three(case, f"bytes{lo}_{hi}"))


def test_tail_bytes_and_row_major_order():
    """bytes behind the last cell never count (the host function is given a longer buffer of free-looking bytes), and
    the free cells are ordered by cy * width + cx"""
    spec = sc.grid_spec(5, 3)
    grid = np.full(40, 0, np.int8)
    grid[:15] = 100
    grid[[1, 5]] = 0                                             # (cx, cy) = (1, 0) before (0, 1)
    noise = dict(seed=1, step=0, first=0)
    words, cells, res = so.seed(grid, spec, sc.table(), 64, noise)
    r = so.ranks_numpy(noise, 0, 64, 2)
    assert res[0] == 2 and set(r.tolist()) == {0, 1} and cells.tolist() == [1 if v == 0 else 5 for v in r]
    buf = np.ascontiguousarray(grid)
    poses = np.zeros((64, 4), F32)
    got_cells = np.zeros(64, np.uint32)
    got_res = np.zeros(8, np.uint32)
    s, n = sc.spec_of(spec), sc.noise_of(noise)
    assert abi.load_library().rplgpu_seed_poses_host(C.byref(s), buf.ctypes.data, sc.table().ctypes.data, 16, 0, 64,
                                                     C.byref(n), poses.ctypes.data, got_cells.ctypes.data,
                                                     got_res.ctypes.data) == abi.OK
    assert got_cells.tobytes() == cells.tobytes() and got_res.tobytes() == res.tobytes()
    assert poses.view(np.uint32).tobytes() == words.tobytes()


@pytest.mark.parametrize("M", sc.EDGE_M)
def test_edge_cases(M):
    case = sc.edge_case(M)
    sc.edge_regime(case, _all_three(case, f"edge{M}"))


@pytest.mark.parametrize("gpg", [0, 1])
def test_groups_cases(gpg):
    case = sc.groups_case(gpg)
    sc.groups_regime(case, _all_three(case, f"groups{gpg}"))


@pytest.mark.parametrize("kind", ["one", "most", "bits"])
def test_headings_cases(kind):
    case = sc.headings_case(kind)
    sc.headings_regime(kind, case, _all_three(case, f"headings_{kind}", both=case["M"] <= so.PYTHON_LIMIT))


@pytest.mark.parametrize("kind", sc.COUNTER_KINDS)
def test_counter_cases(kind):
    case = sc.counter_case(kind)
    sc.counter_regime(kind, _all_three(case, f"counter_{kind}"))


def test_a_list_in_pieces():
    whole, pieces, cuts = sc.piece_cases()
    a = sc.want(whole, "whole")
    host = _host(whole, 0)
    assert host[0].tobytes() == a[0][0].tobytes() and host[1].tobytes() == a[1][0].tobytes()
    for piece, lo, hi in zip(pieces, cuts, cuts[1:]):
        b = _all_three(piece)
        assert b[0][0].tobytes() == a[0][0, lo:hi].tobytes() and b[1][0].tobytes() == a[1][0, lo:hi].tobytes()
    assert a[0][0, :1000].tobytes() != a[0][0, 1000:2000].tobytes()


def test_cell_centres():
    case = sc.centres_case()
    sc.centres_regime(case, _all_three(case, "centres"))


def test_the_round_trip_counts():
    near, far = sc._small(), sc.far_case()
    sc.small_regime(near, _all_three(near, "small"))
    sc.far_regime(far, _all_three(far, "far"))


def test_writers_on_random_inputs():
    rng = np.random.default_rng(1919)
    for _ in range(80):
        _all_three(sc.random_case(rng))


def test_chain_regimes(oracle):
    """the chains of tests/test_gpu_seed.py, every stage's oracle chained here: their regimes hold, and the host
    function gives the seeded stage"""
    a = sc.init_chain(oracle)
    poses, cells, res = abi.seed_poses_host(a["grid"], a["table"], sc.CHAIN_P, sc.spec_of(a["sspec"]),
                                            sc.noise_of(a["noise"]))
    assert poses.view(np.uint32).tobytes() == a["words"].tobytes() and res.tobytes() == a["r19"].tobytes()
    b = sc.inject_chain(oracle)
    poses, cells, res = abi.seed_poses_host(b["grid"], b["table"], sc.CHAIN_INJECT, sc.spec_of(b["sspec"]),
                                            sc.noise_of(b["inoise"]))
    assert poses.view(np.uint32).tobytes() == b["iwords"].tobytes() and res.tobytes() == b["r19"].tobytes()


# ---- scratch, refusals --------------------------------------------------------------------------------------------------
def test_scratch_words():
    big = abi.MAX_OCC_DIM
    for bad in ((0, 64, 64), (65536, 64, 64), (1, 0, 64), (1, 64, 0), (1, big + 1, 1), (1, 1, big + 1)):
        assert abi.seed_scratch_words(*bad) == 0, bad
    one = abi.seed_scratch_words(1, 1, 1)
    assert 0 < one <= 256 and one % 2 == 0
    assert abi.seed_scratch_words(7, 1, 1) == 7 * one
    full = abi.seed_scratch_words(1, big, big)
    assert full % 2 == 0 and 32 * full <= 2 * big * big          # within a few bits per cell: here below two
    assert abi.seed_scratch_words(65535, big, big) == 65535 * full
    sizes = [abi.seed_scratch_words(1, w, 64) for w in (63, 64, 65, 128, 129)]
    assert sizes[0] == sizes[1] < sizes[2] == sizes[3] < sizes[4]          # it grows by whole blocks of 4096 cells


def test_host_function_refusals():
    lib = abi.load_library()
    bad = abi.ERR_INVALID_ARG
    grid = np.zeros(15, np.int8)
    head = sc.table(4)
    poses = np.full(24, 7.0, F32)
    cells = np.full(6, 77, np.uint32)
    res = np.full(12, 77, np.uint32)
    good, noise = sc.spec_of(sc.grid_spec(5, 3)), abi.MotionNoise.defaults()

    def call(spec=good, grid_=grid.ctypes.data, head_=head.ctypes.data, H=4, g=0, M=2, noise_=noise,
             poses_=poses.ctypes.data, cells_=cells.ctypes.data, res_=res.ctypes.data):
        return lib.rplgpu_seed_poses_host(C.byref(spec) if spec is not None else None, grid_, head_, H, g, M,
                                          C.byref(noise_) if noise_ is not None else None, poses_, cells_, res_)

    assert call(spec=None) == bad and call(spec=sc.spec_of(sc.grid_spec(5, 3, flags=2))) == bad
    assert call(grid_=0) == bad and call(head_=0) == bad and call(noise_=None) == bad
    assert call(poses_=0) == bad and call(res_=0) == bad
    assert call(H=0) == bad and call(H=65537) == bad and call(M=0) == bad and call(M=abi.MAX_POSES + 1) == bad
    assert call(g=65535) == bad
    assert (poses == 7.0).all() and (cells == 77).all() and (res == 77).all()
    assert call(g=65534) == abi.OK and (poses[8:] == 7.0).all() and (cells[2:] == 77).all() and (res[8:] == 77).all()
    assert res[0] == 15 and res[4:7].tolist() == [0, 0, 0]
    poses[:] = 7.0
    assert call(cells_=0) == abi.OK and (poses[:8] != 7.0).all()               # the cell indices are optional
    with pytest.raises(abi.RplGpuError) as e:
        abi.seed_poses_host(grid, head, 0, good)
    assert e.value.code == bad
