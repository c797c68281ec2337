"""E16 without a device: the new symbols and the scratch formula, rplgpu_resample_host (the rule in plain C++)
against both writers of tests/resample_oracle.py on every case of tests/resample_cases.py, the writers against each
other, the properties the rule promises, the 64-bit forms of r and t_j against Python's integers, answers worked out
by hand, and the refusals of the host function."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import resample_cases as rc
from tests import resample_oracle as ro

F32 = np.float32
U32_MAX = 0xFFFFFFFF
WRITERS = (ro.ancestors_search, ro.ancestors_counts)


def _host(case, g=0):
    w, poses, M, u, d = rc.group_inputs(case, g)
    return abi.resample_host(w, poses, M, u, d)


def _same(got, want_):
    for a, b in zip(got, want_):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _all_three(case, key=None, groups=None):
    """the host function, the first writer and the second writer: the same bytes"""
    a = rc.want(case, key)
    b = rc.want(case, None, writer=ro.ancestors_counts)
    for g in range(len(a)) if groups is None else groups:
        _same(a[g], b[g])
        _same(_host(case, g), a[g])


# ---- symbols, the scratch formula ----------------------------------------------------------------------------------------
def test_symbols_and_scratch_words():
    lib = abi.load_library()
    for name in ("rplgpu_resample_scratch_words", "rplgpu_resample_poses_dev", "rplgpu_resample_host",
                 "rplgpu_resample_poses"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    for fn in ("resample_poses_dev", "resample_poses"):
        assert callable(getattr(abi.RplGpu, fn))
    for G, P in [(1, 1), (1, 1024), (1, 1025), (7, 4096), (101, 1100), (65535, 3), (1, 1 << 20), (3, (1 << 20) - 1)]:
        n = abi.resample_scratch_words(G, P)
        assert n == ro.scratch_words(G, P) and n % 2 == 0 and n >= G * (16 + 9 * ro.tiles(P) + 1)
    for G, P in [(0, 5), (5, 0), (1, (1 << 20) + 1), (0, 0)]:
        assert abi.resample_scratch_words(G, P) == 0 == ro.scratch_words(G, P)
    assert abi.resample_scratch_words(65535, 1 << 20) == 65535 * (16 + 8 * 1024 + 1026) > 1 << 29  # needs 64 bits of bytes


# ---- every case: host function and both writers ------------------------------------------------------------------------------
@pytest.mark.parametrize("P", rc.EDGE_P)
def test_edge_cases(P):
    for M in rc.edge_ms(P):
        case = rc.edge_case(P, M)
        rc.edge_regime(case)
        _all_three(case, f"edge{P}_{M}")


@pytest.mark.parametrize("kind", rc.DEAD_KINDS)
def test_dead_cases(kind):
    case = rc.dead_case(kind)
    rc.dead_regime(case, kind)
    _all_three(case, f"dead_{kind}")


def test_extreme_cases():
    case = rc.allmax_case()
    rc.allmax_regime(case)
    _all_three(case, "allmax")
    case = rc.small_case()
    rc.small_regime(case)
    _all_three(case, "small")
    rc.u_regime()
    _all_three(rc.u_case(0), "u0")
    _all_three(rc.u_case(U32_MAX), "umax")
    case = rc.walk_case()
    rc.walk_regime(case)
    _all_three(case, "walk")


def test_big_case():
    case = rc.big_case()
    rc.big_regime(case)
    _all_three(case, "big")


@pytest.mark.parametrize("M", rc.ZERO_M)
def test_zero_cases(M):
    case = rc.zero_case(M)
    rc.zero_regime(case)
    _all_three(case)
    small = rc.zero_case(5, P=3)
    rc.zero_regime(small)
    _all_three(small)


@pytest.mark.parametrize("n_delta,G,per_group,special", [
    (0, 1, 0, False), (1, 1, 0, False), (rc.MOVE_M, 1, 0, False), (0, 1, 0, True), (1, 1, 0, True),
    (rc.MOVE_M, 1, 0, True), (1, 3, 0, True), (1, 3, 1, True), (rc.MOVE_M, 3, 0, False), (rc.MOVE_M, 3, 1, True)])
def test_move_cases(n_delta, G, per_group, special):
    case = rc.move_case(n_delta, G, per_group, special)
    rc.move_regime(case, special)
    _all_three(case)


@pytest.mark.parametrize("ppg", [0, 1])
def test_groups_cases(ppg):
    case = rc.groups_case(ppg)
    rc.groups_regime(case)
    _all_three(case, f"groups{len(case['poses'])}", groups=[0, 7, 8, 50, 100])
    a = rc.want(case, f"groups{len(case['poses'])}")
    b = rc.want(case, None, writer=ro.ancestors_counts)
    for x, y in zip(a, b):
        _same(x, y)


def test_words_case():
    case = rc.words_case()
    rc.words_regime(case)
    _all_three(case, "words")


def test_words_wide_case():
    case = rc.words_wide_case()
    rc.words_wide_regime(case)
    _all_three(case, "words_wide")


# ---- the properties the rule promises ---------------------------------------------------------------------------------------
def test_properties_on_random_lists():
    rng = np.random.default_rng(1601)
    for w, M, u in rc.form_samples(rng, 300):
        S = ro.total(w)
        a = ro.ancestors_search(w, M, u)
        b = ro.ancestors_counts(w, M, u)
        assert a.tobytes() == b.tobytes()
        assert (np.diff(a.astype(np.int64)) >= 0).all()                 # non-decreasing
        assert (w[a] > 0).all()                                          # a zero weight is never drawn
        k = np.bincount(a, minlength=len(w))
        r = ro.r_of(u, S)
        assert 0 <= r < S and int(ro.t_all(S, r, M)[-1]) < S             # every output has an ancestor
        for i, wi in enumerate(w.tolist()):
            lo = (M * wi) // S
            assert lo <= k[i] <= lo + (1 if (M * wi) % S else 0)         # floor or ceil of M w / S


def test_host_function_on_random_lists():
    rng = np.random.default_rng(1601)
    for w, M, u in rc.form_samples(rng, 300):
        poses = rc.some_poses(rng, 1, len(w))[0]
        for writer in WRITERS:
            _same(abi.resample_host(w, poses, M, u), ro.resample(w, poses, M, u, writer=writer))


def test_64_bit_forms_against_big_integers():
    rng = np.random.default_rng(1602)
    big_s = (1 << 20) * U32_MAX          # P = 2^20 with every weight 2^32 - 1
    sums = [big_s, big_s - 1, 1, 2, U32_MAX, 1 << 32, (1 << 32) + 1, (1 << 51) + 12345] + \
        [int(v) for v in rng.integers(1, 1 << 52, 200)]
    for S in sums:
        for u in (0, 1, U32_MAX, 0x80000000, int(rng.integers(0, 1 << 32))):
            r = ro.r64(u, S)
            assert r == ro.r_of(u, S) == (u * S) >> 32 and r < S
            for M in (1, 2, 1000, (1 << 20) - 1, 1 << 20, int(rng.integers(1, (1 << 20) + 1))):
                for j in {0, 1, M // 2, M - 1}:
                    if j < M:
                        assert ro.t64(j, S, r, M) == (j * S + r) // M < S


def test_host_function_at_the_largest_sum():
    """the library's own arithmetic where the products are largest: P = 2^20, every weight 2^32 - 1, M = 2^20 - 1, u
    at its end"""
    big_s = (1 << 20) * U32_MAX
    P = 1 << 20
    w = np.full(P, U32_MAX, np.uint32)
    poses = np.zeros((P, 4), F32)
    poses[:, 2] = np.arange(P)
    out, anc, res = abi.resample_host(w, poses, P - 1, U32_MAX)
    t = (np.arange(P - 1, dtype=object) * big_s + ro.r_of(U32_MAX, big_s)) // (P - 1)
    assert anc.tobytes() == (t // U32_MAX).astype(np.uint32).tobytes()   # equal weights: a = t // w
    assert res.tobytes() == ro.result_of(w, P - 1, anc).tobytes() and res[1] == (big_s >> 32)
    assert out[:, 2].tobytes() == anc.astype(F32).tobytes()


# ---- answers by hand ------------------------------------------------------------------------------------------------------------
def test_known_answers():
    rng = np.random.default_rng(1603)
    # equal weights, M = P, any u: r < S = P w, t_j = (j P w + r) // P = j w + r // P with r // P < w: a[j] = j
    for P, wv in [(1, 9), (5, 1), (64, 7), (1025, U32_MAX), (3000, 12345)]:
        w = np.full(P, wv, np.uint32)
        poses = rc.some_poses(rng, 1, P)[0]
        for u in (0, U32_MAX, int(rng.integers(0, 1 << 32))):
            out, anc, res = abi.resample_host(w, poses, P, u)
            assert anc.tolist() == list(range(P)) and out.tobytes() == poses.tobytes() and res[6] == P
            for wr in WRITERS:
                assert wr(w, P, u).tolist() == list(range(P))
    # one-hot: every output is that pose
    for P, at, M in [(1, 0, 7), (9, 4, 1), (2049, 1024, 3000), (2049, 2048, 5)]:
        w = np.zeros(P, np.uint32)
        w[at] = 1 + int(rng.integers(0, 1 << 32 - 1))
        poses = rc.some_poses(rng, 1, P)[0]
        out, anc, res = abi.resample_host(w, poses, M, int(rng.integers(0, 1 << 32)))
        assert (anc == at).all() and (out == poses[at]).all() and res[5] == 1 and res[6] == 1 and res[7] == 0
    # w = (1, 3), M = 4: S = 4, C = (1, 4).
    #   u = 0:        r = 0,                       t = (0, 1, 2, 3)          -> a = (0, 1, 1, 1)
    #   u = 2^32 - 1: r = floor((2^32 - 1) 4 / 2^32) = 3, t_j = (4 j + 3) // 4 = (0, 1, 2, 3) -> a = (0, 1, 1, 1)
    # and with M = 2: u = 0: t = (0, 2) -> a = (0, 1); u = 2^32 - 1: t_j = (4 j + 3) // 2 = (1, 3) -> a = (1, 1)
    w = np.array([1, 3], np.uint32)
    poses = np.array([[1, 0, 10, 20], [0, 1, 30, 40]], F32)
    for u, M, expect in [(0, 4, [0, 1, 1, 1]), (U32_MAX, 4, [0, 1, 1, 1]), (0, 2, [0, 1]), (U32_MAX, 2, [1, 1])]:
        out, anc, res = abi.resample_host(w, poses, M, u)
        assert anc.tolist() == expect and out.tobytes() == poses[expect].tobytes()
        assert res.tolist() == [4, 0, 10, 0, 0, 2, len(set(expect)), 0]
        for wr in WRITERS:
            assert wr(w, M, u).tolist() == expect
    # the move by hand: the pose (0, 1, 2, 3) (heading +90 degrees) moves one metre ahead and turns by +90 degrees
    out, _, _ = abi.resample_host(np.array([1], np.uint32), np.array([[0, 1, 2, 3]], F32), 1, 0,
                                  delta=np.array([0, 1, 1, 0], F32))
    assert out.tolist() == [[-1.0, 0.0, 2.0, 4.0]]
    assert ro.move(np.array([[0, 1, 2, 3]], F32), np.array([[0, 1, 1, 0]], F32)).tolist() == [[-1.0, 0.0, 2.0, 4.0]]


def test_identity_delta_is_not_the_bit_copy():
    case = rc.minus_zero_case()
    moved, anc, _ = _host(case)
    copied, anc2, _ = _host(dict(case, delta=None))
    assert anc.tolist() == anc2.tolist() == [0, 1, 2]
    rc.minus_zero_check(moved, copied)
    _same((moved,), (rc.want(case)[0][0],))
    assert copied.tobytes() == case["poses"][0].tobytes()


def test_all_dead():
    for P, M in [(1, 1), (3, 5), (5, 3), (1500, 1500), (1025, 4000)]:
        w = np.zeros(P, np.uint32)
        poses = rc.some_poses(np.random.default_rng(P), 1, P)[0]
        out, anc, res = abi.resample_host(w, poses, M, 0xDEADBEEF)
        assert anc.tolist() == [j % P for j in range(M)] and out.tobytes() == poses[anc].tobytes()
        assert res.tolist() == [0, 0, 0, 0, 0, 0, min(M, P), 1]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_host_function_refusals():
    lib = abi.load_library()
    w = np.array([1, 2, 3], np.uint32)
    buf = np.full(64, 7.0, F32)          # poses at [0, 12), the outputs at [32, ...)
    anc = np.full(8, 77, np.uint32)
    res = np.full(8, 77, np.uint32)
    delta = np.array([1, 0, 0, 0] * 4, F32)
    at = lambda k: buf.ctypes.data + 4 * k  # noqa: E731

    def call(weights=w.ctypes.data, P=3, M=4, poses=None, dl=0, n_delta=0, out=None, res_=res.ctypes.data):
        return lib.rplgpu_resample_host(weights, P, M, 5, at(0) if poses is None else poses, dl, n_delta,
                                        at(32) if out is None else out, anc.ctypes.data, res_)

    bad = abi.ERR_INVALID_ARG
    assert call(weights=0) == bad and call(poses=0) == bad and call(out=0) == bad and call(res_=0) == bad
    assert call(P=0) == bad and call(M=0) == bad
    assert call(P=abi.MAX_POSES + 1) == bad and call(M=abi.MAX_POSES + 1) == bad
    assert call(dl=delta.ctypes.data, n_delta=0) == bad and call(dl=delta.ctypes.data, n_delta=2) == bad
    assert call(dl=delta.ctypes.data, n_delta=3) == bad
    assert call(out=at(0)) == bad and call(out=at(8)) == bad and call(out=at(11)) == bad   # the overlap
    assert call(poses=at(40)) == bad                                                       # ... from the other side
    assert (buf == 7.0).all() and (anc == 77).all() and (res == 77).all()
    assert call(out=at(12)) == abi.OK                                                      # adjacent is no overlap
    assert call(dl=delta.ctypes.data, n_delta=1) == abi.OK and call(dl=delta.ctypes.data, n_delta=4) == abi.OK
    assert call(n_delta=9) == abi.OK                                                       # n_delta unused without a delta
    assert res[0] == 6 and res[5] == 3
    with pytest.raises(abi.RplGpuError) as e:
        abi.resample_host(w, np.zeros((3, 4), F32), 0)
    assert e.value.code == bad
