"""Inputs for E16 (tests/test_resample_cpu.py, tests/test_gpu_resample.py) and their regime checks.  A case is a dict:
w (G, P) uint32, poses (L, P, 4) float32 with L in (1, G), u (G,) uint32 or None, M, delta None or (Ld, n_delta, 4)
float32 with Ld in (1, G) and n_delta in (1, M).  Every regime check is made from tests/resample_oracle.py alone and
says which path of the kernels the case is there for."""
import numpy as np

from tests import resample_oracle as ro

F32 = np.float32
U32_MAX = 0xFFFFFFFF
_WANT = {}


def mixed_weights(rng, P, zeros=0.3):
    """Weights over the whole uint32 range, small ones and a share of zeros; never all zero."""
    w = rng.integers(0, 1 << 32, P, dtype=np.uint64)
    w >>= rng.integers(0, 32, P).astype(np.uint64)
    w[rng.random(P) < zeros] = 0
    if not w.any():
        w[rng.integers(0, P)] = 1
    return w.astype(np.uint32)


def some_poses(rng, L, P):
    th = rng.uniform(-np.pi, np.pi, (L, P))
    q = np.empty((L, P, 4), F32)
    q[..., 0], q[..., 1] = np.cos(th), np.sin(th)
    q[..., 2:] = rng.uniform(-20, 20, (L, P, 2))
    return q


def make(seed, G, P, M, L=1, delta=None, u=True, w=None):
    rng = np.random.default_rng(seed)
    if w is None:
        w = np.stack([mixed_weights(rng, P) for _ in range(G)])
    w = np.ascontiguousarray(w, np.uint32).reshape(G, P)
    return dict(w=w, poses=some_poses(rng, L, P), M=M, delta=delta,
                u=rng.integers(0, 1 << 32, G, dtype=np.uint64).astype(np.uint32) if u is True else u)


def group_inputs(case, g):
    G = len(case["w"])
    poses = case["poses"][g if len(case["poses"]) == G and G > 1 else 0]
    u = 0 if case["u"] is None else int(case["u"][g])
    d = case["delta"]
    if d is not None:
        d = d[g if len(d) == G and G > 1 else 0]
    return case["w"][g], poses, case["M"], u, d


def want(case, key=None, writer=ro.ancestors_search):
    """[(poses_out, ancestors, result)] per group; cached under `key` (the first writer only)."""
    if key is not None and writer is ro.ancestors_search and key in _WANT:
        return _WANT[key]
    out = []
    for g in range(len(case["w"])):
        w, poses, M, u, d = group_inputs(case, g)
        out.append(ro.resample(w, poses, M, u, d, writer=writer))
    if key is not None and writer is ro.ancestors_search:
        _WANT[key] = out
    return out


def drawn(w, M, u):
    return np.bincount(ro.ancestors_search(w, M, u), minlength=len(w))


# ---- tile edges ---------------------------------------------------------------------------------------------------------
EDGE_P = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4096]


def edge_ms(P):
    return sorted({m for m in (1, P - 1, P, P + 1, 3 * P) if m > 0})


def edge_case(P, M):
    return make(1600 + P * 7 + M, 1, P, M)


def edge_regime(case):
    """mixed weights: zeros, small and large ones, and (beyond one pose) not every pose drawn equally often"""
    w = case["w"][0]
    assert w.any()
    if len(w) >= 63:
        assert (w == 0).any() and (w > 1 << 24).any() and (w < 1 << 12).any()
        k = drawn(w, case["M"], int(case["u"][0]))
        assert (k[w == 0] == 0).all()
        if case["M"] >= len(w):
            assert k.max() >= 2 and ((k == 0) & (w > 0)).any()  # a pose drawn twice, a live one dropped


# ---- dead stretches -------------------------------------------------------------------------------------------------------
DEAD_KINDS = ["first", "middle", "last", "only0", "only1023", "only1024", "onlylast"]
DEAD_P = 4096


def dead_case(kind):
    rng = np.random.default_rng(1650 + DEAD_KINDS.index(kind))
    w = mixed_weights(rng, DEAD_P)
    if kind == "first":
        w[:1024] = 0
    elif kind == "middle":
        w[1024:3072] = 0
    elif kind == "last":
        w[3072:] = 0
    else:
        at = {"only0": 0, "only1023": 1023, "only1024": 1024, "onlylast": DEAD_P - 1}[kind]
        w[:] = 0
        w[at] = 1 + rng.integers(0, 1 << 31)
    return make(1660, 1, DEAD_P, 3001, w=w)


def dead_regime(case, kind):
    """at least one tile gets no output; a single live pose gets all of them"""
    a = ro.ancestors_search(case["w"][0], case["M"], int(case["u"][0]))
    hit = set((a // ro.TILE).tolist())
    assert len(hit) < ro.tiles(DEAD_P)
    if kind.startswith("only"):
        assert len(set(a.tolist())) == 1 and len(hit) == 1
    else:
        gone = {"first": {0}, "middle": {1, 2}, "last": {3}}[kind]
        assert hit == set(range(4)) - gone


# ---- extremes ----------------------------------------------------------------------------------------------------------------
def allmax_case():
    return make(1670, 1, 2049, 2 * 2049 + 1, w=np.full(2049, U32_MAX, np.uint32))


def allmax_regime(case):
    """S needs its high word, every tile sum is above 2^41 and the sum of squares above 2^64"""
    S = ro.total(case["w"][0])
    assert S >> 32 >= 2048 and want(case, "allmax")[0][2][4] >= 2048


def small_case():
    rng = np.random.default_rng(1671)
    return make(1671, 1, 1100, 5000, w=(rng.random(1100) < 0.2).astype(np.uint32))


def small_regime(case):
    """S < M: q = 0 and every live pose is drawn several times"""
    S = ro.total(case["w"][0])
    assert 0 < S < case["M"] and S // case["M"] == 0
    k = drawn(case["w"][0], case["M"], int(case["u"][0]))
    assert (k[case["w"][0] > 0] >= 4).all()


def u_case(u):
    c = make(1672, 1, 1025, 1500)
    c["u"] = np.array([u], np.uint32)
    return c


def u_regime():
    """the two ends of u give different lists, and u = 2^32 - 1 puts r at S - 1 or just below"""
    a, b = u_case(0), u_case(U32_MAX)
    S = ro.total(a["w"][0])
    assert ro.r_of(0, S) == 0 and S - 1 - (S >> 32) <= ro.r_of(U32_MAX, S) <= S - 1
    assert want(a, "u0")[0][1].tobytes() != want(b, "umax")[0][1].tobytes()


WALK_M = 1 << 20


def walk_case():
    return make(1673, 1, 3, WALK_M, w=np.array([1, U32_MAX, 7], np.uint32))


def walk_regime(case):
    """one pose is drawn more than 1024 times: one workgroup walks (nearly) all M outputs"""
    k = drawn(case["w"][0], case["M"], int(case["u"][0]))
    assert k[1] > WALK_M - 8 and k[1] > 1024


BIG = 1 << 20


def big_case():
    rng = np.random.default_rng(1674)
    w = mixed_weights(rng, BIG)
    w[rng.random(BIG) < 0.75] = U32_MAX
    return make(1675, 1, BIG, BIG, w=w)


def big_regime(case):
    """S >= 2^51: the products behind r and t_j are as large as they get; 1024 tiles, poses dropped and doubled"""
    S = ro.total(case["w"][0])
    assert S >= 1 << 51
    a = want(case, "big")[0][1]
    k = np.bincount(a, minlength=BIG)
    assert k.max() >= 2 and (k == 0).sum() > BIG // 8 and len(set((a // ro.TILE).tolist())) == 1024


# ---- S = 0 ----------------------------------------------------------------------------------------------------------------------
ZERO_P = 1500
ZERO_M = [700, 1500, 4000]


def zero_case(M, P=ZERO_P):
    return make(1680 + M, 1, P, M, w=np.zeros(P, np.uint32))


def zero_regime(case):
    out, anc, res = want(case)[0]
    P, M = case["w"].shape[1], case["M"]
    assert res.tolist() == [0, 0, 0, 0, 0, 0, min(M, P), 1]
    assert anc.tolist() == [j % P for j in range(M)]


# ---- the move ----------------------------------------------------------------------------------------------------------------------
MOVE_P, MOVE_M = 1025, 1300
PAYLOADS = [0x7FA00001, 0xFFC12345, 0x7F800001, 0xFF812345, 0x7FFFFFFF]  # NaNs, quiet and signalling, with payloads
SPECIAL = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1e-42, 3e38, -3e38]


def move_case(n_delta, G=1, per_group=0, special=False):
    """n_delta: 0 (no delta), 1 or MOVE_M"""
    rng = np.random.default_rng(1690 + n_delta + 10 * G + per_group)
    c = make(1690 + G, G, MOVE_P, MOVE_M, L=G)
    if n_delta:
        Ld = G if per_group else 1
        th = rng.uniform(-0.2, 0.2, (Ld, n_delta))
        d = np.empty((Ld, n_delta, 4), F32)
        d[..., 0], d[..., 1] = np.cos(th), np.sin(th)
        d[..., 2:] = rng.uniform(-0.5, 0.5, (Ld, n_delta, 2))
        c["delta"] = d
    if special:
        flat = c["poses"].reshape(-1)
        at = rng.choice(flat.size, 400, replace=False)
        flat[at] = np.array(SPECIAL, F32)[rng.integers(0, len(SPECIAL), 400)]
        nan = c["poses"].view(np.uint32).reshape(-1)
        at = rng.choice(flat.size, 5, replace=False)
        nan[at] = PAYLOADS
        c["w"][:, (at // 4) % MOVE_P] = U32_MAX >> 1  # the poses that carry them are heavy: each is drawn
        if n_delta == 1:  # one delta serves a whole group: one special entry each, -0 / Inf / NaN by group
            for g in range(len(c["delta"])):
                c["delta"][g, 0, 3 - g % 3] = [-0.0, float("inf"), float("nan")][g % 3]
        elif n_delta:
            dflat = c["delta"].reshape(-1)
            at = rng.choice(dflat.size, dflat.size // 6, replace=False)
            dflat[at] = np.array(SPECIAL, F32)[rng.integers(0, len(SPECIAL), len(at))]
    return c


def move_regime(case, special):
    """with special values: NaN payloads, infinities and -0 reach the output of a copy unchanged; a move makes NaNs
    (every one stored as 0x7FC00000) and infinities"""
    out = np.concatenate([o for o, _, _ in want(case)]).view(np.uint32).reshape(-1)
    f = out.view(F32)
    if not special:
        assert np.isfinite(f).all()
        return
    if case["delta"] is None:
        assert set(PAYLOADS) <= set(out.tolist())
        assert (out == 0x80000000).any() and np.isinf(f).any()
    else:
        nan = out[np.isnan(f)]
        assert len(nan) and (nan == ro.QNAN).all() and np.isinf(f).any()


def minus_zero_case():
    """c = -0 with a negative s under the identity delta: -0 * 1 - s * 0 = -0 - -0 = +0"""
    poses = np.array([[[-0.0, -1.0, 3.0, 4.0], [-0.0, 1.0, 3.0, 4.0], [1.0, -0.0, -0.0, -0.0]]], F32)
    return dict(w=np.array([[1, 1, 1]], np.uint32), poses=poses, M=3, u=None,
                delta=np.array([[[1.0, 0.0, 0.0, 0.0]]], F32))


def minus_zero_check(out_moved, out_copied):
    assert out_copied.view(np.uint32)[0, 0] == 0x80000000 and out_moved.view(np.uint32)[0, 0] == 0  # -0 became +0
    assert out_moved.view(np.uint32)[1, 0] == 0x80000000   # a positive s: -0 - +0 stays -0
    assert out_moved[:, 1:].tobytes() != out_copied[:, 1:].tobytes()  # (s = -0 + +0 = +0 in pose 2 as well)
    assert (out_moved == out_copied).all()                 # numerically the identity


# ---- groups ------------------------------------------------------------------------------------------------------------------------
GROUPS = 101


def groups_case(ppg):
    rng = np.random.default_rng(1700)
    P = 1100
    w = np.stack([mixed_weights(rng, P) >> np.uint32(g % 29) for g in range(GROUPS)])
    w[7] = 0           # one dead group among them
    w[8, 1:] = 0       # and one with a single live pose
    w[8, 0] = 5
    return make(1701, GROUPS, P, 1300, L=GROUPS if ppg else 1, w=w)


def groups_regime(case):
    res = [r for _, _, r in want(case, f"groups{len(case['poses'])}")]
    assert len({(int(r[0]), int(r[1])) for r in res}) >= GROUPS - 2 and len(set(case["u"].tolist())) == GROUPS
    assert res[7][7] == 1 and res[8][6] == 1 and sum(int(r[7]) for r in res) == 1


# ---- result words ----------------------------------------------------------------------------------------------------------------
def words_case():
    w = np.zeros(2500, np.uint32)
    w[[0, 1023, 1024, 2047, 2499]] = [U32_MAX, U32_MAX, 0xFFFF0000, 3, U32_MAX]
    w[100:200] = 0x80000000
    return make(1710, 1, 2500, 2500, w=w)


def words_regime(case):
    """the sum of squares needs its third word, carried both inside a tile and between tiles"""
    res = want(case, "words")[0][2]
    assert res[4] >= 3 and res[5] == 105 and 0 < res[6] < 105 + 1 and res[1] > 0


WIDE_P = 66600  # 66 tiles: the scan kernel's threads of two waves hold tile sums


def words_wide_case():
    w = np.zeros(WIDE_P, np.uint32)
    w[[0, 65536, 66560]] = U32_MAX   # tiles 0, 64 and 65
    w[30000:30100] = 1000
    return make(1711, 1, WIDE_P, 3000, w=w)


def words_wide_regime(case):
    """the low 64 bits of the squares wrap between tiles 64 and 65 (one wave of the scan kernel) and again between
    that wave's total and the first wave's"""
    w = case["w"][0].astype(object)
    lo = lambda a, b: int((w[a:b] ** 2).sum()) & ro.MASK64  # noqa: E731
    first, second = lo(0, 65536), lo(65536, WIDE_P)
    assert lo(65536, 66560) + lo(66560, WIDE_P) > ro.MASK64 and first + second > ro.MASK64
    assert want(case, "words_wide")[0][2][4] == 2


# ---- the 64-bit forms ---------------------------------------------------------------------------------------------------------------
def form_samples(rng, n):
    for _ in range(n):
        P = int(rng.integers(1, 40))
        M = int(rng.integers(1, 90))
        yield mixed_weights(rng, P, zeros=float(rng.random()) * 0.8), M, int(rng.integers(0, 1 << 32))
