"""The inputs of the E20 tests (tests/test_bins_cpu.py, tests/test_gpu_bins.py).  A case is a dict: ``spec``
(bins_oracle.Spec), ``edges`` (T, 2), ``lists`` (one (P, 4) pose array, shared by every group, or one per group),
``weights`` (per group a (P,) uint32 array or None for no weights at all), ``maps`` (per group the map KEEP ORs into,
or None).  ``want(case, name)`` is the oracle's answer per group, made once; every ``*_regime`` asserts from the oracle
alone that the case is what its name says, before any comparison."""
import numpy as np

from tests import bins_oracle as bo

F32 = np.float32
NONE = bo.NONE
EDGE_P = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4096)     # E18's tile edges
NB_SIZES = (1, 31, 32, 33, 63, 64, 65)
T_SIZES = (1, 2, 36, 1024)
_WANT = {}


def groups(case):
    return len(case["weights"])


def want(case, name, both=None):
    """-> per group (map, bins, result), the oracle's; made once per name and never changed"""
    if name not in _WANT:
        out = []
        for g in range(groups(case)):
            poses = case["lists"][g if len(case["lists"]) > 1 else 0]
            m = case["maps"][g] if case.get("maps") else None
            out.append(bo.bin_poses(case["spec"], poses, case["weights"][g], case["edges"], m, both=both))
        for o in out:
            for a in o:
                a.setflags(write=False)
        _WANT[name] = out
    return _WANT[name]


def make(spec, edges, lists, weights=None, maps=None):
    lists = [np.ascontiguousarray(p, F32).reshape(-1, 4) for p in lists]
    if weights is None:
        weights = [None] * len(lists)
    return dict(spec=spec, edges=np.ascontiguousarray(edges, F32), lists=lists, weights=list(weights), maps=maps)


def centres(s, T, ids, rng=None):
    """poses in the middle of the bins `ids` (with rng: anywhere in the middle half of them)"""
    ids = np.asarray(ids, np.int64)
    bx, by, kt = ids % s.nx, ids // s.nx % s.ny, ids // (s.nx * s.ny)
    j = 0.5 if rng is None else rng.uniform(0.25, 0.75, (3, len(ids)))
    jx, jy, ja = (j, j, j) if rng is None else j
    a = 2.0 * np.pi * (kt + ja) / T
    x = s.origin_x + (bx + jx) / s.inv_size
    y = s.origin_y + (by + jy) / s.inv_size
    return np.stack([np.cos(a), np.sin(a), x, y], axis=1).astype(F32)


def spread(s, T, P, rng, margin=0.0):
    """P poses uniform over the bins' extent (with a margin: some outside), any heading"""
    a = rng.uniform(0.0, 2.0 * np.pi, P)
    x = s.origin_x + rng.uniform(-margin, s.nx + margin, P) / s.inv_size
    y = s.origin_y + rng.uniform(-margin, s.ny + margin, P) / s.inv_size
    return np.stack([np.cos(a), np.sin(a), x, y], axis=1).astype(F32)


# ---- P ------------------------------------------------------------------------------------------------------------------
def edge_case(P):
    rng = np.random.default_rng(2000 + P)
    s = bo.spec(-1.75, -1.75, 2.0, 7, 7)
    lists = [spread(s, 5, P, rng, margin=0.4), spread(s, 5, P, rng, margin=0.4)]
    w = [rng.integers(0, 4, P).astype(np.uint32), None]
    w[0][0] = 7
    return make(s, bo.table(5), lists, w)


def edge_regime(case, w):
    P = len(case["lists"][0])
    for m, bins, res in w:
        assert int(res[1]) + int(res[2]) + int(res[3]) == P
    assert int(w[0][2][1]) + int(w[1][2][1]) > 0
    if P >= 63:
        assert int(w[1][2][0]) > 8 and int(w[1][2][2]) > 0 and int(w[0][2][3]) > 0


# ---- NB -----------------------------------------------------------------------------------------------------------------
def nb_case(NB):
    rng = np.random.default_rng(3000 + NB)
    s = bo.spec(0.0, 0.0, 2.0, NB, 1)
    ids = np.concatenate([np.arange(NB), rng.integers(0, NB, 2 * NB)])
    return make(s, bo.table(1), [centres(s, 1, rng.permutation(ids))])


def nb_regime(case, w):
    NB = case["spec"].nx
    m, bins, res = w[0]
    assert len(m) == (NB + 31) // 32
    assert int(res[5]) == NB - 1 and int(res[4]) == 0 and int(res[0]) == NB       # the highest bin is occupied
    assert int(m[-1]) == (1 << ((NB - 1) % 32 + 1)) - 1


def two_bins_case():
    s = bo.spec(0.0, 0.0, 2.0, 64, 1)
    return make(s, bo.table(1), [centres(s, 1, [32, 31, 31, 32, 32])])


def two_bins_regime(case, w):
    assert w[0][0].tolist() == [0x80000000, 0x00000001] and int(w[0][2][0]) == 2


def one_bin_case():
    s = bo.spec()
    rng = np.random.default_rng(41)
    return make(s, bo.table(36), [centres(s, 36, np.full(65536, (17 * 103 + 40) * 103 + 61), rng)])


def one_bin_regime(case, w):
    m, bins, res = w[0]
    assert int(res[0]) == 1 and int(res[1]) == 65536 and int(res[4]) == int(res[5])


def one_word_case():
    s = bo.spec(-2.0, -1.0, 2.0, 8, 4)
    rng = np.random.default_rng(42)
    ids = np.concatenate([np.arange(32, 64), rng.integers(32, 64, 4096 - 32)])
    return make(s, bo.table(3), [centres(s, 3, rng.permutation(ids), rng)])


def one_word_regime(case, w):
    m, bins, res = w[0]
    assert int(res[0]) == 32 and m.tolist() == [0, 0xFFFFFFFF, 0] and int(res[1]) == 4096


def own_bin_case():
    s = bo.spec(-16.0, -16.0, 2.0, 64, 64)
    rng = np.random.default_rng(43)
    return make(s, bo.table(1), [centres(s, 1, rng.permutation(4096))])


def own_bin_regime(case, w):
    m, bins, res = w[0]
    assert int(res[0]) == 4096 and (m == 0xFFFFFFFF).all() and len(set(bins.tolist())) == 4096


# ---- positions ----------------------------------------------------------------------------------------------------------
def _down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def positions_case():
    """bins of 0.5 m from (0, 0), 5 x 4: the values below on x with y mid-bin, then on y with x mid-bin; a second list
    under the same spec is not possible for another origin, so the far origin is positions_far_case"""
    s = bo.spec(0.0, 0.0, 2.0, 5, 4)
    xs = [1.0, _down(1.0), 0.0, -0.0, _down(2.5), 2.5, -0.25, _down(0.0), np.nan, np.inf, -np.inf, 1e30, 2.4999]
    ys = [1.0, _down(1.0), 0.0, -0.0, _down(2.0), 2.0, -0.25, _down(0.0), np.nan, np.inf, -np.inf, -1e30, 1.9999]
    rows = [(1.0, 0.0, x, 0.75) for x in xs] + [(1.0, 0.0, 1.25, y) for y in ys]
    return make(s, bo.table(1), [np.array(rows, F32)])


def positions_regime(case, w):
    m, bins, res = w[0]
    b = bins.tolist()
    #          edge  below  origin  -0   top  at-top  neg  tiny-neg  nan  inf  -inf  huge  inside
    assert b[:13] == [7, 6, 5, 5, 9, NONE, NONE, NONE, NONE, NONE, NONE, NONE, 9]
    assert b[13:] == [12, 7, 2, 2, 17, NONE, NONE, NONE, NONE, NONE, NONE, NONE, 17]
    assert int(res[2]) == 14 and int(res[7]) & 2


def positions_far_case():
    """an origin of (10^6, -10^6): float32 has steps of 1 / 16 there, bins of 0.5 m hold eight of them"""
    s = bo.spec(1.0e6, -1.0e6, 2.0, 6, 6)
    rng = np.random.default_rng(44)
    x = F32(1.0e6) + (rng.integers(-4, 52, 300) / 16.0).astype(F32)
    y = F32(-1.0e6) + (rng.integers(-4, 52, 300) / 16.0).astype(F32)
    a = rng.uniform(0, 2 * np.pi, 300)
    return make(s, bo.table(4), [np.stack([np.cos(a), np.sin(a), x, y], axis=1).astype(F32)])


def positions_far_regime(case, w):
    m, bins, res = w[0]
    assert int(res[0]) > 100 and int(res[2]) > 10 and int(res[1]) > 200


# ---- headings -----------------------------------------------------------------------------------------------------------
def headings_case():
    """T = 36 over 2 x 1 bins: every edge itself, then the special vectors"""
    s = bo.spec(0.0, 0.0, 2.0, 2, 1)
    t = bo.table(36)
    rows = [(c, v, 0.25, 0.25) for c, v in t]
    e = t[5]
    up, dn = F32(np.inf), F32(-np.inf)
    special = [(e[0], np.nextafter(e[1], up)), (e[0], np.nextafter(e[1], dn)), (np.nextafter(e[0], up), e[1]),
               (np.nextafter(e[0], dn), e[1]), (-1.0, 0.0), (-1.0, -0.0), (t[7][0] * F32(0.5), t[7][1] * F32(0.5)),
               (t[7][0] * F32(2.0), t[7][1] * F32(2.0)), (0.0, 0.0), (1e-8, -1e-8), (8.0, 0.0), (0.0, -8.0),
               (_down(8.0), 0.0), (np.nan, 1.0), (1.0, np.inf), (1.0, -0.75 * 2.0 ** -20), (1.0, -2.0 ** -21),
               (e[0], e[1] - F32(2.0 ** -20)), (e[0], e[1] + F32(2.0 ** -20))]
    rows += [(c, v, 0.75, 0.25) for c, v in special]
    return make(s, t, [np.array(rows, F32)])


def headings_regime(case, w):
    m, bins, res = w[0]
    b = bins.tolist()
    assert b[:36] == [2 * k for k in range(36)]                       # bin k for edge k
    sp = b[36:]
    # the float32 neighbours of edge 5 are a sixteenth of the quantisation step away: on the edge or across it
    assert sp[0] == 11 and sp[2] in (9, 11) and sp[1] in (9, 11) and sp[3] == 11
    assert sp[17] == 9 and sp[18] == 11                                # one quantisation step across edge 5, both ways
    assert sp[4] == sp[5] == 2 * 18 + 1                                # (-1, 0) and (-1, -0.0): edge 18 itself
    assert sp[6] in (13, 15) and sp[7] in (13, 15)                     # half and double length: rounded anew
    assert sp[8] == sp[9] == sp[10] == sp[11] == NONE                  # (0, 0), rounds to (0, 0), out of range twice
    assert sp[12] == 1 and sp[13] == sp[14] == NONE                    # just inside the range; NaN; Inf
    assert sp[15] == 2 * 35 + 1 and sp[16] == 1                        # S = -3 / 4 -> -1: the last bin; -1 / 2 -> -0


def t_case(T, valid=True):
    rng = np.random.default_rng(5000 + T)
    s = bo.spec(-1.0, -1.0, 2.0, 2, 2)
    t = bo.table(T)
    n = 600 if T <= 36 else 150
    p = spread(s, T, n, rng)
    every = t if T <= 36 else np.concatenate([t[::3], t[-1:]])
    on = np.concatenate([every, -t[: min(T, 64)], t[: min(T, 64)] * F32(0.5)])
    q = np.zeros((len(on), 4), F32)
    q[:, :2] = on
    q[:, 2:] = (-0.75, -0.25)
    if not valid:
        t = t.copy()
        t[[3, 20]] = t[[20, 3]]
        t[11] = (np.nan, 0.0)
    return make(s, t, [np.concatenate([p, q])])


def t_regime(case, w, valid=True):
    m, bins, res = w[0]
    T = len(case["edges"])
    assert bo.valid_table(case["edges"]) == valid
    kt = bins[bins != NONE] // 4
    assert len(set(kt.tolist())) >= min(T, 30) * (1 if valid else 0.5) and int(kt.max()) <= T - 1
    if valid:
        assert int(kt.max()) == T - 1


# ---- weights, groups ----------------------------------------------------------------------------------------------------
def weights_case(kind):
    rng = np.random.default_rng(45)
    s = bo.spec(-2.0, -2.0, 2.0, 8, 8)
    p = spread(s, 6, 1500, rng, margin=0.5)
    w = dict(none=None, zero=np.zeros(1500, np.uint32),
             mixed=(rng.integers(0, 3, 1500) * rng.integers(0, 2 ** 31, 1500)).astype(np.uint32))[kind]
    return make(s, bo.table(6), [p], [w])


def weights_regime(kind, case, w):
    m, bins, res = w[0]
    if kind == "zero":
        assert int(res[7]) == 1 and not m.any() and int(res[4]) == NONE and int(res[5]) == 0 and int(res[3]) == 1500
    elif kind == "none":
        assert int(res[3]) == 0 and int(res[2]) > 0 and int(res[1]) > 1000
    else:
        assert int(res[3]) > 300 and int(res[2]) > 0 and int(res[1]) > 500
        # some pose is both skipped and out of range, and counts as skipped
        both = (case["weights"][0] == 0) & (bo.writer_a(case["spec"], case["lists"][0], None, case["edges"])[1] == NONE)
        assert both.any()


def groups_case(shared):
    rng = np.random.default_rng(46 + shared)
    s = bo.spec(-3.0, -2.0, 2.0, 11, 9)
    P = 1300
    w = [rng.integers(0, 2, P).astype(np.uint32), rng.integers(0, 5, P).astype(np.uint32), None]
    if shared:
        w[2] = np.ones(P, np.uint32)
        return make(s, bo.table(7), [spread(s, 7, P, rng, margin=0.3)], w)
    return make(s, bo.table(7), [spread(s, 7, P, rng, margin=0.3) for _ in range(3)], w)


def groups_regime(case, w):
    maps = [x[0].tobytes() for x in w]
    assert len(set(maps)) == 3 and all(int(x[2][0]) > 50 for x in w)


# ---- KEEP ---------------------------------------------------------------------------------------------------------------
def keep_case():
    """one list of 3000 poses, and the map a test pre-fills: every third bin of the first half"""
    rng = np.random.default_rng(47)
    s = bo.spec(-2.0, -2.0, 2.0, 9, 7)
    T = 5
    p = spread(s, T, 3000, rng, margin=0.2)
    pre = np.zeros(bo.map_words(s, T), np.uint32)
    for b in range(0, s.nx * s.ny * T // 2, 3):
        pre[b >> 5] |= np.uint32(1 << (b & 31))
    return make(s._replace(keep=1), bo.table(T), [p], [None], [pre])


def keep_regime(case, w):
    m, bins, res = w[0]
    occupied = len(set(bins[bins != NONE].tolist()))
    pre = case["maps"][0]
    assert int(res[7]) & 4 and 0 < int(res[0]) < occupied and (m & pre).tobytes() == pre.tobytes()


# ---- large --------------------------------------------------------------------------------------------------------------
def large_case():
    rng = np.random.default_rng(48)
    s = bo.spec()
    return make(s, bo.table(36), [spread(s, 36, 1 << 20, rng, margin=0.01)])


def large_regime(case, w):
    m, bins, res = w[0]
    assert int(res[0]) > 300000 and int(res[1]) > 1000000 and int(res[2]) > 0


def widest_case():
    """NB = 2^26: 256 x 256 bins by 1024 headings, 4096 poses that reach the first and the last map word"""
    rng = np.random.default_rng(49)
    s = bo.spec(-64.0, -64.0, 2.0, 256, 256)
    ids = rng.integers(0, 1 << 26, 4096)
    ids[:4] = (0, 31, (1 << 26) - 1, (1 << 26) - 32)
    return make(s, bo.table(1024), [centres(s, 1024, rng.permutation(ids), rng)])


def widest_regime(case, w):
    m, bins, res = w[0]
    assert len(m) == 1 << 21 and m[0] and m[-1] and int(res[4]) == 0 and int(res[5]) == (1 << 26) - 1
    assert int(res[1]) == 4096 and int(res[0]) > 4000


# ---- random inputs (tests/test_bins_cpu.py) -------------------------------------------------------------------------------
def random_case(seed):
    rng = np.random.default_rng(7000 + seed)
    T = int(rng.choice([1, 2, 3, 4, 7, 36, 72]))
    scale = float(rng.choice([0.0, 1.0, 100.0, 1.0e5]))
    s = bo.spec(rng.uniform(-1, 1) * scale, rng.uniform(-1, 1) * scale, float(rng.choice([0.5, 1.0, 2.0, 3.3, 10.0])),
                int(rng.integers(1, 12)), int(rng.integers(1, 12)), keep=int(rng.integers(0, 2)))
    P = int(rng.integers(1, 300))
    p = spread(s, T, P, rng, margin=0.5)
    p[:, :2] *= rng.uniform(0.3, 3.0, (P, 1)).astype(F32)
    bad = rng.integers(0, P, max(P // 20, 1))
    p[bad, rng.integers(0, 4, len(bad))] = rng.choice([np.nan, np.inf, -np.inf, 0.0], len(bad))
    w = None if seed % 4 == 0 else (rng.integers(0, 3, P) * rng.integers(1, 2 ** 31, P)).astype(np.uint32)
    pre = rng.integers(0, 2 ** 32, bo.map_words(s, T), dtype=np.uint64).astype(np.uint32) & \
        rng.integers(0, 2 ** 32, bo.map_words(s, T), dtype=np.uint64).astype(np.uint32)
    last = s.nx * s.ny * T % 32
    if last:
        pre[-1] &= np.uint32((1 << last) - 1)
    return make(s, bo.table(T), [p], [w], [pre] if s.keep else None)
