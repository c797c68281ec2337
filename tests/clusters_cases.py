"""The inputs of the E21 tests (tests/test_clusters_cpu.py, tests/test_gpu_clusters.py).  A case is a dict: ``nx``,
``ny``, ``T``, ``wrap``, ``xy_scale``, ``groups`` (per group a dict of ``poses`` (P, 4), ``weights`` (P,) uint32 or
None, ``map`` and ``bins`` (P,)), ``shared`` (every group reads group 0's poses) and ``regime``, a check computed from
the oracle alone that the case is what its name says.  ``get(name)`` builds a case once, ``want(name)`` is the oracle's
answer per group, made once and never changed."""
import numpy as np

from tests import bins_cases as bc
from tests import bins_oracle as bo
from tests import clusters_oracle as co

F32 = np.float32
NONE = co.NONE
EDGE_P = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
NB_SHAPES = {31: (31, 1, 1), 32: (8, 4, 1), 33: (11, 3, 1), 64: (4, 4, 4)}
_CASES, _WANT = {}, {}


def bin_id(nx, ny, x, y, k):
    return (k * ny + y) * nx + x


def group(nx, ny, T, pose_ids, extra=(), weights=None, rng=None):
    """poses in the bins `pose_ids` (bins of 0.5 m from the origin), the map of those bins and of `extra`"""
    s = bo.spec(0.0, 0.0, 2.0, nx, ny)
    pose_ids = np.asarray(pose_ids, np.int64)
    return dict(poses=bc.centres(s, T, pose_ids, rng), weights=None if weights is None else np.asarray(weights, np.uint32),
                map=co.map_of(nx, ny, T, list(pose_ids.tolist()) + list(extra)), bins=pose_ids.astype(np.uint32))


def make(nx, ny, T, groups, regime, wrap=1, xy_scale=1024.0, shared=False):
    return dict(nx=nx, ny=ny, T=T, wrap=wrap, xy_scale=xy_scale, groups=groups, regime=regime, shared=shared)


def get(name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def want(name):
    if name not in _WANT:
        c = get(name)
        out = [co.cluster(g, c["nx"], c["ny"], c["T"], c["wrap"], c["xy_scale"]) for g in c["groups"]]
        for o in out:
            for a in o:
                a.setflags(write=False)
        _WANT[name] = out
    return _WANT[name]


def check_regime(name):
    get(name)["regime"](get(name), want(name))


def n_c(w, g=0):
    return int(w[g][2][6])


def flags(w, g=0):
    return int(w[g][2][0])


def blob(nx, ny, x0, y0, k0, dx, dy, dk):
    return [bin_id(nx, ny, x, y, k) for k in range(k0, k0 + dk) for y in range(y0, y0 + dy) for x in range(x0, x0 + dx)]


# ---- tile and wave edges ----------------------------------------------------------------------------------------------------
def edge_case(P):
    def build():
        rng = np.random.default_rng(100 + P)
        ids = blob(16, 16, 1, 1, 0, 3, 3, 2) + blob(16, 16, 8, 8, 1, 4, 2, 2) + blob(16, 16, 12, 2, 3, 2, 2, 1)
        w = rng.integers(0, 1000, P).astype(np.uint32)

        def regime(c, w_):
            assert len(c["groups"][0]["poses"]) == P and (n_c(w_) >= 2 or P == 1) and not flags(w_) & 32

        return make(16, 16, 4, [group(16, 16, 4, rng.choice(ids, P), weights=w, rng=rng)], regime, wrap=0)
    return build


# ---- map word and index-block edges -------------------------------------------------------------------------------------------
def nb_case(NB):
    def build():
        nx, ny, T = NB_SHAPES[NB]
        rng = np.random.default_rng(200 + NB)
        occ = rng.permutation(NB)[:NB // 2]
        extra = occ.tolist() + [NB - 1]                             # the last bin of the map among them

        def regime(c, w_):
            assert c["nx"] * c["ny"] * c["T"] == NB and len(c["groups"][0]["map"]) == (NB + 31) // 32
            assert int(w_[0][2][7]) >= NB // 2

        return make(nx, ny, T, [group(nx, ny, T, rng.choice(occ, 40), extra, rng=rng)], regime)
    return build


def blocks_case():
    nx, ny, T = 64, 64, 33                                          # 4224 map words: five index blocks of 1024
    rng = np.random.default_rng(301)
    pair_block = [bin_id(nx, ny, 10, 10, 7), bin_id(nx, ny, 10, 10, 8)]      # words 916 and 1044
    pair_word = [bin_id(nx, ny, 31, 0, 0), bin_id(nx, ny, 32, 0, 0)]         # words 0 and 1
    ids = np.array(pair_block + pair_word + rng.permutation(nx * ny * T)[:3000].tolist())

    def regime(c, w_):
        assert len(c["groups"][0]["map"]) == 4224 and int(w_[0][2][7]) > 2048       # ranks beyond two rank blocks too
        for a, b in (pair_block, pair_word):
            assert b in co.neighbours(a, nx, ny, T, 1)
        assert pair_block[0] >> 15 != pair_block[1] >> 15 and pair_word[0] >> 5 != pair_word[1] >> 5
        lab = dict(zip(c["groups"][0]["bins"].tolist(), w_[0][0].tolist()))
        assert lab[pair_block[0]] == lab[pair_block[1]] and lab[pair_word[0]] == lab[pair_word[1]]
        # ranks (the place among the occupied ids): a neighbour pair whose ranks lie in different blocks of 1024 ranks
        occ = co.occupied_ids(c["groups"][0]["map"], nx * ny * T)
        rank = {int(b): r for r, b in enumerate(occ.tolist())}
        split = [(a, b) for a in rank for b in co.neighbours(a, nx, ny, T, 1) if b in rank and rank[a] >> 10 != rank[b] >> 10]
        assert split and any(lab.get(a) is not None and lab.get(a) == lab.get(b) for a, b in split), len(split)

    picks = np.concatenate([ids[:4], rng.choice(ids, 1496)])
    return make(nx, ny, T, [group(nx, ny, T, picks, ids.tolist(), rng=rng)], regime)


# ---- seams, connectivity, wrap ------------------------------------------------------------------------------------------------
def _ids_case(nx, ny, T, ids, wrap, count):
    def build():
        def regime(c, w_):
            assert n_c(w_) == count, n_c(w_)

        return make(nx, ny, T, [group(nx, ny, T, ids)], regime, wrap=wrap)
    return build


SMALL = {
    "row_seam": (5, 4, 3, [bin_id(5, 4, 4, 1, 0), bin_id(5, 4, 0, 2, 0)], 1, 2),
    "layer_seam": (5, 4, 3, [bin_id(5, 4, 4, 3, 0), bin_id(5, 4, 0, 0, 1)], 1, 2),
    "diagonal": (4, 4, 4, [bin_id(4, 4, 1, 1, 1), bin_id(4, 4, 2, 2, 2)], 0, 1),
    "apart_x": (5, 4, 4, [bin_id(5, 4, 1, 1, 1), bin_id(5, 4, 3, 1, 1)], 0, 2),
    "apart_y": (5, 4, 4, [bin_id(5, 4, 1, 1, 1), bin_id(5, 4, 1, 3, 1)], 0, 2),
    "apart_k": (5, 4, 4, [bin_id(5, 4, 1, 1, 1), bin_id(5, 4, 1, 1, 3)], 1, 2),
    "wrap_on": (4, 4, 5, [bin_id(4, 4, 1, 1, 0), bin_id(4, 4, 2, 2, 4)], 1, 1),
    "wrap_off": (4, 4, 5, [bin_id(4, 4, 1, 1, 0), bin_id(4, 4, 2, 2, 4)], 0, 2),
    "t1_wrap": (6, 5, 1, [0, 1, 7, 4, 29], 1, 3),
    "t1_plain": (6, 5, 1, [0, 1, 7, 4, 29], 0, 3),
    "t2_wrap": (3, 3, 2, [bin_id(3, 3, 0, 0, 0), bin_id(3, 3, 1, 1, 1), bin_id(3, 3, 2, 2, 0)], 1, 1),
    "t2_plain": (3, 3, 2, [bin_id(3, 3, 0, 0, 0), bin_id(3, 3, 1, 1, 1), bin_id(3, 3, 2, 2, 0)], 0, 1),
    "nx1": (1, 5, 3, [bin_id(1, 5, 0, 0, 0), bin_id(1, 5, 0, 1, 2), bin_id(1, 5, 0, 4, 1)], 1, 2),
    "ny1": (5, 1, 3, [bin_id(5, 1, 0, 0, 0), bin_id(5, 1, 1, 0, 2), bin_id(5, 1, 4, 0, 1)], 0, 3),
}


# ---- long chains ----------------------------------------------------------------------------------------------------------------
def serpentine_ids(nx, ny, k, n):
    ids = []
    for y in range(0, n, 2):
        ids += [bin_id(nx, ny, x, y, k) for x in range(n)]
        if y + 1 < n:
            ids.append(bin_id(nx, ny, n - 1 if (y // 2) % 2 == 0 else 0, y + 1, k))
    return ids


def _chain(nx, ny, T, ids, wrap, seed):
    def build():
        rng = np.random.default_rng(seed)

        def regime(c, w_):
            assert n_c(w_) == 1 and not flags(w_) & 32
            assert co.diameter_at_least(c["groups"][0]["map"], nx, ny, T, wrap) >= 200

        return make(nx, ny, T, [group(nx, ny, T, rng.choice(ids, 700), ids, rng=rng)], regime, wrap=wrap)
    return build


def spiral_ids():
    """a serpentine in every second of 9 heading layers, one bin in the layers between: at the serpentine's far end
    and at its near end in turn"""
    n = 15
    ids = []
    ends = [bin_id(n, n, 0, 0, 0), bin_id(n, n, 0, n - 1, 0)]         # 8 full rows: the last one runs back to (0, 14)
    for k in range(0, 9, 2):
        ids += [i + k * n * n for i in serpentine_ids(n, n, 0, n)]
        if k + 1 < 9:
            ids.append(ends[1 - (k // 2) % 2] + (k + 1) * n * n)
    return ids


def comb_ids():
    n = 128
    ids = [bin_id(n, n, x, n - 1, 0) for x in range(n)]
    for x in range(0, n, 2):
        ids += [bin_id(n, n, x, y, 0) for y in range(n - 1)]
    return ids


# ---- KEEP maps ----------------------------------------------------------------------------------------------------------------------
def bridge_case():
    left, right = blob(8, 3, 0, 0, 0, 2, 2, 1), blob(8, 3, 3, 0, 0, 2, 2, 1)
    bridge = [bin_id(8, 3, 2, 1, 0)]

    def regime(c, w_):
        g = dict(c["groups"][0], map=co.map_of(8, 3, 2, left + right))
        assert n_c([co.cluster(g, 8, 3, 2, 1)]) == 2 and n_c(w_) == 1 and int(w_[0][2][7]) == 9

    return make(8, 3, 2, [group(8, 3, 2, left + right + left, bridge)], regime)


def map_only_case():
    a, ghost, b = blob(9, 3, 0, 0, 0, 2, 2, 1), blob(9, 3, 4, 0, 1, 1, 2, 1), blob(9, 3, 7, 1, 2, 2, 2, 1)

    def regime(c, w_):
        assert n_c(w_) == 3 and w_[0][1][1].tolist() == [ghost[0], 0, 0, 0] and flags(w_) == 0

    return make(9, 3, 3, [group(9, 3, 3, a + b + b, ghost)], regime, wrap=0)


# ---- stray and unlabelled entries -------------------------------------------------------------------------------------------------
def strays_case():
    nx, ny, T = 7, 5, 3
    rng = np.random.default_rng(501)
    ids = blob(nx, ny, 0, 0, 0, 2, 2, 1) + blob(nx, ny, 4, 2, 1, 2, 2, 2)
    g = group(nx, ny, T, rng.choice(ids, 300), rng=rng)
    clear = bin_id(nx, ny, 6, 4, 0)                                 # a bin whose bit is not set
    g["bins"][5:300:9] = nx * ny * T                                # the first id past the map
    g["bins"][6:300:9] = 0xFFFFFFFE
    g["bins"][7:300:9] = clear
    g["bins"][8:300:9] = NONE

    def regime(c, w_):
        r = w_[0][2]
        assert int(r[76]) == 99 and int(r[77]) == 33 and flags(w_) & 16 and n_c(w_) == 2
        assert int(r[2]) == 300 - 132 and (w_[0][0][5:300:9] == NONE).all() and (w_[0][0][7:300:9] == NONE).all()

    return make(nx, ny, T, [g], regime)


def empty_case():
    g = group(6, 6, 2, [0] * 70)
    g["map"][:] = 0
    g["bins"][:] = NONE

    def regime(c, w_):
        r = w_[0][2]
        assert n_c(w_) == 0 and int(r[7]) == 0 and flags(w_) == 1 | 4 | 8 and int(r[1]) == NONE == int(r[72])
        assert int(r[77]) == 70

    return make(6, 6, 2, [g], regime)


# ---- the choice of BEST -----------------------------------------------------------------------------------------------------------
def _two(nx=12, ny=4, T=2):
    return blob(nx, ny, 0, 0, 0, 2, 2, 1), blob(nx, ny, 8, 1, 1, 2, 2, 1)


def tie_case():
    a, b = _two()
    ids = a * 3 + b * 4                                             # 12 and 16 poses
    w = [4] * 12 + [3] * 16

    def regime(c, w_):
        t = w_[0][1]
        assert n_c(w_) == 2 and int(t[0][2]) == int(t[1][2]) == 48 and int(w_[0][2][1]) == int(t[0][0]) < int(t[1][0])
        assert int(w_[0][2][72]) == int(t[1][0])

    return make(12, 4, 2, [group(12, 4, 2, ids, weights=w)], regime, wrap=0)


def heavy_few_case():
    a, b = _two()
    ids = a * 10 + b[:3]
    w = [1] * 40 + [1000, 0, 7]

    def regime(c, w_):
        t, r = w_[0][1], w_[0][2]
        assert int(r[1]) == int(t[1][0]) and int(t[1][1]) == 3 < int(t[0][1]) == 40 and int(r[4]) == 3 and int(r[5]) == 2
        assert int(r[72]) == int(t[0][0]) and int(r[73]) == 40 and int(r[74]) == 40

    return make(12, 4, 2, [group(12, 4, 2, ids, weights=w)], regime, wrap=0)


def zero_w_case():
    a, b = _two()
    ids = a * 5 + b * 5

    def regime(c, w_):
        r = w_[0][2]
        assert flags(w_) == 4 | 8 and int(r[1]) == min(a) and int(r[72]) == min(b) and int(r[4]) == 20 and int(r[5]) == 0

    return make(12, 4, 2, [group(12, 4, 2, ids, weights=[0] * 40)], regime, wrap=0)


def big_w_case():
    nx, ny, T, P = 12, 4, 2, 2049
    rng = np.random.default_rng(601)
    a, b = _two()
    ids = rng.choice(a, P)
    ids[::100] = b[0]
    w = (0xFFFFFFFF - rng.integers(0, 5, P)).astype(np.uint32)
    g = group(nx, ny, T, ids, weights=w, rng=rng)
    g["poses"][:, 2:] += F32(4000.0)                                # X, Y near 2^22: the second moments near 2^44

    def regime(c, w_):
        r = w_[0][2]
        assert int(r[75]) > 0 and int(r[8 + 32 + 1]) > 0 and int(w_[0][1][0][3]) >= 2000         # W above 2^32 (2^43)
        assert int(r[8 + 32 + 4 * 5 + 2]) > 0 and not flags(w_)                                  # sum wXX above 2^64

    return make(nx, ny, T, [g], regime, wrap=0)


def out_of_range_case():
    a, b = _two()
    rng = np.random.default_rng(602)
    g = group(12, 4, 2, a * 6 + b * 6, weights=rng.integers(1, 50, 48), rng=rng)
    g["poses"][3, 2] = F32(9000.0)                                  # 9000 m * 1024 >= 2^23
    g["poses"][30, 0] = F32(np.nan)
    g["poses"][31, 3] = F32(-np.inf)

    def regime(c, w_):
        r = w_[0][2]
        assert flags(w_) == 2 and int(r[2]) == 45 and (w_[0][0] != NONE).all()
        assert int(w_[0][1][0][1]) == 23 and int(w_[0][1][1][1]) == 22

    return make(12, 4, 2, [g], regime, wrap=0)


# ---- the table, groups, modes, the larger draw ------------------------------------------------------------------------------------------
def five_case():
    nx, ny, T = 20, 3, 2
    rng = np.random.default_rng(701)
    blobs = [blob(nx, ny, 4 * j, 0, j % 2, 2, 2, 1) for j in range(5)]
    ids = np.concatenate([rng.choice(bl, 20 + 7 * j) for j, bl in enumerate(blobs)])

    def regime(c, w_):
        assert n_c(w_) == 5 and np.all(np.diff(w_[0][1][:, 0].astype(np.int64)) > 0)

    return make(nx, ny, T, [group(nx, ny, T, ids, weights=rng.integers(0, 100, len(ids)), rng=rng)], regime, wrap=0)


def groups_case(shared):
    def build():
        nx, ny, T, P = 10, 6, 4, 1100
        rng = np.random.default_rng(801 + shared)
        gs = []
        for g in range(3):
            blobs = blob(nx, ny, g, g, g, 2, 2, 1) + blob(nx, ny, 6, g + 1, (g + 2) % 4, 3, 2, 1) + \
                (blob(nx, ny, 3, 5, 3, 1, 1, 1) if g == 1 else [])
            gs.append(group(nx, ny, T, rng.choice(blobs, P), weights=rng.integers(0, 9, P) if g != 2 else None, rng=rng))
        if shared:                                                  # one list for every group: a group's bins need not
            for g in gs[1:]:                                        # be where the poses are
                g["poses"] = gs[0]["poses"]

        def regime(c, w_):
            assert len(w_) == 3 and len({w_[g][2][1:8].tobytes() for g in range(3)}) == 3
            assert len({c["groups"][g]["map"].tobytes() for g in range(3)}) == 3

        return make(nx, ny, T, gs, regime, shared=bool(shared))
    return build


MODES = ((3.2, 4.3, 0.4), (17.8, 11.1, 2.5))                        # (x, y, theta) of the two modes


def two_modes_case():
    s, T, P = bo.spec(0.0, 0.0, 2.0, 48, 32), 36, 3000
    rng = np.random.default_rng(901)
    which = rng.random(P) < 0.4
    m = np.array(MODES)[which.astype(int)]
    xyt = m + rng.normal(0.0, 1.0, (P, 3)) * (0.12, 0.12, 0.04)
    poses = np.stack([np.cos(xyt[:, 2]), np.sin(xyt[:, 2]), xyt[:, 0], xyt[:, 1]], axis=1).astype(F32)
    bmap, bins, r20 = bo.bin_poses(s, poses, None, bo.table(T))

    def regime(c, w_):
        t = w_[0][1]
        heavy = t[np.argsort(-t[:, 1].astype(np.int64))][:2]
        assert int(r20[1]) == P and n_c(w_) >= 2 and int(heavy[:, 1].sum()) > 0.97 * P
        assert int(w_[0][2][1]) == int(heavy[0][0]) and int(w_[0][2][72]) == int(heavy[1][0])

    return make(48, 32, T, [dict(poses=poses, weights=None, map=bmap, bins=bins)], regime)


def large_case():
    s, T, P = bo.spec(), 72, 65536
    rng = np.random.default_rng(902)
    poses = bc.spread(s, T, P, rng, margin=0.5)
    w = rng.integers(0, 1 << 16, P).astype(np.uint32)
    bmap, bins, _ = bo.bin_poses(s, poses, w, bo.table(T), both=False)

    def regime(c, w_):
        r = w_[0][2]
        assert n_c(w_) >= 100 and int(r[7]) >= 10000 and int(r[77]) > 0 and not flags(w_) & 32

    return make(s.nx, s.ny, T, [dict(poses=poses, weights=w, map=bmap, bins=bins)], regime)


def over_bound_case():
    nx, ny, T = 128, 128, 65                                        # 1 064 960 bins, every one occupied
    g = group(nx, ny, T, [0, 5, nx * ny * T - 1] * 10)
    g["map"][:] = 0xFFFFFFFF

    def regime(c, w_):
        r = w_[0][2]
        assert int(r[7]) == nx * ny * T > co.MAX_BINS and int(r[0]) == 32 and int(r[6]) == 0

    return make(nx, ny, T, [g], regime)


BUILDERS = {f"edge{P}": edge_case(P) for P in EDGE_P}
BUILDERS.update({f"nb{NB}": nb_case(NB) for NB in NB_SHAPES})
BUILDERS.update({k: _ids_case(*v) for k, v in SMALL.items()})
BUILDERS.update(
    blocks=blocks_case, serpentine=_chain(31, 31, 1, serpentine_ids(31, 31, 0, 31), 1, 401),
    spiral=_chain(15, 15, 9, spiral_ids(), 0, 402), comb=_chain(128, 128, 1, comb_ids(), 1, 403), bridge=bridge_case,
    map_only=map_only_case, strays=strays_case, empty=empty_case, tie=tie_case, heavy_few=heavy_few_case,
    zero_w=zero_w_case, big_w=big_w_case, out_of_range=out_of_range_case, five=five_case, groups0=groups_case(0),
    groups1=groups_case(1), two_modes=two_modes_case, large=large_case, over_bound=over_bound_case)
NAMES = list(BUILDERS)
