"""The oracle of E21 (include/rplgpu_msg.h, the E21 block): the occupied bins of E20's bit map labelled by connected
component, the poses labelled and the clusters weighed, the heaviest reduced to E17's sums — by two writers that share no
step (the quantisation is tests/estimate_oracle.py's, imported).

(a) ``writer_a``: numpy — the map unpacked to a (T, ny, nx) array and labelled by ``scipy.ndimage.label`` under the
    full 3 x 3 x 3 structure (a numpy flood fill where scipy does not import), the labels united across the
    theta = 0 / T - 1 faces for WRAP, relabelled to the smallest bin id by ``np.minimum.at``; W and the counts by
    ``np.bincount`` on limbs, the sums by ``estimate_oracle.sums_limbs``.
(b) ``writer_b``: plain Python — a breadth-first search over a set of bin ids with the neighbour relation spelled out,
    dictionaries for W and the counts, the sums in a loop of Python integers.

``cluster`` runs (a), and (b) beside it up to 4096 poses, and returns (a)'s answer once they agree."""
from collections import deque

import numpy as np

from tests import estimate_oracle as eo

F32 = np.float32
NONE = 0xFFFFFFFF
WORDS = 80
B_LIMIT = 4096
MAX_BINS = 1 << 20

try:
    from scipy import ndimage
except Exception:                                                   # pragma: no cover
    ndimage = None


def map_words(nx, ny, T):
    return (nx * ny * T + 31) // 32


def map_of(nx, ny, T, ids):
    m = np.zeros(map_words(nx, ny, T), np.uint32)
    ids = np.asarray(sorted(set(int(i) for i in ids)), np.int64)
    np.bitwise_or.at(m, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return m


def occupied_ids(bmap, nb):
    bits = np.unpackbits(np.ascontiguousarray(bmap, np.uint32).view(np.uint8), bitorder="little")[:nb]
    return np.flatnonzero(bits)


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def _flood_numpy(occ):
    """a 26-connected labelling without scipy: repeated 3 x 3 x 3 minimum of provisional labels"""
    lab = np.where(occ, np.arange(1, occ.size + 1).reshape(occ.shape), 0)
    big = occ.size + 2
    while True:
        cur = np.where(occ, lab, big)
        p = np.pad(cur, 1, constant_values=big)
        new = cur.copy()
        for dk in range(3):
            for dy in range(3):
                for dx in range(3):
                    new = np.minimum(new, p[dk:dk + occ.shape[0], dy:dy + occ.shape[1], dx:dx + occ.shape[2]])
        new = np.where(occ, new, 0)
        if (new == lab).all():
            break
        lab = new
    names = np.unique(lab[occ])
    return np.where(occ, np.searchsorted(names, lab) + 1, 0), len(names)


def a_bin_labels(bmap, nx, ny, T, wrap):
    """-> label per bin ((NB,) int64, -1 where not occupied)"""
    nb = nx * ny * T
    bits = np.unpackbits(np.ascontiguousarray(bmap, np.uint32).view(np.uint8), bitorder="little")[:nb]
    occ = bits.reshape(T, ny, nx).astype(bool)
    if ndimage is not None:
        comp, n = ndimage.label(occ, structure=np.ones((3, 3, 3), int))
    else:
        comp, n = _flood_numpy(occ)
    head = np.arange(n + 1)

    def find(v):
        while head[v] != v:
            head[v] = head[head[v]]
            v = head[v]
        return v

    if wrap and T >= 3:                                             # (T = 1, 2: the wrap neighbours are the plain ones)
        top, bot = comp[T - 1], comp[0]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                a = top[max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)]
                b = bot[max(0, dy):ny - max(0, -dy), max(0, dx):nx - max(0, -dx)]
                both = (a > 0) & (b > 0)
                for u, v in set(zip(a[both].tolist(), b[both].tolist())):
                    ru, rv = find(u), find(v)
                    if ru != rv:
                        head[max(ru, rv)] = min(ru, rv)
    root = np.array([find(v) for v in range(n + 1)])
    comp = root[comp].reshape(-1)
    ids = np.arange(nb)
    least = np.full(n + 1, nb, np.int64)
    on = comp > 0
    np.minimum.at(least, comp[on], ids[on])
    return np.where(on, least[comp], -1)


def _u64_bincount(idx, w, n):
    lo = np.bincount(idx, (w & 0xFFFF).astype(np.float64), n).astype(np.int64)
    hi = np.bincount(idx, (w >> 16).astype(np.float64), n).astype(np.int64)          # each below 2^16 * 2^20: exact
    return [int(a) + (int(b) << 16) for a, b in zip(lo, hi)]


def writer_a(g, nx, ny, T, wrap, xy_scale):
    nb = nx * ny * T
    P = len(g["poses"])
    bins = np.asarray(g["bins"], np.uint32).astype(np.int64)
    w = np.ones(P, np.int64) if g["weights"] is None else np.asarray(g["weights"], np.uint32).astype(np.int64)
    bin_label = a_bin_labels(g["map"], nx, ny, T, wrap)
    K = int((bin_label >= 0).sum())
    if K > MAX_BINS:
        return over_bound(P, K)
    labels_sorted = np.unique(bin_label[bin_label >= 0])
    unlab = bins == NONE
    lab = np.where(~unlab & (bins < nb), bin_label[np.minimum(bins, nb - 1)], -1)
    labelled = lab >= 0
    stray = ~unlab & ~labelled
    q, inr, _ = eo.quantise(g["poses"], xy_scale)
    use = labelled & inr
    ordinal = np.searchsorted(labels_sorted, lab[use])
    W = _u64_bincount(ordinal, w[use], len(labels_sorted))
    count = np.bincount(ordinal, minlength=len(labels_sorted)).tolist()
    table = np.array([[int(l), c, v & 0xFFFFFFFF, v >> 32] for l, c, v in zip(labels_sorted, count, W)],
                     np.uint32).reshape(-1, 4)
    order = sorted(range(len(W)), key=lambda c: (-W[c], c))
    best = order[0] if order else None
    second = order[1] if len(order) > 1 else None
    in_best = use & (lab == (labels_sorted[best] if best is not None else -2))
    wu = w.astype(np.uint32)
    s0, s1 = eo.sums_limbs(q, wu, use), eo.sums_limbs(q, wu, in_best)
    return assemble(np.where(labelled, lab, NONE).astype(np.uint32), table, best, second, s0, s1,
                    [int(use.sum()), int((use & (w != 0)).sum()), int(in_best.sum()), int((in_best & (w != 0)).sum())],
                    K, int(stray.sum()), int(unlab.sum()), bool((labelled & ~inr).any()))


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def neighbours(b, nx, ny, T, wrap):
    """the bin ids next to b: |dx| <= 1, |dy| <= 1, dk in {0, +1, -1} (modulo T under WRAP), b itself left out"""
    bx, by, kt = b % nx, b // nx % ny, b // (nx * ny)
    out = set()
    for dk in (-1, 0, 1):
        k = kt + dk
        if wrap:
            k %= T
        elif k < 0 or k >= T:
            continue
        for dy in (-1, 0, 1):
            y = by + dy
            if y < 0 or y >= ny:
                continue
            for dx in (-1, 0, 1):
                x = bx + dx
                if x < 0 or x >= nx:
                    continue
                out.add((k * ny + y) * nx + x)
    out.discard(b)
    return out


def b_components(occ, nx, ny, T, wrap):
    """occ: a set of bin ids -> {bin id: label}"""
    label = {}
    for start in sorted(occ):
        if start in label:
            continue
        label[start] = start
        todo = deque([start])
        while todo:
            b = todo.popleft()
            for q in neighbours(b, nx, ny, T, wrap):
                if q in occ and q not in label:
                    label[q] = start
                    todo.append(q)
    return label


def b_far(occ, start, nx, ny, T, wrap):
    """the largest breadth-first distance from `start` inside occ, and a bin that has it"""
    dist = {start: 0}
    todo = deque([start])
    last = start
    while todo:
        b = todo.popleft()
        last = b
        for q in neighbours(b, nx, ny, T, wrap):
            if q in occ and q not in dist:
                dist[q] = dist[b] + 1
                todo.append(q)
    return dist[last], last


def diameter_at_least(bmap, nx, ny, T, wrap):
    """a lower bound of the graph diameter of the component of the smallest occupied bin: two sweeps"""
    occ = set(occupied_ids(bmap, nx * ny * T).tolist())
    _, far = b_far(occ, min(occ), nx, ny, T, wrap)
    return b_far(occ, far, nx, ny, T, wrap)[0]


def writer_b(g, nx, ny, T, wrap, xy_scale):
    nb = nx * ny * T
    P = len(g["poses"])
    occ = set()
    for wi, word in enumerate(np.asarray(g["map"], np.uint32).tolist()):
        occ.update(32 * wi + i for i in range(32) if word >> i & 1 and 32 * wi + i < nb)
    if len(occ) > MAX_BINS:
        return over_bound(P, len(occ))
    label = b_components(occ, nx, ny, T, wrap)
    names = sorted(set(label.values()))
    W = {l: 0 for l in names}
    count = {l: 0 for l in names}
    q, inr, _ = eo.quantise(g["poses"], xy_scale)
    labels, member = [], []
    stray = unlab = 0
    bad = False
    for i, b in enumerate(np.asarray(g["bins"], np.uint32).tolist()):
        w = 1 if g["weights"] is None else int(g["weights"][i])
        if b == NONE:
            unlab += 1
            labels.append(NONE)
            member.append(None)
        elif b not in occ:
            stray += 1
            labels.append(NONE)
            member.append(None)
        else:
            labels.append(label[b])
            if inr[i]:
                W[label[b]] += w
                count[label[b]] += 1
                member.append(label[b])
            else:
                bad = True
                member.append(None)
    best = second = None
    for l in names:
        if best is None or W[l] > W[best]:
            best = l
    for l in names:
        if l != best and (second is None or W[l] > W[second]):
            second = l
    s = [[0] * 8, [0] * 8]
    n = [0, 0, 0, 0]
    for i, ((X, Y, C, S), m) in enumerate(zip(q.tolist(), member)):
        if m is None:
            continue
        w = 1 if g["weights"] is None else int(g["weights"][i])
        for k in range(2 if m == best else 1):
            for j, v in enumerate((1, X, Y, C, S, X * X, X * Y, Y * Y)):
                s[k][j] += w * v
            n[2 * k] += 1
            n[2 * k + 1] += 1 if w else 0
    table = np.array([[l, count[l], W[l] & 0xFFFFFFFF, W[l] >> 32] for l in names], np.uint32).reshape(-1, 4)
    return assemble(np.array(labels, np.uint32), table, names.index(best) if names else None,
                    names.index(second) if second is not None else None, s[0], s[1], n, len(occ), stray, unlab, bad)


# ---- both ---------------------------------------------------------------------------------------------------------------
def over_bound(P, K):
    res = np.zeros(WORDS, np.uint32)
    res[0], res[1], res[72], res[7] = 32, NONE, NONE, K
    return np.full(P, NONE, np.uint32), np.zeros((0, 4), np.uint32), res


def assemble(labels, table, best, second, s0, s1, n, K, stray, unlab, bad):
    res = [0] * WORDS
    res[0] = (1 if len(table) == 0 else 0) | (2 if bad else 0) | (4 if s0[0] == 0 else 0) | (8 if s1[0] == 0 else 0) | \
        (16 if stray else 0)
    res[1] = int(table[best][0]) if best is not None else NONE
    res[2:6] = n
    res[6], res[7] = len(table), K
    at = 8
    for s in (s0, s1):
        for v in s:
            res[at:at + 4] = eo.words_of(v)
            at += 4
    res[72] = NONE
    if second is not None:
        res[72:76] = [int(v) for v in table[second]]
    res[76], res[77] = stray, unlab
    return labels, table, np.array(res, np.uint32)


def cluster(g, nx, ny, T, wrap, xy_scale=1024.0, both=None):
    """one group {poses (P, 4), weights (P,) or None, map, bins (P,)} -> (labels (P,), the WHOLE table (N_c, 4), result
    (80,)); writer (b) beside (a) where the module's header says so (``both`` overrides)"""
    got = writer_a(g, nx, ny, T, wrap, xy_scale)
    if both is None:
        both = len(g["poses"]) <= B_LIMIT
    if both:
        other = writer_b(g, nx, ny, T, wrap, xy_scale)
        for k, (x, y) in enumerate(zip(got, other)):
            assert x.tobytes() == y.tobytes(), f"the two writers differ in output {k}"
    return got
