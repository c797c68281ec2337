"""E16's rule (include/rplgpu_msg.h, the E16 block) restated for the tests: systematic resampling of a weighted pose
list in Python integers, the move in numpy float32 product by product, the eight result words from Python integers.

Two writers of the ancestors that share no step:
  ancestors_search   t_j = (j S + r) // M in Python integers, then np.searchsorted(C, t, 'right') over the cumulative sum;
  ancestors_counts   the number of copies of pose i, J(C[i]) - J(C[i - 1]) with J(c) = the number of outputs whose
                     t_j < c in closed form, expanded with np.repeat.
Neither uses the 64-bit forms of r and t_j that the library computes with; r64 and t64 restate those for the test
that holds them to the big integers."""
import numpy as np

F32 = np.float32
MAX_POSES = 1 << 20
TILE = 1024
QNAN = 0x7FC00000
MASK64 = (1 << 64) - 1


def tiles(P):
    return (P + TILE - 1) // TILE


def scratch_words(G, P):
    """16 header words, 8 per tile and T + 1 boundaries padded to an even count, per group."""
    if G == 0 or not 0 < P <= MAX_POSES:
        return 0
    T = tiles(P)
    return G * (16 + 8 * T + ((T + 2) & ~1))


def total(w):
    return sum(int(v) for v in np.asarray(w).tolist())


def r_of(u, S):
    return (int(u) * S) >> 32


def t_all(S, r, M):
    """t_j for every j, as an object array of Python integers."""
    return (np.arange(M, dtype=object) * S + r) // M


def r64(u, S):
    """The header's 64-bit form of r; every intermediate is checked to fit."""
    a = u * (S >> 32)
    b = (u * (S & 0xFFFFFFFF)) >> 32
    assert a <= MASK64 and u * (S & 0xFFFFFFFF) <= MASK64 and a + b <= MASK64
    return a + b


def t64(j, S, r, M):
    """The header's 64-bit form of t_j; every intermediate is checked to stay below 2^63."""
    q, rho = divmod(S, M)
    assert j * q < 1 << 63 and j * rho + r < 1 << 63
    v = j * q + (j * rho + r) // M
    assert v < 1 << 63
    return v


def ancestors_search(w, M, u):
    w = np.asarray(w, np.uint32)
    P = len(w)
    S = total(w)
    if S == 0:
        return (np.arange(M, dtype=np.int64) % P).astype(np.uint32)
    C = np.cumsum(w.astype(np.uint64), dtype=np.uint64)  # S < 2^52: exact
    assert int(C[-1]) == S
    t = t_all(S, r_of(u, S), M).astype(np.uint64)
    return np.searchsorted(C, t, "right").astype(np.uint32)


def copies(w, M, u):
    """How often each pose is drawn: J(C[i]) - J(C[i - 1]), J in closed form (S > 0)."""
    w = np.asarray(w, np.uint32)
    S = total(w)
    r = r_of(u, S)
    C = np.cumsum(w.astype(object))
    num = C * M - r                         # Python integers
    J = np.where(num <= 0, 0, np.minimum(M, -((-num) // S)))  # ceil(num / S)
    J = np.concatenate([[0], J]).astype(np.int64)
    return np.diff(J)


def ancestors_counts(w, M, u):
    w = np.asarray(w, np.uint32)
    P = len(w)
    if total(w) == 0:
        return np.concatenate([np.arange(P, dtype=np.uint32)] * (M // P + 1))[:M]
    k = copies(w, M, u)
    assert (k >= 0).all() and int(k.sum()) == M
    return np.repeat(np.arange(P, dtype=np.uint32), k)


def move(poses, delta):
    """(n, 4) float32 poses moved by (n, 4) or (1, 4) deltas: each product rounded, then the difference or sum; a
    NaN result is 0x7FC00000."""
    p = np.asarray(poses, F32).reshape(-1, 4)
    d = np.broadcast_to(np.asarray(delta, F32).reshape(-1, 4), p.shape)
    c, s, x, y = (p[:, k] for k in range(4))
    dc, ds, dx, dy = (d[:, k] for k in range(4))
    out = np.empty(p.shape, F32)
    with np.errstate(all="ignore"):
        a = c * dc; b = s * ds; out[:, 0] = a - b                  # noqa: E702
        a = s * dc; b = c * ds; out[:, 1] = a + b                  # noqa: E702
        a = c * dx; b = s * dy; e = a - b; out[:, 2] = e + x       # noqa: E702
        a = s * dx; b = c * dy; e = a + b; out[:, 3] = e + y       # noqa: E702
    bits = out.view(np.uint32)
    bits[np.isnan(out)] = QNAN
    return out


def result_of(w, M, anc):
    w = np.asarray(w, np.uint32)
    S = total(w)
    sq = sum(int(v) ** 2 for v in w.tolist())
    assert S < 1 << 52 and sq < 1 << 96
    distinct = min(M, len(w)) if S == 0 else len(np.unique(anc))
    return np.array([S & 0xFFFFFFFF, S >> 32, sq & 0xFFFFFFFF, (sq >> 32) & 0xFFFFFFFF, sq >> 64,
                     int(np.count_nonzero(w)), distinct, 1 if S == 0 else 0], np.uint32)


def resample(w, poses, M, u=0, delta=None, writer=ancestors_search):
    """One group -> (poses_out (M, 4) float32, ancestors (M,) uint32, result (8,) uint32)."""
    poses = np.asarray(poses, F32).reshape(-1, 4)
    assert len(poses) == len(w) and 0 < len(w) <= MAX_POSES and 0 < M <= MAX_POSES
    anc = writer(w, M, u)
    assert anc.shape == (M,)
    out = poses[anc].copy()  # a gather moves bytes: payloads and -0 survive
    if delta is not None:
        delta = np.asarray(delta, F32).reshape(-1, 4)
        assert len(delta) in (1, M)
        out = move(out, delta)
    return out, anc, result_of(w, M, anc)
