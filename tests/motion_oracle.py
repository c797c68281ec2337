"""The E18 oracle (include/rplgpu_msg.h, the E18 block): M deltas and eight result words of one group, by two writers
that share no step.

(a) `deltas_python`: Philox4x32-10 and Z in Python integers; the float steps in Python doubles rounded to float32
    after every operation.  A double holds the exact sum, difference and product of two float32 or rounds a quotient
    where a second rounding to 24 bits cannot differ from the single one (53 >= 2 * 24 + 2), so this IS float32
    arithmetic.  Inf / Inf and x / 0 are written out, since Python raises where IEEE 754 answers.
(b) `deltas_numpy`: Philox in numpy uint64 arrays over all outputs at once, the float steps in numpy float32.

Above PYTHON_LIMIT outputs writer (b) alone."""
import math
import struct

import numpy as np

F32 = np.float32
MASK = 0xFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
Z_BIAS = 262140
Z_VAR = 2863311530                     # the variance of Z, exactly: 8 * (2^32 - 1) / 12
Z2_VAR = 1.51673e19                    # the variance of Z^2 (the figure of the E18 issue)
QNAN = 0x7FC00000
PYTHON_LIMIT = 4096
DEFAULT = dict(seed=0, step=0, first=0)


# ---- writer (a): Python integers and doubles --------------------------------------------------------------------------
def philox_python(ctr, key, rounds=10):
    c0, c1, c2, c3 = (int(v) for v in ctr)
    k0, k1 = (int(v) for v in key)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def z_of_words(words):
    return sum((int(w) & 0xFFFF) + (int(w) >> 16) for w in words) - Z_BIAS


def z_python(spec, g, j, i):
    seed, step = int(spec["seed"]), int(spec["step"])
    ctr = ((int(spec["first"]) + j) & MASK, (g << 2) | i, step & MASK, step >> 32)
    return z_of_words(philox_python(ctr, (seed & MASK, seed >> 32)))


def _r(x):
    """a double rounded to float32 (ties to even), as a double"""
    if x != x or x in (math.inf, -math.inf):
        return x
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def _div(a, b):
    if a != a or b != b:
        return math.nan
    if b == 0.0:
        if a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    if a in (math.inf, -math.inf) and b in (math.inf, -math.inf):
        return math.nan
    return _r(a / b)


def _noise_python(z, k):
    t = _r(float(z) * k)
    q = _r(t * t)
    den = _r(1.0 + q)
    return _div(_r(1.0 - q), den), _div(_r(t + t), den)


def _compose_python(r, n):
    return _r(_r(r[0] * n[0]) - _r(r[1] * n[1])), _r(_r(r[1] * n[0]) + _r(r[0] * n[1]))


def _bits(x):
    return QNAN if x != x else struct.unpack("<I", struct.pack("<f", x))[0]


def deltas_python(odom, M, spec, g=0):
    """-> (delta words (M, 4) uint32, Z (M, 3) Python integers as an object-free int64 array)"""
    o = [float(v) for v in np.asarray(odom, F32)]
    r1, trans, r2, k1, kt, k2 = (o[0], o[1]), o[2], (o[3], o[4]), o[5], o[6], o[7]
    words = np.zeros((M, 4), np.uint32)
    zs = np.zeros((M, 3), np.int64)
    for j in range(M):
        z = [z_python(spec, g, j, i) for i in range(3)]
        a = _compose_python(r1, _noise_python(z[0], k1))
        b = _compose_python(r2, _noise_python(z[2], k2))
        tr = _r(trans + _r(float(z[1]) * kt))
        d = _compose_python(a, b)
        words[j] = [_bits(d[0]), _bits(d[1]), _bits(_r(a[0] * tr)), _bits(_r(a[1] * tr))]
        zs[j] = z
    return words, zs


# ---- writer (b): numpy arrays -----------------------------------------------------------------------------------------
def philox_numpy(c0, c1, c2, c3, k0, k1, rounds=10):
    """counters as uint64 arrays (values below 2^32), the key as Python integers -> four uint64 arrays"""
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in (c0, c1, c2, c3))
    for r in range(rounds):
        ka, kb = np.uint64((k0 + r * W0) & MASK), np.uint64((k1 + r * W1) & MASK)
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ ka, p1 & m, (p0 >> s32) ^ c3 ^ kb, p0 & m
    return c0, c1, c2, c3


def z_numpy(spec, g, M):
    """-> Z (M, 3) int64"""
    seed, step = int(spec["seed"]), int(spec["step"])
    j = (np.arange(M, dtype=np.uint64) + np.uint64(int(spec["first"]))) & np.uint64(MASK)
    out = np.zeros((M, 3), np.int64)
    for i in range(3):
        full = np.full(M, 1, np.uint64)
        w = philox_numpy(j, full * np.uint64((g << 2) | i), full * np.uint64(step & MASK),
                         full * np.uint64(step >> 32), seed & MASK, seed >> 32)
        halves = sum((x & np.uint64(0xFFFF)) + (x >> np.uint64(16)) for x in w)
        out[:, i] = halves.astype(np.int64) - Z_BIAS
    return out


def _noise_numpy(z, k):
    t = z.astype(F32) * k
    q = t * t
    den = F32(1.0) + q
    return (F32(1.0) - q) / den, (t + t) / den


def _compose_numpy(r, n):
    return r[0] * n[0] - r[1] * n[1], r[1] * n[0] + r[0] * n[1]


def deltas_numpy(odom, M, spec, g=0):
    o = np.asarray(odom, F32)
    zs = z_numpy(spec, g, M)
    with np.errstate(all="ignore"):
        a = _compose_numpy((o[0], o[1]), _noise_numpy(zs[:, 0], o[5]))
        b = _compose_numpy((o[3], o[4]), _noise_numpy(zs[:, 2], o[7]))
        tr = o[2] + zs[:, 1].astype(F32) * o[6]
        d = _compose_numpy(a, b)
        out = np.stack([d[0], d[1], a[0] * tr, a[1] * tr], 1).astype(F32)
    words = np.ascontiguousarray(out).view(np.uint32).copy()
    words[np.isnan(out)] = QNAN
    return words, zs


# ---- the result words ---------------------------------------------------------------------------------------------------
def result_words(words, zs):
    n = int((words == QNAN).any(axis=1).sum())
    z = [int(v) for v in zs.reshape(-1)]
    s, s2 = sum(z), sum(v * v for v in z)
    return np.array([n, max(abs(v) for v in z), s & MASK, (s >> 32) & MASK, s2 & MASK, s2 >> 32, 0, 1 if n else 0],
                    np.uint32)


def sample(odom, M, spec=DEFAULT, g=0, writer=None):
    """-> (delta words (M, 4) uint32, result (8,) uint32, Z (M, 3) int64) of group g"""
    if writer is None:
        writer = deltas_python if M <= PYTHON_LIMIT else deltas_numpy
    words, zs = writer(odom, M, spec, g)
    return words, result_words(words, zs), zs


def sum_z(res):
    v = int(res[2]) | int(res[3]) << 32
    return v - (1 << 64) if v >> 63 else v


def sum_z2(res):
    return int(res[4]) | int(res[5]) << 32


# ---- the odometry helper through Python's math (the same libm) --------------------------------------------------------
def odometry(dx, dy, dtheta, alpha):
    trans = math.sqrt(dx * dx + dy * dy)
    rot1 = math.atan2(dy, dx) if trans >= 0.01 else 0.0
    d = dtheta - rot1
    rot2 = math.atan2(math.sin(d), math.cos(d))
    f1 = min(abs(rot1), math.pi - abs(rot1))
    f2 = min(abs(rot2), math.pi - abs(rot2))
    v1 = alpha[0] * f1 * f1 + alpha[1] * trans * trans
    vt = alpha[2] * trans * trans + alpha[3] * (f1 * f1 + f2 * f2)
    v2 = alpha[0] * f2 * f2 + alpha[1] * trans * trans
    sz = math.sqrt(2863311530.0)
    return np.array([math.cos(rot1), math.sin(rot1), trans, math.cos(rot2), math.sin(rot2),
                     math.sqrt(v1) / (2.0 * sz), math.sqrt(vt) / sz, math.sqrt(v2) / (2.0 * sz)], F32)
