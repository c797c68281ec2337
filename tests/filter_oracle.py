"""E10 restated in numpy (include/rplgpu_msg.h: the scan-shadow and the speckle filter on a LaserScan).

Imported by tests only.  Every float32 operation of the rules is one numpy float32 operation (no fused
multiply-add exists here), the four direction values come from math.cos / math.sin, the two cross
terms are fp64, the neighbours are visited by brute force over y and the runs by a cumulative count."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
QNAN = np.uint32(0x7FC00000)
MAX_WINDOW = 64

DEFAULTS = dict(shadow_enable=1, shadow_min_angle=float(F32(math.radians(10.0))),
                shadow_max_angle=float(F32(math.radians(170.0))), shadow_window=2, shadow_neighbors=1,
                speckle_enable=1, speckle_max_range_difference=float(F32(0.05)), speckle_min_run=4, circular=1)


def flt(**kw):
    """A filter as a dict: DEFAULTS with overrides (float members rounded to float32 as the struct holds them)."""
    d = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in d:
            raise KeyError(k)
        d[k] = v
    for k in ("shadow_min_angle", "shadow_max_angle", "speckle_max_range_difference"):
        d[k] = float(F32(d[k]))
    return d


def dirs(f):
    """cmin, smin, cmax, smax as float32."""
    lo, hi = float(F32(f["shadow_min_angle"])), float(F32(f["shadow_max_angle"]))
    return F32(math.cos(lo)), F32(math.sin(lo)), F32(math.cos(hi)), F32(math.sin(hi))


def inc_mode_a(count):
    return F32(2.0 * math.pi / float(count))


def inc_mode_b(count):
    return F32(2.0 * math.pi / float(max(count - 1, 1)))


def e6_sincos(a):
    """The E6 polynomials (rplgpu_cloud_deskew_batch_dev), one float32 rounding per operation."""
    a = F32(a)
    a2 = F32(a * a)
    ts = F32(a2 * F32(1.0 / 120.0))
    ts = F32(ts + F32(-1.0 / 6.0))
    ts = F32(a2 * ts)
    ts = F32(ts + F32(1.0))
    sn = F32(a * ts)
    tc = F32(a2 * F32(-1.0 / 720.0))
    tc = F32(tc + F32(1.0 / 24.0))
    tc = F32(a2 * tc)
    tc = F32(tc + F32(-0.5))
    tc = F32(a2 * tc)
    cn = F32(tc + F32(1.0))
    return sn, cn


def pair_tests(r1, r2, s, c, d):
    """(theta below min, theta above max) of the pair seen from r1; arrays or scalars of float32."""
    cmin, smin, cmax, smax = d
    with np.errstate(all="ignore"):
        r1 = np.asarray(r1, F32)
        r2 = np.asarray(r2, F32)
        a = (r2 * F32(s)).astype(F32)
        rc = (r2 * F32(c)).astype(F32)
        b = (r1 - rc).astype(F32)
        a64, b64 = a.astype(F64), b.astype(F64)
        below = F64(cmin) * a64 - F64(smin) * b64
        above = F64(cmax) * a64 - F64(smax) * b64
        return below < 0.0, above > 0.0


def _shift(arr, k, circular, fill):
    """out[i] = arr[i + k]; beyond the ends: modulo with circular, else `fill`."""
    n = len(arr)
    if circular:
        return np.roll(arr, -k)
    out = np.full(n, fill, arr.dtype)
    if k >= 0:
        if k < n:
            out[: n - k] = arr[k:]
    elif -k < n:
        out[-k:] = arr[: n + k]
    return out


def windows(f, count):
    """(W, N) in force for a scan of `count` beams."""
    W, N = int(f["shadow_window"]), int(f["shadow_neighbors"])
    if f["circular"]:
        half = (count - 1) // 2
        W, N = min(W, half), min(N, half)
    return W, N


def shadow(r, inc, f):
    """(removed mask, detected mask) of the shadow filter on float32 ranges r."""
    n = len(r)
    circ = bool(f["circular"])
    fin = np.isfinite(r)
    W, N = windows(f, n)
    d = dirs(f)
    det = np.zeros(n, bool)
    for y in range(1, W + 1):
        delta = F32(F32(y) * F32(inc))
        if not delta <= F32(0.5):
            break
        s, c = e6_sincos(delta)
        for k in (y, -y):
            r2 = _shift(r, k, circ, F32(np.inf))
            f2 = _shift(fin, k, circ, False)
            below, above = pair_tests(r, r2, s, c, d)
            det |= fin & f2 & (below | above)
    rd = np.where(det, r, F32(np.inf)).astype(F32)
    m = np.full(n, np.inf, F32)
    for k in range(-N, N + 1):
        m = np.minimum(m, _shift(rd, k, circ, F32(np.inf)))
    with np.errstate(invalid="ignore"):
        removed = fin & (m < r)
    return removed, det


def run_lengths(r, D, circular):
    """Per beam the number of beams of its run (a non-finite beam: 0)."""
    n = len(r)
    fin = np.isfinite(r)
    if n == 0:
        return np.zeros(0, np.int64)
    nxt = _shift(r, 1, circular, F32(np.inf))
    with np.errstate(invalid="ignore"):
        link = fin & np.isfinite(nxt) & (np.abs((nxt - r).astype(F32)) <= F32(D))  # link[k]: k -> k + 1
    if link.all():  # (circular only) the run closes the circle
        return np.full(n, n, np.int64)
    start = 0
    if circular:  # begin behind a missing link, so that no run crosses the array's end
        start = (int(np.argmin(link)) + 1) % n
        link = np.roll(link, -start)
        fin = np.roll(fin, -start)
    first = np.ones(n, bool)
    first[1:] = ~link[:-1]
    run_id = np.cumsum(first) - 1
    length = np.bincount(run_id)[run_id]
    length = np.where(fin, length, 0)
    return np.roll(length, start) if circular else length


def filter_scan(ranges, inc, f):
    """One scan of `len(ranges)` beams -> (ranges_out float32, removed by shadow, removed by speckle)."""
    r = np.ascontiguousarray(ranges, F32).copy()
    out = r.view(np.uint32).copy()
    n_sh = n_sp = 0
    if len(r) == 0:
        return out.view(F32), 0, 0
    if f["shadow_enable"]:
        rem, _ = shadow(r, inc, f)
        out[rem] = QNAN
        n_sh = int(rem.sum())
    if f["speckle_enable"]:
        post = out.view(F32)
        ln = run_lengths(post, f["speckle_max_range_difference"], bool(f["circular"]))
        rem = np.isfinite(post) & (ln < int(f["speckle_min_run"]))
        n_sp = int(rem.sum())
        out[rem] = QNAN
    return out.view(F32), n_sh, n_sp


def filter_batch(ranges, beam_count, scan_processing, f):
    """(B, n_stride) ranges with per-scan beam counts, as rplgpu_filter_laserscan_batch_dev: beams at or
    beyond count keep what `ranges` holds there.  -> (ranges_out, removed (B, 2))."""
    out = np.array(ranges, F32, copy=True)
    removed = np.zeros((len(out), 2), np.int64)
    for b in range(len(out)):
        c = int(min(beam_count[b], out.shape[1]))
        if c == 0:
            continue
        inc = inc_mode_a(c) if scan_processing else inc_mode_b(c)
        out[b, :c], removed[b, 0], removed[b, 1] = filter_scan(ranges[b, :c], inc, f)
    return out, removed


def bisect_flip(r1, y, inc, f, which):
    """The two adjacent float32 values r2 (lo, hi) between which the decision `which` ('min' or 'max')
    of the pair (r1; neighbour at distance y) changes, found by bisection over the bit patterns."""
    s, c = e6_sincos(F32(F32(y) * F32(inc)))
    d = dirs(f)
    idx = 0 if which == "min" else 1

    def dec(bits):
        return bool(pair_tests(F32(r1), np.uint32(bits).view(F32), s, c, d)[idx])

    lo = int(F32(r1 * 1e-3).view(np.uint32))
    hi = int(F32(r1 * 1e3).view(np.uint32))
    assert dec(lo) != dec(hi), (which, dec(lo))
    d_lo = dec(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if dec(mid) == d_lo:
            lo = mid
        else:
            hi = mid
    return np.uint32(lo).view(F32), np.uint32(hi).view(F32)
