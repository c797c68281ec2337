"""The oracle of E28 (include/rplgpu_msg.h, the E28 block): rolled-out candidates weighed and blended into new controls,
and the next candidates spread around them.  Two writers that share no code: ``update_walk`` / ``spread_walk``, a
scalar walk in numpy.float32 scalars and Python integers with the finish in Python floats, and ``update_sweep`` /
``spread_sweep``, all candidates at once on arrays with int64 sums and numpy.float64.  Every float operation is rounded
once (numpy never fuses a product with a sum); int -> float64 is one round to nearest even in both (Python's float() of
an int, numpy's astype).  Nothing here loads the library."""
import numpy as np

ADMISSIBLE = 8
NO_WEIGHT, OFF_RANGE, EMPTY_STEP = 1, 2, 4
MAX_SHIFT, MAX_TABLE, MAX_STEPS, MAX_SPREAD_SHIFT, PER_LANE, BLOCK = 49, 65536, 256, 256, 8, 256
F32 = np.float32
_QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
_LIMIT = F32(8388608.0)
_TH = F32(1048576.0)

DEFAULT = dict(xy_scale=1024.0, shift=0, table_len=1024, steps=32, delta_per_step=1)


def spec(**kw):
    s = dict(DEFAULT)
    for k in kw:
        assert k in s, k
    s.update(kw)
    return s


def spec_valid(s):
    x = float(F32(s["xy_scale"]))
    return bool(np.isfinite(x) and x > 0 and 0 <= s["shift"] <= MAX_SHIFT and 1 <= s["table_len"] <= MAX_TABLE and
                1 <= s["steps"] <= MAX_STEPS and s["delta_per_step"] in (0, 1))


def steps_e(s):
    return s["steps"] if s["delta_per_step"] else 1


def struct_of(s):
    from rplidar_ros2_driver_amd import abi
    m = abi.Mppi()
    for k, v in s.items():
        setattr(m, k, v)
    return m


def layout(K, T_e):
    """-> (lanes of steps, rows, candidates a workgroup of the sums launch takes, its workgroups, the weights launch's)"""
    tw = 1
    while tw < T_e:
        tw *= 2
    rows = BLOCK // tw
    per = rows * PER_LANE
    return tw, rows, per, -(-K // per), -(-K // BLOCK)


def scratch_words(G, K, T_e):
    if not (1 <= G <= 65535 and 1 <= K <= (1 << 20) and 1 <= T_e <= MAX_STEPS and K * T_e <= (1 << 24)):
        return 0
    _, _, _, chunks, wb = layout(K, T_e)
    if chunks * G > (1 << 23) or wb * G > (1 << 23):
        return 0
    return 8 * wb * G + 12 * chunks * T_e * G


def _words64(v):
    v &= (1 << 64) - 1
    return [v & 0xFFFFFFFF, v >> 32]


# ---- writer 1: the scalar walk ---------------------------------------------------------------------------------------------
def update_walk(s, out, rres, delta, table, nominal=None):
    """-> (weights (K,) uint32, sums (T_e, 8) uint32, nominal_out (T_e, 4) float32, result (8,) uint32)"""
    T_e, N, sh = steps_e(s), s["table_len"], s["shift"]
    K = len(out)
    delta = np.asarray(delta, np.float32).reshape(K, T_e, 4)
    best = int(rres[2]) | (int(rres[3]) << 32)
    none = int(rres[7]) & 1
    xy = F32(s["xy_scale"])
    w = []
    clamped = 0
    for k in range(K):
        wk = 0
        if int(out[k][1]) & ADMISSIBLE and not none:
            sc = int(out[k][6]) | (int(out[k][7]) << 32)
            i = (sc - best if sc >= best else 0) >> sh
            if i > N - 1:
                i = N - 1
                clamped += 1
            wk = int(table[i])
        w.append(wk)
    sums = np.zeros((T_e, 8), np.uint32)
    nout = np.zeros((T_e, 4), np.float32)
    off = 0
    empty = False
    with np.errstate(all="ignore"):
        for t in range(T_e):
            W = sH = sX = sY = 0
            for k in range(K):
                if w[k] == 0:
                    continue
                dc, ds, dx, dy = (F32(v) for v in delta[k, t])
                h = ds / (F32(1.0) + dc)
                th, tx, ty = h * _TH, dx * xy, dy * xy
                if not (abs(th) < _LIMIT and abs(tx) < _LIMIT and abs(ty) < _LIMIT):
                    off += 1
                    continue
                W += w[k]
                sH += w[k] * int(np.rint(th))
                sX += w[k] * int(np.rint(tx))
                sY += w[k] * int(np.rint(ty))
            sums[t] = _words64(W) + _words64(sH) + _words64(sX) + _words64(sY)
            if W > 0:
                dW = float(W)
                hb = (float(sH) / dW) * (1.0 / 1048576.0)
                hh = hb * hb
                den = 1.0 + hh
                nout[t] = [F32((1.0 - hh) / den), F32((hb + hb) / den), F32((float(sX) / dW) / float(xy)),
                           F32((float(sY) / dW) / float(xy))]
            else:
                empty = True
                nout[t] = np.asarray(nominal, np.float32).reshape(T_e, 4)[t] if nominal is not None else [1, 0, 0, 0]
    if nominal is not None:   # (bit for bit: a NaN's payload too)
        nb = np.asarray(nominal, np.float32).reshape(T_e, 4).view(np.uint32)
        for t in range(T_e):
            if not any(sums[t][:2]):
                nout.view(np.uint32)[t] = nb[t]
    n_w = sum(1 for v in w if v)
    sw, sw2 = sum(w), sum(v * v for v in w)
    flags = (NO_WEIGHT if n_w == 0 else 0) | (OFF_RANGE if off else 0) | (EMPTY_STEP if empty else 0)
    result = np.array([n_w, clamped] + _words64(sw) + _words64(sw2) + [off, flags], np.uint64).astype(np.uint32)
    return np.array(w, np.uint32), sums, nout, result


def _canon1(v):
    return _QNAN if v != v else v


def spread_walk(nominal, noise, shift=0, keep_first=0):
    """-> (K, T, 4) float32"""
    nominal = np.asarray(nominal, np.float32).reshape(-1, 4)
    noise = np.asarray(noise, np.float32)
    K, T = noise.shape[:2]
    T_n = len(nominal)
    out = np.zeros((K, T, 4), np.float32)
    with np.errstate(all="ignore"):
        for k in range(K):
            for t in range(T):
                p = nominal[min(t + shift, T_n - 1)]
                if keep_first and k == 0:
                    out.view(np.uint32)[k, t] = p.view(np.uint32)
                    continue
                c, sn, x, y = (F32(v) for v in p)
                dc, ds, dx, dy = (F32(v) for v in noise[k, t])
                out[k, t] = [_canon1(c * dc - sn * ds), _canon1(sn * dc + c * ds), _canon1((c * dx - sn * dy) + x),
                             _canon1((sn * dx + c * dy) + y)]
    return out


# ---- writer 2: every candidate at once ------------------------------------------------------------------------------------------
def update_sweep(s, out, rres, delta, table, nominal=None):
    """-> (weights (K,) uint32, sums (T_e, 8) uint32, nominal_out (T_e, 4) float32, result (8,) uint32)"""
    T_e, N = steps_e(s), s["table_len"]
    out = np.asarray(out, np.uint32)
    rres = np.asarray(rres, np.uint32)
    K = len(out)
    d = np.asarray(delta, np.float32).reshape(K, T_e, 4)
    score = out[:, 6].astype(np.uint64) | (out[:, 7].astype(np.uint64) << np.uint64(32))
    best = np.uint64(rres[2]) | (np.uint64(rres[3]) << np.uint64(32))
    gate = ((out[:, 1] & ADMISSIBLE) != 0) & ((rres[7] & 1) == 0)
    diff = np.where(score >= best, score - best, np.uint64(0)) >> np.uint64(s["shift"])
    clamped = gate & (diff > np.uint64(N - 1))
    idx = np.minimum(diff, np.uint64(N - 1)).astype(np.int64)
    w = np.where(gate, np.asarray(table, np.uint16)[idx].astype(np.int64), 0)
    xy = F32(s["xy_scale"])
    with np.errstate(all="ignore"):
        h = d[..., 1] / (F32(1.0) + d[..., 0])
        th, tx, ty = h * _TH, d[..., 2] * xy, d[..., 3] * xy
        ok = (np.abs(th) < _LIMIT) & (np.abs(tx) < _LIMIT) & (np.abs(ty) < _LIMIT)    # (K, T_e)
        q = [np.where(ok, np.rint(np.where(ok, v, 0)), 0).astype(np.int64) for v in (th, tx, ty)]
    live = ok & (w != 0)[:, None]
    wt = np.where(live, w[:, None], 0)                                                 # (K, T_e) int64
    cols = [wt.sum(axis=0)] + [(wt * v).sum(axis=0) for v in q]                        # four (T_e,) int64, exact
    sums = np.stack(cols, axis=1).astype(np.int64).view(np.uint32).reshape(T_e, 8)     # low word first
    W = cols[0]
    has = W > 0
    with np.errstate(all="ignore"):
        dW = np.where(has, W, 1).astype(np.float64)
        hb = (cols[1].astype(np.float64) / dW) * np.float64(1.0 / 1048576.0)
        hh = hb * hb
        den = np.float64(1.0) + hh
        new = np.stack([(np.float64(1.0) - hh) / den, (hb + hb) / den, (cols[2].astype(np.float64) / dW) / np.float64(xy),
                        (cols[3].astype(np.float64) / dW) / np.float64(xy)], axis=1).astype(np.float32)
    keep = np.tile(np.array([1, 0, 0, 0], np.float32), (T_e, 1)) if nominal is None else \
        np.asarray(nominal, np.float32).reshape(T_e, 4)
    nout = np.where(has[:, None], new.view(np.uint32), keep.view(np.uint32)).astype(np.uint32).view(np.float32)
    off = int((~ok & (w != 0)[:, None]).sum())
    n_w = int((w != 0).sum())
    sw, sw2 = int(w.sum()), int((w * w).sum())
    flags = (NO_WEIGHT if n_w == 0 else 0) | (OFF_RANGE if off else 0) | (EMPTY_STEP if (~has).any() else 0)
    result = np.array([n_w, int(clamped.sum())] + _words64(sw) + _words64(sw2) + [off, flags],
                      np.uint64).astype(np.uint32)
    return w.astype(np.uint32), sums, nout, result


def spread_sweep(nominal, noise, shift=0, keep_first=0):
    """-> (K, T, 4) float32"""
    nominal = np.asarray(nominal, np.float32).reshape(-1, 4)
    noise = np.asarray(noise, np.float32)
    K, T = noise.shape[:2]
    p = nominal[np.minimum(np.arange(T) + shift, len(nominal) - 1)]      # (T, 4)
    c, sn, x, y = (p[None, :, i] for i in range(4))
    dc, ds, dx, dy = (noise[..., i] for i in range(4))
    with np.errstate(all="ignore"):
        out = np.stack([c * dc - sn * ds, sn * dc + c * ds, (c * dx - sn * dy) + x, (sn * dx + c * dy) + y],
                       axis=2).astype(np.float32)
    out[np.isnan(out)] = _QNAN
    if keep_first:
        out.view(np.uint32)[0] = p.view(np.uint32)
    return out


def equal(a, b):
    """Two tuples of arrays agree byte for byte."""
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
