"""The inputs of E28's tests (tests/test_mppi_cpu.py, tests/test_gpu_mppi.py) and, per family, the regime each case is
in, asserted from tests/mppi_oracle.py alone: a case that no longer reaches the edge it was built for fails here, with
or without the library.  E27's words are made by hand (``scored``), so E28 is tested apart from E27."""
import functools

import numpy as np

from tests import mppi_oracle as mo

ADM = mo.ADMISSIBLE
ALL_ONES = (1 << 64) - 1


def table_of(lam, shift, N):
    """The softmax table in numpy (not the library's)."""
    t = np.floor(65535.0 * np.exp(-(np.arange(N, dtype=np.float64) * 2.0 ** shift) / lam) + 0.5).astype(np.uint16)
    t[0] = 65535
    return t


def scored(scores, adm, rng=None, T=1):
    """E27's eight words per candidate and its result words for the given scores (Python ints) and admissible mask;
    the words E28 does not read hold other values."""
    K = len(scores)
    out = np.zeros((K, 8), np.uint32)
    if rng is not None:
        out[:, 2:6] = rng.integers(0, 1 << 32, (K, 4), dtype=np.uint64).astype(np.uint32)
    out[:, 0] = T
    sc = [int(s) if a else ALL_ONES for s, a in zip(scores, adm)]
    out[:, 1] = [ADM if a else 1 for a in adm]
    out[:, 6] = [s & 0xFFFFFFFF for s in sc]
    out[:, 7] = [s >> 32 for s in sc]
    ks = [k for k in range(K) if adm[k]]
    best = min((sc[k] for k in ks), default=ALL_ONES)
    same = [k for k in ks if sc[k] == best]
    rres = np.array([len(ks), same[0] if same else 0xFFFFFFFF, best & 0xFFFFFFFF, best >> 32, len(same), K - len(ks),
                     0, 0 if ks else 1], np.uint64).astype(np.uint32)
    return out, rres


def deltas(rng, K, T_e, turn=0.6):
    th = rng.uniform(-turn, turn, (K, T_e))
    return np.stack([np.cos(th), np.sin(th), rng.uniform(-0.3, 0.5, (K, T_e)), rng.uniform(-0.1, 0.1, (K, T_e))],
                    axis=2).astype(np.float32)


def nominal_of(rng, T_e):
    return deltas(rng, 1, T_e, 0.2)[0]


def case(name, K, T, per_step=1, seed=0, share_adm=0.8, top=5000, nominal=True, **kw):
    rng = np.random.default_rng(seed)
    s = mo.spec(**dict(dict(steps=T, delta_per_step=per_step, table_len=64, shift=4), **kw))
    T_e = mo.steps_e(s)
    adm = rng.random(K) < share_adm
    out, rres = scored(rng.integers(100, 100 + top, K).tolist(), adm, rng, T)
    return dict(name=name, spec=s, out=out, rres=rres, delta=deltas(rng, K, T_e),
                table=table_of(300.0, s["shift"], s["table_len"]), nominal=nominal_of(rng, T_e) if nominal else None)


@functools.lru_cache(maxsize=None)
def _want(key):
    c = _REG[key]
    return mo.update_sweep(c["spec"], c["out"], c["rres"], c["delta"], c["table"], c["nominal"])


_REG = {}


def want(c):
    """The sweep's answer for a case, computed once and left unchanged."""
    key = (c["name"], id(c["delta"]))
    _REG[key] = c
    return _want(key)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (31, 2, 1), (32, 31, 1), (33, 33, 1), (257, 56, 1), (257, 65, 1), (40, 256, 1), (33, 7, 0),
          (3000, 12, 0), (1100, 5, 1)]


@functools.lru_cache(maxsize=None)
def shape_case(K, T, per_step):
    return case(f"shape_{K}_{T}_{per_step}", K, T, per_step, seed=K * 1000 + T)


@functools.lru_cache(maxsize=None)
def shapes_regime():
    lay = {sh: mo.layout(sh[0], sh[1] if sh[2] else 1) for sh in SHAPES}
    assert any(l[3] > l[1] > 1 for l in lay.values())           # the close takes a second round over the records
    assert any(l[3] > 1 and l[4] > 1 for l in lay.values())     # several workgroups in both launches
    assert any(l[0] == 256 and l[1] == 1 for l in lay.values()) and any(l[0] == 1 for l in lay.values())
    assert any(l[0] < 64 for l in lay.values()) and any(l[0] > (sh[1] if sh[2] else 1) for sh, l in lay.items())
    for sh in SHAPES:
        w, sums, nout, res = want(shape_case(*sh))
        assert res[7] == 0 or sh[0] == 1, (sh, res.tolist())
        assert 0 < res[1] < res[0] or sh[0] < 31, (sh, res.tolist())   # an index clamped and one not
    return True


@functools.lru_cache(maxsize=None)
def group_cases(per_step=1, G=3):
    return tuple(case(f"group{g}_{per_step}", 70, 9, per_step, seed=50 + g) for g in range(G))


# ---- weights --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight_cases():
    c = {}
    rng = np.random.default_rng(7)
    K, T = 45, 6
    base = case("w_base", K, T, seed=9)
    none = dict(base, name="none_admissible")
    none["out"], none["rres"] = scored([5] * K, [False] * K, rng, T)
    c["none_admissible"] = none
    c["none_admissible_no_nominal"] = dict(none, name="none_admissible_no_nominal", nominal=None)
    scores = rng.permutation(K).astype(int) + 40
    o, r = scored(scores.tolist(), [True] * K, rng, T)
    c["best_only"] = dict(base, name="best_only", out=o, rres=r, spec=dict(base["spec"], table_len=2, shift=0),
                          table=np.array([65535, 0], np.uint16))
    c["shift_0"] = dict(case("shift_0", K, T, seed=11, shift=0, top=90), )
    big = [int(v) for v in rng.integers(0, 1 << 50, K - 2)] + [(1 << 50) - 1, 0]
    o, r = scored(big, [True] * K, rng, T)
    c["shift_49"] = dict(base, name="shift_49", out=o, rres=r, spec=dict(base["spec"], shift=49, table_len=2),
                         table=np.array([65535, 1234], np.uint16))
    # the result's best above some candidates' scores (by hand: E27 would not write this)
    r2 = r.copy()
    r2[2], r2[3] = 0, 1 << 17
    c["below_best"] = dict(base, name="below_best", out=o, rres=r2, spec=dict(base["spec"], shift=40, table_len=700),
                           table=table_of(200.0, 0, 700))
    o, r = scored((np.arange(K) * 3).tolist(), [True] * K, rng, T)
    c["clamp_n1"] = dict(base, name="clamp_n1", out=o, rres=r, spec=dict(base["spec"], shift=0, table_len=1),
                         table=np.array([777], np.uint16))
    o, r = scored((np.arange(K) * 3000).tolist(), [True] * K, rng, T)
    c["clamp_n65536"] = dict(base, name="clamp_n65536", out=o, rres=r,
                             spec=dict(base["spec"], shift=0, table_len=65536), table=table_of(40000.0, 0, 65536))
    # all weights 65535 and |H| near 2^23: a sum beyond 2^53, where int64 -> double rounds
    Kb = 20000
    o, r = scored([3] * Kb, [True] * Kb, None, 4)
    d = np.zeros((Kb, 1, 4), np.float32)
    d[:, 0, 1] = (7.5 + np.arange(Kb) * 2.0 ** -16).astype(np.float32)   # dc = 0: h = ds
    d[0, 0, 1] = 7.5 + 2.0 ** -20                                         # (an odd sum: it is no double)
    d[:, 0, 2] = 0.001 * np.arange(Kb)
    c["big_sums"] = dict(name="big_sums", spec=mo.spec(steps=4, delta_per_step=0, table_len=1, shift=0), out=o, rres=r,
                         delta=d, table=np.array([65535], np.uint16), nominal=None)
    return c


@functools.lru_cache(maxsize=None)
def weight_regime():
    c = weight_cases()
    for name in ("none_admissible", "none_admissible_no_nominal"):
        w, sums, nout, res = want(c[name])
        assert not w.any() and not sums.any() and res.tolist() == [0, 0, 0, 0, 0, 0, 0, mo.NO_WEIGHT | mo.EMPTY_STEP]
        keep = c[name]["nominal"]
        assert nout.tobytes() == (keep.tobytes() if keep is not None else
                                  np.tile(np.array([1, 0, 0, 0], np.float32), (len(nout), 1)).tobytes())
    w, sums, nout, res = want(c["best_only"])
    k = int(c["best_only"]["rres"][1])
    assert res[0] == 1 and w[k] == 65535 and res[1] == len(w) - 2   # every index above 1 is clamped
    d = c["best_only"]["delta"][k]
    assert np.allclose(nout, d, atol=2e-3) and nout.tobytes() != d.tobytes()   # re-expressed, to the quantum
    w, _, _, res = want(c["shift_0"])
    assert res[0] > 0 and len(set(w.tolist())) > 20
    w, _, _, res = want(c["shift_49"])
    o = c["shift_49"]["out"]
    assert int(o[-2, 6]) | (int(o[-2, 7]) << 32) == (1 << 50) - 1 and w[-2] == 1234 and w[-1] == 65535
    assert set(w.tolist()) == {65535, 1234} and res[1] == 0
    w, _, _, res = want(c["below_best"])
    below = [(int(a) | (int(b) << 32)) < (1 << 49) for a, b in c["below_best"]["out"][:, 6:8]]
    assert 0 < sum(below) < len(w) and all(w[k] == 65535 for k in range(len(w)) if below[k]) and (w < 65535).any()
    w, _, _, res = want(c["clamp_n1"])
    assert (w == 777).all() and res[1] == len(w) - 1
    w, _, _, res = want(c["clamp_n65536"])
    assert 0 < res[1] < len(w) - 1 and w[65535 // 3000] > w[-1]
    w, sums, nout, res = want(c["big_sums"])
    sH = int(sums[0, 2]) | (int(sums[0, 3]) << 32)
    assert (w == 65535).all() and (1 << 53) < sH < (1 << 59) and int(float(sH)) != sH
    return True


# ---- ranges ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_cases():
    c = {}
    K, T = 37, 5
    base = case("r_base", K, T, seed=21, share_adm=1.0, top=600)
    d = base["delta"].copy()
    d[3, 1] = [np.nan, 0, 0, 0]
    d[4, 2] = [1, 0, np.inf, 0]
    d[5, 0] = [1, 0, 0, -np.inf]
    d[6, 3] = [-1, 0, 0.1, 0]          # the half turn: 0 / 0
    d[7, 3] = [-1, 0.5, 0.1, 0]        # ... and x / 0
    d[8, 4] = [0, 1, 8192.0, 0]        # tx = 2^23 at xy_scale 1024
    c["not_finite"] = dict(base, name="not_finite", delta=d)
    d = base["delta"].copy()
    below = np.nextafter(np.float32(8.0), np.float32(0.0))
    d[0, 0] = [0, below, 0, 0]
    d[1, 0] = [0, -below, 0, 0]
    d[2, 1] = [0, 8.0, 0, 0]
    d[3, 2] = [0, -8.0, 0, 0]
    c["h_edges"] = dict(base, name="h_edges", delta=d)
    d = base["delta"].copy()
    d[:, 2] = [np.nan, 0, 0, 0]
    c["empty_step"] = dict(base, name="empty_step", delta=d)
    c["empty_step_no_nominal"] = dict(base, name="empty_step_no_nominal", delta=d, nominal=None)
    nom = base["nominal"].copy()
    nom.view(np.uint32)[2] = [0x7FC00123, 0x80000000, 0x7F800000, 0x00000001]   # kept bit for bit
    c["empty_step_odd_nominal"] = dict(base, name="empty_step_odd_nominal", delta=d, nominal=nom)
    return c


@functools.lru_cache(maxsize=None)
def range_regime():
    c = range_cases()
    base = want(dict(c["not_finite"], name="r_base_plain", delta=case("r_base", 37, 5, seed=21, share_adm=1.0,
                                                                        top=600)["delta"]))
    assert base[3][6] == 0 and base[3][7] == 0
    w, sums, nout, res = want(c["not_finite"])
    assert (w != 0).all() and res[6] == 6 and res[7] == mo.OFF_RANGE and np.isfinite(nout).all()
    w, sums, nout, res = want(c["h_edges"])
    assert res[6] == 2 and (w[:4] != 0).all()
    d = c["h_edges"]["delta"]
    th = d[2, 1, 1] * np.float32(1048576.0)
    assert th == np.float32(8388608.0) and d[0, 0, 1] * np.float32(1048576.0) == np.float32(8388607.5)
    # this entry's |th| is the first float at or above 8388608; the one before it rounds (ties to even) to 2^23
    assert np.nextafter(th, np.float32(0)) < np.float32(8388608.0) and int(np.rint(np.float32(8388607.5))) == 1 << 23
    for name in ("empty_step", "empty_step_no_nominal", "empty_step_odd_nominal"):
        w, sums, nout, res = want(c[name])
        Wt = sums[:, 0].astype(np.int64) + (sums[:, 1].astype(np.int64) << 32)
        assert (Wt == 0).tolist() == [False, False, True, False, False], name    # exactly one step has W_t = 0
        assert res[7] == mo.OFF_RANGE | mo.EMPTY_STEP and res[6] == int((w != 0).sum())
        keep = c[name]["nominal"]
        assert nout[2].tobytes() == (keep[2].tobytes() if keep is not None else np.array([1, 0, 0, 0],
                                                                                         np.float32).tobytes())
    return True


# ---- the spread -----------------------------------------------------------------------------------------------------------------
SPREADS = [("shift_0", 33, 7, 7, 0, 0), ("shift_1", 33, 7, 7, 1, 0), ("shift_beyond", 5, 9, 4, 200, 0),
           ("keep_first", 65, 6, 6, 1, 1), ("short_nominal", 300, 3, 1, 0, 1), ("one", 1, 1, 1, 0, 0),
           ("long", 9, 256, 256, 3, 0)]


@functools.lru_cache(maxsize=None)
def spread_case(name):
    _, K, T, T_n, shift, keep = next(s for s in SPREADS if s[0] == name)
    rng = np.random.default_rng(len(name) + K)
    nominal = nominal_of(rng, T_n)
    noise = deltas(rng, K, T, 0.1)
    if K > 4 and T > 2:
        noise[2, 1] = [np.nan, 1, 0, 0]
        noise[3, 2] = [np.inf, 0, 1, 0]
    return dict(name=name, nominal=nominal, noise=noise, shift=shift, keep_first=keep)


@functools.lru_cache(maxsize=None)
def spread_want(name):
    c = spread_case(name)
    return mo.spread_sweep(c["nominal"], c["noise"], c["shift"], c["keep_first"])


@functools.lru_cache(maxsize=None)
def spread_regime():
    for name, K, T, T_n, shift, keep in SPREADS:
        c, w = spread_case(name), spread_want(name)
        assert w.shape == (K, T, 4)
        if keep:
            idx = np.minimum(np.arange(T) + shift, T_n - 1)
            assert w[0].tobytes() == c["nominal"][idx].tobytes() and (K == 1 or w[1].tobytes() != w[0].tobytes())
    w = spread_want("shift_0").view(np.uint32)
    assert (w[2, 1] == 0x7FC00000).any() and (w[3, 2] == 0x7F800000).any()   # a NaN is canonical, an Inf passes
    assert spread_want("shift_1").tobytes() != w.tobytes()
    c = spread_case("shift_beyond")   # every step reads the last nominal delta
    assert mo.spread_sweep(np.tile(c["nominal"][-1], (4, 1)), c["noise"]).tobytes() == spread_want("shift_beyond").tobytes()
    return True
