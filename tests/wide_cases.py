"""The inputs of tests/test_gpu_wide.py (E24), each with a regime check made from the oracle alone
(tests/wide_oracle.py): the check asserts that the case exercises what it claims, so a green test cannot be an empty
one.  tests/test_wide_cpu.py runs every regime without a device.  If a regime check fails, the input is what changes,
never the check.  TEST INFRASTRUCTURE — imported by tests/ only.

A case is the dict of tests/match_cases.py whose spec carries max_blocks (tests/wide_oracle.spec)."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import Params, abi
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import match_path_cases as mpc
from tests import wide_oracle as wo
from tests.occ_cases import nodes, pad

F32 = np.float32
S = wo.S
_CACHE = {}


def widened(case, max_blocks=None, **shifts):
    """A case of tests/match_cases.py as an E24 case: the same spec with a cap (by default the whole volume, so the
    result is proven), other shifts when given."""
    s = dict(case["spec"], max_blocks=1, **shifts)
    s["max_blocks"] = wo.blocks_size(s) if max_blocks is None else max_blocks
    return dict(case, spec=s)


def capped(case, max_blocks):
    return dict(case, spec=dict(case["spec"], max_blocks=max_blocks))


def case_want(oracle, case, key=None):
    """Per group writer 2's dict (tests/wide_oracle.match_bound_refine) with the truncated bit in its status,
    computed once per key."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    n = case["batch"].shape[1]
    out = []
    for g, sl in enumerate(mc.case_groups(case)):
        x, y = mc.case_points(oracle, case, g)
        w = wo.match_bound_refine(x, y, mc.case_pivot(case, g), case["spec"], mc.case_field(case, g))
        if any(int(case["lens"][b]) > n for b in range(sl.start, sl.stop)):
            w["status"] |= abi.SCAN_OUT_TRUNCATED
        out.append(w)
    if key is not None:
        _CACHE[key] = out
    return out


def case_exhaustive(oracle, case, key=None):
    """Per group writer 1's (volume, best, status without the truncated bit), computed once per key."""
    key = None if key is None else "x_" + key
    if key is not None and key in _CACHE:
        return _CACHE[key]
    out = []
    for g in range(len(mc.case_groups(case))):
        x, y = mc.case_points(oracle, case, g)
        out.append(wo.match_exhaustive(x, y, mc.case_pivot(case, g), case["spec"], mc.case_field(case, g)))
    if key is not None:
        _CACHE[key] = out
    return out


def bound_holds(case, want, exhaustive):
    """U is at least the best score of its block, block by block, from the exhaustive volume."""
    s = case["spec"]
    rots, nby, nbx = wo.blocks_shape(s)
    for w, (vol, _, _) in zip(want, exhaustive):
        ny, nx = vol.shape[1:]
        full = np.zeros((rots, nby * S, nbx * S), np.int64)
        full[:, :ny, :nx] = vol
        top = full.reshape(rots, nby, S, nbx, S).max((2, 4))
        assert (w["U"].astype(np.int64) >= top).all()
    return True


def writers_agree(want, exhaustive):
    """A proven result is writer 1's, words 0 - 6; an unproven one is at most writer 1's and says so."""
    for w, (_, best, status) in zip(want, exhaustive):
        if w["best"][7] == 0:
            assert w["best"][:7].tolist() == best[:7].tolist(), (w["best"], best)
        else:
            assert w["best"][7] == wo.UNPROVEN and w["best"][0] <= best[0] and w["work"][4] > w["work"][5]
            assert w["best"][4:6].tolist() == best[4:6].tolist()
        assert w["status"] & ~abi.SCAN_OUT_TRUNCATED == status
    return True


# ---- 1: recovery beyond E13's reach ----------------------------------------------------------------------------------
RECOVERY_SPEC = wo.spec(shift_x=40, shift_y=40, rot_steps=2, rot_step=float(F32(math.radians(1.0))), max_blocks=1024,
                        **mc.ROOM_GRID)
RECOVERY_DISPLACEMENTS = ((1, -36, 38), (-2, 33, -5), (2, 7, -40))  # (k0, j0, i0): |i0| or |j0| in 33 .. 40


def recovery_case(oracle, disp):
    batch, lens, pose2d = mc.room_scans()
    k0, j0, i0 = disp
    return dict(batch=batch, lens=lens, group=2, p=Params.defaults(**mc.ROOM_P), spec=RECOVERY_SPEC,
                fields=mc.room_field(oracle),
                pose2d=mo.displaced_poses(pose2d, mc.ROOM_PIVOT[0], RECOVERY_SPEC, k0, j0, i0), pivot=mc.ROOM_PIVOT,
                disp=disp)


def recovery_regime(oracle, case):
    """Out of E13's reach, the exact inverse, unambiguous and proven."""
    k0, j0, i0 = case["disp"]
    assert max(abs(i0), abs(j0)) > mo.MAX_SHIFT and 33 <= max(abs(i0), abs(j0)) <= 40
    w = case_want(oracle, case, f"recovery{case['disp']}")[0]
    assert w["status"] == 0 and w["best"][4] == 2 * mc.ROOM_N
    assert tuple(w["best"][1:4]) == (-k0, -j0, -i0) and w["best"][6] == 1 and w["best"][7] == 0, w["best"]
    assert w["best"][5] < w["best"][0]
    return w


# ---- 2: the cases E13 has, for the identity on the device ---------------------------------------------------------------
def identity_cases(oracle):
    """name -> case with T <= 32, proven: match_cases' room, edge, tie and front cases."""
    out = {f"room{d}": widened(mc.room_case(oracle, d)) for d in mc.ROOM_DISPLACEMENTS[1:]}
    out.update({f"edge_{n}": widened(c) for n, c in mc.edge_cases().items()})
    out.update({f"tie_{n}": widened(c[0]) for n, c in mc.tie_cases().items()})
    out["front"] = widened(mc.front_case())
    return out


def identity_regime(oracle, name, case):
    s = case["spec"]
    assert mo.spec_valid(wo.scan_match_spec(s)) and wo.spec_valid(s)
    w = case_want(oracle, case, f"id_{name}")[0]
    e13 = mc.case_want(oracle, dict(case, spec=wo.scan_match_spec(s)), f"id13_{name}")[0]
    assert w["best"][7] == 0 and w["best"][:7].tolist() == e13[1][:7].tolist(), (name, w["best"], e13[1])
    return w


# ---- 3: the list --------------------------------------------------------------------------------------------------------
NOISY_SEED = 2400  # (the first seed from 2400 on at which the oracle says what noisy_regime asks)
NOISY_DISP = (-1, 21, -34)
NOISY_CLUTTER = 300


def noisy_case(oracle, seed=NOISY_SEED):
    """The room displaced by NOISY_DISP, every range with 5 cm (one cell) of noise, and 300 clutter cells of value
    100 scattered over the field: bounds that the true scores do not reach."""
    rng = np.random.default_rng(seed)
    batch, lens, pose2d = mc.room_scans()
    batch = batch.copy()
    d = batch["dist_mm_q2"].astype(np.int64)
    batch["dist_mm_q2"] = np.where(d > 0, np.maximum(d + np.round(rng.normal(0.0, 0.05 * 4000.0, d.shape)), 400), 0)
    field = mc.room_field(oracle).copy()
    H, W = field.shape[1:]
    field[0, rng.integers(0, H, NOISY_CLUTTER), rng.integers(0, W, NOISY_CLUTTER)] = 100
    k0, j0, i0 = NOISY_DISP
    return dict(batch=batch, lens=lens, group=2, p=Params.defaults(**mc.ROOM_P), spec=RECOVERY_SPEC, fields=field,
                pose2d=mo.displaced_poses(pose2d, mc.ROOM_PIVOT[0], RECOVERY_SPEC, k0, j0, i0), pivot=mc.ROOM_PIVOT)


def noisy_verdict(w, s):
    """(2 < n < blocks / 2, seed A is not the block of the best): what the regime asks of writer 2's result."""
    blocks, n, seed_a = int(w["work"][0]), int(w["work"][4]), int(w["work"][2])
    return 2 < n < blocks // 2, seed_a != wo.block_of(s, *(int(v) for v in w["best"][1:4]))


def noisy_regime(oracle, case, key="noisy"):
    """The list is neither trivial nor everything, and the floor rises only in refine: the best lies in a block that
    is not seed A, with a score above b0."""
    w = case_want(oracle, case, key)[0]
    sized, elsewhere = noisy_verdict(w, case["spec"])
    assert sized and elsewhere, (w["work"], w["best"])
    assert w["best"][7] == 0 and w["best"][0] > w["work"][3] and w["best"][6] == 1
    return w


PEAK_GRID = dict(origin_x=0.0, origin_y=0.0, resolution=0.25, width=32, height=32)
PEAK_SPEC = wo.spec(shift_x=4, shift_y=4, rot_steps=1, rot_step=0.5, max_blocks=1024, **PEAK_GRID)
PEAK_SENSOR = (0.125, 2.625)  # the middle of cell (0, 10); the one return lies 5 m ahead, in cell (20, 10)
PEAK_VALUE = 90


def equal_peaks_case(oracle):
    """One point, two isolated field cells of equal value: one within the window only at rotation -1 (2 right, 1 up
    of the turned point), one only at rotation +1 (3 left, 1 up)."""
    scan = nodes(np.zeros(1, np.int64), np.full(1, 20000, np.int64))
    batch, lens = pad([scan], 4)
    case = dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=PEAK_SPEC,
                fields=np.zeros((1, 32, 32), np.int8),
                pose2d=np.array([[1, 0, PEAK_SENSOR[0], 0, 1, PEAK_SENSOR[1]]], F32),
                pivot=np.array([PEAK_SENSOR], F32))
    x, y = mc.case_points(oracle, case, 0)
    rot = mo.rotations(PEAK_SPEC)
    at = [mo.rotated_cells(x, y, PEAK_SENSOR[0], PEAK_SENSOR[1], rot[kk, 0], rot[kk, 1], PEAK_SPEC) for kk in range(3)]
    (cx0, cy0), (cx2, cy2) = [(int(a[1][0]), int(a[2][0])) for a in (at[0], at[2])]
    case["fields"][0, cy0 + 1, cx0 + 2] = PEAK_VALUE
    case["fields"][0, cy2 + 1, cx2 - 3] = PEAK_VALUE
    return case


def equal_peaks_regime(oracle, case):
    """U equals b0 at the second block, two candidates tie and the nearer one wins."""
    w = case_want(oracle, case, "equal_peaks")[0]
    s = case["spec"]
    first, second = wo.block_of(s, -1, 1, 2), wo.block_of(s, 1, 1, -3)
    assert first != second and first // 4 != second // 4  # other blocks, other rotations
    assert w["work"][2] == first and w["work"][3] == PEAK_VALUE == w["U"].ravel()[second]
    assert sorted(w["listed"].tolist()) == [first, second] and w["work"][4] == 2
    assert w["best"].tolist() == [PEAK_VALUE, -1, 1, 2, 1, 0, 2, 0], w["best"]
    return w


def uniform_case():
    """match_cases' uniform tie (five points, every byte 100) with a window of 3 x 3 blocks a rotation."""
    return widened(mc.tie_cases()["uniform"][0], shift_x=9, shift_y=9)


def uniform_regime(oracle, case, key="uniform"):
    """Every block listed, and the best is (0, 0, 0)."""
    w = case_want(oracle, case, key)[0]
    assert w["work"][0] == 45 == w["work"][4] == len(w["listed"]) and w["work"][3] == 500
    if w["work"][4] <= w["work"][5]:
        assert w["best"][:6].tolist() == [500, 0, 0, 0, 5, 500] and w["best"][6] > 45 and w["best"][7] == 0, w["best"]
    return w


FAR_TIES = {  # name -> (W, H, the sensor's cell, Tx, Ty, the two peaks as shifts (i, j): the winner first)
    "12_bits": (160, 32, (0, 10), 64, 4, ((10, 0), (64, 2))),          # 100 against 4100 = 4096 + 4
    "17_bits": (600, 600, (290, 300), 256, 256, ((-256, 255), (256, 256))),  # 130561 against 131072 = 2^17
}


def far_ties_case(name):
    """One point (2.5 m ahead of the sensor: 10 cells of 25 cm) and two isolated field cells of equal value whose
    i*i + j*j differ only above the bits E13's tie key had: the nearer one must win."""
    W, H, (sx, sy), Tx, Ty, peaks = FAR_TIES[name]
    scan = nodes(np.zeros(1, np.int64), np.full(1, 10000, np.int64))
    batch, lens = pad([scan], 4)
    sensor = ((sx + 0.5) * 0.25, (sy + 0.5) * 0.25)
    field = np.zeros((1, H, W), np.int8)
    for i, j in peaks:
        field[0, sy + j, sx + 10 + i] = 80
    s = wo.spec(origin_x=0.0, origin_y=0.0, resolution=0.25, width=W, height=H, shift_x=Tx, shift_y=Ty, rot_steps=0,
                rot_step=0.0, max_blocks=1024)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=s, fields=field,
                pose2d=np.array([[1, 0, sensor[0], 0, 1, sensor[1]]], F32), pivot=np.array([sensor], F32))


def far_ties_regime(oracle, name, case):
    (i0, j0), (i1, j1) = FAR_TIES[name][5]
    d0, d1 = i0 * i0 + j0 * j0, i1 * i1 + j1 * j1
    bits = int(name.split("_")[0])
    assert d0 < d1 and (d1 & ((1 << bits) - 1)) < (d0 & ((1 << bits) - 1))  # a key of that many bits picks the other
    w = case_want(oracle, case, f"far_{name}")[0]
    assert w["best"].tolist() == [80, 0, j0, i0, 1, 0, 2, 0], w["best"]
    return w


# ---- 4: the cap -----------------------------------------------------------------------------------------------------------
def cap_cases(oracle):
    """name -> (case, proven): the noisy room with max_blocks = n, n - 1 and 1, the uniform field with 1."""
    base = noisy_case(oracle)
    n = int(case_want(oracle, base, "noisy")[0]["work"][4])
    return {"noisy_n": (capped(base, n), True), "noisy_n-1": (capped(base, n - 1), False),
            "noisy_1": (capped(base, 1), False), "uniform_1": (capped(uniform_case(), 1), False)}


def cap_regime(oracle, name, case, proven):
    w = case_want(oracle, case, f"cap_{name}")[0]
    full = case_want(oracle, noisy_case(oracle), "noisy")[0] if name.startswith("noisy") else \
        case_want(oracle, uniform_case(), "uniform")[0]
    assert (w["best"][7] == 0) == proven and (w["work"][4] <= w["work"][5]) == proven
    assert w["work"][:5].tolist() == full["work"][:5].tolist() and (w["U"] == full["U"]).all()
    if proven:
        assert w["best"].tolist() == full["best"].tolist()
    else:
        assert w["best"][7] == wo.UNPROVEN and w["best"][0] == w["work"][3] <= full["best"][0]
        assert set(w["scores"]) == set(w["seeds"])  # nothing beyond the seeds is scored
    if name.startswith("noisy") and not proven:
        assert w["best"][0] < full["best"][0]  # the seeds alone miss the best
    return w


# ---- 5: layouts -------------------------------------------------------------------------------------------------------------
def layout_of(Tx, Ty):
    """(nb, per, slices, owned) by the formula in k_wide_bound: nb blocks a rotation, a copy of them takes `per`
    threads (whole waves, at most 1024), `slices` copies fit the workgroup; above 1024 blocks there is one copy and a
    thread owns up to `owned` of them."""
    nb = ((2 * Tx + S) // S) * ((2 * Ty + S) // S)
    per = min((nb + 63) & ~63, 1024)
    slices = 1024 // per if nb <= 1024 else 1
    return nb, per, slices, (nb + 1023) // 1024


# (Tx, Ty): 1 block; 64 (16 x 4); 8, 5, 4, 3, 2 copies; 1023, 1024, 1025 blocks around the switch; rows of 65 and of 1;
# 2, 3, 4 and 5 blocks a thread (65 x 65 = 4225 is in the edge cases)
LAYOUTS = [(3, 2), (62, 13), (61, 30), (50, 49), (63, 60), (64, 67), (78, 77), (130, 121), (127, 126), (162, 97),
           (2, 256), (256, 1), (200, 40), (170, 100), (256, 157), (250, 256)]


def layout_name(t):
    return f"tx{t[0]}_ty{t[1]}"


def layout_case(t):
    """match_cases.edge_case (points on and around every border of a small grid, the field with all seven bytes) at
    the window t = (Tx, Ty), K 0 or 1 and the grid 64 or 61 cells wide by the layout's place in the list; the cap is
    the whole volume."""
    at = LAYOUTS.index(t)
    case = widened(mc.edge_case((64, 61)[at % 2], mc.EDGE_H, t[0], t[1], at % 2, 0.01, n_random=60))
    case["nb"], case["per"], case["slices"], case["owned"] = layout_of(*t)
    return case


def layouts_cover_the_kernel():
    """Both paths, every number of copies the narrow path can make, every number of blocks a thread can own, the
    sizes named in the issue, Tx != Ty on both paths."""
    lay = {t: layout_of(*t) for t in LAYOUTS}
    lay[(256, 256)] = layout_of(256, 256)  # (the 4096 x 4096 edge case)
    possible = {1024 // per for per in range(64, 1025, 64)}
    assert {v[2] for v in lay.values() if v[0] <= 1024} == possible == {16, 8, 5, 4, 3, 2, 1}
    assert {v[3] for v in lay.values() if v[0] > 1024} == {2, 3, 4, 5}
    assert {1, 64, 1023, 1024, 1025, 4225} <= {v[0] for v in lay.values()}
    assert any(t[0] != t[1] and v[0] <= 1024 for t, v in lay.items())
    assert any(t[0] != t[1] and v[0] > 1024 for t, v in lay.items())
    shapes = {(wo.blocks_shape(dict(wo.DEFAULT, shift_x=t[0], shift_y=t[1], rot_steps=0))[1:]) for t in LAYOUTS}
    assert (65, 1) in shapes and (1, 65) in shapes  # (nby, nbx): windows of 1 x 65 and 65 x 1 blocks
    return lay


def layout_regime(oracle, t, case):
    s = case["spec"]
    assert (s["shift_x"], s["shift_y"]) == t and wo.spec_valid(s)
    assert wo.blocks_size(s) == (2 * s["rot_steps"] + 1) * case["nb"] == s["max_blocks"]
    w = case_want(oracle, case, f"layout_{layout_name(t)}")[0]
    assert w["best"][0] > 0 and w["best"][7] == 0 and w["status"] == 0
    return w


# ---- 6: edges ---------------------------------------------------------------------------------------------------------------
def _far_points(W, H, res, Tx, Ty):
    """Cell centres on every border of the grid and outside it: 1 cell, T + 7 cells (the last the bound reads P for on
    the low side), T + 8 (dropped), and on the high side T - 1 (the last) and T (dropped)."""
    xs = [0, 1, W // 2, W - 1, -1, -Tx, -Tx - (S - 1), -Tx - S, W, W + Tx - 1, W + Tx]
    ys = [0, 1, H // 2, H - 1, -1, -Ty, -Ty - (S - 1), -Ty - S, H, H + Ty - 1, H + Ty]
    return (np.array([(x, y) for x in xs for y in ys], float) + 0.5) * res


def edge_case(W, H, Tx, Ty, K=0, rot_step=0.0, field=None, n_random=40, res=0.05):
    rng = np.random.default_rng(2410 + W + 7 * H + Tx)
    sensor = ((W / 2 + 0.37) * res, (H / 2 + 0.21) * res)
    rnd = rng.uniform([-3 * res, -3 * res], [(W + 3) * res, (H + 3) * res], (n_random, 2))
    scan = mc.nodes_to(np.concatenate([_far_points(W, H, res, Tx, Ty), rnd]), sensor)
    batch, lens = pad([scan], len(scan))
    s = wo.spec(origin_x=0.0, origin_y=0.0, resolution=res, width=W, height=H, shift_x=Tx, shift_y=Ty, rot_steps=K,
                rot_step=rot_step, max_blocks=1)
    s["max_blocks"] = wo.blocks_size(s)
    return dict(batch=batch, lens=lens, group=1, p=Params.defaults(clip_enable=0), spec=s,
                fields=mc.pattern_field(H, W, W) if field is None else field,
                pose2d=np.array([[1, 0, sensor[0], 0, 1, sensor[1]]], F32), pivot=np.array([sensor], F32))


def edge_cases():
    """name -> case: widths 61 .. 64 with T 20 (rows of P starting at every byte of a word), and T 256, K 0 on
    4096 x 4096, 4096 x 1 and 1 x 4096 fields (65 x 65 blocks, the 13-bit cells and the indices at their largest)."""
    out = {f"w{W}": edge_case(W, mc.EDGE_H, 20, 20, 1, 0.01, n_random=100) for W in mc.EDGE_WIDTHS}
    for name, (W, H) in mpc.BIG.items():
        out[name] = edge_case(W, H, 256, 256, field=mpc.big_field(H, W, W), res=0.01)
    return out


def edge_regime(oracle, name, case):
    """At no rotation the kept cells reach exactly from -T - 7 to W + T - 1 and points beyond are dropped, so P is read
    at its first column and row and beyond its last; the result is proven and not 0."""
    s = case["spec"]
    W, H, Tx, Ty, K = s["width"], s["height"], s["shift_x"], s["shift_y"], s["rot_steps"]
    x, y = mc.case_points(oracle, case, 0)
    pv = case["pivot"][0]
    has, cx, cy = mo.rotated_cells(x, y, pv[0], pv[1], 1.0, 0.0, s)
    assert has.all()
    near = (cx >= -Tx - (S - 1)) & (cx < W + Tx) & (cy >= -Ty - (S - 1)) & (cy < H + Ty)
    assert (~near).any() and cx[near].min() == -Tx - (S - 1) and cy[near].min() == -Ty - (S - 1)
    assert cx[near].max() == W + Tx - 1 and cy[near].max() == H + Ty - 1
    assert (cx == -Tx - S).any() and (cx == W + Tx).any() and (cy == -Ty - S).any() and (cy == H + Ty).any()
    w = case_want(oracle, case, f"edge_{name}")[0]
    assert w["best"][0] > 0 and w["best"][7] == 0 and w["status"] == 0 and w["work"][0] == wo.blocks_size(s)
    if Tx == 256:
        # (the kernel's cell word: 13 bits an axis, biased by 320)
        assert w["work"][0] == 4225 and K == 0 and max(cx[near].max(), cy[near].max()) + 320 == 4096 + 255 + 320 < 8192
    return w


# ---- 7: passes and weights ------------------------------------------------------------------------------------------------
def passes_case():
    """match_path_cases' scans at n_stride = 18432 (nine passes of 2048 for eight workgroups: the first walks a
    second one) — walls, 18432 samples in one cell of value 100 (runs of 64 across every boundary), a noisy ring —
    with a window of 4 x 3 blocks a rotation."""
    return widened(mpc.long_case(18432), shift_x=13, shift_y=10)


def passes_regime(oracle, case):
    """Bounds and scores owe something to the samples from 16384 on, scan by scan."""
    want = case_want(oracle, case, "passes")
    head = case_want(oracle, mpc.truncated(case, mpc.TWO_PASS))
    n = case["batch"].shape[1]
    assert n > mpc.TWO_PASS
    for g, (w, h) in enumerate(zip(want, head)):
        assert int(case["lens"][g]) > mpc.TWO_PASS and w["best"][7] == 0
        assert (w["U"] != h["U"]).any() and w["best"][4] > h["best"][4] and w["best"][0] >= h["best"][0] > 0, g
    w = want[case["n_wall"]]  # the one-cell scan
    assert w["best"][4] == n and w["best"][5] == 100 * n and w["work"][1] >= 100 * n
    return want


# ---- 8: groups ----------------------------------------------------------------------------------------------------------------
def groups_case(per_group):
    """match_path_cases' 344 groups (five empty, one CELL_RANGE, one truncated) with a window of 2 x 2 blocks a
    rotation and a cap of 5 blocks of the 12: most groups list 6 and are unproven, some 3 to 5 and are proven."""
    return widened(mpc.many_case(per_group), max_blocks=5, shift_x=5, shift_y=4)


def groups_regime(oracle, case, key):
    want = case_want(oracle, case, key)
    assert len(want) == 344 and want[0]["work"][0] == 12
    proven = sum(1 for w in want if w["best"][7] == 0)
    assert 8 <= proven <= len(want) - 8, proven
    for g, w in enumerate(want):
        planted = {mpc.MANY_CELL_RANGE: abi.SCAN_CELL_RANGE, mpc.MANY_TRUNCATED: abi.SCAN_OUT_TRUNCATED}.get(g, 0)
        assert w["status"] == planted, (g, w["status"])
        if g in mpc.MANY_EMPTY:  # every block listed, above the cap: block 0 and seed B, 64 candidates each
            assert not w["U"].any() and w["best"].tolist() == [0, 0, 0, 0, 0, 0, 128, wo.UNPROVEN], (g, w["best"])
            assert w["work"].tolist() == [12, 0, 0, 0, 12, 5, 0, 0]
    return want
