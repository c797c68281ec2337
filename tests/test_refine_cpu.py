"""E25 without a device: the spec check and the scratch size, the two writers of the sums against each other, the
library's plain C++ twins (rplgpu_refine_sums_host, rplgpu_refine_step_host) against the oracle byte for byte, known
answers worked out by hand, the bound table's third limb, every branch of the step, the covariance, every regime
check of tests/refine_cases.py, and convergence on the L-shaped room."""
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import refine_cases as rc
from tests import refine_oracle as ro

F32 = np.float32


# ---- the spec, the scratch -----------------------------------------------------------------------------------------
def test_defaults_and_check():
    d = abi.PoseRefine.defaults()
    assert d.check() == abi.OK
    for k, v in ro.DEFAULT.items():
        assert getattr(d, k) == pytest.approx(v), k
    nan, inf = float("nan"), float("inf")
    bad = [dict(target=0), dict(target=128), dict(damping=-1e-9), dict(damping=nan), dict(damping=inf),
           dict(max_step_cells=0.0), dict(max_step_cells=-1.0), dict(max_step_cells=inf), dict(max_rot=0.0),
           dict(max_rot=nan), dict(min_points=2), dict(min_points=0), dict(resolution=0.0), dict(resolution=nan),
           dict(origin_x=inf), dict(origin_y=nan), dict(width=0), dict(width=4097), dict(height=0), dict(height=4097)]
    good = [dict(target=1), dict(target=127), dict(damping=0.0), dict(damping=1e3), dict(min_points=3),
            dict(width=4096, height=1), dict(max_rot=10.0)]
    for kw in bad + good:
        s = ro.spec(**kw)
        assert (ro.struct_of(s).check() == abi.OK) == ro.spec_valid(s) == (kw in good), kw
    with pytest.raises(abi.RplGpuError):
        abi.pose_refine_check(ro.struct_of(ro.spec(target=0)))
    abi.pose_refine_check(d)


def test_scratch_words():
    for G, P in [(0, 1), (1, 0), (1, 1), (3, 5), (65535, 1 << 20), (1, (1 << 20) + 1), (7, 1025)]:
        assert abi.refine_scratch_words(G, P) == ro.scratch_words(G, P), (G, P)
    assert abi.refine_scratch_words(1, 1) == 2 * abi.REFINE_PLANES == 58 and abi.REFINE_WORDS == 32


# ---- the two writers, the host twin -------------------------------------------------------------------------------------
def _point_cases(oracle):
    yield "len129", rc.length_case(129)
    yield "groups", rc.groups_case(1, 1)
    yield "border", rc.border_case()
    yield "limit", rc.limit_case()
    yield "mirror", rc.limb_case(oracle, "mirror")
    yield "many", rc.limb_case(oracle, "many")
    yield "identity", rc.identity_case(oracle)


def test_writers_agree_and_host_twin(oracle):
    for name, case in _point_cases(oracle):
        for g in range(len(rc.case_groups(case))):
            x, y = rc.case_points(oracle, case, g)
            poses, s, field = rc.case_poses(case, g), case["spec"], rc.case_field(case, g)
            a = ro.sums_of(x, y, poses, s, field, ro.sums_python)
            b = ro.sums_of(x, y, poses, s, field, ro.sums_numpy)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], name
            sums, res, status = abi.refine_sums_host(x, y, poses, field, ro.struct_of(s))
            assert sums.tobytes() == b[0].tobytes(), name
            assert res.tobytes() == b[1].tobytes() and status == b[2], name


def test_words_round_trip():
    d = dict(sxx=2 ** 64 - 1, sxy=-2 ** 63, syy=0, sxe=-1, sye=2 ** 63 - 1, sv=5, sxt=-2 ** 95, syt=2 ** 95 - 1,
             stt=2 ** 96 - 1, ste=-2 ** 64 - 1, see=2 ** 64, n=7, dropped=2 ** 32 - 1)
    w = ro.to_words(d)
    assert ro.from_words(w) == d and not w[29:].any()
    assert list(w[21:24]) == [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE] and list(w[24:27]) == [0, 0, 1]


def test_host_twins_refuse():
    s = ro.struct_of(rc.SPEC)
    f = np.zeros((64, 64), np.int8)
    one = np.zeros(1, F32)
    with pytest.raises(abi.RplGpuError):
        abi.refine_sums_host(one, one, np.zeros((1, 4), F32), f, ro.struct_of(ro.spec(target=0, **rc.GRID)))
    with pytest.raises(abi.RplGpuError):
        abi.refine_sums_host(one, one, np.zeros((0, 4), F32), f, s)
    with pytest.raises(abi.RplGpuError):
        abi.refine_step_host(np.zeros(32, np.uint32), ro.struct_of(ro.spec(min_points=1, **rc.GRID)), np.zeros(4, F32))


# ---- known answers -------------------------------------------------------------------------------------------------------------
KNOWN = ro.spec(origin_x=0.0, origin_y=0.0, resolution=1.0, width=5, height=5, target=100, min_points=3)
KNOWN_FIELD = np.array([[10, 20, 30, 40, 50],
                        [11, 21, 31, 41, 51],
                        [12, -5, 32, 42, 52],
                        [13, 23, 33, 43, 53],
                        [14, 24, 34, 44, 54]], np.int8)


def _one(x, y, pose=(1, 0, 0, 0), s=KNOWN, field=KNOWN_FIELD):
    a = ro.sums_python([x], [y], pose, s, field)
    assert ro.to_words(a).tobytes() == ro.to_words(ro.sums_numpy([x], [y], pose, s, field)).tobytes()
    sums, _, _ = abi.refine_sums_host([x], [y], [pose], field, ro.struct_of(s))
    assert sums[0].tobytes() == ro.to_words(a).tobytes()
    return a


def test_known_cell_centre():
    """(2.5, 1.5) is the centre of cell (2, 1): a = b = 0, V = 65536 * 31, Gx = 256 * (41 - 31), Gy = 256 * (32 - 31);
    the lever is (2.5, 1.5) cells: Lx = 40, Ly = 24."""
    a = _one(2.5, 1.5)
    gx, gy, e = 2560, 256, (100 - 31) * 65536
    gt = gy * 40 - gx * 24
    assert a == dict(sxx=gx * gx, sxy=gx * gy, syy=gy * gy, sxe=gx * e, sye=gy * e, sv=31 * 65536, sxt=gx * gt,
                     syt=gy * gt, stt=gt * gt, ste=gt * e, see=e * e, n=1, dropped=0)


def test_known_u_minus_one():
    """x = 0.5 - 1/256: hu = -1, so i0 = -1 and a = 255: the left two bytes are outside the grid (0).  y = 1.5: b = 0.
    V = 255 * 256 * m(0, 1) = 255 * 256 * 11; Gx = 256 * (11 - 0); Gy = 255 * (12 - 11)."""
    a = _one(0.5 - 1.0 / 256.0, 1.5)
    assert a["sv"] == 255 * 256 * 11 and a["sxx"] == (256 * 11) ** 2 and a["syy"] == 255 ** 2 and a["n"] == 1


def test_known_negative_byte_is_zero():
    """(1.5, 2.5) is the centre of cell (1, 2), whose byte is -5: read as 0.  V = 0, Gx = 256 * (32 - 0), Gy = 256 *
    (23 - 0), E = the whole target."""
    a = _one(1.5, 2.5)
    assert a["sv"] == 0 and a["sxx"] == (256 * 32) ** 2 and a["syy"] == (256 * 23) ** 2 and a["see"] == (100 * 65536) ** 2


def test_known_rint_ties_to_even():
    """Levers of 2.53125 and 1.46875 cells: lx * 16 = 40.5 -> 40 and ly * 16 = 23.5 -> 24 (ties to even, not away)."""
    x, y = 2.53125, 1.46875
    _, t = ro.terms(np.array([x], F32), np.array([y], F32), (1, 0, 0, 0), KNOWN, KNOWN_FIELD)
    assert int(t["Lx"][0]) == 40 and int(t["Ly"][0]) == 24 and int(t["a"][0]) == 8 and int(t["b"][0]) == 248
    a = _one(x, y)
    assert a["n"] == 1 and a["stt"] == int(t["Gt"][0]) ** 2


def test_bound_table_third_limb(oracle):
    """One point at a lever of (8191.9, -8191.9) cells beside the one cell of 127: S Gt^2 passes 2^64 and the third
    limb is live at the smallest shape; the mirror image makes S Gx Gt negative, its third limb all ones."""
    for kind in ("single", "mirror"):
        case = rc.limb_case(oracle, kind)
        want = rc.limb_regime(oracle, kind, case)
        x, y = rc.case_points(oracle, case, 0)
        sums, _, _ = abi.refine_sums_host(x, y, rc.case_poses(case, 0), rc.case_field(case, 0), ro.struct_of(case["spec"]))
        assert sums.tobytes() == want[0][1].tobytes()
        d = ro.from_words(sums[0])
        assert d["stt"] > 2 ** 64 and abs(d["stt"]) < 2 ** 66 and abs(d["sxt"]) < 2 ** 48 and abs(d["ste"]) < 2 ** 56


@pytest.mark.parametrize("name", ["lengths", "layouts", "groups", "limbs", "border", "limit", "identity", "front"])
def test_regimes(oracle, name):
    if name == "lengths":
        for n in rc.LENGTHS:
            rc.length_regime(oracle, rc.length_case(n))
    elif name == "layouts":
        for P in rc.LAYOUT_P:
            rc.layout_regime(oracle, rc.layout_case(P))
    elif name == "groups":
        for a in (0, 1):
            for b in (0, 1):
                rc.groups_regime(oracle, rc.groups_case(a, b), f"groups{a}{b}")
    elif name == "limbs":
        for kind in ("many", "deep"):
            rc.limb_regime(oracle, kind, rc.limb_case(oracle, kind))
    elif name == "border":
        rc.border_regime(oracle, rc.border_case())
    elif name == "limit":
        rc.limit_regime(oracle, rc.limit_case())
    elif name == "identity":
        rc.identity_regime(oracle, rc.identity_case(oracle))
    else:
        rc.front_regime(oracle, rc.front_case())


# ---- the step -----------------------------------------------------------------------------------------------------------------
STEP_SPEC = ro.spec(min_points=3, max_step_cells=0.5, max_rot=0.01, **rc.GRID)


def _both(words, s, pose):
    a, b = ro.step_numpy(words, s, pose), ro.step_host(words, s, pose)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (a, b)
    return a


def _sums(**kw):
    d = {k: 0 for k in ro.LAYOUT}
    d.update(kw)
    return ro.to_words(d)


def _diag(g1=0, g2=0, g3=0, n=10):
    """A = diag(1, 1, 1) in the step's units (a11 = sxx 2^-16, a33 = stt 2^-24) and the right-hand side g in 2^-8."""
    return _sums(sxx=1 << 16, syy=1 << 16, stt=1 << 24, sxe=g1 << 16, sye=g2 << 16, ste=g3 << 20, n=n)


def test_step_too_few_points():
    pose = np.array([0.6, 0.8, 1.25, -2.5], F32)
    out, step = _both(_diag(1, 1, 1, n=2), STEP_SPEC, pose)
    assert out.tobytes() == pose.tobytes() and list(step) == [0, 0, 0, ro.FEW]


def test_step_singular_wall():
    """All points on one straight wall along x: the field varies only in y, so Gx = 0 everywhere, a11 = a12 = a13 = 0
    and det = 0: no step, the pose comes back bit for bit."""
    f = np.zeros((64, 64), np.int8)
    f[30, :] = 127
    f[29, :] = f[31, :] = 60
    x = np.linspace(-1.0, 1.0, 50).astype(F32)
    y = np.full(50, -1.6 + 30.7 * 0.05, F32)
    sums, _, _ = ro.sums_of(x, y, [(1, 0, 0, 0)], STEP_SPEC, f)
    d = ro.from_words(sums[0])
    assert d["n"] == 50 and d["sxx"] == 0 and d["syy"] > 0 and d["stt"] > 0
    pose = np.array([1, 0, 0, 0], F32)
    out, step = _both(sums[0], STEP_SPEC, pose)
    assert out.tobytes() == pose.tobytes() and list(step) == [0, 0, 0, ro.SINGULAR]
    assert abi.refine_covariance(sums[0], ro.struct_of(STEP_SPEC)) is None
    # a negative determinant (no sums of squares give one; the rule still names it) is singular too, and the largest
    # words with the largest damping still have a finite determinant: about 1e166
    out, step = _both(_sums(sxx=1 << 16, syy=1 << 16, sxy=2 << 16, stt=1 << 24, n=10), STEP_SPEC, pose)
    assert out.tobytes() == pose.tobytes() and step[3] == ro.SINGULAR
    big = _sums(sxx=2 ** 64 - 1, syy=2 ** 64 - 1, stt=2 ** 96 - 1, sxe=2 ** 62, n=10)
    out, step = _both(big, ro.spec(min_points=3, damping=3.0e38, **rc.GRID), pose)
    assert step[3] & ro.STEPPED


@pytest.mark.parametrize("which,flag", [(0, ro.CLAMP_X), (1, ro.CLAMP_Y), (2, ro.CLAMP_T)])
@pytest.mark.parametrize("sign", [1, -1])
def test_step_clamps(which, flag, sign):
    g = [0, 0, 0]
    g[which] = sign * 256 * 3  # delta = 3 cells or rad: beyond both clamps
    pose = np.array([1, 0, 0.5, -0.25], F32)
    out, step = _both(_diag(*g), STEP_SPEC, pose)
    assert step[3] == ro.STEPPED | flag
    want = [F32(0), F32(0), F32(0)]
    want[which] = F32(sign * np.float64(F32(0.5)) * np.float64(F32(0.05))) if which < 2 else F32(sign * F32(0.01))
    assert [float(v) for v in step[:3].view(F32)] == [float(v) for v in want]
    # inside the clamps nothing is flagged
    g[which] = sign * 64  # a quarter of a cell / a quarter of a radian: only the rotation clamps
    out, step = _both(_diag(*g), STEP_SPEC, pose)
    assert step[3] == ro.STEPPED | (ro.CLAMP_T if which == 2 else 0)


def test_step_zero_rotation_is_exact():
    pose = np.array([0.6, 0.8, 1.0, 2.0], F32)
    out, step = _both(_diag(64, -64, 0), STEP_SPEC, pose)
    assert step[3] == ro.STEPPED and step[2] == 0
    assert out[:2].tobytes() == pose[:2].tobytes()  # (dc, ds) = (1, 0): c * 1 - s * 0
    assert out.view(F32)[2] == F32(F32(1.0) + F32(0.25 * np.float64(F32(0.05))))


def test_step_nan_is_canonical():
    nan_bits = np.array([0x7FA00001, 0xFFC12345], np.uint32).view(F32)
    pose = np.array([nan_bits[0], 0.5, nan_bits[1], float("inf")], F32)
    out, step = _both(_diag(64, 64, 64), ro.spec(min_points=3, **rc.GRID), pose)
    assert step[3] & ro.STEPPED
    assert out[0] == out[1] == out[2] == ro.QNAN and out[3] == np.array([np.inf], F32).view(np.uint32)[0]
    # not stepped: the same pose comes back bit for bit, payloads included
    out, step = _both(_diag(64, 64, 64, n=1), STEP_SPEC, pose)
    assert out.tobytes() == pose.tobytes()


def test_step_damping():
    a, _ = _both(_diag(64, 0, 0), STEP_SPEC, np.array([1, 0, 0, 0], F32))
    s = dict(STEP_SPEC, damping=1.0)
    b, step = _both(_diag(64, 0, 0), s, np.array([1, 0, 0, 0], F32))
    assert a.view(F32)[2] == F32(0.25 * np.float64(F32(0.05))) and b.view(F32)[2] == F32(0.125 * np.float64(F32(0.05)))


def test_covariance():
    s = ro.struct_of(STEP_SPEC)
    cov = abi.refine_covariance(_sums(sxx=4 << 16, syy=16 << 16, stt=64 << 24, n=10), s)
    res = float(F32(0.05))
    assert np.allclose(cov, np.diag([res * res / 4, res * res / 16, 1 / 64]), rtol=1e-15, atol=0)
    rng = np.random.default_rng(2590)
    x, y = rng.uniform(-1, 1, 400).astype(F32), rng.uniform(-1, 1, 400).astype(F32)
    sums, _, _ = ro.sums_of(x, y, [(1, 0, 0, 0)], STEP_SPEC, rc.box_field()[0])
    d = ro.from_words(sums[0])
    A = np.array([[d["sxx"] / 2 ** 16, d["sxy"] / 2 ** 16, d["sxt"] / 2 ** 20],
                  [d["sxy"] / 2 ** 16, d["syy"] / 2 ** 16, d["syt"] / 2 ** 20],
                  [d["sxt"] / 2 ** 20, d["syt"] / 2 ** 20, d["stt"] / 2 ** 24]])
    S = np.diag([res, res, 1.0])
    cov = abi.refine_covariance(sums[0], s)
    assert np.allclose(cov, S @ np.linalg.inv(A) @ S, rtol=1e-9) and np.allclose(cov, cov.T, rtol=0, atol=0)


# ---- convergence ----------------------------------------------------------------------------------------------------------------
def test_convergence_on_the_l_shaped_room():
    """The ORACLE's rounds on the L-shaped room (200 x 200 cells of 0.05 m, walls through cell centres, field
    rint(127 exp(-D2 / 18)), 720 returns with 5 mm of range noise), as measured; the error is (metres, radians) to the
    true pose:
      from 25 mm / 2.2 mrad off (half a cell, half of E13's default rotation step): 1 step 0.3 mm / 0.09 mrad,
        2 and 3 steps 0.3 mm / 0.07 mrad;
      from 100 mm / 30 mrad off (two cells): 1 step 40.9 mm / 13.6 mrad, 2 steps 15.9 mm / 6.2 mrad, 3 steps 0.3 mm /
        0.11 mrad, 4 steps 0.3 mm / 0.07 mrad.
    These are records of the oracle, not thresholds for a device.  Demanded here: the library's twins reproduce the
    oracle's rounds byte for byte, and S V does not fall over the three steps of either start (four sums).  Beyond
    them the pose sits on the noise floor, where a step that lowers S E^2 moves S V by parts in 10^6 either way (the
    sixth sum of the far start measured 5971324490 after 5971329040), so no more steps are held to that.  That the
    oracle ends within the 5 mm of noise and a milliradian of the truth is asserted of the oracle alone."""
    x, y, true = rc.room_points()
    field, s = rc.room_field(), rc.ROOM_SPEC
    for off_m, off_rad, rounds in ((0.025 / math.sqrt(2), 0.0022, 3), (0.1 / math.sqrt(2), 0.03, 3)):
        pose = rc.room_start(true, off_m, off_rad)
        e0 = rc.pose_error(pose, true)
        sv, errs = [], [e0]
        twin = pose.copy()
        for _ in range(rounds + 1):
            out, sums, step, res, status = ro.refine_points(x, y, pose[None], s, field, 1)
            hs, hres, hst = abi.refine_sums_host(x, y, twin[None], field, ro.struct_of(s))
            hout, hstep = abi.refine_step_host(hs[0], ro.struct_of(s), twin)
            assert hs.tobytes() == sums.tobytes() and hout.tobytes() == out[0].tobytes(), len(sv)
            assert hstep.tobytes() == step[0].tobytes() and status == hst == 0
            assert step[0][3] & ro.STEPPED
            sv.append(ro.from_words(sums[0])["sv"])
            pose, twin = out[0], hout
            errs.append(rc.pose_error(pose, true))
        print(f"start {e0[0] * 1e3:.1f} mm / {e0[1] * 1e3:.2f} mrad:",
              ", ".join(f"{a * 1e3:.1f} mm / {b * 1e3:.2f} mrad" for a, b in errs[1:]), "S V", sv)
        assert all(b >= a for a, b in zip(sv, sv[1:])), sv
        assert errs[rounds][0] < 0.005 and errs[rounds][1] < 0.001
