"""Inputs the E10 tests share (tests/test_filter_cpu.py asserts their known answers and regime conditions
on the oracle alone; tests/test_gpu_filter.py runs the device on the very same arrays)."""
import math
from fractions import Fraction

import numpy as np

from rplidar_ros2_driver_amd import synth
from tests import filter_oracle as fo

F32 = np.float32
INF = F32(np.inf)
INC360 = fo.inc_mode_a(360)  # 0.01745 rad: one degree


def step_edge():
    """A near surface (2.0 m, beams 100..149), two mixed pixels hanging between the surfaces (2.4, 2.6 at 150,
    151) and the far surface (2.75 m, beams 152..199); the rest of the circle is empty.  Seen from 149 the
    line to 150 leaves at 176 deg (a shadow pair), 150 -> 151 at 167 deg and 151 -> 152 at 165 deg (none):
    149 and 150 are detected and, with N = 1, exactly 150 (behind 149) and 151 (behind 150) go."""
    r = np.full(360, INF, F32)
    r[100:150] = 2.0
    r[150], r[151] = 2.4, 2.6
    r[152:200] = 2.75
    return r


def far_outlier():
    """A flat 2.0 m surface with one return far behind it at beam 180 (5.0 m): 179, 180 and 181 are all
    detected, but only the farther point goes — 180 never removes 179 or 181."""
    r = np.full(360, F32(2.0), F32)
    r[180] = 5.0
    return r


def seam_scan():
    """The step of step_edge() laid across the seam: near surface on beams 300..359, the mixed pixel at beam
    0 (2.4 m), the far surface (2.55 m) from beam 1 on.  The only shadow pair is (359, 0): on a circle both are
    detected, and with N = 1 beam 0 goes behind 359 and beam 1 behind 0; on an open scan nothing is detected."""
    r = np.full(360, INF, F32)
    r[300:360] = 2.0
    r[0] = 2.4
    r[1:60] = 2.55
    return r


# name -> (ranges, inc, filter overrides, beams removed by shadow, beams removed by speckle)
def known_answers():
    sh = dict(speckle_enable=0, shadow_window=1, shadow_neighbors=1)
    sp = dict(shadow_enable=0, speckle_max_range_difference=0.05)
    broken = np.array([2, 2, 2, 2, 9, 2, 2, 2], F32)  # beam 4 stands alone; 5,6,7,0,1,2,3 is one run on a circle
    short = np.array([2.0, 2.5, 2.0], F32)
    return {
        "step_edge": (step_edge(), INC360, sh, [150, 151], []),
        "step_edge_n0": (step_edge(), INC360, dict(sh, shadow_neighbors=0), [], []),
        # W = 2 adds the pair (151, 149) at 6.6 deg: 151 is detected too, and N = 2 reaches 152 and 153 from it
        "step_edge_n2_w2": (step_edge(), INC360, dict(sh, shadow_neighbors=2, shadow_window=2),
                            [150, 151, 152, 153], []),
        "far_outlier": (far_outlier(), INC360, sh, [180], []),
        "seam_circular": (seam_scan(), INC360, dict(sh, circular=1), [0, 1], []),
        "seam_open": (seam_scan(), INC360, dict(sh, circular=0), [], []),
        # count 3 < 2W + 1 = 5: on a circle W and N shrink to (3 - 1) / 2 = 1, and beam 1 goes behind 0 and 2
        "short_circular": (short, INC360, dict(sh, shadow_window=2, shadow_neighbors=2, circular=1), [1], []),
        "short_open": (short, INC360, dict(sh, shadow_window=2, shadow_neighbors=2, circular=0), [1], []),
        "one_beam": (np.array([2.0], F32), INC360, dict(circular=1), [], [0]),
        "two_beams": (np.array([2.0, 2.01], F32), INC360, dict(circular=1, speckle_min_run=2), [], []),
        "all_inf": (np.full(360, INF, F32), INC360, dict(), [], []),
        "circle_closes_l8": (np.full(8, F32(2.0), F32), INC360, dict(sp, speckle_min_run=8, circular=1), [], []),
        "circle_closes_l9": (np.full(8, F32(2.0), F32), INC360, dict(sp, speckle_min_run=9, circular=1), [],
                             list(range(8))),
        "wrap_run_circular": (broken, INC360, dict(sp, speckle_min_run=7, circular=1), [], [4]),
        "wrap_run_open": (broken, INC360, dict(sp, speckle_min_run=4, circular=0), [], [4, 5, 6, 7]),
        "l1_removes_nothing": (broken, INC360, dict(sp, speckle_min_run=1), [], []),
        # both: the shadow filter takes 150 and 151 out of step_edge(), which leaves the surfaces as two runs
        # of 50 and 48 beams; L = 49 then takes the far surface as well
        "both_filters": (step_edge(), INC360, dict(shadow_window=1, shadow_neighbors=1, speckle_min_run=49),
                         [150, 151], list(range(152, 200))),
        "nan_and_inf_kept": (np.array([2, np.nan, 2, 2, 2, 2, -np.inf, 2, 2, 2, 2, 2], F32), INC360,
                             dict(sp, speckle_min_run=4, circular=0), [], [0]),
    }


# (which test, r1, y) whose boundary value of r2 decides differently when b = r1 - r2 * c is evaluated as ONE
# fused multiply-add instead of a rounded product and a rounded difference (found by search over random r1 with
# fused_b_decision below; tests/test_filter_cpu.py asserts the property): what holds the device to "no FMA in b"
FUSED_FLIPS = [("min", 11.455101013183594, 1), ("min", 4.430145740509033, 1), ("min", 10.664571762084961, 2),
               ("min", 9.205220222473145, 2), ("max", 3.206752061843872, 1), ("max", 7.2964372634887695, 1),
               ("max", 11.85155200958252, 2), ("max", 2.67205548286438, 2)]


def flip_cases():
    """(which test, r1, y): the pairs whose decision boundary the oracle bisects."""
    return [(w, r1, y) for w in ("min", "max") for r1 in (2.0, 7.3) for y in (1, 2)] + FUSED_FLIPS


def _round_f32(fr):
    """A Fraction rounded once to float32 (nearest, ties to even)."""
    x = F32(float(fr))
    cands = [np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(v.view(np.uint32)) & 1))


def fused_b_decision(which, r1, r2, s, c, d):
    """The side test `which` of the pair with b from a fused multiply-add: r1 - r2 * c exact, rounded once."""
    a = F32(F32(r2) * F32(s))
    b = _round_f32(Fraction(float(F32(r1))) - Fraction(float(F32(r2))) * Fraction(float(F32(c))))
    cmin, smin, cmax, smax = d
    if which == "min":
        return float(cmin) * float(a) - float(smin) * float(b) < 0.0
    return float(cmax) * float(a) - float(smax) * float(b) > 0.0


FLIP_FILTER = dict(speckle_enable=0, shadow_window=2, shadow_neighbors=1, circular=0)


def flip_scan(r1, y, r2):
    """Beam 100 at r1 and its neighbour at distance y at r2, alone on an empty scan but for a witness just
    behind beam 100 (1 % farther, at beam 99: no shadow pair of its own, 120 / 60 deg), which goes exactly
    when beam 100 is detected."""
    r = np.full(360, INF, F32)
    r[100] = r1
    r[100 + y] = r2
    r[99] = F32(r1) * F32(1.01)
    return r


# ---- the bench-shaped batch (config 3: 32 000 samples a scan, Mode A, the filter defaults) ----------------
BENCH_SEED, BENCH_B, BENCH_N = 2026, 64, 32000
BENCH_KW = dict(r0_range=(1.0, 12.0), noise_m=0.002)


def bench_nodes(B=BENCH_B):
    return synth.make_batch(BENCH_SEED, B, BENCH_N, **BENCH_KW)


def sized_scan(seed, n):
    """A ring scan of n samples whose range noise grows as the beams thin out (2 mm at 32 000 samples), so
    that both filters find work at every size."""
    return synth.make_scan(seed, n, n, r0_range=(1.0, 12.0), noise_m=0.002 * 32000.0 / n)


assert math.isclose(float(INC360), math.radians(1.0), rel_tol=1e-6)
