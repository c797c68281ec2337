"""E10 without a device: the host functions of include/rplgpu_msg.h (rplgpu_default_scan_filter,
rplgpu_scan_filter_check) and the numpy oracle the GPU tests compare against — its hand-built known
answers, the decision flips, and the regime conditions of the inputs tests/test_gpu_filter.py uses.

Bench-shaped batch: synth.make_batch(2026, 64, 32000, r0_range=(1, 12), noise_m=0.002), Mode A LaserScans
(the oracle's publish_scan, which the parity tests hold the device to bit for bit), filter defaults."""
import ctypes as C
import math

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi
from tests import filter_cases as fc
from tests import filter_oracle as fo
from tests import oracle_lib

F32 = np.float32


def _struct(f):
    return abi.ScanFilter(**{k: f[k] for k, _ in abi.ScanFilter._fields_})


def test_defaults_match_the_header_and_the_oracle():
    f = abi.ScanFilter.defaults()
    assert C.sizeof(abi.ScanFilter) == 36
    assert bytes(f) == bytes(_struct(fo.flt()))
    assert (f.shadow_enable, f.shadow_window, f.shadow_neighbors) == (1, 2, 1)
    assert (f.speckle_enable, f.speckle_min_run, f.circular) == (1, 4, 1)
    assert f.shadow_min_angle == F32(math.radians(10.0)) and f.shadow_max_angle == F32(math.radians(170.0))
    assert f.speckle_max_range_difference == F32(0.05)
    assert abi.MAX_FILTER_WINDOW == fo.MAX_WINDOW == 64


def test_check_accepts_defaults_and_dirs_equal_the_oracle():
    for kw in (dict(), dict(shadow_min_angle=0.3, shadow_max_angle=2.9), dict(shadow_min_angle=1e-3),
               dict(shadow_min_angle=1.5707, shadow_max_angle=1.5709), dict(shadow_max_angle=3.1415),
               dict(shadow_window=64, shadow_neighbors=64, speckle_min_run=64), dict(shadow_neighbors=0),
               dict(speckle_max_range_difference=0.0), dict(shadow_enable=0, speckle_enable=0, circular=0)):
        f = fo.flt(**kw)
        got = abi.scan_filter_check(_struct(f))
        assert got.tobytes() == np.array(fo.dirs(f), F32).tobytes(), kw
    lib = abi.load_library()
    assert lib.rplgpu_scan_filter_check(C.byref(abi.ScanFilter.defaults()), None) == abi.OK  # dirs may be NULL


@pytest.mark.parametrize("kw", [
    dict(shadow_min_angle=0.0), dict(shadow_min_angle=-0.1), dict(shadow_min_angle=math.pi / 2),
    dict(shadow_min_angle=1.6), dict(shadow_min_angle=math.nan), dict(shadow_min_angle=math.inf),
    dict(shadow_max_angle=float(np.nextafter(F32(math.pi / 2), F32(0)))), dict(shadow_max_angle=1.5),
    dict(shadow_max_angle=float(F32(math.pi))),
    dict(shadow_max_angle=3.2), dict(shadow_max_angle=math.nan), dict(shadow_max_angle=-math.inf),
    dict(shadow_window=0), dict(shadow_window=65), dict(shadow_neighbors=65), dict(speckle_min_run=0),
    dict(speckle_min_run=65), dict(speckle_max_range_difference=-1e-6),
    dict(speckle_max_range_difference=math.nan), dict(speckle_max_range_difference=math.inf),
], ids=lambda kw: "{}={}".format(*next(iter(kw.items()))))
def test_check_refuses_each_bound(kw):
    f = abi.ScanFilter.defaults(**kw)
    with pytest.raises(abi.RplGpuError) as e:
        abi.scan_filter_check(f)
    assert e.value.code == abi.ERR_INVALID_ARG
    assert abi.load_library().rplgpu_scan_filter_check(None, None) == abi.ERR_INVALID_ARG


def _removed_sets(r, inc, f):
    only_shadow = dict(f, speckle_enable=0)
    mid, n_sh0, _ = fo.filter_scan(r, inc, only_shadow)
    out, n_sh, n_sp = fo.filter_scan(r, inc, f)
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)  # noqa: E731
    sh = np.flatnonzero(bits(mid) != bits(r))
    sp = np.flatnonzero(bits(out) != bits(mid))
    assert n_sh == n_sh0 == len(sh) and n_sp == len(sp)
    assert np.all(bits(out)[np.concatenate([sh, sp]).astype(int)] == fo.QNAN)
    return sh.tolist(), sp.tolist(), out


@pytest.mark.parametrize("name", list(fc.known_answers()))
def test_known_answers(name):
    r, inc, kw, want_shadow, want_speckle = fc.known_answers()[name]
    sh, sp, out = _removed_sets(r, inc, fo.flt(**kw))
    assert sh == want_shadow and sp == want_speckle
    keep = np.setdiff1d(np.arange(len(r)), sh + sp)
    assert out.view(np.uint32)[keep].tobytes() == r.view(np.uint32)[keep].tobytes()  # NaN and inf bits stay


def test_both_filters_off_is_a_copy_and_empty_scan():
    r = fc.step_edge()
    out, a, b = fo.filter_scan(r, fc.INC360, fo.flt(shadow_enable=0, speckle_enable=0))
    assert out.tobytes() == r.tobytes() and (a, b) == (0, 0)
    out, a, b = fo.filter_scan(np.zeros(0, F32), fc.INC360, fo.flt())
    assert len(out) == 0 and (a, b) == (0, 0)


def test_a_far_point_never_removes_a_nearer_one():
    rng = np.random.default_rng(5)
    for circular in (0, 1):
        r = rng.uniform(1.0, 3.0, 500).astype(F32)
        f = fo.flt(speckle_enable=0, shadow_window=3, shadow_neighbors=2, circular=circular)
        rem, det = fo.shadow(r, fo.inc_mode_a(500), f)
        assert rem.any() and not rem.all()
        for k in np.flatnonzero(rem):
            near = [(k + d) % 500 if circular else k + d for d in range(-2, 3)]
            near = [i for i in near if 0 <= i < 500]
            assert any(det[i] and r[i] < r[k] for i in near)
        assert not rem[np.argmin(r)]


def test_pairs_beyond_half_a_radian_are_not_examined():
    # 12 beams: inc = 0.524 rad > 0.5, so no pair is examined and the shadow filter finds nothing
    r = np.array([2, 9, 2, 9, 2, 9, 2, 9, 2, 9, 2, 9], F32)
    assert not fo.shadow(r, fo.inc_mode_a(12), fo.flt())[1].any()
    assert fo.shadow(r, fo.inc_mode_a(13), fo.flt())[1].any()


@pytest.mark.parametrize("which,r1,y", fc.flip_cases())
def test_decision_flips_are_adjacent_floats_and_visible(which, r1, y):
    f = fo.flt(**fc.FLIP_FILTER)
    lo, hi = fo.bisect_flip(r1, y, fc.INC360, f, which)
    assert int(hi.view(np.uint32)) - int(lo.view(np.uint32)) == 1
    a = fo.filter_scan(fc.flip_scan(r1, y, lo), fc.INC360, f)
    b = fo.filter_scan(fc.flip_scan(r1, y, hi), fc.INC360, f)
    assert a[1] != b[1] and a[0].tobytes() != b[0].tobytes()  # one ulp of r2 changes what is removed


@pytest.mark.parametrize("which,r1,y", fc.FUSED_FLIPS)
def test_fused_flips_would_decide_otherwise_with_an_fma_in_b(which, r1, y):
    """At these boundaries a device that fused r1 - r2 * c into one FMA decides the pair differently from
    the rule on at least one side: tests/test_gpu_filter.py::test_decision_flips runs the device on both."""
    f = fo.flt(**fc.FLIP_FILTER)
    s, c = fo.e6_sincos(F32(F32(y) * fc.INC360))
    d = fo.dirs(f)
    differs = 0
    for r2 in fo.bisect_flip(r1, y, fc.INC360, f, which):
        rule = bool(fo.pair_tests(F32(r1), r2, s, c, d)[0 if which == "min" else 1])
        differs += rule != fc.fused_b_decision(which, r1, r2, s, c, d)
    assert differs >= 1


def test_modes_increment():
    assert fo.inc_mode_a(360) == F32(2 * math.pi / 360) and fo.inc_mode_b(360) == F32(2 * math.pi / 359)
    assert fo.inc_mode_b(1) == fo.inc_mode_b(2) == F32(2 * math.pi)


def test_regime_of_the_bench_shaped_batch(oracle):
    """The shares of removed finite beams the GPU test's batch gives on the oracle: a filter test that
    removes nothing shows nothing."""
    nodes = fc.bench_nodes()
    p = Params.defaults(range_max=40.0)
    f = fo.flt()
    fin = sh = sp = 0
    per_scan = []
    for b in range(len(nodes)):
        r, _, m = oracle.publish_scan(nodes[b], oracle_lib.copy_params(p), 0.1)
        assert m.angle_increment == fo.inc_mode_a(len(r))
        _, n_sh, n_sp = fo.filter_scan(r, fo.inc_mode_a(len(r)), f)
        n_fin = int(np.isfinite(r).sum())
        fin, sh, sp = fin + n_fin, sh + n_sh, sp + n_sp
        per_scan.append(n_sh / n_fin)
    print(f"shadow {sh / fin:.4f} of finite beams, speckle {sp / fin:.4f}; per scan shadow "
          f"{min(per_scan):.4f} .. {max(per_scan):.4f}")
    assert 0.05 <= sh / fin <= 0.70
    assert min(per_scan) < 0.005 and max(per_scan) > 0.25
    assert sp / fin > 0.01


@pytest.mark.parametrize("n", [360, 3200, 32000])
def test_regime_of_the_sized_scans(oracle, n):
    """Both filters find work at every scan size the GPU test sweeps (Mode A and Mode B inputs)."""
    for sp in (1, 0):
        p = Params.defaults(range_max=40.0, scan_processing=sp)
        r, _, m = oracle.publish_scan(fc.sized_scan(70, n), oracle_lib.copy_params(p), 0.1)
        inc = fo.inc_mode_a(len(r)) if sp else fo.inc_mode_b(len(r))
        assert m.angle_increment == inc
        _, n_sh, n_sp = fo.filter_scan(r, inc, fo.flt())
        assert n_sh > 0 and n_sp > 0, (n, sp)
