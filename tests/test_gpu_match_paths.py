"""E13 on the device, on the paths of k_match_score and k_match_best that tests/test_gpu_match.py does not reach:
rplgpu_match_scans_dev against tests/match_oracle.py byte for byte, by that file's _run and _check (score volumes, the
eight result words, status, the guard words behind every volume, the unchanged field).  The inputs and their regime
checks live in tests/match_path_cases.py; tests/test_match_paths_cpu.py runs the regimes without a device."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import RplGpu, abi
from tests import match_cases as mc
from tests import match_path_cases as mp
from tests.test_gpu_match import _check, _run

pytestmark = pytest.mark.gpu


# ---- A: two passes per workgroup ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", sorted(mp.LONG_LENS))
def test_second_pass(gpu, oracle, stride):
    case = mp.long_case(stride)
    want = mp.long_regime(oracle, case, mp.long_key(stride))
    _check(_run(gpu, case), want)


def test_second_pass_wide_window(gpu, oracle):
    case = mp.long_case(32768, wide=True)
    want = mp.long_regime(oracle, case, mp.long_key(32768, True))
    _check(_run(gpu, case), want)


def test_second_pass_full_front_end(gpu, oracle):
    case = mp.long_front_case()
    want = mp.long_front_regime(oracle, case)
    _check(_run(gpu, case), want)


def test_second_pass_ieee_divide_instance(gpu, oracle):
    """A handle whose fast divides are refused (as tests/test_gpu_ieee_div.py arranges): the same bytes."""
    import torch

    from tests.conftest import _shared_stream
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    case = mp.long_front_case()
    want = mc.case_want(oracle, case, "long_front")
    h = RplGpu(device=0, max_samples_per_scan=32768, max_batch=64)
    try:
        h.set_stream(_shared_stream().cuda_stream)
        assert lib.rplgpu_debug_force_ieee_div(h._h, 7) == abi.OK
        got = _run(h, case)
        torch.cuda.synchronize()
    finally:
        h.close()
    _check(got, want)


# ---- B: window layouts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", mp.LAYOUTS, ids=[mp.layout_name(t) for t in mp.LAYOUTS])
def test_window_layouts(gpu, oracle, t):
    case = mp.layout_case(t)
    mp.layout_regime(oracle, t, case)
    _check(_run(gpu, case), mc.case_want(oracle, case, f"layout_{mp.layout_name(t)}"))


# ---- C: runs --------------------------------------------------------------------------------------------------------------------
def test_run_sweep(gpu, oracle):
    case = mp.sweep_case()
    want = mp.sweep_regime(oracle, case)
    _check(_run(gpu, case), want)


def test_run_boundaries(gpu, oracle):
    case = mp.boundary_case()
    want = mp.boundary_regime(oracle, case, "run_boundary")
    _check(_run(gpu, case), want)
    k1 = mp.boundary_case(mp.RUN_SPEC_K1, (63, 64, 65, 130))
    _check(_run(gpu, k1), mp.boundary_regime(oracle, k1, "run_boundary_k1"))


def test_run_across_two_passes(gpu, oracle):
    case = mp.two_pass_run_case()
    want = mp.boundary_regime(oracle, case, "run_two_pass", (mp.TWO_PASS,))
    _check(_run(gpu, case), want)


def test_run_broken(gpu, oracle):
    case = mp.broken_case()
    want = mp.broken_regime(oracle, case)
    _check(_run(gpu, case), want)


# ---- D: the tie key and the count of equals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mp.KEY_NAMES)
def test_tie_key_limits(gpu, oracle, name):
    case, expect, equals = mp.key_cases()[name]
    best = mp.key_regime(oracle, name, case, expect, equals)
    got = _run(gpu, case)
    _check(got, mc.case_want(oracle, case, f"key_{name}"))
    assert got[1][0].view(np.int32)[:4].tolist() == best[:4].tolist() and got[1][0][6] == best[6]


# ---- E: grids at the limits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mp.BIG))
def test_grid_limits(gpu, oracle, name):
    case = mp.big_case(name)
    mp.big_regime(oracle, name, case)
    _check(_run(gpu, case), mp.big_want(oracle, name, case))


# ---- F: many groups ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_group", [0, 1])
def test_many_groups(gpu, oracle, per_group):
    case = mp.many_case(per_group)
    want = mp.many_regime(oracle, case, f"many{per_group}")
    _check(_run(gpu, case), want)
