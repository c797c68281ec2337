"""E24 without a device: the spec's check, defaults and sizes against tests/wide_oracle.py, the pooled field's host
twin byte for byte, the two writers of the oracle against each other on every case of tests/wide_cases.py, the bound
against the exhaustive volume, every case's regime, and the stand-alone program that drives the host twin under the
host sanitizers."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import wide_cases as wc
from tests import wide_oracle as wo

ROOT = Path(__file__).resolve().parents[1]


def _struct(s):
    return abi.WideMatch(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["shift_x"],
                         s["shift_y"], s["rot_steps"], s["rot_step"], s["max_blocks"])


def test_symbols_struct_and_defaults():
    lib = abi.load_library()
    for name in ("rplgpu_default_wide_match", "rplgpu_wide_match_check", "rplgpu_wide_match_blocks",
                 "rplgpu_wide_match_scratch_words", "rplgpu_pool_field_host", "rplgpu_pool_field_dev",
                 "rplgpu_match_wide_dev", "rplgpu_match_wide"):
        assert name in abi.ABI_SYMBOLS and getattr(lib, name)
    assert lib.rplgpu_abi_version() == 1
    assert C.sizeof(abi.WideMatch) == 40
    m = abi.WideMatch.defaults()
    got = {k: getattr(m, k) for k, _ in abi.WideMatch._fields_}
    for k, v in wo.DEFAULT.items():
        assert got[k] == (np.float32(v) if isinstance(v, float) else v), k
    assert m.check() == abi.OK and wo.spec_valid(wo.DEFAULT)
    assert (abi.WIDE_MATCH_BLOCK, abi.MAX_WIDE_SHIFT, abi.MAX_WIDE_BLOCKS) == (wo.S, wo.MAX_SHIFT, wo.MAX_BLOCKS)
    e13 = m.scan_match()
    assert np.array_equal(abi.scan_match_rotations(e13), mo.rotations(wo.DEFAULT))


@pytest.mark.parametrize("kw,ok", [
    (dict(), True), (dict(shift_x=256, shift_y=256), True), (dict(shift_x=257), False), (dict(shift_y=257), False),
    (dict(shift_x=0, shift_y=0), True), (dict(max_blocks=0), False), (dict(max_blocks=1), True),
    (dict(max_blocks=65536), True), (dict(max_blocks=65537), False), (dict(rot_steps=64, rot_step=0.01), True),
    (dict(rot_steps=65, rot_step=0.01), False), (dict(rot_steps=2, rot_step=0.0), False),
    (dict(rot_steps=2, rot_step=1.0), False), (dict(rot_steps=0, rot_step=-1.0), True),
    (dict(rot_steps=0, rot_step=float("inf")), False), (dict(resolution=0.0), False), (dict(width=0), False),
    (dict(height=4097), False), (dict(width=4096, height=4096), True), (dict(origin_x=float("nan")), False),
])
def test_spec_check_matches_the_oracle(kw, ok):
    s = wo.spec(**kw)
    assert wo.spec_valid(s) == ok
    m = _struct(s)
    assert (m.check() == abi.OK) == ok
    assert abi.wide_match_blocks(m) == (wo.blocks_size(s) if ok else 0)
    assert abi.wide_match_scratch_words(m, 3) == (wo.scratch_words(s, 3) if ok else 0)
    if not ok:
        with pytest.raises(abi.RplGpuError):
            abi.wide_match_check(m)


def test_blocks_and_scratch_sizes():
    for T, nb in ((0, 1), (3, 1), (4, 2), (7, 2), (8, 3), (64, 17), (127, 32), (128, 33), (256, 65)):
        m = _struct(wo.spec(shift_x=T, shift_y=3, rot_steps=2, rot_step=0.01))
        assert abi.wide_match_blocks(m) == 5 * nb == wo.blocks_size(wo.spec(shift_x=T, shift_y=3, rot_steps=2))
    last = 0
    for cap in (1, 2, 63, 64, 1024, 65536):  # not decreasing in the cap and in G, and at least the cap's cost
        m = _struct(wo.spec(max_blocks=cap))
        words = [abi.wide_match_scratch_words(m, G) for G in (0, 1, 2, 3, 300, 65535)]
        assert words[0] == 0 and all(a <= b for a, b in zip(words, words[1:]))
        assert words[1] >= 65 * cap and words[1] >= last and words[4] == 300 * words[1]
        last = words[1]


POOL_SHAPES = [(1, 1), (9, 1), (1, 9), (8, 8), (7, 9), (40, 61), (33, 64), (3, 200)]  # (H, W)


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=[f"{h}x{w}" for h, w in POOL_SHAPES])
def test_pool_field_host_against_the_oracle(shape):
    rng = np.random.default_rng(2420 + shape[0] * 7 + shape[1])
    edge = np.array([-128, -1, 0, 1, 127], np.int8)
    fields = [np.full(shape, b, np.int8) for b in edge]                       # each of the bytes alone
    fields.append(rng.choice(edge, size=shape))                               # ... and together
    fields.append(rng.integers(-128, 128, shape).astype(np.int8))
    sparse = np.zeros(shape, np.int8)
    sparse[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = 77         # one cell: an 8 x 8 square of P
    fields.append(sparse)
    for f in fields:
        got = abi.pool_field_host(f)
        want = wo.pool(f)
        assert got.shape == want.shape == (shape[0] + 7, shape[1] + 7) and got.tobytes() == want.tobytes()
        assert got.min() >= 0 and got.max() == max(int(f.max()), 0)
    assert (abi.pool_field_host(sparse) == 77).sum() == 64


def test_pool_field_host_refusals():
    lib = abi.load_library()
    f = np.zeros((2, 2), np.int8)
    out = np.full((9, 9), 0x5A, np.int8)
    bad = abi.ERR_INVALID_ARG
    assert lib.rplgpu_pool_field_host(0, 2, 2, out.ctypes.data) == bad
    assert lib.rplgpu_pool_field_host(f.ctypes.data, 2, 2, 0) == bad
    assert lib.rplgpu_pool_field_host(f.ctypes.data, 0, 2, out.ctypes.data) == bad
    assert lib.rplgpu_pool_field_host(f.ctypes.data, 2, 4097, out.ctypes.data) == bad
    assert (out == 0x5A).all()


# ---- every case of the device test: the two writers, the bound, the regime -------------------------------------------
def _hold(oracle, case, key):
    """Writer 2 against writer 1, U against the exhaustive volume's block maxima, P against the host twin."""
    want = wc.case_want(oracle, case, key)
    exhaustive = wc.case_exhaustive(oracle, case, key)
    assert wc.writers_agree(want, exhaustive) and wc.bound_holds(case, want, exhaustive)
    assert abi.pool_field_host(mc.case_field(case, 0)).tobytes() == want[0]["P"].tobytes()
    return want


@pytest.mark.parametrize("disp", wc.RECOVERY_DISPLACEMENTS, ids=[str(d) for d in wc.RECOVERY_DISPLACEMENTS])
def test_recovery(oracle, disp):
    case = wc.recovery_case(oracle, disp)
    wc.recovery_regime(oracle, case)
    want = _hold(oracle, case, f"recovery{disp}")
    if disp == wc.RECOVERY_DISPLACEMENTS[0]:  # writer 1 against match_oracle's own volume, once (it takes seconds)
        vol, _ = mo.scores_correlate(*mo.finite_points(*mc.case_points(oracle, case, 0)), case["pivot"][0],
                                     case["spec"], case["fields"][0])
        assert vol.tobytes() == wc.case_exhaustive(oracle, case, f"recovery{disp}")[0][0].tobytes()
    assert want[0]["work"][4] <= 1024


def test_identity_cases(oracle):
    for name, case in wc.identity_cases(oracle).items():
        wc.identity_regime(oracle, name, case)
        _hold(oracle, case, f"id_{name}")
        e13 = mc.case_want(oracle, dict(case, spec=wo.scan_match_spec(case["spec"])), f"id13_{name}")[0]
        assert wc.case_exhaustive(oracle, case, f"id_{name}")[0][0].tobytes() == e13[0].tobytes(), name


def test_the_list(oracle):
    case = wc.noisy_case(oracle)
    wc.noisy_regime(oracle, case)
    _hold(oracle, case, "noisy")
    case = wc.equal_peaks_case(oracle)
    wc.equal_peaks_regime(oracle, case)
    _hold(oracle, case, "equal_peaks")
    case = wc.uniform_case()
    wc.uniform_regime(oracle, case)
    _hold(oracle, case, "uniform")


@pytest.mark.parametrize("name", sorted(wc.FAR_TIES))
def test_far_ties(oracle, name):
    case = wc.far_ties_case(name)
    wc.far_ties_regime(oracle, name, case)
    _hold(oracle, case, f"far_{name}")


def test_the_cap(oracle):
    for name, (case, proven) in wc.cap_cases(oracle).items():
        wc.cap_regime(oracle, name, case, proven)
        _hold(oracle, case, f"cap_{name}")


def test_layouts_cover_the_kernel():
    wc.layouts_cover_the_kernel()


@pytest.mark.parametrize("t", wc.LAYOUTS, ids=[wc.layout_name(t) for t in wc.LAYOUTS])
def test_layouts(oracle, t):
    case = wc.layout_case(t)
    wc.layout_regime(oracle, t, case)
    _hold(oracle, case, f"layout_{wc.layout_name(t)}")


@pytest.mark.parametrize("name", sorted(wc.edge_cases()))
def test_edges(oracle, name):
    case = wc.edge_cases()[name]
    wc.edge_regime(oracle, name, case)
    _hold(oracle, case, f"edge_{name}")


def test_passes(oracle):
    case = wc.passes_case()
    wc.passes_regime(oracle, case)
    want = wc.case_want(oracle, case, "passes")
    assert wc.writers_agree(want, wc.case_exhaustive(oracle, case, "passes"))


@pytest.mark.parametrize("per_group", [0, 1])
def test_groups(oracle, per_group):
    case = wc.groups_case(per_group)
    want = wc.groups_regime(oracle, case, f"groups{per_group}")
    exhaustive = wc.case_exhaustive(oracle, case, f"groups{per_group}")
    assert wc.writers_agree(want, exhaustive) and wc.bound_holds(case, want, exhaustive)


# ---- the host twin under the host sanitizers ----------------------------------------------------------------------------
def test_wide_rules_unit_is_plain_cpp_and_clean_under_the_sanitizers(tmp_path):
    """csrc/rplgpu_wide_rules.cpp and tools/dev/wide_rules_asan.cpp, a program with its own main, build from those two
    files alone, warning-free, with -fsanitize=address,undefined (plain where the compiler here has no sanitizer
    runtime) and the program ends clean.  Nothing loaded into Python runs under a sanitizer."""
    rules = ROOT / "rplidar_ros2_driver_amd" / "csrc" / "rplgpu_wide_rules.cpp"
    text = rules.read_text()
    assert "hip/hip_runtime" not in text and "rpl_launch.hpp" not in text
    cxx = shutil.which("clang++") or shutil.which("g++")
    assert cxx
    exe = tmp_path / "wide_rules"
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
            f"-I{rules.parent}", str(rules), str(ROOT / "tools" / "dev" / "wide_rules_asan.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:  # (no sanitizer runtime here; a fault of the sources fails the plain build as well)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "WRONG" not in r.stdout and r.stdout.count("pool ") == 10
