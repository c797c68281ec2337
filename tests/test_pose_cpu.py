"""E15 without a device: the new symbols, the host-only functions of include/rplgpu_msg.h (spec check, pose list)
against tests/pose_oracle.py, the oracle's two writers against each other on every case of tests/pose_cases.py,
the two identities against the E13 and E14 oracles, a known answer worked out by hand, what the kernel's layout
formula says the list of P reaches, and every regime check."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import pose_cases as pc
from tests import pose_oracle as po

F32 = np.float32


def _struct(s):
    return abi.PoseScore(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"])


def test_symbols_and_struct():
    lib = abi.load_library()
    for name in ("rplgpu_default_pose_score", "rplgpu_pose_score_check", "rplgpu_pose_list",
                 "rplgpu_score_poses_dev", "rplgpu_score_poses"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(abi.PoseScore) == 20 and abi.MAX_POSES == po.MAX_POSES == 1 << 20
    d = abi.PoseScore.defaults()
    for k, v in po.spec().items():
        assert getattr(d, k) == (F32(v) if isinstance(v, float) else v), k
    assert abi.PoseScore.defaults(width=9).width == 9
    with pytest.raises(AttributeError):
        abi.PoseScore.defaults(shift=1)


SPECS = [
    (dict(), True),
    (dict(resolution=0.0), False), (dict(resolution=-0.05), False), (dict(resolution=float("nan")), False),
    (dict(resolution=float("inf")), False), (dict(origin_x=float("inf")), False), (dict(origin_y=float("nan")), False),
    (dict(width=0), False), (dict(height=0), False), (dict(width=1, height=1), True),
    (dict(width=4096, height=4096), True), (dict(width=4097), False), (dict(height=4097), False),
]


@pytest.mark.parametrize("kw,ok", SPECS, ids=[str(i) for i in range(len(SPECS))])
def test_spec_check_matches_the_oracle(kw, ok):
    s = po.spec(**kw)
    assert po.spec_valid(s) == ok
    if ok:
        abi.pose_score_check(_struct(s))
    else:
        with pytest.raises(abi.RplGpuError) as e:
            abi.pose_score_check(_struct(s))
        assert e.value.code == abi.ERR_INVALID_ARG
    assert abi.load_library().rplgpu_pose_score_check(None) == abi.ERR_INVALID_ARG


def test_pose_list():
    rng = np.random.default_rng(1500)
    xyt = np.concatenate([rng.uniform(-100, 100, (500, 3)),
                          [[1.5, -2.5, 0.0], [0.0, 0.0, -0.0], [3.0, 4.0, math.pi], [0, 0, math.pi / 2],
                           [1e30, -1e-50, 1e9], [float("nan"), float("inf"), float("nan")], [0, 0, float("inf")]]])
    got = abi.pose_list(xyt)
    want = po.pose_list(xyt)
    assert got.dtype == F32 and got.shape == (len(xyt), 4) and got.tobytes() == want.tobytes()
    assert got[500].tobytes() == np.array([1, 0, 1.5, -2.5], F32).tobytes()   # theta == 0: exactly (1, 0)
    assert got[501].tobytes() == np.array([1, 0, 0, 0], F32).tobytes()        # ... and +0 for theta == -0
    for q in range(500):  # (cos, sin) rounded once from fp64
        assert got[q, 0] == F32(math.cos(xyt[q, 2])) and got[q, 1] == F32(math.sin(xyt[q, 2]))
    lib = abi.load_library()
    out = np.full(8, 7.0, F32)
    assert lib.rplgpu_pose_list(None, 0, None) == abi.OK
    assert lib.rplgpu_pose_list(None, 1, out.ctypes.data) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_pose_list(xyt.ctypes.data, 1, None) == abi.ERR_INVALID_ARG
    assert lib.rplgpu_pose_list(xyt.ctypes.data, abi.MAX_POSES + 1, out.ctypes.data) == abi.ERR_INVALID_ARG
    assert (out == 7.0).all()


def test_layout_formula_is_the_kernels():
    """A tripwire and no more: tests/pose_oracle.layout restates two lines of pose_lane in csrc/rpl_front.hpp (the one
    copy E15, E23 and E25 call), and this test only notices when those lines are edited, so that the restatement is
    looked at again.  It proves nothing about the compiled kernel; tests/test_gpu_pose.py::test_layouts over every P
    of LAYOUT_P is what holds the formula."""
    csrc = Path(__file__).resolve().parent.parent / "rplidar_ros2_driver_amd" / "csrc"
    src = (csrc / "rpl_front.hpp").read_text()
    assert "l.per = min((P + 63u) & ~63u, kPoseTile);" in src
    assert "l.slices = P <= kPoseTile ? kPoseTile / l.per : 1u;" in src
    assert re.search(r"constexpr uint32_t kPoseTile = kBlock;", src)
    assert "pose_lane(tile, P, " in (csrc / "rpl_pose.hip").read_text()
    dev = (Path(__file__).resolve().parent.parent / "rplidar_ros2_driver_amd" / "csrc" / "rpl_device.hpp").read_text()
    assert int(re.search(r"constexpr int kBlock = (\d+);", dev).group(1)) == po.TILE


def test_the_list_of_p_reaches_every_layout():
    got, last, every = pc.layout_reach()
    assert every == [1, 2, 3, 4, 5, 8, 16] and got == every      # every `slices` value
    assert 1 in last and 1023 in last                            # a last tile with 1 and with 1023 poses
    assert {1023, 1024, 1025} <= set(pc.LAYOUT_P)                # both sides of one tile
    for P in pc.LAYOUT_P:
        per, slices, tiles, tail = po.layout(P)
        assert per % 64 == 0 and slices * per <= po.TILE and (tiles - 1) * po.TILE + tail == P and 1 <= tail <= po.TILE
    assert {1, 63, 64, 65, 191, 192, 193, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, 3073} <= set(pc.LAYOUT_P)


def _agree(oracle, case, key):
    a = pc.case_want(oracle, case, key)
    b = pc.case_want(oracle, case, None, writer=po.weight_gather)
    assert len(a) == len(b)
    for (wa, ra, sa), (wb, rb, sb) in zip(a, b):
        assert wa.tobytes() == wb.tobytes() and ra.tobytes() == rb.tobytes() and sa == sb


@pytest.mark.parametrize("P", pc.LAYOUT_P)
def test_layout_cases(oracle, P):
    case = pc.layout_case(P)
    pc.layout_regime(oracle, case)
    _agree(oracle, case, f"layout{P}")


@pytest.mark.parametrize("n,P", [(18432, 65), (32768, 1025)])
def test_pass_cases(oracle, n, P):
    case = pc.pass_case(n, P)
    pc.pass_regime(oracle, case)
    _agree(oracle, case, f"pass{n}_{P}")


def test_limit_case(oracle):
    case = pc.limit_case()
    by = pc.limit_regime(oracle, case)
    assert len(by) == 8 + 12
    _agree(oracle, case, "limits")
    assert pc.case_want(oracle, case, "limits")[0][2] == abi.SCAN_CELL_RANGE
    finite = pc.limit_case([k for k in sorted(pc.limit_poses()) if k.startswith("off_") or k in ("identity", "zero")])
    assert pc.case_want(oracle, finite, "limits_finite")[0][2] == 0


def test_big_case(oracle):
    case = pc.big_case()
    pc.big_regime(oracle, case)
    _agree(oracle, case, "big")


@pytest.mark.parametrize("ppg,fpg", [(0, 0), (1, 1)])
def test_groups_cases(oracle, ppg, fpg):
    case = pc.groups_case(ppg, fpg)
    pc.groups_regime(oracle, case, f"groups{ppg}{fpg}")
    _agree(oracle, case, f"groups{ppg}{fpg}")


def test_front_cases(oracle):
    case = pc.front_case()
    pc.front_regime(oracle, case)
    _agree(oracle, case, "front")
    bare = pc.front_case(with_pose2d=False)
    assert pc.front_regime(oracle, bare, "front_nopose")[0][0].tobytes() != pc.case_want(oracle, case, "front")[0][0].tobytes()


def test_identity_a_against_the_match_oracle(oracle):
    pc.identity_a_regime(oracle)
    _agree(oracle, pc.identity_a_case()[1], "pose_ida")


def test_identity_b_against_the_map_oracle(oracle):
    pc.identity_b_regime(oracle)
    _agree(oracle, pc.identity_b_case()[1], "pose_idb")


@pytest.mark.parametrize("name", sorted(pc.words_cases()))
def test_words_cases(oracle, name):
    case, expect, high = pc.words_cases()[name]
    pc.words_regime(oracle, name, case, expect, high)
    _agree(oracle, case, f"words_{name}")


def test_chain_case(oracle):
    case = pc.chain_case(oracle)
    pc.chain_regime(oracle, case)
    _agree(oracle, case, "chain")


def test_known_answer_by_hand(oracle):
    case, want = pc.known_case()
    for writer in (po.weight_bincount, po.weight_gather):
        w, res, status = pc.case_want(oracle, case, None, writer=writer)[0]
        assert w.tobytes() == want.tobytes() and status == 0 and res[4] == 9
        assert tuple(int(v) for v in res) == (9 * 127, 5, 1, 7, 9, 0, int(want.sum()), 0)


def test_result_words_by_hand():
    assert po.result_of([5, 9, 0, 9, 0, 0], 4).tolist() == [9, 1, 2, 3, 4, 5, 23, 0]
    assert po.result_of([0, 0, 0], 0).tolist() == [0, 0, 3, 3, 0, 0, 0, 0]
    assert po.result_of([0xFFFFFFFF, 0xFFFFFFFF, 3], 1).tolist() == [0xFFFFFFFF, 0, 2, 0, 1, 0xFFFFFFFF, 1, 2]
