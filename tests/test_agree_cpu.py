"""E23 without a device: the new symbols, the spec check's table, the oracle's two writers against each other on every
case of tests/agree_cases.py, the host twin (rplgpu_beam_agree_points_host, through abi.py) against both, identities
1 to 3 on the twin, a known answer worked out by hand and every regime check."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import agree_cases as ac
from tests import agree_oracle as ao
from tests import pose_cases as pc

F32 = np.float32
NAMES = ("counts", "mask", "weights", "result", "agree", "status")


def _struct(s):
    return abi.BeamAgree(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["agree_lo"],
                         s["keep_num"], s["keep_den"], s["err_num"], s["err_den"])


def _twin(oracle, case, g=0, spec=None):
    x, y, slot, idx, ns = ac.case_group_points(oracle, case, g)
    return abi.beam_agree_points_host(x, y, slot, idx, ns, case["batch"].shape[1], pc.case_poses(case, g),
                                      pc.case_field(case, g), _struct(spec or case["spec"]))


def _same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        if name == "status":
            assert int(a) == int(b), (what, name, a, b)
        else:
            assert np.asarray(a).shape == np.asarray(b).shape, (what, name)
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (what, name, a, b)


def test_symbols_and_struct():
    lib = abi.load_library()
    for name in ("rplgpu_default_beam_agree", "rplgpu_beam_agree_check", "rplgpu_score_poses_agree_dev",
                 "rplgpu_score_poses_agree", "rplgpu_beam_agree_points_host"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(abi.BeamAgree) == 40
    d = abi.BeamAgree.defaults()
    for k, v in ao.spec().items():
        assert getattr(d, k) == (F32(v) if isinstance(v, float) else v), k
    assert (d.agree_lo, d.keep_num, d.keep_den, d.err_num, d.err_den) == (1, 3, 10, 9, 10)  # AMCL's 0.3 and 0.9
    with pytest.raises(AttributeError):
        abi.BeamAgree.defaults(skip=1)


SPECS = [
    (dict(), True),
    (dict(resolution=0.0), False), (dict(origin_x=float("nan")), False), (dict(width=0), False),
    (dict(height=4097), False), (dict(width=4096, height=4096), True),
    (dict(agree_lo=0), False), (dict(agree_lo=1), True), (dict(agree_lo=127), True), (dict(agree_lo=128), False),
    (dict(agree_lo=-5), False),
    (dict(keep_den=0), False), (dict(keep_num=0, keep_den=1), True), (dict(keep_num=1, keep_den=1), True),
    (dict(keep_num=2, keep_den=1), False), (dict(keep_num=1 << 20, keep_den=1 << 20), True),
    (dict(keep_num=3, keep_den=(1 << 20) + 1), False),
    (dict(err_den=0), False), (dict(err_num=0), True), (dict(err_num=11, err_den=10), True),
    (dict(err_num=1 << 20, err_den=1), True), (dict(err_num=(1 << 20) + 1, err_den=1), False),
    (dict(err_num=1, err_den=(1 << 20) + 1), False),
]


@pytest.mark.parametrize("kw,ok", SPECS, ids=[str(i) for i in range(len(SPECS))])
def test_spec_check_matches_the_oracle(kw, ok):
    s = ao.spec(**kw)
    assert ao.spec_valid(s) == ok
    assert _struct(s).check() == (abi.OK if ok else abi.ERR_INVALID_ARG)
    assert abi.load_library().rplgpu_beam_agree_check(None) == abi.ERR_INVALID_ARG


def test_known_answer_by_hand(oracle):
    """3 poses, 4 samples, keep 1 / 2, err 3 / 4, agree_lo 60.  The rows are each sample's look-ups at poses 0, 1, 2:
    counts 3, 2, 1, 0; 2 * count > 3 keeps samples 0 and 1; 2 of 4 skipped, 2 * 4 < 3 * 4: no fallback."""
    values = [[70, 70, 70], [70, 70, 10], [70, 5, 5], [0, 0, 0]]
    case = ac.stripe_case(((0, 1, 2, 3),), values, 3, dict(agree_lo=60, keep_num=1, keep_den=2, err_num=3, err_den=4))
    ac.stripe_regime(oracle, case)
    n = case["batch"].shape[1]
    counts = np.zeros((1, n), np.uint32)
    counts[0, :4] = (3, 2, 1, 0)
    want = (counts, np.array([[0b0011]], np.uint32), np.array([140, 140, 80], np.uint32),
            np.array([140, 0, 2, 0, 4, 140, 360, 0], np.uint32), np.array([4, 2, 0, 2, 3, 0, 6, 0], np.uint32), 0)
    for writer in ao.WRITERS:
        _same(ac.case_want(oracle, case, None, writer=writer)[0], want, writer)
    _same(_twin(oracle, case), want, "twin")
    # the fallback by hand: err 1 / 2, 2 * 2 >= 1 * 4: every sample enters, E15's weights
    back = dict(case, spec=dict(case["spec"], err_num=1, err_den=2))
    want_back = (counts, want[1], np.array([210, 145, 85], np.uint32),
                 np.array([210, 0, 1, 0, 4, 210, 440, 0], np.uint32), np.array([4, 2, 1, 4, 3, 0, 6, 0], np.uint32), 0)
    _same(_twin(oracle, back), want_back, "twin, fallback")
    _same(ac.case_want(oracle, back, None, writer="rows")[0], want_back, "rows, fallback")


def _named():
    return dict(
        person=(ac.person_case, ac.person_regime), lost=(ac.lost_case, ac.lost_regime),
        edge=(lambda o: ac.edge_case(), ac.edge_regime),
        all_from_skipped=(lambda o: ac.all_from_skipped_case(), ac.all_from_skipped_regime),
        limits=(lambda o: ac.limits_case(), ac.limits_regime))


@pytest.mark.parametrize("name", sorted(_named()))
def test_named_cases_writers_twin_and_regime(oracle, name):
    make, regime = _named()[name]
    case = make(oracle)
    regime(oracle, case)
    a = ac.case_want(oracle, case, name, writer="pairs")
    b = ac.case_want(oracle, case, name, writer="rows")
    for g in range(len(a)):
        _same(a[g], b[g], (name, g, "writers"))
        _same(_twin(oracle, case, g), a[g], (name, g, "twin"))


@pytest.mark.parametrize("make,regime,key", [
    (lambda: ac.layout_case(65), ac.layout_regime, None),
    (lambda: ac.layout_case(1), ac.layout_regime, None),
    (lambda: ac.samples_case(33), lambda o, c: ac.samples_regime(o, c, "n33"), "n33"),
    (lambda: ac.samples_case(2049), lambda o, c: ac.samples_regime(o, c, "n2049"), "n2049"),
    (lambda: ac.groups_case(1, 1), lambda o, c: ac.groups_regime(o, c, "groups11"), "groups11"),
    (lambda: ac.front_case(), ac.front_regime, "front"),
], ids=["layout65", "layout1", "n33", "n2049", "groups11", "front"])
def test_device_cases_writers_twin_and_regime(oracle, make, regime, key):
    case = make()
    regime(oracle, case)
    key = key or f"layout{case['poses'].shape[1]}"
    a = ac.case_want(oracle, case, key, writer="pairs")
    b = ac.case_want(oracle, case, key, writer="rows")
    for g in range(len(a)):
        _same(a[g], b[g], (key, g, "writers"))
        got = _twin(oracle, case, g)
        want = list(a[g])
        want[5] &= ~abi.SCAN_OUT_TRUNCATED  # (the twin sees points, not scans)
        _same(got, want, (key, g, "twin"))


def test_identities_on_the_twin(oracle):
    # (1) err_num = 0: the weights and result words are E15's
    case = ac.person_case(oracle)
    off = dict(case, spec=dict(case["spec"], err_num=0))
    e15 = pc.case_want(oracle, ac.pose_case(case), "agree_person_e15")[0]
    got = _twin(oracle, off)
    assert got[2].tobytes() == e15[0].tobytes() and got[3].tobytes() == e15[1].tobytes() and got[4][2] == 1
    assert got[1].tobytes() == _twin(oracle, case)[1].tobytes()  # the rule's mask, fallback or not
    # (2) bytes 0 and 1, agree_lo 1: the sum of the counts is the sum of E15's weights
    two = ac.identity2_case()
    e15 = pc.case_want(oracle, ac.pose_case(two), "agree_id2_e15")[0]
    got = _twin(oracle, two)
    assert got[4][6:].tobytes() == e15[1][6:].tobytes() and got[4][6] > 0
    # (3) P = 1, agree_lo 1, keep_num 0, err_num > err_den: E15's weight, the mask is the samples with f >= 1
    one = ac.identity3_case()
    e15 = pc.case_want(oracle, ac.pose_case(one), "agree_id3_e15")[0]
    got = _twin(oracle, one)
    assert got[2].tobytes() == e15[0].tobytes() and got[4][2] == 0
    bits = ac.finite_bits((got[0], got[1]))
    assert (bits == (got[0] >= 1)).all() and 0 < bits.sum() < got[4][0]


def test_twin_refusals():
    lib = abi.load_library()
    s = _struct(ao.spec(width=4, height=4))
    x = np.zeros(2, F32)
    sl = np.zeros(2, np.uint32)
    poses = np.zeros(4, F32)
    field = np.zeros(16, np.int8)
    out = np.full(64, 7, np.uint32)

    def call(n_points=2, n_scans=1, n_stride=4, P=1, spec=s, slot=sl, index=sl, poses_at=poses.ctypes.data):
        return lib.rplgpu_beam_agree_points_host(
            x.ctypes.data, x.ctypes.data, slot.ctypes.data, index.ctypes.data, n_points, n_scans, n_stride, poses_at,
            P, field.ctypes.data, C.byref(spec), out.ctypes.data, out.ctypes.data + 64, out.ctypes.data + 96,
            out.ctypes.data + 128, out.ctypes.data + 160, 0)

    bad = abi.ERR_INVALID_ARG
    assert call(P=0) == bad and call(P=abi.MAX_POSES + 1) == bad and call(n_scans=0) == bad and call(n_stride=0) == bad
    assert call(n_scans=4097, n_stride=4096) == bad and call(poses_at=0) == bad
    assert call(spec=_struct(ao.spec(width=4, height=4, agree_lo=0))) == bad
    assert call(slot=np.array([0, 1], np.uint32)) == bad and call(index=np.array([0, 4], np.uint32)) == bad
    assert (out == 7).all()
    assert call(index=np.array([0, 1], np.uint32)) == abi.OK and out[40] == 2  # agree word 0: two finite points
