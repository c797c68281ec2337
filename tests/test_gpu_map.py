"""E14 on the device: rplgpu_map_update_dev, rplgpu_map_grid_dev and rplgpu_apply_match_dev against
tests/map_oracle.py, byte for byte (counts, grids, d_cells, status, poses, and guard words behind every output).
The inputs and their regime checks live in tests/map_cases.py; tests/test_map_cpu.py runs the regimes."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import RplGpu, abi
from tests import map_cases as mcs
from tests import map_oracle as mp
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import occ_cases as oc
from tests.test_gpu_occ import _run as occ_run
from tests.test_gpu_occ import _struct

pytestmark = pytest.mark.gpu
GUARD = 0x5A
GUARD32 = 0x5A5A5A5A
N_GUARD = 4  # guard words behind the map


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _new_map(W, H, counts=None):
    """The map (zeroed, or holding `counts`) with guard words behind it, as an int32 tensor."""
    host = np.full(2 * W * H + N_GUARD, GUARD32, np.uint32)
    host[:2 * W * H] = 0 if counts is None else mp.as_words(counts).reshape(-1)
    return _up(host.view(np.int32))


def _read_map(gpu, d_map, W, H):
    gpu.synchronize()
    raw = d_map.cpu().numpy().view(np.uint32)
    assert (raw[2 * W * H:] == GUARD32).all(), "words behind the map were written"
    return raw[:2 * W * H].reshape(H, W, 2).astype(np.int64)


def _update(gpu, case, d_map, status=True, p=None):
    """One rplgpu_map_update_dev call of all the case's scans -> status per group (or the untouched 99s)."""
    import torch
    batch, s = case["batch"], case["spec"]
    B, n = batch.shape
    G = len(oc.case_groups(case))
    d_nodes = _up(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8))
    d_len = _up(np.asarray(case["lens"], np.int32))
    d_mo, d_po, d_t0 = _up(case.get("motion")), _up(case.get("pose2d")), _up(case.get("t0"))
    d_st = torch.full((G + 1,), 99, dtype=torch.int32, device=_dev())
    gpu.set_scan_time_offsets_dev(_ptr(d_t0))
    try:
        gpu.map_update_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, case["group"], p or case["p"], _ptr(d_mo),
                           _ptr(d_po), _struct(s), d_map.data_ptr(), d_st.data_ptr() if status else 0)
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    st = d_st.cpu().numpy().astype(np.int64)
    assert st[G] == 99, "the word behind d_status was written"
    return list(st[:G])


def _check_counts(got, want, what=""):
    diff = np.argwhere(got != want)
    print(f"{what}: {int(want.sum())} counts wanted, {len(diff)} words differ")
    assert len(diff) == 0, (what, diff[:8], got[tuple(diff[:8].T)], want[tuple(diff[:8].T)])


def _run_case(gpu, oracle, case, key, **kw):
    s = case["spec"]
    W, H = s["width"], s["height"]
    want, wst = mcs.case_want(oracle, case, key)
    d_map = _new_map(W, H)
    st = _update(gpu, case, d_map, **kw)
    got = _read_map(gpu, d_map, W, H)
    _check_counts(got, want, key)
    if kw.get("status", True):
        assert st == wst, (key, st, wst)
    else:
        assert st == [99] * len(wst)
    return got


def _grid(gpu, d_map, W, H, rule, prev=None, cells=True, fill=GUARD):
    """rplgpu_map_grid_dev -> (grid (H, W) int8, cells (4,) or the untouched 777s)."""
    import torch
    stride = ((W * H + 3) & ~3) + 4  # four guard bytes behind the last word
    d_grid = torch.full((stride,), fill, dtype=torch.uint8, device=_dev())
    d_prev = None
    if prev is not None:
        host = np.full(stride, GUARD, np.uint8)
        host[:W * H] = np.asarray(prev, np.int8).reshape(-1).view(np.uint8)
        d_prev = _up(host)
    d_cells = torch.full((5,), 777, dtype=torch.int32, device=_dev())
    gpu.map_grid_dev(d_map.data_ptr(), W, H, abi.MapRule(rule["min_observations"], rule["occupied_percent"], rule["mode"]),
                     _ptr(d_prev), d_grid.data_ptr(), stride - 4, d_cells.data_ptr() if cells else 0)
    gpu.synchronize()
    raw = d_grid.cpu().numpy()
    assert (raw[W * H:] == fill).all(), "bytes at and beyond width * height were written"
    c = d_cells.cpu().numpy().astype(np.int64)
    assert c[4] == 777
    return raw[:W * H].view(np.int8).reshape(H, W), tuple(c[:4])


# ---- room ------------------------------------------------------------------------------------------------------------------
def test_room_one_call_then_persistence(gpu, oracle):
    c0, c1 = mcs.room_regime(oracle)
    s = mcs.ROOM_SPEC
    W, H = s["width"], s["height"]
    d_map = _new_map(W, H)
    assert _update(gpu, mcs.room_case(0), d_map) == [0]
    _check_counts(_read_map(gpu, d_map, W, H), c0, "room, time step 0")
    assert _update(gpu, mcs.room_case(1), d_map) == [0]
    _check_counts(_read_map(gpu, d_map, W, H), c0 + c1, "room, time steps 0 + 1")
    for rule in (mp.rule(), mp.rule(min_observations=1, mode=1)):
        want, wcells = mp.grid_of_counts(c0 + c1, rule)
        got, cells = _grid(gpu, d_map, W, H, rule)
        assert got.tobytes() == want.tobytes() and cells == wcells, rule


@pytest.mark.parametrize("step", [0, 1])
def test_room_counts_through_rule_100_equal_e11(gpu, oracle, step):
    """Two independent kernels held to each other: map_update + map_grid with rule (1, 0, 0) on a zeroed map writes
    what rplgpu_occupancy_grid_dev writes for the same arguments, with and without a previous grid."""
    case = mcs.room_case(step)
    s = case["spec"]
    W, H = s["width"], s["height"]
    d_map = _new_map(W, H)
    _update(gpu, case, d_map)
    prev = np.random.default_rng(step).choice(np.array([-1, 0, 100, 37], np.int8), size=(1, H, W))
    for pv in (None, prev):
        e11, e11_cells, _, _ = occ_run(gpu, case, prev=pv)
        got, cells = _grid(gpu, d_map, W, H, mp.E11_RULE, prev=None if pv is None else pv[0])
        assert got.tobytes() == e11[0].tobytes()
        if pv is None:
            assert cells == (e11_cells[0][2], e11_cells[0][0], e11_cells[0][1], 0)


# ---- one ray -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut"])
@pytest.mark.parametrize("n", mcs.RAY_LENS)
def test_one_ray_many_times(gpu, oracle, n, cut):
    """n identical samples: n misses in every cell of the ray (n = 32768: the LDS counter at its largest value), n
    hits in the end cell — or, cut, a miss there and no hit.  The answer is written out by hand (map_cases.ray_want;
    tests/test_map_cpu.py holds it against the oracle)."""
    case = mcs.ray_case(n, 1, cut)
    s = case["spec"]
    d_map = _new_map(s["width"], s["height"])
    assert _update(gpu, case, d_map) == [0]
    _check_counts(_read_map(gpu, d_map, s["width"], s["height"]), mcs.ray_want(n, 1, cut), f"one ray x {n}")


def test_one_ray_sums_pass_16_bits(gpu):
    case = mcs.ray_case(32768, 2)
    s = case["spec"]
    W, H = s["width"], s["height"]
    d_map = _new_map(W, H)
    assert _update(gpu, case, d_map) == [0]
    _check_counts(_read_map(gpu, d_map, W, H), mcs.ray_want(32768, 2), "two scans: 65536")
    assert _update(gpu, case, d_map) == [0]
    got = _read_map(gpu, d_map, W, H)
    _check_counts(got, 2 * mcs.ray_want(32768, 2), "the same call again: 131072")
    assert got.max() == 131072


# ---- runs ---------------------------------------------------------------------------------------------------------------------
def test_runs_of_equal_rays(gpu, oracle):
    assert mcs.runs_regime(oracle) > 64
    _run_case(gpu, oracle, mcs.runs_case()[0], "runs")


def test_rays_of_length_zero(gpu, oracle):
    """A whole ray whose end cell is the sensor cell marks it and does not clear it."""
    _run_case(gpu, oracle, mcs.zero_regime(oracle), "zero")


# ---- window -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mcs.WINDOW_GRIDS))
def test_window(gpu, oracle, name):
    case = mcs.window_regime(oracle, name)
    _run_case(gpu, oracle, case, "window_" + name)
    alone = dict(case, group=1)  # the same map; one status word per scan
    _run_case(gpu, oracle, alone, "window_alone_" + name)


# ---- many workgroups --------------------------------------------------------------------------------------------------------------
def test_many_workgroups_one_pose(gpu, oracle):
    mcs.many_regime(oracle)
    _run_case(gpu, oracle, mcs.many_same_case(), "many_same")


def test_many_short_scans(gpu, oracle):
    _run_case(gpu, oracle, mcs.many_short_case(), "many_short")


# ---- front end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverted", [0, 1])
def test_full_front_end(gpu, oracle, inverted):
    if not inverted:
        mcs.front_regime(oracle)
    _run_case(gpu, oracle, mcs.front_case(inverted), f"front{inverted}")


def test_ieee_divide_instance(gpu, oracle):
    """A handle whose fast divides are refused (as tests/test_gpu_ieee_div.py arranges): the same counts."""
    import torch

    from tests.conftest import _shared_stream
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    case = mcs.front_case(0)
    h = RplGpu(device=0, max_samples_per_scan=32768, max_batch=64)
    try:
        h.set_stream(_shared_stream().cuda_stream)
        assert lib.rplgpu_debug_force_ieee_div(h._h, 7) == abi.OK
        _run_case(h, oracle, case, "front0")
        torch.cuda.synchronize()
    finally:
        h.close()


def test_status_left_out(gpu, oracle):
    _run_case(gpu, oracle, mcs.many_short_case(), "many_short", status=False)


def test_host_buffer_doors(gpu, oracle):
    c0, c1 = mcs.room_regime(oracle)
    s = mcs.ROOM_SPEC
    counts = np.zeros((s["height"], s["width"], 2), np.uint32)
    for step in (0, 1):
        case = mcs.room_case(step)
        assert gpu.map_update(case["batch"], case["lens"], case["p"], _struct(s), counts, pose2d=case["pose2d"]) == 0
    _check_counts(counts.astype(np.int64), c0 + c1, "the door, two calls")
    prev = np.random.default_rng(3).choice(np.array([-1, 0, 100, 37], np.int8), size=counts.shape[:2])
    for rule, pv in ((mp.rule(), None), (mp.rule(min_observations=30), prev), (mp.rule(min_observations=1, mode=1), None)):
        want, wcells = mp.grid_of_counts(c0 + c1, rule, pv)
        got, cells = gpu.map_grid(counts, abi.MapRule(rule["min_observations"], rule["occupied_percent"], rule["mode"]), pv)
        assert got.tobytes() == want.tobytes() and cells == wcells, rule
    far = dict(mcs.room_case(0))
    far["pose2d"] = far["pose2d"].copy()
    far["pose2d"][1, 2] = 1.0e6
    before = counts.copy()
    assert gpu.map_update(far["batch"], far["lens"], far["p"], _struct(s), counts, pose2d=far["pose2d"]) == abi.SCAN_CELL_RANGE
    assert (counts >= before).all() and (counts != before).any()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", mcs.RULE_SHAPES + (mcs.RULE_BIG_SHAPE,), ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_rule_on_planted_counts(gpu, wh):
    """Counts planted by upload, no walk: every edge of the rule (map_cases.RULE_COUNTS) under every rule, with
    d_prev present and NULL, d_cells present and NULL, and the masked last word of the grid."""
    W, H = wh
    counts = mcs.rule_counts(W, H)
    d_map = _new_map(W, H, counts.astype(np.int64))
    prev = mcs.rule_prev(W, H)
    for rule in mcs.RULES:
        for pv in (None, prev):
            want, wcells = mp.grid_of_counts(counts, rule, pv)
            got, cells = _grid(gpu, d_map, W, H, rule, prev=pv)
            assert got.tobytes() == want.tobytes(), (rule, np.argwhere(got != want)[:5])
            assert cells == wcells, (rule, cells, wcells)
        got, cells = _grid(gpu, d_map, W, H, rule, cells=False, fill=0xC3)
        assert got.tobytes() == mp.grid_of_counts(counts, rule)[0].tobytes() and cells == (777,) * 4
    assert _read_map(gpu, d_map, W, H).tobytes() == counts.astype(np.int64).tobytes()  # the counts are only read


# ---- apply -------------------------------------------------------------------------------------------------------------------------
def _apply(gpu, c, flags, pivot=True, pose=True, in_place=False, pivot_out=True):
    import torch
    B, G = c["B"], c["G"]
    d_best = _up(c["best"].view(np.int32))
    d_pivot = _up(c["pivot"]) if pivot else None
    host_in = np.full((B + 1, 6), np.float32(7.5), np.float32)
    host_in[:B] = c["pose"]
    d_in = _up(host_in) if pose else None
    d_out = d_in if in_place else torch.full((B + 1, 6), 7.5, dtype=torch.float32, device=_dev())
    d_pout = torch.full((G + 1, 2), 7.5, dtype=torch.float32, device=_dev())
    gpu.apply_match_dev(d_best.data_ptr(), abi.ScanMatch(**c["spec"]), _ptr(d_pivot), _ptr(d_in), B, c["group"], flags,
                        d_out.data_ptr(), d_pout.data_ptr() if pivot_out else 0)
    gpu.synchronize()
    out, pout = d_out.cpu().numpy(), d_pout.cpu().numpy()
    assert (out[B] == 7.5).all() and (pout[G] == 7.5).all(), "words behind the outputs were written"
    if not pivot_out:
        assert (pout == 7.5).all()
    return out[:B], pout[:G]


@pytest.mark.parametrize("flags", [0, 1])
def test_apply_match(gpu, flags):
    c = mcs.apply_regime()
    want, wpivot = mp.apply_match(c["best"], c["spec"], c["pivot"], c["pose"], c["B"], c["group"], flags)
    got, gpivot = _apply(gpu, c, flags)
    assert got.tobytes() == want.tobytes() and gpivot.tobytes() == wpivot.tobytes()
    got, _ = _apply(gpu, c, flags, in_place=True, pivot_out=False)
    assert got.tobytes() == want.tobytes()
    want, wpivot = mp.apply_match(c["best"], c["spec"], None, None, c["B"], c["group"], flags)
    got, gpivot = _apply(gpu, c, flags, pivot=False, pose=False)
    assert got.tobytes() == want.tobytes() and gpivot.tobytes() == wpivot.tobytes()
    one = dict(c, group=c["B"] + 5, G=1, best=c["best"][:1], pivot=c["pivot"][:1])  # group clamped to B
    want, wpivot = mp.apply_match(one["best"], c["spec"], one["pivot"], c["pose"], c["B"], c["B"], flags)
    got, gpivot = _apply(gpu, one, flags)
    assert got.tobytes() == want.tobytes() and gpivot.tobytes() == wpivot.tobytes()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def test_chain_map_field_match_apply_map(gpu, oracle):
    """Time step 0 at its true pose -> map -> grid -> likelihood field; time step 1 with a displaced prior -> match ->
    apply -> map, every call queued on the stream before anything is read back."""
    import torch
    w = mcs.chain_regime(oracle)
    batch, lens, true_pose = mc.room_scans()
    B, n = batch.shape
    occ, spec = mc.room_occ_spec(), mc.ROOM_SPEC
    W, H = occ["width"], occ["height"]
    p = mcs.Params.defaults(**mc.ROOM_P)
    d_nodes = _up(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8))
    d_len = _up(np.asarray(lens, np.int32))
    d_true, d_prior, d_pivot = _up(true_pose), _up(w["prior"]), _up(mc.ROOM_PIVOT)
    d_table = _up(mc.ROOM_TABLE)
    d_map = _new_map(W, H)
    d_grid = torch.full((W * H + 4,), GUARD, dtype=torch.uint8, device=_dev())
    d_field = torch.full((W * H + 4,), GUARD, dtype=torch.uint8, device=_dev())
    vol = mo.volume_size(spec)
    d_scores = torch.zeros(vol, dtype=torch.int32, device=_dev())
    d_best = torch.full((9,), 99, dtype=torch.int32, device=_dev())
    d_pose = torch.full((B + 1, 6), 7.5, dtype=torch.float32, device=_dev())
    d_pivot_out = torch.full((2, 2), 7.5, dtype=torch.float32, device=_dev())
    d_st = torch.full((3,), 99, dtype=torch.int32, device=_dev())
    m = abi.ScanMatch(**spec)
    rule = abi.MapRule(**mcs.CHAIN_RULE)
    gpu.map_update_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, B, p, 0, d_true.data_ptr(), _struct(occ),
                       d_map.data_ptr(), d_st.data_ptr())
    gpu.map_grid_dev(d_map.data_ptr(), W, H, rule, 0, d_grid.data_ptr(), W * H, 0)
    gpu.inflate_grids_dev(d_grid.data_ptr(), W * H, d_field.data_ptr(), W * H, 1, W, H, d_table.data_ptr(), mc.ROOM_RC, 1, 0)
    gpu.match_scans_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, B, p, 0, d_prior.data_ptr(), d_pivot.data_ptr(), m,
                        d_field.data_ptr(), W * H, 0, d_scores.data_ptr(), vol, d_best.data_ptr(), d_st.data_ptr() + 4)
    gpu.apply_match_dev(d_best.data_ptr(), m, d_pivot.data_ptr(), d_prior.data_ptr(), B, B, 1, d_pose.data_ptr(),
                        d_pivot_out.data_ptr())
    gpu.map_update_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, B, p, 0, d_pose.data_ptr(), _struct(occ),
                       d_map.data_ptr(), d_st.data_ptr() + 8)
    gpu.synchronize()
    best = d_best.cpu().numpy().view(np.uint32)
    assert best[:8].tobytes() == mo.best_words(w["best"]).tobytes() and best[8] == 99
    pose = d_pose.cpu().numpy()
    assert pose[:B].tobytes() == w["corrected"].tobytes() and (pose[B] == 7.5).all()
    pv = d_pivot_out.cpu().numpy()
    assert pv[0].tobytes() == w["pivot_out"][0].tobytes() and (pv[1] == 7.5).all()
    assert d_grid.cpu().numpy()[:W * H].view(np.int8).tobytes() == w["grid0"].tobytes()
    assert d_field.cpu().numpy()[:W * H].view(np.int8).tobytes() == w["field"].tobytes()
    assert (d_grid.cpu().numpy()[W * H:] == GUARD).all()
    assert list(d_st.cpu().numpy()) == [0, 0, 0]
    _check_counts(_read_map(gpu, d_map, W, H), w["counts"], "the chain's final map")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_handle(gpu, oracle):
    import torch
    case = mcs.room_case(0)
    batch, s = case["batch"], case["spec"]
    B, n = batch.shape
    W, H = s["width"], s["height"]
    d_nodes = _up(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8))
    d_len = _up(np.asarray(case["lens"], np.int32))
    d_po = _up(case["pose2d"])
    d_map = torch.full((2 * W * H + 4,), GUARD32, dtype=torch.int32, device=_dev())
    d_st = torch.full((2,), 99, dtype=torch.int32, device=_dev())
    d_t0 = torch.zeros(B, dtype=torch.float32, device=_dev())
    host = np.zeros(2 * W * H, np.uint32)

    def code(fn, *a):
        with pytest.raises(abi.RplGpuError) as e:
            fn(*a)
        return e.value.code

    def update(**kw):
        a = dict(nodes=d_nodes.data_ptr(), B=B, group=B, grid=_struct(s), counts=d_map.data_ptr(), st=d_st.data_ptr(), n=n)
        a.update(kw)
        return code(gpu.map_update_dev, a["nodes"], a["n"], d_len.data_ptr(), a["B"], a["group"], case["p"], 0,
                    d_po.data_ptr(), a["grid"], a["counts"], a["st"])

    from tests import occ_oracle as oo
    assert update(grid=_struct(oo.spec(resolution=0.0))) == abi.ERR_INVALID_ARG
    assert update(counts=0) == abi.ERR_INVALID_ARG
    assert update(counts=d_map.data_ptr() + 4) == abi.ERR_INVALID_ARG  # 4-byte, not 8-byte aligned
    assert update(counts=host.ctypes.data) == abi.ERR_INVALID_ARG     # plain host memory
    assert update(st=d_st.data_ptr() + 2) == abi.ERR_INVALID_ARG
    assert update(group=0) == abi.ERR_INVALID_ARG
    assert update(nodes=0) == abi.ERR_INVALID_ARG
    assert update(n=0) == abi.ERR_INVALID_ARG
    assert update(B=gpu.max_batch + 1) == abi.ERR_CAPACITY
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        assert update() == abi.ERR_INVALID_ARG  # offsets set, d_motion NULL
    finally:
        gpu.set_scan_time_offsets_dev(0)

    stride = (W * H + 3) & ~3
    d_grid = torch.full((stride + 8,), GUARD, dtype=torch.uint8, device=_dev())
    d_cells = torch.full((4,), 777, dtype=torch.int32, device=_dev())

    def grid(**kw):
        a = dict(counts=d_map.data_ptr(), W=W, H=H, rule=abi.MapRule.defaults(), prev=0, out=d_grid.data_ptr(),
                 stride=stride, cells=d_cells.data_ptr())
        a.update(kw)
        return code(gpu.map_grid_dev, a["counts"], a["W"], a["H"], a["rule"], a["prev"], a["out"], a["stride"], a["cells"])

    assert grid(rule=abi.MapRule(0, 10, 0)) == abi.ERR_INVALID_ARG
    assert grid(rule=abi.MapRule(2, 101, 0)) == abi.ERR_INVALID_ARG
    assert grid(rule=abi.MapRule(2, 10, 2)) == abi.ERR_INVALID_ARG
    assert grid(W=0) == abi.ERR_INVALID_ARG and grid(H=4097) == abi.ERR_INVALID_ARG
    assert grid(stride=stride - 4) == abi.ERR_INVALID_ARG and grid(stride=stride + 2) == abi.ERR_INVALID_ARG
    assert grid(out=d_grid.data_ptr() + 1) == abi.ERR_INVALID_ARG and grid(out=0) == abi.ERR_INVALID_ARG
    assert grid(counts=d_map.data_ptr() + 4) == abi.ERR_INVALID_ARG and grid(counts=0) == abi.ERR_INVALID_ARG
    assert grid(prev=d_grid.data_ptr()) == abi.ERR_INVALID_ARG
    assert grid(cells=d_cells.data_ptr() + 2) == abi.ERR_INVALID_ARG

    c = mcs.apply_case()
    d_best, d_pivot, d_pose = _up(c["best"].view(np.int32)), _up(c["pivot"]), _up(c["pose"])
    d_out = torch.full((c["B"], 6), 7.5, dtype=torch.float32, device=_dev())
    d_pout = torch.full((c["G"], 2), 7.5, dtype=torch.float32, device=_dev())

    def apply(**kw):
        a = dict(best=d_best.data_ptr(), m=abi.ScanMatch(**c["spec"]), pivot=d_pivot.data_ptr(), B=c["B"], group=c["group"],
                 flags=0, out=d_out.data_ptr(), pout=d_pout.data_ptr())
        a.update(kw)
        return code(gpu.apply_match_dev, a["best"], a["m"], a["pivot"], d_pose.data_ptr(), a["B"], a["group"], a["flags"],
                    a["out"], a["pout"])

    assert apply(best=0) == abi.ERR_INVALID_ARG and apply(out=0) == abi.ERR_INVALID_ARG
    assert apply(group=0) == abi.ERR_INVALID_ARG and apply(flags=2) == abi.ERR_INVALID_ARG
    assert apply(m=abi.ScanMatch(**dict(c["spec"], rot_steps=65))) == abi.ERR_INVALID_ARG
    assert apply(out=d_out.data_ptr() + 2) == abi.ERR_INVALID_ARG
    assert apply(pout=d_pivot.data_ptr()) == abi.ERR_INVALID_ARG
    assert apply(B=gpu.max_batch + 1) == abi.ERR_CAPACITY
    gpu.synchronize()
    assert (d_map.cpu().numpy().view(np.uint32) == GUARD32).all() and (d_st.cpu().numpy() == 99).all()
    assert (d_grid.cpu().numpy() == GUARD).all() and (d_cells.cpu().numpy() == 777).all()
    assert (d_out.cpu().numpy() == 7.5).all() and (d_pout.cpu().numpy() == 7.5).all()
    # a good call of each after them
    _run_case(gpu, oracle, case, "room0")
    got, gp = _apply(gpu, c, 0)
    want, wp = mp.apply_match(c["best"], c["spec"], c["pivot"], c["pose"], c["B"], c["group"], 0)
    assert got.tobytes() == want.tobytes() and gp.tobytes() == wp.tobytes()
