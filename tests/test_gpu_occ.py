"""E11 on the device: rplgpu_occupancy_grid_dev against tests/occ_oracle.py byte for byte (grids, d_cells,
d_status), the serialised messages of rplgpu_occupancy_grid_msgs_dev against the oracle's restatement, and
the tie to E9's points.  The inputs and their regime checks live in tests/occ_cases.py."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import RplGpu, abi
from tests import merge_oracle as mo
from tests import occ_cases as oc
from tests import occ_oracle as oo

pytestmark = pytest.mark.gpu
GUARD = 0x5A


def _struct(s):
    return abi.OccGrid(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["range_min"],
                       s["obstacle_max"], s["raytrace_max"])


def _run(gpu, case, prev=None, p=None, same_prev=False, cells=True, status=True):
    """-> (grids (G, H, W) int8, cells (G, 3), status (G,), guard bytes (G, 4)).  cells / status False: NULL
    goes in for d_cells / d_status, and the buffer comes back as it was filled (777 / 99)."""
    import torch
    dev = torch.device("cuda:0")
    batch, s = case["batch"], case["spec"]
    B, n = batch.shape
    G = len(oc.case_groups(case))
    W, H = s["width"], s["height"]
    stride = ((W * H + 3) & ~3) + 4  # four guard bytes behind every group
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    d_nodes = up(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8))
    d_len = up(np.asarray(case["lens"], np.int32))
    d_mo, d_po, d_t0 = up(case.get("motion")), up(case.get("pose2d")), up(case.get("t0"))
    d_grid = torch.full((G * stride,), GUARD, dtype=torch.uint8, device=dev)
    d_prev = None
    if prev is not None:
        host = np.full((G, stride), GUARD, np.uint8)
        host[:, :W * H] = np.asarray(prev, np.int8).reshape(G, W * H).view(np.uint8)
        d_prev = up(host.reshape(-1))
    d_cells = torch.full((G * 3,), 777, dtype=torch.int32, device=dev)
    d_st = torch.full((G,), 99, dtype=torch.int32, device=dev)
    gpu.set_scan_time_offsets_dev(ptr(d_t0))
    try:
        gpu.occupancy_grid_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, case["group"], p or case["p"], ptr(d_mo),
                               ptr(d_po), _struct(s), d_grid.data_ptr() if same_prev else ptr(d_prev),
                               d_grid.data_ptr(), stride, d_cells.data_ptr() if cells else 0,
                               d_st.data_ptr() if status else 0)
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    raw = d_grid.cpu().numpy().reshape(G, stride)
    return (raw[:, :W * H].view(np.int8).reshape(G, H, W), d_cells.cpu().numpy().reshape(G, 3).astype(np.int64),
            d_st.cpu().numpy().astype(np.int64), raw[:, W * H:])


def _check(got, want, has_cells=True, has_status=True):
    """has_cells / has_status False: the call was made without d_cells / d_status, and nothing wrote there."""
    grids, cells, status, guard = got
    if not has_cells:
        assert (cells == 777).all()
        cells = np.array([wc for _, wc, _ in want])
    if not has_status:
        assert (status == 99).all()
        status = np.array([ws for _, _, ws in want])
    assert len(grids) == len(want)
    for g, (wg, wc, ws) in enumerate(want):
        diff = np.argwhere(grids[g] != wg)
        print(f"group {g}: cells {tuple(cells[g])} want {wc}, status {status[g]} want {ws}, {len(diff)} cells differ")
        assert len(diff) == 0, (g, diff[:8], grids[g][tuple(diff[:8].T)], wg[tuple(diff[:8].T)])
        assert tuple(cells[g]) == wc and status[g] == ws, g
    assert (guard == GUARD).all()


def test_small_exact(gpu, oracle):
    case = oc.small_case(oracle)
    oc.small_regime(oracle, case)
    got = _run(gpu, case)
    _check(got, oc.case_want(oracle, case, "small"))
    for g, dd in enumerate(oc.KNOWN_RAYS):  # and against the cells written out by hand
        assert np.array_equal(got[0][g], oc.known_grid(dd)), dd


def test_grid_edges(gpu, oracle):
    case = oc.edges_case()
    oc.edges_regime(oracle, case)
    _check(_run(gpu, case), oc.case_want(oracle, case, "edges"))


def test_ranges(gpu, oracle):
    case = oc.ranges_case()
    oc.ranges_regime(oracle, case)
    _check(_run(gpu, case), oc.case_want(oracle, case, "ranges"))


def test_marks_beat_clears_and_history_is_kept(gpu, oracle):
    case = oc.wall_case()
    untouched = oc.wall_regime(oracle, case)
    _check(_run(gpu, case), oc.case_want(oracle, case, "wall"))
    prev = oc.wall_prev(case)
    got = _run(gpu, case, prev=prev)
    _check(got, oc.case_want(oracle, case, "wall_prev", prev=prev))
    assert np.array_equal(got[0][0][untouched], prev[0][untouched]) and (got[0][0][untouched] == 37).sum() >= 1
    with pytest.raises(abi.RplGpuError) as e:
        _run(gpu, case, same_prev=True)
    assert e.value.code == abi.ERR_INVALID_ARG


def test_clears_beyond_the_window(gpu, oracle):
    """Rays of 500 cells from three sensors: clears on all four sides of a window inside the grid, from a window
    over two grid edges, and from a sensor whose window is wholly off the grid; then over a previous grid."""
    case = oc.far_case()
    oc.far_regime(oracle, case)
    _check(_run(gpu, case), oc.case_want(oracle, case, "far"))
    prev = oc.far_prev(case)
    _check(_run(gpu, case, prev=prev), oc.case_want(oracle, case, "far_prev", prev=prev))


def test_window_flush_alignments(gpu, oracle):
    """Every (width mod 4, window corner mod 4): the four sensors in one grid, then each in a grid of its own."""
    cases = {W: oc.flush_case(W) for W in oc.FLUSH_WIDTHS}
    oc.flush_regime(oracle, cases)
    for W, case in cases.items():
        _check(_run(gpu, case), oc.case_want(oracle, case, f"flush{W}"))
        alone = dict(case, group=1)
        _check(_run(gpu, alone), oc.case_want(oracle, alone, f"flush{W}_alone"))


@pytest.mark.parametrize("outside", [False, True], ids=["inside", "outside"])
@pytest.mark.parametrize("wh", oc.TINY_GRIDS, ids=[f"{w}x{h}" for w, h in oc.TINY_GRIDS])
def test_tiny_grids(gpu, oracle, wh, outside):
    """Grids narrower than a word or a nibble: the tail of the last word and the guard behind it stay."""
    case = oc.tiny_case(*wh, outside)
    oc.tiny_regime(oracle, case)
    want = oc.case_want(oracle, case, f"tiny{wh}{outside}")
    _check(_run(gpu, case), want)
    prev = np.full((1, wh[1], wh[0]), 37, np.int8)
    _check(_run(gpu, case, prev=prev), oc.case_want(oracle, case, f"tiny{wh}{outside}_prev", prev=prev))


def test_rays_near_the_step_cap(gpu, oracle):
    cases = oc.long_cases()
    oc.long_regime(oracle, cases)
    for i, case in enumerate(cases):
        want = oc.case_want(oracle, case, f"long{i}")
        assert want[0][2] == 0
        _check(_run(gpu, case), want)


def test_ragged_lengths(gpu, oracle):
    case = oc.ragged_case()
    oc.ragged_regime(oracle, case)
    _check(_run(gpu, case), oc.case_want(oracle, case, "ragged"))


def test_optional_outputs(gpu, oracle):
    """d_cells and d_status are optional: without either, or both, the same grids."""
    case = oc.far_case()
    want = oc.case_want(oracle, case, "far")
    for cells, status in ((False, True), (True, False), (False, False)):
        _check(_run(gpu, case, cells=cells, status=status), want, cells, status)
    cut = dict(case, lens=case["lens"].copy())
    cut["lens"][1] = case["batch"].shape[1] + 7  # more than the stride holds: the truncated bit, were it asked for
    wcut = oc.case_want(oracle, cut)
    assert wcut[0][2] == abi.SCAN_OUT_TRUNCATED and np.array_equal(wcut[0][0], want[0][0])
    _check(_run(gpu, cut, status=False), wcut, True, False)
    _check(_run(gpu, cut), wcut)


@pytest.mark.parametrize("ror_mode", [0, 1], ids=["ror_inside", "ror_two_kernels"])  # RPLGPU_ROR_INSIDE / _TWO_KERNELS
@pytest.mark.parametrize("inverted", [0, 1])
def test_full_front_end(gpu, oracle, inverted, ror_mode):
    """E11 always builds the E1 AND E5 keep mask in a pass of its own (as E9 does) and ignores the handle's
    ror mode: both modes run the same kernels, and the second one shows only that the switch changes nothing."""
    case = oc.full_case(inverted)
    want = oc.case_want(oracle, case, f"full{inverted}")
    if not inverted and not ror_mode:
        oc.full_regime(oracle, case, want)
    lib = abi.load_library()
    assert lib.rplgpu_set_ror_mode(gpu._h, ror_mode) == abi.OK
    try:
        got = _run(gpu, case)
    finally:
        assert lib.rplgpu_set_ror_mode(gpu._h, 0) == abi.OK
    _check(got, want)


def test_cell_range(gpu, oracle):
    case = oc.cell_range_case()
    oc.cell_range_regime(oracle, case)
    want = oc.case_want(oracle, case, "cell_range")
    assert want[0][2] == abi.SCAN_CELL_RANGE
    _check(_run(gpu, case), want)


def test_ieee_divide_instance(gpu, oracle):
    """A handle whose fast divides are refused (as tests/test_gpu_ieee_div.py arranges): the same bytes."""
    import torch

    from tests.conftest import _shared_stream
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    case = oc.full_case(0, B=8)
    want = oc.case_want(oracle, oc.full_case(0), "full0")[:1]
    h = RplGpu(device=0, max_samples_per_scan=32768, max_batch=64)
    try:
        h.set_stream(_shared_stream().cuda_stream)
        assert lib.rplgpu_debug_force_ieee_div(h._h, 7) == abi.OK
        got = _run(h, case)
        torch.cuda.synchronize()
    finally:
        h.close()
    _check(got, want)
    fast = _run(gpu, case)
    assert fast[0].tobytes() == got[0].tobytes()


@pytest.mark.parametrize("frame", ["", "base_link"])
def test_messages_match_restatement(gpu, oracle, frame):
    import torch
    dev = torch.device("cuda:0")
    case = oc.edges_case()
    case["batch"], case["lens"], case["pose2d"], case["group"] = (case["batch"][:3], case["lens"][:3],
                                                                  case["pose2d"][:3], 1)
    grids = _run(gpu, case)[0]
    G, s = 3, case["spec"]
    W, H = s["width"], s["height"]
    assert len(grids) == G and (W * H) % 4 != 0
    stride = (W * H + 3) & ~3
    host = np.zeros((G, stride), np.int8)
    host[:, :W * H] = grids.reshape(G, -1)
    d_grid = torch.from_numpy(host.reshape(-1)).to(dev)
    lay = abi.msg_occupancy_layout(len(frame), W, H)
    stamps = np.array([(100 + g, 1000 * g) for g in range(G)], dtype=[("sec", "<i4"), ("nanosec", "<u4")])
    d_stamps = torch.from_numpy(stamps.view(np.uint8)).to(dev)
    full = (lay.total_len + 3) & ~3
    for slot in (full, (lay.total_len - 1) & ~3):
        d_msgs = torch.zeros(G * slot, dtype=torch.uint8, device=dev)
        d_len = torch.full((G,), 77, dtype=torch.int32, device=dev)
        d_st = torch.zeros(G, dtype=torch.int32, device=dev)
        gpu.occupancy_grid_msgs_dev(d_grid.data_ptr(), stride, G, _struct(s), frame, d_stamps.data_ptr(),
                                    d_msgs.data_ptr(), slot, d_len.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
        msgs, lens, st = d_msgs.cpu().numpy(), d_len.cpu().numpy(), d_st.cpu().numpy()
        for g in range(G):
            if slot < lay.total_len:
                assert lens[g] == 0 and st[g] == abi.SCAN_OUT_TRUNCATED
                continue
            want = oo.occupancy_msg(frame, 100 + g, 1000 * g, s["resolution"], W, H, s["origin_x"], s["origin_y"],
                                    grids[g])
            assert lens[g] == len(want) == lay.total_len and st[g] == 0
            assert msgs[g * slot: g * slot + lens[g]].tobytes() == want


@pytest.mark.parametrize("wh", oc.MSG_GRIDS, ids=[f"{w}x{h}" for w, h in oc.MSG_GRIDS])
def test_messages_from_several_workgroups(gpu, wh):
    """Two workgroups per message, and the second trip of the grid-stride loop (tests/test_occ_cpu.py holds the
    two sizes against the kernel's constants).  The call takes any grid: random bytes."""
    import torch
    dev = torch.device("cuda:0")
    W, H = wh
    G, frame = 2, "map"
    s = oo.spec(width=W, height=H)
    stride = (W * H + 3) & ~3
    host = np.random.default_rng(1195).integers(-128, 128, (G, stride), dtype=np.int8)
    d_grid = torch.from_numpy(host.reshape(-1)).to(dev)
    lay = abi.msg_occupancy_layout(len(frame), W, H)
    stamps = np.array([(100 + g, 1000 * g) for g in range(G)], dtype=[("sec", "<i4"), ("nanosec", "<u4")])
    d_stamps = torch.from_numpy(stamps.view(np.uint8)).to(dev)
    full = (lay.total_len + 3) & ~3
    for slot in (full + 4, (lay.total_len - 1) & ~3):
        d_msgs = torch.full((G * slot,), GUARD, dtype=torch.uint8, device=dev)
        d_len = torch.full((G,), 77, dtype=torch.int32, device=dev)
        d_st = torch.zeros(G, dtype=torch.int32, device=dev)
        gpu.occupancy_grid_msgs_dev(d_grid.data_ptr(), stride, G, _struct(s), frame, d_stamps.data_ptr(),
                                    d_msgs.data_ptr(), slot, d_len.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
        msgs, lens, st = d_msgs.cpu().numpy().reshape(G, slot), d_len.cpu().numpy(), d_st.cpu().numpy()
        for g in range(G):
            if slot < lay.total_len:
                assert lens[g] == 0 and st[g] == abi.SCAN_OUT_TRUNCATED and (msgs[g] == GUARD).all()
                continue
            want = oo.occupancy_msg(frame, 100 + g, 1000 * g, s["resolution"], W, H, s["origin_x"], s["origin_y"],
                                    host[g, :W * H])
            assert lens[g] == len(want) == lay.total_len and st[g] == 0
            assert msgs[g, :lens[g]].tobytes() == want
            assert (msgs[g, lens[g]:] == GUARD).all()  # nothing behind the message


def test_marked_cells_hold_e9_points(gpu, oracle):
    """Whatever the walk does: every marked cell holds a point of E9's point set, and every such point that
    is in range for its sensor has its cell marked."""
    case = oc.ranges_case()
    s = case["spec"]
    grid = _run(gpu, case)[0][0]
    x, y, _, slot, _, _ = mo.group_points(oracle, list(case["batch"]), case["p"], None, case["pose2d"], None)
    sx, sy = oo.sensor_xy(2, case["pose2d"])
    r = oo.rays_of(x, y, sx[slot], sy[slot], s)
    has, cx, cy = oo.cells_of(x, y, s)
    inside = has & (cx >= 0) & (cx < s["width"]) & (cy >= 0) & (cy < s["height"])
    holds = np.zeros(grid.shape, bool)
    holds[cy[inside], cx[inside]] = True
    assert (grid == 100).sum() >= 50 and holds[grid == 100].all()
    must = inside & r["mark"]
    assert must.sum() >= 50 and (grid[cy[must], cx[must]] == 100).all()


def test_host_buffers_one_group(gpu, oracle):
    case = oc.wall_case()
    prev = oc.wall_prev(case)
    want = oc.case_want(oracle, case, "wall_prev", prev=prev)[0]
    grid, cells, status = gpu.occupancy_grid(case["batch"], case["lens"], case["p"], _struct(case["spec"]),
                                             pose2d=case["pose2d"], prev=prev[0])
    assert grid.tobytes() == want[0].tobytes() and cells == want[1] and status == want[2]


def test_bad_arguments_leave_a_working_handle(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    case = oc.ranges_case()
    batch, s = case["batch"], case["spec"]
    B, n = batch.shape
    cells = s["width"] * s["height"]
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(cells + 8, dtype=torch.uint8, device=dev)
    d_t0 = torch.zeros(B, dtype=torch.float32, device=dev)
    host = np.zeros(cells, np.int8)

    def call(**kw):
        a = dict(nodes=d_nodes.data_ptr(), B=B, group=B, grid=_struct(s), out=d_grid.data_ptr(), stride=cells, prev=0)
        a.update(kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.occupancy_grid_dev(a["nodes"], n, d_len.data_ptr(), a["B"], a["group"], case["p"], 0, 0, a["grid"],
                                   a["prev"], a["out"], a["stride"], 0, 0)
        return e.value.code

    assert call(grid=_struct(oo.spec(resolution=0.0))) == abi.ERR_INVALID_ARG
    assert call(stride=cells - 4) == abi.ERR_INVALID_ARG
    assert call(stride=cells + 2) == abi.ERR_INVALID_ARG
    assert call(out=d_grid.data_ptr() + 1) == abi.ERR_INVALID_ARG
    assert call(out=0) == abi.ERR_INVALID_ARG
    assert call(out=host.ctypes.data) == abi.ERR_INVALID_ARG  # plain host memory
    assert call(prev=d_grid.data_ptr()) == abi.ERR_INVALID_ARG
    assert call(group=0) == abi.ERR_INVALID_ARG
    assert call(nodes=0) == abi.ERR_INVALID_ARG
    assert call(B=gpu.max_batch + 1) == abi.ERR_CAPACITY
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        assert call() == abi.ERR_INVALID_ARG  # offsets set, d_motion NULL
    finally:
        gpu.set_scan_time_offsets_dev(0)
    _check(_run(gpu, case), oc.case_want(oracle, case, "ranges"))
