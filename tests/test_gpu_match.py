"""E13 on the device: rplgpu_match_scans_dev against tests/match_oracle.py byte for byte — score volumes, d_best,
d_status, the guard words behind every volume and the unchanged field.  The inputs and their regime checks live
in tests/match_cases.py; every input is one the rule defines a result for."""
import ctypes as C

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, RplGpu, abi
from tests import match_cases as mc
from tests import match_oracle as mo

pytestmark = pytest.mark.gpu
GUARD = 0x5A
GUARD_WORD = 0x5A5A5A5A
PAD = 5  # guard words behind every volume


def _struct(s):
    return abi.ScanMatch(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["shift_x"],
                         s["shift_y"], s["rot_steps"], s["rot_step"])


def _upload(case):
    import torch
    dev = torch.device("cuda:0")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    batch = case["batch"]
    B, n = batch.shape
    d = dict(nodes=up(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)),
             lens=up(np.asarray(case["lens"], np.int32)), motion=up(case.get("motion")), pose2d=up(case.get("pose2d")),
             t0=up(case.get("t0")), pivot=up(case.get("pivot")))
    return d


def _field_buffer(case):
    """(host (F, stride) uint8 with four guard bytes behind every field, stride)."""
    s = case["spec"]
    cells = s["width"] * s["height"]
    stride = ((cells + 3) & ~3) + 4
    f = np.asarray(case["fields"], np.int8)
    host = np.full((len(f), stride), GUARD, np.uint8)
    host[:, :cells] = f.reshape(len(f), cells).view(np.uint8)
    return host, stride


def _run(gpu, case, p=None, status=True, d_field=None, field_stride=None, pad=PAD):
    """-> (volumes (G, volume) uint32, best (G, 8) uint32, status (G,), guard words (G, pad)).  status False: NULL
    goes in for d_status and the buffer comes back as it was filled (99).  d_field: a device field to use instead
    of the case's (the chain test); otherwise the field is uploaded with guards and checked to be unchanged."""
    import torch
    dev = torch.device("cuda:0")
    s = case["spec"]
    B, n = case["batch"].shape
    G = len(mc.case_groups(case))
    volume = mo.volume_size(s)
    stride = volume + pad
    d = _upload(case)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    host_field = None
    if d_field is None:
        host_field, field_stride = _field_buffer(case)
        d_field_t = torch.from_numpy(host_field.reshape(-1)).to(dev)
        d_field = d_field_t.data_ptr()
    per_group = 1 if len(case["fields"]) > 1 else 0
    d_scores = torch.full((G * stride,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_best = torch.full((G * 8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_st = torch.full((G,), 99, dtype=torch.int32, device=dev)
    gpu.set_scan_time_offsets_dev(ptr(d["t0"]))
    try:
        gpu.match_scans_dev(d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, case["group"], p or case["p"],
                            ptr(d["motion"]), ptr(d["pose2d"]), ptr(d["pivot"]), _struct(s), d_field, field_stride,
                            per_group, d_scores.data_ptr(), stride, d_best.data_ptr(), d_st.data_ptr() if status else 0)
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    if host_field is not None:
        assert d_field_t.cpu().numpy().tobytes() == host_field.tobytes()  # the field is only read
    raw = d_scores.cpu().numpy().view(np.uint32).reshape(G, stride)
    return (raw[:, :volume], d_best.cpu().numpy().view(np.uint32).reshape(G, 8), d_st.cpu().numpy().astype(np.int64),
            raw[:, volume:])


def _check(got, want, has_status=True):
    vols, best, status, guard = got
    assert len(vols) == len(want)
    if not has_status:
        assert (status == 99).all()
    for g, (wv, wb, ws) in enumerate(want):
        diff = np.flatnonzero(vols[g] != wv.reshape(-1))
        print(f"group {g}: best {best[g].view(np.int32).tolist()} want {wb.tolist()}, status {status[g]} want {ws}, "
              f"{len(diff)} of {wv.size} scores differ")
        assert len(diff) == 0, (g, diff[:8], vols[g][diff[:8]], wv.reshape(-1)[diff[:8]])
        assert best[g].tobytes() == mo.best_words(wb).tobytes(), (g, best[g], wb)
        assert not has_status or status[g] == ws, g
    assert (guard == GUARD_WORD).all()


# ---- recovery, chain, door ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disp", mc.ROOM_DISPLACEMENTS, ids=[str(d) for d in mc.ROOM_DISPLACEMENTS])
def test_recovery(gpu, oracle, disp):
    case = mc.room_case(oracle, disp)
    want = mc.case_want(oracle, case, f"room{disp}")
    mc.room_regime(oracle, case)
    got = _run(gpu, case)
    _check(got, want)
    k0, j0, i0 = disp
    assert got[1][0].view(np.int32)[1:4].tolist() == [-k0, -j0, -i0] and got[1][0][6] == 1


def test_chain_on_the_device(gpu, oracle):
    """E11 -> E12 -> E13 with no host copy between them: the grid E11 wrote from the true poses, inflated by E12
    with the hand-made table, is the field the displaced scans are matched to."""
    import torch
    dev = torch.device("cuda:0")
    disp = mc.ROOM_DISPLACEMENTS[1]
    case = mc.room_case(oracle, disp)
    batch, lens, pose2d = mc.room_scans()
    B, n = batch.shape
    o = mc.room_occ_spec()
    W, H = o["width"], o["height"]
    stride = W * H
    d_nodes = torch.from_numpy(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    d_pose = torch.from_numpy(pose2d).to(dev)
    d_grid = torch.full((stride,), GUARD, dtype=torch.uint8, device=dev)
    d_field = torch.full((stride,), GUARD, dtype=torch.uint8, device=dev)
    d_table = torch.from_numpy(mc.ROOM_TABLE).to(dev)
    grid = abi.OccGrid(o["origin_x"], o["origin_y"], o["resolution"], W, H, o["range_min"], o["obstacle_max"],
                       o["raytrace_max"])
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, B, Params.defaults(**mc.ROOM_P), 0,
                           d_pose.data_ptr(), grid, 0, d_grid.data_ptr(), stride)
    gpu.inflate_grids_dev(d_grid.data_ptr(), stride, d_field.data_ptr(), stride, 1, W, H, d_table.data_ptr(),
                          mc.ROOM_RC, 1)
    got = _run(gpu, case, d_field=d_field.data_ptr(), field_stride=stride)
    _check(got, mc.case_want(oracle, case, f"room{disp}"))
    assert d_field.cpu().numpy().view(np.int8).tobytes() == mc.room_field(oracle).tobytes()


def test_host_buffers_one_group(gpu, oracle):
    disp = mc.ROOM_DISPLACEMENTS[2]
    case = mc.room_case(oracle, disp)
    vol, best, status = mc.case_want(oracle, case, f"room{disp}")[0]
    dev_vols, dev_best, dev_status, _ = _run(gpu, case)
    scores, words, st = gpu.match_scans(case["batch"], case["lens"], case["p"], _struct(case["spec"]),
                                        case["fields"][0], pose2d=case["pose2d"], pivot=case["pivot"][0])
    assert scores.tobytes() == vol.tobytes() == dev_vols[0].tobytes() and scores.shape == vol.shape
    assert words.tobytes() == mo.best_words(best).tobytes() == dev_best[0].tobytes() and st == status == dev_status[0]
    none, words2, _ = gpu.match_scans(case["batch"], case["lens"], case["p"], _struct(case["spec"]),
                                      case["fields"][0], pose2d=case["pose2d"], pivot=case["pivot"][0],
                                      want_scores=False)
    assert none is None and words2.tobytes() == words.tobytes()


# ---- ties, edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.tie_cases()))
def test_ties(gpu, oracle, name):
    case, expect, equals = mc.tie_cases()[name]
    mc.tie_regime(oracle, name, case, expect, equals)
    got = _run(gpu, case)
    _check(got, mc.case_want(oracle, case, f"tie_{name}"))
    assert tuple(got[1][0].view(np.int32)[:4].tolist()) == expect


@pytest.mark.parametrize("name", sorted(mc.edge_cases()))
def test_window_edges(gpu, oracle, name):
    case = mc.edge_cases()[name]
    mc.edge_regime(oracle, name, case)
    _check(_run(gpu, case), mc.case_want(oracle, case, f"edge_{name}"))


# ---- passes, weights, groups -------------------------------------------------------------------------------------------------
def test_passes(gpu, oracle):
    case = mc.passes_case()
    mc.passes_regime(oracle, case)
    _check(_run(gpu, case), mc.case_want(oracle, case, "passes"))


def test_weights_from_many_workgroups(gpu, oracle):
    case = mc.weights_case()
    mc.weights_regime(oracle, case)
    _check(_run(gpu, case), mc.case_want(oracle, case, "weights"))


@pytest.mark.parametrize("per_group", [0, 1])
def test_groups(gpu, oracle, per_group):
    case = mc.groups_case(per_group)
    want = mc.groups_regime(oracle, case, f"groups{per_group}")
    _check(_run(gpu, case, pad=PAD + 64 * per_group), want)
    if per_group:
        _check(_run(gpu, case, status=False), want, has_status=False)  # d_status left out


# ---- the front end ------------------------------------------------------------------------------------------------------------
def test_full_front_end(gpu, oracle):
    case = mc.front_case()
    want = mc.front_regime(oracle, case)
    _check(_run(gpu, case), want)


def test_ieee_divide_instance(gpu, oracle):
    """A handle whose fast divides are refused (as tests/test_gpu_ieee_div.py arranges): the same bytes."""
    import torch

    from tests.conftest import _shared_stream
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    case = mc.front_case()
    want = mc.case_want(oracle, case, "front")
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
    assert fast[0].tobytes() == got[0].tobytes() and fast[1].tobytes() == got[1].tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_outputs_and_a_working_handle(gpu, oracle):
    import torch
    dev = torch.device("cuda:0")
    name = "w61"
    case = mc.edge_cases()[name]
    s = case["spec"]
    B, n = case["batch"].shape
    cells = s["width"] * s["height"]
    volume = mo.volume_size(s)
    d = _upload(case)
    host_field, fstride = _field_buffer(case)
    d_field = torch.from_numpy(host_field.reshape(-1)).to(dev)
    d_scores = torch.full((volume + PAD,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_best = torch.full((8,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_t0 = torch.zeros(B, dtype=torch.float32, device=dev)
    host = np.zeros(volume + 8, np.uint32)
    d_st = torch.full((2,), 99, dtype=torch.int32, device=dev)
    lib = abi.load_library()

    def call(**kw):
        a = dict(nodes=d["nodes"].data_ptr(), n=n, B=B, group=1, match=_struct(s), field=d_field.data_ptr(),
                 fstride=fstride, scores=d_scores.data_ptr(), sstride=volume + PAD, best=d_best.data_ptr(), p=case["p"],
                 motion=0, pivot=d["pivot"].data_ptr(), status=0)
        a.update(kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.match_scans_dev(a["nodes"], a["n"], d["lens"].data_ptr(), a["B"], a["group"], a["p"], a["motion"],
                                d["pose2d"].data_ptr(), a["pivot"], a["match"], a["field"], a["fstride"], 0,
                                a["scores"], a["sstride"], a["best"], a["status"])
        return e.value.code

    def raw(p_ref, m_ref):
        """The C entry point with a NULL p or m (the binding always passes a struct)."""
        return lib.rplgpu_match_scans_dev(gpu._h, d["nodes"].data_ptr(), n, d["lens"].data_ptr(), B, 1, p_ref, 0,
                                          d["pose2d"].data_ptr(), d["pivot"].data_ptr(), m_ref, d_field.data_ptr(),
                                          fstride, 0, d_scores.data_ptr(), volume + PAD, d_best.data_ptr(), 0)

    bad = abi.ERR_INVALID_ARG
    for kw in (dict(resolution=0.0), dict(width=0), dict(height=4097), dict(shift_x=33), dict(shift_y=33),
               dict(rot_steps=65), dict(rot_steps=2, rot_step=0.0), dict(rot_steps=2, rot_step=1.0),
               dict(origin_x=float("nan"))):
        assert call(match=_struct(dict(s, **kw))) == bad, kw
    assert call(fstride=cells - 4) == bad          # below width * height
    assert call(fstride=fstride + 2) == bad        # not a multiple of 4
    assert call(field=d_field.data_ptr() + 1) == bad
    assert call(field=0) == bad
    assert call(scores=0) == bad
    assert call(best=0) == bad
    assert call(scores=d_scores.data_ptr() + 2) == bad
    assert call(best=d_best.data_ptr() + 1) == bad
    assert call(scores=host.ctypes.data) == bad    # plain host memory, pointer by pointer
    assert call(best=host.ctypes.data) == bad
    assert call(field=host.ctypes.data) == bad
    assert call(pivot=host.ctypes.data) == bad
    assert call(status=host.ctypes.data) == bad
    assert call(motion=host.ctypes.data) == bad
    assert call(status=d_st.data_ptr() + 2) == bad  # a misaligned d_status
    assert raw(None, C.byref(_struct(s))) == bad and raw(C.byref(case["p"]), None) == bad
    assert call(sstride=volume - 1) == bad
    assert call(group=0) == bad
    assert call(nodes=0) == bad
    assert call(n=0) == bad
    assert call(B=gpu.max_batch + 1) == abi.ERR_CAPACITY
    ror_bad = Params.defaults(clip_enable=0, ror_enable=1, ror_radius=0.0)
    assert call(p=ror_bad) == bad
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        assert call() == bad  # offsets set, d_motion NULL
    finally:
        gpu.set_scan_time_offsets_dev(0)
    # group x n_stride above 2^24: 513 scans claimed at a stride of 32768 (refused before anything is read)
    assert call(n=32768, B=513, group=513) == bad
    gpu.synchronize()
    assert (d_scores.cpu().numpy().view(np.uint32) == GUARD_WORD).all()
    assert (d_best.cpu().numpy().view(np.uint32) == GUARD_WORD).all() and (d_st.cpu().numpy() == 99).all()
    assert d_field.cpu().numpy().tobytes() == host_field.tobytes()
    _check(_run(gpu, case), mc.case_want(oracle, case, f"edge_{name}"))  # the handle still works
