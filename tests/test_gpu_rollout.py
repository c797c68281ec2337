"""E27 on the device: rplgpu_rollout_dev against tests/rollout_oracle.py byte for byte — the candidates' eight words,
the end poses, the result words, guard words behind every output, behind the scratch and the result, every input
compared after the call — at the kernel's edges (tests/rollout_cases.py), the identity with E16's move, the chains
behind E11 -> E12 -> E26 and behind E18, the host-buffer door, and every refusal.  No grid is larger than 130 x 70 but
the chain's, which is E26's own chain case (257 x 203)."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import rollout_cases as rc
from tests import rollout_oracle as ro

pytestmark = pytest.mark.gpu
GUARD_WORD = 0x5A5A5A5A


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class _Call:
    """The groups of one call on the device (cases of one spec, K, F and delta mode), every output filled with guard
    words, strides padded; run() is one call, checked against the oracle."""

    def __init__(self, cases, share_start=False, share_delta=False, share_grid=False, pad=1, end_poses=True):
        import torch
        dev = torch.device("cuda:0")
        c0 = cases[0]
        self.cases, self.G = cases, len(cases)
        self.s, self.T = c0["spec"], c0["spec"]["steps"]
        self.K, self.F = len(c0["delta"]), len(c0["footprint"])
        self.per_step = 1 if c0["delta"].ndim == 3 else 0
        self.cells = self.s["width"] * self.s["height"]
        self.flags = (0 if share_start else 1, 0 if share_delta else 1, 0 if share_grid else 1)
        n_delta = self.K * (self.T if self.per_step else 1)
        self.delta_stride = 4 * n_delta + 4 * pad
        self.grid_stride = ((self.cells + 3) & ~3) + 4 * pad
        self.pot_stride = self.cells + 3 * pad
        self.out_stride = 8 * self.K + 4 * pad
        self.end_stride = 4 * self.K + 8 * pad
        self.has_pot = c0["potential"] is not None
        G = self.G
        start = np.stack([c["start"] for c in cases])
        delta = np.full((G, self.delta_stride), 1.0e9, np.float32)
        grid = np.full((G, self.grid_stride), 0x5A, np.uint8)
        pot = np.full((G, self.pot_stride), 1, np.uint32)
        for g, c in enumerate(cases):
            delta[g, :4 * n_delta] = c["delta"].reshape(-1)
            grid[g, :self.cells] = c["grid"].reshape(-1).view(np.uint8)
            if self.has_pot:
                pot[g, :self.cells] = c["potential"].reshape(-1)
        self.host_in = [start, delta, np.ascontiguousarray(c0["footprint"]), grid, pot]
        self.d_in = [torch.from_numpy(a.reshape(-1).view(np.int32 if a.dtype != np.uint8 else np.uint8)).to(dev)
                     for a in self.host_in]
        full = lambda n: torch.full((n,), GUARD_WORD, dtype=torch.int32, device=dev)  # noqa: E731
        self.scratch_words = abi.rollout_scratch_words(G, self.K)
        assert self.scratch_words == ro.scratch_words(G, self.K) > 0
        self.d_out, self.d_end = full(G * self.out_stride), full(G * self.end_stride) if end_poses else None
        self.d_res, self.d_scr = full(8 * G + 8), full(self.scratch_words + 8)

    def args(self, **kw):
        d = self.d_in
        a = dict(spec=dict(self.s), start=d[0].data_ptr(), spg=self.flags[0], delta=d[1].data_ptr(),
                 ds=self.delta_stride, dpg=self.flags[1], dps=self.per_step, fp=d[2].data_ptr(), F=self.F,
                 grid=d[3].data_ptr(), gs=self.grid_stride, pot=d[4].data_ptr() if self.has_pot else 0,
                 ps=self.pot_stride, gpg=self.flags[2], G=self.G, K=self.K, out=self.d_out.data_ptr(),
                 os=self.out_stride, end=self.d_end.data_ptr() if self.d_end is not None else 0, es=self.end_stride,
                 res=self.d_res.data_ptr(), scr=self.d_scr.data_ptr())
        spec_kw = {k: kw.pop(k) for k in list(kw) if k in self.s}
        a.update(kw)
        a["spec"].update(spec_kw)
        return a

    def call(self, gpu, **kw):
        a = self.args(**kw)
        gpu.rollout_dev(ro.struct_of(a["spec"]), a["start"], a["spg"], a["delta"], a["ds"], a["dpg"], a["dps"], a["fp"],
                        a["F"], a["grid"], a["gs"], a["pot"], a["ps"], a["gpg"], a["G"], a["K"], a["out"], a["os"],
                        a["end"], a["es"], a["res"], a["scr"])

    def outputs(self):
        """-> (out (G, K, 8), end poses (G, K, 4) as words or None, result (G, 8)); the guards and the inputs are
        checked."""
        G, K = self.G, self.K
        out, res, scr = _u32(self.d_out).reshape(G, self.out_stride), _u32(self.d_res), _u32(self.d_scr)
        assert (out[:, 8 * K:] == GUARD_WORD).all() and (res[8 * G:] == GUARD_WORD).all()
        assert (scr[self.scratch_words:] == GUARD_WORD).all()
        end = None
        if self.d_end is not None:
            end = _u32(self.d_end).reshape(G, self.end_stride)
            assert (end[:, 4 * K:] == GUARD_WORD).all()
            end = end[:, :4 * K].reshape(G, K, 4)
        for host, d in zip(self.host_in, self.d_in):
            assert d.cpu().numpy().tobytes() == host.tobytes()  # the inputs are only read
        return out[:, :8 * K].reshape(G, K, 8), end, res[:8 * G].reshape(G, 8)

    def untouched(self):
        tensors = [self.d_out, self.d_res, self.d_scr] + ([self.d_end] if self.d_end is not None else [])
        return all((_u32(t) == GUARD_WORD).all() for t in tensors)

    def run(self, gpu):
        self.call(gpu)
        gpu.synchronize()
        out, end, res = self.outputs()
        for g, c in enumerate(self.cases):
            w_out, w_end, w_res = rc.want(c)
            bad = np.argwhere((out[g] != w_out).any(axis=1)).reshape(-1)
            print(f"{c['name']}: result {res[g].tolist()}, {len(bad)} candidates differ")
            assert len(bad) == 0, (c["name"], bad[:6], out[g][bad[:6]], w_out[bad[:6]])
            if end is not None:
                assert end[g].tobytes() == w_end.tobytes(), c["name"]
            assert res[g].tolist() == w_res.tolist(), c["name"]
        return out, end, res


def _one(gpu, c, **kw):
    return _Call([c], **kw).run(gpu)


# ---- shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T,F,per_step", rc.SHAPES)
def test_shapes(gpu, K, T, F, per_step):
    rc.shapes_regime()
    _one(gpu, rc.shape_case(K, T, F, per_step))


def _mixed(cases, share_start, share_delta, share_grid):
    """What group g computes when the call shares group 0's start, deltas or costmap."""
    out = []
    for c in cases:
        m = dict(c, name=c["name"] + f"_mix{int(share_start)}{int(share_delta)}{int(share_grid)}")
        if share_start:
            m["start"] = cases[0]["start"]
        if share_delta:
            m["delta"] = cases[0]["delta"]
        if share_grid:
            m["grid"], m["potential"] = cases[0]["grid"], cases[0]["potential"]
        out.append(m)
    return out


@pytest.mark.parametrize("share", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
@pytest.mark.parametrize("per_step", [0, 1])
def test_three_groups_with_padded_strides(gpu, share, per_step):
    cases = _mixed(rc.group_cases(per_step=per_step), *share)
    assert len(cases) == 3
    _Call(cases, *[bool(v) for v in share], pad=3).run(gpu)


def test_without_end_poses_and_without_padding(gpu):
    _Call(rc.group_cases(), pad=0, end_poses=False).run(gpu)


# ---- blocking, D and the score, ties ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["at_step_1", "at_step_T", "last_point", "last_point_without", "edge_east",
                                  "edge_west", "edge_north", "edge_south", "nan_start", "inf_delta", "far_step",
                                  "unknown_below", "unknown_at", "lethal_1", "lethal_100", "min_steps"])
def test_blocking(gpu, name):
    rc.blocking_regime()
    _one(gpu, rc.blocking_cases()[name])


@pytest.mark.parametrize("name", ["d_min_middle", "end_unreached", "centre_outside", "centre_outside_short",
                                  "no_potential", "big_score"])
def test_field_and_score(gpu, name):
    rc.field_regime()
    _one(gpu, rc.field_cases()[name])


@pytest.mark.parametrize("name", ["lanes", "tiles", "waves"])
def test_ties(gpu, name):
    rc.tie_regime()
    _one(gpu, rc.tie_cases()[name])


def test_no_admissible_candidate(gpu):
    rc.none_regime()
    _one(gpu, rc.none_admissible_case())


# ---- the identity, the chains, the door --------------------------------------------------------------------------------------------
def test_identity_with_e16_move_on_the_device(gpu):
    """T = 5 arcs in a free grid: the end poses equal five chained rplgpu_resample_poses_dev moves (the first with
    P = 1, then K weights of 1 with u = 0, where output j descends from pose j)."""
    import torch
    dev = torch.device("cuda:0")
    rc.identity_regime()
    c = rc.identity_case()
    K, T = len(c["delta"]), c["spec"]["steps"]
    call = _Call([c])
    _, end, _ = call.run(gpu)
    d_w = torch.ones(K, dtype=torch.int32, device=dev)
    d_a = torch.from_numpy(c["start"].copy()).to(dev)
    d_b = torch.zeros(4 * K, dtype=torch.float32, device=dev)
    d_res = torch.zeros(8, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(abi.resample_scratch_words(1, K), dtype=torch.int32, device=dev)
    d_delta = call.d_in[1]
    P = 1
    for _ in range(T):
        gpu.resample_poses_dev(d_w.data_ptr(), K, d_a.data_ptr(), 4 * P, 1, 1, P, K, 0, d_delta.data_ptr(), K, 4 * K, 1,
                               d_b.data_ptr(), 4 * K, 0, 0, d_res.data_ptr(), d_scr.data_ptr())
        d_a, d_b, P = d_b, torch.zeros(4 * K, dtype=torch.float32, device=dev), K
    gpu.synchronize()
    assert d_a.cpu().numpy().tobytes() == end[0].tobytes()


def test_chain_behind_e11_e12_e26(gpu, oracle):
    """rplgpu_occupancy_grid_dev -> rplgpu_inflate_grids_dev -> rplgpu_nav_field_dev -> rplgpu_rollout_dev on one
    stream, each reading the buffer the one before wrote (the costmap AND the field), ONE synchronise behind the
    last; the oracles chained the same way.  Two groups, each with its own costmap and field."""
    import torch

    from tests import inflate_cases as ic
    from tests import inflate_oracle as io
    from tests import nav_oracle as no
    from tests import occ_cases as oc
    from tests.test_gpu_occ import _struct
    dev = torch.device("cuda:0")
    case = oc.edges_case()
    occ_want = [w[0] for w in oc.case_want(oracle, case, "edges")]
    G = len(occ_want)
    H, W = occ_want[0].shape
    table = ic.lib_table(4)
    cost_want = [io.inflate(g, table, 4, 0)[0] for g in occ_want]
    ns = no.spec(width=W, height=H, unknown_cost=120, rounds=100)
    ox, oy = case["spec"]["origin_x"], case["spec"]["origin_y"]
    sensor = (int((0.0 - ox) / 0.1), int((0.0 - oy) / 0.1))
    goals = [sensor[1] * W + sensor[0]]
    field_want = [no.field_heap(cw, goals, ns) for cw in cost_want]
    K, T = 2 * rc.TILE + 7, 24
    rng = np.random.default_rng(27)
    delta = rc.arc_deltas(rng.uniform(0.5, 6.0, K), rng.uniform(-2.0, 2.0, K), 1.0 / T)
    s = ro.spec(origin_x=ox, origin_y=oy, resolution=case["spec"]["resolution"], width=W, height=H, steps=T,
                min_steps=T // 2, unknown_value=40, a_end=1, a_min=1, a_sum=2, a_max=3)
    assert case["spec"]["resolution"] == np.float32(0.1) or abs(case["spec"]["resolution"] - 0.1) < 1e-6
    start = rc.pose(1.0, 0.5, 2.5)
    fp = rc.ring(6, 0.15)
    wants = [ro.sweep(s, start, delta, fp, cost_want[g], field_want[g]) for g in range(G)]
    assert all(w[2][0] > 0 for w in wants) and 0 < wants[0][2][5] < K, [w[2].tolist() for w in wants]
    assert wants[0][0].tobytes() != wants[1][0].tobytes()   # (the groups' maps differ where the candidates go)
    stride = (W * H + 3) & ~3
    batch = case["batch"]
    B, n = batch.shape
    d_nodes = torch.from_numpy(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.from_numpy(np.asarray(case["lens"], np.int32)).to(dev)
    d_po = torch.from_numpy(np.ascontiguousarray(case["pose2d"])).to(dev)
    d_occ = torch.full((G * stride,), 0x5A, dtype=torch.int8, device=dev)
    d_cost = torch.full((G * stride,), 0x5A, dtype=torch.int8, device=dev)
    d_table = torch.from_numpy(table).to(dev)
    d_goals = torch.tensor(goals * G, dtype=torch.int32, device=dev)
    d_n = torch.ones(G, dtype=torch.int32, device=dev)
    d_pot = torch.full((G * W * H,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_nscr = torch.zeros(abi.nav_field_scratch_words(no.struct_of(ns), G), dtype=torch.int32, device=dev)
    d_nres = torch.zeros(8 * G, dtype=torch.int32, device=dev)
    d_start = torch.from_numpy(start).to(dev)
    d_delta = torch.from_numpy(delta.reshape(-1)).to(dev)
    d_fp = torch.from_numpy(fp.reshape(-1)).to(dev)
    d_out = torch.full((G * 8 * K,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_end = torch.full((G * 4 * K,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((8 * G,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(abi.rollout_scratch_words(G, K), dtype=torch.int32, device=dev)
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, case["group"], case["p"], 0, d_po.data_ptr(),
                           _struct(case["spec"]), 0, d_occ.data_ptr(), stride, 0, 0)
    gpu.inflate_grids_dev(d_occ.data_ptr(), stride, d_cost.data_ptr(), stride, G, W, H, d_table.data_ptr(), 4, 0, 0)
    gpu.nav_field_dev(no.struct_of(ns), d_cost.data_ptr(), stride, G, d_goals.data_ptr(), 1, d_n.data_ptr(),
                      d_pot.data_ptr(), W * H, d_nscr.data_ptr(), 0, d_nres.data_ptr())
    gpu.rollout_dev(ro.struct_of(s), d_start.data_ptr(), 0, d_delta.data_ptr(), 4 * K, 0, 0, d_fp.data_ptr(), len(fp),
                    d_cost.data_ptr(), stride, d_pot.data_ptr(), W * H, 1, G, K, d_out.data_ptr(), 8 * K,
                    d_end.data_ptr(), 4 * K, d_res.data_ptr(), d_scr.data_ptr())
    gpu.synchronize()
    nres = _u32(d_nres).reshape(G, 8)
    out, end, res = _u32(d_out).reshape(G, K, 8), _u32(d_end).reshape(G, K, 4), _u32(d_res).reshape(G, 8)
    pot = _u32(d_pot).reshape(G, H, W)
    print("field", nres.tolist(), "rollout", res.tolist())
    for g in range(G):
        assert nres[g, 0] == 0 and pot[g].tobytes() == field_want[g].tobytes()
        assert out[g].tobytes() == wants[g][0].tobytes() and end[g].tobytes() == wants[g][1].tobytes()
        assert res[g].tolist() == wants[g][2].tolist()


def test_chain_behind_e18(gpu):
    """rplgpu_sample_motion_dev with M = K T writes the per-step deltas rplgpu_rollout_dev reads, both queued on
    one stream with one synchronise behind the last; the oracle rolls rplgpu_sample_motion_host's deltas."""
    import torch
    dev = torch.device("cuda:0")
    K, T, G = rc.TILE + 9, rc.CHUNK + 3, 2
    odom = abi.motion_odometry(0.2, 0.01, 0.03, np.array([0.2, 0.2, 0.1, 0.1]))
    noise = abi.MotionNoise.defaults()
    grid = rc.rough_grid(18)
    pot = rc.slope_field(grid)
    s = rc.base_spec(steps=T, min_steps=T // 2, a_end=1, a_sum=4)
    start, fp = rc.pose(*rc.centre_of(8, 33), 0.1), rc.ring(4, 0.2)
    wants = []
    for g in range(G):
        delta, _ = abi.sample_motion_host(odom, K * T, noise, group=g)
        wants.append(ro.sweep(s, start, delta.reshape(K, T, 4), fp, grid, pot))
    assert wants[0][0].tobytes() != wants[1][0].tobytes() and all(0 < w[2][5] < K for w in wants)
    d_odom = torch.from_numpy(odom).to(dev)
    d_delta = torch.zeros(G * 4 * K * T, dtype=torch.float32, device=dev)
    d_mres = torch.zeros(8 * G, dtype=torch.int32, device=dev)
    d_start, d_fp = torch.from_numpy(start).to(dev), torch.from_numpy(fp.reshape(-1)).to(dev)
    d_grid = torch.from_numpy(grid.reshape(-1)).to(dev)
    d_pot = torch.from_numpy(pot.reshape(-1).view(np.int32)).to(dev)
    d_out = torch.full((G * 8 * K,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_end = torch.full((G * 4 * K,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_res = torch.full((8 * G,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(abi.rollout_scratch_words(G, K), dtype=torch.int32, device=dev)
    gpu.sample_motion_dev(d_odom.data_ptr(), 0, G, K * T, noise, d_delta.data_ptr(), 4 * K * T, d_mres.data_ptr())
    gpu.rollout_dev(ro.struct_of(s), d_start.data_ptr(), 0, d_delta.data_ptr(), 4 * K * T, 1, 1, d_fp.data_ptr(),
                    len(fp), d_grid.data_ptr(), grid.size, d_pot.data_ptr(), grid.size, 0, G, K, d_out.data_ptr(),
                    8 * K, d_end.data_ptr(), 4 * K, d_res.data_ptr(), d_scr.data_ptr())
    gpu.synchronize()
    out, end, res = _u32(d_out).reshape(G, K, 8), _u32(d_end).reshape(G, K, 4), _u32(d_res).reshape(G, 8)
    print("rollout", res.tolist())
    for g in range(G):
        assert out[g].tobytes() == wants[g][0].tobytes() and end[g].tobytes() == wants[g][1].tobytes()
        assert res[g].tolist() == wants[g][2].tolist()


def test_host_buffers(gpu):
    for c in (rc.shape_case(*rc.SHAPES[4]), rc.field_cases()["no_potential"], rc.blocking_cases()["nan_start"]):
        got = gpu.rollout(ro.struct_of(c["spec"]), c["start"], c["delta"], c["footprint"], c["grid"], c["potential"])
        assert ro.equal(got, rc.want(c)), c["name"]
    c = rc.field_cases()["d_min_middle"]
    with pytest.raises(abi.RplGpuError) as e:
        gpu.rollout(ro.struct_of(dict(c["spec"], lethal=101)), c["start"], c["delta"], c["footprint"], c["grid"])
    assert e.value.code == abi.ERR_INVALID_ARG


def test_refusals_leave_every_output(gpu):
    cases = rc.group_cases(G=2)
    f = _Call(cases)
    host = np.zeros(4096, np.uint32)
    K, T = f.K, f.T

    def code(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            f.call(gpu, **kw)
        return e.value.code

    ptr = lambda t: t.data_ptr()  # noqa: E731
    refused = [dict(width=0), dict(height=4097), dict(lethal=0), dict(lethal=101), dict(unknown_value=101),
               dict(steps=0), dict(steps=257), dict(min_steps=0), dict(min_steps=T + 1), dict(a_end=65536),
               dict(a_max=65536), dict(resolution=0.0), dict(origin_x=float("nan")),
               dict(G=0), dict(G=65536), dict(K=0), dict(K=(1 << 20) + 1), dict(F=0), dict(F=65), dict(dps=2),
               dict(steps=256, min_steps=1, K=(1 << 16) + 1),
               dict(start=0), dict(delta=0), dict(fp=0), dict(grid=0), dict(out=0), dict(res=0), dict(scr=0),
               dict(start=ptr(f.d_in[0]) + 4), dict(delta=ptr(f.d_in[1]) + 8), dict(fp=ptr(f.d_in[2]) + 4),
               dict(grid=ptr(f.d_in[3]) + 1), dict(pot=ptr(f.d_in[4]) + 2), dict(out=ptr(f.d_out) + 8),
               dict(end=ptr(f.d_end) + 4), dict(res=ptr(f.d_res) + 2), dict(scr=ptr(f.d_scr) + 8),
               dict(ds=4 * K * T - 4), dict(ds=f.delta_stride + 2), dict(dps=0, ds=4 * K - 4),
               dict(gs=f.cells - 4), dict(gs=f.grid_stride + 2), dict(ps=f.cells - 1), dict(os=8 * K - 4),
               dict(os=f.out_stride + 2), dict(es=4 * K - 4), dict(es=f.end_stride + 2),
               # an output that overlaps an input or another output
               dict(out=ptr(f.d_in[1])), dict(end=ptr(f.d_in[1])), dict(res=ptr(f.d_in[0])), dict(scr=ptr(f.d_in[3])),
               dict(end=ptr(f.d_out) + 16), dict(res=ptr(f.d_scr)), dict(scr=ptr(f.d_out)),
               # host memory
               dict(out=host.ctypes.data), dict(grid=host.ctypes.data), dict(res=host.ctypes.data)]
    for kw in refused:
        assert code(**dict(kw)) == abi.ERR_INVALID_ARG, kw
    # G x tiles above RPLGPU_ROLLOUT_MAX_TILES: refused before anything is queued
    assert code(G=65535, K=4097, dps=0, ds=1 << 20, os=1 << 20, es=1 << 20) == abi.ERR_CAPACITY
    gpu.synchronize()
    assert f.untouched()
    f.run(gpu)  # and the handle goes on working
