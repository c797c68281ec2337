"""E26 on the device: rplgpu_nav_field_dev and rplgpu_nav_paths_dev against tests/nav_oracle.py byte for byte once a
field is finished — the field, result words 0 - 5, the guard words behind every grid's field, behind the scratch and
the result, the grid only read — resumed calls, the chain behind E11 and E12, the host-buffer door, and every refusal.
The inputs and their regime checks live in tests/nav_cases.py; no grid is larger than 257 x 203."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import nav_cases as nc
from tests import nav_oracle as no

pytestmark = pytest.mark.gpu
GUARD = 0x5A
GUARD_WORD = 0x5A5A5A5A
U = no.UNREACHED


class _Field:
    """G grids of one spec on the device, every output filled with guard words; run() is one call."""

    def __init__(self, cases, grid_pad=4, pot_pad=3, goal_pad=2, spec=None):
        import torch
        dev = torch.device("cuda:0")
        self.cases, self.G = cases, len(cases)
        self.s = dict(spec or cases[0]["spec"])
        self.W, self.H = self.s["width"], self.s["height"]
        self.cells = self.W * self.H
        self.grid_stride = ((self.cells + 3) & ~3) + grid_pad
        self.pot_stride = self.cells + pot_pad
        self.goal_stride = max(max(len(c["goals"]) for c in cases), 1) + goal_pad
        self.host_grid = np.full((self.G, self.grid_stride), GUARD, np.uint8)
        goals = np.full((self.G, self.goal_stride), 7, np.uint32)  # (7: a cell, were a word beyond the count read)
        for g, c in enumerate(cases):
            self.host_grid[g, :self.cells] = c["grid"].reshape(-1).view(np.uint8)
            goals[g, :len(c["goals"])] = c["goals"]
        self.d_grid = torch.from_numpy(self.host_grid.reshape(-1)).to(dev)
        self.d_goals = torch.from_numpy(goals.reshape(-1).view(np.int32)).to(dev)
        self.d_n = torch.tensor([len(c["goals"]) for c in cases], dtype=torch.int32, device=dev)
        full = lambda n: torch.full((n,), GUARD_WORD, dtype=torch.int32, device=dev)  # noqa: E731
        self.scratch_words = abi.nav_field_scratch_words(no.struct_of(self.s), self.G)
        self.d_pot, self.d_scr, self.d_res = full(self.G * self.pot_stride), full(self.scratch_words + 8), full(8 * self.G + 8)

    def run(self, gpu, resume=0, rounds=None):
        """-> (fields (G, H, W) uint32, result (G, 8)); the guards and the grid are checked."""
        s = dict(self.s, rounds=rounds or self.s["rounds"])
        gpu.nav_field_dev(no.struct_of(s), self.d_grid.data_ptr(), self.grid_stride, self.G, self.d_goals.data_ptr(),
                          self.goal_stride, self.d_n.data_ptr(), self.d_pot.data_ptr(), self.pot_stride,
                          self.d_scr.data_ptr(), resume, self.d_res.data_ptr())
        gpu.synchronize()
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        pot, scr, res = u32(self.d_pot).reshape(self.G, self.pot_stride), u32(self.d_scr), u32(self.d_res)
        assert (pot[:, self.cells:] == GUARD_WORD).all() and (scr[self.scratch_words:] == GUARD_WORD).all()
        assert (res[8 * self.G:] == GUARD_WORD).all()
        assert self.d_grid.cpu().numpy().tobytes() == self.host_grid.tobytes()  # the grid is only read
        return pot[:, :self.cells].reshape(self.G, self.H, self.W).copy(), res[:8 * self.G].reshape(self.G, 8).copy()


def _finish(gpu, f, calls=40):
    """Calls until every grid reports no dirty tile (a bounded number of resumed calls, each of the spec's rounds)."""
    pot, res = f.run(gpu)
    for _ in range(calls):
        if not res[:, 0].any():
            break
        pot, res = f.run(gpu, resume=1)
    return pot, res


def _check(got, cases, wants=None):
    pot, res = got
    for g, c in enumerate(cases):
        want = nc.want(c) if wants is None else wants[g]
        diff = np.argwhere(pot[g] != want)
        print(f"{c['name']}: result {res[g].tolist()}, {len(diff)} cells differ")
        assert res[g, 0] == 0 and res[g, 1] == 0, (c["name"], res[g])
        assert len(diff) == 0, (c["name"], diff[:8], pot[g][tuple(diff[:8].T)], want[tuple(diff[:8].T)])
        assert res[g, 2:6].tolist() == no.result_words(want, c["goals"]), (c["name"], res[g])


def _field(gpu, c, **kw):
    got = _finish(gpu, _Field([c], **kw))
    _check(got, [c])
    return got


# ---- the field ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", nc.SIZES)
def test_sizes(gpu, W, H):
    nc.sizes_regime()
    _field(gpu, nc.size_case(W, H))


@pytest.mark.parametrize("name", ["corners", "wall", "double", "outside", "only_outside", "none", "many"])
def test_goals(gpu, name):
    nc.goals_regime()
    _field(gpu, nc.goal_cases()[name])


@pytest.mark.parametrize("name", ["row", "row_west", "col", "door", "wall", "corner"])
def test_goal_that_only_its_neighbour_tiles_can_use(gpu, name):
    """The goal's own tile changes nothing, so the tiles across its border run only because the goal was placed."""
    nc.border_goals_regime()
    _field(gpu, nc.border_goal_cases()[name])


def test_doors_at_tile_corners(gpu):
    nc.doors_regime()
    _field(gpu, nc.doors_case())


@pytest.mark.parametrize("blocked", ["", "x", "y", "xy"])
def test_corner_rule_across_a_tile_corner(gpu, blocked):
    nc.corner_regime()
    pot, _ = _field(gpu, nc.corner_case(blocked))
    assert pot[0][63, 63] == {"": 350, "x": 500, "y": 500}.get(blocked, pot[0][63, 63])


@pytest.mark.parametrize("name", ["unknown_shut", "unknown_open", "lethal100", "factor0", "dear"])
def test_costs(gpu, name):
    nc.costs_regime()
    _field(gpu, nc.cost_cases()[name])


@pytest.mark.parametrize("last_x", [40, 63, 64])
def test_cap_on_and_off_a_tile_border(gpu, last_x):
    nc.cap_regime()
    _field(gpu, nc.cap_case(last_x))


def test_cap_over_random_walls(gpu):
    _field(gpu, nc.cap_regime())


def test_serpentine(gpu):
    """Corridors that cross the tile borders every four rows: the number of rounds depends on the schedule, the
    answer does not."""
    nc.serpentine_regime()
    c = nc.serpentine_case()
    pot, res = _finish(gpu, _Field([c]), calls=60)
    _check((pot, res), [c])


def test_corridor_unfinished_resumed_finished(gpu):
    """3 x 330, six tiles, the goal in tile 0: a tile at tile distance >= r from every goal cannot have run within r
    rounds, on any schedule."""
    nc.corridor_regime()
    c = nc.corridor_case(2)
    want = nc.want(c)
    f = _Field([c])
    pot, res = f.run(gpu)  # two rounds
    print("after 2 rounds:", res[0].tolist())
    assert res[0, 0] > 0 and res[0, 1] == abi.NAV_UNFINISHED
    assert (pot[0][:, 2 * 64:] == U).all()  # tiles 2 - 5
    assert ((pot[0] == U) | (pot[0] >= want)).all()
    pot, res = f.run(gpu, resume=1)  # two more
    print("after 4 rounds:", res[0].tolist())
    assert res[0, 0] > 0 and res[0, 1] == abi.NAV_UNFINISHED and (pot[0][:, 4 * 64:] == U).all()
    assert ((pot[0] == U) | (pot[0] >= want)).all()
    pot, res = f.run(gpu, resume=1, rounds=8)
    print("after 12 rounds:", res[0].tolist())
    _check((pot, res), [c])
    again, res2 = f.run(gpu, resume=1, rounds=8)  # a finished field resumed
    assert again.tobytes() == pot.tobytes() and res2[0, 0] == 0 and res2[0, 6] == 0 and res2[0, 7] == 0
    assert res2[0, 2:6].tolist() == res[0, 2:6].tolist()


def test_three_grids_padded_strides(gpu):
    nc.batch_regime()
    cs = nc.batch_cases()
    _check(_finish(gpu, _Field(cs, grid_pad=8, pot_pad=5, goal_pad=3)), cs)
    _check(_finish(gpu, _Field(cs, grid_pad=0, pot_pad=0, goal_pad=0)), cs)


# ---- paths ---------------------------------------------------------------------------------------------------------------------
def _paths(gpu, c, field, starts, max_len, fill=GUARD_WORD):
    """-> (paths (S, max_len), info (S, 4)) of one grid down `field` (H, W) uint32."""
    import torch
    dev = torch.device("cuda:0")
    s = c["spec"]
    W, H = s["width"], s["height"]
    stride = (W * H + 3) & ~3
    host = np.full(stride, GUARD, np.uint8)
    host[:W * H] = c["grid"].reshape(-1).view(np.uint8)
    d_grid = torch.from_numpy(host).to(dev)
    d_pot = torch.from_numpy(np.ascontiguousarray(field).reshape(-1).view(np.int32)).to(dev)
    d_starts = torch.from_numpy(np.asarray(starts, np.uint32).view(np.int32)).to(dev)
    S = len(starts)
    d_paths = torch.full((S * max_len + 4,), fill, dtype=torch.int32, device=dev)
    d_info = torch.full((4 * S + 4,), fill, dtype=torch.int32, device=dev)
    gpu.nav_paths_dev(no.struct_of(s), d_grid.data_ptr(), stride, d_pot.data_ptr(), W * H, 1, d_starts.data_ptr(), S,
                      d_paths.data_ptr(), max_len, d_info.data_ptr())
    gpu.synchronize()
    paths, info = d_paths.cpu().numpy().view(np.uint32), d_info.cpu().numpy().view(np.uint32)
    assert (paths[S * max_len:] == fill).all() and (info[4 * S:] == fill).all()
    assert d_pot.cpu().numpy().view(np.uint32).tobytes() == np.ascontiguousarray(field).tobytes()
    return paths[:S * max_len].reshape(S, max_len), info[:4 * S].reshape(S, 4)


def _check_paths(c, field, starts, max_len, got):
    paths, info = got
    seen = 0
    for i, st in enumerate(starts):
        cells, winfo = no.path(c["grid"], field, c["spec"], st, max_len)
        assert info[i].tolist() == winfo, (i, st, info[i], winfo)
        assert paths[i, :len(cells)].tolist() == cells and (paths[i, len(cells):] == GUARD_WORD).all(), (i, st)
        seen |= winfo[1]
    return seen


@pytest.mark.parametrize("S", [1, 300])
def test_paths(gpu, S):
    c = nc.cost_cases()["unknown_open"]
    field = nc.want(c)
    starts = nc.path_starts(c, S)
    got = _paths(gpu, c, field, starts, 400)
    seen = _check_paths(c, field, starts, 400, got)
    assert seen & no.REACHED
    if S > 1:
        assert seen & no.NO_START and seen & no.PATH_UNREACHED and got[1][0].tolist() == [1, no.REACHED, 0, starts[0]]


def test_paths_truncated_and_broken(gpu):
    c = nc.doors_case()
    field = nc.want(c)
    start = 100 * 130 + 100
    cells, info = no.path(c["grid"], field, c["spec"], start, 10000)
    assert info[1] == no.REACHED and len(cells) > 100
    for max_len in (1, len(cells) - 1, len(cells)):
        got = _paths(gpu, c, field, [start, 5 * 130 + 5], max_len)
        seen = _check_paths(c, field, [start, 5 * 130 + 5], max_len, got)
        assert bool(seen & no.TRUNCATED) == (max_len < len(cells))
    # the potential of another grid: the walk stops where no neighbour satisfies the equality, and it ends
    other = nc.want(nc.corner_case(""))
    starts = [start, 20 * 130 + 100, 63 * 130 + 63]
    got = _paths(gpu, c, other, starts, 400)
    assert _check_paths(c, other, starts, 400, got) & no.BROKEN


def test_long_path_down_the_serpentine(gpu):
    c = nc.serpentine_case()
    field = nc.want(c)
    start = int(np.argmax(np.where(field == U, 0, field)))
    cells, info = no.path(c["grid"], field, c["spec"], start, 8000)
    assert info[1] == no.REACHED and len(cells) > 3000 and no.path_cost(c["grid"], c["spec"], cells) == info[2]
    _check_paths(c, field, [start], 8000, _paths(gpu, c, field, [start], 8000))


# ---- the chain, the door, the refusals -----------------------------------------------------------------------------------------
def test_chain_behind_e11_and_e12(gpu, oracle):
    """257 x 203, two groups: rplgpu_occupancy_grid_dev -> rplgpu_inflate_grids_dev -> rplgpu_nav_field_dev ->
    rplgpu_nav_paths_dev queued on one stream, each reading the buffer the one before wrote, ONE synchronise behind the
    last; the oracles chained the same way."""
    import torch

    from tests import inflate_cases as ic
    from tests import inflate_oracle as io
    from tests import occ_cases as oc
    from tests.test_gpu_occ import _struct
    dev = torch.device("cuda:0")
    case = oc.edges_case()
    occ_want = [w[0] for w in oc.case_want(oracle, case, "edges")]
    G = len(occ_want)
    H, W = occ_want[0].shape
    assert G == 2 and case.get("motion") is None and case.get("t0") is None
    table = ic.lib_table(4)
    cost_want = [io.inflate(g, table, 4, 0)[0] for g in occ_want]
    s = no.spec(width=W, height=H, unknown_cost=120, rounds=100)
    sensor = (int((0.0 - case["spec"]["origin_x"]) / 0.1), int((0.0 - case["spec"]["origin_y"]) / 0.1))
    goals = [sensor[1] * W + sensor[0]]
    field_want = [no.field_heap(cw, goals, s) for cw in cost_want]
    assert all((fw != U).sum() > 5000 and (fw == U).any() for fw in field_want)
    stride = (W * H + 3) & ~3
    batch = case["batch"]
    B, n = batch.shape
    d_nodes = torch.from_numpy(np.ascontiguousarray(batch).view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.from_numpy(np.asarray(case["lens"], np.int32)).to(dev)
    d_po = torch.from_numpy(np.ascontiguousarray(case["pose2d"])).to(dev)
    d_occ = torch.full((G * stride,), GUARD, dtype=torch.int8, device=dev)
    d_cost = torch.full((G * stride,), GUARD, dtype=torch.int8, device=dev)
    d_table = torch.from_numpy(table).to(dev)
    d_goals = torch.tensor(goals * G, dtype=torch.int32, device=dev)
    d_n = torch.ones(G, dtype=torch.int32, device=dev)
    d_pot = torch.full((G * W * H,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(abi.nav_field_scratch_words(no.struct_of(s), G), dtype=torch.int32, device=dev)
    d_res = torch.zeros(8 * G, dtype=torch.int32, device=dev)
    starts = [[(H - 3) * W + 5, 3 * W + W // 2, goals[0]], [100 * W + 200, 0, W * H]]
    max_len = 600
    d_starts = torch.tensor(sum(starts, []), dtype=torch.int32, device=dev)
    d_paths = torch.full((G * 3 * max_len,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_info = torch.zeros(G * 3 * 4, dtype=torch.int32, device=dev)
    spec = no.struct_of(s)
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, case["group"], case["p"], 0, d_po.data_ptr(),
                           _struct(case["spec"]), 0, d_occ.data_ptr(), stride, 0, 0)
    gpu.inflate_grids_dev(d_occ.data_ptr(), stride, d_cost.data_ptr(), stride, G, W, H, d_table.data_ptr(), 4, 0, 0)
    gpu.nav_field_dev(spec, d_cost.data_ptr(), stride, G, d_goals.data_ptr(), 1, d_n.data_ptr(), d_pot.data_ptr(),
                      W * H, d_scr.data_ptr(), 0, d_res.data_ptr())
    gpu.nav_paths_dev(spec, d_cost.data_ptr(), stride, d_pot.data_ptr(), W * H, G, d_starts.data_ptr(), 3,
                      d_paths.data_ptr(), max_len, d_info.data_ptr())
    gpu.synchronize()
    occ = d_occ.cpu().numpy().reshape(G, stride)[:, :W * H].reshape(G, H, W)
    cost = d_cost.cpu().numpy().reshape(G, stride)[:, :W * H].reshape(G, H, W)
    pot = d_pot.cpu().numpy().view(np.uint32).reshape(G, H, W)
    res = d_res.cpu().numpy().view(np.uint32).reshape(G, 8)
    paths = d_paths.cpu().numpy().view(np.uint32).reshape(G, 3, max_len)
    info = d_info.cpu().numpy().view(np.uint32).reshape(G, 3, 4)
    print("result", res.tolist())
    for g in range(G):
        assert occ[g].tobytes() == occ_want[g].tobytes()
        assert cost[g].tobytes() == cost_want[g].tobytes()
        assert res[g, 0] == 0 and pot[g].tobytes() == field_want[g].tobytes()
        assert res[g, 2:6].tolist() == no.result_words(field_want[g], goals)
        c = dict(grid=cost_want[g], spec=s)
        _check_paths(c, field_want[g], starts[g], max_len, (paths[g], info[g]))


def test_host_buffers(gpu):
    c = nc.doors_case()
    spec = no.struct_of(dict(c["spec"], rounds=3))  # (the door resumes until the field is finished)
    pot, res = gpu.nav_field(spec, c["grid"], c["goals"])
    want = nc.want(c)
    assert pot.tobytes() == want.tobytes() and res[0] == 0 and res[1] == 0
    assert res[2:6].tolist() == no.result_words(want, c["goals"]) and res[6] >= 4 and res[7] > 3
    starts = [100 * 130 + 100, 130 * 130, 64 * 130 + 64]
    pot, res, paths, info = gpu.nav_field(spec, c["grid"], c["goals"], starts=starts, max_len=500, path_fill=GUARD_WORD)
    assert pot.tobytes() == want.tobytes()
    _check_paths(c, want, starts, 500, (paths, info))
    empty = nc.goal_cases()["none"]
    pot, res = gpu.nav_field(no.struct_of(empty["spec"]), empty["grid"], [])
    assert (pot == U).all() and res.tolist()[:6] == [0, 0, 0, 0, 0, 0]
    with pytest.raises(abi.RplGpuError) as e:
        gpu.nav_field(no.struct_of(dict(c["spec"], lethal=101)), c["grid"], c["goals"])
    assert e.value.code == abi.ERR_INVALID_ARG


def test_refusals_leave_every_output(gpu):
    import torch
    dev = torch.device("cuda:0")
    c = nc.size_case(65, 65)
    f = _Field([c])
    host = np.zeros(64, np.uint32)
    S, max_len = 2, 8
    d_starts = torch.zeros(S, dtype=torch.int32, device=dev)
    d_paths = torch.full((S * max_len,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_info = torch.full((4 * S,), GUARD_WORD, dtype=torch.int32, device=dev)

    def field(**kw):
        a = dict(spec=dict(f.s), grid=f.d_grid.data_ptr(), gs=f.grid_stride, G=1, goals=f.d_goals.data_ptr(),
                 gos=f.goal_stride, n=f.d_n.data_ptr(), pot=f.d_pot.data_ptr(), ps=f.pot_stride,
                 scr=f.d_scr.data_ptr(), resume=0, res=f.d_res.data_ptr())
        spec_kw = {k: kw.pop(k) for k in list(kw) if k in f.s}
        a.update(kw)
        a["spec"].update(spec_kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.nav_field_dev(no.struct_of(a["spec"]), a["grid"], a["gs"], a["G"], a["goals"], a["gos"], a["n"],
                              a["pot"], a["ps"], a["scr"], a["resume"], a["res"])
        return e.value.code

    def paths(**kw):
        a = dict(spec=dict(f.s), grid=f.d_grid.data_ptr(), gs=f.grid_stride, pot=f.d_pot.data_ptr(), ps=f.pot_stride,
                 G=1, starts=d_starts.data_ptr(), S=S, paths=d_paths.data_ptr(), max_len=max_len,
                 info=d_info.data_ptr())
        spec_kw = {k: kw.pop(k) for k in list(kw) if k in f.s}
        a.update(kw)
        a["spec"].update(spec_kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.nav_paths_dev(no.struct_of(a["spec"]), a["grid"], a["gs"], a["pot"], a["ps"], a["G"], a["starts"],
                              a["S"], a["paths"], a["max_len"], a["info"])
        return e.value.code

    shared = [dict(width=0), dict(height=4097), dict(lethal=0), dict(lethal=101), dict(neutral=0), dict(neutral=256),
              dict(factor=17), dict(unknown_cost=2048), dict(cap=0xFFFF0001), dict(rounds=0), dict(rounds=4097),
              dict(G=0), dict(G=65536), dict(gs=f.cells - 1), dict(gs=f.grid_stride + 2), dict(ps=f.cells - 1),
              dict(grid=f.d_grid.data_ptr() + 1), dict(pot=f.d_pot.data_ptr() + 2), dict(grid=0), dict(pot=0),
              dict(pot=host.ctypes.data)]
    for kw in shared + [dict(goals=0), dict(n=0), dict(scr=0), dict(res=0), dict(resume=2), dict(gos=0),
                        dict(goals=f.d_goals.data_ptr() + 1), dict(n=f.d_n.data_ptr() + 2),
                        dict(scr=f.d_scr.data_ptr() + 1), dict(res=f.d_res.data_ptr() + 2),
                        dict(res=host.ctypes.data)]:
        assert field(**dict(kw)) == abi.ERR_INVALID_ARG, kw
    for kw in shared + [dict(starts=0), dict(paths=0), dict(info=0), dict(S=0), dict(S=65537), dict(max_len=0),
                        dict(starts=d_starts.data_ptr() + 1), dict(paths=d_paths.data_ptr() + 2),
                        dict(info=d_info.data_ptr() + 1), dict(info=host.ctypes.data)]:
        assert paths(**dict(kw)) == abi.ERR_INVALID_ARG, kw
    # G x tiles above RPLGPU_NAV_MAX_TILES: refused before anything is queued (no buffer of that size is needed)
    assert field(width=4096, height=4096, G=2049, gs=1 << 24, ps=1 << 24) == abi.ERR_CAPACITY
    gpu.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    for t in (f.d_pot, f.d_scr, f.d_res, d_paths, d_info):
        assert (u32(t) == GUARD_WORD).all()
    _check(_finish(gpu, f), [c])  # and the handle goes on working
