"""E29 on the device: rplgpu_frontiers_dev against tests/frontier_oracle.py byte for byte — the result words, the
labels, the rows, the goal words, guard words behind every output, the scratch and the result, the grid and the field
only read — the identity with E26, the chain behind E14 and E12, the host-buffer door, and every refusal.  The inputs
and their regime checks live in tests/frontier_cases.py; no grid is larger than 256 x 256 but the two 4096 x 3 strips."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import frontier_cases as fc
from tests import frontier_oracle as fo

pytestmark = pytest.mark.gpu
GUARD = 0x5A
GUARD_WORD = 0x5A5A5A5A


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class _Front:
    """G grids of one spec on the device, every output filled with guard words; run() is one call."""

    def __init__(self, cases, grid_pad=4, pot_pad=3, label_pad=5, row_pad=3, goal_pad=2, labels=True, goal=True):
        import torch
        dev = torch.device("cuda:0")
        c0 = cases[0]
        self.cases, self.G = cases, len(cases)
        self.s, self.comp_cap, self.row_cap = dict(c0["spec"]), c0["comp_cap"], c0["row_cap"]
        self.W, self.H = self.s["width"], self.s["height"]
        self.cells = self.W * self.H
        self.has_pot = c0["potential"] is not None
        assert all((c["potential"] is not None) == self.has_pot and c["grid"].shape == (self.H, self.W) for c in cases)
        self.grid_stride = ((self.cells + 3) & ~3) + grid_pad
        self.pot_stride = self.cells + pot_pad
        self.label_stride = self.cells + label_pad
        self.row_stride = 8 * self.row_cap + row_pad
        self.goal_stride = 1 + goal_pad
        self.host_grid = np.full((self.G, self.grid_stride), GUARD, np.uint8)
        self.host_pot = np.full((self.G, self.pot_stride), 3, np.uint32)
        for g, c in enumerate(cases):
            self.host_grid[g, :self.cells] = c["grid"].reshape(-1).view(np.uint8)
            if self.has_pot:
                self.host_pot[g, :self.cells] = c["potential"].reshape(-1)
        self.d_grid = torch.from_numpy(self.host_grid.reshape(-1)).to(dev)
        self.d_pot = torch.from_numpy(self.host_pot.reshape(-1).view(np.int32)).to(dev) if self.has_pot else None
        full = lambda n: torch.full((n,), GUARD_WORD, dtype=torch.int32, device=dev)  # noqa: E731
        self.full = full
        self.scratch_words = abi.frontiers_scratch_words(fo.struct_of(self.s), self.G, self.comp_cap)
        assert self.scratch_words == fo.scratch_words(self.s, self.G, self.comp_cap) > 0
        self.d_lab = full(self.G * self.label_stride) if labels else None
        self.d_rows = full(self.G * self.row_stride + 1)
        self.d_goal = full(self.G * self.goal_stride) if goal else None
        self.d_n = full(self.G + 1) if goal else None
        self.d_scr, self.d_res = full(self.scratch_words + 8), full(16 * self.G + 8)

    def call(self, gpu, **kw):
        p = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        a = dict(spec=dict(self.s), grid=p(self.d_grid), gs=self.grid_stride, pot=p(self.d_pot), ps=self.pot_stride,
                 G=self.G, cap=self.comp_cap, lab=p(self.d_lab), ls=self.label_stride, rows=p(self.d_rows),
                 rs=self.row_stride, rc=self.row_cap, goal=p(self.d_goal), gos=self.goal_stride, n=p(self.d_n),
                 res=p(self.d_res), scr=p(self.d_scr))
        spec_kw = {k: kw.pop(k) for k in list(kw) if k in self.s}
        a.update(kw)
        a["spec"].update(spec_kw)
        gpu.frontiers_dev(fo.struct_of(a["spec"]), a["grid"], a["gs"], a["pot"], a["ps"], a["G"], a["cap"], a["lab"],
                          a["ls"], a["rows"], a["rs"], a["rc"], a["goal"], a["gos"], a["n"], a["res"], a["scr"])

    def run(self, gpu):
        """-> one dictionary per grid, as abi.frontiers_host's; the guards and the inputs are checked."""
        self.call(gpu)
        gpu.synchronize()
        scr, res = _u32(self.d_scr), _u32(self.d_res)
        assert (scr[self.scratch_words:] == GUARD_WORD).all() and (res[16 * self.G:] == GUARD_WORD).all()
        assert self.d_grid.cpu().numpy().tobytes() == self.host_grid.tobytes()  # the grid is only read
        if self.has_pot:
            assert _u32(self.d_pot).tobytes() == self.host_pot.tobytes()        # and so is the field
        rows = _u32(self.d_rows)
        assert rows[-1] == GUARD_WORD
        rows = rows[:-1].reshape(self.G, self.row_stride)
        assert (rows[:, 8 * self.row_cap:] == GUARD_WORD).all()
        out = [dict(result=res[16 * g:16 * g + 16].copy(), rows=rows[g, :8 * self.row_cap].reshape(-1, 8).copy(),
                    labels=None, goal=None, n_goal=None) for g in range(self.G)]
        if self.d_lab is not None:
            lab = _u32(self.d_lab).reshape(self.G, self.label_stride)
            assert (lab[:, self.cells:] == GUARD_WORD).all()  # words at and beyond width * height are never changed
            for g in range(self.G):
                out[g]["labels"] = lab[g, :self.cells].reshape(self.H, self.W).copy()
        if self.d_goal is not None:
            goal, n = _u32(self.d_goal).reshape(self.G, self.goal_stride), _u32(self.d_n)
            assert (goal[:, 1:] == GUARD_WORD).all() and n[self.G] == GUARD_WORD
            for g in range(self.G):
                out[g]["goal"], out[g]["n_goal"] = int(goal[g, 0]), int(n[g])
        return out


def _same(got, want, name):
    print(f"{name}: result {got['result'].tolist()}")
    assert got["result"].tolist() == want["result"].tolist(), (name, got["result"].tolist(), want["result"].tolist())
    if got["labels"] is not None:
        diff = np.argwhere(got["labels"] != want["labels"])
        assert len(diff) == 0, (name, len(diff), diff[:8], got["labels"][tuple(diff[:8].T)],
                                want["labels"][tuple(diff[:8].T)])
    assert got["rows"].tobytes() == want["rows"].tobytes(), (name, got["rows"][:4], want["rows"][:4])
    if got["goal"] is not None:
        assert got["n_goal"] == want["n_goal"], name
        assert got["goal"] == (GUARD_WORD if want["goal"] is None else want["goal"]), name


def _run(gpu, cases, **kw):
    cases = cases if isinstance(cases, list) else [cases]
    got = _Front(cases, **kw).run(gpu)
    for g, c in enumerate(cases):
        _same(got[g], fc.want(c), c["name"])
    return got


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", fc.SIZES)
def test_sizes(gpu, W, H):
    """Every byte class (-128, -1, 0, 1, lethal - 1, lethal, 100, 127), fields with 0, 0xFFFFFFFE and UNREACHED."""
    _run(gpu, fc.size_case(W, H))


@pytest.mark.parametrize("lethal", [1, 100])
def test_lethal_at_its_ends(gpu, lethal):
    _run(gpu, fc.size_case(65, 65, lethal=lethal))


@pytest.mark.parametrize("name", ["vertical", "horizontal", "diagonal", "antidiagonal", "ne", "hook"])
def test_seams(gpu, name):
    fc.seams_regime()
    _run(gpu, fc.seam_cases()[name])


def test_serpentine_inside_one_tile(gpu):
    fc.chains_regime()
    _run(gpu, fc.serpentine_case())


def test_spiral_over_nine_tiles(gpu):
    _run(gpu, fc.spiral_case())


@pytest.mark.parametrize("name", ["no_unknown", "no_free", "walls"])
def test_nothing_to_find(gpu, name):
    fc.counts_regime()
    got = _run(gpu, fc.empty_cases()[name])
    assert got[0]["n_goal"] == 0 and got[0]["goal"] == GUARD_WORD


# ---- counts, bounds, rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_size", [1, 2])
def test_lattice(gpu, min_size):
    _run(gpu, fc.lattice_case(min_size))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_comp_cap(gpu, delta):
    got = _run(gpu, fc.lattice_case(1, comp_cap=fc.LATTICE_N + delta))
    assert bool(got[0]["result"][0] & fo.BOUND) == (delta < 0)


@pytest.mark.parametrize("row_cap", [0, fc.LATTICE_N - 1, fc.LATTICE_N + 1])
def test_row_cap(gpu, row_cap):
    _run(gpu, fc.lattice_case(1, row_cap=row_cap))


def test_no_optional_output(gpu):
    c = dict(fc.size_case(131, 70), row_cap=0)
    f = _Front([c], labels=False, goal=False)
    f.call(gpu, rows=0)
    gpu.synchronize()
    want = fc.want(c)["result"]
    assert _u32(f.d_res)[:16].tolist() == want.tolist() and (_u32(f.d_rows) == GUARD_WORD).all()


# ---- the potential and the cost ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["none", "split", "equal", "huge", "zero"])
def test_potential(gpu, name):
    fc.potential_regime()
    _run(gpu, fc.potential_cases()[name])


@pytest.mark.parametrize("name", ["default", "size_only", "dist_only", "kept_one", "tie", "all_tie", "mixed", "big"])
def test_cost(gpu, name):
    fc.cost_regime()
    _run(gpu, fc.cost_cases()[name])


def test_three_grids_padded_strides(gpu):
    cases = [fc.size_case(131, 70, seed=s) for s in (0, 1, 2)]
    assert len({c["grid"].tobytes() for c in cases}) == 3
    _run(gpu, cases, grid_pad=8, pot_pad=7, label_pad=9, row_pad=5, goal_pad=3)
    _run(gpu, [fc.size_case(131, 70, with_potential=False)] * 2)


def test_called_twice_the_scratch_holds_nothing(gpu):
    f = _Front([fc.spiral_case()])
    first = f.run(gpu)
    second = f.run(gpu)
    _same(second[0], fc.want(fc.spiral_case()), "spiral again")
    assert first[0]["result"].tolist() == second[0]["result"].tolist()


# ---- with E26 ------------------------------------------------------------------------------------------------------------------
def test_goal_words_feed_nav_field(gpu):
    """The goal words E29 writes, fed unchanged into rplgpu_nav_field_dev, give the field of the oracle's BEST cell."""
    import torch
    from tests import nav_oracle as no
    dev = torch.device("cuda:0")
    c = fc.room_case()
    W, H = c["spec"]["width"], c["spec"]["height"]
    ns = no.spec(width=W, height=H, rounds=60)
    robot = 120 * W + 60
    d_from = no.field_heap(c["grid"], [robot], ns)
    c = dict(c, name="room_from_robot", potential=d_from)
    want = fc.want(c)
    assert want["n_goal"] == 1 and want["result"][3] >= 2
    f = _Front([c])
    f.call(gpu)
    d_pot = torch.full((W * H,), GUARD_WORD, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(abi.nav_field_scratch_words(no.struct_of(ns), 1), dtype=torch.int32, device=dev)
    d_res = torch.zeros(8, dtype=torch.int32, device=dev)
    gpu.nav_field_dev(no.struct_of(ns), f.d_grid.data_ptr(), f.grid_stride, 1, f.d_goal.data_ptr(), f.goal_stride,
                      f.d_n.data_ptr(), d_pot.data_ptr(), W * H, d_scr.data_ptr(), 0, d_res.data_ptr())
    gpu.synchronize()
    assert _u32(f.d_goal)[0] == want["goal"] and _u32(f.d_n)[0] == 1
    res = _u32(d_res)
    assert res[0] == 0 and res[2] == 1 and res[3] == 0
    assert _u32(d_pot).reshape(H, W).tobytes() == no.field_heap(c["grid"], [want["goal"]], ns).tobytes()


def test_chain_behind_e14_and_e12(gpu):
    """256 x 256, a room with a doorway into unknown space: rplgpu_map_grid_dev (a count map as rplgpu_map_update_dev
    leaves it) -> rplgpu_inflate_grids_dev -> rplgpu_nav_field_dev from the robot's cell -> rplgpu_frontiers_dev ->
    rplgpu_nav_field_dev to the frontier -> rplgpu_nav_paths_dev, queued on one stream, each reading the buffer the
    one before wrote, ONE synchronise behind the last; the oracles chained the same way."""
    import torch
    from tests import inflate_cases as ic
    from tests import inflate_oracle as io
    from tests import map_oracle as mo
    from tests import nav_oracle as no
    dev = torch.device("cuda:0")
    room = fc.room_case()
    W, H = room["spec"]["width"], room["spec"]["height"]
    counts = np.zeros((H, W, 2), np.uint32)  # (misses, hits)
    counts[room["grid"] == fc.FREE] = (3, 0)
    counts[room["grid"] == fc.WALL] = (0, 3)
    rule = mo.rule()
    grid_want = mo.grid_of_counts(counts, rule)[0]
    assert grid_want.tobytes() == room["grid"].tobytes()
    table = ic.lib_table(2)
    cost_want = io.inflate(grid_want, table, 2, 0)[0]
    ns = no.spec(width=W, height=H, rounds=60)
    robot = 120 * W + 60
    from_want = no.field_heap(cost_want, [robot], ns)
    fs = dict(room["spec"])
    c = dict(room, name="room_chain", grid=cost_want, potential=from_want, spec=fs)
    fw = fc.want(c)
    assert fw["n_goal"] == 1 and fw["result"][3] >= 2 and fw["result"][0] == 0
    to_want = no.field_heap(cost_want, [fw["goal"]], ns)
    path_want, info_want = no.path(cost_want, to_want, ns, robot, 600)
    assert info_want[1] == no.REACHED and len(path_want) > 20

    stride = (W * H + 3) & ~3
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
    d_counts = torch.from_numpy(counts.reshape(-1).view(np.int32)).to(dev)
    d_grid = torch.full((stride,), GUARD, dtype=torch.int8, device=dev)
    d_cost = torch.full((stride,), GUARD, dtype=torch.int8, device=dev)
    d_table = torch.from_numpy(table).to(dev)
    d_robot, d_one = i32(1, robot), i32(1, 1)
    d_from, d_to = i32(W * H, GUARD_WORD), i32(W * H, GUARD_WORD)
    d_nscr = i32(abi.nav_field_scratch_words(no.struct_of(ns), 1))
    d_nres, d_nres2 = i32(8), i32(8)
    d_fscr = i32(abi.frontiers_scratch_words(fo.struct_of(fs), 1, c["comp_cap"]))
    d_fres, d_goal, d_ngoal = i32(16), i32(1, GUARD_WORD), i32(1, GUARD_WORD)
    d_rows = i32(8 * 4, GUARD_WORD)
    d_paths, d_info = i32(600, GUARD_WORD), i32(4)
    spec = no.struct_of(ns)
    gpu.map_grid_dev(d_counts.data_ptr(), W, H, abi.MapRule(**rule), 0, d_grid.data_ptr(), stride, 0)
    gpu.inflate_grids_dev(d_grid.data_ptr(), stride, d_cost.data_ptr(), stride, 1, W, H, d_table.data_ptr(), 2, 0, 0)
    gpu.nav_field_dev(spec, d_cost.data_ptr(), stride, 1, d_robot.data_ptr(), 1, d_one.data_ptr(), d_from.data_ptr(),
                      W * H, d_nscr.data_ptr(), 0, d_nres.data_ptr())
    gpu.frontiers_dev(fo.struct_of(fs), d_cost.data_ptr(), stride, d_from.data_ptr(), W * H, 1, c["comp_cap"], 0, 0,
                      d_rows.data_ptr(), 32, 4, d_goal.data_ptr(), 1, d_ngoal.data_ptr(), d_fres.data_ptr(),
                      d_fscr.data_ptr())
    gpu.nav_field_dev(spec, d_cost.data_ptr(), stride, 1, d_goal.data_ptr(), 1, d_ngoal.data_ptr(), d_to.data_ptr(),
                      W * H, d_nscr.data_ptr(), 0, d_nres2.data_ptr())
    gpu.nav_paths_dev(spec, d_cost.data_ptr(), stride, d_to.data_ptr(), W * H, 1, d_robot.data_ptr(), 1,
                      d_paths.data_ptr(), 600, d_info.data_ptr())
    gpu.synchronize()
    assert d_grid.cpu().numpy()[:W * H].tobytes() == grid_want.tobytes()
    assert d_cost.cpu().numpy()[:W * H].tobytes() == cost_want.tobytes()
    assert _u32(d_nres)[0] == 0 and _u32(d_from).tobytes() == from_want.tobytes()
    print("frontiers", _u32(d_fres).tolist())
    assert _u32(d_fres).tolist() == fw["result"].tolist() and _u32(d_rows).reshape(4, 8).tobytes() == fw["rows"].tobytes()
    assert _u32(d_goal)[0] == fw["goal"] and _u32(d_ngoal)[0] == 1
    assert _u32(d_nres2)[0] == 0 and _u32(d_to).tobytes() == to_want.tobytes()
    info = _u32(d_info).tolist()
    assert info == list(info_want) and _u32(d_paths)[:info[0]].tolist() == list(path_want)
    assert (_u32(d_paths)[info[0]:] == GUARD_WORD).all()


# ---- the door, the refusals ----------------------------------------------------------------------------------------------------
def test_host_buffers(gpu):
    for c in (fc.spiral_case(), fc.size_case(131, 70), fc.lattice_case(1, comp_cap=fc.LATTICE_N - 1),
              fc.empty_cases()["no_free"]):
        got = gpu.frontiers(fo.struct_of(c["spec"]), c["grid"], c["potential"], comp_cap=c["comp_cap"],
                            row_cap=c["row_cap"], row_fill=GUARD_WORD, goal_fill=GUARD_WORD)
        _same(dict(got, goal=int(got["goal"][0]), n_goal=int(got["n_goal"][0])), fc.want(c), c["name"] + " (door)")
    c = fc.size_case(65, 65)
    got = gpu.frontiers(fo.struct_of(c["spec"]), c["grid"], None, comp_cap=c["comp_cap"], row_cap=0, labels=False)
    assert got["result"][1] == fo.frontiers_walk(c["grid"], None, c["spec"], c["comp_cap"])["result"][1]
    with pytest.raises(abi.RplGpuError) as e:
        gpu.frontiers(fo.struct_of(dict(c["spec"], lethal=101)), c["grid"])
    assert e.value.code == abi.ERR_INVALID_ARG
    with pytest.raises(abi.RplGpuError) as e:
        gpu.frontiers(fo.struct_of(c["spec"]), c["grid"], comp_cap=0)
    assert e.value.code == abi.ERR_INVALID_ARG


def test_refusals_leave_every_output(gpu):
    c = fc.size_case(65, 65)
    f = _Front([c])
    host = np.zeros(64, np.uint32)

    def code(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            f.call(gpu, **kw)
        return e.value.code

    p = lambda t: t.data_ptr()  # noqa: E731
    words = lambda t, n: p(t) + 4 * n  # noqa: E731
    refused = [dict(width=0), dict(height=4097), dict(lethal=0), dict(lethal=101), dict(min_size=0),
               dict(dist_weight=65536), dict(size_weight=65536), dict(G=0), dict(G=65536), dict(cap=0),
               dict(cap=(1 << 20) + 1), dict(grid=0), dict(res=0), dict(scr=0), dict(rows=0), dict(goal=0), dict(n=0),
               dict(gs=f.cells - 1), dict(gs=f.grid_stride + 2), dict(ps=f.cells - 1), dict(ls=f.cells - 1),
               dict(rs=8 * f.row_cap - 1), dict(gos=0), dict(grid=p(f.d_grid) + 1), dict(pot=p(f.d_pot) + 2),
               dict(lab=p(f.d_lab) + 1), dict(rows=p(f.d_rows) + 2), dict(goal=p(f.d_goal) + 1), dict(n=p(f.d_n) + 2),
               dict(res=p(f.d_res) + 1), dict(scr=p(f.d_scr) + 8), dict(scr=p(f.d_scr) + 4),
               dict(res=host.ctypes.data), dict(grid=host.ctypes.data),
               # an output on an input, an output on an output (over the ranges used)
               dict(lab=p(f.d_pot)), dict(rows=words(f.d_pot, f.cells - 1)), dict(res=p(f.d_scr)),
               dict(goal=words(f.d_res, 15)), dict(n=p(f.d_goal)), dict(lab=words(f.d_scr, 16)),
               dict(scr=p(f.d_lab)), dict(res=words(f.d_lab, f.cells - 1)), dict(rows=p(f.d_grid))]
    for kw in refused:
        assert code(**dict(kw)) == abi.ERR_INVALID_ARG, kw
    # G x tiles above RPLGPU_NAV_MAX_TILES: refused before anything is queued (no buffer of that size is needed)
    assert code(width=4096, height=4096, G=2049, gs=1 << 24, ps=1 << 24, ls=1 << 24, pot=0, lab=0, rows=0, rc=0,
                goal=0, n=0, cap=1) == abi.ERR_CAPACITY
    gpu.synchronize()
    for t in (f.d_lab, f.d_rows, f.d_goal, f.d_n, f.d_res, f.d_scr):
        assert (_u32(t) == GUARD_WORD).all()
    assert f.d_grid.cpu().numpy().tobytes() == f.host_grid.tobytes()
    got = f.run(gpu)  # and the handle goes on working
    _same(got[0], fc.want(c), c["name"])
