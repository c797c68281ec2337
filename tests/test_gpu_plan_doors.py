"""The doors of the six device calls of E26 - E29 (rplgpu_nav_field_dev, rplgpu_nav_paths_dev, rplgpu_rollout_dev,
rplgpu_mppi_update_dev, rplgpu_mppi_spread_dev, rplgpu_frontiers_dev), where their checks are shared: which of two
faults at once is reported, that the text names the function (and says "overlap" for an overlap), the in-place forms
that are accepted and the near misses that are not, that an optional pointer given as NULL clashes with nothing, that
a refused call leaves every output and that the next good call gives the oracle's answer.  Tiny shapes: 70 x 3 grids
(two tiles, padded strides), G = 2, K = 5, T = 2, F = 1, comp_cap 4.  The expected codes were recorded from the
library before its doors shared these checks; the helpers that hold a call's buffers are the stage tests' own."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import frontier_cases as fc
from tests import mppi_cases as mc
from tests import mppi_oracle as mo
from tests import nav_cases as nc
from tests import nav_oracle as no
from tests import rollout_cases as rc
from tests import rollout_oracle as ro
from tests import test_gpu_frontier as tf
from tests import test_gpu_mppi as tm
from tests import test_gpu_nav as tn
from tests import test_gpu_rollout as tr

pytestmark = pytest.mark.gpu
GUARD_WORD = 0x5A5A5A5A
W, H, G, K, T, F, CAP = 70, 3, 2, 5, 2, 1, 4
INVALID, CAPACITY = abi.ERR_INVALID_ARG, abi.ERR_CAPACITY
FAR = 1 << 40  # a stride that, times a group, reaches over every buffer of the process


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ptr(t, byte=0):
    return t.data_ptr() + byte


def _refused(fn, do, code, overlap=False):
    """do() is refused with `code`, and the handle's text begins with the function's name."""
    with pytest.raises(abi.RplGpuError) as e:
        do()
    text = str(e.value).split(": ", 1)[1]
    print(f"{fn}: {e.value.code}: {text}")
    assert e.value.code == code, (e.value.code, code, text)
    assert text.startswith(fn + ": "), text
    assert not overlap or "overlap" in text, text


def _host():
    return np.zeros(4096, np.uint32).ctypes.data


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _nav_cases():
    out = []
    for g in range(G):
        grid = nc.random_grid(7000 + g, W, H)
        grid[1, 5 + g] = 0
        out.append(nc.case(f"plan{W}x{H}_{g}", grid, [W + 5 + g]))
    return out


def _rollout_cases(potential=True):
    out = []
    for g in range(G):
        rng = np.random.default_rng(40 + g)
        grid = rng.integers(0, 40, (H, W)).astype(np.int8)
        grid[:, 40 + g] = 100
        grid[0, 10] = -1
        delta = np.zeros((K, T, 4), np.float32)
        delta[..., 0] = 1.0
        delta[..., 2] = rng.uniform(0.1, 2.5, (K, T))
        s = ro.spec(origin_x=0.0, origin_y=0.0, resolution=0.1, width=W, height=H, steps=T, min_steps=1, a_end=3,
                    a_min=2, a_sum=5, a_max=11)
        pot = rng.integers(0, 5000, (H, W)).astype(np.uint32) if potential else None
        out.append(rc.case(f"plan{W}x{H}_{g}_{int(potential)}", s, rc.pose(0.35, 0.15), delta, rc.ring(F), grid, pot))
    return out


def _mppi_cases(nominal=True):
    return [mc.case(f"plan_{g}_{int(nominal)}", K, T, 1, seed=900 + g, nominal=nominal) for g in range(G)]


def _frontier_cases(**kw):
    return [dict(fc.size_case(W, H, seed=g, **kw), comp_cap=CAP) for g in range(G)]


def _spread_cases():
    out = []
    for g in range(G):
        rng = np.random.default_rng(300 + g)
        out.append(dict(name=f"plan_spread_{g}", nominal=mc.nominal_of(rng, T), noise=mc.deltas(rng, K, T, 0.1),
                        shift=1, keep_first=1))
    return out


# ---- E26 ------------------------------------------------------------------------------------------------------------------------
class _Nav:
    def __init__(self):
        import torch
        self.cases = _nav_cases()
        self.f = f = tn._Field(self.cases)
        self.S, self.max_len = 2, 80
        starts = np.array([[W + 60, 2 * W + 69], [3, W + 30]], np.uint32)
        self.starts = starts
        self.d_starts = torch.from_numpy(starts.reshape(-1).view(np.int32)).to("cuda:0")
        self.d_paths, self.d_info = tm._full(G * self.S * self.max_len + 4), tm._full(4 * G * self.S + 4)
        self.field_args = dict(spec=dict(f.s), grid=_ptr(f.d_grid), gs=f.grid_stride, G=G, goals=_ptr(f.d_goals),
                               gos=f.goal_stride, n=_ptr(f.d_n), pot=_ptr(f.d_pot), ps=f.pot_stride, scr=_ptr(f.d_scr),
                               resume=0, res=_ptr(f.d_res))
        self.paths_args = dict(spec=dict(f.s), grid=_ptr(f.d_grid), gs=f.grid_stride, pot=_ptr(f.d_pot),
                               ps=f.pot_stride, G=G, starts=_ptr(self.d_starts), S=self.S, paths=_ptr(self.d_paths),
                               max_len=self.max_len, info=_ptr(self.d_info))

    @staticmethod
    def _merged(base, kw):
        a = dict(base, spec=dict(base["spec"]))
        a["spec"].update({k: kw.pop(k) for k in list(kw) if k in a["spec"]})
        a.update(kw)
        return a

    def field(self, gpu, **kw):
        a = self._merged(self.field_args, kw)
        gpu.nav_field_dev(no.struct_of(a["spec"]), a["grid"], a["gs"], a["G"], a["goals"], a["gos"], a["n"], a["pot"],
                          a["ps"], a["scr"], a["resume"], a["res"])

    def paths(self, gpu, **kw):
        a = self._merged(self.paths_args, kw)
        gpu.nav_paths_dev(no.struct_of(a["spec"]), a["grid"], a["gs"], a["pot"], a["ps"], a["G"], a["starts"], a["S"],
                          a["paths"], a["max_len"], a["info"])


def test_nav_doors(gpu):
    n = _Nav()
    f = n.f
    big = dict(width=4096, height=4096, G=2049, gs=1 << 24, ps=1 << 24)  # G x tiles above RPLGPU_NAV_MAX_TILES
    field = [(dict(lethal=0, G=0), INVALID), (dict(rounds=0, gs=f.cells - 1), INVALID),
             (dict(grid=_ptr(f.d_grid, 1), ps=f.cells - 1), INVALID), (dict(G=65536, pot=_ptr(f.d_pot, 2)), INVALID),
             (dict(big, gs=(1 << 24) - 4), INVALID), (dict(big, ps=(1 << 24) - 1), INVALID),
             (dict(big, scr=_ptr(f.d_scr, 2)), INVALID), (dict(big, gos=0), INVALID), (dict(big), CAPACITY),
             (dict(big, res=_host()), CAPACITY), (dict(big, goals=_host(), pot=_host()), CAPACITY),
             (dict(resume=2, res=_host()), INVALID), (dict(gos=0, goals=_host()), INVALID)]
    for kw, code in field:
        _refused("rplgpu_nav_field_dev", lambda: n.field(gpu, **dict(kw)), code)
    paths = [(dict(lethal=101, S=0), INVALID), (dict(G=0, gs=f.cells - 1), INVALID),
             (dict(grid=_ptr(f.d_grid, 2), ps=f.cells - 1), INVALID), (dict(gs=f.grid_stride + 2, max_len=0), INVALID),
             (dict(S=0, starts=_ptr(n.d_starts, 1)), INVALID), (dict(ps=f.cells - 1, info=_host()), INVALID),
             (dict(paths=_ptr(n.d_paths, 2), info=_host()), INVALID), (dict(S=65537, paths=_host()), INVALID)]
    for kw, code in paths:
        _refused("rplgpu_nav_paths_dev", lambda: n.paths(gpu, **dict(kw)), code)
    gpu.synchronize()
    for t in (f.d_pot, f.d_scr, f.d_res, n.d_paths, n.d_info):
        assert (_u32(t) == GUARD_WORD).all()
    pot, res = tn._finish(gpu, f)  # the next good calls
    tn._check((pot, res), n.cases)
    n.paths(gpu)
    gpu.synchronize()
    got_paths, info = _u32(n.d_paths), _u32(n.d_info)
    assert (got_paths[G * n.S * n.max_len:] == GUARD_WORD).all() and (info[4 * G * n.S:] == GUARD_WORD).all()
    got_paths = got_paths[:G * n.S * n.max_len].reshape(G, n.S, n.max_len)
    info = info[:4 * G * n.S].reshape(G, n.S, 4)
    for g, c in enumerate(n.cases):
        tn._check_paths(c, pot[g], n.starts[g].tolist(), n.max_len, (got_paths[g], info[g]))


# ---- E27 ------------------------------------------------------------------------------------------------------------------------
def test_rollout_doors(gpu):
    f = tr._Call(_rollout_cases())
    d = f.d_in
    big = dict(G=65535, K=4097, dps=0, ds=1 << 20, os=1 << 20, es=1 << 20)  # above RPLGPU_ROLLOUT_MAX_TILES
    cases = [(dict(lethal=0, G=0), INVALID, False), (dict(steps=0, K=0), INVALID, False),
             (dict(G=0, F=0), INVALID, False), (dict(F=65, out=0), INVALID, False),
             (dict(grid=_ptr(d[3], 1), gs=f.cells - 4), INVALID, False),
             (dict(pot=_ptr(d[4], 2), os=8 * K - 4), INVALID, False),
             (dict(out=_ptr(f.d_out, 8), ps=f.cells - 1), INVALID, False),
             (dict(big, gs=f.cells - 4), INVALID, False), (dict(big, ps=f.cells - 1), INVALID, False),
             (dict(big, grid=_ptr(d[3], 2)), INVALID, False), (dict(big), CAPACITY, False),
             (dict(big, out=_ptr(d[1])), CAPACITY, False), (dict(big, res=_host()), CAPACITY, False),
             (dict(scr=_ptr(f.d_out), res=_host()), INVALID, True), (dict(out=_ptr(d[1]), grid=_host()), INVALID, True),
             (dict(end=_ptr(f.d_out, 16), out=_ptr(f.d_out)), INVALID, True),
             (dict(res=_ptr(d[0])), INVALID, True), (dict(scr=_ptr(d[4])), INVALID, True)]
    for kw, code, overlap in cases:
        _refused("rplgpu_rollout_dev", lambda: f.call(gpu, **dict(kw)), code, overlap)
    gpu.synchronize()
    assert f.untouched()
    f.run(gpu)


def test_rollout_absent_optionals_clash_with_nothing(gpu):
    """No field and no end poses: their strides, whatever they are, span nothing."""
    f = tr._Call(_rollout_cases(potential=False), end_poses=False)
    assert not f.has_pot and f.d_end is None
    f.pot_stride = f.end_stride = FAR
    f.run(gpu)


# ---- E28 ------------------------------------------------------------------------------------------------------------------------
def test_mppi_update_doors(gpu):
    f = tm._Update(_mppi_cases())
    d = f.d_in
    fn = "rplgpu_mppi_update_dev"
    big = 1 << 22
    over = dict(G=65535, K=1 << 16, delta_per_step=0, os=big, ds=big, ws=big)  # above RPLGPU_MPPI_MAX_BLOCKS
    assert f.nout_stride != f.nom_stride
    cases = [(dict(shift=50, G=0), INVALID, False), (dict(table_len=0, K=0), INVALID, False),
             (dict(G=65536, K=0), INVALID, False), (dict(K=0, out=0), INVALID, False),
             (dict(out=_ptr(d[0], 8), os=8 * K - 4), INVALID, False), (dict(over, ws=K - 1), INVALID, False),
             (dict(over, sums=_ptr(f.d_sums, 8)), INVALID, False), (dict(over), CAPACITY, False),
             (dict(over, w=_ptr(d[0])), CAPACITY, False), (dict(over, res=_host()), CAPACITY, False),
             (dict(w=_ptr(d[0]), res=_host()), INVALID, True), (dict(sums=_ptr(f.d_w), out=_host()), INVALID, True),
             (dict(scr=_ptr(d[2])), INVALID, True),
             # nominal_out on nominal: another stride, 16 bytes in, one nominal for two groups
             (dict(nout=_ptr(d[4])), INVALID, True), (dict(nout=_ptr(d[4], 16), nos=f.nom_stride), INVALID, True),
             (dict(nout=_ptr(d[4]), nos=f.nom_stride, npg=0), INVALID, True)]
    for kw, code, overlap in cases:
        _refused(fn, lambda: f.call(gpu, **dict(kw)), code, overlap)
    gpu.synchronize()
    assert f.untouched()
    f.run(gpu)
    # the accepted forms: a nominal per group; one group with a shared nominal
    tm._Update(_mppi_cases(), in_place=True).run(gpu)
    tm._Update(_mppi_cases()[:1], share_nominal=True, in_place=True).run(gpu)


def test_mppi_update_absent_nominal_clashes_with_nothing(gpu):
    f = tm._Update(_mppi_cases(nominal=False))
    assert not f.has_nom
    f.nom_stride = FAR
    f.run(gpu)


def test_mppi_spread_doors(gpu):
    cases = _spread_cases()
    n = 4 * K * T
    d_nom, d_noise, d_out = tm._full(G * 4 * T), tm._full(G * n + 8), tm._full(G * n + 8)
    fn = "rplgpu_mppi_spread_dev"

    def call(**kw):
        a = dict(nom=_ptr(d_nom), ns=4 * T, npg=1, T_n=T, noise=_ptr(d_noise), zs=n, zpg=1, G=G, K=K, T=T, shift=0,
                 keep=0, out=_ptr(d_out), os=n)
        a.update(kw)
        gpu.mppi_spread_dev(a["nom"], a["ns"], a["npg"], a["T_n"], a["noise"], a["zs"], a["zpg"], a["G"], a["K"],
                            a["T"], a["shift"], a["keep"], a["out"], a["os"])

    over = dict(G=65535, K=1 << 16, T=1, zs=1 << 20, os=1 << 20)  # above RPLGPU_MPPI_MAX_BLOCKS
    refused = [(dict(G=0, K=0), INVALID, False), (dict(T=257, nom=0), INVALID, False),
               (dict(shift=257, out=_ptr(d_out, 4)), INVALID, False), (dict(nom=_ptr(d_nom, 4), ns=4 * T - 4), INVALID, False),
               (dict(over, ns=2), INVALID, False), (dict(over, noise=_ptr(d_noise, 8)), INVALID, False),
               (dict(over), CAPACITY, False), (dict(over, out=_ptr(d_nom)), CAPACITY, False),
               (dict(over, out=_host()), CAPACITY, False),
               (dict(out=_ptr(d_nom), noise=_host()), INVALID, True), (dict(out=_ptr(d_nom), nom=_ptr(d_nom)), INVALID, True),
               # the output on the noise: another stride, 16 bytes in, one noise for two groups
               (dict(out=_ptr(d_noise), os=n + 4), INVALID, True), (dict(out=_ptr(d_noise, 16)), INVALID, True),
               (dict(out=_ptr(d_noise), zpg=0), INVALID, True)]
    for kw, code, overlap in refused:
        _refused(fn, lambda: call(**dict(kw)), code, overlap)
    gpu.synchronize()
    assert all((_u32(t) == GUARD_WORD).all() for t in (d_nom, d_noise, d_out))
    tm._spread(gpu, cases)
    # the accepted forms: a noise per group; one group with a shared noise
    tm._spread(gpu, cases, in_place=True)
    tm._spread(gpu, cases[:1], share_noise=True, in_place=True)


# ---- E29 ------------------------------------------------------------------------------------------------------------------------
def test_frontier_doors(gpu):
    cases = _frontier_cases()
    f = tf._Front(cases)
    fn = "rplgpu_frontiers_dev"
    over = dict(width=4096, height=4096, G=2049, gs=1 << 24, ps=1 << 24, ls=1 << 24, pot=0, lab=0, rows=0, rc=0,
                goal=0, n=0, cap=1)  # G x tiles above RPLGPU_NAV_MAX_TILES
    refused = [(dict(lethal=0, G=0), INVALID, False), (dict(min_size=0, cap=0), INVALID, False),
               (dict(G=65536, cap=0), INVALID, False), (dict(cap=0, grid=0), INVALID, False),
               (dict(grid=_ptr(f.d_grid, 1), gs=f.cells - 1), INVALID, False),
               (dict(rows=_ptr(f.d_rows, 2), gs=f.cells - 1), INVALID, False),
               (dict(pot=_ptr(f.d_pot, 2), rs=8 * f.row_cap - 1), INVALID, False),
               (dict(over, gs=(1 << 24) - 4), INVALID, False), (dict(over, scr=_ptr(f.d_scr, 4)), INVALID, False),
               (dict(over), CAPACITY, False), (dict(over, res=_ptr(f.d_scr)), CAPACITY, False),
               (dict(over, res=_host()), CAPACITY, False),
               (dict(lab=_ptr(f.d_pot), res=_host()), INVALID, True), (dict(rows=_ptr(f.d_pot), grid=_host()), INVALID, True),
               (dict(n=_ptr(f.d_goal)), INVALID, True), (dict(scr=_ptr(f.d_lab)), INVALID, True)]
    for kw, code, overlap in refused:
        _refused(fn, lambda: f.call(gpu, **dict(kw)), code, overlap)
    gpu.synchronize()
    for t in (f.d_lab, f.d_rows, f.d_goal, f.d_n, f.d_res, f.d_scr):
        assert (_u32(t) == GUARD_WORD).all()
    assert f.d_grid.cpu().numpy().tobytes() == f.host_grid.tobytes()
    got = f.run(gpu)
    for g, c in enumerate(cases):
        tf._same(got[g], fc.want(c), c["name"])


def test_frontier_absent_optionals_clash_with_nothing(gpu):
    """No field, no labels, no rows and no goal words: their strides span nothing."""
    cases = [dict(c, row_cap=0) for c in _frontier_cases(with_potential=False)]
    f = tf._Front(cases, labels=False, goal=False)
    f.pot_stride = f.label_stride = f.row_stride = f.goal_stride = FAR
    f.call(gpu, rows=0)
    gpu.synchronize()
    res = _u32(f.d_res)
    for g, c in enumerate(cases):
        assert res[16 * g:16 * g + 16].tolist() == fc.want(c)["result"].tolist(), c["name"]
    assert (res[16 * G:] == GUARD_WORD).all() and (_u32(f.d_rows) == GUARD_WORD).all()
