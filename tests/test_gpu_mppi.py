"""E28 on the device: rplgpu_mppi_update_dev and rplgpu_mppi_spread_dev against tests/mppi_oracle.py byte for byte —
the weights, the sums, the new nominal sequence and the result words, guard words behind every output, behind the
scratch and the result, every input compared after the call — at the kernels' edges (tests/mppi_cases.py), the spread's
identity with E16's move, the chain E18 -> spread -> E27 -> update -> spread -> E27 on one stream, both host-buffer
doors, and every refusal.  E27's words are made by hand but in the chain, whose grid is E27's own test grid."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import mppi_cases as mc
from tests import mppi_oracle as mo

pytestmark = pytest.mark.gpu
GUARD_WORD = 0x5A5A5A5A


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int16 if a.dtype == np.uint16 else np.int32)).to("cuda:0")


def _full(n):
    import torch
    return torch.full((n,), GUARD_WORD, dtype=torch.int32, device="cuda:0")


class _Update:
    """The groups of one update call on the device (cases of one spec and K, one table), every output filled with
    guard words, strides padded; run() is one call, checked against the oracle."""

    def __init__(self, cases, share_delta=False, share_nominal=False, pad=1, in_place=False):
        c0 = cases[0]
        self.cases, self.G = cases, len(cases)
        self.s, self.T_e = c0["spec"], mo.steps_e(c0["spec"])
        self.K = len(c0["out"])
        self.has_nom = c0["nominal"] is not None
        self.flags = (0 if share_delta else 1, 0 if share_nominal else 1)
        self.in_place = in_place
        G, K, T_e = self.G, self.K, self.T_e
        self.out_stride = 8 * K + 4 * pad
        self.delta_stride = 4 * K * T_e + 4 * pad
        self.nom_stride = 4 * T_e + 8 * pad
        self.w_stride = K + pad
        self.sums_stride = 8 * T_e + 4 * pad
        self.nout_stride = self.nom_stride if in_place else 4 * T_e + 4 * pad
        out = np.full((G, self.out_stride), 7, np.uint32)
        delta = np.full((G, self.delta_stride), 1.0e9, np.float32)
        nom = np.full((G, self.nom_stride), 3.0e9, np.float32)
        for g, c in enumerate(cases):
            out[g, :8 * K] = c["out"].reshape(-1)
            delta[g, :4 * K * T_e] = c["delta"].reshape(-1)
            if self.has_nom:
                nom[g, :4 * T_e] = c["nominal"].reshape(-1)
        rres = np.stack([c["rres"] for c in cases])
        self.host_in = [out, rres, delta, np.ascontiguousarray(c0["table"]), nom]
        self.d_in = [_dev(a) for a in self.host_in]
        self.scratch_words = abi.mppi_scratch_words(G, K, T_e)
        assert self.scratch_words == mo.scratch_words(G, K, T_e) > 0
        self.d_w, self.d_sums = _full(G * self.w_stride), _full(G * self.sums_stride)
        self.d_nout = self.d_in[4] if in_place else _full(G * self.nout_stride)
        self.d_res, self.d_scr = _full(8 * G + 8), _full(self.scratch_words + 8)

    def args(self, **kw):
        d = self.d_in
        a = dict(spec=dict(self.s), out=d[0].data_ptr(), os=self.out_stride, rres=d[1].data_ptr(),
                 delta=d[2].data_ptr(), ds=self.delta_stride, dpg=self.flags[0], table=d[3].data_ptr(),
                 nom=d[4].data_ptr() if self.has_nom else 0, ns=self.nom_stride, npg=self.flags[1], G=self.G, K=self.K,
                 w=self.d_w.data_ptr(), ws=self.w_stride, sums=self.d_sums.data_ptr(), ss=self.sums_stride,
                 nout=self.d_nout.data_ptr(), nos=self.nout_stride, res=self.d_res.data_ptr(),
                 scr=self.d_scr.data_ptr())
        spec_kw = {k: kw.pop(k) for k in list(kw) if k in self.s}
        a.update(kw)
        a["spec"].update(spec_kw)
        return a

    def call(self, gpu, **kw):
        a = self.args(**kw)
        gpu.mppi_update_dev(mo.struct_of(a["spec"]), a["out"], a["os"], a["rres"], a["delta"], a["ds"], a["dpg"],
                            a["table"], a["nom"], a["ns"], a["npg"], a["G"], a["K"], a["w"], a["ws"], a["sums"],
                            a["ss"], a["nout"], a["nos"], a["res"], a["scr"])

    def outputs(self):
        G, K, T_e = self.G, self.K, self.T_e
        w = _u32(self.d_w).reshape(G, self.w_stride)
        sums = _u32(self.d_sums).reshape(G, self.sums_stride)
        nout = _u32(self.d_nout).reshape(G, self.nout_stride)
        res, scr = _u32(self.d_res), _u32(self.d_scr)
        assert (w[:, K:] == GUARD_WORD).all() and (sums[:, 8 * T_e:] == GUARD_WORD).all()
        assert (res[8 * G:] == GUARD_WORD).all() and (scr[self.scratch_words:] == GUARD_WORD).all()
        if self.in_place:
            assert nout[:, 4 * T_e:].tobytes() == self.host_in[4][:, 4 * T_e:].tobytes()
        else:
            assert (nout[:, 4 * T_e:] == GUARD_WORD).all()
        for host, d in list(zip(self.host_in, self.d_in))[:4 if self.in_place else 5]:
            assert d.cpu().numpy().tobytes() == host.tobytes()  # the inputs are only read
        return w[:, :K], sums[:, :8 * T_e].reshape(G, T_e, 8), nout[:, :4 * T_e].reshape(G, T_e, 4), \
            res[:8 * G].reshape(G, 8)

    def untouched(self):
        tensors = [self.d_w, self.d_sums, self.d_res, self.d_scr] + ([] if self.in_place else [self.d_nout])
        return all((_u32(t) == GUARD_WORD).all() for t in tensors)

    def run(self, gpu, wants=None):
        self.call(gpu)
        gpu.synchronize()
        w, sums, nout, res = self.outputs()
        for g, c in enumerate(self.cases):
            want = wants[g] if wants else mc.want(c)
            print(f"{c['name']}: result {res[g].tolist()}")
            assert w[g].tobytes() == want[0].tobytes(), c["name"]
            assert sums[g].tobytes() == want[1].tobytes(), (c["name"], np.argwhere(sums[g] != want[1])[:4])
            assert nout[g].tobytes() == want[2].tobytes(), (c["name"], nout[g].view(np.float32)[:3], want[2][:3])
            assert res[g].tolist() == want[3].tolist(), c["name"]
        return w, sums, nout, res


# ---- the update: shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T,per_step", mc.SHAPES)
def test_shapes(gpu, K, T, per_step):
    mc.shapes_regime()
    _Update([mc.shape_case(K, T, per_step)]).run(gpu)


def _mixed(cases, share_delta, share_nominal):
    """What group g computes when the call shares group 0's deltas or nominal."""
    out = []
    for c in cases:
        m = dict(c, name=c["name"] + f"_mix{int(share_delta)}{int(share_nominal)}")
        if share_delta:
            m["delta"] = cases[0]["delta"]
        if share_nominal:
            m["nominal"] = cases[0]["nominal"]
        out.append(m)
    return out


@pytest.mark.parametrize("share", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("per_step", [0, 1])
def test_three_groups_with_padded_strides(gpu, share, per_step):
    cases = _mixed(mc.group_cases(per_step), *share)
    assert len(cases) == 3
    _Update(cases, bool(share[0]), bool(share[1]), pad=3).run(gpu)


def test_without_padding(gpu):
    _Update(list(mc.group_cases()), pad=0).run(gpu)


# ---- the update: weights and ranges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["none_admissible", "none_admissible_no_nominal", "best_only", "shift_0", "shift_49",
                                  "below_best", "clamp_n1", "clamp_n65536", "big_sums"])
def test_weights(gpu, name):
    mc.weight_regime()
    _Update([mc.weight_cases()[name]]).run(gpu)


@pytest.mark.parametrize("name", ["not_finite", "h_edges", "empty_step", "empty_step_no_nominal",
                                  "empty_step_odd_nominal"])
def test_ranges(gpu, name):
    mc.range_regime()
    _Update([mc.range_cases()[name]]).run(gpu)


def test_nominal_out_on_nominal(gpu):
    mc.range_regime()
    _Update([mc.range_cases()["empty_step_odd_nominal"]], in_place=True).run(gpu)
    _Update(list(mc.group_cases()), pad=2, in_place=True).run(gpu)


# ---- the spread -----------------------------------------------------------------------------------------------------------------
def _spread(gpu, cases, share_nominal=False, share_noise=False, pad=1, in_place=False):
    c0 = cases[0]
    G, (K, T), T_n = len(cases), c0["noise"].shape[:2], len(c0["nominal"])
    n_stride, z_stride = 4 * T_n + 4 * pad, 4 * K * T + 8 * pad
    o_stride = z_stride if in_place else 4 * K * T + 4 * pad
    nom = np.full((G, n_stride), 2.0e9, np.float32)
    noise = np.full((G, z_stride), 4.0e9, np.float32)
    for g, c in enumerate(cases):
        nom[g, :4 * T_n] = c["nominal"].reshape(-1)
        noise[g, :4 * K * T] = c["noise"].reshape(-1)
    d_nom, d_noise = _dev(nom), _dev(noise)
    d_out = d_noise if in_place else _full(G * o_stride)
    gpu.mppi_spread_dev(d_nom.data_ptr(), n_stride, 0 if share_nominal else 1, T_n, d_noise.data_ptr(), z_stride,
                        0 if share_noise else 1, G, K, T, c0["shift"], c0["keep_first"], d_out.data_ptr(), o_stride)
    gpu.synchronize()
    out = _u32(d_out).reshape(G, o_stride)
    assert d_nom.cpu().numpy().tobytes() == nom.tobytes()
    if in_place:
        assert out[:, 4 * K * T:].tobytes() == noise[:, 4 * K * T:].tobytes()
    else:
        assert (out[:, 4 * K * T:] == GUARD_WORD).all() and d_noise.cpu().numpy().tobytes() == noise.tobytes()
    for g, c in enumerate(cases):
        want = mo.spread_sweep(cases[0 if share_nominal else g]["nominal"], cases[0 if share_noise else g]["noise"],
                               c0["shift"], c0["keep_first"])
        assert out[g, :4 * K * T].tobytes() == want.tobytes(), (c["name"], g)
    return out


@pytest.mark.parametrize("name", [s[0] for s in mc.SPREADS])
@pytest.mark.parametrize("in_place", [False, True])
def test_spread(gpu, name, in_place):
    mc.spread_regime()
    c = mc.spread_case(name)
    out = _spread(gpu, [c], in_place=in_place)
    assert out[0, :c["noise"].size].tobytes() == mc.spread_want(name).tobytes()


@pytest.mark.parametrize("share", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_spread_three_groups(gpu, share):
    base = mc.spread_case("keep_first")
    cases = [base] + [dict(mc.spread_case("shift_1"), shift=base["shift"], keep_first=1, name=f"g{g}",
                           nominal=mc.nominal_of(np.random.default_rng(g), 6),
                           noise=mc.deltas(np.random.default_rng(9 + g), 65, 6, 0.1)) for g in (1, 2)]
    _spread(gpu, cases, bool(share[0]), bool(share[1]), pad=3)
    if not share[1]:
        _spread(gpu, cases, bool(share[0]), False, pad=2, in_place=True)


def test_spread_identity_with_e16_move_on_the_device(gpu):
    """Without keep_first, step t of all candidates equals rplgpu_resample_poses_dev with P = 1, the nominal step as
    the pose, weight 1, M = K, n_delta = M."""
    import torch
    c = mc.spread_case("shift_1")
    K, T = c["noise"].shape[:2]
    got = _spread(gpu, [c], pad=0)[0].reshape(K, T, 4)
    d_w = torch.ones(1, dtype=torch.int32, device="cuda:0")
    d_res = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    d_scr = torch.zeros(abi.resample_scratch_words(1, 1), dtype=torch.int32, device="cuda:0")
    outs = []
    for t in range(T):
        d_pose = _dev(c["nominal"][min(t + 1, len(c["nominal"]) - 1)])
        d_delta = _dev(np.ascontiguousarray(c["noise"][:, t]))
        d_o = torch.zeros(4 * K, dtype=torch.int32, device="cuda:0")
        gpu.resample_poses_dev(d_w.data_ptr(), 1, d_pose.data_ptr(), 4, 1, 1, 1, K, 0, d_delta.data_ptr(), K, 4 * K, 1,
                               d_o.data_ptr(), 4 * K, 0, 0, d_res.data_ptr(), d_scr.data_ptr())
        outs.append((d_pose, d_delta, d_o))
    gpu.synchronize()
    for t in range(T):
        assert _u32(outs[t][2]).tobytes() == got[:, t].tobytes(), t


# ---- the chain and the doors ---------------------------------------------------------------------------------------------------
def test_chain_e18_spread_e27_update_spread_e27(gpu):
    """rplgpu_sample_motion_dev -> spread -> rplgpu_rollout_dev -> update -> spread (shift 1, keep_first) ->
    rplgpu_rollout_dev queued on one stream with ONE synchronise behind the last, each reading the buffers the one
    before wrote; the oracles chained the same way.  Two groups with their own noise."""
    import torch

    from tests import rollout_cases as rc
    from tests import rollout_oracle as ro
    K, T, G = 70, 12, 2
    odom = np.array([1, 0, 0, 1, 0, 4e-6, 2e-6, 4e-6], np.float32)   # the identity with E18's three scales
    noise_spec = abi.MotionNoise.defaults()
    grid = rc.rough_grid(18)
    pot = rc.slope_field(grid)
    rs = rc.base_spec(steps=T, min_steps=T // 2, a_end=1, a_sum=4)
    start, fp = rc.pose(*rc.centre_of(8, 33), 0.1), rc.ring(4, 0.2)
    ms = mo.spec(steps=T, delta_per_step=1, table_len=256, shift=3)
    table = mc.table_of(400.0, 3, 256)
    nominal0 = np.tile(np.array([1, 0, 0.12, 0], np.float32), (T, 1))
    wants = []
    for g in range(G):
        noise, _ = abi.sample_motion_host(odom, K * T, noise_spec, group=g)
        noise = noise.reshape(K, T, 4)
        cand1 = mo.spread_sweep(nominal0, noise, 0, 0)
        roll1 = ro.sweep(rs, start, cand1, fp, grid, pot)
        upd = mo.update_sweep(ms, roll1[0], roll1[2], cand1, table, nominal0)
        cand2 = mo.spread_sweep(upd[2], noise, 1, 1)
        wants.append((cand1, roll1, upd, cand2, ro.sweep(rs, start, cand2, fp, grid, pot)))
    assert all(1 < w[2][3][0] <= K and w[2][3][7] == 0 and w[4][2][0] > 0 for w in wants), [w[2][3].tolist() for w in wants]
    assert wants[0][2][2].tobytes() != wants[1][2][2].tobytes() != nominal0.tobytes()
    n = 4 * K * T
    d_odom, d_nom0, d_table = _dev(odom), _dev(nominal0), _dev(table)
    d_start, d_fp, d_pot = _dev(start), _dev(fp), _dev(pot)
    d_grid = torch.from_numpy(grid.reshape(-1)).to("cuda:0")
    d_noise, d_cand1, d_cand2 = _full(G * n), _full(G * n), _full(G * n)
    d_mres = _full(8 * G)
    d_out1, d_end, d_res1, d_out2, d_res2 = _full(G * 8 * K), _full(G * 4 * K), _full(8 * G), _full(G * 8 * K), _full(8 * G)
    d_rscr = _full(abi.rollout_scratch_words(G, K))
    d_w, d_sums, d_nom1, d_ures = _full(G * K), _full(G * 8 * T), _full(G * 4 * T), _full(8 * G)
    d_uscr = _full(abi.mppi_scratch_words(G, K, T))

    def roll(d_cand, d_out, d_res):
        gpu.rollout_dev(ro.struct_of(rs), d_start.data_ptr(), 0, d_cand.data_ptr(), n, 1, 1, d_fp.data_ptr(), len(fp),
                        d_grid.data_ptr(), grid.size, d_pot.data_ptr(), grid.size, 0, G, K, d_out.data_ptr(), 8 * K,
                        d_end.data_ptr(), 4 * K, d_res.data_ptr(), d_rscr.data_ptr())

    gpu.sample_motion_dev(d_odom.data_ptr(), 0, G, K * T, noise_spec, d_noise.data_ptr(), n, d_mres.data_ptr())
    gpu.mppi_spread_dev(d_nom0.data_ptr(), 4 * T, 0, T, d_noise.data_ptr(), n, 1, G, K, T, 0, 0, d_cand1.data_ptr(), n)
    roll(d_cand1, d_out1, d_res1)
    gpu.mppi_update_dev(mo.struct_of(ms), d_out1.data_ptr(), 8 * K, d_res1.data_ptr(), d_cand1.data_ptr(), n, 1,
                        d_table.data_ptr(), d_nom0.data_ptr(), 4 * T, 0, G, K, d_w.data_ptr(), K, d_sums.data_ptr(),
                        8 * T, d_nom1.data_ptr(), 4 * T, d_ures.data_ptr(), d_uscr.data_ptr())
    gpu.mppi_spread_dev(d_nom1.data_ptr(), 4 * T, 1, T, d_noise.data_ptr(), n, 1, G, K, T, 1, 1, d_cand2.data_ptr(), n)
    roll(d_cand2, d_out2, d_res2)
    gpu.synchronize()
    got = [_u32(t).reshape(G, -1) for t in (d_cand1, d_out1, d_res1, d_w, d_sums, d_nom1, d_ures, d_cand2, d_out2, d_res2)]
    print("update", got[6].tolist(), "rollout 2", got[9].tolist())
    for g, (cand1, roll1, upd, cand2, roll2) in enumerate(wants):
        want = (cand1, roll1[0], roll1[2], upd[0], upd[1], upd[2], upd[3], cand2, roll2[0], roll2[2])
        for i, (a, b) in enumerate(zip(got, want)):
            assert a[g].tobytes() == np.ascontiguousarray(b).tobytes(), (g, i)


def test_host_buffers(gpu):
    for c in (mc.shape_case(257, 56, 1), mc.shape_case(33, 7, 0), mc.range_cases()["empty_step_no_nominal"]):
        got = gpu.mppi_update(mo.struct_of(c["spec"]), c["out"], c["rres"], c["delta"], c["table"], c["nominal"])
        assert mo.equal(got, mc.want(c)), c["name"]
    for name in ("shift_1", "keep_first"):
        c = mc.spread_case(name)
        got = gpu.mppi_spread(c["nominal"], c["noise"], c["shift"], c["keep_first"])
        assert got.tobytes() == mc.spread_want(name).tobytes(), name
    c = mc.shape_case(33, 7, 0)
    with pytest.raises(abi.RplGpuError) as e:
        gpu.mppi_update(mo.struct_of(dict(c["spec"], shift=50)), c["out"], c["rres"], c["delta"], c["table"])
    assert e.value.code == abi.ERR_INVALID_ARG
    c = mc.spread_case("shift_1")
    with pytest.raises(abi.RplGpuError) as e:
        gpu.mppi_spread(c["nominal"], c["noise"], 257, 0)
    assert e.value.code == abi.ERR_INVALID_ARG


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_update_refusals_leave_every_output(gpu):
    f = _Update(list(mc.group_cases(G=2)))
    host = np.zeros(4096, np.uint32)
    K, T = f.K, f.T_e

    def code(**kw):
        with pytest.raises(abi.RplGpuError) as e:
            f.call(gpu, **kw)
        return e.value.code

    ptr = lambda t: t.data_ptr()  # noqa: E731
    d = f.d_in
    refused = [dict(xy_scale=0.0), dict(xy_scale=float("nan")), dict(shift=50), dict(table_len=0),
               dict(table_len=65537), dict(steps=0), dict(steps=257), dict(delta_per_step=2),
               dict(G=0), dict(G=65536), dict(K=0), dict(K=(1 << 20) + 1), dict(steps=256, K=(1 << 16) + 1),
               dict(out=0), dict(rres=0), dict(delta=0), dict(table=0), dict(w=0), dict(sums=0), dict(nout=0),
               dict(res=0), dict(scr=0),
               dict(out=ptr(d[0]) + 8), dict(rres=ptr(d[1]) + 2), dict(delta=ptr(d[2]) + 4), dict(table=ptr(d[3]) + 1),
               dict(nom=ptr(d[4]) + 8), dict(w=ptr(f.d_w) + 2), dict(sums=ptr(f.d_sums) + 8),
               dict(nout=ptr(f.d_nout) + 4), dict(res=ptr(f.d_res) + 1), dict(scr=ptr(f.d_scr) + 8),
               dict(os=8 * K - 4), dict(os=f.out_stride + 2), dict(ds=4 * K * T - 4), dict(ds=f.delta_stride + 1),
               dict(ns=4 * T - 4), dict(ns=f.nom_stride + 2), dict(ws=K - 1), dict(ss=8 * T - 4),
               dict(ss=f.sums_stride + 2), dict(nos=4 * T - 4), dict(nos=f.nout_stride + 3),
               # an output that overlaps an input or another output
               dict(w=ptr(d[0])), dict(sums=ptr(d[2])), dict(nout=ptr(d[2])), dict(res=ptr(d[1])), dict(scr=ptr(d[0])),
               dict(w=ptr(d[3])), dict(sums=ptr(f.d_w)), dict(res=ptr(f.d_scr)), dict(nout=ptr(f.d_sums) + 16),
               dict(nout=ptr(d[4]) + 16), dict(nout=ptr(d[4])),           # on nominal, but with another stride
               dict(nout=ptr(d[4]), nos=f.nom_stride, npg=0),            # ... or shared by two groups
               # host memory
               dict(out=host.ctypes.data), dict(w=host.ctypes.data), dict(res=host.ctypes.data)]
    assert f.nout_stride != f.nom_stride
    for kw in refused:
        assert code(**dict(kw)) == abi.ERR_INVALID_ARG, kw
    # a launch above RPLGPU_MPPI_MAX_BLOCKS workgroups: refused before anything is queued
    big = 1 << 22
    assert code(G=65535, K=1 << 16, delta_per_step=0, os=big, ds=big, ws=big) == abi.ERR_CAPACITY
    gpu.synchronize()
    assert f.untouched()
    f.run(gpu)  # and the handle goes on working


def test_spread_refusals_leave_the_output(gpu):
    K, T, T_n, G = 20, 5, 5, 2
    d_nom, d_noise, d_out = _full(G * 4 * T_n), _full(G * 4 * K * T + 8), _full(G * 4 * K * T + 8)
    host = np.zeros(4096, np.float32)

    def code(**kw):
        a = dict(nom=d_nom.data_ptr(), ns=4 * T_n, npg=1, T_n=T_n, noise=d_noise.data_ptr(), zs=4 * K * T, zpg=1, G=G,
                 K=K, T=T, shift=0, keep=0, out=d_out.data_ptr(), os=4 * K * T)
        a.update(kw)
        with pytest.raises(abi.RplGpuError) as e:
            gpu.mppi_spread_dev(a["nom"], a["ns"], a["npg"], a["T_n"], a["noise"], a["zs"], a["zpg"], a["G"], a["K"],
                                a["T"], a["shift"], a["keep"], a["out"], a["os"])
        return e.value.code

    p = lambda t: t.data_ptr()  # noqa: E731
    refused = [dict(G=0), dict(G=65536), dict(K=0), dict(K=(1 << 20) + 1), dict(T=0), dict(T=257), dict(T_n=0),
               dict(T_n=257), dict(shift=257), dict(K=(1 << 16) + 1, T=256), dict(nom=0), dict(noise=0), dict(out=0),
               dict(nom=p(d_nom) + 4), dict(noise=p(d_noise) + 8), dict(out=p(d_out) + 4), dict(ns=4 * T_n - 4),
               dict(ns=4 * T_n + 2), dict(zs=4 * K * T - 4), dict(zs=4 * K * T + 1), dict(os=4 * K * T - 4),
               dict(os=4 * K * T + 2), dict(out=p(d_nom)), dict(out=p(d_noise) + 16),
               dict(out=p(d_noise), os=4 * K * T + 4),        # in place, but with another stride
               dict(out=p(d_noise), zpg=0),                   # ... or one noise for two groups
               dict(out=host.ctypes.data), dict(noise=host.ctypes.data)]
    for kw in refused:
        assert code(**dict(kw)) == abi.ERR_INVALID_ARG, kw
    assert code(G=65535, K=1 << 16, T=1, zs=1 << 20, os=1 << 20) == abi.ERR_CAPACITY
    gpu.synchronize()
    assert all((_u32(t) == GUARD_WORD).all() for t in (d_nom, d_noise, d_out))
