"""What E17 and E21 share, on the device.  (1) One list through E20 -> E21, then E17 with an open gate on the same list
with the weights zeroed outside a sub-list: E21's two sets of sums are E17's set 0 of the two sub-lists word for word
(every sum is an integer, so equal is exact).  (2) The refusals every pose-list door shares — G, P, the pose stride and
the weight stride — with the texts rplgpu_last_error gives, for E16, E17, E20, E21 and E22."""
import functools

import numpy as np
import pytest

from rplidar_ros2_driver_amd import abi
from tests import bins_oracle as bo
from tests import estimate_oracle as eo

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD_WORD = 0x5A5A5A5A
PAD = 5
NONE = 0xFFFFFFFF
T = 8
BINS = bo.spec(-8.0, -8.0, 2.0, 32, 32)                            # 16 m x 16 m in bins of 0.5 m
XY_SCALE = float(1 << 21)                                           # E17's range: |x|, |y| < 4 m, inside the bins
# the wave edge, the tile edge (1025: one live lane in the second tile) and the finish kernel's second round per lane
SIZES = [63, 65, 1024, 1025, 65 * 1024 + 1]


def _up(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda:0"))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _full(k):
    import torch
    return torch.full((k,), GUARD_WORD, dtype=torch.int32, device=torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _list(P, seed):
    """-> (poses (P, 4), weights (P,)): two clusters of unequal weight with coordinates of both signs (mirrored for an
    odd seed), every seventh weight 0, pose 1 in a bin of its own beyond E17's range; the last pose is the heavy
    cluster's and has a weight"""
    rng = np.random.default_rng(seed)
    i = np.arange(P)
    heavy = (P - 1 - i) % 5 < 3
    sign = -1.0 if seed & 1 else 1.0
    xy = sign * np.where(heavy[:, None], (-2.0, 1.0), (2.5, -1.5)) + rng.uniform(-0.2, 0.2, (P, 2))
    th = np.where(heavy, 0.3, -2.0) + rng.uniform(-0.05, 0.05, P)
    poses = np.stack([np.cos(th), np.sin(th), xy[:, 0], xy[:, 1]], axis=1).astype(F32)
    poses[1, 2:] = (6.0, 6.0)
    w = rng.integers(1, 1000, P).astype(np.uint32)
    w[~heavy] = w[~heavy] // 2 + 1
    w[i % 7 == 3] = 0
    assert w[P - 1] != 0 and w[1] != 0 and heavy[P - 1]
    poses.setflags(write=False)
    w.setflags(write=False)
    return poses, w


def _estimate(gpu, d_p, pstride, ppg, h_w, G, P):
    """E17 with an open gate over the device lists at d_p with the weights h_w (G, P) -> (G, 72) words"""
    d_w, d_r = _up(h_w), _full(72 * G + 8)
    d_s = _full(abi.estimate_scratch_words(G, P) + 2)
    gpu.estimate_poses_dev(d_p.data_ptr(), pstride, ppg, d_w.data_ptr(), P, G, P,
                           abi.PoseEstimate.open_gate(xy_scale=XY_SCALE), 0, 0, d_r.data_ptr(), d_s.data_ptr())
    gpu.synchronize()
    r = _u32(d_r)
    assert (r[72 * G:] == GUARD_WORD).all()
    return r[:72 * G].reshape(G, 72)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_group"])
@pytest.mark.parametrize("P", SIZES)
def test_shared_sums(gpu, P, shared):
    G = 2
    lists = [_list(P, 0)] if shared else [_list(P, 0), _list(P, 1)]
    L = len(lists)
    h_w = np.stack([_list(P, g)[1] for g in range(G)])              # a shared list still has a weight row per group
    h_p = np.full((L, P + PAD, 4), 123.0, F32)
    for g in range(L):
        h_p[g, :P] = lists[g][0]
    pstride, ppg = 4 * (P + PAD), 1 if L > 1 else 0
    words = bo.map_words(BINS, T)
    mstride = words + (words & 1)
    d_p, d_w, d_e = _up(h_p.view(np.uint32)), _up(h_w), _up(bo.table(T).view(np.uint32))
    d_m, d_b, d_r20 = _full(G * mstride), _full(G * P), _full(8 * G)
    d_l, d_r21 = _full(G * P), _full(80 * G + 8)
    d_s = _full(abi.cluster_scratch_words(G, P, BINS.nx, BINS.ny, T) + 2)
    gpu.bin_poses_dev(abi.PoseBins(BINS.origin_x, BINS.origin_y, BINS.inv_size, BINS.nx, BINS.ny, 0), d_p.data_ptr(),
                      pstride, ppg, d_w.data_ptr(), P, G, P, d_e.data_ptr(), T, d_m.data_ptr(), mstride, d_b.data_ptr(),
                      P, d_r20.data_ptr())
    gpu.cluster_poses_dev(abi.PoseClusters(BINS.nx, BINS.ny, XY_SCALE, 1), d_p.data_ptr(), pstride, ppg, d_w.data_ptr(),
                          P, G, P, T, d_m.data_ptr(), mstride, d_b.data_ptr(), P, d_l.data_ptr(), P, 0, 0, 0,
                          d_r21.data_ptr(), d_s.data_ptr())
    gpu.synchronize()
    labels, r21 = _u32(d_l).reshape(G, P), _u32(d_r21)
    assert (r21[80 * G:] == GUARD_WORD).all()
    r21 = r21[:80 * G].reshape(G, 80)
    w_best, w_all = h_w.copy(), h_w.copy()
    for g in range(G):
        poses = lists[g if L > 1 else 0][0]
        inr = eo.quantise(poses, XY_SCALE)[1]
        print(f"P {P} group {g}: E21 words 0-7 {r21[g][:8].tolist()} 72-77 {r21[g][72:78].tolist()}")
        # the regime: at least three clusters, BEST heavier than SECOND, weights of 0 (unlabelled), pose 1 labelled
        # but out of E17's range (flag bit 1), no loop bound hit
        assert int(r21[g][6]) >= 3 and int(r21[g][0]) & 0x3F == 2 and int(r21[g][77]) > 0
        assert not inr[1] and labels[g][1] != NONE and inr.sum() == P - 1
        w_second = int(r21[g][74]) | int(r21[g][75]) << 32
        assert 0 < w_second < (int(r21[g][40]) | int(r21[g][41]) << 32)
        w_best[g][labels[g] != r21[g][1]] = 0
        w_all[g][(labels[g] == NONE) | ~inr] = 0
        assert w_best[g][P - 1] != 0                                # the last lane of the last tile contributes
    e_best, e_all = _estimate(gpu, d_p, pstride, ppg, w_best, G, P), _estimate(gpu, d_p, pstride, ppg, w_all, G, P)
    for g in range(G):
        assert r21[g][40:72].tobytes() == e_best[g][8:40].tobytes(), g
        assert r21[g][8:40].tobytes() == e_all[g][8:40].tobytes(), g
        assert int(r21[g][5]) == int(e_best[g][3]) and int(r21[g][3]) == int(e_all[g][3])     # the poses with w != 0
        assert r21[g][8:40].tobytes() != r21[g][40:72].tobytes()


# ---- the refusals the pose-list doors share -------------------------------------------------------------------------------
# the text behind "<function>: " that rplgpu_last_error gives, per door: G, P, pose_stride, weight_stride
STRIDES = "pose_stride >= 4 P and a multiple of 4 and weight_stride >= P are required"
P_RANGE = "P must be in 1 .. RPLGPU_MAX_POSES"
RESAMPLE_STRIDES = ("weight_stride >= P, pose_stride >= 4 P, out_stride >= 4 M (both multiples of 4) and anc_stride >= M "
                    "are required")
TEXTS = {
    "rplgpu_resample_poses_dev": ("G must be in 1 .. 65535", "P and M must be in 1 .. RPLGPU_MAX_POSES", RESAMPLE_STRIDES,
                                  RESAMPLE_STRIDES),
    "rplgpu_estimate_poses_dev": ("G must be in 1 .. 65535", P_RANGE, STRIDES, STRIDES),
    "rplgpu_bin_poses_dev": ("G must be in 1 .. 65535", P_RANGE, STRIDES, STRIDES),
    "rplgpu_cluster_poses_dev": ("G must be in 1 .. 65535", P_RANGE, STRIDES, STRIDES),
    "rplgpu_cast_ranges_dev": ("G must be in 1 .. 65535",
                               "P must be in 1 .. RPLGPU_MAX_POSES, A in 1 .. RPLGPU_MAX_MERGE_BEAMS and P * A at most 2^28",
                               "pose_stride >= 4 P and a multiple of 4 is required",
                               "weight_stride >= P and meas_first + (A - 1) * meas_step < meas_stride are required"),
}


@pytest.mark.parametrize("door", sorted(TEXTS))
def test_refusal_texts(gpu, door):
    import torch
    P, A, words = 8, 4, 2                                           # 4 x 4 x 4 bins: two map words
    ins = {k: _up(np.zeros(n, np.uint32)) for k, n in
           (("poses", 4 * P), ("w", P), ("edges", 2 * T), ("map", words), ("bins", P), ("u", 1), ("beams", 2 * A),
            ("grid", 64), ("meas", A), ("table", 64))}
    outs = {k: _full(n) for k, n in (("res", 96), ("scratch", 4096), ("out", 4 * P), ("anc", P), ("labels", P),
                                     ("ranges", P * A), ("cast", 8), ("map_out", words), ("bins_out", P), ("w_out", P))}
    p = {k: t.data_ptr() for k, t in {**ins, **outs}.items()}

    def call(G=1, P=P, pstride=4 * P, wstride=P):
        if door == "rplgpu_resample_poses_dev":
            gpu.resample_poses_dev(p["w"], wstride, p["poses"], pstride, 0, G, P, 8, p["u"], 0, 0, 0, 0, p["out"], 32,
                                   p["anc"], 8, p["res"], p["scratch"])
        elif door == "rplgpu_estimate_poses_dev":
            gpu.estimate_poses_dev(p["poses"], pstride, 0, p["w"], wstride, G, P, abi.PoseEstimate.defaults(), 0, 0,
                                   p["res"], p["scratch"])
        elif door == "rplgpu_bin_poses_dev":
            gpu.bin_poses_dev(abi.PoseBins.defaults(nx=4, ny=4), p["poses"], pstride, 0, p["w"], wstride, G, P,
                              p["edges"], 4, p["map_out"], words, p["bins_out"], 8, p["res"])
        elif door == "rplgpu_cluster_poses_dev":
            gpu.cluster_poses_dev(abi.PoseClusters.defaults(nx=4, ny=4), p["poses"], pstride, 0, p["w"], wstride, G, P, 4,
                                  p["map"], words, p["bins"], 8, p["labels"], 8, 0, 0, 0, p["res"], p["scratch"])
        else:
            gpu.cast_ranges_dev(abi.RangeCast.defaults(width=8, height=8), p["poses"], pstride, 0, G, P, p["beams"], A,
                                p["grid"], 64, 0, p["meas"], A, 0, 1, p["table"], p["ranges"], 8 * A, p["w_out"], wstride,
                                p["res"], p["cast"])

    t_g, t_p, t_ps, t_ws = TEXTS[door]
    for kw, text in ((dict(G=0), t_g), (dict(P=0), t_p), (dict(P=abi.MAX_POSES + 1), t_p),
                     (dict(pstride=4 * P - 4), t_ps), (dict(wstride=P - 1), t_ws)):
        with pytest.raises(abi.RplGpuError) as e:
            call(**kw)
        print(door, kw, "->", e.value)
        assert e.value.code == abi.ERR_INVALID_ARG, kw
        assert str(e.value) == f"rplgpu error {abi.ERR_INVALID_ARG}: {door}: {text}", kw
    gpu.synchronize()
    torch.cuda.synchronize()
    for k, t in outs.items():                                       # all of them fail before any launch
        assert (_u32(t) == GUARD_WORD).all(), k
