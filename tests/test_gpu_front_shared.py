"""What the scan front end of csrc/rpl_front.hpp is shared for, on the device: the stages that open a scan through it
agree WITH EACH OTHER on the same scans, which no per-stage test checks.  One input — two groups of two scans, an E1
clip and an E5 mask that each drop samples, inverted, motion with per-scan time offsets, a mount per scan, samples
whose transformed position is not finite — goes through E13, E15, E23, E24 and E25 with one shared field:
  * the "finite points" words (E13 d_best 4, E15 d_result 4, E23 d_result 4 and agree 0, E24 d_best 4, E25 d_result 7)
    are equal to each other and to pose_oracle.finite_points of the oracle's points;
  * with one identity pose and a zero window, E15's weight of pose 0 is E13's d_best word 0 and E24's d_best word 5;
  * E25's summed V for that pose is refine_oracle.sums_numpy's for the same points.
The scan lengths are the edges of the pair load, the wave and the pass; guard words lie behind every output."""
import ctypes as C
import functools

import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth
from tests import agree_oracle as ao
from tests import match_cases as mc
from tests import match_oracle as mo
from tests import pose_oracle as po
from tests import refine_oracle as ro
from tests import wide_oracle as wo
from tests.occ_cases import rot_poses

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 0x5A
GUARD_WORD = 0x5A5A5A5A
PAD = 5
B, GROUP, G = 4, 2, 2
# the pair load (an odd n leaves i1 = n to be dropped), the wave (128 samples) and the pass (2048: 2049 and 4097 need a
# second and a third one)
LENGTHS = (1, 2, 127, 128, 129, 2047, 2048, 2049, 4097)
IEEE_LENGTHS = (129, 2049)
GRID = dict(origin_x=-6.4, origin_y=-6.4, resolution=0.05, width=256, height=256)
IDENTITY = np.array([[[1, 0, 0, 0]]], F32)  # one list of one pose


@functools.lru_cache(maxsize=None)
def _case(n):
    """Four scans of n samples around a ring of mounts.  From 127 samples on every scan has two isolated returns for
    E5 to remove; the E1 clip cuts the ranges beyond 5 m and the qualities below 40 (a third of each, about).  Scan 3
    stands under a mount whose first row is scaled by 1e38: a sample more than 3.4 m off along x overflows to a
    position that is not finite, a nearer one lands 1e38 m away (finite, without a cell)."""
    batch = synth.make_batch(3100 + n, B, n, noise_m=0.01, r0_range=(2.0, 5.5)).copy()
    if n >= 127:
        for b in range(B):
            for i in (n // 3 + 5 * b, (2 * n) // 3 + 3 * b):
                batch[b]["dist_mm_q2"][i - 2:i + 3] = 0
                batch[b]["dist_mm_q2"][i] = 4000
                batch[b]["quality"][i] = 200
    rng = np.random.default_rng(3101)
    ang = 2 * np.pi * np.arange(B) / B
    pose2d = rot_poses(ang + 0.3, 0.6 * np.cos(ang), 0.6 * np.sin(ang))
    pose2d[3, 0] = F32(1.0e38)
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                       for _ in range(B)]).astype(F32)
    t0 = rng.uniform(-0.02, 0.02, B).astype(F32)
    # E5 with a radius that holds a scan's neighbours at its length (the samples of a scan of 127 lie 0.1 - 0.3 m apart)
    # and lets the isolated returns, 1 m or more from theirs, go; a scan of one or two samples has no two neighbours
    p = Params.defaults(clip_enable=1, q_min=40, range_min=0.15, range_max=5.0, inverted=1, ror_enable=1,
                        ror_radius=max(0.10, 100.0 / n), ror_min_neighbors=min(2, n - 1))
    fields = mc.random_field(3102, 1, GRID["height"], GRID["width"])
    for a in (batch, pose2d, motion, t0, fields):
        a.setflags(write=False)
    return dict(batch=batch, lens=np.full(B, n), group=GROUP, p=p, fields=fields, pose2d=pose2d, motion=motion, t0=t0,
                spec=mo.spec(shift_x=0, shift_y=0, rot_steps=0, **GRID))


@functools.lru_cache(maxsize=None)
def _want(oracle, n):
    """Per group, from the oracle's points alone: (finite points, E15's weight of the identity, E25's sums of the
    identity, some position has no cell).  The regime: what the case claims to exercise is there."""
    case = _case(n)
    p_ror_off = Params.defaults(**{k: getattr(case["p"], k) for k, _ in Params._fields_})
    p_ror_off.ror_enable = 0
    p_plain = Params.defaults(**{k: getattr(p_ror_off, k) for k, _ in Params._fields_})
    p_plain.clip_enable = 0
    out = []
    with np.errstate(over="ignore", invalid="ignore"):  # (scan 3's mount overflows on purpose)
        for g in range(G):
            x, y = mc.case_points(oracle, case, g)
            fx, fy = po.finite_points(x, y)
            w, status, _ = po.weights_of(fx, fy, IDENTITY[0], po.spec(**GRID), case["fields"][0])
            sums = ro.sums_numpy(fx, fy, IDENTITY[0][0], ro.spec(min_points=3, **GRID), case["fields"][0])
            out.append(dict(finite=len(fx), weight=int(w[0]), sums=sums, no_cell=bool(status)))
            if n >= 127:
                assert len(x) < len(mc.case_points(oracle, case, g, p_ror_off)[0]) < \
                    len(mc.case_points(oracle, case, g, p_plain)[0]), "E5 drops samples, and E1 drops others"
        if n >= 127:
            x1, y1 = mc.case_points(oracle, case, 1)
            assert len(po.finite_points(x1, y1)[0]) < len(x1), "group 1 has positions that are not finite"
            assert out[1]["no_cell"] and all(o["finite"] > 20 and o["weight"] > 0 for o in out)
    return out


def _dev():
    import torch
    return torch.device("cuda:0")


def _full(k):
    import torch
    return torch.full((k,), GUARD_WORD, dtype=torch.int32, device=_dev())


def _words(t, k):
    """the first k words of a guarded output; everything behind them is still the guard"""
    w = t.cpu().numpy().view(np.uint32)
    assert (w[k:] == GUARD_WORD).all(), "words behind an output were written"
    return w[:k]


def _run(gpu, case):
    """The five stages on one upload of the case -> the result words of each, (G, 8), and what goes with them."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())  # noqa: E731
    n = case["batch"].shape[1]
    d_nodes = up(np.ascontiguousarray(case["batch"]).view(np.uint8).reshape(B, n * 8))
    d_lens, d_motion, d_pose2d, d_t0 = (up(a) for a in (np.asarray(case["lens"], np.int32), case["motion"],
                                                         case["pose2d"], case["t0"]))
    cells = GRID["width"] * GRID["height"]
    fstride = cells + 4
    host_field = np.full(fstride, GUARD, np.uint8)
    host_field[:cells] = case["fields"][0].reshape(-1).view(np.uint8)
    d_field = up(host_field)
    host_poses = np.full(8, 123.0, F32)
    host_poses[:4] = IDENTITY.reshape(-1)
    d_poses = up(host_poses)
    front = (d_nodes.data_ptr(), n, d_lens.data_ptr(), B, GROUP, case["p"], d_motion.data_ptr(), d_pose2d.data_ptr())
    grid = tuple(GRID[k] for k in ("origin_x", "origin_y", "resolution", "width", "height"))
    list_of_one = (d_poses.data_ptr(), 1, 8, 0, d_field.data_ptr(), fstride, 0)
    s13 = case["spec"]
    s24 = wo.spec(max_blocks=4, **s13)
    m13 = abi.ScanMatch(*grid, 0, 0, 0, s13["rot_step"])
    m24 = abi.WideMatch(*grid, 0, 0, 0, s13["rot_step"], s24["max_blocks"])
    s23 = ao.spec(**GRID)
    words = (n + 31) // 32
    pcells = (GRID["width"] + 7) * (GRID["height"] + 7)
    pstride = ((pcells + 3) & ~3) + 4
    scratch24, scratch25 = wo.scratch_words(s24, G), abi.refine_scratch_words(G, 1)
    o = dict(scores=_full(G * (1 + PAD)), best13=_full(8 * G + PAD), w15=_full(G * (1 + PAD)), res15=_full(8 * G + PAD),
             w23=_full(G * (1 + PAD)), res23=_full(8 * G + PAD), agree=_full(8 * G + PAD), counts=_full(B * (n + PAD)),
             mask=_full(B * (words + PAD)), bounds=_full(G * (1 + PAD)), scratch24=_full(scratch24 + PAD),
             best24=_full(8 * G + PAD), work=_full(8 * G + PAD), sums=_full(G * 36),
             scratch25=_full(scratch25 + PAD), res25=_full(8 * G + PAD))
    st = {k: _full(G + PAD) for k in ("13", "15", "23", "24", "25")}
    d_pooled = torch.full((pstride,), GUARD, dtype=torch.uint8, device=_dev())
    ptr = {k: t.data_ptr() for k, t in o.items()}
    gpu.set_scan_time_offsets_dev(d_t0.data_ptr())
    try:
        gpu.match_scans_dev(*front, 0, m13, d_field.data_ptr(), fstride, 0, ptr["scores"], 1 + PAD, ptr["best13"],
                            st["13"].data_ptr())
        gpu.score_poses_dev(*front, abi.PoseScore(*grid), *list_of_one, ptr["w15"], 1 + PAD, ptr["res15"],
                            st["15"].data_ptr())
        gpu.score_poses_agree_dev(*front, abi.BeamAgree(*grid, s23["agree_lo"], s23["keep_num"], s23["keep_den"],
                                                        s23["err_num"], s23["err_den"]),
                                  *list_of_one, ptr["w23"], 1 + PAD, ptr["res23"], st["23"].data_ptr(), ptr["counts"],
                                  n + PAD, ptr["mask"], words + PAD, ptr["agree"])
        gpu.pool_field_dev(m24, d_field.data_ptr(), fstride, 1, d_pooled.data_ptr(), pstride)
        gpu.match_wide_dev(*front, 0, m24, d_field.data_ptr(), fstride, 0, d_pooled.data_ptr(), pstride,
                           ptr["bounds"], 1 + PAD, ptr["scratch24"], ptr["best24"], ptr["work"], st["24"].data_ptr())
        gpu.refine_sums_dev(*front, ro.struct_of(ro.spec(min_points=3, **GRID)), *list_of_one, ptr["sums"], 36,
                            ptr["scratch25"], ptr["res25"], st["25"].data_ptr())
        gpu.synchronize()
    finally:
        gpu.set_scan_time_offsets_dev(0)
    assert d_field.cpu().numpy().tobytes() == host_field.tobytes()
    assert d_poses.cpu().numpy().tobytes() == host_poses.tobytes()
    assert (d_pooled.cpu().numpy()[pcells:] == GUARD).all()
    _words(o["scratch24"], scratch24), _words(o["scratch25"], scratch25), _words(o["work"], 8 * G)
    rows = lambda k, r, w: o[k].cpu().numpy().view(np.uint32).reshape(r, -1)  # noqa: E731
    for k, r, w in (("scores", G, 1), ("w15", G, 1), ("w23", G, 1), ("bounds", G, 1), ("sums", G, 32), ("counts", B, n),
                    ("mask", B, words)):  # (E25's stride is a multiple of 4: four guard words behind a group's sums)
        assert (rows(k, r, w)[:, w:] == GUARD_WORD).all(), k
    return dict(best13=_words(o["best13"], 8 * G).reshape(G, 8), res15=_words(o["res15"], 8 * G).reshape(G, 8),
                res23=_words(o["res23"], 8 * G).reshape(G, 8), agree=_words(o["agree"], 8 * G).reshape(G, 8),
                best24=_words(o["best24"], 8 * G).reshape(G, 8), res25=_words(o["res25"], 8 * G).reshape(G, 8),
                w15=rows("w15", G, 1)[:, 0], sums=rows("sums", G, 32)[:, :32],
                status={k: _words(t, G) for k, t in st.items()})


def _check(got, want):
    for g, w in enumerate(want):
        finite = [int(v) for v in (got["best13"][g][4], got["res15"][g][4], got["res23"][g][4], got["agree"][g][0],
                                   got["best24"][g][4], got["res25"][g][7])]
        weight = [int(v) for v in (got["w15"][g], got["best13"][g][0], got["best24"][g][5])]
        sv = int(got["sums"][g][10]) | (int(got["sums"][g][11]) << 32)
        print(f"group {g}: finite points E13 E15 E23 E23-agree E24 E25 {finite} want {w['finite']}; weight E15, E13 "
              f"word 0, E24 word 5 {weight} want {w['weight']}; E25 S V {sv} want {w['sums']['sv']}; status "
              f"{ {k: int(v[g]) for k, v in got['status'].items()} }")
        assert finite == [w["finite"]] * 6, (g, finite, w["finite"])
        assert weight == [w["weight"]] * 3, (g, weight, w["weight"])
        assert got["sums"][g].tobytes() == ro.to_words(w["sums"]).tobytes(), (g, ro.from_words(got["sums"][g]))
        cell_range = abi.SCAN_CELL_RANGE if w["no_cell"] else 0
        assert all(int(v[g]) == cell_range for v in got["status"].values()), (g, got["status"])


@pytest.mark.parametrize("n", LENGTHS)
def test_stages_agree(gpu, oracle, n):
    _check(_run(gpu, _case(n)), _want(oracle, n))


@pytest.mark.parametrize("n", IEEE_LENGTHS)
def test_stages_agree_ieee_divide(gpu, oracle, n):
    """A handle whose fast divides are refused (as tests/test_gpu_ieee_div.py arranges): the other instance of every
    kernel, the same words."""
    import torch

    from tests.conftest import _shared_stream
    lib = abi.load_library()
    lib.rplgpu_debug_force_ieee_div.argtypes = [C.c_void_p, C.c_uint32]
    lib.rplgpu_debug_force_ieee_div.restype = C.c_int32
    h = RplGpu(device=0, max_samples_per_scan=32768, max_batch=64)
    try:
        h.set_stream(_shared_stream().cuda_stream)
        assert lib.rplgpu_debug_force_ieee_div(h._h, 7) == abi.OK
        got = _run(h, _case(n))
        torch.cuda.synchronize()
    finally:
        h.close()
    _check(got, _want(oracle, n))
