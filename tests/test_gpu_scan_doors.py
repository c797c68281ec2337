"""The four host-buffer doors that take scans (rplgpu_occupancy_grid, rplgpu_match_scans, rplgpu_map_update,
rplgpu_score_poses) with motion, pose2d and t0 ALL given and with NONE of them, each against its _dev entry point on
the same inputs, byte for byte.  The _dev paths are the ones the stages' own tests hold to the oracles; here only
the door's per-call device buffer is in question, so the shapes make a wrong part offset show: 3 scans in one group
(lengths and t0 12 bytes, pose2d 72: no multiple of 16), lengths that differ, 37 x 29 cells (1073, the stride padded
to 1076), a 3 x 5 x 5 score volume (300 bytes) and 5 poses.  Every output is an integer accumulated with integer
atomics, so equality is exact."""
import numpy as np
import pytest

from rplidar_ros2_driver_amd import Params, abi

pytestmark = pytest.mark.gpu

S, N = 3, 256
LENS = np.array([250, 233, 241], np.uint32)
W, H = 37, 29
CELLS, STRIDE = W * H, (W * H + 3) & ~3
ORIGIN, RES = (-0.9, -0.7), 0.05
P = 5
_INPUTS = {}


def _inputs():
    """Three rings of 0.35 .. 0.6 m around sensors a few centimetres apart, inside the 1.85 m x 1.45 m grid; the
    motion moves a scan's last sample by ~0.2 m and t0 shifts the scans against each other, so the results with and
    without them differ."""
    if _INPUTS:
        return _INPUTS
    rng = np.random.default_rng(20)
    batch = np.zeros((S, N), abi.NODE_DTYPE)
    for sc in range(S):
        n = int(LENS[sc])
        i = np.arange(n)
        batch[sc]["angle_z_q14"][:n] = (i * 65536) // n
        dist_m = 0.35 + 0.08 * sc + 0.1 * np.abs(np.sin(3.0 * np.pi * i / n))
        batch[sc]["dist_mm_q2"][:n] = (4000 * dist_m).astype(np.uint32)
        batch[sc]["quality"][:n] = 200
    th = np.array([0.0, 0.11, -0.07])
    pose2d = np.stack([np.cos(th), -np.sin(th), [-0.05, 0.0, 0.06], np.sin(th), np.cos(th), [0.02, -0.03, 0.0]],
                      axis=1).astype(np.float32)
    motion = np.array([[2.0, -1.0, 1.0, 4e-4], [-1.5, 0.5, -0.8, 4e-4], [1.0, 1.0, 0.5, 3e-4]], np.float32)
    t0 = np.array([-0.02, 0.0, 0.03], np.float32)
    field = rng.integers(-1, 101, (H, W)).astype(np.int8)
    prev = rng.integers(-1, 101, (H, W)).astype(np.int8)
    counts = rng.integers(0, 9, (H, W, 2)).astype(np.uint32)
    a = np.array([0.0, 0.05, -0.05, 0.2, -0.3])
    poses = np.stack([np.cos(a), np.sin(a), [0.0, 0.05, -0.05, 0.1, 0.0], [0.0, 0.0, 0.05, -0.1, 0.15]],
                     axis=1).astype(np.float32)
    _INPUTS.update(batch=batch, pose2d=pose2d, motion=motion, t0=t0, field=field, prev=prev, counts=counts,
                   poses=poses, pivot=np.array([0.1, -0.05], np.float32), p=Params.defaults(clip_enable=0))
    assert pose2d.nbytes == 72 and t0.nbytes == 12 and motion.nbytes == 48 and CELLS != STRIDE
    return _INPUTS


def _optional(x, given):
    """The door's keyword arguments, host side: all of motion, pose2d and t0, or none of them."""
    return dict(motion=x["motion"], pose2d=x["pose2d"], t0=x["t0"]) if given else {}


class _Dev:
    """The scans on the device and the handle's time offsets set for the length of a `with` block."""

    def __init__(self, gpu, x, given):
        import torch
        self.torch, self.dev, self.gpu = torch, torch.device("cuda:0"), gpu
        self.nodes = self.up(x["batch"].view(np.uint8).reshape(S, N * 8))
        self.lens = self.up(LENS.astype(np.int32))
        self.motion, self.pose2d, self.t0 = (self.up(x[k]) if given else None for k in ("motion", "pose2d", "t0"))

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def fill(self, words, value=0x5A5A5A5A):
        return self.torch.full((words,), value, dtype=self.torch.int32, device=self.dev)

    @staticmethod
    def ptr(t):
        return 0 if t is None else t.data_ptr()

    def scan_args(self, p):
        return (self.nodes.data_ptr(), N, self.lens.data_ptr(), S, S, p, self.ptr(self.motion), self.ptr(self.pose2d))

    def __enter__(self):
        self.gpu.set_scan_time_offsets_dev(self.ptr(self.t0))
        return self

    def __exit__(self, *exc):
        self.gpu.set_scan_time_offsets_dev(0)  # (the handle is shared)


def _occupancy(gpu, x, given):
    spec = abi.OccGrid(ORIGIN[0], ORIGIN[1], RES, W, H, 0.0, 2.0, 2.5)
    prev = x["prev"] if given else None
    grid, cells, status = gpu.occupancy_grid(x["batch"], LENS, x["p"], spec, prev=prev, **_optional(x, given))
    with _Dev(gpu, x, given) as d:
        d_prev = None if prev is None else d.up(np.pad(prev.reshape(-1), (0, STRIDE - CELLS)))
        d_grid, d_cells, d_st = d.up(np.full(STRIDE, 0x5A, np.uint8)), d.fill(3), d.fill(1)
        gpu.occupancy_grid_dev(*d.scan_args(x["p"]), spec, d.ptr(d_prev), d_grid.data_ptr(), STRIDE,
                               d_cells.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
    want = (d_grid.cpu().numpy()[:CELLS].tobytes(), d_cells.cpu().numpy().view(np.uint32).tolist(),
            int(d_st.cpu().numpy().view(np.uint32)[0]))
    print(f"occupancy given={given}: cells {cells} status {status}")
    assert (grid.tobytes(), list(cells), status) == want
    assert cells[1] > 20  # the rings are on the grid
    return grid.tobytes()


def _match(gpu, x, given):
    spec = abi.ScanMatch(ORIGIN[0], ORIGIN[1], RES, W, H, 2, 2, 1, 0.02)
    pivot = x["pivot"] if given else None
    scores, best, status = gpu.match_scans(x["batch"], LENS, x["p"], spec, x["field"], pivot=pivot,
                                           **_optional(x, given))
    volume = scores.size
    with _Dev(gpu, x, given) as d:
        d_field = d.up(np.pad(x["field"].reshape(-1), (0, STRIDE - CELLS)))
        d_pivot = None if pivot is None else d.up(pivot)
        d_scores, d_best, d_st = d.fill(volume), d.fill(8), d.fill(1)
        gpu.match_scans_dev(*d.scan_args(x["p"]), d.ptr(d_pivot), spec, d_field.data_ptr(), STRIDE, 0,
                            d_scores.data_ptr(), volume, d_best.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
    print(f"match given={given}: best {best.view(np.int32).tolist()} status {status}")
    assert volume == 75 and scores.tobytes() == d_scores.cpu().numpy().tobytes()
    assert best.tobytes() == d_best.cpu().numpy().tobytes() and status == int(d_st.cpu().numpy().view(np.uint32)[0])
    assert scores.max() > 0
    return scores.tobytes()


def _map_update(gpu, x, given):
    spec = abi.OccGrid(ORIGIN[0], ORIGIN[1], RES, W, H, 0.0, 2.0, 2.5)
    counts = x["counts"].copy()
    status = gpu.map_update(x["batch"], LENS, x["p"], spec, counts, **_optional(x, given))
    with _Dev(gpu, x, given) as d:
        d_counts, d_st = d.up(x["counts"].view(np.int32).reshape(-1)), d.fill(1)
        gpu.map_update_dev(*d.scan_args(x["p"]), spec, d_counts.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
    added = int((counts.astype(np.int64) - x["counts"]).sum())
    print(f"map_update given={given}: {added} observations added, status {status}")
    assert counts.tobytes() == d_counts.cpu().numpy().tobytes() and status == int(d_st.cpu().numpy().view(np.uint32)[0])
    assert added > 100 and (counts >= x["counts"]).all()  # the rays were ADDED to the counts that came in
    return counts.tobytes()


def _score(gpu, x, given):
    spec = abi.PoseScore(ORIGIN[0], ORIGIN[1], RES, W, H)
    weights, result, status = gpu.score_poses(x["batch"], LENS, x["p"], spec, x["poses"], x["field"],
                                              **_optional(x, given))
    with _Dev(gpu, x, given) as d:
        d_field, d_poses = d.up(np.pad(x["field"].reshape(-1), (0, STRIDE - CELLS))), d.up(x["poses"].reshape(-1))
        d_w, d_res, d_st = d.fill(P), d.fill(8), d.fill(1)
        gpu.score_poses_dev(*d.scan_args(x["p"]), spec, d_poses.data_ptr(), P, 4 * P, 0, d_field.data_ptr(), STRIDE, 0,
                            d_w.data_ptr(), P, d_res.data_ptr(), d_st.data_ptr())
        gpu.synchronize()
    print(f"score given={given}: weights {weights.tolist()} result {result.tolist()} status {status}")
    assert len(weights) == P and weights.tobytes() == d_w.cpu().numpy().tobytes()
    assert result.tobytes() == d_res.cpu().numpy().tobytes() and status == int(d_st.cpu().numpy().view(np.uint32)[0])
    assert weights.max() > 0
    return weights.tobytes()


@pytest.mark.parametrize("door", [_occupancy, _match, _map_update, _score], ids=lambda f: f.__name__.strip("_"))
def test_scan_doors_with_and_without_motion_pose_and_offsets(gpu, door):
    x = _inputs()
    with_all = door(gpu, x, True)
    with_none = door(gpu, x, False)
    assert with_all != with_none  # motion, pose2d and t0 reached the kernels
