"""E17 (rplgpu_estimate_poses_dev) on E15's weights: the weights are those rplgpu_score_poses_dev gives P poses spread
over +-5 m and every heading on one time step of posebench.py's shape (8 sensors x 32 000 samples, the E11 + E12 field
of the time step), the centre is E15's result word 1 (d_center = d_result + 1, center_stride 8), the default spec,
P in {1024, 16384, 2^20}.  Median (min) of device-event timings of the whole call (two launches: they are not timed
apart); beside it, in the same session, rplgpu_estimate_host on one CPU thread and the device-to-host copies of the
list and its weights that the call replaces (20 P bytes, pinned memory).  The 72 result words of every run are
checked against rplgpu_estimate_host.

    python tools/dev/estimatebench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if
    given; RPLGPU_LIBRARY picks the library, `label` names it in the report)"""
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402

S, N = 8, 32000
SIZES = (1024, 16384, 1 << 20)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def host_timed(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    label = sys.argv[3] if len(sys.argv) > 3 else "the library as built"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=S)
    gpu.set_stream(stream.cuda_stream)
    grid = abi.OccGrid.defaults()
    spec = abi.PoseScore.defaults()
    est = abi.PoseEstimate.defaults()
    cells = grid.width * grid.height
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=1, ror_radius=0.10,
                        ror_min_neighbors=2)
    ang = 2 * math.pi * np.arange(S) / S
    pose2d = np.stack([np.cos(ang), -np.sin(ang), 0.6 * np.cos(ang), np.sin(ang), np.cos(ang), 0.6 * np.sin(ang)],
                      1).astype(np.float32)
    batch = synth.make_batch(2026 + 5, S, N, noise_m=0.01)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(S, N * 8)).to(dev)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_len = torch.full((S,), N, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_field = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_res15 = torch.zeros(8, dtype=torch.int32, device=dev)
    inflation = abi.Inflation.defaults()
    table, rc = abi.inflation_table(inflation, grid.resolution)
    d_table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), grid, 0,
                           d_grid.data_ptr(), cells)
    gpu.inflate_grids_dev(d_grid.data_ptr(), cells, d_field.data_ptr(), cells, 1, grid.width, grid.height,
                          d_table.data_ptr(), rc, inflation.inflate_unknown)
    gpu.synchronize()
    lines = [f"E17 rplgpu_estimate_poses_dev [{label}]: 1 group, weights and centre from rplgpu_score_poses_dev ({S} "
             f"scans x {N} samples, poses over +-5 m and every heading), the default spec, median (min) of {reps} "
             f"timings: device events around the whole call; rplgpu_estimate_host on one CPU thread; D2H of 20 P bytes, "
             f"pinned"]
    rng = np.random.default_rng(2026)
    for P in SIZES:
        xyt = np.stack([rng.uniform(-5, 5, P), rng.uniform(-5, 5, P), rng.uniform(-math.pi, math.pi, P)], 1)
        xyt[0] = 0.0
        poses = abi.pose_list(xyt)
        d_poses = torch.from_numpy(poses.reshape(-1)).to(dev)
        d_w = torch.zeros(P, dtype=torch.int32, device=dev)
        gpu.score_poses_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), spec,
                            d_poses.data_ptr(), P, 4 * P, 0, d_field.data_ptr(), cells, 0, d_w.data_ptr(), P,
                            d_res15.data_ptr(), 0)
        gpu.synchronize()
        w = d_w.cpu().numpy().view(np.uint32)
        center = int(d_res15.cpu().numpy().view(np.uint32)[1])
        d_res = torch.zeros(abi.ESTIMATE_WORDS, dtype=torch.int32, device=dev)
        d_scr = torch.zeros(abi.estimate_scratch_words(1, P), dtype=torch.int32, device=dev)

        def stage(weighted=True):
            gpu.estimate_poses_dev(d_poses.data_ptr(), 4 * P, 0, d_w.data_ptr() if weighted else 0, P, 1, P, est,
                                   d_res15.data_ptr() + 4, 8, d_res.data_ptr(), d_scr.data_ptr())

        n_med, n_min = timed(lambda: stage(False), reps)
        e_med, e_min = timed(stage, reps)
        gpu.synchronize()
        want = abi.estimate_host(poses, w, est, center)
        same = d_res.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()
        h_med, h_min = host_timed(lambda: abi.estimate_host(poses, w, est, center), min(reps, 5))
        pin_w = torch.zeros(P, dtype=torch.int32).pin_memory()
        pin_p = torch.zeros(4 * P, dtype=torch.float32).pin_memory()

        def copies():
            pin_w.copy_(d_w, non_blocking=True)
            pin_p.copy_(d_poses, non_blocking=True)

        x_med, x_min = timed(copies, reps)
        a, g = abi.estimate_pose(want, est.xy_scale, 0), abi.estimate_pose(want, est.xy_scale, 1)
        lines.append(f"P = {P}: {e_med:.3f} ms ({e_min:.3f}), {20 * P / (e_med * 1e-3) / 1e9:.1f} GB / s of poses and "
                     f"weights; weights NULL {n_med:.3f} ms ({n_min:.3f}); host {h_med:.3f} ms ({h_min:.3f}); the copies "
                     f"it replaces {x_med:.3f} ms ({x_min:.3f}); equal to rplgpu_estimate_host: {same}; centre "
                     f"{int(want[1])}, {int(want[2])} in range, {int(want[4])} in the gate; all: ({a[0]:.3f}, {a[1]:.3f}) "
                     f"R {a[6]:.3f}; gate: ({g[0]:.3f}, {g[1]:.3f}) heading {g[2]:.3f} R {g[6]:.3f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
