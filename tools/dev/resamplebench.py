"""E16 (rplgpu_resample_poses_dev) on E15-shaped weights: the weights are those rplgpu_score_poses_dev gives P poses
spread over +-5 m and every heading on one time step of posebench.py's shape (8 sensors x 32 000 samples, the E11 +
E12 field of the time step), P = M in {1024, 16384, 2^20}, plus the one-hot list at 2^20 (one pose holds all the
weight: one workgroup walks every output).  Median (min) of device-event timings of the whole call (three launches:
they are not timed apart), without a delta and with one delta per output; beside it, in the same session,
rplgpu_resample_host on one CPU thread and the device-to-host copy of the weights plus the host-to-device copy of
the new list that the call replaces (4 P + 16 M bytes, pinned memory).  The ancestors, the list and the result
words of every run are checked against rplgpu_resample_host.

    python tools/dev/resamplebench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if
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
    lines = [f"E16 rplgpu_resample_poses_dev [{label}]: 1 group, P = M, weights from rplgpu_score_poses_dev ({S} scans x "
             f"{N} samples, poses over +-5 m and every heading), median (min) of {reps} timings: device events around "
             f"the whole call; rplgpu_resample_host on one CPU thread; D2H of 4 P + H2D of 16 M bytes, pinned"]
    rng = np.random.default_rng(2026)
    for name, P in [(str(n), n) for n in SIZES] + [("one-hot", 1 << 20)]:
        M = P
        xyt = np.stack([rng.uniform(-5, 5, P), rng.uniform(-5, 5, P), rng.uniform(-math.pi, math.pi, P)], 1)
        xyt[0] = 0.0
        poses = abi.pose_list(xyt)
        d_poses = torch.from_numpy(poses.reshape(-1)).to(dev)
        d_w = torch.zeros(P, dtype=torch.int32, device=dev)
        if name == "one-hot":
            d_w[P // 3] = 12345
        else:
            gpu.score_poses_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), spec,
                                d_poses.data_ptr(), P, 4 * P, 0, d_field.data_ptr(), cells, 0, d_w.data_ptr(), P,
                                d_res15.data_ptr(), 0)
        gpu.synchronize()
        w = d_w.cpu().numpy().view(np.uint32)
        u = int(rng.integers(0, 1 << 32))
        d_u = torch.from_numpy(np.array([u], np.uint32).view(np.int32)).to(dev)
        th = rng.normal(0, 0.02, M)
        delta = np.stack([np.cos(th), np.sin(th), rng.normal(0.1, 0.01, M), rng.normal(0, 0.01, M)], 1).astype(np.float32)
        d_delta = torch.from_numpy(delta.reshape(-1)).to(dev)
        d_out = torch.zeros(4 * M, dtype=torch.float32, device=dev)
        d_anc = torch.zeros(M, dtype=torch.int32, device=dev)
        d_res = torch.zeros(8, dtype=torch.int32, device=dev)
        d_scr = torch.zeros(abi.resample_scratch_words(1, P), dtype=torch.int32, device=dev)

        def stage(with_delta):
            gpu.resample_poses_dev(d_w.data_ptr(), P, d_poses.data_ptr(), 4 * P, 0, 1, P, M, d_u.data_ptr(),
                                   d_delta.data_ptr() if with_delta else 0, M, 4 * M, 0, d_out.data_ptr(), 4 * M,
                                   d_anc.data_ptr(), M, d_res.data_ptr(), d_scr.data_ptr())

        c_med, c_min = timed(lambda: stage(False), reps)
        m_med, m_min = timed(lambda: stage(True), reps)
        gpu.synchronize()
        want = abi.resample_host(w, poses, M, u, delta)
        same = (d_out.cpu().numpy().tobytes() == want[0].tobytes() and
                d_anc.cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes() and
                d_res.cpu().numpy().view(np.uint32).tobytes() == want[2].tobytes())
        h_med, h_min = host_timed(lambda: abi.resample_host(w, poses, M, u, delta), min(reps, 5))
        pin_w = torch.zeros(P, dtype=torch.int32).pin_memory()
        pin_p = torch.from_numpy(want[0].reshape(-1).copy()).pin_memory()

        def copies():
            pin_w.copy_(d_w, non_blocking=True)
            d_out.copy_(pin_p, non_blocking=True)

        x_med, x_min = timed(copies, reps)
        res = want[2]
        s_sum = int(res[0]) | int(res[1]) << 32
        sq = int(res[2]) | int(res[3]) << 32 | int(res[4]) << 64
        lines.append(f"{name}: P = M = {P}: copy {c_med:.3f} ms ({c_min:.3f}), one delta per output {m_med:.3f} ms "
                     f"({m_min:.3f}), {M / (m_med * 1e-3) / 1e6:.0f} M outputs / s; host {h_med:.3f} ms ({h_min:.3f}); "
                     f"the copies it replaces {x_med:.3f} ms ({x_min:.3f}); equal to rplgpu_resample_host: {same}; "
                     f"{int(res[5])} weights not 0, {int(res[6])} distinct ancestors, N_eff "
                     f"{(s_sum * s_sum / sq if sq else 0.0):.1f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
