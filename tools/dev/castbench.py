"""E22 (rplgpu_cast_ranges_dev) on the default grid (1024 x 1024 cells of 0.05 m), N = 240 (12 m), K = 40: a room-like
map (an outer wall 40 m x 30 m, unknown outside it, partition walls with doors, pillars) with the poses spread over its
inside and every heading, and the worst case — an empty map with the poses kept 12 m from its edge, so that every ray
walks its 240 steps and ends NONE.  The beams are every (360 / A)-th beam centre of a 360-beam merged scan
(rplgpu_cast_beams), the measured scan is what pose 0 sees (the host twin), 3 cm noise.

Per shape: median (min) of device-event timings of the whole call with range words and weights, and with weights alone;
the cell steps walked (cast words 6, 7) and steps per second; rplgpu_cast_ranges_host on the first TWIN poses of the
same list, one CPU thread, compared byte for byte with the device's words and weights; and E15
(rplgpu_score_poses_dev) at the same P on one scan with as many samples as beams against the same grid as its field:
the price of the beam model against the likelihood field.

    python tools/dev/castbench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if given;
    RPLGPU_LIBRARY picks the library, `label` names it in the report)"""
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

SHAPES = (("room", 1 << 16, 60), ("room", 1 << 20, 30), ("empty", 1 << 16, 60), ("empty", 1 << 20, 30))
TWIN = 1 << 13


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


def room_map(spec):
    """unknown outside an outer wall of 800 x 600 cells, free inside, two partition walls with doors, a row of pillars"""
    g = np.full((spec.height, spec.width), -1, np.int8)
    x0, x1, y0, y1 = 112, 912, 212, 812
    g[y0:y1, x0:x1] = 0
    g[y0:y0 + 3, x0:x1] = g[y1 - 3:y1, x0:x1] = 100
    g[y0:y1, x0:x0 + 3] = g[y0:y1, x1 - 3:x1] = 100
    for x in (380, 640):
        g[y0:y1, x:x + 3] = 100
        for door in (300, 520, 700):
            g[door:door + 20, x:x + 3] = 0
    for x in range(160, 900, 60):
        g[500:504, x:x + 4] = 100
    return g


def poses_over(rng, spec, grid, P, margin_m):
    """P poses over the free cells at least margin_m from the grid's edge"""
    m = int(round(margin_m / spec.resolution))
    free = np.argwhere(grid[m:spec.height - m, m:spec.width - m] == 0) + m
    pick = free[rng.integers(0, len(free), P)]
    th = rng.uniform(-math.pi, math.pi, P)
    x = spec.origin_x + (pick[:, 1] + rng.uniform(0, 1, P)) * spec.resolution
    y = spec.origin_y + (pick[:, 0] + rng.uniform(0, 1, P)) * spec.resolution
    return np.stack([np.cos(th), np.sin(th), x, y], 1).astype(np.float32)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    label = sys.argv[3] if len(sys.argv) > 3 else "the library as built"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=4)
    gpu.set_stream(stream.cuda_stream)
    spec = abi.RangeCast.defaults()
    cells = spec.width * spec.height
    merge = abi.ScanMerge(-math.pi, math.pi, 360, 0.0, 40.0, 0.1)
    K = spec.table_half
    j = np.arange(-K, K + 1)
    table = np.concatenate([np.maximum(np.round(250.0 * np.exp(-0.5 * (j / 3.0) ** 2)), 3), [77]]).astype(np.uint8)
    p15 = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)
    score = abi.PoseScore.defaults()
    maps = {"room": room_map(spec), "empty": np.zeros((spec.height, spec.width), np.int8)}
    lines = [f"E22 rplgpu_cast_ranges_dev [{label}]: 1 group, grid {spec.width} x {spec.height} x {spec.resolution:.2f} m, "
             f"N = {spec.max_steps}, K = {K}, hit_lo {spec.hit_lo}, unknown stops; median (min) of {reps} device-event "
             f"timings of the whole call; the host twin once, on the first {TWIN} poses, one CPU thread"]
    rng = np.random.default_rng(2026)
    d_table = torch.from_numpy(table).to(dev)
    d_res = torch.zeros(8, dtype=torch.int32, device=dev)
    d_cast = torch.zeros(8, dtype=torch.int32, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, P, A in SHAPES:
        grid = maps[name]
        poses = poses_over(rng, spec, grid, P, 12.1 if name == "empty" else 0.0)
        beams = abi.cast_beams(merge, 0, 360 // A, A)
        seen, _, _, _ = abi.cast_ranges_host(poses[:1], beams, grid, spec)
        z = np.array([abi.cast_range_m(w, spec.resolution) for w in seen[0]])
        z = np.where(np.isfinite(z), np.maximum(z + rng.normal(0, 0.03, A), 0), np.inf).astype(np.float32)
        d_grid = torch.from_numpy(grid.reshape(-1)).to(dev)
        d_poses = torch.from_numpy(poses.reshape(-1)).to(dev)
        d_beams = torch.from_numpy(beams.reshape(-1)).to(dev)
        d_z = torch.from_numpy(z).to(dev)
        d_rng = torch.zeros(P * A, dtype=torch.int32, device=dev)
        d_w = torch.zeros(P, dtype=torch.int32, device=dev)

        def stage(ranges=True):
            gpu.cast_ranges_dev(spec, d_poses.data_ptr(), 4 * P, 0, 1, P, d_beams.data_ptr(), A, d_grid.data_ptr(), cells,
                                0, d_z.data_ptr(), A, 0, 1, d_table.data_ptr(), d_rng.data_ptr() if ranges else 0, P * A,
                                d_w.data_ptr(), P, d_res.data_ptr(), d_cast.data_ptr())

        t_med, t_min = timed(stage, reps)
        w_med, w_min = timed(lambda: stage(False), reps)
        stage()
        gpu.synchronize()
        cast = d_cast.cpu().numpy().view(np.uint32)
        steps = int(cast[6]) | int(cast[7]) << 32
        n = min(TWIN, P)
        t0 = time.perf_counter()
        tr, tw, _, tc = abi.cast_ranges_host(poses[:n], beams, grid, spec, z, table)
        t_twin = (time.perf_counter() - t0) * 1e3
        same = (d_rng[:n * A].cpu().numpy().view(np.uint32).tobytes() == tr.tobytes()
                and d_w[:n].cpu().numpy().view(np.uint32).tobytes() == tw.tobytes())
        twin_steps = int(tc[6]) | int(tc[7]) << 32
        # E15 at the same P: one scan of A samples on a 2 m circle, the grid as the field
        batch = synth.make_batch(2026, 1, A, noise_m=0.01, r0_range=(2.0, 2.0))
        d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(1, A * 8)).to(dev)
        d_len = torch.full((1,), A, dtype=torch.int32, device=dev)
        d_w15 = torch.zeros(P, dtype=torch.int32, device=dev)
        d_r15 = torch.zeros(8, dtype=torch.int32, device=dev)

        def e15():
            gpu.score_poses_dev(d_nodes.data_ptr(), A, d_len.data_ptr(), 1, 1, p15, 0, 0, score, d_poses.data_ptr(), P,
                                4 * P, 0, d_grid.data_ptr(), cells, 0, d_w15.data_ptr(), P, d_r15.data_ptr(),
                                d_st.data_ptr())

        s_med, s_min = timed(e15, reps)
        points = int(d_r15.cpu().numpy().view(np.uint32)[4])
        lines.append(
            f"{name} P {P} x A {A}: {t_med:.3f} ms ({t_min:.3f}), weights alone {w_med:.3f} ms ({w_min:.3f}); {steps} cell "
            f"steps ({steps / (P * A):.1f} per ray), {steps / (t_med * 1e-3) / 1e9:.1f} G steps / s; cast {cast.tolist()}, "
            f"result {d_res.cpu().numpy().view(np.uint32).tolist()}; twin on {n} poses {t_twin:.0f} ms "
            f"({twin_steps / (t_twin * 1e-3) / 1e9:.3f} G steps / s, x {P // n} for the list), equal to the device: "
            f"{same}; E15 with {points} points {s_med:.3f} ms ({s_min:.3f}): E22 / E15 = {t_med / s_med:.1f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
