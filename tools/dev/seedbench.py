"""E19 (rplgpu_seed_poses_dev): one group, M = 2^20 poses (and 16384) over E11's default grid (1024 x 1024) with about
half the cells free in patches of 8 x 8, and over a 4096 x 4096 grid with half and with 0.02 % of its cells free, 360
headings.  Median (min) of device-event timings of the whole call (three launches: index, scan, emit); their split comes
from a kernel trace of this script taken in a run of its own (`rocprofv3 --kernel-trace --stats -- python
tools/dev/seedbench.py`), not from here.  Beside it, in the same session, what the call replaces: the grid read back
(width * height bytes, pinned), rplgpu_seed_poses_host on one CPU thread, and the host-to-device copy of the list (16 M
bytes, pinned).  The poses and the result words of every run are checked against rplgpu_seed_poses_host.

    python tools/dev/seedbench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if given;
    RPLGPU_LIBRARY picks the library, `label` names it in the report)"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import RplGpu, abi  # noqa: E402

H = 360


def patches(width, height, seed, free_share=0.5, patch=8):
    """a grid of 100s with `free_share` of its patch x patch blocks cleared to 0"""
    rng = np.random.default_rng(seed)
    coarse = np.where(rng.random((height // patch, width // patch)) < free_share, 0, 100).astype(np.int8)
    return np.kron(coarse, np.ones((patch, patch), np.int8)).astype(np.int8).reshape(-1)


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
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=8)
    gpu.set_stream(stream.cuda_stream)
    table = abi.seed_headings(H)
    d_table = torch.from_numpy(table.reshape(-1)).to(dev)
    noise = abi.MotionNoise.defaults(seed=2026, step=21)
    lines = [f"E19 rplgpu_seed_poses_dev [{label}]: 1 group, {H} headings, median (min) of {reps} timings: device events "
             f"around the whole call (index + scan + emit); D2H of the grid and H2D of 16 M bytes, pinned; "
             f"rplgpu_seed_poses_host on one CPU thread"]
    shapes = ((1024, 1024, 0.5, 1 << 14), (1024, 1024, 0.5, 1 << 20), (4096, 4096, 0.5, 1 << 20),
              (4096, 4096, 0.0002, 1 << 20))
    for width, height, share, M in shapes:
        grid = patches(width, height, width + M, share, 8 if share >= 0.01 else 1)
        spec = abi.PoseSeed.defaults(width=width, height=height, origin_x=-0.025 * width, origin_y=-0.025 * height)
        d_grid = torch.from_numpy(grid).to(dev)
        d_out = torch.zeros(4 * M, dtype=torch.float32, device=dev)
        d_res = torch.zeros(8, dtype=torch.int32, device=dev)
        d_scr = torch.zeros(abi.seed_scratch_words(1, width, height), dtype=torch.int32, device=dev)

        def stage():
            gpu.seed_poses_dev(spec, d_grid.data_ptr(), width * height, 0, d_table.data_ptr(), H, 1, M, noise,
                               d_out.data_ptr(), 4 * M, 0, 0, d_res.data_ptr(), d_scr.data_ptr())

        e_med, e_min = timed(stage, reps)
        gpu.synchronize()
        want, _, want_res = abi.seed_poses_host(grid, table, M, spec, noise)
        res = d_res.cpu().numpy().view(np.uint32)
        same = d_out.cpu().numpy().tobytes() == want.tobytes() and res.tobytes() == want_res.tobytes()
        h_med, h_min = host_timed(lambda: abi.seed_poses_host(grid, table, M, spec, noise), min(reps, 3))
        pin_grid = torch.empty(width * height, dtype=torch.int8).pin_memory()
        g_med, g_min = timed(lambda: pin_grid.copy_(d_grid, non_blocking=True), reps)
        pin = torch.from_numpy(want.reshape(-1)).pin_memory()
        x_med, x_min = timed(lambda: d_out.copy_(pin, non_blocking=True), reps)
        lines.append(f"{width} x {height}, F = {int(res[0])}, M = {M}: {e_med:.3f} ms ({e_min:.3f}), "
                     f"{M / (e_med * 1e-3) / 1e9:.2f} G poses / s; replaces the grid read back {g_med:.3f} ms "
                     f"({g_min:.3f}) + host {h_med:.3f} ms ({h_min:.3f}) + the list copied up {x_med:.3f} ms "
                     f"({x_min:.3f}); scratch {4 * d_scr.numel() / 1e6:.2f} MB; equal to rplgpu_seed_poses_host: {same}; "
                     f"OFF-CELL {int(res[1])}, cells {int(res[2])} .. {int(res[3])}, flags {int(res[7])}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
