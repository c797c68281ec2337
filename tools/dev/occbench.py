"""E11 (rplgpu_occupancy_grid_dev) on the config-5 shape: G time steps of 8 sensors x 32 000 samples, the
default grid (1024 x 1024 cells of 0.05 m), the sensors on a 0.6 m circle, E5 on as in config 5.  Median of
device-event timings, once on clean rings and once with 1 cm noise; a plain device fill plus copy of the same
G grids timed in the same run; cell visits per second (the visits of the spec's walk, max(|dx|, |dy|) + 1 per
ray, counted by tests/occ_oracle.py on group 0 and scaled by G).

    python tools/dev/occbench.py [G reps [out.txt]]      (prints the report; also writes it to out.txt if given)"""
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402
from tests import occ_oracle as oo  # noqa: E402
from tests import oracle_lib  # noqa: E402

S, N = 8, 32000


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


def main():
    G = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    B = G * S
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=B)
    gpu.set_stream(stream.cuda_stream)
    oracle = oracle_lib.load_oracle()
    grid = abi.OccGrid.defaults()
    spec = oo.spec()
    cells = grid.width * grid.height
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=1, ror_radius=0.10,
                        ror_min_neighbors=2)
    ang = 2 * math.pi * (np.arange(B) % S) / S
    pose2d = np.stack([np.cos(ang), -np.sin(ang), 0.6 * np.cos(ang), np.sin(ang), np.cos(ang), 0.6 * np.sin(ang)],
                      1).astype(np.float32)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_len = torch.full((B,), N, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(G * cells, dtype=torch.int8, device=dev)
    d_copy = torch.zeros(G * cells, dtype=torch.int8, device=dev)
    d_cells = torch.zeros(G * 3, dtype=torch.int32, device=dev)
    d_st = torch.zeros(G, dtype=torch.int32, device=dev)
    lines = [f"E11 rplgpu_occupancy_grid_dev: {G} groups x {S} scans x {N} samples, grid {grid.width} x {grid.height} "
             f"x {grid.resolution:.2f} m, E5 on, median (min) of {reps} device-event timings"]

    def fill_copy():
        d_grid.fill_(-1)
        d_copy.copy_(d_grid)

    for label, noise in (("clean rings", 0.0), ("1 cm noise", 0.01)):
        batch = synth.make_batch(2026 + 5, B, N, noise_m=noise)
        d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, N * 8)).to(dev)

        def stage():
            gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), B, S, p, 0, d_po.data_ptr(), grid, 0,
                                   d_grid.data_ptr(), cells, d_cells.data_ptr(), d_st.data_ptr())

        t_med, t_min = timed(stage, reps)
        f_med, f_min = timed(fill_copy, reps)
        stage()
        gpu.synchronize()
        got = d_grid[:cells].cpu().numpy().reshape(grid.height, grid.width)
        r = oo.group_rays(oracle, list(batch[:S]), p, spec, None, pose2d[:S])
        live = r["ray"] & ~r["dropped"]
        visits = int((np.maximum(np.abs(r["x1"] - r["x0"]), np.abs(r["y1"] - r["y0"]))[live] + 1).sum())
        want, _, _ = oo.grid_of_rays(r, spec)
        same = bool(np.array_equal(got, want))
        lines.append(f"{label}: stage {t_med:.3f} ms ({t_min:.3f}), fill + copy {f_med:.3f} ms ({f_min:.3f}), ratio "
                     f"{t_med / f_med:.1f} x; {visits / max(1, int(live.sum())):.0f} visits per ray, "
                     f"{visits * G / (t_med * 1e-3) / 1e9:.2f} G cell visits / s, {t_med / G * 1e3:.1f} us per time "
                     f"step; group 0 equals the oracle: {same}; cells 0 / 100 / -1 of group 0: "
                     f"{d_cells[:3].cpu().numpy().tolist()}, status {d_st.cpu().numpy().tolist()[:2]}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).write_text(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
