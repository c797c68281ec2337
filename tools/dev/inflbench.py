"""E12 (rplgpu_inflate_grids_dev) on E11's benchmark shape: G time steps of the default grid (1024 x 1024 cells
of 0.05 m), the grids E11 makes of occbench.py's inputs (8 sensors x 32 000 samples on a 0.6 m circle, 1 cm
noise, E5 on), inflated with the defaults (Rc 12) and with a 3.2 m inflation radius (Rc 64).  Median of
device-event timings next to a plain device copy of the same grids timed in the same run — the floor: 2 B per
cell — the ratio to it, and the share of 64 x 64 tiles whose window holds no lethal cell (the early exit).
Grid 0 is checked against tests/inflate_oracle.py.

    python tools/dev/inflbench.py [G reps [out.txt]]      (prints the report; also writes it to out.txt if given)"""
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from occbench import N, S, timed  # noqa: E402
from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402
from tests import inflate_oracle as io  # noqa: E402

TILE = 64


def empty_tile_share(grid, rc):
    """Share of TILE x TILE output tiles of `grid` whose (TILE + 2 rc)^2 window holds no lethal cell."""
    L = np.pad(io.lethal(grid), rc)
    H, W = grid.shape
    n = empty = 0
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            n += 1
            empty += not L[ty:ty + TILE + 2 * rc, tx:tx + TILE + 2 * rc].any()
    return empty / n


def main():
    G = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    B = G * S
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=B)
    gpu.set_stream(stream.cuda_stream)
    grid = abi.OccGrid.defaults()
    W, H = grid.width, grid.height
    cells = W * H
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=1, ror_radius=0.10,
                        ror_min_neighbors=2)
    ang = 2 * math.pi * (np.arange(B) % S) / S
    pose2d = np.stack([np.cos(ang), -np.sin(ang), 0.6 * np.cos(ang), np.sin(ang), np.cos(ang), 0.6 * np.sin(ang)],
                      1).astype(np.float32)
    batch = synth.make_batch(2026 + 5, B, N, noise_m=0.01)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, N * 8)).to(dev)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_len = torch.full((B,), N, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(G * cells, dtype=torch.int8, device=dev)
    d_cost = torch.zeros(G * cells, dtype=torch.int8, device=dev)
    d_cells = torch.zeros(G * 4, dtype=torch.int32, device=dev)
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), B, S, p, 0, d_po.data_ptr(), grid, 0,
                           d_grid.data_ptr(), cells, 0, 0)
    gpu.synchronize()
    host = d_grid.cpu().numpy().reshape(G, H, W)
    lines = [f"E12 rplgpu_inflate_grids_dev: {G} grids of {W} x {H} x {grid.resolution:.2f} m (E11 of {S} scans x {N} "
             f"samples each, 1 cm noise, E5 on; {int(io.lethal(host[0]).sum())} lethal cells in grid 0), median (min) "
             f"of {reps} device-event timings"]

    def copy():
        d_cost.copy_(d_grid)

    c_med, c_min = timed(copy, reps)
    lines.append(f"plain device copy of the {G} grids (2 B per cell): {c_med:.3f} ms ({c_min:.3f}), "
                 f"{2 * G * cells / (c_med * 1e-3) / 1e12:.2f} TB/s")
    for label, f in (("defaults", abi.Inflation.defaults()),
                     ("Rc 64", abi.Inflation.defaults(inscribed_radius=0.3, inflation_radius=3.2,
                                                      cost_scaling_factor=1.0))):
        table, rc = abi.inflation_table(f, grid.resolution)
        d_table = torch.from_numpy(table).to(dev)

        def stage():
            gpu.inflate_grids_dev(d_grid.data_ptr(), cells, d_cost.data_ptr(), cells, G, W, H, d_table.data_ptr(),
                                  rc, f.inflate_unknown, d_cells.data_ptr())

        t_med, t_min = timed(stage, reps)
        stage()
        gpu.synchronize()
        got = d_cost[:cells].cpu().numpy().reshape(H, W)
        want, wc = io.inflate(host[0], table, rc, f.inflate_unknown)
        same = bool(np.array_equal(got, want)) and tuple(d_cells[:4].cpu().numpy().tolist()) == wc
        share = float(np.mean([empty_tile_share(host[g], rc) for g in range(G)]))
        lines.append(f"{label} (Rc {rc}): stage {t_med:.3f} ms ({t_min:.3f}), ratio to the copy {t_med / c_med:.1f} x, "
                     f"{t_med / G * 1e3:.1f} us per grid, {G * cells / (t_med * 1e-3) / 1e9:.1f} G cells / s; "
                     f"{100 * share:.1f} % of the tiles leave early; grid 0 equals the oracle: {same}; cells "
                     f"100 / 99 / 1..98 / -1 of grid 0: {d_cells[:4].cpu().numpy().tolist()}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
