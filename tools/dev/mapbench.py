"""E14 (rplgpu_map_update_dev, rplgpu_map_grid_dev, rplgpu_apply_match_dev) on the config-5 shape occbench.py
uses: G time steps of 8 sensors x 32 000 samples into ONE count map over the default grid (1024 x 1024 cells of
0.05 m), the sensors on a 0.6 m circle, E5 on.  Median of device-event timings, once on clean rings and once with
1 cm noise.  In the same session and on the same input: rplgpu_occupancy_grid_dev, the nearest existing kernel
(same front end and walk, bits instead of counts, G grids instead of one map).  The E5 mask pass and the walk are
one call and are NOT timed apart, in either stage.  Cell visits are those of the spec's walk, max(|dx|, |dy|) + 1
per ray, counted by tests/occ_oracle.py on time step 0 and scaled by G; "merged" is the share of time step 0's rays
that ride on another queue entry's weight (equal to the ray before, and not sample 0 of lanes 0 / 32).

    python tools/dev/mapbench.py [G reps [out.txt]]      (prints the report; also writes it to out.txt if given)"""
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402
from tests import map_oracle as mp  # noqa: E402
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


def merged_share(r, n_scans):
    """Rays of a group that become weight, not entries, in k_map_walk's queue."""
    rays, entries = 0, 0
    for slot in range(n_scans):
        m = np.flatnonzero((r["slot"] == slot) & r["ray"] & ~r["dropped"])
        if len(m) == 0:
            continue
        word = np.stack([r["x1"][m], r["y1"][m], r["cut"][m].astype(np.int64), r["mark"][m].astype(np.int64)], 1)
        idx = r["idx"][m]
        cont = (np.diff(idx) == 1) & (word[1:] == word[:-1]).all(1) & (idx[1:] % 64 != 0)
        rays += len(m)
        entries += len(m) - int(cont.sum())
    return 1.0 - entries / max(1, rays)


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
    d_map = torch.zeros(2 * cells, dtype=torch.int32, device=dev)
    d_grids = torch.zeros(G * cells, dtype=torch.int8, device=dev)
    d_grid = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_cells = torch.zeros(4, dtype=torch.int32, device=dev)
    d_st = torch.zeros(G, dtype=torch.int32, device=dev)
    match = abi.ScanMatch.defaults()
    d_best = torch.zeros(G * 8, dtype=torch.int32, device=dev)
    d_best.view(G, 8)[:, 6] = 1
    d_pose_out = torch.zeros(B * 6, dtype=torch.float32, device=dev)
    rule = abi.MapRule.defaults()
    lines = [f"E14 rplgpu_map_update_dev: {G} time steps x {S} scans x {N} samples into one map, grid {grid.width} x "
             f"{grid.height} x {grid.resolution:.2f} m, E5 on, median (min) of {reps} device-event timings; the E5 mask "
             f"pass and the walk are not timed apart"]
    for label, noise in (("clean rings", 0.0), ("1 cm noise", 0.01)):
        batch = synth.make_batch(2026 + 5, B, N, noise_m=noise)
        d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, N * 8)).to(dev)

        def update(b=B):
            gpu.map_update_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), b, S, p, 0, d_po.data_ptr(), grid,
                               d_map.data_ptr(), d_st.data_ptr())

        def e11():
            gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), B, S, p, 0, d_po.data_ptr(), grid, 0,
                                   d_grids.data_ptr(), cells, 0, d_st.data_ptr())

        def to_grid():
            gpu.map_grid_dev(d_map.data_ptr(), grid.width, grid.height, rule, 0, d_grid.data_ptr(), cells,
                             d_cells.data_ptr())

        def apply():
            gpu.apply_match_dev(d_best.data_ptr(), match, 0, d_po.data_ptr(), B, S, 1, d_pose_out.data_ptr(), 0)

        d_map.zero_()
        u_med, u_min = timed(update, reps)
        o_med, o_min = timed(e11, reps)
        g_med, g_min = timed(to_grid, reps)
        a_med, a_min = timed(apply, reps)
        d_map.zero_()
        update(S)
        gpu.synchronize()
        got = d_map.cpu().numpy().view(np.uint32).reshape(grid.height, grid.width, 2).astype(np.int64)
        r = oo.group_rays(oracle, list(batch[:S]), p, spec, None, pose2d[:S])
        live = r["ray"] & ~r["dropped"]
        visits = int((np.maximum(np.abs(r["x1"] - r["x0"]), np.abs(r["y1"] - r["y0"]))[live] + 1).sum())
        want, _ = mp.counts_of_rays(r, spec)
        same = bool(np.array_equal(got, want))
        lines.append(f"{label}: map update {u_med:.3f} ms ({u_min:.3f}), E11 on the same input {o_med:.3f} ms "
                     f"({o_min:.3f}), ratio {u_med / o_med:.2f} x; {visits / max(1, int(live.sum())):.0f} visits per "
                     f"ray, {visits * G / (u_med * 1e-3) / 1e9:.2f} G cell visits / s, {u_med / G * 1e3:.1f} us per "
                     f"time step; merged by weight {100.0 * merged_share(r, S):.1f} % of the rays; map grid "
                     f"{g_med * 1e3:.1f} us ({g_min * 1e3:.1f}), apply match {a_med * 1e3:.1f} us ({a_min * 1e3:.1f}); "
                     f"time step 0 equals the oracle: {same}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).write_text(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
