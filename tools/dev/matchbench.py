"""E13 (rplgpu_match_scans_dev) on occbench.py's shape: G time steps of 8 sensors x 32 000 samples, the default
grid (1024 x 1024 cells of 0.05 m) and the default window (Tx = Ty = 6, K = 10, 0.25 degrees), the sensors on a
0.6 m circle, E5 on as in config 5.  The field is E11 + E12 (default inflation) of time step 0, made on the device,
and serves every time step.  Median of device-event timings, once on clean rings and once with 1 cm noise;
look-ups per second (= finite points x volume / time); the share of samples merged by weight (at rotation 0,
counted on the host by the kernel's rule: a sample with the cell of its predecessor, except every 64th); next to
it a device read of the same field bytes once per rotation and time step — a torch reduction over a stride-0
view, whose memory traffic is up to its kernel and the caches (the field stays in L2): an indication of scale, not
a controlled floor; group 0 checked against tests/match_oracle.py.

    python tools/dev/matchbench.py [G reps [out.txt]]      (prints the report; also writes it to out.txt if given)"""
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402
from tests import match_oracle as mo  # noqa: E402
from tests import occ_oracle as oo  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests.fused_oracle import group_points  # noqa: E402

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


def merged_share(oracle, scans, p, pose2d, spec):
    """Samples the kernel folds into their predecessor's list entry at rotation 0, over the finite points."""
    x, y, _, slot, idx, _ = group_points(oracle, scans, p, None, pose2d, None)
    has, cx, cy = oo.cells_of(x, y, spec)
    near = has & (cx >= -spec["shift_x"]) & (cx < spec["width"] + spec["shift_x"]) & \
        (cy >= -spec["shift_y"]) & (cy < spec["height"] + spec["shift_y"])
    follows = (slot[1:] == slot[:-1]) & (idx[1:] == idx[:-1] + 1) & (idx[1:] % 64 != 0) & near[1:] & near[:-1] & \
        (cx[1:] == cx[:-1]) & (cy[1:] == cy[:-1])
    return float(follows.sum()) / max(1, len(x))


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
    match = abi.ScanMatch.defaults()
    spec = mo.spec()
    cells = grid.width * grid.height
    volume = abi.scan_match_volume(match)
    rots = 2 * match.rot_steps + 1
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=1, ror_radius=0.10,
                        ror_min_neighbors=2)
    ang = 2 * math.pi * (np.arange(B) % S) / S
    pose2d = np.stack([np.cos(ang), -np.sin(ang), 0.6 * np.cos(ang), np.sin(ang), np.cos(ang), 0.6 * np.sin(ang)],
                      1).astype(np.float32)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_len = torch.full((B,), N, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_field = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_scores = torch.zeros(G * volume, dtype=torch.int32, device=dev)
    d_best = torch.zeros(G * 8, dtype=torch.int32, device=dev)
    d_st = torch.zeros(G, dtype=torch.int32, device=dev)
    inflation = abi.Inflation.defaults()
    table, rc = abi.inflation_table(inflation, grid.resolution)
    d_table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    lines = [f"E13 rplgpu_match_scans_dev: {G} groups x {S} scans x {N} samples, field {grid.width} x {grid.height} x "
             f"{grid.resolution:.2f} m (E11 + E12 of time step 0), window Tx {match.shift_x} Ty {match.shift_y} K "
             f"{match.rot_steps} x {math.degrees(match.rot_step):.2f} deg = {volume} candidates, E5 on, median (min) "
             f"of {reps} device-event timings"]

    def read_field():
        return d_field.view(1, cells).expand(G * rots, cells).sum(dtype=torch.int32)

    for label, noise in (("clean rings", 0.0), ("1 cm noise", 0.01)):
        batch = synth.make_batch(2026 + 5, B, N, noise_m=noise)
        d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, N * 8)).to(dev)
        gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), grid, 0,
                               d_grid.data_ptr(), cells)
        gpu.inflate_grids_dev(d_grid.data_ptr(), cells, d_field.data_ptr(), cells, 1, grid.width, grid.height,
                              d_table.data_ptr(), rc, inflation.inflate_unknown)

        def stage():
            gpu.match_scans_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), B, S, p, 0, d_po.data_ptr(), 0, match,
                                d_field.data_ptr(), cells, 0, d_scores.data_ptr(), volume, d_best.data_ptr(),
                                d_st.data_ptr())

        t_med, t_min = timed(stage, reps)
        f_med, f_min = timed(read_field, reps)
        stage()
        gpu.synchronize()
        best = d_best.cpu().numpy().view(np.uint32).reshape(G, 8)
        points = int(best[:, 4].astype(np.int64).sum())
        field = d_field.cpu().numpy().reshape(grid.height, grid.width)
        want_vol, want_best, _ = mo.match_group(oracle, list(batch[:S]), p, spec, field, None, pose2d[:S])
        got_vol = d_scores[:volume].cpu().numpy().view(np.uint32)
        same = bool(np.array_equal(got_vol, want_vol.reshape(-1))) and \
            best[0].tobytes() == mo.best_words(want_best).tobytes()
        share = merged_share(oracle, list(batch[:S]), p, pose2d[:S], spec)
        lines.append(f"{label}: stage {t_med:.3f} ms ({t_min:.3f}), {t_med / G * 1e3:.1f} us per time step, "
                     f"{points * volume / (t_med * 1e-3) / 1e9:.1f} G look-ups / s ({points} finite points); field "
                     f"read (torch sum over a stride-0 view, cached) {G * rots} x {cells} B: {f_med:.3f} ms ({f_min:.3f}), ratio {t_med / f_med:.1f} x; "
                     f"{100 * share:.1f} % of group 0's samples merged by weight; group 0 equals the oracle: {same}; "
                     f"best of group 0 {best[0].view(np.int32).tolist()}, status {d_st.cpu().numpy().tolist()[:2]}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
