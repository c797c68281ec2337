"""E25 (rplgpu_refine_sums_dev, rplgpu_refine_poses_dev) beside E15 (rplgpu_score_poses_dev) on the same inputs in one
process, medians of device-event timings.  The workload is matchbench.py's: G time steps of 8 sensors x 32 000
samples, the default grid (1024 x 1024 cells of 0.05 m), the sensors on a 0.6 m circle, E5 on, 1 cm noise, the field
E11 + E12 (default inflation) of time step 0 made on the device (its top value, 100, is the target).
  (a) P = 1, the SLAM case: every time step's one pose, a little off the truth;
  (b) one time step with P = 4096 distinct poses around the truth.
Timed: E15's whole call, E25's sums call (prepare + sums + finish + best), rplgpu_refine_step_dev apart, and
rplgpu_refine_poses_dev with iters = 4.  Not timed apart: E25's prepare, finish and best launches (they are inside the
sums call's time), and E1 / E5's keep mask, which both stages queue.  E25 reads four field bytes where E15 reads one
and adds four IEEE divides and about forty integer operations per point and pose: the ratio to E15 is the figure of
merit.  Group 0 is checked against tests/refine_oracle.py in the same run (in (b) four poses of the list).

    python tools/dev/refinebench.py [G reps [out.txt]]      (prints the report; also writes it to out.txt if given)"""
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests import refine_oracle as ro  # noqa: E402
from tests.fused_oracle import group_points  # noqa: E402

S, N = 8, 32000
ITERS = 4


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
    cells = grid.width * grid.height
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=1, ror_radius=0.10,
                        ror_min_neighbors=2)
    ang = 2 * math.pi * (np.arange(B) % S) / S
    pose2d = np.stack([np.cos(ang), -np.sin(ang), 0.6 * np.cos(ang), np.sin(ang), np.cos(ang), 0.6 * np.sin(ang)],
                      1).astype(np.float32)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_len = torch.full((B,), N, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_field = torch.zeros(cells, dtype=torch.int8, device=dev)
    inflation = abi.Inflation.defaults()
    table, rc = abi.inflation_table(inflation, grid.resolution)
    d_table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    batch = synth.make_batch(2026 + 5, B, N, noise_m=0.01)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, N * 8)).to(dev)
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), grid, 0,
                           d_grid.data_ptr(), cells)
    gpu.inflate_grids_dev(d_grid.data_ptr(), cells, d_field.data_ptr(), cells, 1, grid.width, grid.height,
                          d_table.data_ptr(), rc, inflation.inflate_unknown)
    gpu.synchronize()
    field = d_field.cpu().numpy().reshape(grid.height, grid.width)
    x, y, *_ = group_points(oracle, list(batch[:S]), p, None, pose2d[:S], None)
    s = ro.spec(target=100)
    spec = ro.struct_of(s)
    score = abi.PoseScore(grid.origin_x, grid.origin_y, grid.resolution, grid.width, grid.height)
    lines = [f"E25 rplgpu_refine_*_dev beside E15: {S} scans x {N} samples a time step, field {grid.width} x "
             f"{grid.height} x {grid.resolution:.2f} m (E11 + E12 of time step 0, target 100), E5 on, 1 cm noise, median "
             f"(min) of {reps} device-event timings"]
    rng = np.random.default_rng(2900)
    for label, groups, P in ((f"(a) {G} time steps, P = 1", G, 1), ("(b) one time step, P = 4096", 1, 4096)):
        Bc = groups * S
        th = rng.uniform(-0.004, 0.004, P)
        sh = rng.uniform(-0.03, 0.03, (P, 2))
        poses = np.stack([np.cos(th), np.sin(th), sh[:, 0], sh[:, 1]], 1).astype(np.float32)
        d_poses = torch.from_numpy(poses).to(dev)
        d_out = torch.zeros(groups * 4 * P, dtype=torch.float32, device=dev)
        d_sums = torch.zeros(groups * 32 * P, dtype=torch.int32, device=dev)
        d_step = torch.zeros(groups * 4 * P, dtype=torch.int32, device=dev)
        d_scratch = torch.zeros(abi.refine_scratch_words(groups, P), dtype=torch.int32, device=dev)
        d_res = torch.zeros(groups * 8, dtype=torch.int32, device=dev)
        d_w = torch.zeros(groups * P, dtype=torch.int32, device=dev)
        d_res15 = torch.zeros(groups * 8, dtype=torch.int32, device=dev)
        d_st = torch.zeros(groups, dtype=torch.int32, device=dev)
        front = (d_nodes.data_ptr(), N, d_len.data_ptr(), Bc, S, p, 0, d_po.data_ptr())
        lst = (d_poses.data_ptr(), P, 4 * P, 0, d_field.data_ptr(), cells, 0)

        def e15():
            gpu.score_poses_dev(*front, score, *lst, d_w.data_ptr(), P, d_res15.data_ptr(), d_st.data_ptr())

        def sums():
            gpu.refine_sums_dev(*front, spec, *lst, d_sums.data_ptr(), 32 * P, d_scratch.data_ptr(), d_res.data_ptr(),
                                d_st.data_ptr())

        def step():
            gpu.refine_step_dev(d_sums.data_ptr(), 32 * P, spec, d_poses.data_ptr(), 4 * P, 0, groups, P,
                                d_out.data_ptr(), 4 * P, d_step.data_ptr(), 4 * P, d_res.data_ptr())

        def rounds():
            gpu.refine_poses_dev(*front, spec, *lst, ITERS, d_out.data_ptr(), 4 * P, d_sums.data_ptr(), 32 * P,
                                 d_step.data_ptr(), 4 * P, d_scratch.data_ptr(), d_res.data_ptr(), d_st.data_ptr())

        e_med, e_min = timed(e15, reps)
        s_med, s_min = timed(sums, reps)
        gpu.synchronize()
        got_sums = d_sums.cpu().numpy().view(np.uint32).reshape(groups, P, 32)[0]
        t_med, t_min = timed(step, reps)
        r_med, r_min = timed(rounds, reps)
        gpu.synchronize()
        pick = [0] if P == 1 else [0, 1, 1000, P - 1]
        want_sums, _, _ = ro.sums_of(x, y, poses[pick], s, field)
        same = got_sums[pick].tobytes() == want_sums.tobytes()
        if P == 1:
            wo, ws, wstep, wres, _ = ro.refine_points(x, y, poses, s, field, ITERS)
            same = same and d_out.cpu().numpy()[:4].tobytes() == wo.tobytes() and \
                d_sums.cpu().numpy().view(np.uint32)[:32].tobytes() == ws.tobytes() and \
                d_res.cpu().numpy().view(np.uint32)[:8].tobytes() == wres.tobytes()
        lines.append(f"{label}: E15 {e_med:.3f} ms ({e_min:.3f}); E25 sums {s_med:.3f} ms ({s_min:.3f}), "
                     f"{s_med / groups * 1e3:.1f} us per time step, sums / E15 = {s_med / e_med:.2f}; step apart "
                     f"{t_med:.3f} ms ({t_min:.3f}); iters = {ITERS}: {r_med:.3f} ms ({r_min:.3f}), "
                     f"{r_med / groups * 1e3:.1f} us per time step, / (4 x E15) = {r_med / (ITERS * e_med):.2f}; "
                     f"group 0 equals the oracle: {same}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
