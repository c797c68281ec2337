"""E15 (rplgpu_score_poses_dev) on one time step of occbench.py's shape: 8 sensors x 32 000 samples on a 0.6 m
circle, E5 on as in config 5, the default grid (1024 x 1024 cells of 0.05 m).  The field is E11 + E12 (default
inflation) of the time step itself, made on the device.  P poses spread over +-5 m and every heading, pose 0 the
true one.  Median (min) of device-event timings of the whole call (E5 mask, prepare, score, best: the passes are
not timed apart), look-ups per second (= finite points x P / time), and next to it E13 (rplgpu_match_scans_dev) on
the same input with a window of about as many candidates; then P = 1025 and 2048 (a last tile of one pose against
two whole tiles) without E13; the first 128 weights of P = 1024 are checked against
tests/pose_oracle.py.

    python tools/dev/posebench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if given;
    RPLGPU_LIBRARY picks the library, `label` names it in the report)"""
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
from tests import pose_oracle as po  # noqa: E402

S, N = 8, 32000
POSES = (1024, 4096, 16384)
TAILS = (1025, 2048)  # a last tile of one pose, and two whole tiles beside it: what the short tile costs
WINDOWS = {1024: (3, 3, 10), 4096: (6, 6, 12), 16384: (6, 6, 48)}  # (Tx, Ty, K): 1029, 4225 and 16393 candidates


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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    label = sys.argv[3] if len(sys.argv) > 3 else "the library as built"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=S)
    gpu.set_stream(stream.cuda_stream)
    oracle = oracle_lib.load_oracle()
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
    d_res = torch.zeros(8, dtype=torch.int32, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    inflation = abi.Inflation.defaults()
    table, rc = abi.inflation_table(inflation, grid.resolution)
    d_table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), grid, 0,
                           d_grid.data_ptr(), cells)
    gpu.inflate_grids_dev(d_grid.data_ptr(), cells, d_field.data_ptr(), cells, 1, grid.width, grid.height,
                          d_table.data_ptr(), rc, inflation.inflate_unknown)
    gpu.synchronize()
    field = d_field.cpu().numpy().reshape(grid.height, grid.width)
    lines = [f"E15 rplgpu_score_poses_dev [{label}]: 1 group x {S} scans x {N} samples (1 cm noise, E5 on), field "
             f"{grid.width} x {grid.height} x {grid.resolution:.2f} m (E11 + E12 of the time step), poses over +-5 m and "
             f"every heading, median (min) of {reps} device-event timings of the whole call"]
    rng = np.random.default_rng(2026)
    for P in POSES + TAILS:
        xyt = np.stack([rng.uniform(-5, 5, P), rng.uniform(-5, 5, P), rng.uniform(-math.pi, math.pi, P)], 1)
        xyt[0] = 0.0
        poses = abi.pose_list(xyt)
        d_poses = torch.from_numpy(poses.reshape(-1)).to(dev)
        d_w = torch.zeros(P, dtype=torch.int32, device=dev)

        def stage():
            gpu.score_poses_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), spec,
                                d_poses.data_ptr(), P, 4 * P, 0, d_field.data_ptr(), cells, 0, d_w.data_ptr(), P,
                                d_res.data_ptr(), d_st.data_ptr())

        t_med, t_min = timed(stage, reps)
        stage()
        gpu.synchronize()
        res = d_res.cpu().numpy().view(np.uint32)
        points = int(res[4])
        same = "not checked"
        if P == POSES[0]:
            w, _, _ = po.score_group(oracle, list(batch), p, po.spec(), poses[:128], field, None, pose2d)
            same = str(d_w[:128].cpu().numpy().view(np.uint32).tobytes() == w.tobytes())
        if P not in WINDOWS:
            lines.append(f"P {P}: {t_med:.3f} ms ({t_min:.3f}), {points * P / (t_med * 1e-3) / 1e9:.1f} G look-ups / s")
            continue
        Tx, Ty, K = WINDOWS[P]
        match = abi.ScanMatch.defaults(shift_x=Tx, shift_y=Ty, rot_steps=K)
        volume = abi.scan_match_volume(match)
        d_scores = torch.zeros(volume, dtype=torch.int32, device=dev)
        d_best = torch.zeros(8, dtype=torch.int32, device=dev)

        def e13():
            gpu.match_scans_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), 0, match,
                                d_field.data_ptr(), cells, 0, d_scores.data_ptr(), volume, d_best.data_ptr(),
                                d_st.data_ptr())

        m_med, m_min = timed(e13, reps)
        per_pose, per_cand = t_med / (points * P), m_med / (points * volume)
        lines.append(f"P {P}: {t_med:.3f} ms ({t_min:.3f}), {points * P / (t_med * 1e-3) / 1e9:.1f} G look-ups / s "
                     f"({points} finite points); first 128 weights equal the oracle: {same}; result {res.tolist()}, status "
                     f"{d_st.cpu().numpy().tolist()}; E13 Tx {Tx} Ty {Ty} K {K} = {volume} candidates: {m_med:.3f} ms "
                     f"({m_min:.3f}), {points * volume / (m_med * 1e-3) / 1e9:.1f} G look-ups / s; per look-up E15 / "
                     f"E13 = {per_pose / per_cand:.2f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
