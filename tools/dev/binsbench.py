"""E20 (rplgpu_bin_poses_dev): one group, the default bins (103 x 103 of 0.5 m) with 36 heading bins, P = 16384 and
2^20, for three lists — SPREAD (an E19 list over a grid whose cells are all free), CONVERGED (an E16 output: that list
resampled by weights that are not 0 only in a box of 0.6 m and one heading, fewer than 10 bins) and ONE BIN (copies of
one pose) — and P = 2^20 spread over NB = 2^26 bins (256 x 256 x 1024), where the clear dominates.  Median, minimum
and maximum of device-event timings of the whole call (two launches: clear and start, mark).  Beside it, in the same
session, what the call replaces: the list read back (16 P bytes, pinned) and rplgpu_bin_poses_host on one CPU thread.
The map and the result words of every run are checked against rplgpu_bin_poses_host.

THE CONDITION the stage is held to, against its own other row: at P = 2^20 the one-bin and the converged list must not
take longer than the spread list by more than that session's run-to-run spread (maximum - minimum) of the spread list;
otherwise the marks serialise on their few map words.  The last line says whether it holds.

    python tools/dev/binsbench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if given;
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

T = 36


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
    return statistics.median(out), min(out), max(out)


def host_timed(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out)


def lists(P, table):
    """-> {name: (P, 4) float32}: spread, converged, one bin"""
    seed = abi.PoseSeed.defaults()
    grid = np.zeros(seed.width * seed.height, np.int8)
    spread = abi.seed_poses_host(grid, table, P, seed, abi.MotionNoise.defaults(seed=2026, step=22))[0]
    near = (np.abs(spread[:, 2] - 3.3) < 0.3) & (np.abs(spread[:, 3] + 7.1) < 0.3)
    near &= (spread[:, 0] == table[5, 0]) & (spread[:, 1] == table[5, 1])
    if not near.any():                                       # (a short list: the poses nearest the box's centre)
        near[np.argsort(np.hypot(spread[:, 2] - 3.3, spread[:, 3] + 7.1))[:4]] = True
    converged = abi.resample_host(near.astype(np.uint32), spread, P, 0x9E3779B9)[0]
    one = np.repeat(spread[:1], P, axis=0)
    return dict(spread=spread, converged=converged, one_bin=one)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    label = sys.argv[3] if len(sys.argv) > 3 else "the library as built"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=8)
    gpu.set_stream(stream.cuda_stream)
    lines = [f"E20 rplgpu_bin_poses_dev [{label}]: 1 group, median (min .. max) of {reps} timings: device events around "
             f"the whole call (clear and start + mark); D2H of 16 P bytes, pinned; rplgpu_bin_poses_host on one CPU "
             f"thread"]
    rows = []
    for P in (1 << 14, 1 << 20):
        table = abi.seed_headings(T)
        for name, poses in lists(P, table).items():
            rows.append((name, abi.PoseBins.defaults(), table, poses))
    rng = np.random.default_rng(22)
    wide = abi.seed_headings(1024)
    a = rng.uniform(0, 2 * np.pi, 1 << 20)
    xy = rng.uniform(-64.0, 64.0, (2, 1 << 20))
    rows.append(("spread", abi.PoseBins.defaults(origin_x=-64.0, origin_y=-64.0, nx=256, ny=256), wide,
                 np.stack([np.cos(a), np.sin(a), xy[0], xy[1]], axis=1).astype(np.float32)))
    med = {}
    for name, spec, table, poses in rows:
        P, nT = len(poses), len(table)
        words = abi.bin_map_words(spec.nx, spec.ny, nT)
        d_p = torch.from_numpy(poses.reshape(-1)).to(dev)
        d_e = torch.from_numpy(table.reshape(-1)).to(dev)
        d_m = torch.zeros(words, dtype=torch.int32, device=dev)
        d_r = torch.zeros(8, dtype=torch.int32, device=dev)

        def stage():
            gpu.bin_poses_dev(spec, d_p.data_ptr(), 4 * P, 0, 0, 0, 1, P, d_e.data_ptr(), nT, d_m.data_ptr(), words, 0, 0,
                              d_r.data_ptr())

        e_med, e_min, e_max = timed(stage, reps)
        gpu.synchronize()
        want_map, _, want_res = abi.bin_poses_host(poses, table, None, spec)
        res = d_r.cpu().numpy().view(np.uint32)
        got_map = d_m.cpu().numpy().view(np.uint32)[:len(want_map)]
        same = got_map.tobytes() == want_map.tobytes() and res.tobytes() == want_res.tobytes()
        h_med, h_min = host_timed(lambda: abi.bin_poses_host(poses, table, None, spec), min(reps, 3))
        pin = torch.empty(4 * P, dtype=torch.float32).pin_memory()
        x_med, x_min, _ = timed(lambda: pin.copy_(d_p, non_blocking=True), reps)
        nb = spec.nx * spec.ny * nT
        med[(name, P, nb)] = (e_med, e_min, e_max)
        lines.append(f"{name}, NB = {nb}, P = {P}: {e_med:.4f} ms ({e_min:.4f} .. {e_max:.4f}), "
                     f"{P / (e_med * 1e-3) / 1e9:.2f} G poses / s; K = {int(res[0])}, counted {int(res[1])}, out of range "
                     f"{int(res[2])}; replaces the list read back {x_med:.3f} ms ({x_min:.3f}) + host {h_med:.3f} ms "
                     f"({h_min:.3f}); map {4 * words / 1e6:.2f} MB; equal to rplgpu_bin_poses_host: {same}; "
                     f"next list by rplgpu_kld_samples: {abi.kld_samples(int(res[0]))}")
    nb = 103 * 103 * T
    s_med, s_min, s_max = med[("spread", 1 << 20, nb)]
    for name in ("converged", "one_bin"):
        m = med[(name, 1 << 20, nb)][0]
        lines.append(f"the condition at P = 2^20, {name}: {m:.4f} ms <= spread {s_med:.4f} ms + its run-to-run spread "
                     f"{s_max - s_min:.4f} ms: {m <= s_med + (s_max - s_min)}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
