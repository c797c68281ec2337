"""E18 (rplgpu_sample_motion_dev): one group, M in {1024, 16384, 2^20} deltas from an ordinary odometry increment
(0.25 m ahead, a turn before and after, noise of 0.05 rad and 0.02 m).  Median (min) of device-event timings of the
whole call (two launches: they are not timed apart); beside it, in the same session, what the call replaces: the host
making the same list with rplgpu_sample_motion_host on one CPU thread, and the host-to-device copy of the list (16 M
bytes, pinned memory).  The deltas and the result words of every size are checked against rplgpu_sample_motion_host.

    python tools/dev/motionbench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if
    given; RPLGPU_LIBRARY picks the library, `label` names it in the report)"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import RplGpu, abi  # noqa: E402

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
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=8)
    gpu.set_stream(stream.cuda_stream)
    odom = abi.motion_odometry(0.24, 0.07, 0.1, [0.02, 0.02, 0.006, 0.0])
    d_odom = torch.from_numpy(odom).to(dev)
    spec = abi.MotionNoise.defaults(seed=2026, step=20)
    lines = [f"E18 rplgpu_sample_motion_dev [{label}]: 1 group, odometry {odom.tolist()}, median (min) of {reps} "
             f"timings: device events around the whole call; rplgpu_sample_motion_host on one CPU thread; H2D of 16 M "
             f"bytes, pinned"]
    for M in SIZES:
        d_delta = torch.zeros(4 * M, dtype=torch.float32, device=dev)
        d_res = torch.zeros(8, dtype=torch.int32, device=dev)

        def stage():
            gpu.sample_motion_dev(d_odom.data_ptr(), 0, 1, M, spec, d_delta.data_ptr(), 4 * M, d_res.data_ptr())

        e_med, e_min = timed(stage, reps)
        gpu.synchronize()
        want, want_res = abi.sample_motion_host(odom, M, spec)
        res = d_res.cpu().numpy().view(np.uint32)
        same = d_delta.cpu().numpy().tobytes() == want.tobytes() and res.tobytes() == want_res.tobytes()
        h_med, h_min = host_timed(lambda: abi.sample_motion_host(odom, M, spec), min(reps, 5))
        pin = torch.from_numpy(want.reshape(-1)).pin_memory()
        x_med, x_min = timed(lambda: d_delta.copy_(pin, non_blocking=True), reps)
        n = 3 * M
        s = int(res[2]) | int(res[3]) << 32
        s = s - (1 << 64) if s >> 63 else s
        s2 = int(res[4]) | int(res[5]) << 32
        lines.append(f"M = {M}: {e_med:.3f} ms ({e_min:.3f}), {16 * M / (e_med * 1e-3) / 1e9:.1f} GB / s of deltas "
                     f"written; host {h_med:.3f} ms ({h_min:.3f}); the copy it replaces {x_med:.3f} ms ({x_min:.3f}); "
                     f"equal to rplgpu_sample_motion_host: {same}; mean Z {s / n:.1f}, variance {s2 / n - (s / n) ** 2:.4g}"
                     f" (2.8633e+09), max |Z| {int(res[1])}, NaN outputs {int(res[0])}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
