"""Developer aid: E10 (rplgpu_filter_laserscan_batch_dev, include/rplgpu_msg.h) on a config-3-shaped LaserScan
batch — 4096 scans x 32 000 samples through rplgpu_laserscan_batch_dev in Mode A, filter defaults — timed with
device events after a warm-up (median of `reps` calls), next to a plain device copy of the same four arrays
in the same run.  The floor is 16 B per beam (ranges and intensities read and written) at 8 TB/s.
The batch is the one the tests use, synth.make_batch(2026, B, 32000, r0_range=(1, 12), noise_m=0.002), so
that both filters find work; `plain` takes the bench's own noiseless config-3 batch instead.
  python tools/dev/filterbench.py [reps=20] [scans=4096] [noisy|plain]"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
kind = sys.argv[3] if len(sys.argv) > 3 else "noisy"
n = 32000
HBM = 8.0e12
dev = torch.device("cuda:0")
kw = dict(r0_range=(1.0, 12.0), noise_m=0.002) if kind == "noisy" else {}
batch = synth.make_batch(2026, B, n, **kw)

gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=B)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
gpu.set_stream(stream.cuda_stream)

d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
d_r = torch.empty(B, n, dtype=torch.float32, device=dev)
d_i = torch.empty(B, n, dtype=torch.float32, device=dev)
d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
p = Params.defaults(range_max=40.0)
gpu.laserscan_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, p, d_r.data_ptr(), d_i.data_ptr(),
                        d_cnt.data_ptr())
gpu.synchronize()
del d_nodes
d_ro, d_io = torch.empty_like(d_r), torch.empty_like(d_i)
d_rm = torch.zeros(B, 2, dtype=torch.int32, device=dev)
beams = int(d_cnt.sum().item())


def timed(fn, k):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


def copy():
    d_ro.copy_(d_r)
    d_io.copy_(d_i)


def leg(f):
    def call():
        gpu.filter_laserscan_batch_dev(d_r.data_ptr(), d_i.data_ptr(), n, d_cnt.data_ptr(), B, p, f,
                                       d_ro.data_ptr(), d_io.data_ptr(), d_rm.data_ptr())
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t = timed(call, reps)
    return float(np.median(t)), t[0], t[-1]


res = {"workload": f"{B} scans x {n} samples ({kind}), Mode A, {beams} beams", "reps": reps}
for _ in range(3):
    copy()
torch.cuda.synchronize()
t = timed(copy, reps)
copy_ms = float(np.median(t))
# the copy moves the whole slots (B x n), the filter only the beams below each scan's count
res["copy"] = {"ms": round(copy_ms, 4), "floor_ms": round(16.0 * B * n / HBM * 1e3, 4),
               "frac_of_floor": round(16.0 * B * n / HBM * 1e3 / copy_ms, 3)}
floor_ms = 16.0 * beams / HBM * 1e3
legs = {"defaults": abi.ScanFilter.defaults(),
        "shadow_only": abi.ScanFilter.defaults(speckle_enable=0),
        "speckle_only": abi.ScanFilter.defaults(shadow_enable=0),
        "off_copy": abi.ScanFilter.defaults(shadow_enable=0, speckle_enable=0),
        "w64_n64_l64": abi.ScanFilter.defaults(shadow_window=64, shadow_neighbors=64, speckle_min_run=64)}
for name, f in legs.items():
    ms, lo, hi = leg(f)
    rm = d_rm.cpu().numpy().astype(np.int64)
    fin = int(torch.isfinite(torch.where(torch.arange(n, device=dev)[None, :] < d_cnt[:, None], d_r,
                                         torch.full_like(d_r, float("inf")))).sum().item())
    res[name] = {"ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "floor_ms": round(floor_ms, 4),
                 "frac_of_floor": round(floor_ms / ms, 3), "ratio_to_copy": round(ms / copy_ms, 3),
                 "shadow_share": round(rm[:, 0].sum() / max(fin, 1), 4),
                 "speckle_share": round(rm[:, 1].sum() / max(fin, 1), 4)}
print(json.dumps(res))
