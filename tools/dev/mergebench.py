"""Developer aid: E9 (rplgpu_merge_scans_dev, include/rplgpu_msg.h) on the bench's config-5 batch (4096 scans =
512 time steps x 8 sensors x 32 000 samples, 1 cm noise, the bench's motion and pose generator), group 8,
device events after a warm-up.  Legs: E5 on (k_ror_mask + the merge kernels) and E5 off (the merge kernels
alone), each at the given beam counts over a full circle; then the messages of one call.  The read floor is
8 B per sample + 8 B per beam of the output at 8 TB/s.
  python tools/dev/mergebench.py [reps=10] [counts=1440,16384]"""
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
counts = [int(c) for c in (sys.argv[2] if len(sys.argv) > 2 else "1440,16384").split(",")]
B, n, S = 4096, 32000, 8
T = B // S
HBM = 8.0e12
dev = torch.device("cuda:0")
batch = synth.make_batch(2026 + 5, B, n, noise_m=0.01)
rng = np.random.default_rng(2026)
motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                   for _ in range(B)]).astype(np.float32)
ang = rng.uniform(-3, 3, B)
pose2d = np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, B), np.sin(ang), np.cos(ang),
                   rng.uniform(-2, 2, B)], 1).astype(np.float32)
d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, n * 8)).to(dev)
d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
d_mo, d_po = torch.from_numpy(motion).to(dev), torch.from_numpy(pose2d).to(dev)
d_hit = torch.zeros(T, dtype=torch.int32, device=dev)
d_st = torch.zeros(T, dtype=torch.int32, device=dev)

gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=B)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
gpu.set_stream(stream.cuda_stream)


def timed(fn, k):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


res = {"workload": f"{S} sensors x {T} time steps x {n} samples, group {S}, motion + poses", "reps": reps}
for count in counts:
    m = abi.ScanMerge(-math.pi, math.pi, count, 0.0, 40.0, 0.1)
    d_r = torch.empty(T * count, dtype=torch.float32, device=dev)
    d_i = torch.empty(T * count, dtype=torch.float32, device=dev)
    floor_ms = (8.0 * B * n + 8.0 * T * count) / HBM * 1e3
    for ror in (1, 0):
        p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=ror,
                            ror_radius=0.10, ror_min_neighbors=2)

        def call():
            gpu.merge_scans_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, S, p, d_mo.data_ptr(), d_po.data_ptr(),
                                m, d_r.data_ptr(), d_i.data_ptr(), d_hit.data_ptr(), d_st.data_ptr())

        call()
        torch.cuda.synchronize()
        best = min(float(np.median(timed(call, reps))) for _ in range(2))
        res[f"count{count}_e5{'on' if ror else 'off'}"] = {
            "ms": round(best, 4), "floor_ms": round(floor_ms, 4), "frac_of_read_floor": round(floor_ms / best, 3),
            "beams_hit_mean": round(float(d_hit.float().mean().item()), 1), "status_max": int(d_st.max().item())}
    # the G messages of the last call
    lay = abi.LaserScanLayout()
    abi.load_library().rplgpu_msg_laserscan_layout(len("base_link"), count, lay)
    stride = (lay.total_len + 3) & ~3
    d_msgs = torch.empty(T * stride, dtype=torch.uint8, device=dev)
    d_ml = torch.zeros(T, dtype=torch.int32, device=dev)
    d_stamps = torch.zeros(T * 8, dtype=torch.uint8, device=dev)

    def msgs():
        gpu.merged_laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), T, m, "base_link", d_stamps.data_ptr(),
                                      d_msgs.data_ptr(), stride, d_ml.data_ptr(), 0)

    msgs()
    res[f"count{count}_msgs_ms"] = round(min(timed(msgs, reps)), 4)
print(json.dumps(res))
