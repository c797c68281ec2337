"""E23 (rplgpu_score_poses_agree_dev) beside E15 (rplgpu_score_poses_dev) in the same process on the same inputs: one
group of one scan of N = 240 returns (AMCL's beam counts: a few hundred at most enter its sensor update) over the
default grid (1024 x 1024 cells of 0.05 m), P = 2^16 and 2^20 poses.  The map is a 20 m x 16 m room, its field
max(0, 100 - 12 d) with d the distance to the wall in cells; the scan is what the origin sees, 1 cm noise.  Regimes:
  person    24 of the 240 returns come from something 0.3 m in front of the wall that the map does not hold (the field
            is 28 there, below agree_lo 40); poses within 5 cm and
            0.02 rad of the truth (some samples are skipped, no fallback);
  no_skip   the plain scan, the same poses (nothing is skipped, the apply pass lists nothing);
  fallback  the person's scan, poses over +-8 m and every heading (the group falls back, the apply pass returns).
Per regime and P: median (min) of device-event timings of the whole call of both stages, their ratio, the agree words,
and whether the weights are those the agree words promise (E15's on a fallback or with nothing skipped).

    python tools/dev/agreebench.py [reps [out.txt [label [regime P]]]]   (prints the report; also appends it to
    out.txt if given; RPLGPU_LIBRARY picks the library, `label` names it; regime and P run one shape alone — for a
    kernel trace)"""
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import Params, RplGpu, abi  # noqa: E402

N = 240
POSES = (1 << 16, 1 << 20)
REGIMES = ("person", "no_skip", "fallback")
HALF = (10.0, 8.0)  # the room's half sides [m]


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


def room_field(spec):
    xs = spec.origin_x + (np.arange(spec.width) + 0.5) * spec.resolution
    ys = spec.origin_y + (np.arange(spec.height) + 0.5) * spec.resolution
    X, Y = np.meshgrid(xs, ys)
    dx, dy = np.abs(X) - HALF[0], np.abs(Y) - HALF[1]
    outside = np.hypot(np.maximum(dx, 0), np.maximum(dy, 0))
    inside = np.minimum(np.maximum(dx, dy), 0)
    d = np.abs(outside + inside) / spec.resolution
    return np.clip(100.0 - 12.0 * d, 0, 100).astype(np.int8)


def room_scan(rng, person):
    th = 2 * math.pi * np.arange(N) / N
    with np.errstate(divide="ignore"):
        r = np.minimum(HALF[0] / np.abs(np.cos(th)), HALF[1] / np.abs(np.sin(th)))
    r = r + rng.normal(0, 0.01, N)
    if person:
        r[100:124] -= 0.3
    nodes = np.zeros((1, N), abi.NODE_DTYPE)
    nodes["angle_z_q14"] = np.round(th / (2 * math.pi) * 65536).astype(np.int64) % 65536
    nodes["dist_mm_q2"] = np.round(r * 4000.0).astype(np.int64)
    nodes["quality"] = 200
    return nodes


def pose_lists(rng, regime, P):
    if regime == "fallback":
        xyt = np.stack([rng.uniform(-8, 8, P), rng.uniform(-6, 6, P), rng.uniform(-math.pi, math.pi, P)], 1)
    else:
        xyt = np.stack([rng.uniform(-0.05, 0.05, P), rng.uniform(-0.05, 0.05, P), rng.uniform(-0.02, 0.02, P)], 1)
    xyt[0] = 0.0
    return abi.pose_list(xyt)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    label = sys.argv[3] if len(sys.argv) > 3 else "the library as built"
    shapes = [(sys.argv[4], int(sys.argv[5]))] if len(sys.argv) > 5 else [(r, P) for P in POSES for r in REGIMES]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=8)
    gpu.set_stream(stream.cuda_stream)
    spec = abi.BeamAgree.defaults(agree_lo=40)
    e15 = abi.PoseScore.defaults()
    cells = spec.width * spec.height
    p = Params.defaults(clip_enable=0)
    d_field = torch.from_numpy(room_field(spec).reshape(-1)).to(dev)
    d_len = torch.full((1,), N, dtype=torch.int32, device=dev)
    words = (N + 31) // 32
    d_counts = torch.zeros(N, dtype=torch.int32, device=dev)
    d_mask = torch.zeros(words, dtype=torch.int32, device=dev)
    d_res, d_res15, d_agree = (torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(3))
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    lines = [f"E23 rplgpu_score_poses_agree_dev beside E15 rplgpu_score_poses_dev [{label}]: 1 group x 1 scan x {N} "
             f"samples (1 cm noise), field {spec.width} x {spec.height} x {spec.resolution:.2f} m (a 20 m x 16 m room), "
             f"agree_lo {spec.agree_lo}, keep {spec.keep_num} / {spec.keep_den}, err {spec.err_num} / {spec.err_den}; "
             f"median (min) of {reps} device-event timings of the whole call, both stages in this process"]
    for regime, P in shapes:
        rng = np.random.default_rng(2600 + P % 1000)
        nodes = room_scan(rng, regime != "no_skip")
        d_nodes = torch.from_numpy(nodes.view(np.uint8).reshape(1, N * 8)).to(dev)
        d_poses = torch.from_numpy(pose_lists(rng, regime, P).reshape(-1)).to(dev)
        d_w = torch.zeros(P, dtype=torch.int32, device=dev)
        d_w15 = torch.zeros(P, dtype=torch.int32, device=dev)

        def agree():
            gpu.score_poses_agree_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), 1, 1, p, 0, 0, spec, d_poses.data_ptr(),
                                      P, 4 * P, 0, d_field.data_ptr(), cells, 0, d_w.data_ptr(), P, d_res.data_ptr(),
                                      d_st.data_ptr(), d_counts.data_ptr(), N, d_mask.data_ptr(), words,
                                      d_agree.data_ptr())

        def score():
            gpu.score_poses_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), 1, 1, p, 0, 0, e15, d_poses.data_ptr(), P,
                                4 * P, 0, d_field.data_ptr(), cells, 0, d_w15.data_ptr(), P, d_res15.data_ptr(),
                                d_st.data_ptr())

        s_med, s_min = timed(score, reps)
        a_med, a_min = timed(agree, reps)
        gpu.synchronize()
        agr = d_agree.cpu().numpy().view(np.uint32)
        F, K, back = int(agr[0]), int(agr[1]), int(agr[2])
        same = bool((d_w == d_w15).all().item())
        lower = bool((d_w.cpu().numpy().view(np.uint32) <= d_w15.cpu().numpy().view(np.uint32)).all())
        promise = same if (back or K == F) else (lower and not same)
        lines.append(f"{regime} P {P}: E23 {a_med:.3f} ms ({a_min:.3f}), E15 {s_med:.3f} ms ({s_min:.3f}), E23 / E15 = "
                     f"{a_med / s_med:.2f}; {F * P / (a_med * 1e-3) / 1e9:.1f} G look-ups / s; agree words "
                     f"{agr.tolist()} (skipped share {(F - K) / max(F, 1):.3f}); weights as the agree words promise: "
                     f"{promise}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2 and sys.argv[2] != "-":
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
