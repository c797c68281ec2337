"""E27 (rplgpu_rollout_dev) at a planner's own shapes, on a 1024 x 1024 costmap (a room with inflated walls) with an E26
field to a goal:

    dwb      G = 1, K = 1024 arcs, T = 32, F = 16
    mppi1    G = 1, K = 2048 control sequences of T = 56 steps from E18 on the device (M = K T), F = 1
    mppi16   the same with F = 16
    batch    G = 64 of the dwb shape (one start per group, the map shared)

Per shape: the whole call (both launches) by device events around a burst of calls, per call, the median of the
timings after a warm-up; next to it an empty-launch floor (two launches of a fill of eight words, timed the same way)
and ONE core of this machine running rplgpu_rollout_host, the library's own host twin (one group; NOT the reference
project, which plans nothing).  Group 0's output is compared with the host twin's byte for byte.

Every library runs in a fresh process of its own under its own time limit, started one after the other by the parent,
which never opens the device; a child that fails ends the run.  With a second library (the other form of the kernel,
built from tools/dev/patches/rollout_plain_r34.diff) the two alternate, ROUNDS times each: an A-B on the same device.

    python tools/dev/rolloutbench.py [out.txt [reps [other_library.so]]]    (the report is appended to out.txt)
    python tools/dev/rolloutbench.py --one LABEL REPS HOST      (one child: prints its lines; HOST 1 times the twin)"""
import math
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

N = 1024
ROUNDS = 3
BURST = 50      # calls between two events: a call is tens of microseconds
LIMIT_S = 240   # a child's time limit
SHAPES = (("dwb", 1, 1024, 32, 16, 0), ("mppi1", 1, 2048, 56, 1, 1), ("mppi16", 1, 2048, 56, 16, 1),
          ("batch", 64, 1024, 32, 16, 0))


def room_costmap():
    """Walls of a room with two inner walls and a door each, inflated by a linear decay over 12 cells."""
    g = np.zeros((N, N), np.int16)
    g[100:104, 100:924] = g[920:924, 100:924] = 100
    g[100:924, 100:104] = g[100:924, 920:924] = 100
    g[100:600, 400:404] = 100
    g[350:924, 650:654] = 100
    g[300:340, 400:404] = 0
    g[700:740, 650:654] = 0
    cost = g.copy()
    for r in range(1, 13):   # a diamond-shaped decay: good enough for a benchmark's costmap
        grown = np.zeros_like(g)
        for dy, dx in ((r, 0), (-r, 0), (0, r), (0, -r)):
            grown = np.maximum(grown, np.roll(g, (dy, dx), (0, 1)))
        cost = np.maximum(cost, np.where(grown == 100, 98 - 8 * (r - 1), 0))
    return cost.astype(np.int8)


def arcs(K, T, rng):
    from rplidar_ros2_driver_amd import abi
    v = np.stack([rng.uniform(0.0, 1.0, K), np.zeros(K), rng.uniform(-1.5, 1.5, K)], 1)
    return abi.rollout_deltas(v, 3.2 / T)


def one(label, reps, with_host):
    import torch

    from rplidar_ros2_driver_amd import RplGpu, abi
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=16)
    gpu.set_stream(stream.cuda_stream)
    cost = room_costmap()
    nav = abi.NavField.defaults(width=N, height=N)
    goal = 800 * N + 800
    field, _ = abi.nav_field_host(nav, cost, [goal])
    d_cost = torch.from_numpy(cost.reshape(-1)).to(dev)
    d_pot = torch.from_numpy(field.reshape(-1).view(np.int32)).to(dev)
    d_floor = torch.zeros(8, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(27)
    lines = [f"{label}: {abi.library_path()}"]

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BURST):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / BURST

    def floor():
        d_floor.fill_(0)
        d_floor.fill_(1)

    for name, G, K, T, F, per_step in SHAPES:
        spec = abi.Rollout.defaults(steps=T, min_steps=T // 2, a_end=1, a_min=0, a_sum=2, a_max=1)
        ang = 2 * math.pi * np.arange(F) / F
        fp = (np.stack([0.3 * np.cos(ang), 0.2 * np.sin(ang)], 1) if F > 1 else np.zeros((1, 2))).astype(np.float32)
        starts = np.stack([abi.pose_list([[-25.6 + 0.05 * (340 + 0.5 * g), -25.6 + 0.05 * (500 + g), 0.1 * g]])[0]
                           for g in range(G)])
        d_start = torch.from_numpy(starts.reshape(-1)).to(dev)
        d_fp = torch.from_numpy(fp.reshape(-1)).to(dev)
        if per_step:   # E18 on the device, M = K T
            odom = abi.motion_odometry(3.2 / T * 0.6, 0.0, 3.2 / T * 0.2, np.array([0.3, 0.3, 0.2, 0.2]))
            d_odom = torch.from_numpy(odom).to(dev)
            d_delta = torch.zeros(4 * K * T, dtype=torch.float32, device=dev)
            d_mres = torch.zeros(8, dtype=torch.int32, device=dev)
            gpu.sample_motion_dev(d_odom.data_ptr(), 0, 1, K * T, abi.MotionNoise.defaults(), d_delta.data_ptr(),
                                  4 * K * T, d_mres.data_ptr())
            gpu.synchronize()
            delta = d_delta.cpu().numpy().reshape(K, T, 4)
        else:
            delta = arcs(K, T, rng)
            d_delta = torch.from_numpy(delta.reshape(-1)).to(dev)
        d_out = torch.zeros(G * 8 * K, dtype=torch.int32, device=dev)
        d_end = torch.zeros(G * 4 * K, dtype=torch.float32, device=dev)
        d_res = torch.zeros(8 * G, dtype=torch.int32, device=dev)
        d_scr = torch.zeros(abi.rollout_scratch_words(G, K), dtype=torch.int32, device=dev)

        def call():
            gpu.rollout_dev(spec, d_start.data_ptr(), 1, d_delta.data_ptr(), delta.size, 0, per_step, d_fp.data_ptr(),
                            F, d_cost.data_ptr(), N * N, d_pot.data_ptr(), N * N, 0, G, K, d_out.data_ptr(), 8 * K,
                            d_end.data_ptr(), 4 * K, d_res.data_ptr(), d_scr.data_ptr())

        for _ in range(3):
            event_ms(call)
            event_ms(floor)
        times = [event_ms(call) for _ in range(reps)]
        floors = [event_ms(floor) for _ in range(reps)]
        t, fl = statistics.median(times), statistics.median(floors)
        res = d_res.cpu().numpy().view(np.uint32).reshape(G, 8)
        t0 = time.perf_counter()
        want = abi.rollout_host(spec, starts[0], delta, fp, cost, field)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = (d_out.cpu().numpy().view(np.uint32)[:8 * K].tobytes() == want[0].tobytes() and
                d_end.cpu().numpy()[:4 * K].tobytes() == want[1].tobytes() and res[0].tobytes() == want[2].tobytes())
        line = (f"  {name} (G {G}, K {K}, T {T}, F {F}, {'per-step' if per_step else 'arc'} deltas): {t * 1e3:.1f} us a "
                f"call (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}, {reps} timings of {BURST} calls); "
                f"empty-launch floor {fl * 1e3:.1f} us; group 0: {int(res[0, 0])} admissible, {int(res[0, 5])} blocked, "
                f"best {int(res[0, 1])}; equals the host twin: {same}")
        if with_host:
            line += (f"; rplgpu_rollout_host on one core {host_ms:.2f} ms a group, {G * host_ms / t:.0f} x the device's "
                     f"time for the {G} group(s)")
        lines.append(line)
    gpu.close()
    print("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]), sys.argv[4] == "1")
        return
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    other = sys.argv[3] if len(sys.argv) > 3 else None
    text = ["E27 rplgpu_rollout_dev: the whole call per shape, median of device-event timings over bursts of calls, one "
            "fresh process per library and round; the CPU figure is the library's host twin rplgpu_rollout_host on one "
            "core of the same machine, not the reference project"]
    runs = [("library", None)] if other is None else [("library", None), ("other form", other)] * ROUNDS
    failed = False
    for i, (label, lib) in enumerate(runs):
        env = dict(os.environ)
        if lib:
            env["RPLGPU_LIBRARY"] = str(Path(lib).resolve())
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, str(Path(__file__).resolve()), "--one",
               f"round {i // 2 + 1}, {label}" if other else label, str(reps), "1" if i == 0 else "0"]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        failed = r.returncode != 0
        if failed:  # a fault, an abort or the time limit: nothing more is started on the device
            text.append(f"{label}: child ended with status {r.returncode}; the run stops here\n{r.stderr[-2000:]}")
        else:
            text.append(r.stdout.rstrip())
        print(text[-1], flush=True)
        if failed:
            break
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[1], "a") as fh:
            fh.write("\n".join(text) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
