"""E26 (rplgpu_nav_field_dev) on costmaps of 1024 x 1024 and 4096 x 4096 cells, one goal each: an empty map, a room
map (occbench.py's scene — 8 sensors x 32 000 samples on a 0.6 m circle, 1 cm noise, E5 on — through E11 and E12 on
the device, the same scene at 0.05 m and at 0.0125 m a cell) and a serpentine (walls every size / 64 rows with a gap at
alternating ends, so a least path crosses every tile column once per corridor).

Per map: the time to a finished field from scratch, (a) with the default rounds per call, resumed until finished, as
a caller who knows nothing about the map gets it, and (b) with the number of rounds the map needs known from a run
before — device events around the calls, resumed calls and their synchronisations included, the median of the timings
— the rounds that had a dirty tile and the tile visits; next to it, timed in the same run, a
plain device fill + copy of the potential plane (the floor: the field must be written once) and ONE core of this
machine running rplgpu_nav_field_host, the library's own host twin (a binary-heap Dijkstra; NOT the reference project,
which plans nothing).  The finished field is compared with the host twin's word for word.

Every (map, size) runs in a fresh process of its own under its own time limit, started one after the other by the
parent, which never opens the device; a child that fails ends the run.

    python tools/dev/navbench.py [out.txt [reps [size]]]      (size: 1024 or 4096 alone; the report is appended to out.txt)
    python tools/dev/navbench.py --one MAP SIZE REPS      (one child: prints its lines)"""
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
sys.path.insert(0, str(Path(__file__).resolve().parent))

MAPS = ("empty", "room", "serpentine")
SIZES = (1024, 4096)
LIMIT_S = {1024: 150, 4096: 420}  # a child's time limit: the host twin on 16 M cells alone takes many seconds


def serpentine(n):
    g = np.zeros((n, n), np.int8)
    pitch = n // 64
    for i, y in enumerate(range(pitch - 1, n - 1, pitch)):
        g[y, :] = 100
        if i % 2 == 0:
            g[y, n - 3:] = 0
        else:
            g[y, :3] = 0
    return g


def room_costmap(gpu, torch, n):
    """occbench.py's scene through E11 and E12 on the device, n x n cells over the default grid's 51.2 m."""
    from occbench import N, S
    from rplidar_ros2_driver_amd import Params, abi, synth
    dev = torch.device("cuda:0")
    res = 51.2 / n
    grid = abi.OccGrid.defaults(width=n, height=n, resolution=res)
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=1, ror_radius=0.10,
                        ror_min_neighbors=2)
    ang = 2 * math.pi * np.arange(S) / S
    pose2d = np.stack([np.cos(ang), -np.sin(ang), 0.6 * np.cos(ang), np.sin(ang), np.cos(ang), 0.6 * np.sin(ang)],
                      1).astype(np.float32)
    batch = synth.make_batch(2026 + 5, S, N, noise_m=0.01)
    d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(S, N * 8)).to(dev)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_len = torch.full((S,), N, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(n * n, dtype=torch.int8, device=dev)
    d_cost = torch.zeros(n * n, dtype=torch.int8, device=dev)
    gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), grid, 0,
                           d_grid.data_ptr(), n * n, 0, 0)
    f = abi.Inflation.defaults()
    table, rc = abi.inflation_table(f, res)
    d_table = torch.from_numpy(table).to(dev)
    gpu.inflate_grids_dev(d_grid.data_ptr(), n * n, d_cost.data_ptr(), n * n, 1, n, n, d_table.data_ptr(), rc,
                          f.inflate_unknown, 0)
    gpu.synchronize()
    return d_cost.cpu().numpy().reshape(n, n), rc


def one(name, n, reps):
    import torch

    from rplidar_ros2_driver_amd import RplGpu, abi
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=16)
    gpu.set_stream(stream.cuda_stream)
    note = ""
    if name == "empty":
        cost = np.zeros((n, n), np.int8)
    elif name == "serpentine":
        cost = serpentine(n)
    else:
        cost, rc = room_costmap(gpu, torch, n)
        note = f" (E11 + E12 on the device, Rc {rc}, {int((cost >= 99).sum())} impassable and {int((cost < 0).sum())} unknown cells)"
    goal = (n // 2) * n + n // 2 if name != "serpentine" else 0
    cells = n * n
    spec = abi.NavField.defaults(width=n, height=n, rounds=abi.NAV_MAX_ROUNDS)
    t0 = time.perf_counter()
    want, wres = abi.nav_field_host(spec, cost, [goal])
    host_ms = (time.perf_counter() - t0) * 1e3
    d_cost = torch.from_numpy(cost.reshape(-1)).to(dev)
    d_goal = torch.tensor([goal], dtype=torch.int32, device=dev)
    d_n = torch.ones(1, dtype=torch.int32, device=dev)
    d_pot = torch.zeros(cells, dtype=torch.int32, device=dev)
    d_copy = torch.zeros(cells, dtype=torch.int32, device=dev)
    d_scr = torch.zeros(abi.nav_field_scratch_words(spec, 1), dtype=torch.int32, device=dev)
    d_res = torch.zeros(8, dtype=torch.int32, device=dev)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def floor():
        d_pot.fill_(-1)
        d_copy.copy_(d_pot)

    floor()
    torch.cuda.synchronize()
    floor_ms = statistics.median(event_ms(floor)[0] for _ in range(reps))
    lines = [f"{name} {n} x {n}{note}: goal cell {goal}, {int(wres[4])} cells in reach, greatest D {int(wres[5])}; "
             f"fill + copy of the plane {floor_ms:.3f} ms; rplgpu_nav_field_host on one core {host_ms:.0f} ms"]

    def field(rounds):
        """From scratch to finished: -> (calls, rounds with a dirty tile, tile visits)."""
        spec.rounds = rounds
        calls = dirty_rounds = visits = 0
        while True:
            gpu.nav_field_dev(spec, d_cost.data_ptr(), cells, 1, d_goal.data_ptr(), 1, d_n.data_ptr(),
                              d_pot.data_ptr(), cells, d_scr.data_ptr(), 1 if calls else 0, d_res.data_ptr())
            gpu.synchronize()
            r = d_res.cpu().numpy().view(np.uint32)
            calls, dirty_rounds, visits = calls + 1, dirty_rounds + int(r[7]), visits + int(r[6])
            if r[0] == 0 or calls == 64:
                return calls, dirty_rounds, visits, int(r[0])

    form = os.environ.get("RPLGPU_NAV_SWEEP", "directional")  # (plain: only with tools/dev/patches/nav_plain_sweeps_r33.diff)
    default = abi.nav_field_default_rounds(n, n)
    _, (calls, need, visits, left) = event_ms(lambda: field(abi.NAV_MAX_ROUNDS))  # how many rounds it takes
    n_rep = reps if need <= 2000 else max(3, reps // 5)
    # (a) what a caller gets: the default rounds per call, resumed until finished; (b) the rounds known in advance
    for label, rounds in ((f"the default {default} rounds a call", default),
                          (f"{min(need + 2, abi.NAV_MAX_ROUNDS)} rounds a call, the number known from the run before",
                           min(need + 2, abi.NAV_MAX_ROUNDS))):
        outs = [event_ms(lambda: field(rounds)) for _ in range(n_rep)]
        times = [o[0] for o in outs]
        calls, _, visits, left = outs[-1][1]
        t = statistics.median(times)
        same = left == 0 and bool(np.array_equal(d_pot.cpu().numpy().view(np.uint32).reshape(n, n), want))
        lines.append(f"  {form}, {label}: finished in {t:.3f} ms (min {min(times):.3f}, {n_rep} timings, {calls} call(s)), "
                     f"{need} rounds had a dirty tile, {visits} tile visits ({visits / ((n // 64) ** 2):.2f} per tile); "
                     f"{t / floor_ms:.1f} x the fill + copy, {host_ms / t:.1f} x faster than the host twin on one core; "
                     f"equals the host twin: {same}")
    gpu.close()
    print("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    text = ["E26 rplgpu_nav_field_dev: time to a finished field from scratch, median of device-event timings, one fresh "
            "process per map; the CPU figure is the library's host twin rplgpu_nav_field_host on one core of the same "
            "machine, not the reference project"]
    sizes = (int(sys.argv[3]),) if len(sys.argv) > 3 else SIZES
    failed = False
    for n, name in ((n, name) for n in sizes for name in MAPS):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[n]), sys.executable, str(Path(__file__).resolve()), "--one", name,
               str(n), str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        failed = r.returncode != 0
        if failed:  # a fault, an abort or the time limit: nothing more is started on the device
            text.append(f"{name} {n}: child ended with status {r.returncode}; the run stops here\n{r.stderr[-2000:]}")
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
