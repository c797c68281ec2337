"""E28 (rplgpu_mppi_update_dev, rplgpu_mppi_spread_dev) at MPPI's shapes, behind E27 on rolloutbench.py's 1024 x 1024
costmap with an E26 field:

    mppi     G = 1, K = 2048 control sequences of T = 56 steps (E27's own MPPI shape), F = 16
    small    G = 1, K = 1024, T = 32
    batch    G = 64 of the small shape (one start and one noise draw per group, the map shared)

Per shape, by device events around bursts of calls, per call, the median of the timings after a warm-up: the update
(three launches), the spread (one launch), E27's call at the same shape, and the whole iteration E18 + spread + E27 +
update queued on one stream; next to them an empty-launch floor of three launches and of one (fills of eight words,
timed the same way) and ONE core of this machine running the library's own host twins rplgpu_mppi_update_host and
rplgpu_mppi_spread_host (one group; NOT the reference project, which plans nothing).  Group 0's outputs are compared
with the host twins' byte for byte.

Every library runs in a fresh process of its own under its own time limit, started one after the other by the parent,
which never opens the device; a child that fails ends the run.  With a second library (the other form of the
cross-workgroup fold, built from tools/dev/patches/mppi_atomic_r35.diff) the two alternate, ROUNDS times each.

    python tools/dev/mppibench.py [out.txt [reps [other_library.so]]]    (the report is appended to out.txt)
    python tools/dev/mppibench.py --one LABEL REPS HOST      (one child: prints its lines; HOST 1 times the twins)"""
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

N = 1024
ROUNDS = 3
BURST = 50
LIMIT_S = 240
F = 16
SHAPES = (("mppi", 1, 2048, 56), ("small", 1, 1024, 32), ("batch", 64, 1024, 32))


def one(label, reps, with_host):
    import torch

    from rolloutbench import room_costmap
    from rplidar_ros2_driver_amd import RplGpu, abi
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=16)
    gpu.set_stream(stream.cuda_stream)
    cost = room_costmap()
    nav = abi.NavField.defaults(width=N, height=N)
    field, _ = abi.nav_field_host(nav, cost, [800 * N + 800])
    d_cost = torch.from_numpy(cost.reshape(-1)).to(dev)
    d_pot = torch.from_numpy(field.reshape(-1).view(np.int32)).to(dev)
    d_floor = torch.zeros(8, dtype=torch.int32, device=dev)
    lib = Path(abi.library_path()).resolve()
    lines = [f"{label}: {lib.relative_to(ROOT) if ROOT in lib.parents else lib.name}"]

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BURST):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / BURST

    def floor1():
        d_floor.fill_(0)

    def floor3():
        d_floor.fill_(0)
        d_floor.fill_(1)
        d_floor.fill_(2)

    def med(fn):
        return statistics.median([event_ms(fn) for _ in range(reps)]) * 1e3

    zeros = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    for name, G, K, T in SHAPES:
        n = 4 * K * T
        rs = abi.Rollout.defaults(steps=T, min_steps=T // 2, a_end=1, a_min=0, a_sum=2, a_max=1)
        ms = abi.Mppi.defaults(steps=T, delta_per_step=1, table_len=4096, shift=2)
        table = abi.mppi_table(2000.0, 2, 4096)
        ang = 2 * math.pi * np.arange(F) / F
        fp = np.stack([0.3 * np.cos(ang), 0.2 * np.sin(ang)], 1).astype(np.float32)
        starts = np.stack([abi.pose_list([[-25.6 + 0.05 * (340 + 0.5 * g), -25.6 + 0.05 * (500 + g), 0.1 * g]])[0]
                           for g in range(G)])
        step = abi.rollout_deltas(np.array([[0.6, 0.0, 0.2]]), 3.2 / T)[0]
        nominal = np.tile(step, (T, 1))
        odom = np.array([1, 0, 0, 1, 0, 2e-6, 1e-6, 2e-6], np.float32)   # the identity with E18's three scales
        noise_spec = abi.MotionNoise.defaults()
        d_start, d_fp = torch.from_numpy(starts.reshape(-1)).to(dev), torch.from_numpy(fp.reshape(-1)).to(dev)
        d_odom, d_table = torch.from_numpy(odom).to(dev), torch.from_numpy(table.view(np.int16)).to(dev)
        d_nom = torch.from_numpy(np.tile(nominal.reshape(-1), G)).to(dev)
        d_noise, d_cand, d_mres = zeros(G * n, torch.float32), zeros(G * n, torch.float32), zeros(8 * G)
        d_out, d_end, d_rres = zeros(G * 8 * K), zeros(G * 4 * K, torch.float32), zeros(8 * G)
        d_rscr = zeros(abi.rollout_scratch_words(G, K))
        d_w, d_sums, d_nout, d_res = zeros(G * K), zeros(G * 8 * T), zeros(G * 4 * T, torch.float32), zeros(8 * G)
        d_scr = zeros(abi.mppi_scratch_words(G, K, T))

        def sample():
            gpu.sample_motion_dev(d_odom.data_ptr(), 0, G, K * T, noise_spec, d_noise.data_ptr(), n, d_mres.data_ptr())

        def spread():
            gpu.mppi_spread_dev(d_nom.data_ptr(), 4 * T, 1, T, d_noise.data_ptr(), n, 1, G, K, T, 1, 1,
                                d_cand.data_ptr(), n)

        def roll():
            gpu.rollout_dev(rs, d_start.data_ptr(), 1, d_cand.data_ptr(), n, 1, 1, d_fp.data_ptr(), F,
                            d_cost.data_ptr(), N * N, d_pot.data_ptr(), N * N, 0, G, K, d_out.data_ptr(), 8 * K,
                            d_end.data_ptr(), 4 * K, d_rres.data_ptr(), d_rscr.data_ptr())

        def update():
            gpu.mppi_update_dev(ms, d_out.data_ptr(), 8 * K, d_rres.data_ptr(), d_cand.data_ptr(), n, 1,
                                d_table.data_ptr(), d_nom.data_ptr(), 4 * T, 1, G, K, d_w.data_ptr(), K,
                                d_sums.data_ptr(), 8 * T, d_nout.data_ptr(), 4 * T, d_res.data_ptr(), d_scr.data_ptr())

        def iteration():
            sample()
            spread()
            roll()
            update()

        iteration()
        gpu.synchronize()
        for fn in (update, spread, roll, iteration, floor1, floor3) * 3:
            event_ms(fn)
        t_upd, t_spr, t_roll, t_it = med(update), med(spread), med(roll), med(iteration)
        f1, f3 = med(floor1), med(floor3)
        res = d_res.cpu().numpy().view(np.uint32).reshape(G, 8)
        rres = d_rres.cpu().numpy().view(np.uint32).reshape(G, 8)
        cand = d_cand.cpu().numpy()[:n].reshape(K, T, 4)
        noise = d_noise.cpu().numpy()[:n].reshape(K, T, 4)
        out0 = d_out.cpu().numpy().view(np.uint32)[:8 * K].reshape(K, 8)
        t0 = time.perf_counter()
        want = abi.mppi_update_host(ms, out0, rres[0], cand, table, nominal)
        host_upd = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        want_cand = abi.mppi_spread_host(nominal, noise, 1, 1)
        host_spr = (time.perf_counter() - t0) * 1e3
        got = (d_w.cpu().numpy().view(np.uint32)[:K], d_sums.cpu().numpy().view(np.uint32)[:8 * T],
               d_nout.cpu().numpy()[:4 * T], res[0])
        same = all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and cand.tobytes() == want_cand.tobytes()
        sw, sw2 = int(res[0, 2]) | int(res[0, 3]) << 32, int(res[0, 4]) | int(res[0, 5]) << 32
        line = (f"  {name} (G {G}, K {K}, T {T}): update {t_upd:.1f} us a call (floor of three launches {f3:.1f}), spread "
                f"{t_spr:.1f} us (floor of one launch {f1:.1f}), E27 {t_roll:.1f} us, the iteration E18 + spread + E27 + "
                f"update {t_it:.1f} us: the update is {100 * t_upd / t_it:.0f} % of it ({reps} timings of {BURST} "
                f"calls each); group 0: {int(res[0, 0])} weighted of {int(rres[0, 0])} admissible, "
                f"{int(res[0, 1])} clamped, N_eff {sw * sw / max(sw2, 1):.1f}, flags {int(res[0, 7])}; equals the host "
                f"twins: {same}")
        if with_host:
            line += (f"; rplgpu_mppi_update_host on one core {host_upd:.2f} ms a group ({G * host_upd / t_upd * 1e3:.0f} x "
                     f"the device's time for the {G} group(s)), rplgpu_mppi_spread_host {host_spr:.2f} ms "
                     f"({G * host_spr / t_spr * 1e3:.0f} x)")
        lines.append(line)
    gpu.close()
    print("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]), sys.argv[4] == "1")
        return
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    other = sys.argv[3] if len(sys.argv) > 3 else None
    text = ["E28 rplgpu_mppi_update_dev / rplgpu_mppi_spread_dev: whole calls per shape, medians of device-event timings "
            "over bursts of calls, one fresh process per library and round; the CPU figures are the library's host twins "
            "on one core of the same machine, not the reference project"]
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
