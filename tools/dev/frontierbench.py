"""E29 (rplgpu_frontiers_dev) on maps of a room being explored:

    1024         G = 1, 1024 x 1024: a walled room seen from its middle out to a ragged sensor horizon, the rest unknown
    1024 noise   the same with one cell in a hundred of the outer part of the seen area left unknown (what range
                 noise leaves before a horizon): thousands of small components
    4096, 4096 noise   the same at 4096 x 4096
    batch        G = 64 grids of 256 x 256, each another room

The maps are made on the host by this file (NOT by E14 from occbench.py's scans); the field D of every map is E26's,
computed on the device from the robot's cell before anything is timed.  Per shape, by device events around bursts of
calls, per call, the median of the timings after a warm-up: the whole call (seven launches); next to it a plain device
copy of the same grids plus fields (the bandwidth floor), seven empty launches (fills of eight words, the launch
floor) and ONE core of this machine running the library's own host twin rplgpu_frontiers_host (one grid; NOT the
reference project, which explores nothing).  Group 0's result words, labels, rows and goal are compared with the host
twin's byte for byte.  The share of tiles with no frontier cell (they leave the tile pass early), F, N and the kept
components are reported per shape.

Every library runs in a fresh process of its own under its own time limit, started one after the other by the parent,
which never opens the device; a child that fails ends the run.  With a second library (the other form, built from
tools/dev/patches/) the two alternate, ROUNDS times each.

    python tools/dev/frontierbench.py [out.txt [reps [other_library.so]]]    (the report is appended to out.txt)
    python tools/dev/frontierbench.py --one LABEL REPS HOST      (one child: prints its lines; HOST 1 times the twin)"""
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

ROUNDS = 3
BURST = 20
LIMIT_S = 400
COMP_CAP = 1 << 18
ROW_CAP = 64
SHAPES = (("1024", 1, 1024, False), ("1024 noise", 1, 1024, True), ("4096", 1, 4096, False),
          ("4096 noise", 1, 4096, True), ("batch", 64, 256, False))


def room_map(n, noise, seed=0):
    """(n, n) int8: -1 unknown, 0 free, 100 wall; the robot stands in the middle."""
    rng = np.random.default_rng(seed + n)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    cx = cy = n / 2
    dx, dy = x - cx, y - cy
    r = np.hypot(dx, dy)
    th = np.arctan2(dy, dx)
    k = rng.integers(3, 9, 4)
    ph = rng.random(4) * 6.28
    horizon = n * (0.30 + 0.05 * np.sin(k[0] * th + ph[0]) + 0.04 * np.sin(k[1] * th + ph[1]) +
                   0.02 * np.sin(5 * k[2] * th + ph[2]) + 0.01 * np.sin(17 * k[3] * th + ph[3]))
    half = 0.36 * n
    with np.errstate(divide="ignore"):
        wall = np.minimum(half / np.maximum(np.abs(np.cos(th)), 1e-6), half / np.maximum(np.abs(np.sin(th)), 1e-6))
    g = np.full((n, n), -1, np.int8)
    g[r < np.minimum(horizon, wall)] = 0
    g[(r >= wall) & (r < wall + 2) & (wall <= horizon)] = 100
    if noise:
        hole = (rng.random((n, n)) < 0.01) & (g == 0) & (r > 0.6 * horizon)
        g[hole] = -1
    return g


def one(label, reps, with_host):
    import torch

    from rplidar_ros2_driver_amd import RplGpu, abi
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=16)
    gpu.set_stream(stream.cuda_stream)
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

    def floor7():
        for i in range(7):
            d_floor.fill_(i)

    def med(fn):
        t = [event_ms(fn) * 1e3 for _ in range(reps)]
        return statistics.median(t), min(t), max(t)

    zeros = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    for name, G, n, noise in SHAPES:
        cells = n * n
        grids = np.stack([room_map(n, noise, seed=g) for g in range(G)])
        spec = abi.Frontiers.defaults(width=n, height=n)
        nav = abi.NavField.defaults(width=n, height=n)
        robot = (n // 2) * n + n // 2
        d_grid = torch.from_numpy(grids.reshape(-1)).to(dev)
        d_goals, d_one = torch.full((G,), robot, dtype=torch.int32, device=dev), torch.ones(G, dtype=torch.int32, device=dev)
        d_pot, d_nres = zeros(G * cells), zeros(8 * G)
        d_nscr = zeros(abi.nav_field_scratch_words(nav, G))
        for call in range(64):  # the field from the robot's cell, resumed until it is finished
            gpu.nav_field_dev(nav, d_grid.data_ptr(), cells, G, d_goals.data_ptr(), 1, d_one.data_ptr(), d_pot.data_ptr(),
                              cells, d_nscr.data_ptr(), 1 if call else 0, d_nres.data_ptr())
            gpu.synchronize()
            if not d_nres.cpu().numpy().reshape(G, 8)[:, 0].any():
                break
        else:
            raise RuntimeError("the field did not finish")
        d_lab, d_rows, d_goal, d_n, d_res = zeros(G * cells), zeros(G * 8 * ROW_CAP), zeros(G), zeros(G), zeros(16 * G)
        d_scr = zeros(abi.frontiers_scratch_words(spec, G, COMP_CAP))
        d_copy_g, d_copy_p = torch.empty_like(d_grid), torch.empty_like(d_pot)

        def call():
            gpu.frontiers_dev(spec, d_grid.data_ptr(), cells, d_pot.data_ptr(), cells, G, COMP_CAP, d_lab.data_ptr(),
                              cells, d_rows.data_ptr(), 8 * ROW_CAP, ROW_CAP, d_goal.data_ptr(), 1, d_n.data_ptr(),
                              d_res.data_ptr(), d_scr.data_ptr())

        def copy():
            d_copy_g.copy_(d_grid)
            d_copy_p.copy_(d_pot)

        call()
        gpu.synchronize()
        for fn in (call, copy, floor7) * 3:
            event_ms(fn)
        t_call, t_copy, t_floor = med(call), med(copy), med(floor7)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        res = u32(d_res).reshape(G, 16)
        lab0 = u32(d_lab)[:cells].reshape(n, n)
        pot0 = u32(d_pot)[:cells].reshape(n, n)
        t0 = time.perf_counter()
        want = abi.frontiers_host(spec, grids[0], pot0, comp_cap=COMP_CAP, row_cap=ROW_CAP)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = (want["result"].tolist() == res[0].tolist() and want["labels"].tobytes() == lab0.tobytes() and
                want["rows"].tobytes() == u32(d_rows)[:8 * ROW_CAP].tobytes() and
                int(want["n_goal"][0]) == int(u32(d_n)[0]) and
                (int(want["n_goal"][0]) == 0 or int(want["goal"][0]) == int(u32(d_goal)[0])))
        t = n // 64
        busy = (lab0 != 0xFFFFFFFF).reshape(t, 64, t, 64).any(axis=(1, 3))
        line = (f"  {name} (G {G}, {n} x {n}): the call {t_call[0]:.1f} us ({t_call[1]:.1f} to {t_call[2]:.1f}), a device "
                f"copy of the grids and fields {t_copy[0]:.1f} us ({t_copy[1]:.1f} to {t_copy[2]:.1f}), seven empty "
                f"launches {t_floor[0]:.1f} us ({t_floor[1]:.1f} to {t_floor[2]:.1f}) ({reps} timings of {BURST} calls "
                f"each); group 0: F {int(res[0, 1])}, N {int(res[0, 2])}, kept {int(res[0, 3])}, flags {int(res[0, 0])}, "
                f"{100 * (1 - busy.mean()):.1f} % of its {t * t} tiles leave early; equals the host twin: {same}")
        if with_host:
            line += (f"; rplgpu_frontiers_host on one core {host_ms:.1f} ms a grid "
                     f"({G * host_ms / t_call[0] * 1e3:.0f} x the device's time for the {G} grid(s))")
        lines.append(line)
        del d_grid, d_pot, d_lab, d_scr, d_copy_g, d_copy_p
    gpu.close()
    print("\n".join(lines))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]), sys.argv[4] == "1")
        return
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    other = sys.argv[3] if len(sys.argv) > 3 else None
    text = ["E29 rplgpu_frontiers_dev: whole calls per shape, medians (least to greatest) of device-event timings over "
            "bursts of calls, one fresh process per library and round; the CPU figures are the library's host twin on "
            "one core of the same machine, not the reference project"]
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
