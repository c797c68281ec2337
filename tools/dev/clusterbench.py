"""E21 (rplgpu_cluster_poses_dev): one group, the default map (103 x 103 bins of 0.5 m, 72 heading bins, WRAP), P = 2^20,
for three lists — CONVERGED (an E19 list resampled by weights that are not 0 only in a box of 0.6 m and one heading),
TWO MODES (two such boxes, weights 3 and 2) and SPREAD (an E19 list over a grid whose cells are all free).
Per list: E20 makes the map and the bin ids on the device, then median, minimum and maximum of device-event timings of
the whole E21 call (its nine launches together; their split comes from a kernel trace of ONE list of this script taken
in a run of its own: tools/dev/clusterprof.sh, `rocprofv3 --kernel-trace --stats -- python tools/dev/clusterbench.py
--list NAME reps`), beside E20's call on the same list and rplgpu_cluster_poses_host on one CPU thread.
The result words, labels and table rows of every run are checked against rplgpu_cluster_poses_host.

Every list runs in a child process of its own under its own `timeout`, so a list that hangs ends there and the lists
after it are not started.

    python tools/dev/clusterbench.py [reps [out.txt [label]]]   (prints the report; also appends it to out.txt if given;
    RPLGPU_LIBRARY picks the library, `label` names it in the report)"""
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

T = 72
P = 1 << 20
LISTS = ("converged", "two_modes", "spread")
LIMIT_S = 240                                                       # per list: the host twin on a spread list is the long part


def make_list(name, abi, table):
    seed = abi.PoseSeed.defaults()
    grid = np.zeros(seed.width * seed.height, np.int8)
    spread = abi.seed_poses_host(grid, table, P, seed, abi.MotionNoise.defaults(seed=2026, step=23))[0]
    if name == "spread":
        return spread

    def box(x, y, k):
        return (np.abs(spread[:, 2] - x) < 0.3) & (np.abs(spread[:, 3] - y) < 0.3) & \
            (spread[:, 0] == table[k, 0]) & (spread[:, 1] == table[k, 1])

    w = 3 * box(3.3, -7.1, 5).astype(np.uint32)
    if name == "two_modes":
        w += 2 * box(-11.2, 9.4, 40).astype(np.uint32)
    return abi.resample_host(w, spread, P, 0x9E3779B9)[0]


def run_list(name, reps):
    import torch

    from rplidar_ros2_driver_amd import RplGpu, abi

    def timed(fn):
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

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=8)
    gpu.set_stream(stream.cuda_stream)
    table = abi.seed_headings(T)
    poses = make_list(name, abi, table)
    bspec, cspec = abi.PoseBins.defaults(), abi.PoseClusters.defaults()
    words = abi.bin_map_words(bspec.nx, bspec.ny, T)
    cap = 4096
    d_p = torch.from_numpy(poses.reshape(-1)).to(dev)
    d_e = torch.from_numpy(table.reshape(-1)).to(dev)
    d_m = torch.zeros(words, dtype=torch.int32, device=dev)
    d_b = torch.zeros(P, dtype=torch.int32, device=dev)
    d_r20 = torch.zeros(8, dtype=torch.int32, device=dev)
    d_l = torch.zeros(P, dtype=torch.int32, device=dev)
    d_t = torch.zeros(4 * cap, dtype=torch.int32, device=dev)
    d_r = torch.zeros(80, dtype=torch.int32, device=dev)
    scratch = abi.cluster_scratch_words(1, P, cspec.nx, cspec.ny, T)
    d_s = torch.zeros(scratch, dtype=torch.int32, device=dev)

    def bins():
        gpu.bin_poses_dev(bspec, d_p.data_ptr(), 4 * P, 0, 0, 0, 1, P, d_e.data_ptr(), T, d_m.data_ptr(), words,
                          d_b.data_ptr(), P, d_r20.data_ptr())

    def clusters():
        gpu.cluster_poses_dev(cspec, d_p.data_ptr(), 4 * P, 0, 0, 0, 1, P, T, d_m.data_ptr(), words, d_b.data_ptr(), P,
                              d_l.data_ptr(), P, d_t.data_ptr(), 4 * cap, cap, d_r.data_ptr(), d_s.data_ptr())

    b_med, b_min, b_max = timed(bins)
    c_med, c_min, c_max = timed(clusters)
    gpu.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    nb_words = (bspec.nx * bspec.ny * T + 31) // 32
    bmap, bin_ids = u32(d_m)[:nb_words].copy(), u32(d_b).copy()
    t0 = time.perf_counter()
    want = abi.cluster_poses_host(poses, bmap, bin_ids, T, None, cspec, cap)
    host_ms = (time.perf_counter() - t0) * 1e3
    res = u32(d_r)
    n = min(cap, int(res[6]))
    same = res.tobytes() == want[2].tobytes() and u32(d_l).tobytes() == want[0].tobytes() and \
        u32(d_t)[:4 * n].tobytes() == want[1].reshape(-1)[:4 * n].tobytes()
    print(f"{name}, NB = {bspec.nx * bspec.ny * T}, P = {P}: E21 {c_med:.4f} ms ({c_min:.4f} .. {c_max:.4f}); K = "
          f"{int(res[7])}, N_c = {int(res[6])}, BEST label {int(res[1])} with {int(res[4])} poses, flags {int(res[0])}; E20 "
          f"on the same list {b_med:.4f} ms ({b_min:.4f} .. {b_max:.4f}); rplgpu_cluster_poses_host {host_ms:.1f} ms "
          f"(one run); scratch {4 * scratch / 1e6:.1f} MB; equal to rplgpu_cluster_poses_host: {same}")
    gpu.close()
    return 0 if same else 3


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        return run_list(sys.argv[2], int(sys.argv[3]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    label = sys.argv[3] if len(sys.argv) > 3 else "the library as built"
    lines = [f"E21 rplgpu_cluster_poses_dev [{label}]: 1 group, median (min .. max) of {reps} timings: device events "
             f"around the whole call (nine launches; apart: tools/dev/clusterprof.sh); E20's call on the same list; the host twin on one "
             f"CPU thread"]
    for name in LISTS:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--list", name, str(reps)],
                           capture_output=True, text=True)
        lines.append(r.stdout.strip() or f"{name}: no output")
        if r.returncode != 0:                                       # a fault, a hang or a wrong answer: nothing more is started
            lines.append(f"{name}: exit status {r.returncode}; stopped here\n{r.stderr.strip()[-2000:]}")
            break
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
