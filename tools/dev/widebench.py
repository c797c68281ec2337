"""E24 (rplgpu_match_wide_dev) on matchbench.py's workload: G time steps of 8 sensors x 32 000 samples, the default
grid (1024 x 1024 cells of 0.05 m), the sensors on a 0.6 m circle, E5 on, the field E11 + E12 (default inflation) of
time step 0 made on the device, once on clean rings and once with 1 cm noise.  Two measurements, medians of
device-event timings:
  (a) E24 beside E13 (rplgpu_match_scans_dev) in one process at E13's largest window, T = 32, K = 10: the ratio
      E24 / E13, the list length n of group 0, and rplgpu_pool_field_dev timed apart (a static map is pooled once);
  (b) E24 alone at T = 256, K = 10, which E13 cannot do.
max_blocks is the default 1024.  Group 0's bounds volume, result words and work words are checked against
tests/wide_oracle.py (writer 2), and in (a) words 0 - 6 against E13's own on the device.

    python tools/dev/widebench.py [G reps [out.txt]]      (prints the report; also writes it to out.txt if given)"""
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402
from tests import match_oracle as mo  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests import wide_oracle as wo  # noqa: E402
from tests.fused_oracle import group_points  # noqa: E402

S, N = 8, 32000


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


def main():
    G = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    B = G * S
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(stream)
    gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=B)
    gpu.set_stream(stream.cuda_stream)
    oracle = oracle_lib.load_oracle()
    grid = abi.OccGrid.defaults()
    cells = grid.width * grid.height
    pcells = (grid.width + 7) * (grid.height + 7)
    pstride = (pcells + 3) & ~3
    p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, ror_enable=1, ror_radius=0.10,
                        ror_min_neighbors=2)
    ang = 2 * math.pi * (np.arange(B) % S) / S
    pose2d = np.stack([np.cos(ang), -np.sin(ang), 0.6 * np.cos(ang), np.sin(ang), np.cos(ang), 0.6 * np.sin(ang)],
                      1).astype(np.float32)
    d_po = torch.from_numpy(pose2d).to(dev)
    d_len = torch.full((B,), N, dtype=torch.int32, device=dev)
    d_grid = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_field = torch.zeros(cells, dtype=torch.int8, device=dev)
    d_pooled = torch.zeros(pstride, dtype=torch.int8, device=dev)
    d_best = torch.zeros(G * 8, dtype=torch.int32, device=dev)
    d_best13 = torch.zeros(G * 8, dtype=torch.int32, device=dev)
    d_work = torch.zeros(G * 8, dtype=torch.int32, device=dev)
    d_st = torch.zeros(G, dtype=torch.int32, device=dev)
    inflation = abi.Inflation.defaults()
    table, rc = abi.inflation_table(inflation, grid.resolution)
    d_table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    lines = [f"E24 rplgpu_match_wide_dev: {G} groups x {S} scans x {N} samples, field {grid.width} x {grid.height} x "
             f"{grid.resolution:.2f} m (E11 + E12 of time step 0), K 10 x 0.25 deg, max_blocks 1024, E5 on, median "
             f"(min) of {reps} device-event timings"]
    for label, noise in (("clean rings", 0.0), ("1 cm noise", 0.01)):
        batch = synth.make_batch(2026 + 5, B, N, noise_m=noise)
        d_nodes = torch.from_numpy(batch.view(np.uint8).reshape(B, N * 8)).to(dev)
        gpu.occupancy_grid_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), S, S, p, 0, d_po.data_ptr(), grid, 0,
                               d_grid.data_ptr(), cells)
        gpu.inflate_grids_dev(d_grid.data_ptr(), cells, d_field.data_ptr(), cells, 1, grid.width, grid.height,
                              d_table.data_ptr(), rc, inflation.inflate_unknown)
        gpu.synchronize()
        field = d_field.cpu().numpy().reshape(grid.height, grid.width)
        x, y, *_ = group_points(oracle, list(batch[:S]), p, None, pose2d[:S], None)
        for T in (32, 256):
            wide = abi.WideMatch.defaults(shift_x=T, shift_y=T)
            spec = wo.spec(shift_x=T, shift_y=T)
            blocks = abi.wide_match_blocks(wide)
            d_bounds = torch.zeros(G * blocks, dtype=torch.int32, device=dev)
            d_scratch = torch.zeros(abi.wide_match_scratch_words(wide, G), dtype=torch.int32, device=dev)

            def pool():
                gpu.pool_field_dev(wide, d_field.data_ptr(), cells, 1, d_pooled.data_ptr(), pstride)

            def stage():
                gpu.match_wide_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), B, S, p, 0, d_po.data_ptr(), 0, wide,
                                   d_field.data_ptr(), cells, 0, d_pooled.data_ptr(), pstride, d_bounds.data_ptr(),
                                   blocks, d_scratch.data_ptr(), d_best.data_ptr(), d_work.data_ptr(), d_st.data_ptr())

            p_med, p_min = timed(pool, reps)
            t_med, t_min = timed(stage, reps)
            gpu.synchronize()
            best = d_best.cpu().numpy().view(np.uint32).reshape(G, 8)
            work = d_work.cpu().numpy().view(np.uint32).reshape(G, 8)
            w = wo.match_bound_refine(x, y, None, spec, field)
            same = best[0].tobytes() == mo.best_words(w["best"]).tobytes() and \
                work[0].tobytes() == mo.best_words(w["work"]).tobytes() and \
                d_bounds[:blocks].cpu().numpy().view(np.uint32).tobytes() == w["U"].tobytes() and \
                d_pooled[:pcells].cpu().numpy().tobytes() == w["P"].tobytes()
            text = (f"{label}, T {T}: E24 {t_med:.3f} ms ({t_min:.3f}), {t_med / G * 1e3:.1f} us per time step; pool "
                    f"apart {p_med:.3f} ms ({p_min:.3f}); group 0: n = {int(work[0][4])} of {int(work[0][0])} blocks "
                    f"listed, b0 {int(work[0][3])}, greatest bound {int(work[0][1])}, best "
                    f"{best[0].view(np.int32).tolist()}; unproven groups {int((best[:, 7] != 0).sum())} of {G}; "
                    f"group 0 equals the oracle: {same}")
            if T == 32:
                match = wide.scan_match(T, T)
                volume = abi.scan_match_volume(match)
                d_scores = torch.zeros(G * volume, dtype=torch.int32, device=dev)

                def e13():
                    gpu.match_scans_dev(d_nodes.data_ptr(), N, d_len.data_ptr(), B, S, p, 0, d_po.data_ptr(), 0, match,
                                        d_field.data_ptr(), cells, 0, d_scores.data_ptr(), volume,
                                        d_best13.data_ptr(), d_st.data_ptr())

                e_med, e_min = timed(e13, reps)
                gpu.synchronize()
                best13 = d_best13.cpu().numpy().view(np.uint32).reshape(G, 8)
                proven = best[:, 7] == 0
                agree = bool((best[proven, :7] == best13[proven, :7]).all())
                faster = "E24 is the faster one" if t_med < e_med else "E24 is NOT the faster one here"
                text += (f"; E13 at the same window ({volume} candidates) {e_med:.3f} ms ({e_min:.3f}): E24 / E13 = "
                         f"{t_med / e_med:.3f}, with the pool {(t_med + p_med) / e_med:.3f} ({faster}); words 0 - 6 of "
                         f"every proven group equal E13's: {agree}")
                del d_scores
            lines.append(text)
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
