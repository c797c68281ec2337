"""Developer aid: the cell exchange (include/rplgpu_comm.h) on the bench's config-5 fused workload (4096 scans =
512 time steps x 8 sensors x 32 000 samples, 1 cm noise, ROR 0.10 m / 2, voxel 5 cm, the bench's motion and pose
generator), device events after a warm-up, alternating:
  (a) rplgpu_cloud_fused_voxel_dev, group 8 (the single-GPU E8 grid)
  (b) rplgpu_cloud_fused_cells_dev, group 1, over all 4096 scans (one record list per scan)
  (c) rplgpu_merge_cells_dev over 8 virtual ranks: rank r = sensor r's 512 scans through the same producer
      (group 1) into its own slot, META by rplgpu_pack_cloud_meta_dev, as behind rplgpu_gather_cells_dev
  (d) b + c
and the cells / bytes each stage moves; (c)'s output is checked against (a) byte for byte.
  python tools/dev/cellbench.py [reps=10]"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B, n, S = 4096, 32000, 8
T = B // S
dev = torch.device("cuda:0")
batch = synth.make_batch(2026 + 5, B, n, noise_m=0.01)
p = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, voxel_enable=1, voxel_leaf=0.05,
                    ror_enable=1, ror_radius=0.10, ror_min_neighbors=2)
rng = np.random.default_rng(2026)
motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                   for _ in range(B)]).astype(np.float32)
ang = rng.uniform(-3, 3, B)
pose2d = np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, B), np.sin(ang), np.cos(ang),
                   rng.uniform(-2, 2, B)], 1).astype(np.float32)
# (b) runs over the scans SENSOR-major (scan t * 8 + s -> s * 512 + t): sensor s's 512 scans are the
# contiguous records of virtual rank s, its groups (group 1 = one scan) the time steps
perm = np.array([t * S + s for s in range(S) for t in range(T)])


def dev_of(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


d_nodes = dev_of(batch.view(np.uint8).reshape(B, n * 8))
d_nodes_sm = dev_of(batch[perm].view(np.uint8).reshape(B, n * 8))
d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
d_mo, d_po = dev_of(motion), dev_of(pose2d)
d_mo_sm, d_po_sm = dev_of(motion[perm]), dev_of(pose2d[perm])
cap = B * n
d_arena = torch.empty(cap, 4, dtype=torch.float32, device=dev)
d_cur = torch.zeros(1, dtype=torch.int64, device=dev)
d_gs = torch.zeros(T, dtype=torch.int64, device=dev)
d_np = torch.zeros(T, dtype=torch.int32, device=dev)
d_st = torch.zeros(T, dtype=torch.int32, device=dev)
d_cells = torch.empty(cap * 8 // 4, dtype=torch.int32, device=dev)  # (b)'s records: room for B * n / 4 cells
cells_cap = cap // 4
d_ccur = torch.zeros(1, dtype=torch.int64, device=dev)
d_cstart = torch.zeros(B, dtype=torch.int64, device=dev)
d_cn = torch.zeros(B, dtype=torch.int32, device=dev)
d_cst = torch.zeros(B, dtype=torch.int32, device=dev)
mw = abi.cloud_meta_words(T)
d_meta = torch.zeros(S, mw, dtype=torch.int32, device=dev)  # one META block per virtual rank
d_out = torch.empty(cap, 4, dtype=torch.float32, device=dev)
d_ocur = torch.zeros(1, dtype=torch.int64, device=dev)
d_ogs = torch.zeros(T, dtype=torch.int64, device=dev)
d_onp = torch.zeros(T, dtype=torch.int32, device=dev)
d_ost = torch.zeros(T, dtype=torch.int32, device=dev)

gpu = RplGpu(device=0, max_samples_per_scan=32768, max_batch=B)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
gpu.set_stream(stream.cuda_stream)


def fused():
    gpu.cloud_fused_voxel_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, S, p, d_mo.data_ptr(), d_po.data_ptr(),
                              d_arena.data_ptr(), cap, d_cur.data_ptr(), d_gs.data_ptr(), d_np.data_ptr(),
                              d_st.data_ptr())


def cells():
    gpu.cloud_fused_cells_dev(d_nodes_sm.data_ptr(), n, d_len.data_ptr(), B, 1, p, d_mo_sm.data_ptr(),
                              d_po_sm.data_ptr(), d_cells.data_ptr(), cells_cap, d_ccur.data_ptr(),
                              d_cstart.data_ptr(), d_cn.data_ptr(), d_cst.data_ptr())


def ranks():
    """(c)'s input: virtual rank s = sensor s's 512 scans through the producer into ITS slot of the gathered
    buffer (group 1: a time step of one sensor is one group) + its META block, as behind rplgpu_gather_cells_dev."""
    for s in range(S):
        sl = slice(s * T, (s + 1) * T)
        gpu.cloud_fused_cells_dev(d_nodes_sm[sl].data_ptr(), n, d_len.data_ptr(), T, 1, p, d_mo_sm[sl].data_ptr(),
                                  d_po_sm[sl].data_ptr(), d_slots[s].data_ptr(), slot, d_rcur[s].data_ptr(),
                                  d_rstart[s].data_ptr(), d_rn[s].data_ptr(), d_rst[s].data_ptr())
        gpu.pack_cloud_meta_dev(d_rcur[s].data_ptr(), d_rstart[s].data_ptr(), d_rn[s].data_ptr(), T, slot, T,
                                d_meta[s].data_ptr())


def merge():
    gpu.merge_cells_dev(d_slots.data_ptr(), slot, d_meta.data_ptr(), mw, S, T, p, d_out.data_ptr(), cap,
                        d_ocur.data_ptr(), d_ogs.data_ptr(), d_onp.data_ptr(), d_ost.data_ptr())


def b_and_c():
    cells()
    merge()


def timed(fn, k):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


fused()
cells()
torch.cuda.synchronize()
ncells_b = int(d_ccur.item())
assert ncells_b <= cells_cap, "cell arena too small"
slot = int(d_cn.view(S, T).sum(1).max().item()) + 1024  # the largest rank's records
d_slots = torch.empty(S, slot * 8, dtype=torch.int32, device=dev)
d_rcur = torch.zeros(S, 1, dtype=torch.int64, device=dev)
d_rstart = torch.zeros(S, T, dtype=torch.int64, device=dev)
d_rn = torch.zeros(S, T, dtype=torch.int32, device=dev)
d_rst = torch.zeros(S, T, dtype=torch.int32, device=dev)
ranks()
merge()  # (warm-up: grows the merge scratch once)
torch.cuda.synchronize()
assert int(d_rcur.max().item()) <= slot
# (c) against (a), byte for byte per time step
a_tot, c_tot = int(d_cur.item()), int(d_ocur.item())
A, Cc = d_arena[:a_tot].cpu().numpy(), d_out[:c_tot].cpu().numpy()
ga, na, gc, nc = (x.cpu().numpy().astype(np.int64) for x in (d_gs, d_np, d_ogs, d_onp))
same = a_tot == c_tot and all(A[ga[t]:ga[t] + na[t]].tobytes() == Cc[gc[t]:gc[t] + nc[t]].tobytes() for t in range(T))
res = {"identical_to_fused_voxel": bool(same), "cells_out": c_tot, "records_b": ncells_b,
       "records_c_in": int(d_rcur.sum().item()), "reps": reps}
for _ in range(2):  # alternating rounds
    for name, fn in (("a_fused_voxel", fused), ("b_fused_cells", cells), ("c_merge", merge), ("d_b_plus_c", b_and_c)):
        fn()
        t = timed(fn, reps)
        res.setdefault(name, []).append(round(float(np.median(t)), 4))
for k in ("a_fused_voxel", "b_fused_cells", "c_merge", "d_b_plus_c"):
    res[k + "_ms"] = min(res.pop(k))
res["bytes"] = {"b_writes_records": 32 * ncells_b, "c_reads_records": 32 * res["records_c_in"],
                "c_writes_points": 16 * c_tot, "a_writes_points": 16 * a_tot,
                "c_merge_scratch_words": S * slot}
print(json.dumps(res))
