"""Worker of tests/test_gpu2_fused_cells.py (one process per rank, started by torch.distributed.run): ONE fused
voxel grid across ranks through the cell exchange (include/rplgpu_comm.h).  Every rank turns ITS sensors' scans of
the time step into cell records (rplgpu_cloud_fused_cells_dev, group = its sensors, motion + pose), packs its META
block, and gathers both to rank 0 (rplgpu_gather_cells_dev); rank 0 merges them (rplgpu_merge_cells_dev) and
serialises the fused PointCloud2.  It then builds the same message in one process — rplgpu_cloud_fused_voxel_dev
over all eight sensors + rplgpu_fused_cloud_msg_dev — and the two must be the same bytes.  Prints
RCCL_CELLS_OK <ranks> on rank 0."""
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rplidar_ros2_driver_amd import Params, RplGpu, abi, synth  # noqa: E402

FID = "base_link"


def main():
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    S, n = 8, 32000
    assert S % world == 0
    per = S // world
    batch = np.stack([synth.make_scan(700 + s, 0, n, noise_m=0.01) for s in range(S)])
    rng = np.random.default_rng(11)
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                       for _ in range(S)]).astype(np.float32)
    ang = rng.uniform(-3, 3, S)
    pose = np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, S), np.sin(ang), np.cos(ang),
                     rng.uniform(-2, 2, S)], 1).astype(np.float32)
    p = Params.defaults(clip_enable=1, range_max=40.0, ror_enable=1, voxel_enable=1)

    def on_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    with RplGpu(device=local, max_samples_per_scan=32768, max_batch=S) as gpu:
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(stream)
        gpu.set_stream(stream.cuda_stream)
        uid = torch.zeros(128, dtype=torch.uint8, device=dev)
        if rank == 0:
            uid.copy_(torch.from_numpy(RplGpu.comm_unique_id()))
        dist.broadcast(uid, src=0)
        gpu.comm_init(rank, world, uid.cpu().numpy())
        sl = slice(rank * per, (rank + 1) * per)
        d_nodes = on_dev(batch[sl].view(np.uint8).reshape(per, n * 8))
        d_len = torch.full((S,), n, dtype=torch.int32, device=dev)
        d_mo, d_po = on_dev(motion[sl]), on_dev(pose[sl])
        slot = per * n
        d_cells = torch.zeros(slot * 8, dtype=torch.int32, device=dev)  # 32-byte records
        cur = torch.zeros(1, dtype=torch.int64, device=dev)
        gs = torch.zeros(1, dtype=torch.int64, device=dev)
        nc = torch.zeros(1, dtype=torch.int32, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        gpu.cloud_fused_cells_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), per, per, p, d_mo.data_ptr(),
                                  d_po.data_ptr(), d_cells.data_ptr(), slot, cur.data_ptr(), gs.data_ptr(),
                                  nc.data_ptr(), st.data_ptr())
        mw = abi.cloud_meta_words(1)
        d_meta = torch.zeros(mw, dtype=torch.int32, device=dev)
        gpu.pack_cloud_meta_dev(cur.data_ptr(), gs.data_ptr(), nc.data_ptr(), 1, slot, 1, d_meta.data_ptr())
        root = 0
        all_c = torch.zeros(world, slot * 8, dtype=torch.int32, device=dev) if rank == root else None
        all_m = torch.zeros(world, mw, dtype=torch.int32, device=dev) if rank == root else None
        gpu.gather_cells_dev(root, d_cells.data_ptr(), slot, d_meta.data_ptr(), mw,
                             all_c.data_ptr() if rank == root else 0, all_m.data_ptr() if rank == root else 0)
        gpu.comm_fence()
        ok = True
        if rank == root:
            cap = S * n
            msg_cap = abi.msg_cloud_layout(len(FID), cap).total_len

            def message(arena, total):
                d_msg = torch.zeros(msg_cap, dtype=torch.uint8, device=dev)
                d_ml = torch.zeros(1, dtype=torch.int64, device=dev)
                d_ms = torch.zeros(1, dtype=torch.int32, device=dev)
                gpu.fused_cloud_msg_dev(arena.data_ptr(), total.data_ptr(), cap, FID, 5, 6, d_msg.data_ptr(),
                                        msg_cap, d_ml.data_ptr(), d_ms.data_ptr())
                gpu.synchronize()
                assert int(d_ms.item()) == 0
                return d_msg.cpu().numpy()[: int(d_ml.item())].tobytes()

            arena = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            mgs = torch.zeros(1, dtype=torch.int64, device=dev)
            mnp = torch.zeros(1, dtype=torch.int32, device=dev)
            mst = torch.zeros(1, dtype=torch.int32, device=dev)
            gpu.merge_cells_dev(all_c.data_ptr(), slot, all_m.data_ptr(), mw, world, 1, p, arena.data_ptr(), cap,
                                total.data_ptr(), mgs.data_ptr(), mnp.data_ptr(), mst.data_ptr())
            got = message(arena, total)
            # one process, all sensors, no exchange
            f_nodes = on_dev(batch.view(np.uint8).reshape(S, n * 8))
            f_mo, f_po = on_dev(motion), on_dev(pose)
            f_arena = torch.zeros(cap, 4, dtype=torch.float32, device=dev)
            f_total = torch.zeros(1, dtype=torch.int64, device=dev)
            gpu.cloud_fused_voxel_dev(f_nodes.data_ptr(), n, d_len.data_ptr(), S, S, p, f_mo.data_ptr(),
                                      f_po.data_ptr(), f_arena.data_ptr(), cap, f_total.data_ptr(), mgs.data_ptr(),
                                      mnp.data_ptr(), mst.data_ptr())
            want = message(f_arena, f_total)
            ok = got == want and int(total.item()) == int(f_total.item()) > 0
        gpu.comm_destroy()
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0 and int(flag.item()) == 1:
        print(f"RCCL_CELLS_OK {world}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
