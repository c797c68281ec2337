#!/usr/bin/env python3
"""bench.py — raw scans -> filtered, voxelised PointCloud2 on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of synthetic raw scans that is
already resident in HBM: BASELINE config 3 — 4096 scans x 32 000 samples (131 072 000
input samples, 1 048 576 000 B of packed 8-byte nodes) -> E1 quality/range clip -> polar->XYZ
-> 5 cm voxel grid (kernel ``k_cloud_voxel``), the clouds of all scans written to one
contiguous arena (every scan reserves exactly its cells; no packing pass).
With --gpus N > 1 (config 4) the SAME batch is sharded by scan index (strong scaling), each
rank processes its block in chunks and the voxelised clouds are all-gathered with RCCL over
xGMI through the library's own C entry points (rplgpu_comm_*), the gather of chunk k
overlapping the compute of chunk k + 1 on a second stream.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up,
times the K steps and reports them (``roofline`` from the events around those steps and the
committed traffic profile).  With --full the line also carries the measurements that take runs
of their own: ``roofline`` per-launch minimum and live HBM traffic, ``cpu_baseline`` (the CPU
oracle timed on this box's host cores on a bounded sample of the same buffers), ``variants`` (the
same 4096 x 32 000 shape on the other data regimes of SURVEY.md §8(d): 1 cm range noise, uniformly
random ranges, quality filter on), ``c5`` (8 sensors x 512 frames, E5 + E4, fused arena),
``single_scan_us`` (the node's per-scan entry points at the scan sizes the reference produces),
``decode`` (the step before the path, per answer type), the PCIe-inclusive rate and, for N > 1,
the compute-only and exchange-only loops.

--dump-outputs DIR writes what the last timed step computed as .npy files (see dump_outputs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s)
HBM_COPY_GBS = 6290.0   # achievable streaming rate (same guide; tools/ubench/cu_stream: 6.2-6.3 TB/s)
TRAFFIC_JSON = ROOT / "profiles" / "traffic.json"  # PMC-derived HBM bytes per launch (tools/prof.sh)


def static_traffic(kernel: str, B: int, n: int):
    """HBM bytes per launch of `kernel` from the COMMITTED rocprofv3 PMC passes
    (profiles/traffic.json, written by tools/prof_summary.py from separate --pmc runs of this
    very command, with the gfx950 FETCH_SIZE x2 correction of MI355X_MICROARCH.md).  Static:
    counters cannot be read from inside this process; None when no profile of this workload
    shape is on record."""
    try:
        rec = json.loads(TRAFFIC_JSON.read_text())
    except Exception:
        return None, None
    ent = rec.get(kernel)
    if not ent or ent.get("scans") != B or ent.get("samples_per_scan") != n:
        return None, None
    # the record names the kernel source it was measured on: a kernel edited since then gets no
    # traffic figure (re-run tools/prof.sh) instead of the old one
    want = ent.get("source_sha256")
    have = source_sha256(ent.get("source_files") or [ent.get("source_file",
                                                              "rplidar_ros2_driver_amd/csrc/rpl_voxel.hip")])
    if not want or want != have:
        return None, "stale: profiles/traffic.json was measured on another state of the kernel source " \
                     f"(recorded {str(want)[:12]}, now {str(have)[:12]}); re-run tools/prof.sh"
    return int(ent["hbm_bytes_per_launch"]), "static: " + str(ent.get("source"))


def live_traffic(args, B: int, n: int):
    """HBM bytes per launch of k_cloud_voxel measured on THIS box, now: two short child runs of this
    script's headline launch under `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes,
    counters only — never combined with a tracing domain), bytes = (2 x FETCH_SIZE + WRITE_SIZE) x 1024
    as MI355X_MICROARCH.md prescribes for gfx950 (FETCH_SIZE in KiB reports half of a wide streaming
    read).  Runs AFTER the timed region.  Returns (bytes, source note) or (None, reason): rocprofv3
    missing, a pass failing or taking longer than its limit all fall back to the committed figure."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    tmp = tempfile.mkdtemp(prefix="rplpmc_", dir="/tmp")
    child = [sys.executable, str(Path(__file__).resolve()), "--steps", "4", "--warmup", "1", "--cpu-seconds", "0",
             "--no-variants", "--no-single", "--no-laserscan", "--no-decode", "--no-live-traffic",
             "--scans", str(B), "--samples", str(n), "--seed", str(args.seed), "--out-stride", str(args.out_stride)]
    env = dict(os.environ, TMPDIR="/tmp")
    vals = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            r = subprocess.run([prof, "--pmc", ctr, "--output-format", "csv", "-d", out, "-o", "p", "--"] + child,
                               cwd="/tmp", env=env, capture_output=True, text=True, timeout=150)
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {ctr} failed (rc {r.returncode})"
            got = []
            for f in glob.glob(out + "/**/*counter_collection.csv", recursive=True):
                for row in csv.DictReader(open(f)):
                    if "k_cloud_voxel" in row["Kernel_Name"] and row["Counter_Name"] == ctr:
                        got.append(float(row["Counter_Value"]))
            if not got:
                return None, f"no {ctr} rows for k_cloud_voxel"
            vals[ctr] = (sum(got) / len(got), len(got))
    except subprocess.TimeoutExpired:
        return None, "rocprofv3 pass took longer than 150 s"
    except Exception as e:  # (a profiler problem must never cost the bench line)
        return None, f"live PMC pass failed: {type(e).__name__}: {e}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    f, w = vals["FETCH_SIZE"][0], vals["WRITE_SIZE"][0]
    return int((2.0 * f + w) * 1024), (
        f"live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes of this command's headline launch on this "
        f"box ({vals['FETCH_SIZE'][1]} + {vals['WRITE_SIZE'][1]} dispatches; FETCH_SIZE {f:.1f} KiB x 2 (gfx950) + "
        f"WRITE_SIZE {w:.1f} KiB)")


def source_sha256(rels):
    """one digest over the kernel's source file and what sets its launch geometry and store sizing
    (rpl_device.hpp, rpl_launch.hpp, rplgpu_api.hip: tools/prof_summary.py lists them per kernel)"""
    import hashlib
    h = hashlib.sha256()
    try:
        for rel in rels:
            h.update((ROOT / rel).read_bytes())
        return h.hexdigest()
    except Exception:
        return None


def host_cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except Exception:
        pass
    return None


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)  # (0.46 ms each: the timed region is ~50 ms)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scans", type=int, default=4096, help="scans in the whole batch (config 3)")
    ap.add_argument("--samples", type=int, default=32000, help="samples per scan")
    ap.add_argument("--out-stride", type=int, default=8192, help="cloud slots per scan")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--chunks", type=int, default=0,
                    help="N > 1: pieces a rank's block is cut into (gather of piece k overlaps "
                         "compute of piece k + 1)")
    ap.add_argument("--exchange", choices=["allgather", "gather"], default="allgather",
                    help="N > 1: every rank ends up with the whole voxelised cloud (all-gather, BASELINE "
                         "config 4) or only rank 0 does (gather to root, config 5's fused message: "
                         "rplgpu_gather_clouds_dev, one slot per link instead of one per link and direction)")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement (CPU baseline, reference-path kernels, data "
                         "regimes and config 5, decode stage, per-scan table, per-launch and live-traffic "
                         "roofline figures, PCIe-inclusive rate, N > 1 compute / exchange loops); the "
                         "--no-* and --cpu-seconds options below select among them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0,
                    help="target wall time of the CPU baseline sample (0 disables)")
    ap.add_argument("--no-laserscan", action="store_true",
                    help="skip the secondary ascend+LaserScan measurement")
    ap.add_argument("--no-variants", action="store_true",
                    help="skip the data-regime variants and the config-5 leg (they launch the "
                         "headline kernel on other batches; profiles of the headline launch use this)")
    ap.add_argument("--no-c5", action="store_true", help="alias of --no-variants (round-1 flag)")
    ap.add_argument("--no-decode", action="store_true",
                    help="skip the secondary decode-stage measurement (capsules -> nodes -> scans)")
    ap.add_argument("--no-single", action="store_true", help="skip the per-scan latency table")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not measure roofline.traffic with two rocprofv3 --pmc child runs (the committed "
                         "profiles/traffic.json figure is reported instead, when its source hash still matches)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: N ranks over gloo move synthetic clouds through the exchange layout "
                         "of the C ABI (host entry points) and check the result; exercises the spawn "
                         "path and the rendezvous of --gpus N on a CPU-only machine")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.warmup < 0:
        ap.error("--warmup must be >= 0")
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run with N
    ranks on this node (the contract's own launch line) and hand its output through."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["RPL_BENCH_SPAWNED"] = "1"
    return subprocess.call(cmd, env=env)


def dry_run(args, world, rank):
    """--dry-run: the N > 1 plumbing without a device.  Every rank lays a synthetic cloud out as
    rplgpu_cloud_arena_dev does, compacts it and builds its META block with the library's host
    entry points, the slots travel over gloo, and the unpacked cloud must be the concatenation."""
    import torch
    import torch.distributed as dist
    from rplidar_ros2_driver_amd import abi
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per_rank, rng = 3, np.random.default_rng(100 + rank)
    counts = rng.integers(5, 40, per_rank).astype(np.uint32)

    def cloud(r):
        g = np.random.default_rng(100 + r)
        c = g.integers(5, 40, per_rank).astype(np.uint32)
        pts = g.standard_normal((int(c.sum()), 4)).astype(np.float32)
        pts[:, 2] = 0.0
        return c, pts
    counts, pts = cloud(rank)
    slot = 200
    starts = (np.cumsum(counts) - counts).astype(np.uint64)
    arena = np.zeros((slot, 4), np.float32)
    arena[: len(pts)] = pts
    meta = abi.pack_cloud_meta_host(len(pts), starts, counts, slot, per_rank)
    mine = abi.pack_cloud_xyi_host(arena, len(pts), slot)
    all_pts = torch.empty(world * slot * 3)
    dist.all_gather_into_tensor(all_pts, torch.from_numpy(mine).view(-1))
    all_meta = torch.empty(world * len(meta), dtype=torch.int32)
    dist.all_gather_into_tensor(all_meta, torch.from_numpy(meta.view(np.int32).copy()))
    packed, st, npts, status = abi.unpack_gathered_host(
        all_pts.view(world, slot, 3).numpy(), slot, all_meta.numpy().view(np.uint32), world, per_rank)
    want = np.concatenate([cloud(r)[1] for r in range(world)])
    ok = packed.tobytes() == want.tobytes() and int(status.sum()) == 0 and int(npts.sum()) == len(want)
    if args.exchange == "gather":  # the gather to root (rplgpu_gather_clouds_dev's layout): rank 0 only
        from rplidar_ros2_driver_amd.sharding import gather_slots_to_root
        g_slots, g_meta = gather_slots_to_root(torch.from_numpy(mine).view(-1),
                                               torch.from_numpy(meta.view(np.int32).copy()), 0)
        if rank == 0:
            gp, _, gn, gs = abi.unpack_gathered_host(g_slots.view(world, slot, 3).numpy(), slot,
                                                     g_meta.numpy().view(np.uint32), world, per_rank)
            ok = ok and gp.tobytes() == want.tobytes() and int(gs.sum()) == 0 and int(gn.sum()) == len(want)
        else:
            ok = ok and g_slots is None
    t = torch.tensor([int(ok)])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "ok": bool(int(t.item())),
                          "points": int(len(packed)), "exchange": args.exchange,
                          "exchange_backend": "gloo (dry run, host layout entry points)"}))
    return 0 if int(t.item()) else 1


def cpu_baseline(batch_np, lens_np, params, target_s):
    """Time the CPU oracle (a port of the spec; the reference has no cloud path) on this
    host, all cores, on a bounded prefix of the same scans.  Only this function (and
    `cpu_single_scan`) touch oracle/."""
    from tests import oracle_lib

    orc = oracle_lib.load_oracle()
    op = oracle_lib.copy_params(params)
    import ctypes as C

    cores = os.cpu_count() or 1
    B, n = batch_np.shape

    def run(nscans, threads):
        nodes = np.ascontiguousarray(batch_np[:nscans])
        lens = np.ascontiguousarray(lens_np[:nscans].astype(np.uint32))
        t0 = time.perf_counter()
        tot = orc.lib.orc_batch_cloud(nodes.ctypes.data, n, lens.ctypes.data, nscans,
                                      C.byref(op), threads)
        return time.perf_counter() - t0, int(tot)

    probe = min(B, max(cores, 8))
    t, _ = run(probe, cores)
    rate = probe * n / max(t, 1e-9)
    nscans = int(min(B, max(probe, rate * target_s / n)))
    # the sample is bounded by the batch; repeat it so that the timing covers ~target_s of
    # wall time at most and take the best pass (the box's cores are shared with nothing else)
    passes, t_all, tot, spent = 0, float("inf"), 0, 0.0
    while passes < 3 or (spent < min(target_s, 6.0) and passes < 12):
        tp, tot = run(nscans, cores)
        t_all = min(t_all, tp)
        spent += tp
        passes += 1
    t_one_scans = min(nscans, 32)
    t_one, _ = run(t_one_scans, 1)
    # the reference's own per-scan loop (ascendScanData + publish_scan Mode A), same threads:
    # the oracle's restatement (pinned bit for bit against the genuine code, tests/golden/)
    pl = oracle_lib.copy_params(params)
    pl.clip_enable = 0
    nodes = np.ascontiguousarray(batch_np[:nscans]).copy()
    lens = np.ascontiguousarray(lens_np[:nscans].astype(np.uint32))
    t0 = time.perf_counter()
    orc.lib.orc_batch_ascend(nodes.ctypes.data, n, lens.ctypes.data, nscans, cores)
    t_asc = time.perf_counter() - t0
    t0 = time.perf_counter()
    orc.lib.orc_batch_laserscan(nodes.ctypes.data, n, lens.ctypes.data, nscans, C.byref(pl), cores)
    t_ls = time.perf_counter() - t0
    out = {
        "value": round(nscans * n / t_all / 1e6, 3),
        "unit": "Mpoints/s",
        "cores": cores,
        "cpu_model": host_cpu_model(),
        "kind": "port",
        "sample": f"first {nscans} scans x {n} samples of the same batch, best of {passes} "
                  f"passes ({t_all:.2f} s wall each, {cores * t_all:.0f} core-seconds), "
                  f"{cores} threads over scans (g++ -O2 oracle, clip + polar->XYZ + voxel)",
        "single_thread_value": round(t_one_scans * n / t_one / 1e6, 3),
        "cells_out": tot,
        "reference_path": {
            "kind": "port (restatement of ascendScanData / publish_scan, pinned bit for bit against "
                    "the genuine SDK and node: tests/golden/, tests/test_oracle_golden.py)",
            "ascend_mpts": round(nscans * n / t_asc / 1e6, 1),
            "laserscan_mpts": round(nscans * n / t_ls / 1e6, 1),
            "threads": cores,
        },
    }
    # the GENUINE reference code (oracle/_ref/, built from /root/reference where it exists and
    # shipped as binaries): one thread on a few scans, and every host core on >= 256 scans (the
    # calls are ctypes calls, which release the interpreter lock; one RPlidarNode / driver object
    # per call, no shared state between them)
    ref = oracle_lib.load_ref()
    if ref is not None:
        from concurrent.futures import ThreadPoolExecutor
        k = min(nscans, 16)
        # (in place on byte copies made beforehand: a numpy copy of the packed record dtype costs
        # more than the SDK call itself)
        work = [np.ascontiguousarray(batch_np[s]).view(np.uint8).copy() for s in range(k)]
        t0 = time.perf_counter()
        for s in range(k):
            ref.sl.ref_ascend(work[s].ctypes.data, n)
        t_ra = time.perf_counter() - t0
        del work
        t0 = time.perf_counter()
        for s in range(k):
            ref.publish_scan(batch_np[s], driver_kind=1, inverted=0, scan_processing=1,
                             range_max=40.0, scan_duration=0.1)
        t_rp = time.perf_counter() - t0
        out["reference_path_genuine"] = {
            "kind": "reference (oracle/_ref: the SDK's ascendScanData and the node's publish_scan "
                    "compiled from /root/reference), 1 thread",
            "ascend_mpts": round(k * n / t_ra / 1e6, 1),
            "laserscan_mpts": round(k * n / t_rp / 1e6, 1),
            "scans": k,
        }
        km = min(nscans, max(256, 2 * cores))
        workers = max(1, min(cores, km))
        work = [np.ascontiguousarray(batch_np[s]).view(np.uint8).copy() for s in range(km)]

        def asc_slice(w):
            for s in range(w, km, workers):
                ref.sl.ref_ascend(work[s].ctypes.data, n)

        def pub_slice(w):
            for s in range(w, km, workers):
                ref.publish_scan(batch_np[s], driver_kind=1, inverted=0, scan_processing=1,
                                 range_max=40.0, scan_duration=0.1)
        try:
            with ThreadPoolExecutor(workers) as ex:
                t0 = time.perf_counter()
                list(ex.map(asc_slice, range(workers)))
                t_ma = time.perf_counter() - t0
                t0 = time.perf_counter()
                list(ex.map(pub_slice, range(workers)))
                t_mp = time.perf_counter() - t0
            out["reference_path_genuine"]["all_cores"] = {
                "threads": workers, "scans": km,
                "ascend_mpts": round(km * n / t_ma / 1e6, 1),
                "laserscan_mpts": round(km * n / t_mp / 1e6, 1),
                "note": "Python threads over ctypes calls into the genuine libraries (the wrapper's "
                        "per-call allocations included)",
            }
        except Exception as e:  # (a baseline leg must not take the bench down)
            out["reference_path_genuine"]["all_cores"] = {"error": str(e)}
        del work
    return out


def timed(fn, stream, reps, sync):
    """Back-to-back launches between two events on the launch stream: ms per call."""
    import torch
    fn()
    sync()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    sync()
    return a.elapsed_time(b) / reps


def decode_stage(gpu, dev, stream, cpu_seconds):
    """Secondary measurement (not `value`): the step before the path, SURVEY.md §8(f) rows 1-2.
    4096 recorded streams per answer type (resident in HBM) -> k_decode (sync list + scans
    written straight into the batch layout where the type allows), plus the CPU oracle
    restatement of the SDK unpacker on one core for DenseBoost."""
    import torch

    from rplidar_ros2_driver_amd import capsules as cp

    B = 4096
    out = {}
    sync = lambda: torch.cuda.synchronize(dev)
    # ("ultra_dense": the generator's 2.5-5.5 m ring clamped to that format's scale 0, i.e. a CONSTANT
    # 2046 mm — the one input on which the smoothing pass has to walk every segment twice;
    # "ultra_dense_near": a noiseless 0.9-1.9 m ring — runs of equal 2 mm codes, the smoothing pass's
    # hardest input; "ultra_dense_noisy": the same ring with 4 mm of range noise, what a sensor sends)
    for name, ans, nf, payload in (("dense", cp.ANS_DENSE_CAPSULED, 801, "ring"),
                                   ("express", cp.ANS_CAPSULED, 1001, "ring"),
                                   ("ultra", cp.ANS_CAPSULED_ULTRA, 334, "ring"),
                                   ("ultra_dense", cp.ANS_ULTRA_DENSE_CAPSULED, 501, "ring"),
                                   ("ultra_dense_near", cp.ANS_ULTRA_DENSE_CAPSULED, 501, "ring_near"),
                                   ("ultra_dense_noisy", cp.ANS_ULTRA_DENSE_CAPSULED, 501, "ring_noisy"),
                                   ("hq", cp.ANS_HQ, 334, "ring"),
                                   ("normal", cp.ANS_MEASUREMENT, 4000, "ring")):
        S, npf = cp.FRAME_SIZE[ans], cp.NODES_PER_FRAME[ans]
        uniq = 16  # distinct streams (host generation time); the batch repeats them
        # two revolutions per stream so that scan assembly has one complete scan to cut out
        base = np.stack([cp.make_stream(ans, nf, 10 + s, payload=payload, frames_per_rev=nf / 2.0 + 0.3)
                         for s in range(uniq)])
        buf = torch.from_numpy(base).to(dev).repeat(B // uniq, 1).contiguous()
        d_nf = torch.full((B,), nf, dtype=torch.int32, device=dev)
        node_stride = nf * npf
        d_nodes = torch.empty(B, node_stride * 8, dtype=torch.uint8, device=dev)
        d_nn = torch.zeros(B, dtype=torch.int32, device=dev)
        d_rst = torch.zeros(B, 8, dtype=torch.int32, device=dev)
        d_nr = torch.zeros(B, dtype=torch.int32, device=dev)

        def dec():
            gpu.decode_batch_dev(ans, 125, buf.data_ptr(), nf * S, 0, 0, d_nf.data_ptr(), nf, B, 0, 0,
                                 d_nodes.data_ptr(), node_stride, d_nn.data_ptr(), d_rst.data_ptr(), 8,
                                 d_nr.data_ptr())

        ms = timed(dec, stream, 5, sync)
        nodes = int(d_nn.sum().item())
        gbs = (B * nf * S + 8 * nodes) / ms / 1e6
        out[name] = {"ms": round(ms, 4), "gnodes_s": round(nodes / ms / 1e6, 1), "gbs": round(gbs, 1),
                     "frac": round(gbs / HBM_PEAK_GBS, 4)}
        if ans == cp.ANS_DENSE_CAPSULED:
            d_seg = torch.empty_like(d_nodes)
            scan_cap = 8
            d_off = torch.zeros(B, scan_cap + 1, dtype=torch.int32, device=dev)
            d_ns = torch.zeros(B, dtype=torch.int32, device=dev)

            def seg():
                gpu.segment_batch_dev(d_nodes.data_ptr(), node_stride, d_nn.data_ptr(), d_rst.data_ptr(),
                                      8, d_nr.data_ptr(), B, 32768, d_seg.data_ptr(), node_stride,
                                      d_off.data_ptr(), scan_cap, d_ns.data_ptr())

            out["segment_ms"] = round(timed(seg, stream, 5, sync), 4)
            out["segment_scans"] = int(d_ns.sum().item())
            del d_seg
            # the same step in ONE call: the decoder's sync list, completed scans written straight
            # into batch slots (rplgpu_decode_scans_dev) — what replaces decode + segment + to_batch
            scap, nst = 4, min(node_stride, 32768)
            d_batch = torch.empty(B * scap, nst * 8, dtype=torch.uint8, device=dev)
            d_len = torch.zeros(B * scap, dtype=torch.int32, device=dev)
            d_st2 = torch.zeros(B, dtype=torch.int32, device=dev)

            def fused_scans():
                gpu.decode_scans_dev(ans, 125, buf.data_ptr(), nf * S, 0, 0, d_nf.data_ptr(), nf, B, 0, 0,
                                     32768, d_batch.data_ptr(), nst, scap, d_len.data_ptr(), d_ns.data_ptr(),
                                     0, d_st2.data_ptr())

            ms2 = timed(fused_scans, stream, 5, sync)
            kept = int(d_len.to(torch.int64).sum().item())
            out["decode_scans"] = {"ms": round(ms2, 4), "scans": int(d_ns.sum().item()), "nodes_in_scans": kept,
                                   "status_bits": int(d_st2.max().item()),
                                   "frac": round((B * nf * S + 8 * kept) / ms2 / 1e6 / HBM_PEAK_GBS, 4)}
            del d_batch
            if cpu_seconds > 0:  # the oracle restatement of the SDK unpacker, one core, one stream
                from tests import oracle_lib

                orc = oracle_lib.load_oracle()
                orc.unpack(ans, base[0], 125)
                t0 = time.perf_counter()
                reps = 0
                while time.perf_counter() - t0 < min(cpu_seconds, 2.0):
                    orc.unpack(ans, base[reps % uniq], 125)
                    reps += 1
                out["dense_cpu1_mnodes"] = round(reps * (nf - 1) * npf / (time.perf_counter() - t0) / 1e6, 1)
        del buf, d_nodes
    return out


def regime(gpu, dev, stream, name, batch_np, params, arena, cursor, start, npts, stat, reps):
    """One data regime at the full batch shape: k_cloud_voxel (E5, when on, inside it or as k_ror_mask in
    front of it: rplgpu_set_ror_mode) into the arena; ms per launch, Gpts/s, roofline fractions.  Returns (dict, cells)."""
    import torch

    B, n = batch_np.shape
    d_nodes = torch.from_numpy(batch_np.view(np.uint8).reshape(B, n * 8)).to(dev)
    d_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    cap = arena.shape[0]

    def fn():
        gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, params, arena.data_ptr(),
                            cap, cursor.data_ptr(), start.data_ptr(), npts.data_ptr(), stat.data_ptr())

    ms = timed(fn, stream, reps, lambda: torch.cuda.synchronize(dev))
    cells = int(cursor.item())
    st = int(stat.max().item())
    algo = 8 * B * n + 16 * cells
    res = {"ms": round(ms, 4), "gpts_s": round(B * n / ms / 1e6, 1),
           "frac": round(algo / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "frac_read": round(8 * B * n / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "cells": cells, "status_bits": st}
    del d_nodes
    return res


def single_scan_table(gpu, params_voxel, seed, cpu_seconds):
    """The drop-in seam, one scan at a time through the host-buffer entry points the node calls
    (wall clock per call: copies, kernels, synchronisation), at the scan sizes the reference
    produces (360 Standard / ~3 200 DenseBoost S2 / 8 192 = the SDK's buffer,
    src/lidar_driver_wrapper.cpp:316-318 / 32 000 config 2), next to the CPU loop it replaces."""
    from rplidar_ros2_driver_amd import Params, synth

    table = {}
    pl1 = Params.defaults(range_max=40.0)
    pin = gpu.host_alloc(1 << 20)
    params_ror = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0,
                                 voxel_enable=1, voxel_leaf=0.05, ror_enable=1, ror_radius=0.10,
                                 ror_min_neighbors=2)
    for n in (360, 3200, 8192, 32000):
        one = synth.make_scan(seed, 9000 + n, n)
        # ascend works in place: every call gets a fresh copy of the scan — as a byte memcpy (a
        # numpy copy of the packed record dtype goes element by element: 200 us at 32 000 nodes,
        # which round 2's first table had inside both the GPU and the CPU ascend figures)
        raw = np.ascontiguousarray(one).view(np.uint8).copy()
        work_u8 = raw.copy()
        work = work_u8.view(one.dtype)

        def fresh():
            np.copyto(work_u8, raw)
            return work

        row = {}
        for name, fn in (
            ("laserscan", lambda: gpu.scan_to_laserscan(one, pl1, 0.1)),
            ("laserscan_msg_pinned", lambda: gpu.scan_to_laserscan_msg(one, pl1, 0.1, "laser_frame",
                                                                       1, 2, out=pin)),
            ("ascend", lambda: gpu.ascend(fresh())),
            ("voxel_cloud", lambda: gpu.scan_to_cloud(one, params_voxel)),
            ("ror_voxel_cloud", lambda: gpu.scan_to_cloud(one, params_ror)),
            ("voxel_cloud_msg_pinned", lambda: gpu.scan_to_cloud_msg(one, params_voxel, "laser_frame",
                                                                     1, 2, out=pin)),
        ):
            for _ in range(20):
                fn()
            reps = 200
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            row[name] = round((time.perf_counter() - t0) / reps * 1e6, 1)
        if cpu_seconds > 0:  # the CPU loops the node runs today, same scan, one core
            from tests import oracle_lib
            orc = oracle_lib.load_oracle()
            op = oracle_lib.copy_params(pl1)
            for name, fn in (("cpu_publish_scan", lambda: orc.publish_scan(one, op, 0.1)),
                             ("cpu_ascend", lambda: orc.lib.orc_ascend(fresh().ctypes.data, n))):
                t0 = time.perf_counter()
                reps = 0
                while time.perf_counter() - t0 < 0.25:
                    fn()
                    reps += 1
                row[name] = round((time.perf_counter() - t0) / reps * 1e6, 1)
        table[str(n)] = row
    gpu.host_free(pin)
    return table


DUMP_BYTES_MAX = 64_000_000  # --dump-outputs: all files together
DUMP_SCANS = 512             # scans whose voxelised clouds are written in full (~22 MB on config 3)


def dump_outputs(out_dir, seed, d_arena, d_cursor, d_start, d_np, d_st):
    """--dump-outputs: what a caller of rplgpu_cloud_arena_dev receives from the last timed step.

    n_points.npy / status.npy   per scan (float64, exact), cells_total.npy the arena cursor;
    cloud_sample.npy            the clouds (x, y, z, intensity; float32) of a fixed, seeded sample of
                                scans, concatenated in the order of cloud_sample_scans.npy (their scan
                                indices), each scan's cells in the library's order.
    The arena offsets (d_scan_start) are not written: scans lie in the arena in completion order, which
    differs from run to run; the per-scan slices do not."""
    import torch
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    start = d_start.cpu().numpy().astype(np.int64)
    npts = d_np.cpu().numpy().astype(np.int64)
    B = len(npts)
    head = {"n_points": npts.astype(np.float64),
            "status": d_st.cpu().numpy().astype(np.uint32).astype(np.float64),
            "cells_total": np.array([float(d_cursor.item())], np.float64)}
    pick = np.sort(np.random.default_rng(seed).permutation(B)[:min(B, DUMP_SCANS)])
    # (a fixed prefix of the sample, cut where the byte budget would be exceeded)
    budget = DUMP_BYTES_MAX - sum(a.nbytes for a in head.values()) - 8 * len(pick) - 4096
    keep = np.cumsum(16 * npts[pick]) <= budget
    pick = pick[: int(np.argmin(keep)) if not keep.all() else len(pick)]
    parts = [d_arena[int(start[b]): int(start[b]) + int(npts[b])] for b in pick]
    cloud = torch.cat(parts).cpu().numpy() if parts else np.zeros((0, 4), np.float32)
    head["cloud_sample_scans"] = pick.astype(np.float64)
    head["cloud_sample"] = np.ascontiguousarray(cloud, dtype=np.float32)
    for name, arr in head.items():
        np.save(out / f"{name}.npy", arr)


def main():
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: start the ranks ourselves (and fail if they cannot all come up)
        if not args.dry_run:
            import torch
            if not torch.cuda.is_available() or torch.cuda.device_count() < args.gpus:
                have = torch.cuda.device_count() if torch.cuda.is_available() else 0
                raise SystemExit(f"--gpus {args.gpus} but only {have} HIP device(s) are visible")
        raise SystemExit(spawn_ranks(args))
    # stdout carries ONE JSON line: everything the libraries print there (RCCL's version banner
    # ...) is sent to stderr while the bench runs
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist

    from rplidar_ros2_driver_amd import Params, RplGpu, synth
    from rplidar_ros2_driver_amd.sharding import CloudExchange, best_chunks, launch_rel, predicted_step_ms, shard_range

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:  # (a launcher that started fewer or more ranks than --gpus asks for)
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the bench does not run with "
                         "a different number of ranks than it was asked for")
    if args.dry_run:
        os.dup2(real_stdout, 1)
        raise SystemExit(dry_run(args, world, rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback exists)")
    if torch.cuda.device_count() < args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} HIP device(s) are visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # RPL_BENCH_FORCE_DIST=1: run the N > 1 code path (process group, exchange, max over ranks)
    # with a single rank — the only way to exercise it on a 1-GPU box
    use_dist = world > 1 or os.environ.get("RPL_BENCH_FORCE_DIST") == "1"
    if use_dist and args.dump_outputs:
        raise SystemExit("--dump-outputs writes the single-rank path's outputs; it is not available with "
                         "--gpus N > 1 or RPL_BENCH_FORCE_DIST=1")
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    B_total, n = args.scans, args.samples
    lo, hi = shard_range(B_total, world, rank)
    B = hi - lo
    out_stride = args.out_stride
    no_variants = args.no_variants or args.no_c5

    # ---- synthetic input, generated on the host then made resident in HBM --------------
    t0 = time.perf_counter()
    batch_np = synth.make_batch(args.seed, B, n, first_scan=lo)
    gen_s = time.perf_counter() - t0
    lens_np = np.full(B, n, np.int32)
    h_nodes = torch.from_numpy(batch_np.view(np.uint8).reshape(B, n * 8))
    d_nodes = h_nodes.to(dev)
    d_len = torch.from_numpy(lens_np).to(dev)
    d_np = torch.zeros(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    # the voxelised clouds of the whole batch go to one contiguous arena (every scan reserves
    # exactly its cells): no packing pass, and the all-gather payload for N > 1 as it is
    arena_cap = B * out_stride
    d_arena = torch.empty(arena_cap, 4, dtype=torch.float32, device=dev)
    d_cursor = torch.zeros(1, dtype=torch.int64, device=dev)
    d_start = torch.zeros(B, dtype=torch.int64, device=dev)

    params = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0,
                             voxel_enable=1, voxel_leaf=0.05)
    gpu = RplGpu(device=local_rank, max_samples_per_scan=32768, max_batch=max(B, 1))
    # a real (non-null) stream shared by torch and the library, so that HIP events
    # recorded through torch bracket exactly the library's kernels
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    gpu.set_stream(stream.cuda_stream)

    def compute_only_step():
        gpu.cloud_arena_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, params,
                            d_arena.data_ptr(), arena_cap, d_cursor.data_ptr(),
                            d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())

    exch = None
    if use_dist:
        # N > 1: the library's own exchange (RCCL behind the C ABI): the rank's block is cut into
        # chunks; chunk k is voxelised into arena half (k & 1) while chunk k - 1 is gathered
        # (auto: with one rank there is no transfer to hide, so one chunk = one launch; with peers
        # two chunks, so that the first half's clouds travel while the second half is voxelised)
        # (round 5: with peers the chunk count comes from DESIGN.md section 7's model — sharding.best_chunks: more
        # chunks hide more of the exchange under compute, but every chunk is a launch with its own fixed cost and,
        # below one scan per compute unit, idle units; a priori figures: the one-GPU launch time of this workload
        # and 12 bytes x ~2670 cells per scan of cloud)
        if args.chunks > 0:
            n_chunks = args.chunks
        else:
            n_chunks = best_chunks(world, 0.449 * launch_rel(B_total) / launch_rel(4096), 12.0 * 2670.0 * B_total,
                                   B_total)
        exch = CloudExchange(gpu, dist, dev, world, rank, B, n, out_stride, n_chunks,
                             root=0 if args.exchange == "gather" else None)
        if exch.native and exch.comm_ranks != world:
            raise SystemExit(f"--gpus {args.gpus}: the RCCL communicator spans {exch.comm_ranks} rank(s), "
                             f"not {world}")

    def step():
        if exch is None:
            compute_only_step()
        else:
            exch.step(d_nodes, d_len, params)

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    fence()
    # the K timed steps: wall clock between two fences (the contract), and HIP events on the launch
    # stream around the SAME K steps (the device time of the launches alone, <= the wall time)
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev_a.record(stream)
    for _ in range(args.steps):
        step()
    ev_b.record(stream)
    fence()
    elapsed = time.perf_counter() - t0
    loop_dev_ms = ev_a.elapsed_time(ev_b) / args.steps
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:  # (before any later leg reuses the arena and the per-scan words)
        dump_outputs(args.dump_outputs, args.seed, d_arena, d_cursor, d_start, d_np, d_st)

    # N > 1 (--full): the same K steps without the exchange, and the exchange alone
    compute_only = None
    if use_dist and args.full:
        def timed_loop(fn):
            fence()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            fence()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item()) / args.steps * 1e3
        ms_c = timed_loop(compute_only_step)
        ms_x = timed_loop(exch.exchange_only)
        compute_only = {"value": round(B_total * n / ms_c / 1e3, 1), "ms_per_step": round(ms_c, 4),
                        "exchange_only_ms": round(ms_x, 4),
                        "overlapped_ms": round(elapsed / args.steps * 1e3, 4),
                        "gathered_bytes_per_rank": exch.last_bytes(),
                        "exchange_backend": exch.backend, "chunks": exch.chunks,
                        "comm_ranks": exch.comm_ranks, "exchange": args.exchange,
                        "model_ms_per_step": round(predicted_step_ms(
                            world, ms_c * world, 12.0 * world * exch.chunks * (exch.slot or 0), exch.chunks,
                            scans_total=B_total), 4),
                        # both exchanges' rows: the model prices them the same — see
                        # sharding.predicted_step_ms — so one row per chunk count serves both
                        "model_rows_ms": {str(c): round(predicted_step_ms(
                            world, ms_c * world, 12.0 * world * exch.chunks * (exch.slot or 0), c,
                            scans_total=B_total), 4) for c in (1, 2, 4, 8)},
                        "model_note": "DESIGN.md section 7: a piece = one launch over the rank's scans / chunks (measured "
                                      "launch-time curve) + its slot on one 76.8 GB/s link + 0.015 ms, pieces "
                                      "pipelined; measured = overlapped_ms; chunks chosen by the same model; "
                                      "all-gather and gather-to-root are priced the same (the root's inbound slots "
                                      "arrive on different links; nothing with two ranks has been measured)",
                        "note": "compute = the rank's whole block in one launch, no exchange; "
                                "exchange_only = RCCL all-gather of the last step's clouds; "
                                "overlapped = the timed step (chunked, two streams)"}
    if use_dist:
        compute_only_step()  # (status / cells below refer to the plain launch)
        torch.cuda.synchronize(dev)

    status = int(d_st.max().item())
    cells_local = int(d_cursor.item())

    # PCIe-inclusive rate (NOT `value`, --full): the same batch handed over as a pinned host buffer
    h2d_ms = None
    if args.full and rank == 0 and world == 1:
        try:
            h_pin = h_nodes.pin_memory()
            d_tmp = torch.empty_like(d_nodes)
            d_tmp.copy_(h_pin, non_blocking=True)
            torch.cuda.synchronize(dev)
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            d_tmp.copy_(h_pin, non_blocking=True)
            b_.record(stream)
            torch.cuda.synchronize(dev)
            h2d_ms = a.elapsed_time(b_)
            del d_tmp, h_pin
        except Exception:
            h2d_ms = None

    # ---- dominant kernel alone: HIP events on the launch stream ---------------------------
    # back to back (the figure the roofline uses: one event pair around `reps` launches, so the
    # gaps between an event and a launch are not counted reps times) and per launch (min, --full)
    reps = max(args.steps, 5)
    # N = 1: the step IS the launch, so the kernel's average duration is the device time of the
    # timed loop itself; N > 1: the step also holds the exchange, the launch is timed on its own (--full)
    k_ms_b2b = loop_dev_ms if exch is None else None
    k_ms_min = None
    if args.full:
        if exch is not None:
            k_ms_b2b = timed(compute_only_step, stream, reps, lambda: torch.cuda.synchronize(dev))
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(reps)]
        for a, b in ev:
            a.record(stream)  # the same launch as in the step (k_cloud_voxel + two tiny memsets)
            compute_only_step()
            b.record(stream)
        torch.cuda.synchronize(dev)
        k_ms_min = min(a.elapsed_time(b) for a, b in ev)
    algo_bytes = 8 * B * n + 16 * cells_local  # 8 B read/sample + 16 B/cell out
    achieved = None if k_ms_b2b is None else algo_bytes / (k_ms_b2b * 1e-3) / 1e9

    extra = {}
    sync = lambda: torch.cuda.synchronize(dev)
    if args.full and not args.no_laserscan:
        # secondary: the reference's own path (ascend + publish_scan Mode A) on a copy
        d_nodes2 = d_nodes.clone()
        d_r = torch.empty(B, n, dtype=torch.float32, device=dev)
        d_i = torch.empty(B, n, dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
        pl = Params.defaults(range_max=40.0)
        res = {}
        for name, fn in (
            ("ascend", lambda: gpu.ascend_batch_dev(d_nodes2.data_ptr(), n, d_len.data_ptr(), B,
                                                    d_st.data_ptr())),
            ("laserscan", lambda: gpu.laserscan_batch_dev(
                d_nodes2.data_ptr(), n, d_len.data_ptr(), B, pl, d_r.data_ptr(),
                d_i.data_ptr(), d_cnt.data_ptr())),
        ):
            ts = []
            for it in range(4):
                if name == "ascend":
                    d_nodes2.copy_(d_nodes)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                torch.cuda.synchronize(dev)
                ts.append(a.elapsed_time(b))
            res[name] = min(ts[1:])
        valid = int(d_cnt.to(torch.int64).sum().item())

        def ascend_row(d_src, Bv, ms):
            """what the call did to the batch: nodes rewritten (filled angle word or moved by the
            sort), scans whose nodes were reordered; algorithmic bytes = 8 read per node + 8 written
            per node that changed"""
            d_w = d_src.clone()
            gpu.ascend_batch_dev(d_w.data_ptr(), n, d_len.data_ptr(), Bv, d_st.data_ptr())
            torch.cuda.synchronize(dev)
            a, b = d_src.view(Bv, n, 8), d_w.view(Bv, n, 8)
            changed = int((a != b).any(dim=2).sum().item())
            reordered = int((a[:, :, 2:6] != b[:, :, 2:6]).any(dim=2).any(dim=1).sum().item())
            del d_w
            return {"ms": round(ms, 4), "gpts_s": round(Bv * n / ms / 1e6, 1), "scans": Bv,
                    "nodes_rewritten_frac": round(changed / (Bv * n), 4),
                    "scans_reordered_frac": round(reordered / Bv, 4),
                    "frac": round((8 * Bv * n + 8 * changed) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

        asc = {"uniform_angles": ascend_row(d_nodes, B, res["ascend"])}
        asc["uniform_angles"]["note"] = "the headline batch: exactly uniform angle words, the fill pass " \
            "recomputes the word already there and nothing needs the sort — the best case"
        Bv = B  # (round 5: the regimes at the full batch, like the headline row — rounds 3-4 used 1024 scans,
        # where ramp-up and tail of the launch weigh four times as much)
        for name, jit, note in (
                ("jitter1", 1, "valid samples' angle words jittered by +-1 (step 2.05): every filled word "
                               "differs from the stored one (8-byte stores), the order survives"),
                ("jitter3", 3, "jitter +-3: neighbouring samples swap in every scan; repaired inside the "
                               "streaming kernel (odd-even transposition per 128-sample chunk, 32-sample "
                               "windows across chunk boundaries, wrapped fills moved to the front); only a "
                               "scan that fails the final order check goes to the sorting kernel"),
                ("jitter10", 10, "jitter +-10: samples up to ~10 places from their sorted position, 89 % of "
                                 "the nodes rewritten; still repaired in the streaming pass"),
                ("jitter20", 20, "jitter +-20: disorder reaches past the 32-sample repair windows in part of the scans; "
                                 "round 6: those boundaries are repaired by merging the two sorted 128-sample chunks "
                                 "(phase C), nothing goes to the sorting kernel any more"),
                ("jitter64", 64, "jitter +-64 (round 6): nodes up to ~40 places from home; every chunk needs dozens of "
                                 "odd-even rounds and every boundary a merge, still one launch of the streaming kernel "
                                 "(round 5: every scan through the one-workgroup sort, 2.6 ms)")):
            vb = synth.make_batch(args.seed + 11, Bv, n, jitter=jit)
            d_v = torch.from_numpy(vb.view(np.uint8).reshape(Bv, n * 8)).to(dev)
            d_w = d_v.clone()
            ts = []
            for it in range(4):
                d_w.copy_(d_v)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                gpu.ascend_batch_dev(d_w.data_ptr(), n, d_len.data_ptr(), Bv, d_st.data_ptr())
                b.record(stream)
                torch.cuda.synchronize(dev)
                ts.append(a.elapsed_time(b))
            asc[name] = ascend_row(d_v, Bv, min(ts[1:]))
            asc[name]["note"] = note
            del vb, d_v, d_w
        extra["reference_path_gpu"] = {
            "ascend_ms": round(res["ascend"], 4),
            "laserscan_ms": round(res["laserscan"], 4),
            "ascend_mpts": round(B * n / res["ascend"] / 1e3, 1),
            "laserscan_mpts": round(B * n / res["laserscan"] / 1e3, 1),
            "ascend_frac": asc["uniform_angles"]["frac"],
            "ascend_regimes": asc,
            "laserscan_frac": round((8 * B * n + 8 * valid) / (res["laserscan"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        }
        # S1 -> S3 as the node runs them (grab_scan_data with geometric correction, then publish_scan)
        # through rplgpu_ascend_laserscan_batch_dev: the LaserScan does not depend on the ascend step
        # (include/rplgpu.h), so ONE pass over the raw nodes; the two-kernel figure next to it
        ts = []
        for it in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            gpu.ascend_laserscan_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, pl, d_r.data_ptr(),
                                           d_i.data_ptr(), d_cnt.data_ptr())
            b.record(stream)
            torch.cuda.synchronize(dev)
            ts.append(a.elapsed_time(b))
        fused_ms = min(ts[1:])
        extra["reference_path_gpu"]["ascend_laserscan_one_pass"] = {
            "ms": round(fused_ms, 4), "two_kernels_ms": round(res["ascend"] + res["laserscan"], 4),
            "frac": round((8 * B * n + 8 * valid) / (fused_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "note": "LaserScans of the batch as grab_scan_data + publish_scan deliver them, ascended nodes "
                    "not requested: 8 B read + 8 B written per valid sample, once"}
        # secondary: the LaserScans of the batch as serialised (CDR) messages in HBM, and the
        # LaserScans projected to clouds (E7, laser_geometry-style)
        from rplidar_ros2_driver_amd import abi as _abi
        fid = "laser_frame"
        mstride = _abi.msg_laserscan_layout(len(fid), n).total_len
        d_msgs = torch.empty(B, mstride, dtype=torch.uint8, device=dev)
        d_ml = torch.zeros(B, dtype=torch.int32, device=dev)
        d_stamps = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        d_dur = torch.full((B,), 0.1, dtype=torch.float64, device=dev)
        ms = timed(lambda: gpu.laserscan_msgs_dev(d_r.data_ptr(), d_i.data_ptr(), n, d_cnt.data_ptr(), B,
                                                  pl, fid, d_stamps.data_ptr(), d_dur.data_ptr(),
                                                  d_msgs.data_ptr(), mstride, d_ml.data_ptr(), 0),
                   stream, 3, sync)
        msg_bytes = int(d_ml.to(torch.int64).sum().item())
        extra["reference_path_gpu"]["laserscan_msgs_ms"] = round(ms, 4)
        extra["reference_path_gpu"]["laserscan_msgs_gbps_rw"] = round(2 * msg_bytes / ms / 1e6, 1)
        del d_msgs
        d_pc = torch.empty(B, n, 4, dtype=torch.float32, device=dev)
        ms = timed(lambda: gpu.laserscan_to_cloud_batch_dev(d_r.data_ptr(), d_i.data_ptr(), n,
                                                            d_cnt.data_ptr(), B, pl, d_pc.data_ptr(), n,
                                                            d_np.data_ptr(), d_st.data_ptr()),
                   stream, 3, sync)
        pts = int(d_np.to(torch.int64).sum().item())
        extra["reference_path_gpu"]["laserscan_to_cloud_ms"] = round(ms, 4)
        extra["reference_path_gpu"]["laserscan_to_cloud_frac"] = round(
            (8 * valid + 16 * pts) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        del d_nodes2, d_r, d_i, d_pc

    variants = None
    c5 = None
    if args.full and not no_variants and rank == 0 and world == 1:
        # the other data regimes of SURVEY.md §8(d) at the SAME shape (4096 x 32 000), same kernel
        vreps = max(3, min(args.steps, 10))
        variants = {"ring_clean": {"ms": round(k_ms_b2b, 4), "gpts_s": round(B * n / k_ms_b2b / 1e6, 1),
                                   "frac": round(achieved / HBM_PEAK_GBS, 4),
                                   "frac_read": round(8 * B * n / (k_ms_b2b * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                   "cells": cells_local, "status_bits": status}}
        pq = Params.defaults(clip_enable=1, q_min=48, range_min=0.15, range_max=40.0, voxel_enable=1,
                             voxel_leaf=0.05)
        variants["ring_clean_q_min48"] = regime(gpu, dev, stream, "q", batch_np, pq, d_arena, d_cursor,
                                                d_start, d_np, d_st, vreps)
        big_arena = torch.empty(B * n, 4, dtype=torch.float32, device=dev) if B * n * 16 < 8e9 else d_arena
        if big_arena is not d_arena:
            # the UNVOXELISED cloud of the same batch (E1 + E2 + E3: k_cloud, rplgpu_cloud_batch_dev):
            # 8 B read + 16 B written per kept sample
            pc = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0)

            def plain_cloud():
                gpu.cloud_batch_dev(d_nodes.data_ptr(), n, d_len.data_ptr(), B, pc, big_arena.data_ptr(), n,
                                    d_np.data_ptr(), d_st.data_ptr())
            ms_pc = timed(plain_cloud, stream, vreps, lambda: torch.cuda.synchronize(dev))
            pts_pc = int(d_np.to(torch.int64).sum().item())
            variants["plain_cloud_no_voxel"] = {
                "ms": round(ms_pc, 4), "gpts_s": round(B * n / ms_pc / 1e6, 1), "points": pts_pc,
                "frac": round((8 * B * n + 16 * pts_pc) / (ms_pc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "frac_read": round(8 * B * n / (ms_pc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "status_bits": int(d_st.max().item()),
                "note": "k_cloud: the same batch without the voxel grid, one 16-byte point per kept sample "
                        "in its scan's region (write bound: 1.9 GB out for 1.05 GB in)"}
        for name, kw in (("ring_noise_1cm", dict(noise_m=0.01)), ("uniform", dict(kind="uniform"))):
            vb = synth.make_batch(args.seed, B, n, **kw)
            variants[name] = regime(gpu, dev, stream, name, vb, params, big_arena, d_cursor, d_start,
                                    d_np, d_st, vreps if name != "uniform" else 3)
            del vb
        # BASELINE config 5 at throughput scale: 8 sensors x 512 frames of 32 000 samples with 1 cm
        # range noise, E5 radius-outlier removal + E4 voxel grid into one fused arena
        c5b = synth.make_batch(args.seed + 5, B, n, noise_m=0.01)
        p5 = Params.defaults(clip_enable=1, q_min=0, range_min=0.15, range_max=40.0, voxel_enable=1,
                             voxel_leaf=0.05, ror_enable=1, ror_radius=0.10, ror_min_neighbors=2)
        c5 = regime(gpu, dev, stream, "c5", c5b, p5, big_arena, d_cursor, d_start, d_np, d_st, vreps)
        c5["workload"] = f"8 sensors x {B // 8} frames x {n} samples, 1 cm range noise, ROR(0.10 m, >= 2) + voxel 5 cm"
        # (round 6) E5 runs inside the voxel kernel's streaming pass (include/rplgpu.h RPLGPU_ROR_INSIDE: one pass
        # over the scans); work items it cannot settle go to the two kernels of rounds 1-5, timed here as well
        c5["e5"] = "inside the voxel kernel (RPLGPU_ROR_INSIDE)"
        c5["items_left_to_two_kernels"] = gpu.debug_ror_listed()
        gpu.set_ror_mode(1)
        try:
            two = regime(gpu, dev, stream, "c5", c5b, p5, big_arena, d_cursor, d_start, d_np, d_st, vreps)
        finally:
            gpu.set_ror_mode(0)
        c5["two_kernels"] = {"ms": two["ms"], "frac": two["frac"], "cells": two["cells"],
                             "note": "k_ror_mask + k_cloud_voxel with the mask (RPLGPU_ROR_TWO_KERNELS)"}
        # ... and as ONE grid per time step (E8): per-sensor motion de-skew + planar pose, the 8
        # sensors of a frame voxelised together (rplgpu_cloud_fused_voxel_dev, group = 8)
        rng = np.random.default_rng(args.seed)
        motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                           for _ in range(B)]).astype(np.float32)
        ang = rng.uniform(-3, 3, B)
        pose2d = np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, B), np.sin(ang), np.cos(ang),
                           rng.uniform(-2, 2, B)], 1).astype(np.float32)
        d_c5 = torch.from_numpy(c5b.view(np.uint8).reshape(B, n * 8)).to(dev)
        d_mo, d_po = torch.from_numpy(motion).to(dev), torch.from_numpy(pose2d).to(dev)
        cap5 = big_arena.shape[0]

        def fused():
            gpu.cloud_fused_voxel_dev(d_c5.data_ptr(), n, d_len.data_ptr(), B, 8, p5, d_mo.data_ptr(),
                                      d_po.data_ptr(), big_arena.data_ptr(), cap5, d_cursor.data_ptr(),
                                      d_start.data_ptr(), d_np.data_ptr(), d_st.data_ptr())

        gpu.set_ror_mode(1)
        try:
            ms_two = timed(fused, stream, vreps, sync)
        finally:
            gpu.set_ror_mode(0)
        ms = timed(fused, stream, vreps, sync)
        cells = int(d_cursor.item())
        c5["fused_grid"] = {"ms": round(ms, 4), "ms_two_kernels": round(ms_two, 4),
                            "gpts_s": round(B * n / ms / 1e6, 1),
                            "frac": round((8 * B * n + 16 * cells) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                            "cells": cells, "status_bits": int(d_st[: B // 8].max().item()),
                            "workload": "the same scans, de-skewed + posed, one voxel grid per time step "
                                        "(8 sensors), E5 mask on"}
        del c5b, big_arena, d_c5

    # (the side legs below are single-GPU properties: at N > 1 the ranks leave together)
    if args.full and not args.no_decode and rank == 0 and world == 1:
        extra["decode"] = decode_stage(gpu, dev, stream, args.cpu_seconds)

    cpu = None
    if args.full and rank == 0 and world == 1 and args.cpu_seconds > 0:
        cpu = cpu_baseline(batch_np, lens_np, params, args.cpu_seconds)

    if args.full and rank == 0 and world == 1 and not args.no_single:
        extra["single_scan_us"] = single_scan_table(gpu, params, args.seed, args.cpu_seconds)

    if rank == 0:
        traffic, traffic_src = (None, "not measured" if args.full else "taken with --full only")
        if args.full and world == 1 and not args.no_live_traffic and not args.dry_run:
            traffic, traffic_src = live_traffic(args, B, n)
        if traffic is None:
            why = traffic_src
            traffic, traffic_src = static_traffic("k_cloud_voxel", B, n)
            if traffic_src:
                traffic_src += f" (live measurement: {why})"
            else:
                traffic_src = f"none (live measurement: {why})"
        ms_per_step = elapsed / args.steps * 1e3
        rnd = lambda x, d: None if x is None else round(x, d)  # (figures a plain N > 1 run does not take)
        value = B_total * n / (elapsed / args.steps) / 1e6
        line = {
            "metric": "Mpoints/s raw-scan->filtered PointCloud2",
            "value": round(value, 1),
            "unit": "Mpoints/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u32/f32",
            "data": "synthetic",
            "config": {
                "workload": f"config3: {B_total} scans x {n} samples (ring, 10% invalid runs), "
                            f"clip [0.15,40] m, q_min 0 (BASELINE config 3's filter at its SURVEY 8(a-ext) "
                            f"default; the q_min 48 leg is in `variants`) + polar->XYZ + 5 cm voxel grid "
                            f"into one contiguous cloud"
                            + ("" if world == 1 else f", sharded by scan over {world} GPUs + "
                               "RCCL all-gather of voxelised clouds (chunked, overlapped)"),
                "scans": B_total, "samples_per_scan": n, "voxel_leaf_m": 0.05,
                "input_bytes": 8 * B_total * n,
            },
            "roofline": {
                "kernel": "k_cloud_voxel",
                "bound": "hbm",
                "achieved": rnd(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": rnd(achieved and achieved / HBM_PEAK_GBS, 4),
                "frac_read": rnd(k_ms_b2b and 8 * B * n / (k_ms_b2b * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "frac_of_copy_rate": rnd(achieved and achieved / HBM_COPY_GBS, 4),
                "traffic": traffic,
                "traffic_source": traffic_src,
                "kernel_ms_avg": rnd(k_ms_b2b, 4),
                "kernel_ms_min": rnd(k_ms_min, 4),
                "kernel_ms_note": "avg = HIP events on the launch stream around the K timed steps "
                                  "themselves (N = 1: a step is the launch + two 8-byte memsets; N > 1: "
                                  "the launch alone, back to back); min = best single launch bracketed "
                                  "by its own events (launches of their own, as N > 1's avg: --full only)",
                "algorithmic_bytes": algo_bytes,
                "note": "priced against HBM as SURVEY 8(d) asks; the kernel is not HBM bound (traffic = 1.02 x the "
                        "algorithmic bytes).  Per scan and CU 62.6 k cycles: the streaming phase 41.6 k — a wave needs "
                        "~2150 cycles per 128-sample block (1070 waiting for the raw pair it asked for two blocks "
                        "earlier, 260 table entries + arithmetic, 580 aggregation, 250 loop) whether two or four waves "
                        "share its SIMD: latency of the raw load -> table gather chain per wave, through a vector-memory "
                        "path that the raw loads and the two gathers per block keep busy — and the reduce phase 21 k, a "
                        "chain of barrier-separated LDS round trips (rank + permute 7.3 k, emit 6.1 k), the two in series "
                        "on one 1024-thread workgroup per CU (profiles/r06/voxel_keys_in_lds_r06.txt section 3, "
                        "tools/voxdbg.py; vector ALU busy 56 % of the launch, profiles/r05/rocprof_summary_r05.txt).  "
                        "Round 6 built the form that overlaps the two phases of different scans (two 512-thread "
                        "workgroups per CU, 32-bit keys in LDS, records in L2): bit-exact, at parity, not shipped",
            },
            "cpu_baseline": cpu,
            "variants": variants,
            "c5": c5,
            "compute_only": compute_only,
            "compute_only_ms": None if compute_only is None else compute_only["ms_per_step"],
            "exchange_only_ms": None if compute_only is None else compute_only["exchange_only_ms"],
            "gathered_bytes_per_rank": None if compute_only is None else compute_only["gathered_bytes_per_rank"],
            "exchange_backend": None if compute_only is None else compute_only["exchange_backend"],
            "exchange_ranks": None if compute_only is None else compute_only.get("comm_ranks"),
            "exchange_bytes_per_point": None if compute_only is None else 12,
            "status_bits": status,
            "cells_out_rank0": cells_local,
            "host_gen_s": round(gen_s, 2),
            "h2d_ms_pinned": None if h2d_ms is None else round(h2d_ms, 3),
            "value_incl_pcie_h2d": None if h2d_ms is None else round(
                B_total * n / ((ms_per_step + h2d_ms) * 1e-3) / 1e6, 1),
        }
        line.update(extra)
        result_line = json.dumps(line)
    else:
        result_line = None

    if exch is not None:
        exch.close()
    gpu.close()
    if use_dist:
        dist.destroy_process_group()
    sys.stdout.flush()
    try:  # the C libraries' own stdio buffers (RCCL's banner sits there until exit)
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    os.dup2(real_stdout, 1)
    if result_line is not None:
        os.write(1, (result_line + "\n").encode())


if __name__ == "__main__":
    main()
