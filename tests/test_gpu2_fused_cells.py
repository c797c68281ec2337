"""One fused voxel grid across real RCCL ranks (include/rplgpu_comm.h, the cell exchange): four sensors per rank,
records gathered to rank 0 and merged there; the serialised PointCloud2 must equal the single-process
rplgpu_cloud_fused_voxel_dev + rplgpu_fused_cloud_msg_dev.  A 1-GPU box runs the worker with one rank; the
two-rank form is marked gpu2 and skipped below two devices."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def _run_worker(world, port):
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(ROOT / "tests" / "rccl_cells_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"RCCL_CELLS_OK {world}" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_cells_worker_one_rank():
    _run_worker(1, 29561)


@pytest.mark.gpu2
def test_fused_grid_two_ranks_equals_single_process():
    _run_worker(2, 29562)
