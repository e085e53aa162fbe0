"""Grouped quantiles and exceedance of a sharded ensemble with REAL ensembles: two ranks share the one GPU of the box, the int64
all-reduces of rscm_amd.distributed run over gloo.  The ranks are CHILD processes, as in tests/test_multirank_quantiles_gpu.py.
What is asserted is computed inside the workers (tests/_multirank_grouped_worker.py): sharded == one handle, bit for bit."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpus() -> int:
    import torch
    return torch.cuda.device_count()   # does not initialise the GPU


@pytest.mark.skipif(_gpus() < 1, reason="needs a GPU")
@pytest.mark.gpu
@pytest.mark.gpu_ranks
def test_sharded_grouped_statistics_equal_the_single_handle(tmp_path):
    port, ranks = 29583, 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_multirank_grouped_worker.py"), "4099", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(ranks):
        res = json.load(open(os.path.join(tmp_path, f"rank{k}.json")))
        assert res["world"] == ranks and res["ok"], res
