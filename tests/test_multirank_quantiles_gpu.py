"""Sharded ensemble quantiles with REAL ensembles: several ranks share the one GPU of the box, the int64 histogram all-reduces of
rscm_amd.distributed.quantile_rows_global run over gloo.  The ranks are CHILD processes (subprocess), as in
tests/test_multirank_gpu.py; 2 ranks are in the driver's tier (pytest + two ranks = three processes on the card), 4 ranks only
under `gpu_ranks`, run as their own pytest process:

    python -m pytest tests/test_multirank_quantiles_gpu.py -m gpu_ranks -q

What is asserted is computed inside the workers (scripts/rehearse_quantiles.py): sharded == single process, bit for bit."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpus() -> int:
    import torch
    return torch.cuda.device_count()   # does not initialise the GPU


def _launch(ranks, port, out, extra=()):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
               RSCM_BENCH_BACKEND="gloo", RSCM_BENCH_DEVICE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "scripts", "rehearse_quantiles.py"), "--out", str(out), *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [json.load(open(os.path.join(out, f"rank{k}.json"))) for k in range(ranks)]


@pytest.mark.skipif(_gpus() < 1, reason="needs a GPU")
@pytest.mark.parametrize("ranks", [pytest.param(2, marks=[pytest.mark.gpu, pytest.mark.gpu_ranks]), pytest.param(4, marks=pytest.mark.gpu_ranks)])
def test_sharded_quantiles_equal_the_single_process(tmp_path, ranks):
    """ShardedEnsemble.quantile_rows_global: the ranks sum int64 radix-select histograms (gloo) and every rank ends with the
    quantiles of the whole ensemble -- bit for bit the single-process quantile_rows of the same global LHS ensemble, on full
    storage and on a windowed handle's output store."""
    for res in _launch(ranks, 29561 + ranks, tmp_path, ["--members", "30001"]):
        assert res["world"] == ranks and res["ok"], res
        assert all(res["checks"].values()), res["checks"]
