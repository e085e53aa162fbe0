"""Sharded anomaly plumes, indicator quantiles and exceedance with REAL ensembles: several ranks share the one GPU of the box and
reduce int64 histograms and counts over gloo.  The ranks are CHILD processes, as in tests/test_multirank_quantiles_gpu.py: 2 ranks
in the driver's tier (pytest + two ranks = three processes on the card), 4 ranks only under `gpu_ranks`, run as their own pytest
process:

    python -m pytest tests/test_multirank_indicators_gpu.py -m gpu_ranks -q

What is asserted is computed inside the workers (scripts/rehearse_indicators.py): sharded == single process, bit for bit."""
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
           "--master-port", str(port), os.path.join(ROOT, "scripts", "rehearse_indicators.py"), "--out", str(out), *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [json.load(open(os.path.join(out, f"rank{k}.json"))) for k in range(ranks)]


@pytest.mark.skipif(_gpus() < 1, reason="needs a GPU")
@pytest.mark.parametrize("ranks", [pytest.param(2, marks=[pytest.mark.gpu, pytest.mark.gpu_ranks]), pytest.param(4, marks=pytest.mark.gpu_ranks)])
def test_sharded_indicators_equal_the_single_process(tmp_path, ranks):
    """Every rank's anomaly plume (plain and weighted), indicators, indicator quantiles and exceedance equal the single process
    bit for bit, on full storage and on a windowed handle's output store."""
    for res in _launch(ranks, 29591 + ranks, tmp_path, ["--members", "30001"]):
        assert res["world"] == ranks and res["ok"], res
        for tag in ("full", "windowed"):
            for k in ("anomaly_bit_equal", "weighted_anomaly_bit_equal", "vectors_bit_equal", "weighted_exceedance_equal"):
                assert f"{tag}_{k}" in res["checks"], res["checks"]
        assert all(res["checks"].values()), res["checks"]
