"""Reference-period targets over two ranks with REAL ensembles: the ranks share the one GPU of the box, collectives over gloo, the
ranks are CHILD processes under a time limit (as in tests/test_multirank_gpu.py: pytest + two ranks = three processes on the card).

What is asserted is computed inside the workers (scripts/rehearse_reference_period.py): the sharded device sampler with a
reference-period target is the single-rank chain bit for bit, and ShardedEnsemble.constrain(..., reference=...) followed by
quantile_rows_global(weighted=True, anomaly=True) is the single process's constrained anomaly plume bit for bit."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpus() -> int:
    import torch
    return torch.cuda.device_count()   # does not initialise the GPU


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("reference_period_ranks")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29583", HSA_ENABLE_IPC_MODE_LEGACY="0", RSCM_BENCH_BACKEND="gloo",
               RSCM_BENCH_DEVICE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29583", os.path.join(ROOT, "scripts", "rehearse_reference_period.py"), "--out", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [json.load(open(os.path.join(out, f"rank{k}.json"))) for k in range(2)]


@pytest.mark.gpu
@pytest.mark.gpu_ranks
@pytest.mark.skipif(_gpus() < 1, reason="needs a GPU")
def test_sharded_sampler_with_a_reference_period_reproduces_the_single_rank_chain(results):
    for res in results:
        assert res["world"] == 2, res
        c = {k: v for k, v in res["checks"].items() if k.startswith("sampler_")}
        assert len(c) == 9 and all(c.values()), c


@pytest.mark.gpu
@pytest.mark.gpu_ranks
@pytest.mark.skipif(_gpus() < 1, reason="needs a GPU")
def test_sharded_constrain_with_a_reference_period_equals_the_single_process(results):
    for res in results:
        assert res["world"] == 2, res
        c = {k: v for k, v in res["checks"].items() if not k.startswith("sampler_")}
        assert len(c) == 6 and all(c.values()), c
