"""CPU tier: rscm_amd.distributed.quantile_rows_global over a real 2-rank gloo group (stand-in ensembles, tests/_dist_quantile_worker.py):
the quantiles of the whole member set on every rank, equal to numpy.nanquantile of the concatenation and, bit for bit, to the
one-shard select."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._dist_quantile_worker import global_rows
from tests.helpers import same_values
from tests.host_select import sharded_quantiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = [0.0, 0.05, 0.5, 0.95, 1.0, 1e-12]


@pytest.mark.parametrize("n_total", [9, 1001])
def test_two_rank_gloo_quantiles(n_total, tmp_path):
    port = str(29600 + n_total % 89)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_quantile_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    rows = global_rows(n_total)
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        want = np.nanquantile(rows, Q, axis=1).T
    whole = sharded_quantiles([rows], Q)[0]["quantiles"]
    strided = sharded_quantiles([rows[1:5:2]], Q)[0]["quantiles"]
    for x in res:
        assert x["world"] == 2
        got = np.array(x["bits"], dtype=np.uint64).view(np.float64)
        assert same_values(got, want)
        assert np.array_equal(got.view(np.uint64), whole.view(np.uint64))
        assert np.array_equal(np.array(x["strided_bits"], dtype=np.uint64), strided.view(np.uint64))
        assert x["count"] == (~np.isnan(rows)).sum(axis=1).tolist()
