"""CPU tier: ShardedEnsemble.constrain and the weighted rscm_amd.distributed.quantile_rows_global over a real 2-rank gloo group
(stand-in ensembles, tests/_dist_wquantile_worker.py): every rank ends with one global ll_max and bits, and with the weighted
quantiles of the whole member set -- bit for bit the one-shard select and numpy's weighted inverted_cdf."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests._dist_quantile_worker import global_rows
from tests._dist_wquantile_worker import global_loglik, quantise
from tests.host_wselect import sharded_wquantiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = [0.0, 0.05, 0.5, 0.95, 1.0, 1e-12]


@pytest.mark.parametrize("n_total", [9, 1001])
def test_two_rank_gloo_weighted_quantiles(n_total, tmp_path):
    port = str(29700 + n_total % 89)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_wquantile_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    rows = global_rows(n_total)
    ll, status = global_loglik(n_total)
    ok = np.isfinite(ll) & (status == 0)
    ll_max = float(ll[ok].max())
    bits = 53 - int(np.ceil(np.log2(n_total)))
    w = quantise(ll, status, ll_max, bits)
    whole = sharded_wquantiles([rows], [w], Q)[0]
    for x in res:
        assert x["world"] == 2 and x["ll_max"] == ll_max and x["bits"] == bits
        got = np.array(x["bits_q"], dtype=np.uint64).view(np.float64)
        assert np.array_equal(got.view(np.uint64), whole["quantiles"].view(np.uint64))
        assert x["weight"] == whole["weight"].tolist()
        for r_, row in enumerate(rows):
            if whole["weight"][r_] == 0:
                assert np.isnan(got[r_]).all()
                continue
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = [np.nanquantile(row, qq, weights=w, method="inverted_cdf") for qq in Q]
            assert np.array_equal(np.where(got[r_] == 0, 0.0, got[r_]), np.where(np.asarray(want) == 0, 0.0, want))
