"""CPU tier: the anomaly select, quantiles of per-member vectors and exceedance over a real 2-rank gloo group
(rscm_amd.distributed.quantile_rows_global(anomaly=True), quantile_vectors_global, exceedance_global; stand-in ensembles,
tests/_dist_indicator_worker.py): every rank ends with the numbers of the whole member set -- bit for bit the one-shard select of
the same values, and numpy's quantiles."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests._dist_indicator_worker import Q, REF, THR, global_series, global_weights
from tests.helpers import same_values
from tests.host_indicators import anomaly, baseline, exceedance_counts, indicators
from tests.host_select import sharded_quantiles
from tests.host_wselect import sharded_wquantiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _unsign(x):
    return np.where(x == 0, 0.0, x)


@pytest.mark.parametrize("n_total", [9, 1001])
def test_two_rank_gloo_indicators(n_total, tmp_path):
    port = str(29800 + n_total % 89)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_indicator_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    x, w = global_series(n_total), global_weights(n_total)
    b = baseline(x[REF[0]:REF[1]])
    a = anomaly(x, b)
    ind = indicators(x[2:8], 2002.0 + np.arange(6), THR, b)
    vecs = np.stack([ind["mean"], ind["peak"], ind["peak_time"]] + ind["crossing"])
    for tag, wt in (("u", None), ("w", w)):
        if wt is None:
            wa, wv = sharded_quantiles([a], Q)[0], sharded_quantiles([vecs], Q)[0]
        else:
            wa, wv = sharded_wquantiles([a], [w], Q)[0], sharded_wquantiles([vecs], [w], Q)[0]
        hits, total = exceedance_counts(ind["peak"], THR, wt)
        for x_ in res:
            got = x_[tag]
            assert np.array_equal(_f(got["anomaly"]).view(np.uint64), wa["quantiles"].view(np.uint64))
            assert np.array_equal(_f(got["vectors"]).view(np.uint64), wv["quantiles"].view(np.uint64))
            assert got["hits"] == hits and got["total"] == total
            assert np.array_equal(_f(got["prob"]), np.array(hits) / total)
        if wt is None:                                          # and the select's numbers are numpy's
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = np.nanquantile(a, Q, axis=1).T
            assert same_values(_unsign(_f(res[0][tag]["anomaly"])), _unsign(want))
            assert res[0][tag]["n"] == (~np.isnan(a)).sum(axis=1).tolist()
            assert res[0][tag]["vn"] == (~np.isnan(vecs)).sum(axis=1).tolist()
