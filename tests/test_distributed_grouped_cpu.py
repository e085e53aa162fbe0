"""CPU tier: the grouped rscm_amd.distributed.quantile_rows_global and exceedance_global over a real 2-rank gloo group (stand-in
ensembles, tests/_dist_grouped_worker.py): per group the quantiles of the whole member set on every rank, equal to
numpy.nanquantile of the group's members and, bit for bit, to the one-shard grouped select; the exceedance sums equal the
whole set's."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests._dist_grouped_worker import G, Q, THR, global_groups, global_rows
from tests.helpers import same_values
from tests.host_gselect import exceedance_grouped, sharded_gquantiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nanq(x):
    if x.shape[1] == 0:
        return np.full((x.shape[0], len(Q)), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(x, Q, axis=1).T


@pytest.mark.parametrize("n_total", [9, 1001])
def test_two_rank_gloo_grouped_quantiles_and_exceedance(n_total, tmp_path):
    port = str(29700 + n_total % 89)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_grouped_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    rows, group = global_rows(n_total), global_groups(n_total)
    want = np.stack([_nanq(rows[:, group == g]) for g in range(G)])
    count = np.stack([(~np.isnan(rows[:, group == g])).sum(axis=1) for g in range(G)])
    whole = sharded_gquantiles([rows], [group], G, Q)[0]["quantiles"]
    strided = sharded_gquantiles([rows[1:5:2]], [group], G, Q)[0]["quantiles"]
    hits, total = exceedance_grouped(rows[1], group, G, THR)
    for x in res:
        assert x["world"] == 2
        got = np.array(x["bits"], dtype=np.uint64).view(np.float64)
        assert got.shape == (G, rows.shape[0], len(Q))
        assert same_values(got, want)
        assert np.array_equal(got.view(np.uint64), whole.view(np.uint64))
        assert np.array_equal(np.array(x["strided_bits"], dtype=np.uint64), strided.view(np.uint64))
        assert x["count"] == count.tolist()
        assert x["hits"] == hits.tolist() and x["total"] == total.tolist()
        prob = np.array(x["probability"])
        assert np.array_equal(prob[total > 0], (hits / np.maximum(total, 1)[:, None])[total > 0]) and (prob[total == 0] == -1.0).all()
    assert (count[G - 1] == 0).all() and total[G - 1] == 0          # the group no rank holds a member of
