"""CPU tier: ShardedEnsemble.constrain_loglik -- the half of ``constrain`` that takes a per-member log-likelihood (e.g.
``ensemble.loglik_vectors`` over variability statistics), so a sharded run can weight by one -- on stand-in ensembles: alone in
one process, and over a real 2-rank gloo group (tests/_dist_variability_worker.py).  ``constrain`` itself gives what it gave:
the global ll_max, the default bits and the weights numpy forms from them."""
import json
import os
import subprocess
import sys

import numpy as np

from tests._dist_quantile_worker import global_rows
from tests._dist_wquantile_worker import StandInEnsemble, global_loglik, quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want(n_total):
    ll, status = global_loglik(n_total)
    ll_max = float(ll[np.isfinite(ll) & (status == 0)].max())
    bits = 53 - int(np.ceil(np.log2(n_total)))
    return ll, status, ll_max, bits


def test_one_process_constrain_and_constrain_loglik():
    from rscm_amd.distributed import ShardedEnsemble
    n_total = 1001
    ll, status, ll_max, bits = _want(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: StandInEnsemble(c, 0, global_rows(n_total), ll, status), rank=0, world=1)
    assert se.constrain(1, [0], [0.0], [1.0]) == (ll_max, bits)
    w = se.ensemble.w.copy()
    assert np.array_equal(w, quantise(ll, status, ll_max, bits)) and w.max() == 2 ** bits
    se.ensemble.w = None
    assert se.constrain_loglik(ll) == (ll_max, bits) and np.array_equal(se.ensemble.w, w)
    assert se.constrain_loglik(ll, bits=20) == (ll_max, 20) and np.array_equal(se.ensemble.w, quantise(ll, status, ll_max, 20))
    shifted = ll - 3.0                                       # another vector: its own maximum
    assert se.constrain_loglik(shifted) == (ll_max - 3.0, bits)


def test_two_rank_gloo_constrain_loglik(tmp_path):
    n_total = 1001
    port = "29871"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_variability_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    ll, status, ll_max, bits = _want(n_total)
    w = quantise(ll, status, ll_max, bits)
    assert sum(x["count"] for x in res) == n_total
    for x in res:
        assert x["world"] == 2
        assert x["constrain"] == [ll_max, bits] and x["constrain_loglik"] == [ll_max, bits] and x["constrain_loglik_bits20"] == [ll_max, 20]
        sl = slice(x["offset"], x["offset"] + x["count"])
        assert x["w_constrain"] == w[sl].tolist() and x["w_constrain_loglik"] == w[sl].tolist()
