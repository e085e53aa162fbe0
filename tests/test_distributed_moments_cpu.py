"""CPU tier: rscm_amd.distributed.moments_global / ShardedEnsemble.moments_global on stand-in ensembles whose ``moment_sums`` is
the reference's limb scheme (tests/_dist_moments_worker.py): alone in one process, and over a real 2-rank gloo group on
127.0.0.1.  Either way every rank gets the bits of the reference over ALL members: the int64 arrays of shards add up element by
element, and the finishing step (rscm_gpu_moment_finish of the built library, which needs no device) rounds the exact quotient once."""
import json
import os
import subprocess
import sys

import numpy as np

from tests import host_moments as hm
from tests._dist_moments_worker import N_GROUPS, StandInEnsemble, bits, global_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want(n_total):
    X, w, groups = global_data(n_total)
    plain = {k: v[0] for k, v in hm.moments(X).items()}
    return bits(plain), bits(hm.moments(X[[2, 0]], w, groups, N_GROUPS))


def test_one_process_moments_global():
    from rscm_amd.distributed import ShardedEnsemble
    n_total = 1001
    X, w, groups = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: StandInEnsemble(c, 0, X, w, groups), rank=0, world=1)
    plain, wg = _want(n_total)
    got = se.moments_global([0, 1, 2])
    assert got["mean"].shape == (3,) and got["cov"].shape == (3, 3) and got["count"] == n_total - 3
    assert bits(got) == plain
    got = se.moments_global([2, 0], weighted=True, grouped=True)
    assert got["mean"].shape == (N_GROUPS, 2) and got["corr"].shape == (N_GROUPS, 2, 2)
    assert bits(got) == wg
    assert se.ensemble.calls == [(1, False, False), (2, False, False), (1, True, True), (2, True, True)]


def test_two_rank_gloo_moments_global(tmp_path):
    n_total = 1001
    port = "29877"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.join(ROOT, "tests", "_dist_moments_worker.py"), str(n_total), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    plain, wg = _want(n_total)
    assert sum(x["count"] for x in res) == n_total and all(0 < x["count"] < n_total for x in res)
    for x in res:
        assert x["world"] == 2
        assert x["plain"] == plain and x["weighted_grouped"] == wg
        assert x["calls"] == [[1, False, False], [2, False, False], [1, True, True], [2, True, True]]
    assert np.isfinite(np.array(plain["mean"], dtype=np.uint64).view(np.float64)).all()
