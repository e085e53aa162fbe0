"""Worker for tests/test_distributed_weighted_quantiles_cpu.py: one rank of a gloo group running ShardedEnsemble.constrain and the
weighted rscm_amd.distributed.quantile_rows_global.  The compute needs a GPU, so the rank's ensemble is a stand-in: rows,
log-likelihoods and status are known functions of the GLOBAL member id, the weights are quantised in numpy as the device does,
and the staged select is the numpy restatement of the weighted select of csrc/select.hip (tests/host_wselect.py).  What is
under test is the product's loops: the MAX all-reduce of the local maxima, then pass, all-reduce (int64 SUM over gloo), commit,
result."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests._dist_quantile_worker import global_rows  # noqa: E402
from tests.host_wselect import HostWSelect  # noqa: E402


def global_loglik(n_total):
    """[n_total] log-likelihoods with -inf members, and the status bytes (every 7th member failed)."""
    g = np.arange(n_total)
    ll = -0.5 * ((g % 13) - 6.0) ** 2 - 0.01 * g
    ll[g % 11 == 5] = -np.inf
    return ll, np.where(g % 7 == 3, 1, 0).astype(np.uint8)


def quantise(ll, status, ll_max, bits):
    ok = np.isfinite(ll) & (status == 0)
    d = np.minimum(np.where(ok, ll - ll_max, 0.0), 0.0)
    return np.where(ok, np.floor(np.ldexp(np.exp(d), bits) + 0.5), 0).astype(np.int64)


class _Select:
    def __init__(self, rows, w, q):
        self.s = HostWSelect(rows, w, q)

    def next_pass(self):
        return self.s.next_pass()

    def commit(self, reduced=None):
        self.s.commit(reduced)

    def result(self):
        return self.s.result()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class StandInEnsemble:
    def __init__(self, count, offset, rows, ll, status):
        self.rows = rows[:, offset:offset + count]
        self.ll, self.status = ll[offset:offset + count], status[offset:offset + count]
        self.w = None

    def loglik(self, *a, **k):
        return self.ll

    def loglik_max(self, ll):
        x = ll[np.isfinite(ll) & (self.status == 0)]
        return float(x.max()) if x.size else -np.inf

    def set_weights_from_loglik(self, ll, bits, ll_max):
        self.w = quantise(ll, self.status, ll_max, bits)
        return ll_max, bits

    def select(self, var, q, t_begin=0, t_end=None, t_stride=1, weighted=False):
        assert weighted
        return _Select(self.rows[t_begin:t_end:t_stride], self.w, q)


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    q = [0.0, 0.05, 0.5, 0.95, 1.0, 1e-12]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    rows = global_rows(n_total)
    ll, status = global_loglik(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, rows, ll, status)
    ll_max, bits = se.constrain(1, [0], [0.0], [1.0])
    res = se.quantile_rows_global(1, q, 0, None, 1, weighted=True)
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump({"rank": rank, "world": dist.get_world_size(), "ll_max": ll_max, "bits": bits, "weight": res["weight"].tolist(),
                   "bits_q": res["quantiles"].view(np.uint64).astype(str).tolist()}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
