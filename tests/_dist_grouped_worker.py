"""Worker for tests/test_distributed_grouped_cpu.py: one rank of a gloo group running the grouped
rscm_amd.distributed.quantile_rows_global and exceedance_global.  The compute needs a GPU, so the rank's ensemble is a stand-in
whose rows and groups are known functions of the GLOBAL member id and whose staged select is the numpy restatement of the grouped
select (tests/host_gselect.py); what is under test is the product's loop over buffers of the grouped size -- pass, all-reduce
(int64 SUM over gloo), commit, result -- and the [G][k] + [G] reduction of the exceedance sums."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests.host_gselect import HostGSelect, exceedance_grouped  # noqa: E402

G = 5
Q = [0.0, 0.05, 0.5, 0.95, 1.0, 1e-12]
THR = [0.0, 1.2, 2.5]


def global_rows(n_total):
    """[rows][n_total] without negative zeros: clustered, ties and +-inf, NaNs of both signs, an all-NaN row, one member."""
    rng = np.random.default_rng(5)
    g = np.arange(n_total)
    return np.stack([1.2 + 1e-3 * rng.standard_normal(n_total),
                     rng.choice([-1.0, 0.0, 2.5, np.inf, -np.inf], n_total),
                     np.where(g % 3 == 0, np.nan, np.where(g % 3 == 1, -np.float64(np.nan), g * 0.5)),
                     np.full(n_total, np.nan),
                     np.where(g == n_total - 1, 4.0, np.nan)])


def global_groups(n_total):
    """Contiguous blocks of groups 0..3 (so the first rank holds no member of the last ones; group 4 is empty), some members in none."""
    g = (np.arange(n_total) * 4) // n_total
    g[np.arange(n_total) % 7 == 3] = -1
    return g


class _Select:
    def __init__(self, rows, group, q):
        self.s = HostGSelect(rows, group, G, q)

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
    def __init__(self, count, offset, rows, group):
        self.rows, self.group = rows[:, offset:offset + count], group[offset:offset + count]

    def select(self, var, q, t_begin=0, t_end=None, t_stride=1, grouped=False):
        assert grouped
        return _Select(self.rows[t_begin:t_end:t_stride], self.group, q)

    def exceedance(self, vector, thresholds, weighted=False, grouped=False):
        assert grouped and not weighted
        hits, total = exceedance_grouped(self.rows[vector], self.group, G, thresholds)
        return {"hits": hits, "total": total}


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, global_rows(n_total), global_groups(n_total))
    res = se.quantile_rows_global(1, Q, 0, None, 1, grouped=True)
    part = se.quantile_rows_global(1, Q, 1, 5, 2, grouped=True)
    exc = se.exceedance_global(1, THR, grouped=True)
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump({"rank": rank, "world": dist.get_world_size(), "count": res["count"].tolist(),
                   "bits": res["quantiles"].view(np.uint64).astype(str).tolist(),
                   "strided_bits": part["quantiles"].view(np.uint64).astype(str).tolist(),
                   "hits": exc["hits"].tolist(), "total": exc["total"].tolist(),
                   "probability": np.nan_to_num(exc["probability"], nan=-1.0).tolist()}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
