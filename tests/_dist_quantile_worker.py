"""Worker for tests/test_distributed_quantiles_cpu.py: one rank of a gloo group running
rscm_amd.distributed.quantile_rows_global.  The compute needs a GPU, so the rank's ensemble is a stand-in whose rows are known
functions of the GLOBAL member id and whose staged select is the numpy restatement of csrc/select.hip (tests/host_select.py);
what is under test is the product's loop: pass, all-reduce (int64 SUM over gloo), commit, result."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests.host_select import HostSelect  # noqa: E402


def global_rows(n_total):
    """[rows][n_total]: the global member set, with ties, +-inf, +-0, NaNs of both signs and an all-NaN row."""
    rng = np.random.default_rng(5)
    g = np.arange(n_total)
    rows = np.stack([1.2 + 1e-3 * rng.standard_normal(n_total),
                     rng.choice([-1.0, -0.0, 0.0, 2.5, np.inf, -np.inf], n_total),
                     np.where(g % 3 == 0, np.nan, np.where(g % 3 == 1, -np.float64(np.nan), g * 0.5)),
                     np.full(n_total, np.nan),
                     np.where(g == n_total - 1, 4.0, np.nan)])
    return rows


class _Select:
    def __init__(self, rows, q):
        self.s = HostSelect(rows, q)

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
    def __init__(self, count, device, offset, rows):
        self.rows = rows[:, offset:offset + count]

    def select(self, var, q, t_begin=0, t_end=None, t_stride=1):
        return _Select(self.rows[t_begin:t_end:t_stride], q)


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    q = [0.0, 0.05, 0.5, 0.95, 1.0, 1e-12]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    rows = global_rows(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, 0, se.offset, rows)
    res = se.quantile_rows_global(1, q, 0, None, 1)
    part = se.quantile_rows_global(1, q, 1, 5, 2)
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump({"rank": rank, "world": dist.get_world_size(), "count": res["count"].tolist(),
                   "bits": res["quantiles"].view(np.uint64).astype(str).tolist(),
                   "strided_bits": part["quantiles"].view(np.uint64).astype(str).tolist()}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
