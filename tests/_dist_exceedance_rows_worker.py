"""Worker for tests/test_exceedance_rows_cpu.py: one rank of a gloo group running ShardedEnsemble.exceedance_rows_global and
rank_rows_global on a stand-in ensemble whose ``exceedance_rows`` and ``rank_rows`` are the restatement
(tests/host_exceedance_rows.py) over the rank's shard of a global data set that is a known function of the seed.  What is under
test is the product's half: the one all-reduce of the concatenated int64 arrays and the finishers on every rank."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests import host_exceedance_rows as he  # noqa: E402

N_GROUPS = 3
N_ROWS = 6
THRESHOLDS = [0.0, 0.3, np.inf]


def global_data(n_total: int):
    """(rows[N_ROWS][n_total], record[N_ROWS], weights, groups, baseline): a warming plume rounded to one decimal, so full of ties, a
    member that turns NaN from row 2 on, infinite values, a NaN in the baseline, a weight of 2^40 among 20-bit ones, three groups
    and members of none; the record has a gap, a value below every member and one above."""
    rng = np.random.default_rng(n_total)
    rows = np.round(np.stack([0.1 * t + 0.3 * rng.standard_normal(n_total) for t in range(N_ROWS)]), 1)
    rows[2:, 5] = np.nan
    rows[3, n_total - 2] = np.inf
    rows[4, 3] = -np.inf
    baseline = np.round(rows[:2].mean(axis=0), 1)
    baseline[7] = np.nan
    w = rng.integers(0, 1 << 20, n_total)
    w[n_total // 3] = 1 << 40
    record = np.array([0.1, np.nan, 0.2, -50.0, 50.0, 0.4])
    return rows, record, w, rng.integers(-1, N_GROUPS, n_total).astype(np.int32), baseline


class StandInEnsemble:
    """The members [offset, offset + count) of the global data; ``var`` is ignored."""

    def __init__(self, count, offset, rows, record, w, groups, baseline):
        sl = slice(offset, offset + count)
        self.rows, self.w, self.groups, self.baseline = rows[:, sl], w[sl], groups[sl], baseline[sl]
        self.calls = []

    def _kw(self, weighted, anomaly, grouped):
        return dict(weights=self.w if weighted else None, groups=self.groups if grouped else None, n_groups=N_GROUPS if grouped else None,
                    baseline=self.baseline if anomaly else None)

    def exceedance_rows(self, var, thresholds, t_begin=0, t_end=None, t_stride=1, weighted=False, anomaly=False, grouped=False):
        self.calls.append(("exceedance", weighted, anomaly, grouped))
        return he.exceedance_rows(self.rows[t_begin:t_end:t_stride], thresholds, **self._kw(weighted, anomaly, grouped))

    def rank_rows(self, var, record, t_begin=0, t_end=None, t_stride=1, weighted=False, anomaly=False, grouped=False):
        self.calls.append(("rank", weighted, anomaly, grouped))
        return he.rank_rows(self.rows[t_begin:t_end:t_stride], record, **self._kw(weighted, anomaly, grouped))


def bits(d):
    """A result dict as lists json can carry: integers as they are, doubles as their bits."""
    return {k: (np.asarray(v, dtype=np.float64).view(np.uint64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)).tolist() for k, v in d.items()}


def results(se, record):
    return {"exc_plain": bits(se.exceedance_rows_global("T", THRESHOLDS)),
            "exc_full": bits(se.exceedance_rows_global("T", THRESHOLDS, 1, N_ROWS, 2, weighted=True, anomaly=True, grouped=True)),
            "rank_plain": bits(se.rank_rows_global("T", record)),
            "rank_full": bits(se.rank_rows_global("T", record[1:N_ROWS:2], 1, N_ROWS, 2, weighted=True, anomaly=True, grouped=True))}


CALLS = [["exceedance", False, False, False], ["exceedance", True, True, True], ["rank", False, False, False], ["rank", True, True, True]]


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    data = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, *data)
    out = {"rank": rank, "world": dist.get_world_size(), "offset": se.offset, "count": se.count}
    out.update(results(se, data[1]))
    out["calls"] = [list(c) for c in se.ensemble.calls]
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
