"""Worker for tests/test_moment_rows_cpu.py: one rank of a gloo group running ShardedEnsemble.moment_rows_global on a stand-in
ensemble whose ``moment_rows_sums`` is the reference's limb scheme (tests/host_moment_rows.sums_array) over the rank's shard of a
global data set that is a known function of the seed.  What is under test is the product's half: the two all-reduces of the int64
arrays and the finishing step on every rank."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests import host_moment_rows as hr  # noqa: E402

N_GROUPS = 3
N_ROWS = 6


def global_data(n_total: int):
    """(rows[N_ROWS][n_total], V[2][n_total], weights, groups, baseline): a warming plume whose spread grows with the row, a member
    that turns NaN from row 2 on, an infinite value, a NaN in a vector and in the baseline, 30-bit weights, three groups and
    members of none."""
    rng = np.random.default_rng(n_total)
    V = np.stack([rng.uniform(0.5, 1.5, n_total), rng.normal(0.0, 3.0, n_total)])
    rows = np.stack([0.1 * t * V[0] + 0.02 * t * rng.normal(0.0, 1.0, n_total) for t in range(N_ROWS)])
    rows[2:, 5] = np.nan
    rows[3, n_total - 2] = np.inf
    V[1, n_total // 2] = np.nan
    baseline = rows[:2].mean(axis=0)
    baseline[7] = np.nan
    return rows, V, rng.integers(0, 1 << 30, n_total), rng.integers(-1, N_GROUPS, n_total).astype(np.int32), baseline


class StandInEnsemble:
    """The members [offset, offset + count) of the global data; ``var`` is ignored, the vectors are row indices of V."""

    def __init__(self, count, offset, rows, V, w, groups, baseline):
        sl = slice(offset, offset + count)
        self.rows, self.V, self.w, self.groups, self.baseline = rows[:, sl], V[:, sl], w[sl], groups[sl], baseline[sl]
        self.calls = []

    def moment_rows_sums(self, var, order, t_begin=0, t_end=None, t_stride=1, vectors=(), center=None, weighted=False, anomaly=False,
                         grouped=False):
        self.calls.append((order, weighted, anomaly, grouped))
        rows = self.rows[t_begin:t_end:t_stride]
        return hr.sums_array(rows, order, self.V[list(vectors)], center, self.w if weighted else None, self.groups if grouped else None,
                             N_GROUPS if grouped else None, self.baseline if anomaly else None)


def bits(d):
    return {k: np.asarray(v, dtype=np.float64).view(np.uint64).tolist() for k, v in d.items()}


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    data = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, *data)
    out = {"rank": rank, "world": dist.get_world_size(), "offset": se.offset, "count": se.count}
    out["plain"] = bits(se.moment_rows_global("T"))
    out["full"] = bits(se.moment_rows_global("T", 1, N_ROWS, 2, vectors=[1, 0], weighted=True, anomaly=True, grouped=True))
    out["calls"] = se.ensemble.calls
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
