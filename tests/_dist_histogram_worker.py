"""Worker for tests/test_histogram_cpu.py: one rank of a gloo group running ShardedEnsemble.histogram_rows_global,
histogram_vectors_global and histogram2d_global on a stand-in ensemble whose ``histogram_rows``, ``histogram_vectors`` and
``histogram2d`` are the restatement (tests/host_histogram.py) over the rank's shard of a global data set that is a known function of
the seed.  What is under test is the product's half: the one all-reduce of the concatenated int64 arrays and the finishers on every
rank."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests import host_histogram as hh  # noqa: E402
from tests._dist_exceedance_rows_worker import N_GROUPS, N_ROWS, bits, global_data  # noqa: E402,F401

EDGES = [-0.5, 0.0, 0.1, 0.3, 0.4, 1.0]
EDGES_PER_VECTOR = [[-1.0, 0.0, 0.5, 2.0], [-0.2, 0.2, 0.3, 0.9]]
EDGES_Y = [-2.0, 0.2, 0.6]


class StandInEnsemble:
    """The members [offset, offset + count) of the global data; ``var`` is ignored, and a "vector" is the index of a row."""

    def __init__(self, count, offset, rows, record, w, groups, baseline):
        sl = slice(offset, offset + count)
        self.rows, self.w, self.groups, self.baseline = rows[:, sl], w[sl], groups[sl], baseline[sl]
        self.calls = []

    def _kw(self, weighted, grouped):
        return dict(weights=self.w if weighted else None, groups=self.groups if grouped else None, n_groups=N_GROUPS if grouped else None)

    def histogram_rows(self, var, edges, t_begin=0, t_end=None, t_stride=1, weighted=False, anomaly=False, grouped=False):
        self.calls.append(("rows", weighted, anomaly, grouped))
        return hh.histogram_rows(self.rows[t_begin:t_end:t_stride], edges, baseline=self.baseline if anomaly else None, **self._kw(weighted, grouped))

    def histogram_vectors(self, vectors, edges, weighted=False, grouped=False):
        self.calls.append(("vectors", weighted, False, grouped))
        return hh.histogram_rows(self.rows[list(vectors)], edges, **self._kw(weighted, grouped))

    def histogram2d(self, x, y, edges_x, edges_y, weighted=False, grouped=False):
        self.calls.append(("2d", weighted, False, grouped))
        return hh.histogram2d(self.rows[x], self.rows[y], edges_x, edges_y, **self._kw(weighted, grouped))


def results(se):
    return {"rows_plain": bits(se.histogram_rows_global("T", EDGES)),
            "rows_full": bits(se.histogram_rows_global("T", EDGES, 1, N_ROWS, 2, weighted=True, anomaly=True, grouped=True)),
            "vectors_plain": bits(se.histogram_vectors_global([0, 3], EDGES_PER_VECTOR)),
            "vectors_full": bits(se.histogram_vectors_global([4, 2, 5], EDGES, weighted=True, grouped=True)),
            "joint_plain": bits(se.histogram2d_global(0, 3, EDGES, EDGES_Y)),
            "joint_full": bits(se.histogram2d_global(4, 2, EDGES, EDGES_Y, weighted=True, grouped=True))}


CALLS = [["rows", False, False, False], ["rows", True, True, True], ["vectors", False, False, False], ["vectors", True, False, True],
         ["2d", False, False, False], ["2d", True, False, True]]


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    data = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, *data)
    out = {"rank": rank, "world": dist.get_world_size(), "offset": se.offset, "count": se.count}
    out.update(results(se))
    out["calls"] = [list(c) for c in se.ensemble.calls]
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
