"""Worker for tests/test_distributed_moments_cpu.py: one rank of a gloo group running ShardedEnsemble.moments_global on a stand-in
ensemble whose ``moment_sums`` is the reference's limb scheme (tests/host_moments.sums_array) over the rank's shard of a global
data set that is a known function of the seed.  What is under test is the product's half: the two all-reduces of the int64 arrays
and the finishing step on every rank."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests import host_moments as hm  # noqa: E402

N_GROUPS = 3


def global_data(n_total: int):
    """(X[3][n_total], weights, groups): full-mantissa doubles over 2^+-40, a few non-finite values, 30-bit weights, three groups and
    members of none."""
    rng = np.random.default_rng(n_total)
    X = rng.uniform(1.0, 2.0, (3, n_total)) * np.exp2(rng.integers(-40, 41, (3, n_total))) * rng.choice([-1.0, 1.0], (3, n_total))
    X[1] += 0.5 * X[0]
    X[0, 3], X[2, n_total - 2], X[1, n_total // 2] = np.nan, np.inf, -np.inf
    return X, rng.integers(0, 1 << 30, n_total), rng.integers(-1, N_GROUPS, n_total).astype(np.int32)


class StandInEnsemble:
    """The members [offset, offset + count) of the global data; the vectors are row indices."""

    def __init__(self, count, offset, X, w, groups):
        sl = slice(offset, offset + count)
        self.X, self.w, self.groups = X[:, sl], w[sl], groups[sl]
        self.calls = []

    def moment_sums(self, vectors, order, center=None, weighted=False, grouped=False):
        self.calls.append((order, weighted, grouped))
        return hm.sums_array(self.X[list(vectors)], order, center, self.w if weighted else None,
                             self.groups if grouped else None, N_GROUPS if grouped else None)


def bits(d):
    return {k: np.asarray(v, dtype=np.float64).view(np.uint64).tolist() for k, v in d.items()}


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    X, w, groups = global_data(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, X, w, groups)
    out = {"rank": rank, "world": dist.get_world_size(), "offset": se.offset, "count": se.count}
    out["plain"] = bits(se.moments_global([0, 1, 2]))
    out["weighted_grouped"] = bits(se.moments_global([2, 0], weighted=True, grouped=True))
    out["calls"] = se.ensemble.calls
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
