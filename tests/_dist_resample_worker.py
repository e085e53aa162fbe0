"""Worker for tests/test_host_resample.py: one rank of a gloo group running rscm_amd.distributed.resample_global and
weights_stats_global.  The draw needs a GPU, so the rank's ensemble is a stand-in whose resample and weights_stats are the
numpy restatement (tests/host_resample.py) on its block of one global weight vector.  What is under test is the product's
loop: the all-gather of the exact totals into w_before / w_total, the one offset every rank derives, the reduced statistics."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests import host_resample as hr  # noqa: E402


def global_weights(n_total):
    """[n_total] int64 weights with runs of zeros, a few heavy members and weights up to 2^40."""
    g = np.arange(n_total, dtype=np.int64)
    w = (g * 2654435761 % 1000003) * ((g % 5 == 0) * ((1 << 40) // 1000003) + 1)
    w[(g % 9 == 4) | (g % 17 < 3)] = 0
    return w.astype(np.int64)


class _Vector:
    def __init__(self, k_first, anc):
        self.k_first, self.anc = k_first, anc

    def __len__(self):
        return len(self.anc)


class StandInEnsemble:
    def __init__(self, w):
        self.w = w

    def weights_stats(self):
        return hr.stats(self.w)

    def resample(self, n_draws, seed=0, offset=None, w_before=0, w_total=None):
        k_first, count, anc = hr.ancestors(self.w, n_draws, offset, w_before, w_total)
        return _Vector(k_first, anc)


def main():
    n_total, n_draws, seed, out_dir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    w = global_weights(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(w[se.offset:se.offset + se.count])
    k_first, count, anc = se.resample(n_draws, seed)
    st = se.weights_stats_global()
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump({"rank": rank, "world": dist.get_world_size(), "offset": se.offset, "k_first": int(k_first), "count": int(count),
                   "ancestors": [int(a) for a in anc.anc], "stats": {k: (v if k == "ess" else str(v)) for k, v in st.items()}}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
