"""Worker for tests/test_distributed_variability_cpu.py: one rank of a gloo group running ShardedEnsemble.constrain and then
ShardedEnsemble.constrain_loglik with the same per-member log-likelihood, on the stand-in ensemble of
tests/_dist_wquantile_worker.py (log-likelihoods and status are known functions of the GLOBAL member id; the weights are quantised in
numpy as the device does).  What is under test is the product's half of the call: the local max, the MAX all-reduce, the weights."""
import json
import os
import sys

import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rscm_amd.distributed import ShardedEnsemble  # noqa: E402
from tests._dist_quantile_worker import global_rows  # noqa: E402
from tests._dist_wquantile_worker import StandInEnsemble, global_loglik  # noqa: E402


def main():
    n_total, out_dir = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    ll, status = global_loglik(n_total)
    se = ShardedEnsemble(n_total, lambda c, d: None)
    se.ensemble = StandInEnsemble(se.count, se.offset, global_rows(n_total), ll, status)
    out = {"rank": rank, "world": dist.get_world_size(), "offset": se.offset, "count": se.count}
    out["constrain"] = list(se.constrain(1, [0], [0.0], [1.0]))
    out["w_constrain"] = se.ensemble.w.tolist()
    se.ensemble.w = None
    out["constrain_loglik"] = list(se.constrain_loglik(se.ensemble.ll))
    out["w_constrain_loglik"] = se.ensemble.w.tolist()
    out["constrain_loglik_bits20"] = list(se.constrain_loglik(se.ensemble.ll, 20))
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
