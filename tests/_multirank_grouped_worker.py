"""Worker for tests/test_multirank_grouped_gpu.py: one rank of a gloo group sharing GPU 0 with the others.  Each rank holds its
block of one global Latin-hypercube two-layer ensemble and its block of one global group vector, every rank also runs the whole
ensemble alone, and the grouped quantiles and exceedance of the sharded ensemble must carry the one-handle bits."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOW = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HIGH = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
Q = [0.0, 0.05, 0.5, 0.95, 1.0]
G = 5


def main():
    n_total, out = int(sys.argv[1]), sys.argv[2]
    import torch.distributed as dist
    import rscm_amd
    from rscm_amd.distributed import ShardedEnsemble
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    t = np.arange(1750, 1771, dtype=np.float64)
    bounds = np.append(t, t[-1] + 1.0)
    rng = np.random.default_rng(3)
    group = np.sort(rng.integers(0, G - 1, n_total)).astype(np.int32)     # contiguous: rank 0 holds no member of the last groups
    group[rng.random(n_total) < 0.1] = -1
    w = rng.integers(0, 1 << 30, n_total, dtype=np.int64)
    spoiled = np.where(rng.random(n_total) < 0.3, np.nan, rng.standard_normal(n_total))

    def make(count, _d=0):
        e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, count, bounds)
        e.set_forcing(4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        return e

    se = ShardedEnsemble(n_total, make)
    sl = slice(se.offset, se.offset + se.count)
    se.sample_lhs(11, LOW, HIGH)
    se.ensemble.run()
    se.ensemble.set_state(1, 7, np.ascontiguousarray(spoiled[sl]))
    se.ensemble.set_member_groups(group[sl], G)
    se.ensemble.set_member_weights(w[sl])
    checks = {}
    with make(n_total) as whole:
        whole.sample_lhs(11, LOW, HIGH, 0, n_total)
        whole.run()
        whole.set_state(1, 7, spoiled)
        whole.set_member_groups(group, G)
        whole.set_member_weights(w)
        for weighted in (False, True):
            key, tag = ("weight", "weighted") if weighted else ("count", "plain")
            got = se.quantile_rows_global(1, Q, weighted=weighted, grouped=True)
            want = whole.quantile_rows(1, Q, weighted=weighted, grouped=True)
            checks[f"{tag}_bit_equal"] = bool(np.array_equal(got["quantiles"].view(np.uint64), want["quantiles"].view(np.uint64)))
            checks[f"{tag}_{key}_equal"] = bool(np.array_equal(got[key], want[key]))
            a = se.exceedance_global(se.ensemble.params_vector(4), [8.0, 12.0], weighted=weighted, grouped=True)
            b = whole.exceedance(whole.params_vector(4), [8.0, 12.0], weighted=weighted, grouped=True)
            checks[f"{tag}_exceedance_equal"] = bool(np.array_equal(a["hits"], b["hits"]) and np.array_equal(a["total"], b["total"]))
            v = se.quantile_vectors_global([se.ensemble.params_vector(0)], Q, weighted=weighted, grouped=True)
            u = whole.quantile_vectors([whole.params_vector(0)], Q, weighted=weighted, grouped=True)
            checks[f"{tag}_vectors_bit_equal"] = bool(np.array_equal(v["quantiles"].view(np.uint64), u["quantiles"].view(np.uint64)))
        checks["a_group_absent_from_rank_0"] = bool(world == 1 or rank != 0 or (group[sl] < G - 2).all())
    se.ensemble.close()
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"rank": rank, "world": world, "ok": all(checks.values()), "checks": checks}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
