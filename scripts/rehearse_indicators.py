"""Rehearsal of the sharded anomaly plume, indicator quantiles and exceedance (rscm_amd.distributed.quantile_rows_global(anomaly=True),
quantile_vectors_global, exceedance_global) with REAL ensembles on a one-GPU box: the ranks started by torch.distributed.run share
GPU 0 and reduce over gloo.

Each rank holds its block of ONE global Latin-hypercube two-layer ensemble (ShardedEnsemble.sample_lhs), runs it, overwrites a few
rows with its slice of a global adversarial member set, sets each member's baseline (a per-member mean: no collective), forms its
members' indicators, weights them by a fit to three "observations" (ShardedEnsemble.constrain) and asks for the numbers of the
whole ensemble.  Every rank also runs the whole ensemble alone and checks, bit for bit, that the sharded results are the single
process's -- on full storage and on a windowed handle's output store.

    RSCM_BENCH_BACKEND=gloo python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \\
        --master-addr 127.0.0.1 --master-port 29581 scripts/rehearse_indicators.py --out OUT_DIR
Every rank writes <out>/rank<k>.json; exit code 0 iff all checks hold.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.rehearse_quantiles import HIGH, LOW, Q, SEED, adversarial_rows, f_syn  # noqa: E402

THR = [0.5, 1.0, 1.5, 2.0]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=30_001)
    ap.add_argument("--out", required=True, help="directory for the per-rank result files")
    args = ap.parse_args()
    import torch.distributed as dist
    import rscm_amd
    from rscm_amd.distributed import ShardedEnsemble

    dist.init_process_group(os.environ.get("RSCM_BENCH_BACKEND", "gloo"))
    rank, world = dist.get_rank(), dist.get_world_size()
    device = int(os.environ.get("RSCM_BENCH_DEVICE", "0"))
    n_total = args.members
    t = np.arange(1750, 1901, dtype=np.float64)
    bounds = np.append(t, t[-1] + 1.0)
    adv = adversarial_rows(n_total)

    def make(count, window):
        kw = dict(window_rows=8, output_stride=5) if window else {}
        e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, count, bounds, device=device, **kw)
        e.set_forcing(f_syn(t))
        e.set_initial("Surface Temperature", 0.0)
        e.set_initial("Deep Ocean Temperature", 0.0)
        return e

    def advance(e):
        while e.time_index < len(t) - 1:
            e.run(min(e.time_index + 4, len(t) - 1))

    checks = {}
    for window in (False, True):
        tag = "windowed" if window else "full"
        stride = 5 if window else 1
        se = ShardedEnsemble(n_total, lambda c, _d: make(c, window), device=device)
        se.sample_lhs(SEED, LOW, HIGH)
        advance(se.ensemble)
        with make(n_total, window) as whole:
            whole.sample_lhs(SEED, LOW, HIGH, 0, n_total)
            advance(whole)
            rows = [150] if window else [60, 100, 120]   # (windowed: a row the window holds)
            for r, x in zip(rows, adv):
                whole.set_state(1, r, x)
                se.ensemble.set_state(1, r, np.ascontiguousarray(x[se.offset:se.offset + se.count]))
            ref = (100, 131, stride)                      # 1850-1880 (every 5th year in the output store)
            for h in (se.ensemble, whole):
                h.set_baseline("Surface Temperature", *ref)
            checks[f"{tag}_baseline_equal"] = bool(np.array_equal(_bits(se.ensemble.baseline()),
                                                                  _bits(whole.baseline()[se.offset:se.offset + se.count])))
            obs = dict(obs_var=["Surface Temperature"] * 3, obs_tidx=[144, 146, 148] if window else [60, 100, 140],
                       obs_value=[0.3, 0.5, 0.7], obs_sigma=[0.2, 0.2, 0.2])
            se.constrain(**obs)
            whole.set_weights_from_loglik(whole.loglik(**obs, on_device=True), n_total=n_total)
            for weighted in (False, True):
                wt = "_weighted" if weighted else ""
                got = se.quantile_rows_global("Surface Temperature", Q, 0, None, stride, weighted=weighted, anomaly=True)
                want = whole.quantile_rows("Surface Temperature", Q, 0, None, stride, weighted=weighted, anomaly=True)
                checks[f"{tag}{wt}_anomaly_bit_equal"] = bool(np.array_equal(_bits(got["quantiles"]), _bits(want["quantiles"])))
                mine = se.ensemble.indicators("Surface Temperature", 120, len(t), stride, THR, anomaly=True)
                full = whole.indicators("Surface Temperature", 120, len(t), stride, THR, anomaly=True)
                vm = [mine["mean"], mine["peak"], mine["peak_time"]] + mine["crossing"]
                vf = [full["mean"], full["peak"], full["peak_time"]] + full["crossing"]
                checks[f"{tag}{wt}_indicators_equal"] = all(
                    np.array_equal(_bits(a.to_host()), _bits(b.to_host()[se.offset:se.offset + se.count])) for a, b in zip(vm, vf))
                gq = se.quantile_vectors_global(vm, Q, weighted=weighted)
                wq = whole.quantile_vectors(vf, Q, weighted=weighted)
                checks[f"{tag}{wt}_vectors_bit_equal"] = bool(np.array_equal(_bits(gq["quantiles"]), _bits(wq["quantiles"])))
                ge = se.exceedance_global(mine["peak"], THR, weighted=weighted)
                we = whole.exceedance(full["peak"], THR, weighted=weighted)
                checks[f"{tag}{wt}_exceedance_equal"] = bool(ge["hits"].tolist() == we["hits"].tolist() and ge["total"] == we["total"]
                                                            and np.array_equal(_bits(ge["probability"]), _bits(we["probability"])))
        se.ensemble.close()
    ok = all(checks.values())
    res = {"rank": rank, "world": world, "members": n_total, "ok": ok, "checks": checks}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    if rank == 0:
        print(json.dumps(res), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
