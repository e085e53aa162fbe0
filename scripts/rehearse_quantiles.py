"""Rehearsal of rscm_amd.distributed.quantile_rows_global with REAL ensembles on a one-GPU box: the ranks started by
torch.distributed.run share GPU 0, the int64 histogram all-reduces run over gloo (RCCL refuses two ranks on one device).

Each rank holds its block of ONE global Latin-hypercube two-layer ensemble (ShardedEnsemble.sample_lhs), runs it, overwrites a
few rows with its slice of a global adversarial member set (NaNs of both signs, +-inf, +-0, ties, denormals, an all-NaN row, a
row with one member), then asks for the quantiles of the whole ensemble.  Every rank also runs the whole ensemble alone and
checks, bit for bit, that the sharded result is its quantile_rows -- on full storage and on a windowed handle's strided output
store.

    RSCM_BENCH_BACKEND=gloo python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \\
        --master-addr 127.0.0.1 --master-port 29561 scripts/rehearse_quantiles.py --out OUT_DIR
Every rank writes <out>/rank<k>.json; exit code 0 iff all checks hold.

--weighted also constrains the ensemble by its fit to three surface-temperature "observations" (ShardedEnsemble.constrain: the
device log-likelihood, a MAX all-reduce of the local maxima, quantisation with the global member count) and checks the
likelihood-weighted quantiles of the whole ensemble (quantile_rows_global(weighted=True)) against the single process that
quantises the gathered log-likelihood itself: the same weights and the same bits, and numpy's weighted "inverted_cdf".
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOW = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HIGH = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
SEED = 20261015
Q = [0.0, 0.05, 0.17, 0.5, 0.83, 0.95, 1.0, 1e-12]


def f_syn(t):
    return 4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)) + 0.3 * np.sin(2.0 * np.pi * (t - 1750.0) / 11.0)


def adversarial_rows(n):
    rng = np.random.default_rng(11)
    neg_nan = -np.float64(np.nan)
    return [rng.choice([-np.inf, np.inf, -0.0, 0.0, 5e-324, -5e-324, np.nan, neg_nan, 1.0], n),
            rng.choice([-1.0, 0.0, 2.5, 2.5, 7.0], n),
            np.full(n, np.nan),
            np.where(np.arange(n) == n // 3, 2.0, neg_nan),
            rng.choice([-0.0, 0.0], n)]


def weighted_checks(tag, se, whole, stride, n_total, obs_tidx):
    """Sharded constrain + weighted quantiles of the whole ensemble against the single process, bit for bit."""
    from rscm_amd.ensemble import default_weight_bits
    obs = dict(obs_var=["Surface Temperature"] * 3, obs_tidx=obs_tidx, obs_value=[0.3, 0.5, 0.7], obs_sigma=[0.2, 0.2, 0.2])
    ll_max, bits = se.constrain(**obs)
    ll = whole.loglik(**obs, on_device=True)
    want_max, want_bits = whole.set_weights_from_loglik(ll, n_total=n_total)
    out = {f"{tag}_w_scale_equal": ll_max == want_max and bits == want_bits == default_weight_bits(n_total),
           f"{tag}_w_equal": bool(np.array_equal(se.ensemble.member_weights(), whole.member_weights()[se.offset:se.offset + se.count]))}
    got = se.quantile_rows_global("Surface Temperature", Q, 0, None, stride, weighted=True)
    want = whole.quantile_rows("Surface Temperature", Q, 0, None, stride, weighted=True)
    out[f"{tag}_weighted_bit_equal"] = bool(np.array_equal(got["quantiles"].view(np.uint64), want["quantiles"].view(np.uint64)))
    out[f"{tag}_weighted_weight_equal"] = bool(np.array_equal(got["weight"], want["weight"]))
    ser = whole.get_series("Surface Temperature", 0, None, stride)
    w = whole.member_weights()
    ok = want["weight"] > 0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        npq = np.nanquantile(ser[ok], Q, axis=1, weights=np.broadcast_to(w, ser[ok].shape), method="inverted_cdf").T
    unsign = lambda x: np.where(x == 0, 0.0, x)  # noqa: E731  (the key order puts -0.0 first; numpy keeps member order)
    out[f"{tag}_weighted_numpy_equal"] = bool(np.array_equal(unsign(got["quantiles"][ok]), unsign(npq))
                                              and np.isnan(got["quantiles"][~ok]).all())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=30_001)
    ap.add_argument("--out", required=True, help="directory for the per-rank result files")
    ap.add_argument("--weighted", action="store_true", help="also check the likelihood-weighted quantiles (ShardedEnsemble.constrain)")
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

    def advance(e):   # a windowed handle steps in ranges its window holds
        while e.time_index < len(t) - 1:
            e.run(min(e.time_index + 4, len(t) - 1))

    checks = {}
    for window in (False, True):
        tag = "windowed" if window else "full"
        se = ShardedEnsemble(n_total, lambda c, _d: make(c, window), device=device)
        se.sample_lhs(SEED, LOW, HIGH)
        advance(se.ensemble)
        with make(n_total, window) as whole:
            whole.sample_lhs(SEED, LOW, HIGH, 0, n_total)
            advance(whole)
            rows = [150 - 5 * k for k in range(len(adv))] if window else [2, 3, 4, 5, 6]
            for r, x in zip(rows, adv):     # (windowed: the last row is in the window; the others in the output store)
                if window and r != 150:
                    continue
                whole.set_state(1, r, x)
                se.ensemble.set_state(1, r, np.ascontiguousarray(x[se.offset:se.offset + se.count]))
            stride = 5 if window else 1
            got = se.quantile_rows_global("Surface Temperature", Q, 0, None, stride)
            want = whole.quantile_rows("Surface Temperature", Q, 0, None, stride)
            checks[f"{tag}_bit_equal"] = bool(np.array_equal(got["quantiles"].view(np.uint64), want["quantiles"].view(np.uint64)))
            checks[f"{tag}_count_equal"] = bool(np.array_equal(got["count"], want["count"]))
            ser = whole.get_series("Surface Temperature", 0, len(t), stride)
            with np.errstate(all="ignore"):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    npq = np.nanquantile(ser, Q, axis=1).T
            checks[f"{tag}_numpy_equal"] = bool(np.array_equal(got["quantiles"], npq, equal_nan=True))
            if args.weighted:
                checks.update(weighted_checks(tag, se, whole, stride, n_total, [144, 146, 148] if window else [60, 100, 140]))
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
