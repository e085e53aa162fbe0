"""Reference-period targets ("Reference periods") over several ranks, rehearsed on a one-GPU box: the ranks
started by torch.distributed.run share GPU 0, collectives over gloo.

  * the device sampler sharded over the ranks against a target whose observations are anomalies from 1850-1900
    (rscm_sampler_set_reference on every rank's evaluator): the single-rank chain, bit for bit;
  * ShardedEnsemble.constrain(..., reference=...) then quantile_rows_global(weighted=True, anomaly=True): the single process that
    weights the whole ensemble by its anomaly fit, bit for bit.

    RSCM_BENCH_BACKEND=gloo python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \\
        --master-addr 127.0.0.1 --master-port 29581 scripts/rehearse_reference_period.py --out OUT_DIR
Every rank writes <out>/rank<k>.json; exit code 0 iff all checks hold on all ranks.
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
NAMES = ["lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep"]
SEED = 20261016
Q = [0.05, 0.17, 0.5, 0.83, 0.95]


def f_syn(t):
    return 4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)) + 0.3 * np.sin(2.0 * np.pi * (t - 1750.0) / 11.0)


def sampler_checks(args, device):
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    t = np.arange(1750, 2101, dtype=np.float64)
    axis = core.TimeAxis.from_values(t)
    defaults = dict(lambda0=1.0, a=0.0, efficacy=1.0, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    b = (core.ModelBuilder().with_device(device).with_time_axis(axis)
         .with_rust_component(TwoLayerBuilder.from_parameters(defaults).build())
         .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(f_syn(t), axis, "W/m^2", core.InterpolationStrategy.Linear))
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))
    runner = cal.ModelRunner(b, NAMES, ["Surface Temperature"])
    truth = runner.run([defaults[k] for k in NAMES])["Surface Temperature"]
    base = sum(truth[float(y)] for y in range(1850, 1901)) / 51
    target = cal.Target()
    for yr in range(1850, 2021, 10):
        target.add_observation("Surface Temperature", float(yr), truth[float(yr)] - base, 0.1)
    plain = dev_chain = None
    params = cal.ParameterSet()
    for k, lo, hi in zip(NAMES, LOW, HIGH):
        params.add(k, cal.Uniform(float(lo), float(hi)))
    W = args.walkers
    pos = params.sample_random(W, np.random.default_rng(2026 + W))
    out = {}
    for period in (False, True):
        if period:
            target.set_reference_period("Surface Temperature", 1850, 1900)
        dev = cal.DeviceEnsembleSampler(params, runner, cal.GaussianLikelihood(), target)
        sharded = dev.run(args.sweeps, cal.WalkerInit.explicit(pos), n_walkers=W, seed=17)
        acc_s, prop_s = dev.n_accepted.copy(), dev.n_proposed.copy()
        single = dev.run(args.sweeps, cal.WalkerInit.explicit(pos), n_walkers=W, seed=17, shard=False)
        xs, x1 = np.stack(sharded._samples), np.stack(single._samples)
        ls, l1 = np.stack(sharded._log_probs), np.stack(single._log_probs)
        tag = "period" if period else "plain"
        out[f"sampler_{tag}_positions_bit_equal"] = bool(np.array_equal(xs.view(np.uint64), x1.view(np.uint64)))
        out[f"sampler_{tag}_log_probs_bit_equal"] = bool(np.array_equal(ls.view(np.uint64), l1.view(np.uint64)))
        out[f"sampler_{tag}_counters_equal"] = bool(np.array_equal(acc_s, dev.n_accepted) and np.array_equal(prop_s, dev.n_proposed))
        out[f"sampler_{tag}_some_walkers_moved"] = bool(0.0 < (xs[-1] != pos).any(axis=1).mean() < 1.0)
        if period:
            dev_chain = ls
        else:
            plain = ls
    out["sampler_period_changes_the_scores"] = bool(not np.array_equal(plain, dev_chain))
    runner.close()
    return out


def constrain_checks(args, device):
    import rscm_amd
    from rscm_amd.distributed import ShardedEnsemble
    n_total = args.members
    t = np.arange(1750, 2051, dtype=np.float64)
    bounds = np.append(t, t[-1] + 1.0)

    def make(count, _device=None):
        e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, count, bounds, device=device)
        e.set_forcing(f_syn(t))
        e.set_initial("Surface Temperature", 0.0)
        e.set_initial("Deep Ocean Temperature", 0.0)
        return e

    reference = {"Surface Temperature": (100, 151)}   # 1850-1900
    obs = dict(obs_var=["Surface Temperature"] * 4, obs_tidx=[160, 200, 240, 270], obs_value=[0.05, 0.3, 0.7, 1.1],
               obs_sigma=[0.1, 0.1, 0.15, 0.15])
    se = ShardedEnsemble(n_total, make, device=device)
    se.sample_lhs(SEED, LOW, HIGH)
    se.run()
    out = {}
    with make(n_total) as whole:
        whole.sample_lhs(SEED, LOW, HIGH, 0, n_total)
        whole.run()
        for e in (se.ensemble, whole):
            e.set_baseline("Surface Temperature", 100, 151)
        ll_max, bits = se.constrain(**obs, reference=reference)
        ll = whole.loglik(**obs, on_device=True, reference=reference)
        want_max, want_bits = whole.set_weights_from_loglik(ll, n_total=n_total)
        out["constrain_scale_equal"] = bool(ll_max == want_max and bits == want_bits)
        out["constrain_weights_equal"] = bool(np.array_equal(se.ensemble.member_weights(),
                                                             whole.member_weights()[se.offset:se.offset + se.count]))
        got_ll = se.loglik_global(**obs, reference=reference)
        out["loglik_global_bit_equal"] = bool(np.array_equal(got_ll.view(np.uint64), ll.to_host().view(np.uint64)))
        absolute = whole.loglik(**obs)
        out["anomaly_fit_differs_from_absolute_fit"] = bool(not np.array_equal(absolute, got_ll))
        got = se.quantile_rows_global("Surface Temperature", Q, 150, None, 10, weighted=True, anomaly=True)
        want = whole.quantile_rows("Surface Temperature", Q, 150, None, 10, weighted=True, anomaly=True)
        out["constrained_anomaly_plume_bit_equal"] = bool(np.array_equal(got["quantiles"].view(np.uint64), want["quantiles"].view(np.uint64)))
        out["constrained_anomaly_plume_weight_equal"] = bool(np.array_equal(got["weight"], want["weight"]) and (want["weight"] > 0).all())
    se.ensemble.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--members", type=int, default=30_001)
    ap.add_argument("--out", required=True, help="directory for the per-rank result files")
    args = ap.parse_args()
    import torch.distributed as dist

    dist.init_process_group(os.environ.get("RSCM_BENCH_BACKEND", "gloo"))
    rank, world = dist.get_rank(), dist.get_world_size()
    device = int(os.environ.get("RSCM_BENCH_DEVICE", "0"))
    checks = sampler_checks(args, device)
    checks.update(constrain_checks(args, device))
    ok = all(checks.values())
    res = {"rank": rank, "world": world, "ok": ok, "checks": checks}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    flags = [None] * world
    dist.all_gather_object(flags, ok)
    if rank == 0:
        print(json.dumps(res), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
