#!/usr/bin/env python3
"""What a reference period costs ("Reference periods"): the likelihood of a two-layer ensemble on the
1750-2500 axis against annual `Surface Temperature` observations 1850..2020, with and without the reference period 1850-1900
(51 deferred observations in the fused kernel).

  fused    rscm_ens_run_loglik[_ref] at --members (default 1e5): device-event time of the launch (rscm_ens_last_run_ms), median
           and spread of --repeats launches after --warmup;
  stored   rscm_ens_loglik[_ref] at --stored-members (default 1e6) on a run ensemble: host clock around the synchronous call;
  sampler  DeviceEnsembleSampler at --walkers (default 1e5): device milliseconds per iteration;
  copy     a device-to-device copy of the fused kernel's scratch traffic (16 B x deferred observations x members).

One JSON line.  `--root DIR` measures the checkout at DIR instead of this one (the parent commit's, built there: its period-free
figures are what this feature must not slow down); `--no-period` leaves the period out (the only mode an older checkout has).

    python scripts/bench_reference_period.py
    python scripts/bench_reference_period.py --root ../parent --no-period
"""
import argparse
import json
import os
import sys
import time

import numpy as np

LOW = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HIGH = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
NAMES = ["lambda0", "a", "efficacy", "eta", "heat_capacity_surface", "heat_capacity_deep"]
PERIOD_ROWS = (100, 151)   # 1850-1900 on the 1750-2500 axis


def stats(ms):
    ms = np.sort(np.asarray(ms, dtype=np.float64))
    return {"median": float(np.median(ms)), "min": float(ms[0]), "max": float(ms[-1]),
            "p25": float(np.percentile(ms, 25)), "p75": float(np.percentile(ms, 75)), "n": int(len(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--no-period", action="store_true")
    ap.add_argument("--members", type=int, default=100_000)
    ap.add_argument("--stored-members", type=int, default=1_000_000)
    ap.add_argument("--walkers", type=int, default=100_000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--skip", nargs="*", default=[], choices=["fused", "stored", "sampler", "copy"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import rscm_amd
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder

    t = np.arange(1750.0, 2501.0)
    bounds = np.append(t, t[-1] + 1.0)
    F = 4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)) + 0.3 * np.sin(2 * np.pi * (t - 1750.0) / 11.0)
    ot = np.arange(100, 271, dtype=np.int32)   # 1850..2020, annual
    ov = np.ones(len(ot), dtype=np.int32)
    val = np.linspace(-0.2, 1.2, len(ot))
    sig = np.full(len(ot), 0.1)
    modes = [False] if args.no_period else [False, True]
    out = {"root": os.path.abspath(args.root), "observations": int(len(ot)), "deferred_observations": 51}

    def ensemble(n, store):
        e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, bounds, store_series=store)
        e.sample_lhs(20261016, LOW, HIGH)
        e.set_forcing(F)
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        return e

    def kw(period):
        return {"reference": {1: PERIOD_ROWS}} if period else {}

    if "fused" not in args.skip:
        with ensemble(args.members, False) as e:
            for period in modes:
                ms = []
                for k in range(args.warmup + args.repeats):
                    e.run_loglik(ov, ot, val, sig, on_device=True, **kw(period))
                    if k >= args.warmup:
                        ms.append(e.last_run_ms())
                out["fused_period_ms" if period else "fused_ms"] = stats(ms)
        out["fused_members"] = args.members
    if "stored" not in args.skip:
        with ensemble(args.stored_members, True) as e:
            e.run()
            for period in modes:
                ms = []
                for k in range(args.warmup + args.repeats):
                    t0 = time.perf_counter()
                    e.loglik(ov, ot, val, sig, on_device=True, **kw(period))
                    if k >= args.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                out["stored_period_ms" if period else "stored_ms"] = stats(ms)
        out["stored_members"] = args.stored_members
    if "copy" not in args.skip:
        import torch
        n_bytes = 16 * 51 * args.members
        src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        ms = []
        for k in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(src)
            b.record()
            b.synchronize()
            if k >= args.warmup:
                ms.append(a.elapsed_time(b))
        out["copy_ms"] = stats(ms)
        out["copy_bytes"] = n_bytes
    if "sampler" not in args.skip:
        fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
        axis = core.TimeAxis.from_values(t)
        b = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
             .with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(F, axis, "W/m^2", core.InterpolationStrategy.Linear))
             .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))
        runner = cal.ModelRunner(b, NAMES, ["Surface Temperature"])
        truth = runner.run([fixed[k] for k in NAMES])["Surface Temperature"]
        base = sum(truth[float(y)] for y in range(1850, 1901)) / 51
        params = cal.ParameterSet()
        for k, lo, hi in zip(NAMES, LOW, HIGH):
            params.add(k, cal.Uniform(float(lo), float(hi)))
        for period in modes:
            target = cal.Target()
            for yr in range(1850, 2021, 10):   # the README's calibration problem: 18 observations, sigma 0.1 K
                target.add_observation("Surface Temperature", float(yr), truth[float(yr)] - (base if period else 0.0), 0.1)
            if period:
                target.set_reference_period("Surface Temperature", 1850, 1900)
            sampler = cal.DeviceEnsembleSampler(params, runner, cal.GaussianLikelihood(), target)
            rng = np.random.default_rng(20260327)
            sampler.run(2, cal.WalkerInit.from_prior(), n_walkers=args.walkers, rng=rng)  # warm-up
            per_iteration = []
            for rep in range(3):
                start = cal.WalkerInit.explicit(params.sample_random(args.walkers, rng))
                sampler.run(args.iterations, start, n_walkers=args.walkers, thin=args.iterations, seed=rep)
                per_iteration.append(sampler.device_ms / args.iterations)
            out["sampler_period_ms_per_iteration" if period else "sampler_ms_per_iteration"] = stats(per_iteration)
        out["walkers"] = args.walkers
        runner.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
