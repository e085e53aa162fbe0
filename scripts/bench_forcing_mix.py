"""Cost of the two-layer mix ensemble (per-member forcing as a scaled sum of K shared components, rscm_ens_create_mix) on the
GPU, against the plain two-layer run, the workaround it replaces and the plain device sampler.  Device-event times
(rscm_ens_last_run_ms, the sampler's device_ms), two warm-up runs, then --runs timed runs per variant taken in alternation; the
median and the minimum are printed.  profiles/forcing_mix_bench.txt holds one output of this script.

    python scripts/bench_forcing_mix.py [--runs 10] [--sizes 1000000 100000]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd import _lib as L  # noqa: E402

T = 751
BOUNDS = np.arange(T + 1, dtype=np.float64) + 1750.0
LO = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HI = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])


def block(n_scen, K):
    t = np.arange(T, dtype=np.float64)
    base = 4.0 * (1.0 - np.exp(-t / 120.0)) + 0.3 * np.sin(2.0 * np.pi * t / 11.0)
    S = np.empty((n_scen, K, T))
    for s in range(n_scen):
        for k in range(K):
            S[s, k] = (1.0 + 0.2 * s) * base / K * (1.0 + 0.1 * np.cos(0.05 * t * (k + 1)))
    return S


def ensemble(n, K, n_scen, mode):
    """K == 0: the plain two-layer handle."""
    e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS, forcing_components=K if K else None)
    e.set_mode(mode)
    lo, hi = (np.r_[LO, np.full(K, 0.7)], np.r_[HI, np.full(K, 1.3)]) if K else (LO, HI)
    e.sample_lhs(20260327, lo, hi)
    scen = (np.arange(n) % n_scen).astype(np.int32) if n_scen > 1 else None
    S = block(n_scen, max(K, 1))
    e.set_forcing(S if K else S[:, 0], scen)
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    return e


def timed(variants, runs):
    """{name: [ms]}: two warm-up runs each, then `runs` rounds over all variants in turn."""
    out = {name: [] for name in variants}
    for r in range(runs + 2):
        for name, e in variants.items():
            e.rewind()
            e.run()
            if r >= 2:
                out[name].append(e.last_run_ms())
    return out


def report(title, times, base=None):
    print(title)
    ref = np.median(times[base]) if base else None
    for name, ms in times.items():
        ms = np.asarray(ms)
        ratio = f"  x{np.median(ms) / ref:.3f} of {base}" if base else ""
        print(f"  {name:<34s} median {np.median(ms):9.3f} ms   min {ms.min():9.3f} ms   ({ms.size} runs){ratio}")


def runs_section(sizes, runs):
    for n in sizes:
        for mode, mode_name in ((rscm_amd.MODE_EXACT, "EXACT"), (rscm_amd.MODE_FAST, "FAST")):
            specs = [("plain two-layer", 0, 1), ("mix K=1 S=1", 1, 1), ("mix K=4 S=1", 4, 1), ("mix K=8 S=1", 8, 1),
                     ("mix K=4 S=3 scenario_of_member", 4, 3)]
            variants = {name: ensemble(n, K, S, mode) for name, K, S in specs}
            report(f"{n} members x {T - 1} steps, {mode_name}", timed(variants, runs), "plain two-layer")
            for e in variants.values():
                e.close()


def workaround_section(n, runs):
    """A plain handle with one host-formed series per member (n_scen = N): the upload and the run."""
    K = 4
    S = block(1, K)
    with ensemble(n, K, 1, rscm_amd.MODE_EXACT) as mix:
        coeff = mix.get_params()[6:]
        P6 = mix.get_params()[:6]
        t0 = time.perf_counter()
        F = S[0, 0][None, :] * coeff[0][:, None]
        for k in range(1, K):
            F = F + S[0, k][None, :] * coeff[k][:, None]
        form_s = time.perf_counter() - t0
        with rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS) as e:
            e.set_params(P6)
            e.set_initial(1, 0.0)
            e.set_initial(2, 0.0)
            up = []
            for _ in range(3):
                t0 = time.perf_counter()
                e.set_forcing(F, np.arange(n, dtype=np.int32))
                up.append(time.perf_counter() - t0)
            times = timed({"plain, n_scen = N host-formed series": e, "mix K=4 S=1": mix}, runs)
            report(f"the workaround at {n} members, EXACT", times, "mix K=4 S=1")
            print(f"  forming the {F.nbytes / 1e6:.0f} MB of series on the host: {form_s * 1e3:.1f} ms; uploading them (set_forcing, host "
                  f"wall time, best of 3): {min(up) * 1e3:.1f} ms; the mix handle's table: {S.nbytes} bytes")


def sampler_section(walkers, iters):
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    t = BOUNDS[:-1]
    axis = core.TimeAxis.from_values(t)
    lin = core.InterpolationStrategy.Linear
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    S = block(1, 4)[0]

    def builder(mix):
        b = (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())
             .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))
        if mix:
            return b.with_forcing_components("Effective Radiative Forcing", {f"c{k}": core.Timeseries(S[k], axis, "W/m^2", lin) for k in range(4)})
        return b.with_exogenous_variable("Effective Radiative Forcing", core.Timeseries(S.sum(axis=0), axis, "W/m^2", lin))

    six = list(core.TL_PARAM_ORDER)
    ranges = dict(zip(six, zip(LO, HI)))
    print(f"device sampler, {walkers} walkers, 18 observations (1850..2020 every 10 years), ms per iteration over {iters} iterations")
    for name, mix, names in (("6 dimensions, plain evaluator", False, six),
                             ("8 dimensions (two coefficients), mix K=4 evaluator", True, six + ["forcing_scale|c0", "forcing_scale|c1"])):
        runner = cal.ModelRunner(builder(mix), names, ["Surface Temperature"])
        truth = runner.run([fixed.get(k, 1.0) for k in names])["Surface Temperature"]
        target = cal.Target()
        for yr in range(1850, 2021, 10):
            target.add_observation("Surface Temperature", float(yr), truth[float(yr)], 0.1)
        params = cal.ParameterSet()
        for k in names:
            lo, hi = ranges.get(k, (0.7, 1.3))
            params.add(k, cal.Uniform(float(lo), float(hi)))
        dev = cal.DeviceEnsembleSampler(params, runner, cal.GaussianLikelihood(), target)
        ms = []
        for r in range(4):
            dev.run(iters, cal.WalkerInit.from_prior(), thin=iters, n_walkers=walkers, seed=r, rng=np.random.default_rng(r))
            if r:
                ms.append(dev.device_ms / iters)
        print(f"  {name:<52s} median {np.median(ms):8.3f} ms   min {min(ms):8.3f} ms   (3 chains)")
        runner.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 100_000])
    ap.add_argument("--walkers", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    L.load()
    if L.device_count() < 1:
        raise SystemExit("needs a HIP device")
    runs_section(a.sizes, max(a.runs, 10))
    workaround_section(100_000, max(a.runs, 10))
    sampler_section(a.walkers, a.iters)


if __name__ == "__main__":
    main()
