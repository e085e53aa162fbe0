"""Cost of the per-member covariability of two variables (Ensemble.covariability, csrc/covariability.hip) on the GPU, against the two
Ensemble.variability calls that read the same rows: 171 annual rows of Surface Temperature and of the ocean heat content (a
diagnostic variable) of a two-layer ensemble after a run.  covariability() -- temperature linearly detrended at the midpoints
against the heat content's differences, lags=0 and lags=3 -- is timed in alternation in one process with variability() of the
temperature followed by variability() of the heat content.  Each call is timed by the host clock around it; a call returns after
its kernel has finished (the entry points synchronise the handle's stream), so the time is the row-pointer uploads, the launch and
the kernel.  Two warm-up rounds, then --runs timed rounds; the median, minimum and maximum are printed, the bytes the kernel reads
by count (covariability: two variables, two passes, 2 x 2 x 8 x R x N; one variability call: 2 x 8 x R x N) over the median, and
the ratio of the covariability medians to the sum of the two variability medians, which move the same bytes in two launches.
profiles/covariability_bench.txt holds one output of this script.

    python scripts/bench_covariability.py [--runs 20] [--sizes 100000 1000000]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402

R = 171
YEARS = np.arange(1850.0, 1850.0 + R)
BOUNDS = np.append(YEARS, YEARS[-1] + 1.0)
LO = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HI = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
TS = "Surface Temperature"


def ensemble(n):
    e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, BOUNDS)
    e.sample_lhs(20260327, LO, HI)
    t = YEARS - 1850.0
    e.set_forcing(0.035 * t + 0.25 * np.sin(2.0 * np.pi * t / 11.0))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.set_forcing_noise(0.4, 1, 0, 0.6)
    e.run()
    return e


def timed(e, runs):
    """{call: [ms]}: two warm-up rounds, then `runs` rounds of the four calls in alternation."""
    heat = e.define_heat_content()
    e.compute_diagnostic(heat, 0, R)
    calls = {"covariability, lags=0": lambda: e.covariability(TS, heat, 0, R, 1, "linear", "difference", 0, slot=0),
             "covariability, lags=3": lambda: e.covariability(TS, heat, 0, R, 1, "linear", "difference", 3, slot=0),
             "variability(Ts)": lambda: e.variability(TS, 0, R, detrend="linear", slot=1),
             "variability(heat)": lambda: e.variability(heat, 0, R, detrend="difference", slot=2)}
    out = {name: [] for name in calls}
    for r in range(runs + 2):
        for name, call in calls.items():
            e.sync()
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if r >= 2:
                out[name].append(1e3 * dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs must be at least 1")
    for n in a.sizes:
        with ensemble(n) as e:
            ms = timed(e, a.runs)
        pair = [ms["variability(Ts)"], ms["variability(heat)"]]
        base = sum(statistics.median(x) for x in pair)
        spread = sum(max(x) - min(x) for x in pair)
        print(f"N = {n}, {R} rows, {a.runs} rounds (wall ms per call, synchronised)")
        for name, x in ms.items():
            reads = 4 if name.startswith("covariability") else 2
            med = statistics.median(x)
            gbs = reads * 8.0 * R * n / (med * 1e-3) / 1e9
            line = f"  {name:<22} median {med:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}   {reads} x 8 B x R x N over the median: {gbs:7.0f} GB/s"
            if reads == 4:
                line += f"   ratio to the two variability calls {med / base:5.2f}  (median - their sum {med - base:+.3f} ms, spread {max(x) - min(x):.3f} ms)"
            print(line)
        print(f"  the two variability calls: sum of the medians {base:8.3f} ms, sum of their min-max spreads {spread:.3f} ms")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
