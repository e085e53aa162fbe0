"""Cost of a diagnostic variable (Ensemble.compute_diagnostic, csrc/diagnostic.hip) on the GPU, against the per-member indicators
(Ensemble.indicators, csrc/indicators.hip) over the same rows as the yardstick: the ocean heat content (two terms) of a two-layer
ensemble after a run, 171 annual rows, the two calls in alternation in one process.  Each call is timed by the host clock around
it; a call returns after its kernel has finished (the entry points synchronise the handle's stream), so the time is the
row-pointer upload, the launch and the kernel.  Two warm-up rounds, then --runs timed rounds; the median, minimum and maximum are
printed, the bytes each kernel moves by count over the median -- the diagnostic reads K = 2 rows and writes one per row and
member, (K + 1) x 8 x R x N, the indicators read one, 8 x R x N -- and the ratio of the medians, which the byte count puts at
K + 1 = 3.  profiles/diagnostic_bench.txt holds one output of this script.

    python scripts/bench_diagnostic.py [--runs 20] [--sizes 100000 1000000]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402

R = 171
K = 2
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
    """{"indicators" | "diagnostic": [ms]}: two warm-up rounds, then `runs` rounds of the two calls in alternation."""
    heat = e.define_heat_content()
    calls = {"indicators": lambda: e.indicators(TS, 0, R, slot=0), "diagnostic": lambda: e.compute_diagnostic(heat, 0, R)}
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
        base = statistics.median(ms["indicators"])
        print(f"N = {n}, {R} rows, {a.runs} rounds (wall ms per call, synchronised)")
        for name, x in ms.items():
            rows = 1 if name == "indicators" else K + 1
            med = statistics.median(x)
            gbs = rows * 8.0 * R * n / (med * 1e-3) / 1e9
            print(f"  {name:<11} median {med:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}   {rows} x 8 B x R x N over the median: {gbs:7.0f} GB/s"
                  f"   ratio to indicators {med / base:5.2f}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
