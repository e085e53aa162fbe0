"""Cost of the per-member co-spectra of two variables (Ensemble.cross_spectrum, csrc/cross_spectrum.hip) on the GPU, against the two
Ensemble.spectrum calls over the same rows and bands, one per variable: 171 annual rows of Surface Temperature and of the ocean heat
content (a diagnostic variable) of a two-layer ensemble after a run.  cross_spectrum() -- temperature linearly detrended at the
midpoints against the heat content's differences, over three bands that hold all 84 frequencies and over one band that holds the
lowest eighth -- is timed in alternation in one process with spectrum() of the temperature (linear) followed by spectrum() of the heat
content (difference) over the same edges.  The spectrum kernel is the yardstick: it advances the same recurrence, one series per call,
at a tile of 16 frequencies against this kernel's 8 for two series.  Each call is timed by the host clock around it; a call returns
after its kernel has finished (the entry points synchronise the handle's stream), so the time is the uploads, the launch and the
kernel.  Two warm-up rounds, then --runs timed rounds; the median, minimum and maximum are printed and the ratio of the cross_spectrum
median to the sum of the two spectrum medians.  By operation count the recurrences cost the same on both sides, 6 f64 operations per
term and frequency for the two series.  profiles/cross_spectrum_bench.txt holds one output of this script.

    python scripts/bench_cross_spectrum.py [--runs 20] [--sizes 100000 1000000]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd.variability import band_edges  # noqa: E402

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
    """{call: [ms]}: two warm-up rounds, then `runs` rounds of the six calls in alternation."""
    heat = e.define_heat_content()
    e.compute_diagnostic(heat, 0, R)
    n = R - 1                                   # terms of the cross-spectrum's working series and of the differenced heat content
    J = (n - 1) // 2
    cases = {"3 bands, all frequencies": band_edges(n, 3), "1 band, the lowest eighth": np.array([1, 1 + max(J // 8, 1)], dtype=np.int32)}
    calls = {}
    for label, edges in cases.items():
        calls[f"cross_spectrum, {label}"] = lambda edges=edges: e.cross_spectrum(TS, heat, 0, R, 1, "linear", "difference", edges, slot=0)
        # (the temperature alone has n + 1 terms and the same J = 84 here: the same edges are valid for both calls)
        calls[f"spectrum(Ts), {label}"] = lambda edges=edges: e.spectrum(TS, 0, R, detrend="linear", bands=edges, slot=1)
        calls[f"spectrum(heat), {label}"] = lambda edges=edges: e.spectrum(heat, 0, R, detrend="difference", bands=edges, slot=2)
    out = {name: [] for name in calls}
    for r in range(runs + 2):
        for name, call in calls.items():
            e.sync()
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if r >= 2:
                out[name].append(1e3 * dt)
    return out, {label: edges.tolist() for label, edges in cases.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs must be at least 1")
    for n in a.sizes:
        with ensemble(n) as e:
            ms, cases = timed(e, a.runs)
        print(f"N = {n}, {R} rows, {a.runs} rounds (wall ms per call, synchronised)")
        for label, edges in cases.items():
            print(f"  {label}: edges {edges}")
            pair = [ms[f"spectrum(Ts), {label}"], ms[f"spectrum(heat), {label}"]]
            base = sum(statistics.median(x) for x in pair)
            spread = sum(max(x) - min(x) for x in pair)
            for name in (f"cross_spectrum, {label}", f"spectrum(Ts), {label}", f"spectrum(heat), {label}"):
                x = ms[name]
                med = statistics.median(x)
                line = f"    {name.split(',')[0]:<16} median {med:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}"
                if name.startswith("cross_spectrum"):
                    line += f"   ratio to the two spectrum calls {med / base:5.2f}  (median - their sum {med - base:+.3f} ms, spread {max(x) - min(x):.3f} ms)"
                print(line)
            print(f"    the two spectrum calls: sum of the medians {base:8.3f} ms, sum of their min-max spreads {spread:.3f} ms")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
