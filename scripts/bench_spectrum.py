"""Cost of the per-member band powers (Ensemble.spectrum, csrc/spectrum.hip) on the GPU, against the per-member variability
statistics (Ensemble.variability, csrc/variability.hip) over the same rows as the yardstick: 171 annual rows of Surface Temperature
of a two-layer ensemble after a run, eight bands over every frequency, the three detrending modes of both calls in alternation in
one process.  Each call is timed by the host clock around it; a call returns after its kernel has finished (the entry points
synchronise the handle's stream), so the time is the uploads (row pointers, coefficient table), the launch and the kernel.  Two
warm-up rounds, then --runs timed rounds; the median, minimum and maximum are printed, each mode's ratio to variability()'s median,
and the median against the two counts that bound the kernel from below:
    3 J n N  f64 operations of the recurrence over the FP64 vector issue peak (--peak-tflops, counted as operations, not FMAs), and
    8 R N (ceil(J / F) + 1)  bytes of row traffic over --peak-gbs,
with n the working series' length, J = (n - 1) // 2 and F the kernel's tile of frequencies (kSpecF).  profiles/spectrum_bench.txt
holds one output of this script.

    python scripts/bench_spectrum.py [--runs 20] [--sizes 100000 1000000]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402

R = 171
F = 16                # kSpecF of csrc/spectrum.hip
YEARS = np.arange(1850.0, 1850.0 + R)
BOUNDS = np.append(YEARS, YEARS[-1] + 1.0)
LO = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HI = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
TS = "Surface Temperature"
MODES = ("mean", "linear", "difference")


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
    """{("spectrum" | "variability", mode): [ms]}: two warm-up rounds, then `runs` rounds of the six calls in alternation."""
    calls = {}
    for m in MODES:
        calls[("spectrum", m)] = lambda m=m: e.spectrum(TS, 0, R, detrend=m, bands=8, slot=0)
        calls[("variability", m)] = lambda m=m: e.variability(TS, 0, R, detrend=m, slot=1)
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
    ap.add_argument("--peak-tflops", type=float, default=39.3,
                    help="FP64 vector issue peak in 1e12 operations per second (the MI355X data sheet's 78.6 TFLOPS counts an FMA as two)")
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak in GB/s (data sheet)")
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs must be at least 1")
    for n in a.sizes:
        with ensemble(n) as e:
            ms = timed(e, a.runs)
        print(f"N = {n}, {R} rows, 8 bands, tile F = {F}, {a.runs} rounds (wall ms per call, synchronised)")
        for m in MODES:
            terms = R - 1 if m == "difference" else R
            J = (terms - 1) // 2
            ops = 3.0 * J * terms * n
            passes = -(-J // F) + 1
            traffic = 8.0 * R * n * passes
            base = statistics.median(ms[("variability", m)])
            x = ms[("spectrum", m)]
            med = statistics.median(x)
            t_ops, t_bytes = 1e3 * ops / (a.peak_tflops * 1e12), 1e3 * traffic / (a.peak_gbs * 1e9)
            v = ms[("variability", m)]
            print(f"  variability {m:<10} median {base:8.3f}  min {min(v):8.3f}  max {max(v):8.3f}")
            print(f"  spectrum    {m:<10} median {med:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}   ratio to variability {med / base:6.2f}")
            print(f"      3 J n N = {ops:.3e} operations: {t_ops:7.3f} ms at the issue peak ({ops / (med * 1e-3) / 1e12:5.1f} T/s achieved);"
                  f"  {passes} passes = {traffic / 1e9:.2f} GB: {t_bytes:7.3f} ms at the HBM peak ({traffic / (med * 1e-3) / 1e9:6.0f} GB/s achieved);"
                  f"  median / larger count {med / max(t_ops, t_bytes):5.2f}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
