"""Cost of a running-mean diagnostic (Ensemble.define_running_mean / compute_diagnostic, csrc/running_mean.hip) on the GPU, beside
two yardsticks over the same output rows: compute_diagnostic of a one-term linear diagnostic ([(1, None, 1.0)], csrc/diagnostic.hip),
which reads one row and writes one per output -- the 16 B per element that are the running mean's floor -- and the host route
(get_series of the source rows, rscm_amd.variability.series_running_mean, and the upload of the result with set_state).

A two-layer ensemble with red forcing noise is run over an annual axis of R + 63 rows, R the output rows of the size; the cases
are the centred mean of the surface temperature over 20 terms and over 64 terms at t_stride 1 (R outputs), and the disjoint
12-term means at t_stride 12 (as many outputs as the axis holds).  The two device calls alternate in one process; each is timed by
the host clock around it, and a call returns after its kernel has finished (the entry points synchronise the handle's stream), so
the time is the row-pointer upload, the launch and the kernel.  Two warm-up rounds, then --runs timed rounds: median, minimum and
maximum.  Bytes by count: the floor 16 B x R x N, and what the running mean moves with its tile's overlap, 8 B x N x (source rows
read per tile x tiles + R).  The host route is timed once per size, at 20 terms, after everything else (its upload writes rows).
profiles/running_mean_bench.txt holds one output of this script.

    python scripts/bench_running_mean.py [--runs 20] [--sizes 1000000:171 100000:751] [--no-host]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd.variability import running_mean_back, series_running_mean  # noqa: E402

LO = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
HI = np.array([1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
TS = "Surface Temperature"
MAX_WINDOW = 64
CASES = (("W = 20, t_stride 1", 20, 1), ("W = 64, t_stride 1", 64, 1), ("W = 12, t_stride 12", 12, 12))
# kRunMeanThreads, kRunMeanBatch, kRunMeanMinBlocks and kRunMeanMaxOverlap of csrc/running_mean.hpp
THREADS, BATCH, MIN_BLOCKS, MAX_OVERLAP = 256, 8, 2048, 4


def tile_rows(n_rows, window, m, n):
    """running_mean_tile of csrc/running_mean.hip: the outputs a block forms."""
    blocks_x = -(-n // THREADS)
    tiles = -(-MIN_BLOCKS // blocks_x)
    rows = -(-n_rows // tiles)
    if m < window:
        rows = max(rows, -(-MAX_OVERLAP * (window - m) // m))
    return -(-max(rows, 1) // BATCH) * BATCH


def rows_read(n_rows, window, m, n):
    """(source rows the launch reads over all its tiles, the tile length)."""
    tile = tile_rows(n_rows, window, m, n)
    total = 0
    for r0 in range(0, n_rows, tile):
        k = min(tile, n_rows - r0)
        total += k * window if m >= window else (k - 1) * m + window
    return total, tile


def ensemble(n, T):
    years = np.arange(1850.0, 1850.0 + T)
    e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, np.append(years, years[-1] + 1.0))
    e.sample_lhs(20260327, LO, HI)
    t = years - 1850.0
    e.set_forcing(0.035 * t + 0.25 * np.sin(2.0 * np.pi * t / 11.0))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.set_forcing_noise(0.4, 1, 0, 0.6)
    e.run()
    return e


def timed(e, calls, runs):
    """{name: [ms]}: two warm-up rounds, then `runs` rounds of the calls in alternation."""
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


def line(name, x, nbytes, what):
    med = statistics.median(x)
    return f"  {name:<13} median {med:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}   {what}: {nbytes / (med * 1e-3) / 1e9:7.0f} GB/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", nargs="+", default=["1000000:171", "100000:751"], help="members:output rows")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    a = ap.parse_args()
    if a.runs < 1:
        ap.error("--runs must be at least 1")
    for size in a.sizes:
        n, R = (int(x) for x in size.split(":"))
        T = R + MAX_WINDOW - 1
        with ensemble(n, T) as e:
            copy = e.define_diagnostic("copy", [(1, None, 1.0)])
            print(f"N = {n}, axis of {T} rows, {a.runs} rounds (wall ms per call, synchronised)")
            for what, window, t_stride in CASES:
                name = f"mean{window}"
                vid = e.define_running_mean(name, TS, window, "centre")
                tb = running_mean_back(window, "centre")
                last = T - 1 - (window - 1 - tb)
                rows = min(R, (last - tb) // t_stride + 1)
                te = tb + (rows - 1) * t_stride + 1
                ms = timed(e, {"one term": lambda: e.compute_diagnostic(copy, tb, te, t_stride),
                               "running mean": lambda: e.compute_diagnostic(vid, tb, te, t_stride)}, a.runs)
                read, tile = rows_read(rows, window, t_stride, n)
                floor = 16.0 * rows * n
                base = statistics.median(ms["one term"])
                med = statistics.median(ms["running mean"])
                spread = max(max(x) - min(x) for x in ms.values()) / base
                print(f" {what}: {rows} output rows from {tb}; tile {tile} outputs, {-(-rows // tile)} tiles, "
                      f"overlap factor {read / (rows * t_stride) if t_stride < window else 1.0:.3f} (source rows read {read})")
                print(line("one term", ms["one term"], floor, "16 B x R x N over the median"))
                print(line("running mean", ms["running mean"], floor, "16 B x R x N over the median"))
                print(f"  {'':<13} counted bytes 8 B x N x ({read} + {rows}) over the median: {8.0 * n * (read + rows) / (med * 1e-3) / 1e9:7.0f} GB/s"
                      f"   ratio to one term {med / base:5.2f}   (largest max - min of the two, over the one-term median: {spread:.2f})")
                sys.stdout.flush()
            if not a.no_host:   # once, at 20 terms, last: the upload writes rows and every diagnostic goes stale
                window, tb = 20, running_mean_back(20, "centre")
                e.sync()
                t0 = time.perf_counter()
                src = e.get_series(TS, 0, R + window - 1)
                t1 = time.perf_counter()
                values, first = series_running_mean(src, window, "centre")
                t2 = time.perf_counter()
                for k in range(values.shape[0]):
                    e.set_state(2, first + k, values[k])
                e.sync()
                t3 = time.perf_counter()
                assert first == tb and values.shape[0] == R
                e.compute_diagnostic("mean20", tb, tb + R)
                got = e.get_series("mean20", tb, tb + R)
                same = bool(((got.view(np.uint64) == values.view(np.uint64)) | (np.isnan(got) & np.isnan(values))).all())
                print(f" host route, W = 20, {R} output rows, once: get_series {1e3 * (t1 - t0):9.1f} ms, numpy loop {1e3 * (t2 - t1):9.1f} ms, "
                      f"upload {1e3 * (t3 - t2):9.1f} ms, total {1e3 * (t3 - t0):9.1f} ms; equal to the device rows: {same}")
                sys.stdout.flush()


if __name__ == "__main__":
    main()
