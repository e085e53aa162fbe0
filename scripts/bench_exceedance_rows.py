"""Times Ensemble.exceedance_rows and Ensemble.rank_rows (the exceedance and observation rank of a stored variable at every row,
csrc/exceedance_rows.hip) against the three calls that already read the same rows.

Shapes: two-layer ensembles of 1e6 members x 171 rows and 1e5 members x 751 rows of surface temperature after a run, fully
stored.  Variants: plain, weighted (random weights below 2^30), anomaly (baseline = the mean of the first 51 rows), three member
groups contiguous and interleaved (i % 3), K = 1, 3, 8 fixed thresholds, per-row thresholds (K = 3) and rank_rows (the row medians
as the record).  The yardsticks, over the same rows: Ensemble.indicators() with three thresholds, Ensemble.moment_rows with no
vectors, Ensemble.quantile_rows at three quantiles.

Every variant and every yardstick is timed as the median (with minimum and maximum) of --repeats synchronous calls after one
warm-up round, all in ONE alternation (v0, v1, ..., y0, y1, y2, v0, ...), so that they share whatever else the machine does.
Times are host clocks around calls that return after the device has finished.  The rows' bytes (members x rows x 8) over the
median time are given as a rate and as a share of the HBM peak of 8 TB/s; a variant re-reads 8 (weights), 4 (groups) or 8
(baseline) bytes per member and row besides, which the rate does not count.  One JSON line per timed call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402

Q = [0.05, 0.5, 0.95]
G = 3
HBM_PEAK = 8.0e12   # bytes per second


def alternate_ms(fns, repeats):
    for fn in fns:
        fn()                                                # warm-up: code objects, first allocations
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return [{"median": round(statistics.median(x), 3), "min": round(min(x), 3), "max": round(max(x), 3)} for x in out]


def ensemble(n, rows):
    t = np.arange(rows, dtype=np.float64) + 1750.0
    rng = np.random.default_rng(n)
    lo = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])[:, None]
    hi = np.array([1.5, 0.02, 1.8, 1.0, 15.0, 200.0])[:, None]   # (a weak state dependence: no member runs away in 750 years)
    e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0))
    e.set_params(lo + rng.random((6, n)) * (hi - lo))
    e.set_forcing(4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)) + 0.3 * np.sin(2 * np.pi * (t - 1750.0) / 11.0))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["1000000x171", "100000x751"])
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    for shape in args.shapes:
        n, rows = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(rows)
        with ensemble(n, rows) as e, ensemble(n, rows) as ec, ensemble(n, rows) as ei:
            for x in (e, ec, ei):
                x.set_member_weights(rng.integers(0, 1 << 30, n))
                x.set_baseline(1, 0, min(51, rows))
            ec.set_member_groups((np.arange(n) * G // n).astype(np.int32), G)
            ei.set_member_groups((np.arange(n) % G).astype(np.int32), G)
            median = e.quantile_rows(1, [0.5])["quantiles"][:, 0]
            thr8 = np.quantile(median, np.linspace(0.1, 0.9, 8))      # thresholds the plume crosses within the run
            table = np.ascontiguousarray(median[:, None] * np.array([0.8, 1.0, 1.2]))
            calls = [
                ("plain K=3", lambda: e.exceedance_rows(1, thr8[:3])),
                ("weighted K=3", lambda: e.exceedance_rows(1, thr8[:3], weighted=True)),
                ("anomaly K=3", lambda: e.exceedance_rows(1, thr8[:3], anomaly=True)),
                ("grouped contiguous K=3", lambda: ec.exceedance_rows(1, thr8[:3], grouped=True)),
                ("grouped interleaved K=3", lambda: ei.exceedance_rows(1, thr8[:3], grouped=True)),
                ("plain K=1", lambda: e.exceedance_rows(1, thr8[:1])),
                ("plain K=8", lambda: e.exceedance_rows(1, thr8)),
                ("weighted K=8", lambda: e.exceedance_rows(1, thr8, weighted=True)),
                ("per-row thresholds K=3", lambda: e.exceedance_rows(1, table)),
                ("rank_rows", lambda: e.rank_rows(1, median)),
                ("rank_rows weighted", lambda: e.rank_rows(1, median, weighted=True)),
                ("yardstick indicators() 3 thresholds", lambda: e.indicators(1, 0, rows, thresholds=thr8[:3])),
                ("yardstick moment_rows no vectors", lambda: e.moment_rows(1)),
                ("yardstick quantile_rows 3 quantiles", lambda: e.quantile_rows(1, Q)),
            ]
            times = alternate_ms([fn for _, fn in calls], args.repeats)
            row_bytes = n * rows * 8
            plain = e.exceedance_rows(1, thr8[:3])
            rank = e.rank_rows(1, median)
            for (name, _), t in zip(calls, times):
                rate = row_bytes / (t["median"] * 1e-3)
                print(json.dumps({"members": n, "rows": rows, "call": name, "ms": t, "rows_TB_per_s": round(rate / 1e12, 3),
                                  "share_of_hbm_peak": round(rate / HBM_PEAK, 3)}), flush=True)
            print(json.dumps({"members": n, "rows": rows, "check": "last row", "probability": plain["probability"][-1].tolist(),
                              "total": int(plain["total"][-1]), "pit_of_the_median": float(rank["pit"][-1])}), flush=True)


if __name__ == "__main__":
    main()
