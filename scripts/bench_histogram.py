"""Times Ensemble.histogram_rows (the histogram of a stored variable at every row, csrc/histogram.hip) against the route that existed
before it: ceil(E / 8) calls of Ensemble.exceedance_rows, eight edges at a time as thresholds, over the same rows.

Shapes: two-layer ensembles of 1e6 members x 171 rows and 1e5 members x 751 rows of surface temperature after a run under a
Latin-hypercube parameter box, fully stored.  Edges: E = 17, 65, 257, 1025, of two kinds --
  spread:        equally spaced from the smallest to the largest value of the whole series, so a row's plume covers a run of bins;
  concentrated:  one bin in the middle holds every value of every row and the other edges lie outside the data, so every lane of
                 every wave adds to one slot (the search over the edges still takes its full depth).
Variants: plain, weighted (random weights below 2^30) and three interleaved member groups (i % 3), each beside its yardstick, the
exceedance_rows route with the same flags (the last call of a route takes the edges that are left, fewer than eight).  Further
yardsticks over the same rows: Ensemble.indicators() with three thresholds.  At 1e6 members also Ensemble.histogram2d at 50 x 50 bins
and Ensemble.histogram_vectors of the six parameter rows (65 edges each, per vector), each against copying the vectors to the host
and numpy.histogram2d / numpy.histogram there.

Every variant and every yardstick is timed as the median (with minimum and maximum) of --repeats synchronous calls after one
warm-up round, all in ONE alternation (c0, c1, ..., c0, ...), so that they share whatever else the machine does.  Times are host
clocks around calls that return after the device has finished.  One JSON line per timed call; a histogram line carries the ratio
of its yardstick's median to its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402

G = 3
EDGE_COUNTS = (17, 65, 257, 1025)
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


def latin_hypercube(rng, lo, hi, n):
    """[P][n]: every parameter's range cut into n strata, one member per stratum, the strata shuffled per parameter."""
    u = (np.stack([rng.permutation(n) for _ in range(len(lo))]) + rng.random((len(lo), n))) / n
    return lo[:, None] + u * (hi - lo)[:, None]


def ensemble(n, rows):
    t = np.arange(rows, dtype=np.float64) + 1750.0
    lo = np.array([0.8, 0.0, 1.0, 0.5, 5.0, 50.0])
    hi = np.array([1.5, 0.02, 1.8, 1.0, 15.0, 200.0])       # (a weak state dependence: no member runs away in 750 years)
    e = rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0))
    e.set_params(latin_hypercube(np.random.default_rng(n), lo, hi, n))
    e.set_forcing(4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)) + 0.3 * np.sin(2 * np.pi * (t - 1750.0) / 11.0))
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run()
    return e


def edges_of(kind, E, lo, hi):
    if kind == "spread":
        return np.linspace(lo, hi, E)
    span, k = hi - lo, (E - 1) // 2                         # the bin [e[k], e[k+1]) holds [lo, hi]
    lower = lo - 0.5 * span - span * np.arange(k, -1, -1)   # k + 1 edges, the last of them half a span below the data
    upper = hi + 0.5 * span + span * np.arange(E - k - 1)   # E - k - 1 edges, the first of them half a span above
    return np.concatenate([lower, upper])


def exceedance_route(e, edges, **kw):
    """The distribution through exceedance_rows: eight edges at a time."""
    return [e.exceedance_rows(1, edges[k:k + 8], **kw) for k in range(0, len(edges), 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["1000000x171", "100000x751"])
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    for shape in args.shapes:
        n, rows = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(rows)
        with ensemble(n, rows) as e:
            e.set_member_weights(rng.integers(0, 1 << 30, n))
            e.set_member_groups((np.arange(n) % G).astype(np.int32), G)
            q = e.quantile_rows(1, [0.0, 1.0])["quantiles"]
            lo, hi = float(q[:, 0].min()), float(q[:, 1].max())
            variants = (("plain", {}), ("weighted", {"weighted": True}), ("grouped interleaved", {"grouped": True}))
            calls = []
            for kind in ("spread", "concentrated"):
                for E in EDGE_COUNTS:
                    ed = edges_of(kind, E, lo, hi)
                    for name, kw in variants:
                        calls.append((kind, E, name, "histogram_rows", lambda ed=ed, kw=kw: e.histogram_rows(1, ed, **kw)))
                        calls.append((kind, E, name, "exceedance_rows route", lambda ed=ed, kw=kw: exceedance_route(e, ed, **kw)))
            thr3 = np.linspace(lo, hi, 5)[1:4]
            calls.append(("", 0, "", "yardstick indicators() 3 thresholds", lambda: e.indicators(1, 0, rows, thresholds=thr3)))
            calls.append(("", 0, "", "yardstick exceedance_rows K=8, one call", lambda: e.exceedance_rows(1, np.linspace(lo, hi, 8))))
            if n >= 1000000:
                vecs = [e.params_vector(k) for k in range(6)]
                P = e.get_params()
                own = np.stack([np.linspace(P[k].min(), P[k].max(), 65) for k in range(6)])
                ex, ey = np.linspace(P[0].min(), P[0].max(), 51), np.linspace(P[3].min(), P[3].max(), 51)
                calls.append(("", 65, "6 vectors", "histogram_vectors", lambda: e.histogram_vectors(vecs, own)))
                calls.append(("", 65, "6 vectors", "yardstick to_host + numpy.histogram",
                              lambda: [np.histogram(v.to_host(), bins=own[k]) for k, v in enumerate(vecs)]))
                calls.append(("", 51, "50 x 50", "histogram2d", lambda: e.histogram2d(vecs[0], vecs[3], ex, ey)))
                calls.append(("", 51, "50 x 50", "yardstick to_host + numpy.histogram2d",
                              lambda: np.histogram2d(vecs[0].to_host(), vecs[3].to_host(), bins=(ex, ey))))
            times = alternate_ms([c[4] for c in calls], args.repeats)
            row_bytes = n * rows * 8
            by_key = {c[:4]: t for c, t in zip(calls, times)}
            for (kind, E, name, call, _), t in zip(calls, times):
                line = {"members": n, "rows": rows, "call": call, "edges": E, "kind": kind, "variant": name, "ms": t}
                if call in ("histogram_rows", "exceedance_rows route"):
                    rate = row_bytes / (t["median"] * 1e-3)
                    line["rows_TB_per_s"] = round(rate / 1e12, 3)
                    line["share_of_hbm_peak"] = round(rate / HBM_PEAK, 3)
                if call == "histogram_rows":
                    line["route_over_histogram"] = round(by_key[(kind, E, name, "exceedance_rows route")]["median"] / t["median"], 2)
                print(json.dumps(line), flush=True)
            # the two routes say the same: for every edge but the last, the weight at or above it
            ed = edges_of("spread", 17, lo, hi)
            h = e.histogram_rows(1, ed)
            at_or_above = np.cumsum(h["counts"][:, ::-1], axis=1)[:, ::-1] + h["above"][:, None]
            hits = np.concatenate([r["hits"] for r in exceedance_route(e, ed[:16])], axis=1)
            one = e.histogram_rows(1, edges_of("concentrated", 17, lo, hi))
            print(json.dumps({"members": n, "rows": rows, "check": "the routes agree", "equal": bool((hits == at_or_above).all()),
                              "bins_filled_last_row_spread": int((h["counts"][-1] > 0).sum()),
                              "bins_filled_concentrated": int((one["counts"] > 0).any(axis=0).sum()),
                              "outside_concentrated": int(one["below"].sum() + one["above"].sum())}), flush=True)


if __name__ == "__main__":
    main()
