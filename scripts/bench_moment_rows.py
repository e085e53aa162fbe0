"""Times Ensemble.moment_rows (the exact weighted mean and spread of a stored variable at every row, csrc/moment_rows.hip) against
the route a user had before it and against the quantiles of the same rows.

Shapes: two-layer ensembles of 1e5 members x 751 rows and 1e6 members x 171 rows, fully stored.  Modes: plain, weighted (random
weights below 2^30), anomaly (baseline = the mean of the first 51 rows), three member groups contiguous and interleaved (i % 3),
and K = 2 member vectors (two parameter rows); and the all-walk case, every row overwritten by an ill-conditioned one (1e150, 1,
1e-300, subnormals and zeros mixed inside every tile: fifteen of sixteen terms of order 1 walk; the squares about the mean are all
of the mean's size and stay inside the window, as they do for any row).  Per case, as the median, minimum and maximum of --repeats synchronous
calls taken in alternation (a, b, c, a, b, c, ...) after one warm-up round:

  (a) Ensemble.moment_rows over all rows: two launches;
  (b) the per-row loop of Ensemble.moments([row]) (with K = 2: [row, v0, v1]) over the same rows, each row a DeviceVector into the
      stored series -- the route that existed; it has no anomaly, so the anomaly mode times it on the plain rows;
  (c) Ensemble.quantile_rows at q = (0.05, 0.5, 0.95) over the same rows.

Times are host clocks around calls that return after the device has finished.  One JSON line per case with a/b and a/c, whether
(a) beats (b) by more than the min-max spread of the two, and the path counts of (a)'s two launches."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd  # noqa: E402
from rscm_amd.ensemble import DeviceVector  # noqa: E402

Q = [0.05, 0.5, 0.95]
G = 3


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


def last_stats(e):
    out = (C.c_int64 * 3)()
    e._lib.rscm_gpu_moment_rows_last_stats(out)
    return list(out)


def measure(e, mode, K, repeats, group=None):
    n, rows = e.n_members, e.n_times
    vecs = [e.params_vector(k) for k in range(K)]
    kw = dict(weighted=mode == "weighted", anomaly=mode == "anomaly", grouped=group is not None)
    kw_b = dict(weighted=kw["weighted"], grouped=kw["grouped"])
    if group is not None:
        e.set_member_groups(group, G)
    base = e.series_devptr(1)
    row_vecs = [DeviceVector(base + 8 * n * t, n, np.float64, e) for t in range(rows)]

    def loop():
        return [e.moments([r] + vecs, **kw_b) for r in row_vecs]

    a, b, c = alternate_ms([lambda: e.moment_rows(1, vectors=vecs, **kw), loop, lambda: e.quantile_rows(1, Q, **kw)], repeats)
    e.moment_rows_sums(1, 1, vectors=vecs, **kw)
    stats1 = last_stats(e)
    got = e.moment_rows(1, vectors=vecs, **kw)
    stats2 = last_stats(e)
    if mode != "anomaly":   # the two routes agree bit for bit
        ref = loop()
        mean = np.array([np.ravel(m["mean"][..., 0]) for m in ref]).reshape(np.shape(got["mean"]))
        assert np.array_equal(mean, got["mean"], equal_nan=True)
    res = {"members": n, "rows": rows, "mode": mode, "K": K, "a_moment_rows_ms": a, "b_moments_loop_ms": b, "c_quantile_rows_ms": c,
           "a_over_b": round(a["median"] / b["median"], 4), "a_over_c": round(a["median"] / c["median"], 3),
           "a_beats_b_beyond_spread": a["max"] < b["min"], "order1_window_walked_rebases": stats1, "order2_window_walked_rebases": stats2,
           "mean_last": float(np.ravel(got["mean"])[-1])}
    print(json.dumps(res), flush=True)
    if group is not None:
        e.clear_member_groups()
    return res


def ill_conditioned(rng, n):
    """Every tile of 64 holds 1e150-sized values beside 1, 1e-300, subnormals and zeros: the window sits at the top, the rest walks."""
    x = rng.choice([1.0, 1e-300, 5e-324, 3e-310, 0.0, 1.0, 1e-300], n) * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    x[::16] = 1e150 * rng.uniform(1.0, 1.7, x[::16].size)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["100000x751", "1000000x171"])
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    for shape in args.shapes:
        n, rows = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(rows)
        with ensemble(n, rows) as e:
            e.set_member_weights(rng.integers(0, 1 << 30, n))
            e.set_baseline(1, 0, min(51, rows))
            measure(e, "plain", 0, args.repeats)
            measure(e, "weighted", 0, args.repeats)
            measure(e, "anomaly", 0, args.repeats)
            measure(e, "grouped contiguous", 0, args.repeats, (np.arange(n) * G // n).astype(np.int32))
            measure(e, "grouped interleaved", 0, args.repeats, (np.arange(n) % G).astype(np.int32))
            measure(e, "plain", 2, args.repeats)
            x = ill_conditioned(rng, n)
            for t in range(rows):
                e.set_state(1, t, x)
            measure(e, "all-walk", 0, args.repeats)


if __name__ == "__main__":
    main()
