"""Times Ensemble.moments (the exact weighted means, covariances and correlations across members, csrc/moments.hip) against the
host route it replaces and against a device statistic of the same inputs.

Cases: K = 1, 4, 8 parameter rows of a two-layer mix ensemble of 1e5 and 1e6 members; plain, weighted (random weights below 2^30),
and with three member groups, contiguous and interleaved (i % 3).  Per case, as the median, minimum and maximum of --repeats
synchronous calls taken in alternation (a, b, c, a, b, c, ...) after one warm-up round:

  (a) Ensemble.moments;
  (b) the host route: the K vectors copied device to host, then numpy.cov(aweights=...) and numpy.average (per group: on the
      group's members) -- f64 sums that are not exact and differ with the order;
  (c) Ensemble.quantile_vectors of the same vectors at q = (0.05, 0.5, 0.95): the radix select, eight passes over the same bytes.

Times are host clocks around calls that return after the device has finished.  One JSON line per case with a/b and a/c."""
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


def host_route(vecs, w, group):
    X = np.stack([v.to_host() for v in vecs])
    sets = [np.ones(X.shape[1], dtype=bool)] if group is None else [group == g for g in range(G)]
    out = []
    for m in sets:
        m = m & np.isfinite(X).all(axis=0)
        aw = None if w is None else w[m].astype(np.float64)
        out.append((np.average(X[:, m], axis=1, weights=aw), np.cov(X[:, m], aweights=aw, ddof=0)))
    return out


def measure(e, K, variant, w, group, repeats):
    vecs = [e.params_vector(k) for k in range(K)]
    weighted, grouped = variant == "weighted", variant.startswith("grouped")
    if grouped:
        e.set_member_groups(group, G)
    kw = dict(weighted=weighted, grouped=grouped)
    a, b, c = alternate_ms([lambda: e.moments(vecs, **kw), lambda: host_route(vecs, w if weighted else None, group if grouped else None),
                            lambda: e.quantile_vectors(vecs, Q, **kw)], repeats)
    got = e.moments(vecs, **kw)
    res = {"members": e.n_members, "K": K, "sums": K + K * (K + 1) // 2, "variant": variant, "a_moments_ms": a, "b_host_route_ms": b,
           "c_quantile_vectors_ms": c, "a_over_b": round(a["median"] / b["median"], 3), "a_over_c": round(a["median"] / c["median"], 3),
           "counted": int(np.sum(got["count"])), "corr_01": None if K < 2 else float(np.ravel(got["corr"][..., 0, 1])[0])}
    print(json.dumps(res), flush=True)
    if grouped:
        e.clear_member_groups()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--vectors", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    for n in args.members:
        rng = np.random.default_rng(n)
        P = rng.standard_normal((8, n)) * np.arange(1.0, 9.0)[:, None] + 3.0
        P[1] += 0.8 * P[0]
        w = rng.integers(0, 1 << 30, n)
        with rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, np.arange(1750.0, 1754.0), forcing_components=2) as e:
            e.set_params(P)
            e.set_member_weights(w)
            for K in args.vectors:
                for variant, group in (("plain", None), ("weighted", None), ("grouped contiguous", (np.arange(n) * G // n).astype(np.int32)),
                                       ("grouped interleaved", (np.arange(n) % G).astype(np.int32))):
                    measure(e, K, variant, w, group, args.repeats)


if __name__ == "__main__":
    main()
