"""Times the grouped select (Ensemble.quantile_rows(..., grouped=True), RSCM_SELECT_GROUPED) against its floor and against the
route it replaces.

Cases: a two-layer ensemble of 1e6 members x 751 rows with 3 contiguous groups (the posterior layout) and with 3 interleaved groups
(i % 3), and -- unless --no-graph -- one variable of the configs[3] share (the MAGICC graph at 125 000 members, 750 years monthly, a
96-row window and annual outputs: 751 resident rows) with 3 contiguous groups.  q = (0.05, 0.5, 0.95) throughout.  Per case, as
the median, minimum and maximum of --repeats synchronous calls after a warm-up:

  (a) the grouped select;
  (b) the ungrouped select over all members on the same rows: it moves the same bytes at least once per pass, so it is the floor;
  (c) the single-handle route without member groups: three weighted selects with the member weights masked to one group each
      (numpy's "inverted_cdf", not the plume's "linear"), the three weight uploads included.

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


def timed_ms(fn, repeats):
    fn()                                                    # warm-up: code objects, first allocations
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3)}


def measure(config, layout, ens, var, t_stride, repeats):
    """ens: the Ensemble holding `var`; its groups and weights are set here and cleared afterwards."""
    n = ens.n_members
    group = (np.arange(n) * G // n if layout == "contiguous" else np.arange(n) % G).astype(np.int32)
    masks = [(group == g).astype(np.int64) for g in range(G)]
    ens.set_member_groups(group, G)
    rows = len(range(0, ens.time_index + 1, t_stride))

    def masked():
        out = []
        for m in masks:
            ens.set_member_weights(m)
            out.append(ens.quantile_rows(var, Q, t_stride=t_stride, weighted=True)["quantiles"])
        return out

    a = timed_ms(lambda: ens.quantile_rows(var, Q, t_stride=t_stride, grouped=True), repeats)
    b = timed_ms(lambda: ens.quantile_rows(var, Q, t_stride=t_stride), repeats)
    c = timed_ms(masked, repeats)
    got = ens.quantile_rows(var, Q, t_stride=t_stride, grouped=True)
    res = {"config": config, "groups": f"{G} {layout}", "members": n, "rows": rows, "q": Q,
           "a_grouped_ms": a, "b_ungrouped_ms": b, "c_three_masked_weighted_ms": c,
           "a_over_b": round(a["median"] / b["median"], 3), "a_over_c": round(a["median"] / c["median"], 3),
           "c_spread_ms": round(c["max"] - c["min"], 3), "a_spread_ms": round(a["max"] - a["min"], 3),
           "members_counted": int(got["count"][:, rows - 1].sum()),
           "bytes_per_pass": rows * n * 8, "grouped_tb_per_s_over_8_passes": round(8 * rows * n * 8 / (a["median"] * 1e-3) / 1e12, 3)}
    print(json.dumps(res), flush=True)
    ens.clear_member_groups()
    return res


def two_layer(n, repeats):
    t = np.arange(1750, 2501, dtype=np.float64)
    with rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0)) as e:
        e.sample_lhs(20261017, [0.8, 0.0, 1.0, 0.5, 5.0, 50.0], [1.5, 0.1, 1.8, 1.0, 15.0, 200.0])
        e.set_forcing(4.0 * (1.0 - np.exp(-(t - 1750.0) / 120.0)) + 0.3 * np.sin(2.0 * np.pi * (t - 1750.0) / 11.0))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.run()
        return [measure("two-layer", layout, e, 1, 1, repeats) for layout in ("contiguous", "interleaved")]


def graph_share(n, years, repeats):
    from bench_magicc_chain import build_chain
    from rscm_amd import _lib as L
    model = build_chain(n, years, "topological", steps_per_year=12, series_window=96, output_stride=12)
    try:
        model.set_mode(L.MODE_FAST)
        model.run()
        ens, vid = model.variable_home("Atmospheric Concentration|CO2")
        return [measure("configs[3] share, Atmospheric Concentration|CO2", "contiguous", ens, vid, 12, repeats)]
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1_000_000)
    ap.add_argument("--graph-members", type=int, default=125_000)
    ap.add_argument("--graph-years", type=int, default=750)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    two_layer(args.members, args.repeats)
    if not args.no_graph:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        graph_share(args.graph_members, args.graph_years, args.repeats)


if __name__ == "__main__":
    main()
