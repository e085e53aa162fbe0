"""A probabilistic warming assessment on the device: BASELINE.json configs[3]'s share (the windowed MAGICC graph of
scripts/run_configs3_share.py, annual rows of every variable in the output store), then

  * the 5-95 % plume of surface-temperature ANOMALIES relative to 1850-1900 (each member's own anomaly), unweighted and weighted
    by a fit to a historical record;
  * per-member indicators -- peak warming and its year, mean 2081-2100 warming, the first years 1.5 / 2 / 3 K are crossed --
    and their quantiles, unweighted and weighted;
  * exceedance probabilities P(peak >= 1.5 / 2 / 3 K), unweighted and weighted;

each timed after a warm-up call, and all compared with numpy on the rows copied to the host (tests/host_indicators.py).

    python scripts/assess_plume.py [--members 125000] [--years 750] [--exact]
    python scripts/assess_plume.py --bench [--sizes 100000,1000000]     # two-layer N x 751 rows: plain vs anomaly select, indicators

Prints one JSON line; exit code 0 iff every comparison holds."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.run_configs3_share import HIST_YEARS, OBS_SIGMA, build  # noqa: E402
from tests.host_indicators import anomaly, baseline, exceedance_counts, indicators  # noqa: E402

Q = [0.05, 0.17, 0.5, 0.83, 0.95]
THR = [1.5, 2.0, 3.0]
NAME = "Surface Temperature"


def _timed(fn, reps=1):
    fn()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best * 1e3


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ua = np.where((a == 0) | np.isnan(a), 0.0, a)
    ub = np.where((b == 0) | np.isnan(b), 0.0, b)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(ua.view(np.uint64), ub.view(np.uint64)))


def _np_q(rows, w=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        rows = np.asarray(rows)
        if w is None:
            return np.nanquantile(rows, Q, axis=1).T
        live = ((~np.isnan(rows)) * w[None, :]).sum(axis=1) > 0
        out = np.full((rows.shape[0], len(Q)), np.nan)
        out[live] = np.nanquantile(rows[live], Q, axis=1, weights=np.broadcast_to(w, rows[live].shape), method="inverted_cdf").T
        return out


def assess(members, years, exact, window):
    model = build(members, years, exact, window)
    model.run()
    ens, _vid = model.variable_home(NAME)
    year = lambda y: (y - 1750) * 12  # noqa: E731  (annual rows: every 12th monthly row)
    last = ens.n_times
    ref = (year(1850), year(1900) + 1, 12)
    late = (year(2081), year(2100) + 1, 12)
    peak_rows = (year(1850), last, 12)
    # weights from each member's fit to a historical record (member 0's run as the stand-in record, as run_configs3_share.py)
    ser = model.get_series(NAME, t_stride=12)
    hist = ser[HIST_YEARS[0] - 1750:HIST_YEARS[1] - 1750 + 1]
    with np.errstate(all="ignore"):
        ll = -0.5 * (((hist - hist[:, :1]) / OBS_SIGMA) ** 2).sum(axis=0)
    model.set_weights_from_loglik(ll)
    w = ens.member_weights()

    dev = {}
    t_all = time.perf_counter()
    _, dev["set_baseline_ms"] = _timed(lambda: model.set_baseline(NAME, *ref))
    plume, dev["anomaly_plume_ms"] = _timed(lambda: model.quantile_rows(NAME, Q, t_stride=12, anomaly=True))
    wplume, dev["weighted_anomaly_plume_ms"] = _timed(lambda: model.quantile_rows(NAME, Q, t_stride=12, weighted=True, anomaly=True))
    pk, dev["indicators_peak_ms"] = _timed(lambda: model.indicators(NAME, *peak_rows, thresholds=THR, anomaly=True, slot=0))
    lt, dev["indicators_2081_2100_ms"] = _timed(lambda: model.indicators(NAME, *late, anomaly=True, slot=1))
    vecs = [pk["peak"], pk["peak_time"], lt["mean"]] + pk["crossing"]
    vq, dev["indicator_quantiles_ms"] = _timed(lambda: model.quantile_vectors(vecs, Q))
    wvq, dev["weighted_indicator_quantiles_ms"] = _timed(lambda: model.quantile_vectors(vecs, Q, weighted=True))
    ex, dev["exceedance_ms"] = _timed(lambda: model.exceedance(pk["peak"], THR))
    wex, dev["weighted_exceedance_ms"] = _timed(lambda: model.exceedance(pk["peak"], THR, weighted=True))
    dev["total_wall_ms_with_warmups"] = (time.perf_counter() - t_all) * 1e3
    dev["total_ms"] = sum(v for k, v in dev.items() if k.endswith("_ms") and k != "total_wall_ms_with_warmups")

    host = {}
    t0 = time.perf_counter()
    ser = model.get_series(NAME, t_stride=12)
    host["copy_ms"] = (time.perf_counter() - t0) * 1e3
    times = ens.bounds[:ens.n_times][::12]
    t0 = time.perf_counter()
    b = baseline(ser[100:151])
    a = anomaly(ser, b)
    want_plume, want_wplume = _np_q(a), _np_q(a, w)
    ind_pk = indicators(ser[100:], times[100:], THR, b)
    ind_lt = indicators(ser[331:351], times[331:351], (), b)
    hv = np.stack([ind_pk["peak"], ind_pk["peak_time"], ind_lt["mean"]] + ind_pk["crossing"])
    want_vq, want_wvq = _np_q(hv), _np_q(hv, w)
    want_ex, want_wex = exceedance_counts(hv[0], THR), exceedance_counts(hv[0], THR, w)
    host["numpy_ms"] = (time.perf_counter() - t0) * 1e3
    checks = {"baseline": bool(np.array_equal(model.baseline(NAME), b, equal_nan=True)),
              "anomaly_plume": _same(plume["quantiles"], want_plume), "weighted_anomaly_plume": _same(wplume["quantiles"], want_wplume),
              "indicators": all(_same(v.to_host(), h) for v, h in zip(vecs, hv)),
              "indicator_quantiles": _same(vq["quantiles"], want_vq), "weighted_indicator_quantiles": _same(wvq["quantiles"], want_wvq),
              "exceedance": [ex["hits"].tolist(), ex["total"]] == [want_ex[0], want_ex[1]],
              "weighted_exceedance": [wex["hits"].tolist(), wex["total"]] == [want_wex[0], want_wex[1]]}
    model.close()
    rows = ["peak_K", "peak_year", "mean_2081_2100_K"] + [f"crossing_{t}K_year" for t in THR]
    return {"members": members, "years": years, "quantiles": Q, "device": dev, "host": host, "checks": checks,
            "anomaly_plume_2100_K": plume["quantiles"][350].tolist(), "weighted_anomaly_plume_2100_K": wplume["quantiles"][350].tolist(),
            "indicator_quantiles": dict(zip(rows, vq["quantiles"].tolist())),
            "weighted_indicator_quantiles": dict(zip(rows, wvq["quantiles"].tolist())),
            "p_peak_at_least": dict(zip([str(t) for t in THR], ex["probability"].tolist())),
            "weighted_p_peak_at_least": dict(zip([str(t) for t in THR], wex["probability"].tolist()))}


def bench(sizes, reps):
    """Two-layer ensembles of N members x 751 rows: the plain and the anomaly select (5 quantiles, all rows) and the indicator
    kernel over all rows (wall time of the synchronous calls; kernel times: rocprofv3 --kernel-trace --stats)."""
    import rscm_amd
    from tests.helpers import axis_values, f_syn, two_layer_params
    out = []
    t = axis_values()
    for n in sizes:
        with rscm_amd.Ensemble(rscm_amd.KIND_TWO_LAYER, n, np.append(t, t[-1] + 1.0)) as e:
            e.set_params(two_layer_params(n))
            e.set_forcing(f_syn(t))
            e.set_initial(1, 0.0)
            e.set_initial(2, 0.0)
            e.run()
            e.set_baseline(1, 100, 151)
            _, plain = _timed(lambda: e.quantile_rows(1, Q), reps)
            _, anom = _timed(lambda: e.quantile_rows(1, Q, anomaly=True), reps)
            _, ind = _timed(lambda: e.indicators(1, 0, e.n_times, 1, THR, anomaly=True), reps)
            gb = n * e.n_times * 8 / 1e9
            out.append({"members": n, "rows": e.n_times, "select_ms": plain, "anomaly_select_ms": anom, "anomaly_over_plain": anom / plain,
                        "indicators_ms": ind, "indicators_row_read_tb_s": gb / ind})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=125_000)
    ap.add_argument("--years", type=int, default=750)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--bench", action="store_true", help="time the kernels on two-layer ensembles instead")
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.bench:
        print(json.dumps({"bench": bench([int(s) for s in args.sizes.split(",")], args.reps)}), flush=True)
        return
    res = assess(args.members, args.years, args.exact, args.window)
    print(json.dumps(res), flush=True)
    sys.exit(0 if all(res["checks"].values()) else 1)


if __name__ == "__main__":
    main()
