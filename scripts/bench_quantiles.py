"""Plume statistics on the device (run on the GPU box): rscm_ens_summary (one row), rscm_ens_summary_series,
rscm_ens_quantile_series and rscm_ens_quantile_rows (both the radix select of csrc/select.hip) over all 751 rows of a
two-layer ensemble, against moving the series to the host and calling numpy.
Wall times of a call after a warm-up: median (min-max) over --repeats calls; the kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/bench_quantiles.py` run.

    python scripts/bench_quantiles.py [--sizes 100000,1000000] [--repeats 7] [--weighted]

--weighted also times the likelihood-weighted select (quantile_rows(weighted=True), csrc/select.hip) next to the unweighted
one: member weights quantised from a synthetic log-likelihood (set_weights_from_loglik), and numpy's weighted "inverted_cdf"
on the host at 1e5 members for the bits."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rscm_amd as ra  # noqa: E402
from tests.helpers import axis_values, f_syn, two_layer_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="100000,1000000", help="ensemble sizes, comma-separated")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--weighted", action="store_true")
args = ap.parse_args()


def timed(f):
    """(last result, 'median (min-max) ms') of args.repeats calls of f."""
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return r, f"{np.median(ms):.3f} ({min(ms):.3f}-{max(ms):.3f}) ms"


t = axis_values()
b = np.append(t, 2501.0)
q = [0.05, 0.17, 0.5, 0.83, 0.95]
for n in (int(s) for s in args.sizes.split(",")):
    with ra.Ensemble(ra.KIND_TWO_LAYER, n, b) as e:
        e.set_params(two_layer_params(n))
        e.set_forcing(f_syn(t))
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        e.run()
        e.summary(1, 8)
        e.summary_series(1, 0, 8)
        e.quantile_series(1, q, 0, 8)
        e.quantile_rows(1, q, 0, 8)
        _, t_one = timed(lambda: e.summary(1, 750))
        _, t_sum = timed(lambda: e.summary_series(1))
        g, t_q = timed(lambda: e.quantile_series(1, q))
        r, t_r = timed(lambda: e.quantile_rows(1, q))
        same = np.array_equal(r["quantiles"].view(np.uint64), g["quantiles"].view(np.uint64))
        line = (f"N={n}: summary (one row) {t_one}, summary_series (751 rows) {t_sum}, quantile_series (5 quantiles x 751 rows) {t_q}, "
                f"quantile_rows {t_r} (bit-equal: {same})")
        if n <= 100_000:
            t0 = time.perf_counter(); ts = e.get_series(1); t_copy = time.perf_counter() - t0
            t0 = time.perf_counter()
            with np.errstate(all="ignore"):
                w = np.nanquantile(ts, q, axis=1).T
            t_np = time.perf_counter() - t0
            line += f"; host: D2H {t_copy*1e3:.0f} ms + numpy.nanquantile {t_np*1e3:.0f} ms; same bits: {np.array_equal(w, g['quantiles'], equal_nan=True)}"
        print(line + f"; median warming in 2500: {g['quantiles'][-1][2]:.3f} K", flush=True)
        if args.weighted:
            ll = -0.5 * ((e.get_series(1, 250, 251)[0] - 1.0) / 0.3) ** 2     # fit to 1 K in 2000
            e.set_weights_from_loglik(ll)
            e.quantile_rows(1, q, 0, 8, weighted=True)
            r, t_r = timed(lambda: e.quantile_rows(1, q))
            wr, t_w = timed(lambda: e.quantile_rows(1, q, weighted=True))
            line = f"N={n}: weighted quantile_rows (5 quantiles x 751 rows) {t_w}, unweighted {t_r}; ESS {e.weights_ess():.0f}"
            if n <= 100_000:
                ts, w = e.get_series(1), e.member_weights()
                t0 = time.perf_counter()
                with np.errstate(all="ignore"):
                    nw = np.nanquantile(ts, q, axis=1, weights=np.broadcast_to(w, ts.shape), method="inverted_cdf").T
                t_np = time.perf_counter() - t0
                line += f"; host numpy weighted {t_np*1e3:.0f} ms; same bits: {np.array_equal(nw, wr['quantiles'])}"
            print(line + f"; constrained median warming in 2500: {wr['quantiles'][-1][2]:.3f} K", flush=True)
