"""CPU tier: the numpy restatement of baselines, anomalies, indicators and exceedance (tests/host_indicators.py) against the
definitions written out member by member, on NaN and inf members, ties at the peak, thresholds never crossed and uneven shards;
and the product's host-side pieces: ``exceedance_result`` and the single-process paths of ``rscm_amd.distributed``."""
import math

import numpy as np
import pytest

from tests.helpers import same_values
from tests.host_indicators import anomaly, baseline, exceedance_counts, indicators

THR = (1.5, 2.0, 3.0)


def _rows():
    rng = np.random.default_rng(3)
    R, N = 40, 23
    x = np.cumsum(rng.normal(0.1, 0.2, (R, N)), axis=0)
    x[:, 0] = np.nan                       # NaN from the start
    x[17, 1] = np.nan                      # one NaN row
    x[5, 2] = np.inf                       # +inf: the peak, crossed everywhere from there
    x[:, 3] = -np.inf                      # all -inf: peak at the first row, never crossed
    x[:, 4] = 0.0
    x[[3, 9, 30], 5] = 7.0                 # tie at the peak: the first row wins
    x[:, 6] = -1.0                         # never crosses any threshold
    x[2, 7] = -0.0
    return x, 1850.0 + np.arange(R)


def _member(v, times, thr):
    """The definitions for one member, in plain Python."""
    if any(math.isnan(a) for a in v):
        return [math.nan] * (3 + len(thr))
    s = v[0]
    for a in v[1:]:
        s = s + a
    peak, pt = v[0], times[0]
    for a, t in zip(v, times):
        if a > peak:
            peak, pt = a, t
    cross = [next((t for a, t in zip(v, times) if a >= th), math.inf) for th in thr]
    return [s / len(v), peak, pt] + cross


@pytest.mark.parametrize("anom", [False, True])
def test_indicators_match_the_definitions(anom):
    x, times = _rows()
    b = baseline(x[:10]) if anom else None
    got = indicators(x, times, THR, base=b)
    vals = anomaly(x, b) if anom else x
    for i in range(x.shape[1]):
        want = _member([float(a) for a in vals[:, i]], list(times), THR)
        have = [got["mean"][i], got["peak"][i], got["peak_time"][i]] + [c[i] for c in got["crossing"]]
        assert same_values(np.array(have), np.array(want)), i
    if not anom:
        assert got["peak_time"][5] == times[3] and got["peak_time"][3] == times[0]
        assert all(c[6] == np.inf for c in got["crossing"]) and np.isnan(got["crossing"][0][0])
        assert got["crossing"][0][2] <= times[5]


def test_baseline_is_the_left_to_right_mean_and_nan_propagates():
    x, _ = _rows()
    b = baseline(x[:10])
    assert np.isnan(b[0]) and b[2] == np.inf and b[3] == -np.inf
    assert same_values(b, indicators(x[:10], np.arange(10.0))["mean"])   # mean over R_ref == baseline
    acc = x[0].copy()
    for r in x[1:10]:
        acc = acc + r
    assert same_values(b, acc / 10)
    assert np.isnan(baseline(x[15:20])[1]) and not np.isnan(baseline(x[:10])[1])
    a = anomaly(x, b)
    assert same_values(a, x - b)


def test_exceedance_counts_and_uneven_shards():
    rng = np.random.default_rng(8)
    n = 1001
    v = rng.normal(2.0, 1.0, n)
    v[rng.random(n) < 0.05] = np.nan
    v[:4] = [np.inf, -np.inf, 2.0, 1.5]
    w = rng.integers(0, 1 << 40, n, dtype=np.int64)
    for wt in (None, w):
        hits, total = exceedance_counts(v, THR, wt)
        ok = ~np.isnan(v)
        ww = np.ones(n, dtype=np.int64) if wt is None else wt
        assert total == int(ww[ok].sum())
        assert hits == [int(ww[ok & (v >= t)].sum()) for t in THR]
        cuts = [0, 1, 400, 401, 1001]                           # uneven shards, one of one member
        parts = [exceedance_counts(v[a:b_], THR, None if wt is None else wt[a:b_]) for a, b_ in zip(cuts[:-1], cuts[1:])]
        assert [sum(p[0][k] for p in parts) for k in range(len(THR))] == hits
        assert sum(p[1] for p in parts) == total


def test_exceedance_result_and_single_process_paths():
    from rscm_amd.distributed import exceedance_global, quantile_vectors_global
    from rscm_amd.ensemble import exceedance_result

    r = exceedance_result([3, 0, 5], 8)
    assert r["hits"].dtype == np.int64 and r["total"] == 8
    assert np.array_equal(r["probability"], np.array([3, 0, 5]) / 8.0)
    assert np.isnan(exceedance_result([0, 0], 0)["probability"]).all()

    class Stand:
        def exceedance(self, vector, thresholds, weighted=False):
            return exceedance_result(*exceedance_counts(vector, thresholds))

        def quantile_vectors(self, vectors, q, weighted=False):
            return {"count": np.array([len(v) for v in vectors]), "quantiles": np.array([np.nanquantile(v, q) for v in vectors])}

    v = np.array([1.0, 2.5, np.nan, 3.5])
    got = exceedance_global(Stand(), v, THR)
    assert got["hits"].tolist() == [2, 2, 1] and got["total"] == 3
    assert quantile_vectors_global(Stand(), [v[:2]], [0.5])["quantiles"][0][0] == 1.75
