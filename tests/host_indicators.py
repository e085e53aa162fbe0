"""Baselines, anomalies, per-member indicators and exceedance (rscm_amd/csrc/indicators.hip, the anomaly select of
select.hip) restated in numpy: the definitions of DESIGN.md section 8k, which the GPU tests compare the device against bit for bit
and the CPU rehearsal of rscm_amd.distributed (tests/_dist_indicator_worker.py) uses as its stand-in ensemble's arithmetic."""
import numpy as np


def baseline(rows) -> np.ndarray:
    """b[i]: the sum of member i's values over the rows in row order (f64, left to right) divided by the row count."""
    rows = np.asarray(rows, dtype=np.float64)
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = acc + r
    return acc / len(rows)


def anomaly(rows, b) -> np.ndarray:
    """a_i(t) = x_i(t) - b_i, one IEEE subtraction per value."""
    return np.asarray(rows, dtype=np.float64) - np.asarray(b, dtype=np.float64)[None, :]


def indicators(rows, times, thresholds=(), base=None):
    """{"mean", "peak", "peak_time", "crossing": [k]} per member over ``rows`` ([R][N]) at ``times`` ([R]), of the values or
    (``base``) of their anomalies.  A member with a NaN in any row has NaN in every indicator."""
    v = np.asarray(rows, dtype=np.float64) if base is None else anomaly(rows, base)
    times = np.asarray(times, dtype=np.float64)
    n = v.shape[1]
    nan = np.isnan(v).any(axis=0)
    idx = np.argmax(np.where(np.isnan(v), -np.inf, v), axis=0)
    out = {"mean": baseline(v), "peak": v[idx, np.arange(n)], "peak_time": times[idx], "crossing": []}
    for thr in np.atleast_1d(np.asarray(thresholds, dtype=np.float64)):
        hit = v >= thr
        out["crossing"].append(np.where(hit.any(axis=0), times[np.argmax(hit, axis=0)], np.inf))
    for k in ("mean", "peak", "peak_time"):
        out[k] = np.where(nan, np.nan, out[k])
    out["crossing"] = [np.where(nan, np.nan, c) for c in out["crossing"]]
    return out


def exceedance_counts(v, thresholds, w=None):
    """(hits [k], total) as Python ints: members (or their summed int64 weights) of the non-NaN ones with v >= thresholds[k]."""
    v = np.asarray(v, dtype=np.float64)
    ok = ~np.isnan(v)
    wt = np.ones(v.shape, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    hits = [int(wt[ok & (v >= t)].sum()) for t in np.atleast_1d(np.asarray(thresholds, dtype=np.float64))]
    return hits, int(wt[ok].sum())
