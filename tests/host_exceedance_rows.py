"""The restatement of rscm_ens_exceedance_rows (the definition is stated in include/rscm_gpu.h) in numpy and Python integers: the
sums, what the finishers of rscm_amd.ensemble make of them, and the integer binning of the rank histogram.  Comparisons are numpy's
IEEE comparisons; every sum and every quotient is formed in Python integers and fractions, so nothing here rounds but the one
conversion of an exact quotient to a double."""
import math
from fractions import Fraction

import numpy as np


def row_values(X, baseline=None):
    """The values the thresholds are compared with: the rows, or with a baseline each member's row value minus it, one subtraction."""
    X = np.asarray(X, dtype=np.float64)
    if baseline is None:
        return X
    with np.errstate(invalid="ignore"):   # (an infinity minus an infinity is a NaN, which takes no part)
        return X - np.asarray(baseline, dtype=np.float64)[None, :]


def thresholds_of(thr, rows):
    """[rows][K] from [K] (the same for every row) or [rows][K]."""
    thr = np.asarray(thr, dtype=np.float64)
    return np.broadcast_to(thr, (rows, thr.shape[-1])) if thr.ndim == 1 else thr


def sums(X, thr, weights=None, groups=None, n_groups=None, baseline=None):
    """(hits[rows][G][K], equal[rows][G][K], total[rows][G]) as int64 arrays, summed in Python integers; G is 1 without groups."""
    x = row_values(X, baseline)
    R, n = x.shape
    th = thresholds_of(thr, R)
    K = th.shape[1]
    w = np.ones(n, dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    G = 1 if groups is None else int(n_groups)
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    hits, equal, total = (np.zeros(s, dtype=np.int64) for s in ((R, G, K), (R, G, K), (R, G)))
    with np.errstate(invalid="ignore"):
        for r in range(R):
            part = ~np.isnan(x[r])
            for j in range(G):
                m = part & (g == j)
                total[r, j] = sum(w[m].tolist())
                for k in range(K):
                    hits[r, j, k] = sum(w[m & (x[r] >= th[r, k])].tolist())
                    equal[r, j, k] = sum(w[m & (x[r] == th[r, k])].tolist())
    return hits, equal, total


def ratio(num, den):
    """num / den as float64 arrays of one shape, each the exact quotient rounded once (through Fraction); NaN where den is 0."""
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    out = [float(Fraction(a, b)) if b else math.nan for a, b in zip(num.ravel().tolist(), den.ravel().tolist())]
    return np.array(out, dtype=np.float64).reshape(num.shape)


def exceedance_rows(X, thr, weights=None, groups=None, n_groups=None, baseline=None):
    """What Ensemble.exceedance_rows returns (the group axis after the rows with groups, absent without)."""
    hits, _, total = sums(X, thr, weights, groups, n_groups, baseline)
    out = {"hits": hits, "total": total, "probability": ratio(hits, np.broadcast_to(total[..., None], hits.shape))}
    return out if groups is not None else {k: v[:, 0] for k, v in out.items()}


def rank_rows(X, record, weights=None, groups=None, n_groups=None, baseline=None):
    """What Ensemble.rank_rows returns for record[rows] (NaN: no observation in that row)."""
    record = np.asarray(record, dtype=np.float64)
    hits, equal, total = sums(X, record[:, None], weights, groups, n_groups, baseline)
    below, equal = total - hits[..., 0], equal[..., 0]
    pit = ratio(2 * below + equal, 2 * total)
    pit[np.isnan(record)] = np.nan
    out = {"below": below, "equal": equal, "total": total, "pit": pit}
    return out if groups is not None else {k: v[:, 0] for k, v in out.items()}


def rank_histogram(below, equal, total, n_bins, record=None):
    """int64 [n_bins] (or [G][n_bins]): the rows with a record and with weight, binned by floor(n_bins (2 below + equal) / (2 total))
    in Python integers, the top edge in the last bin."""
    below, equal, total = (np.asarray(a, dtype=np.int64) for a in (below, equal, total))
    grouped = below.ndim == 2
    b2, e2, t2 = (a.reshape(a.shape[0], -1) for a in (below, equal, total))
    out = np.zeros((b2.shape[1], n_bins), dtype=np.int64)
    for r in range(b2.shape[0]):
        if record is not None and math.isnan(float(record[r])):
            continue
        for g in range(b2.shape[1]):
            b, e, t = int(b2[r, g]), int(e2[r, g]), int(t2[r, g])
            if t == 0:
                continue
            k = (n_bins * (2 * b + e)) // (2 * t)
            out[g, n_bins - 1 if k >= n_bins else k] += 1
    return out if grouped else out[0]


def same(got, want):
    """Two result dicts: equal keys, shapes and dtypes kinds; integers equal, doubles bit for bit (any NaN for a NaN)."""
    if set(got) != set(want):
        return False
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or a.dtype.kind != b.dtype.kind:
            return False
        if a.dtype.kind == "f":
            if not (((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all()):
                return False
        elif not (a == b).all():
            return False
    return True
