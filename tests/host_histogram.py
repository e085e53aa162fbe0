"""The restatement of rscm_ens_histogram_rows, rscm_ens_histogram_vectors and rscm_ens_histogram2d (the definition is stated in
include/rscm_gpu.h) in numpy and Python integers: the bin of a value by the comparison definition, the sums, what the finishers of
rscm_amd.ensemble make of them, the CRPS bracket, and a brute-force exact CRPS that sorts in Fractions.

The definition.  Edges e[0] < e[1] < ... < e[E-1], finite, 2 <= E <= 1025, B = E - 1 bins.  For a value v that is not NaN let k be
the number of edges with e[j] <= v (IEEE comparisons: -0 equals +0, infinities take part).  k == 0: `below`.  1 <= k <= B: bin k - 1.
k == E: the last bin when v == e[E-1], else `above`.  A member takes part when its value is not NaN; its weight is 1 or w[i]; with
groups it counts in group g[i], ids outside [0, G) are left out; with a baseline the value is x - b[i], one rounded subtraction.
All sums are integers, so total = below + sum(counts) + above holds exactly.

Comparisons are numpy's IEEE comparisons; sums are int64 (no sum here comes near 2^63); every quotient is formed in Fractions and
rounded once."""
import math
from fractions import Fraction

import numpy as np

from tests.host_exceedance_rows import ratio, row_values, same  # noqa: F401  (same: how two result dicts are compared)


def slot_of(edges, v):
    """The slot of every value of v (not NaN) among B + 2 slots [bins 0 .. B-1, below = B, above = B + 1], by counting edges."""
    e = np.asarray(edges, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    B = e.size - 1
    k = (e[None, :] <= v[:, None]).sum(axis=1)
    return np.where(k == 0, B, np.where(k <= B, k - 1, np.where(v == e[B], B - 1, B + 1)))


def _members(n, weights, groups, n_groups):
    w = np.ones(n, dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    G = 1 if groups is None else int(n_groups)
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    return w, g, G


def sums(X, edges, weights=None, groups=None, n_groups=None, baseline=None):
    """(counts[rows][G][B], below[rows][G], above[rows][G], total[rows][G]) as int64; G is 1 without groups.  edges is [E], or
    [rows][E] with one table per row."""
    x = row_values(X, baseline)
    R, n = x.shape
    e = np.asarray(edges, dtype=np.float64)
    e = np.broadcast_to(e, (R, e.shape[-1]))
    B = e.shape[1] - 1
    w, g, G = _members(n, weights, groups, n_groups)
    acc = np.zeros((R, G, B + 2), dtype=np.int64)
    for r in range(R):
        m = ~np.isnan(x[r]) & (g >= 0) & (g < G)
        np.add.at(acc[r], (g[m], slot_of(e[r], x[r][m])), w[m])
    return acc[..., :B].copy(), acc[..., B].copy(), acc[..., B + 1].copy(), acc.sum(axis=2)


def sums2d(x, y, edges_x, edges_y, weights=None, groups=None, n_groups=None):
    """(counts[G][Bx][By], outside[G], total[G]) as int64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    Bx, By = len(edges_x) - 1, len(edges_y) - 1
    w, g, G = _members(x.size, weights, groups, n_groups)
    m = ~np.isnan(x) & ~np.isnan(y) & (g >= 0) & (g < G)
    sx, sy = slot_of(edges_x, x[m]), slot_of(edges_y, y[m])
    inside = (sx < Bx) & (sy < By)
    acc = np.zeros((G, Bx * By + 1), dtype=np.int64)
    np.add.at(acc, (g[m], np.where(inside, sx * By + sy, Bx * By)), w[m])
    return acc[:, :Bx * By].reshape(G, Bx, By).copy(), acc[:, Bx * By].copy(), acc.sum(axis=1)


def histogram_rows(X, edges, weights=None, groups=None, n_groups=None, baseline=None):
    """What Ensemble.histogram_rows and histogram_vectors return (the group axis after the rows with groups, absent without)."""
    counts, below, above, total = sums(X, edges, weights, groups, n_groups, baseline)
    out = {"counts": counts, "below": below, "above": above, "total": total,
           "probability": ratio(counts, np.broadcast_to(total[..., None], counts.shape))}
    return out if groups is not None else {k: v[:, 0] for k, v in out.items()}


def histogram2d(x, y, edges_x, edges_y, weights=None, groups=None, n_groups=None):
    """What Ensemble.histogram2d returns (the group axis leading with groups, absent without)."""
    counts, outside, total = sums2d(x, y, edges_x, edges_y, weights, groups, n_groups)
    out = {"counts": counts, "outside": outside, "total": total,
           "probability": ratio(counts, np.broadcast_to(total[:, None, None], counts.shape))}
    return out if groups is not None else {k: v[0] for k, v in out.items()}


def crps_bracket_fractions(counts, below, above, edges, y):
    """One row's (lower, upper) as Fractions, or None when the row is refused: weight outside the edges, no weight, a NaN record or a
    record outside [e[0], e[E-1]].  C_k is the weight below e[k]; inside bin k, C_k / T <= F <= C_{k+1} / T; the record's bin is
    split at y; left of y the score integrates F^2, right of it (1 - F)^2."""
    counts = [int(c) for c in counts]
    e = [Fraction(float(v)) for v in edges]
    T = sum(counts)
    if int(below) or int(above) or T == 0 or math.isnan(y) or not float(edges[0]) <= y <= float(edges[-1]):
        return None
    yf = Fraction(y)
    lo = hi = Fraction(0)
    C = 0
    for k, c in enumerate(counts):
        a, b = Fraction(C, T), Fraction(C + c, T)
        C += c
        pieces = []                                   # (width, left of y)
        if yf <= e[k]:
            pieces.append((e[k + 1] - e[k], False))
        elif yf >= e[k + 1]:
            pieces.append((e[k + 1] - e[k], True))
        else:
            pieces += [(yf - e[k], True), (e[k + 1] - yf, False)]
        for width, left in pieces:
            lo += width * (a * a if left else (1 - b) * (1 - b))
            hi += width * (b * b if left else (1 - a) * (1 - a))
    return lo, hi


def crps_bracket(hist, edges, record):
    """What rscm_amd.ensemble.crps_bracket returns for an ungrouped histogram dict: each bound rounded once, NaN for a refused row."""
    counts = np.asarray(hist["counts"])
    lower, upper = np.full(counts.shape[0], np.nan), np.full(counts.shape[0], np.nan)
    for r in range(counts.shape[0]):
        got = crps_bracket_fractions(counts[r], hist["below"][r], hist["above"][r], edges, float(record[r]))
        if got is not None:
            lower[r], upper[r] = float(got[0]), float(got[1])
    return {"lower": lower, "upper": upper}


def crps_exact(x, w, y):
    """The CRPS of the weighted empirical distribution of the values x (none NaN) with integer weights w against y, as a Fraction:
    the integral of (F(t) - [t >= y])^2 over t, piece by piece between the sorted values and y."""
    pts = sorted((Fraction(float(v)), int(k)) for v, k in zip(x, w))
    T = sum(k for _, k in pts)
    yf = Fraction(float(y))
    cuts = sorted({v for v, _ in pts} | {yf})
    total = Fraction(0)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        F = Fraction(sum(k for v, k in pts if v <= lo), T)      # constant on [lo, hi)
        d = F - (1 if lo >= yf else 0)
        total += (hi - lo) * d * d
    return total
