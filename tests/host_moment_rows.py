"""Reference of the exact moments of stored rows (include/rscm_gpu.h, rscm_ens_moment_rows_sums), in Python integers and fractions,
built on tests/host_moments.py (``exact_sum``, ``block_of``, ``canonical``, ``finish``).

What is restated here is what the rows add to the vector moments: the value of a member in a row (``series[t][i]``, or one rounded
subtraction of the baseline), the PER-ROW counting rule (a member counts in a row when its value there and all its vector values
are finite and its group is valid), and the blocks in the order of the definition -- order 1: x, v_0 .. v_(K-1); order 2: xx,
x v_0 .. x v_(K-1), v_0 v_0 .. v_(K-1) v_(K-1), each term one IEEE product of two IEEE differences, formed in numpy float64."""
import numpy as np

from tests import host_moments as hm

MAX_VECTORS = 4


def row_values(rows, baseline=None):
    """x[R][N]: the rows, or with a baseline rows - baseline, one rounded subtraction each."""
    rows = np.asarray(rows, dtype=np.float64)
    if baseline is None:
        return rows
    with np.errstate(invalid="ignore", over="ignore"):
        return rows - np.asarray(baseline, dtype=np.float64)[None, :]


def counted(x_row, V, groups=None, n_groups=None):
    """[G] boolean masks of the members counted in ONE row, per group."""
    ok = np.isfinite(x_row)
    for v in V:
        ok = ok & np.isfinite(v)
    if groups is None:
        return [ok]
    groups = np.asarray(groups)
    return [ok & (groups == g) for g in range(n_groups)]


def _vectors(V, n):
    V = np.asarray(V, dtype=np.float64).reshape(-1, n)
    assert V.shape[0] <= MAX_VECTORS
    return V


def _terms(xg, Vg, order, c):
    """The member terms of every block of one (row, group), in the definition's order; c is the centre [1 + K]."""
    K = Vg.shape[0]
    if order == 1:
        return [xg] + [Vg[k] for k in range(K)]
    with np.errstate(over="ignore", invalid="ignore"):
        dx = xg - np.float64(c[0])
        dv = [Vg[k] - np.float64(c[1 + k]) for k in range(K)]
        return [dx * dx] + [dx * dv[k] for k in range(K)] + [dv[k] * dv[k] for k in range(K)]


def _walk(rows, order, V, center, weights, groups, n_groups, baseline, per_group):
    """Calls per_group(r, g, n, wg, terms or None) for every (row, group); terms None: a non-finite centre."""
    x = row_values(rows, baseline)
    R, N = x.shape
    V = _vectors(V, N)
    K = V.shape[0]
    w = np.array([1] * N if weights is None else [int(v) for v in np.asarray(weights).tolist()], dtype=object)
    G = 1 if groups is None else n_groups
    c_all = None if order == 1 else np.asarray(center, dtype=np.float64).reshape(R, G, 1 + K)
    for r in range(R):
        for g, ok in enumerate(counted(x[r], V, groups, n_groups)):
            idx = np.flatnonzero(ok)
            wg = w[idx].tolist()
            c = None if order == 1 else c_all[r, g]
            if order == 2 and not np.isfinite(c).all():
                per_group(r, g, int(idx.size), wg, None)
            else:
                per_group(r, g, int(idx.size), wg, _terms(x[r, idx], V[:, idx], order, c))
    return R, G, K


def sums(rows, order, V=(), center=None, weights=None, groups=None, n_groups=None, baseline=None):
    """[R][G] of (n, W, [(canonical value, count of non-finite terms) per block]) as Python ints."""
    K = _vectors(V, np.asarray(rows).shape[1]).shape[0]
    out = {}

    def per_group(r, g, n, wg, terms):
        blocks = [hm.exact_sum(t, wg) for t in terms] if terms is not None else [(0, n)] * (1 + 2 * K)
        out[(r, g)] = (n, int(sum(wg)), blocks)

    R, G, _ = _walk(rows, order, V, center, weights, groups, n_groups, baseline, per_group)
    return [[out[(r, g)] for g in range(G)] for r in range(R)]


def sums_array(rows, order, V=(), center=None, weights=None, groups=None, n_groups=None, baseline=None) -> np.ndarray:
    """What ``Ensemble.moment_rows_sums`` returns, formed by the limb scheme term by term: int64 [R][G][2 + B * 69]."""
    K = _vectors(V, np.asarray(rows).shape[1]).shape[0]
    B = 1 + K if order == 1 else 1 + 2 * K
    flat = {}

    def per_group(r, g, n, wg, terms):
        row = [n, int(sum(wg))]
        for b in range(B):
            row += hm.block_of(terms[b], wg) if terms is not None else [0] * hm.LIMBS + [n]
        flat[(r, g)] = row

    R, G, _ = _walk(rows, order, V, center, weights, groups, n_groups, baseline, per_group)
    return np.array([[flat[(r, g)] for g in range(G)] for r in range(R)], dtype=np.int64).reshape(R, G, 2 + B * hm.BLOCK)


def array_sums(arr, K, order):
    """An int64 array [R][G][2 + B * 69] (the device's, or a sum of several) in the form of ``sums``: blocks as canonical integers."""
    arr = np.asarray(arr)
    B = 1 + K if order == 1 else 1 + 2 * K
    assert arr.ndim == 3 and arr.shape[2] == 2 + B * hm.BLOCK, arr.shape
    return [hm.array_sums(arr[r], B, 1) for r in range(arr.shape[0])]   # B blocks a group, as B vectors of order 1 lay them out


def n_terms(rows, order, V=(), center=None, weights=None, groups=None, n_groups=None, baseline=None) -> int:
    """The finite non-zero terms over all rows, groups and blocks: what the kernel adds through its window or walks."""
    total = [0]

    def per_group(r, g, n, wg, terms):
        if terms is None:
            return
        nz = np.array([int(v) != 0 for v in wg], dtype=bool)
        for t in terms:
            t = np.asarray(t, dtype=np.float64)
            total[0] += int((np.isfinite(t) & (t != 0.0) & nz).sum())

    _walk(rows, order, V, center, weights, groups, n_groups, baseline, per_group)
    return total[0]


def means(s1):
    """center[R][G][1 + K] of the order-1 ``sums``."""
    return np.array([[[hm.finish(v, nb, W) for v, nb in blocks] for _, W, blocks in row] for row in s1], dtype=np.float64)


def moment_rows(rows, V=(), weights=None, groups=None, n_groups=None, baseline=None, with_sums=False):
    """The reference of ``Ensemble.moment_rows`` with the group axis kept ([R][G] ..., [R][G][K]): every mean, variance and
    covariance the exact sum over W rounded once; sd, corr and slope one IEEE operation each on those."""
    N = np.asarray(rows).shape[1]
    K = _vectors(V, N).shape[0]
    s1 = sums(rows, 1, V, None, weights, groups, n_groups, baseline)
    mean = means(s1)
    s2 = sums(rows, 2, V, mean, weights, groups, n_groups, baseline)
    second = np.array([[[hm.finish(v, nb, W) for v, nb in blocks] for _, W, blocks in row] for row in s2], dtype=np.float64)
    R, G = len(s1), len(s1[0]) if s1 else 1
    mean, second = mean.reshape(R, G, 1 + K), second.reshape(R, G, 1 + 2 * K)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = second[..., 0]
        out = {"count": np.array([[n for n, _, _ in row] for row in s1], dtype=np.int64).reshape(R, G),
               "weight": np.array([[W for _, W, _ in row] for row in s1], dtype=np.int64).reshape(R, G),
               "mean": mean[..., 0], "var": var, "sd": np.sqrt(var)}
        if K:
            cov, vec_var = second[..., 1:1 + K], second[..., 1 + K:]
            corr = np.empty_like(cov)
            for k in range(K):   # the rule of host_moments.corr_rules: cov_ab / (sd_a * sd_b)
                corr[..., k] = cov[..., k] / (np.sqrt(var) * np.sqrt(vec_var[..., k]))
            out.update({"vec_mean": mean[..., 1:], "vec_var": vec_var, "cov": cov, "corr": corr, "slope": cov / vec_var})
    return (out, s1, s2) if with_sums else out


def ungrouped(d):
    """The dict without its group axis (of length 1): the form ``Ensemble.moment_rows`` returns without ``grouped``."""
    return {k: v[:, 0] for k, v in d.items()}
