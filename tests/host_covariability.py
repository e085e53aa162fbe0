"""The per-member covariability of two variables (rscm_amd/csrc/covariability.hip; the definition stated in include/rscm_gpu.h under
rscm_ens_member_covariability) restated in numpy over two ``[R][N]`` blocks of rows: row loops, every operation one float64
operation rounded on its own, sums left to right from their first term.  The GPU tests compare the device against this bit for
bit, the CPU tests ``rscm_amd.variability.series_covariability``.  No product code."""
import numpy as np

from tests.host_variability import DIFFERENCE, LINEAR, MODES, working_series

MAX_LAGS = 3
NAMES = ("var_x", "var_y", "cov", "corr", "slope")


def pair_series(rows, mode, other):
    """u [n][N] of one variable under its own ``mode`` when the other variable's mode is ``other``: host_variability's working
    series, except that next to a differenced partner a variable that is not differenced itself is taken at the midpoints."""
    rows = np.asarray(rows, dtype=np.float64)
    if mode != DIFFERENCE and other == DIFFERENCE:
        return np.stack([(rows[k] + rows[k + 1]) * np.float64(0.5) for k in range(len(rows) - 1)]) if len(rows) > 1 else rows[:0]
    return working_series(rows, mode)


def residuals(u, mode):
    """[a_0 .. a_{n-1}] of the working series u under ``mode``: the residual steps of host_variability.variability."""
    n = len(u)
    h = np.float64(n - 1) * np.float64(0.5)
    tau = [np.float64(k) - h for k in range(n)]
    S = u[0]
    for k in range(1, n):
        S = S + u[k]
    m = S / np.float64(n)
    if mode == LINEAR:
        Q = tau[0] * u[0]
        for k in range(1, n):
            Q = Q + tau[k] * u[k]
        b = Q / (np.float64(n * (n * n - 1)) / np.float64(12.0))
    a = []
    for k in range(n):
        ak = u[k] - m
        if mode == LINEAR:
            ak = ak - b * tau[k]
        a.append(ak)
    return a


def lagged(a, c, l, fused=False):
    """G_l = a_0 c_l + a_1 c_{l+1} + ... (l >= 0, x leads) or G_{-m} = a_m c_0 + a_{m+1} c_1 + ... (l = -m < 0), left to right.
    ``fused``: as a compiler that contracts a*b + c into one fused multiply-add would form it (exact product, one rounding; the
    exact product in Python fractions) -- not the definition: what the comparison must be able to tell apart from it."""
    n = len(a)
    pairs = [(a[k], c[k + l]) for k in range(max(0, -l), n - max(0, l))]
    acc = pairs[0][0] * pairs[0][1]
    for p, q in pairs[1:]:
        acc = _fma(p, q, acc) if fused else acc + p * q
    return acc


def _fma(p, q, acc):
    from fractions import Fraction
    out = np.empty_like(acc)
    for i in range(len(acc)):
        out[i] = float(Fraction(float(p[i])) * Fraction(float(q[i])) + Fraction(float(acc[i])))    # float(Fraction) rounds to nearest even, once
    return out


def covariability(rows_x, rows_y, detrend_x, detrend_y, lags=0, fused=False):
    """{"var_x", "var_y", "cov", "corr", "slope": [N]; "lead", "lag": lists of ``lags`` [N]} of the rows [R][N] of two variables;
    NaN everywhere for a member with a non-finite value in a row of either."""
    mx, my = MODES[detrend_x], MODES[detrend_y]
    rows_x, rows_y = np.asarray(rows_x, dtype=np.float64), np.asarray(rows_y, dtype=np.float64)
    assert rows_x.ndim == 2 and rows_x.shape == rows_y.shape
    if not 0 <= lags <= MAX_LAGS:
        raise ValueError(f"{lags} lags: 0 to {MAX_LAGS}")
    with np.errstate(all="ignore"):
        u, v = pair_series(rows_x, mx, my), pair_series(rows_y, my, mx)
        n = len(u)
        assert len(v) == n
        if n < 3 + lags:
            raise ValueError(f"{n} terms: at least {3 + lags} are needed at {lags} lags")
        a, c = residuals(u, mx), residuals(v, my)
        Cxx, Cyy, G0 = lagged(a, a, 0, fused), lagged(c, c, 0, fused), lagged(a, c, 0, fused)
        D = np.sqrt(Cxx) * np.sqrt(Cyy)
        dn = np.float64(n)
        out = {"var_x": Cxx / dn, "var_y": Cyy / dn, "cov": G0 / dn, "corr": G0 / D, "slope": G0 / Cxx,
               "lead": [lagged(a, c, l, fused) / D for l in range(1, lags + 1)],
               "lag": [lagged(a, c, -l, fused) / D for l in range(1, lags + 1)]}
    bad = ~(np.isfinite(rows_x).all(axis=0) & np.isfinite(rows_y).all(axis=0))
    return {k: [np.where(bad, np.nan, w) for w in val] if isinstance(val, list) else np.where(bad, np.nan, val) for k, val in out.items()}


def flat(d):
    """The vectors of a result in the order of the C boundary's output: var_x, var_y, cov, corr, slope, r_+1, r_-1, r_+2, ..."""
    out = [d[k] for k in NAMES]
    for p, m in zip(d["lead"], d["lag"]):
        out += [p, m]
    return out
