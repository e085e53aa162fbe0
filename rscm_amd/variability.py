"""The variability statistics of ``Ensemble.variability`` for a series on the host: the targets of a likelihood on variability come
from an observed record through the estimator the device applies to the members (include/rscm_gpu.h, rscm_ens_member_variability:
the one definition).  Pure numpy; every operation is one float64 operation rounded on its own and every sum runs left to right
over the rows, so a record put through this function and the same values put through the kernel agree bit for bit.

The same for the band powers of ``Ensemble.spectrum`` (rscm_ens_member_spectrum): ``series_spectrum`` with the default band edges of
``band_edges`` and the library's own coefficient table (``spectrum_coefficients``), and for the covariability of two series
(``Ensemble.covariability``, rscm_ens_member_covariability): ``series_covariability``, and for their co-spectra in frequency bands
(``Ensemble.cross_spectrum``, rscm_ens_member_cross_spectrum): ``series_cross_spectrum`` with the library's sine table
(``spectrum_sines``).

And for the running-mean diagnostics (``Ensemble.define_running_mean``, rscm_ens_define_running_mean): ``series_running_mean`` puts a
record through the mean the members' rows go through, so that a period-mean target comes out of the estimator it is compared with."""
import ctypes as C
from typing import Dict, Tuple

import numpy as np

from . import _lib as L

DETREND = {"mean": L.VAR_MEAN, "linear": L.VAR_LINEAR, "difference": L.VAR_DIFFERENCE}
STATISTICS = ("mean", "slope", "variance", "sd", "r1")


def detrend_mode(detrend) -> int:
    """``"mean"`` / ``"linear"`` / ``"difference"`` as the C boundary's ``RSCM_VAR_*`` value."""
    try:
        return DETREND[detrend]
    except (KeyError, TypeError):
        raise ValueError(f"detrend must be one of {sorted(DETREND)}, got {detrend!r}") from None


def running_mean_back(window: int, align: str = "centre") -> int:
    """The terms of a running-mean window that lie before its row: ``window - 1`` for ``"trailing"``, ``(window - 1) // 2`` for
    ``"centre"`` (a window of 20 spans t - 9 .. t + 10).  ``ValueError`` for a window outside 2 .. 64 or another ``align``."""
    window = int(window)
    if window < 2 or window > L.RUNMEAN_MAX_WINDOW:
        raise ValueError(f"window must be in 2 .. {L.RUNMEAN_MAX_WINDOW}, got {window}")
    if align not in L.RUNMEAN_ALIGN:
        raise ValueError(f"align must be one of {sorted(L.RUNMEAN_ALIGN)}, got {align!r}")
    return window - 1 if align == "trailing" else (window - 1) // 2


def series_running_mean(series, window: int, align: str = "centre", step: int = 1) -> Tuple[np.ndarray, int]:
    """``(values, first_index)``: the running mean of ``series`` -- ``[R]`` or ``[R][N]``, rows by members -- as
    ``Ensemble.define_running_mean(name, source, window, align, step)`` forms it, for every row whose window is complete:
    ``values[k]`` belongs to row ``first_index + k`` of the series, ``first_index = back * step`` (``running_mean_back``), and
    there are ``R - (window - 1) * step`` of them.  For row t: ``s = x[t - back*step]``, then ``s = s + x[t + (j - back)*step]`` for
    ``j = 1 .. window - 1`` in that order, then ``s / float(window)``; every add and the division is one float64 operation, so a
    record put through this function and the same values put through the kernel agree bit for bit (rscm_ens_define_running_mean
    states the arithmetic).  Nothing is padded: a series shorter than one window is a ``ValueError``."""
    back = running_mean_back(window, align)
    window, step = int(window), int(step)
    if step < 1:
        raise ValueError(f"step must be at least 1, got {step}")
    x = np.asarray(series, dtype=np.float64)
    if x.ndim not in (1, 2):
        raise ValueError(f"series_running_mean: [R] or [R][N] expected, got shape {x.shape}")
    n = x.shape[0] - (window - 1) * step
    if n < 1:
        raise ValueError(f"series_running_mean: {x.shape[0]} rows hold no window of {window} terms {step} apart")
    with np.errstate(all="ignore"):
        s = x[0:n].copy()
        for j in range(1, window):
            s = s + x[j * step:j * step + n]
        return s / float(window), back * step


def series_variability(x, detrend: str = "linear") -> Dict[str, object]:
    """``{"mean", "slope", "variance", "sd", "r1"}`` of ``x``: ``[R]`` (one series: floats) or ``[R][N]`` (rows by members:
    arrays of ``[N]``).  ``detrend`` as ``Ensemble.variability``; with ``"difference"`` the working series is ``x[1:] - x[:-1]``.
    At least three terms in the working series.  A series with a non-finite value has NaN in all five; a constant one has
    variance 0 and ``r1`` NaN (0/0)."""
    mode = detrend_mode(detrend)
    rows = np.asarray(x, dtype=np.float64)
    if rows.ndim not in (1, 2):
        raise ValueError(f"series_variability: [R] or [R][N] expected, got shape {rows.shape}")
    single = rows.ndim == 1
    if single:
        rows = rows[:, None]
    bad = ~np.isfinite(rows).all(axis=0)
    u = rows[1:] - rows[:-1] if mode == L.VAR_DIFFERENCE else rows
    n = u.shape[0]
    if n < 3:
        raise ValueError(f"series_variability: the working series has {n} terms, at least 3 are needed")
    with np.errstate(all="ignore"):
        a, m, b, C0 = _series_residuals(u, mode)
        C1 = a[0] * a[1]
        for k in range(2, n):
            C1 = C1 + a[k - 1] * a[k]
        variance = C0 / float(n)
        out = {"mean": m, "slope": b, "variance": variance, "sd": np.sqrt(variance), "r1": C1 / C0}
    return _finish(out, bad, single)


def _pair_series(rows, mode, other):
    """The working series of ``rows`` [R][N] under ``mode`` when the other variable's mode is ``other`` (rscm_ens_member_covariability):
    the rows, their differences, or -- next to a differenced partner -- their midpoints."""
    if mode == L.VAR_DIFFERENCE:
        return rows[1:] - rows[:-1]
    if other == L.VAR_DIFFERENCE:
        return (rows[:-1] + rows[1:]) * 0.5
    return rows


COV_MAX_LAGS = L.COV_MAX_LAGS
COV_STATISTICS = ("var_x", "var_y", "cov", "corr", "slope")


def series_covariability(x, y, detrend_x: str = "linear", detrend_y: str = "linear", lags: int = 0) -> Dict[str, object]:
    """``{"var_x", "var_y", "cov", "corr", "slope", "lead": [r_+1 ..], "lag": [r_-1 ..]}`` of the series ``x`` and ``y``: both
    ``[R]`` (floats come back) or both ``[R][N]`` (rows by members: arrays of ``[N]``) -- ``Ensemble.covariability`` for a record.
    ``detrend_x`` and ``detrend_y`` as ``series_variability``; when exactly one is ``"difference"`` the other series is taken at the
    midpoints ``(x[k] + x[k + 1]) * 0.5`` and then detrended by its own mode.  ``lags``: 0 to 3; at least ``3 + lags`` terms in the
    working series.  ``corr`` and ``slope`` (of ``y`` on ``x``) are those of the two residual series; ``lead[l - 1]`` is their
    correlation with ``x`` leading ``y`` by ``l`` terms, ``lag[l - 1]`` with ``y`` leading.  Operation for operation the definition
    of rscm_ens_member_covariability: what the kernel gives for the same values, bit for bit.  A non-finite value in either series
    gives NaN everywhere; a constant series variance 0 and NaN in ``corr`` and the lags."""
    mode_x, mode_y = detrend_mode(detrend_x), detrend_mode(detrend_y)
    rx, ry = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if rx.ndim not in (1, 2) or rx.shape != ry.shape:
        raise ValueError(f"series_covariability: two series of one shape [R] or [R][N] expected, got {rx.shape} and {ry.shape}")
    lags = int(lags)
    if not 0 <= lags <= COV_MAX_LAGS:
        raise ValueError(f"series_covariability: lags must be in [0, {COV_MAX_LAGS}], got {lags}")
    single = rx.ndim == 1
    if single:
        rx, ry = rx[:, None], ry[:, None]
    n = rx.shape[0] - (1 if L.VAR_DIFFERENCE in (mode_x, mode_y) else 0)
    if n < 3 + lags:
        raise ValueError(f"series_covariability: the working series has {n} terms, at least {3 + lags} are needed at {lags} lags")
    bad = ~(np.isfinite(rx).all(axis=0) & np.isfinite(ry).all(axis=0))
    with np.errstate(all="ignore"):
        a, _, _, Cxx = _series_residuals(_pair_series(rx, mode_x, mode_y), mode_x)
        c, _, _, Cyy = _series_residuals(_pair_series(ry, mode_y, mode_x), mode_y)

        def G(l):              # sum over k of a_k c_{k + l}, in order of k
            lo = max(0, -l)
            acc = a[lo] * c[lo + l]
            for k in range(lo + 1, n - max(0, l)):
                acc = acc + a[k] * c[k + l]
            return acc

        G0 = G(0)
        D = np.sqrt(Cxx) * np.sqrt(Cyy)
        out = {"var_x": Cxx / float(n), "var_y": Cyy / float(n), "cov": G0 / float(n), "corr": G0 / D, "slope": G0 / Cxx,
               "lead": [G(l) / D for l in range(1, lags + 1)], "lag": [G(-l) / D for l in range(1, lags + 1)]}
    return _finish(out, bad, single)


MAX_BANDS = 8          # rscm_ens_member_spectrum: 1 .. 8 bands
MAX_TERMS = 4096       # ... over a working series of 3 .. 4096 terms


def _iroot(x: int, k: int) -> int:
    """The largest integer e with e**k <= x, in integers."""
    e = int(round(x ** (1.0 / k)))
    while e ** k > x:
        e -= 1
    while (e + 1) ** k <= x:
        e += 1
    return e


def band_edges(n: int, bands: int = MAX_BANDS) -> np.ndarray:
    """The default band edges of ``Ensemble.spectrum`` for a working series of ``n`` terms: int32 ``[B + 1]`` with
    ``edges[0] = 1``, ``edges[B] = J + 1``, ``J = (n - 1) // 2``, strictly ascending; band ``b`` holds the frequencies
    ``edges[b] <= j < edges[b + 1]`` (cycles per ``n`` terms).  ``B = min(bands, J)``: with fewer frequencies than bands, fewer
    bands come back, one frequency each.

    The rule, in integers: the edges are spaced geometrically over ``1 .. J + 1`` -- ``g_b`` is the largest integer with
    ``g_b**B <= (J + 1)**b``, i.e. ``floor((J + 1)**(b / B))`` -- and then made strictly ascending from the left while leaving room on
    the right: ``edges[b] = min(max(g_b, edges[b - 1] + 1), J + 1 - (B - b))``.  Low frequencies so get narrow bands (few ordinates,
    where the spectrum of a red process changes fastest) and high frequencies wide ones."""
    n, bands = int(n), int(bands)
    if n < 3:
        raise ValueError(f"band_edges: the working series has {n} terms, at least 3 are needed")
    if bands < 1:
        raise ValueError(f"band_edges: {bands} bands, at least 1 is needed")
    J = (n - 1) // 2
    B = min(bands, J)
    edges = [1]
    for b in range(1, B + 1):
        g = _iroot((J + 1) ** b, B)
        edges.append(min(max(g, edges[-1] + 1), J + 1 - (B - b)))
    return np.asarray(edges, dtype=np.int32)


def check_edges(n: int, edges) -> np.ndarray:
    """``edges`` as contiguous int32 after the checks of rscm_ens_member_spectrum: 1 to 8 bands, strictly ascending, inside
    ``[1, J + 1]``."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).ravel())
    J = (int(n) - 1) // 2
    if not (2 <= e.size <= MAX_BANDS + 1):
        raise ValueError(f"band edges: 1 to {MAX_BANDS} bands (2 to {MAX_BANDS + 1} edges), got {e.size} edges")
    if e[0] < 1 or e[-1] > J + 1 or (np.diff(e) <= 0).any():
        raise ValueError(f"band edges must be strictly ascending inside [1, {J + 1}], got {e.tolist()}")
    return e.astype(np.int32)


def spectrum_coefficients(n: int) -> np.ndarray:
    """``[J]`` float64, ``J = (n - 1) // 2``: ``c2_j = 2 * (the double nearest cos(2 pi j / n))`` at ``[j - 1]``, from the library
    (rscm_gpu_spectrum_coefficients) -- the table the kernel is given, so that a restatement does not depend on numpy's cosine.
    ``3 <= n <= 4096``.  Needs the built library, not a GPU."""
    n = int(n)
    out = np.empty(max((n - 1) // 2, 0), dtype=np.float64)
    L.check(L.load().rscm_gpu_spectrum_coefficients(n, out.ctypes.data_as(C.POINTER(C.c_double)) if out.size else None))
    return out


def spectrum_sines(n: int) -> np.ndarray:
    """``[J]`` float64, ``J = (n - 1) // 2``: ``g_j`` = the double nearest ``sin(2 pi j / n)`` at ``[j - 1]``, from the library
    (rscm_gpu_spectrum_sines) -- the second table the cross-spectrum kernel is given.  ``3 <= n <= 4096``.  Needs the built library,
    not a GPU."""
    n = int(n)
    out = np.empty(max((n - 1) // 2, 0), dtype=np.float64)
    L.check(L.load().rscm_gpu_spectrum_sines(n, out.ctypes.data_as(C.POINTER(C.c_double)) if out.size else None))
    return out


def _series_residuals(u, mode):
    """(a [n][N], m, b, C0) of the working series ``u`` [n][N]: its residuals, mean, slope and their sum of squares, with the
    operations of ``series_variability``."""
    n = u.shape[0]
    h = (n - 1) * 0.5
    tau = np.arange(n, dtype=np.float64) - h
    S = u[0].copy()
    for k in range(1, n):
        S = S + u[k]
    m = S / float(n)
    b = np.zeros_like(m)
    if mode == L.VAR_LINEAR:
        Q = tau[0] * u[0]
        for k in range(1, n):
            Q = Q + tau[k] * u[k]
        b = Q / (float(n * (n * n - 1)) / 12.0)
    a = np.empty_like(u)
    C0 = None
    for k in range(n):
        ak = u[k] - m
        if mode == L.VAR_LINEAR:
            ak = ak - b * tau[k]
        a[k] = ak
        C0 = ak * ak if k == 0 else C0 + ak * ak
    return a, m, b, C0


def _residuals(rows, mode):
    """(a [n][N], m, b, C0 / n, bad) of ``rows`` [R][N]: the working series' residuals and the first three statistics."""
    bad = ~np.isfinite(rows).all(axis=0)
    u = rows[1:] - rows[:-1] if mode == L.VAR_DIFFERENCE else rows
    a, m, b, C0 = _series_residuals(u, mode)
    return a, m, b, C0 / float(u.shape[0]), bad


def _finish(out, bad, single):
    """``out`` (arrays of ``[N]`` and lists of them) with NaN where ``bad``; for a ``single`` series as floats and lists of floats."""
    nan = (lambda v: float(np.where(bad, np.nan, v)[0])) if single else (lambda v: np.where(bad, np.nan, v))
    return {k: [nan(w) for w in v] if isinstance(v, list) else nan(v) for k, v in out.items()}


def _goertzel(a, c):
    """``(s1, s2)``, each ``[F][N]``: the last value and the one before it of Goertzel's recurrence over the residuals ``a`` [n][N]
    with the coefficients ``c`` [F][1]."""
    s1 = np.zeros((c.shape[0], a.shape[1]))
    s2 = np.zeros_like(s1)
    for ak in a:
        s0 = (ak + c * s1) - s2
        s2 = s1
        s1 = s0
    return s1, s2


def _band_means(I, edges):
    """The mean of the ordinates ``I`` [F][N] (frequency ``edges[0]`` first) over each band, summed in ascending frequency."""
    lo, means = int(edges[0]), []
    for e0, e1 in zip(edges[:-1], edges[1:]):
        acc = I[e0 - lo].copy()
        for j in range(int(e0) + 1, int(e1)):
            acc = acc + I[j - lo]
        means.append(acc / float(int(e1) - int(e0)))
    return means


def series_spectrum(x, detrend: str = "difference", edges=None) -> Dict[str, object]:
    """``{"mean", "slope", "variance", "power": [one per band], "edges", "counts"}`` of ``x``: ``[R]`` (one series: floats) or
    ``[R][N]`` (rows by members: arrays of ``[N]``) -- ``Ensemble.spectrum`` for a record.  ``detrend`` as
    ``series_variability``; ``edges`` the band edges (default ``band_edges(n, 8)``).  ``power[b]`` is the mean periodogram ordinate
    ``I_j`` over ``edges[b] <= j < edges[b + 1]``, ``I_j`` by Goertzel's recurrence over the residuals with the library's
    coefficient table, scaled so that white noise has ``I_j`` = its variance on average.  Operation for operation the definition
    of rscm_ens_member_spectrum: what the kernel gives for the same values, bit for bit.  3 to 4096 terms in the working series.
    A series with a non-finite value has NaN everywhere; a constant one has variance 0 and all powers 0."""
    mode = detrend_mode(detrend)
    rows = np.asarray(x, dtype=np.float64)
    if rows.ndim not in (1, 2):
        raise ValueError(f"series_spectrum: [R] or [R][N] expected, got shape {rows.shape}")
    single = rows.ndim == 1
    if single:
        rows = rows[:, None]
    n = rows.shape[0] - (1 if mode == L.VAR_DIFFERENCE else 0)
    if n < 3 or n > MAX_TERMS:
        raise ValueError(f"series_spectrum: the working series has {n} terms, 3 to {MAX_TERMS} are needed")
    edges = band_edges(n) if edges is None else check_edges(n, edges)
    c2 = spectrum_coefficients(n)
    lo, hi = int(edges[0]), int(edges[-1])
    with np.errstate(all="ignore"):
        a, m, b, variance, bad = _residuals(rows, mode)
        c = c2[lo - 1:hi - 1, None]                       # [F][1] against the members' [N]
        s1, s2 = _goertzel(a, c)
        I = ((s1 * s1 + s2 * s2) - (c * s1) * s2) / float(n)
        out = {"mean": m, "slope": b, "variance": variance, "power": _band_means(I, edges)}
    out = _finish(out, bad, single)
    out["edges"] = edges
    out["counts"] = np.diff(edges).astype(np.int32)
    return out


XSPEC_MAX_BANDS = L.XSPEC_MAX_BANDS


def series_cross_spectrum(x, y, detrend_x: str = "linear", detrend_y: str = "linear", edges=None) -> Dict[str, object]:
    """``{"var_x", "var_y", "coherence2": [one per band], "gain": [..], "gain_quad": [..], "edges", "counts"}`` of the series ``x``
    and ``y``: both ``[R]`` (floats come back) or both ``[R][N]`` (rows by members: arrays of ``[N]``) --
    ``Ensemble.cross_spectrum`` for a record.  ``detrend_x`` and ``detrend_y`` and the pairing at the midpoints as
    ``series_covariability``; ``edges`` the band edges, 1 to 3 bands (default ``band_edges(n, 3)``).  Per band: the squared
    coherence of the two residual series, the gain of ``y`` on ``x`` (co-spectrum over the power of ``x``) and its quadrature part
    (positive where ``x`` leads), from two Goertzel recurrences over the residuals with the library's tables.  Operation for
    operation the definition of rscm_ens_member_cross_spectrum: what the kernel gives for the same values, bit for bit.  3 to 4096
    terms in the working series.  A non-finite value in either series gives NaN everywhere; a constant series variance 0 and NaN in
    the band statistics."""
    mode_x, mode_y = detrend_mode(detrend_x), detrend_mode(detrend_y)
    rx, ry = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if rx.ndim not in (1, 2) or rx.shape != ry.shape:
        raise ValueError(f"series_cross_spectrum: two series of one shape [R] or [R][N] expected, got {rx.shape} and {ry.shape}")
    single = rx.ndim == 1
    if single:
        rx, ry = rx[:, None], ry[:, None]
    n = rx.shape[0] - (1 if L.VAR_DIFFERENCE in (mode_x, mode_y) else 0)
    if n < 3 or n > MAX_TERMS:
        raise ValueError(f"series_cross_spectrum: the working series has {n} terms, 3 to {MAX_TERMS} are needed")
    edges = band_edges(n, XSPEC_MAX_BANDS) if edges is None else check_edges(n, edges)
    if edges.size - 1 > XSPEC_MAX_BANDS:
        raise ValueError(f"series_cross_spectrum: 1 to {XSPEC_MAX_BANDS} bands, got {edges.size - 1}")
    c2, g = spectrum_coefficients(n), spectrum_sines(n)
    lo, hi = int(edges[0]), int(edges[-1])
    bad = ~(np.isfinite(rx).all(axis=0) & np.isfinite(ry).all(axis=0))
    dn = float(n)
    with np.errstate(all="ignore"):
        a, _, _, Cxx = _series_residuals(_pair_series(rx, mode_x, mode_y), mode_x)
        c, _, _, Cyy = _series_residuals(_pair_series(ry, mode_y, mode_x), mode_y)
        cf, gf = c2[lo - 1:hi - 1, None], g[lo - 1:hi - 1, None]         # [F][1] against the members' [N]
        (s1, s2), (t1, t2) = _goertzel(a, cf), _goertzel(c, cf)
        ordinates = (((s1 * s1 + s2 * s2) - (cf * s1) * s2) / dn, ((t1 * t1 + t2 * t2) - (cf * t1) * t2) / dn,
                     ((s1 * t1 + s2 * t2) - (cf * 0.5) * (s1 * t2 + s2 * t1)) / dn, (gf * (s2 * t1 - s1 * t2)) / dn)
        out = {"var_x": Cxx / dn, "var_y": Cyy / dn, "coherence2": [], "gain": [], "gain_quad": []}
        for Pxx, Pyy, K, Q in zip(*(_band_means(I, edges) for I in ordinates)):
            D = np.sqrt(Pxx) * np.sqrt(Pyy)
            kc, qc = K / D, Q / D
            out["coherence2"].append(kc * kc + qc * qc)
            out["gain"].append(K / Pxx)
            out["gain_quad"].append(Q / Pxx)
    out = _finish(out, bad, single)
    out["edges"] = edges
    out["counts"] = np.diff(edges).astype(np.int32)
    return out
