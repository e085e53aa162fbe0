"""The variability statistics of ``Ensemble.variability`` for a series on the host: the targets of a likelihood on variability come
from an observed record through the estimator the device applies to the members (include/rscm_gpu.h, rscm_ens_member_variability:
the one definition).  Pure numpy; every operation is one float64 operation rounded on its own and every sum runs left to right
over the rows, so a record put through this function and the same values put through the kernel agree bit for bit.

The same for the band powers of ``Ensemble.spectrum`` (rscm_ens_member_spectrum): ``series_spectrum`` with the default band edges of
``band_edges`` and the library's own coefficient table (``spectrum_coefficients``)."""
import ctypes as C
from typing import Dict

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
    h = (n - 1) * 0.5
    tau = np.arange(n, dtype=np.float64) - h
    with np.errstate(all="ignore"):
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
        C0 = C1 = prev = None
        for k in range(n):
            a = u[k] - m
            if mode == L.VAR_LINEAR:
                a = a - b * tau[k]
            C0 = a * a if k == 0 else C0 + a * a
            if k == 1:
                C1 = prev * a
            elif k > 1:
                C1 = C1 + prev * a
            prev = a
        variance = C0 / float(n)
        out = {"mean": m, "slope": b, "variance": variance, "sd": np.sqrt(variance), "r1": C1 / C0}
    out = {k: np.where(bad, np.nan, v) for k, v in out.items()}
    return {k: float(v[0]) for k, v in out.items()} if single else out


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


def _residuals(rows, mode):
    """(a [n][N], m, b, C0 / n, bad) of ``rows`` [R][N]: the working series' residuals and the first three statistics, with the
    operations of ``series_variability``."""
    bad = ~np.isfinite(rows).all(axis=0)
    u = rows[1:] - rows[:-1] if mode == L.VAR_DIFFERENCE else rows
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
    return a, m, b, C0 / float(n), bad


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
        s1 = np.zeros((hi - lo, rows.shape[1]))
        s2 = np.zeros_like(s1)
        for k in range(n):
            s0 = (a[k] + c * s1) - s2
            s2 = s1
            s1 = s0
        I = ((s1 * s1 + s2 * s2) - (c * s1) * s2) / float(n)
        power = []
        for e0, e1 in zip(edges[:-1], edges[1:]):
            acc = I[e0 - lo].copy()
            for j in range(int(e0) + 1, int(e1)):
                acc = acc + I[j - lo]
            power.append(acc / float(int(e1) - int(e0)))
    nan = lambda v: np.where(bad, np.nan, v)
    out = {"mean": nan(m), "slope": nan(b), "variance": nan(variance), "power": [nan(p) for p in power]}
    if single:
        out = {"mean": float(out["mean"][0]), "slope": float(out["slope"][0]), "variance": float(out["variance"][0]),
               "power": [float(p[0]) for p in out["power"]]}
    out["edges"] = edges
    out["counts"] = np.diff(edges).astype(np.int32)
    return out
