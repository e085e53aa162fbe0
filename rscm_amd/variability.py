"""The variability statistics of ``Ensemble.variability`` for a series on the host: the targets of a likelihood on variability come
from an observed record through the estimator the device applies to the members (include/rscm_gpu.h, rscm_ens_member_variability:
the one definition).  Pure numpy; every operation is one float64 operation rounded on its own and every sum runs left to right
over the rows, so a record put through this function and the same values put through the kernel agree bit for bit."""
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
