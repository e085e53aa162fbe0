"""The per-member variability statistics (rscm_amd/csrc/variability.hip; the definition stated in include/rscm_gpu.h under
rscm_ens_member_variability) and the Gaussian likelihood over per-member vectors (rscm_ens_loglik_vectors_device) restated in numpy
over ``[R][N]``: row loops, every operation one float64 operation rounded on its own, sums left to right from their first term.  The
GPU tests compare the device against this bit for bit, the CPU tests ``rscm_amd.variability.series_variability``.  No product code."""
import numpy as np

MEAN, LINEAR, DIFFERENCE = 0, 1, 2
MODES = {"mean": MEAN, "linear": LINEAR, "difference": DIFFERENCE}
NAMES = ("mean", "slope", "variance", "sd", "r1")


def working_series(rows, mode):
    """u [n][N]: the rows themselves, or (DIFFERENCE) x_{k+1} - x_k, one IEEE subtraction each."""
    rows = np.asarray(rows, dtype=np.float64)
    if mode != DIFFERENCE:
        return rows
    return np.stack([rows[k + 1] - rows[k] for k in range(len(rows) - 1)]) if len(rows) > 1 else rows[:0]


def variability(rows, detrend):
    """{"mean", "slope", "variance", "sd", "r1"}, each [N], of ``rows`` [R][N]; NaN in all five for a member with a non-finite row."""
    mode = MODES[detrend]
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.ndim == 2
    with np.errstate(all="ignore"):
        u = working_series(rows, mode)
        n = len(u)
        if n < 3:
            raise ValueError(f"{n} terms: at least 3 are needed")
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
            stt = np.float64(n * (n * n - 1)) / np.float64(12.0)
            b = Q / stt
        else:
            b = np.zeros(rows.shape[1])
        a = []
        for k in range(n):
            ak = u[k] - m
            if mode == LINEAR:
                ak = ak - b * tau[k]
            a.append(ak)
        C0 = a[0] * a[0]
        for k in range(1, n):
            C0 = C0 + a[k] * a[k]
        C1 = a[0] * a[1]
        for k in range(1, n - 1):
            C1 = C1 + a[k] * a[k + 1]
        var = C0 / np.float64(n)
        out = {"mean": m, "slope": b, "variance": var, "sd": np.sqrt(var), "r1": C1 / C0}
    bad = ~np.isfinite(rows).all(axis=0)
    return {k: np.where(bad, np.nan, v) for k, v in out.items()}


def loglik_vectors(vectors, values, sigmas, add=None):
    """[N]: (add or 0.0) + sum_j -0.5 ((values[j] - vectors[j])^2 / sigmas[j]^2) in order j; -inf where a vector or add is not finite."""
    vectors = [np.asarray(v, dtype=np.float64) for v in vectors]
    n = len(vectors[0])
    base = np.zeros(n) if add is None else np.asarray(add, dtype=np.float64)
    bad = ~np.isfinite(base)
    with np.errstate(all="ignore"):
        partial = np.zeros(n)
        for v, value, sigma in zip(vectors, values, sigmas):
            bad = bad | ~np.isfinite(v)
            value, sigma = np.float64(value), np.float64(sigma)
            r = value - v
            chi = (r * r) / (sigma * sigma)
            partial = partial + np.float64(-0.5) * chi
        total = base + partial
    return np.where(bad, -np.inf, total)
