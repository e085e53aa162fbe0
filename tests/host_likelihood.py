"""The Gaussian log-likelihood with reference periods ("Reference periods") restated in numpy over ``[T][N]``
series: what the GPU tests compare ``loglik`` / ``run_loglik`` / the device sampler against and the host
``GaussianLikelihood.ln_likelihood`` equals member by member.  Built on ``host_indicators.baseline`` / ``anomaly``: the likelihood's
``b`` and ``x - b`` are the bits of ``rscm_ens_set_baseline`` and ``RSCM_SELECT_ANOMALY``."""
import numpy as np

from tests.host_indicators import anomaly, baseline

LN_2PI = 1.8378770664093453   # ln(2*pi) rounded to f64, the constant of the kernels (= math.log(2.0 * math.pi))


def reference_baseline(series, period):
    """``b[N]`` of the rows ``t_begin, t_begin + t_stride, ... < t_end`` of ``series`` ([T][N]); ``period`` = (t_begin, t_end[, t_stride])."""
    t_begin, t_end = int(period[0]), int(period[1])
    t_stride = int(period[2]) if len(period) > 2 else 1
    with np.errstate(all="ignore"):
        return baseline(np.asarray(series, dtype=np.float64)[t_begin:t_end:t_stride])


def loglik(series, obs_var, obs_tidx, obs_value, obs_sigma, normalize=False, reference=None, computed=None):
    """Per-member ln L, ``[N]``.

    ``series``: ``{variable: [T][N]}``; the observations in the caller's order, grouped by variable; ``reference``:
    ``{variable: (t_begin, t_end[, t_stride])}`` in row indices (end exclusive, the row convention of ``rscm_ens_set_baseline``).
    Per-variable partial sums in observation order, then the total in variable order; a member with a non-finite ``b`` or a
    non-finite value at an observed row is ``-inf``.  ``computed``: the last computed row; an observation or a reference row beyond
    it makes every member ``-inf``."""
    reference = dict(reference or {})
    n = next(iter(series.values())).shape[1]
    total = np.zeros(n)
    bad = np.zeros(n, dtype=bool)
    if computed is not None:
        last = max([int(t) for t in obs_tidx] + [range(*(int(x) for x in p))[-1] for p in reference.values()], default=0)
        if last > computed:
            return np.full(n, -np.inf)
    groups = []
    for j, v in enumerate(obs_var):
        if not groups or groups[-1][0] != v:
            groups.append((v, []))
        groups[-1][1].append(j)
    with np.errstate(all="ignore"):
        for v, members in groups:
            x = np.asarray(series[v], dtype=np.float64)
            b = None
            if v in reference:
                b = reference_baseline(x, reference[v])
                bad |= ~np.isfinite(b)
            partial = np.zeros(n)
            for j in members:
                row = x[int(obs_tidx[j])]
                bad |= ~np.isfinite(row)
                m = row if b is None else anomaly(row[None, :], b)[0]
                sigma = float(obs_sigma[j])
                residual = float(obs_value[j]) - m
                chi = (residual * residual) / (sigma * sigma)
                l = -0.5 * chi
                if normalize:
                    l = l - 0.5 * LN_2PI
                    l = l - np.log(sigma)
                partial = partial + l
            total = total + partial
    return np.where(bad, -np.inf, total)
