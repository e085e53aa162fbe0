"""The per-member band powers (rscm_amd/csrc/spectrum.hip; the definition stated in include/rscm_gpu.h under rscm_ens_member_spectrum)
and the spectral likelihood over them (rscm_ens_loglik_spectrum_device) restated in numpy over ``[R][N]``: row loops, every operation
one float64 operation rounded on its own, sums left to right from their first term.  The working series and its residuals are those
of tests/host_variability.py.  The coefficients 2 cos(2 pi j / n) come from the library's accessor (rscm_gpu_spectrum_coefficients),
as the definition demands of every restatement; tests/test_spectrum_cpu.py holds that table to a high-precision cosine.  The GPU tests
compare the device against this bit for bit, the CPU tests ``rscm_amd.variability.series_spectrum``.  Also the references the CPU tests
need: a direct DFT in np.longdouble and AR(1) series.  No product code."""
import ctypes as C

import numpy as np

from tests import host_variability as hv

LD = np.longdouble
MAX_TERMS = 4096
FIRST = ("mean", "slope", "variance")


def coefficients(n):
    """[J] float64: the library's table c2_j = 2 C_j, j = 1 .. J = (n - 1) // 2."""
    from rscm_amd import _lib
    out = np.empty((n - 1) // 2, dtype=np.float64)
    _lib.check(_lib.load().rscm_gpu_spectrum_coefficients(int(n), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def residuals(rows, detrend):
    """(a: list of n arrays [N], m, b, variance): the residuals a_k and the first three statistics, with host_variability's operations."""
    mode = hv.MODES[detrend]
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.ndim == 2
    u = hv.working_series(rows, mode)
    n = len(u)
    if n < 3 or n > MAX_TERMS:
        raise ValueError(f"{n} terms: 3 to {MAX_TERMS} are needed")
    h = np.float64(n - 1) * np.float64(0.5)
    tau = [np.float64(k) - h for k in range(n)]
    S = u[0]
    for k in range(1, n):
        S = S + u[k]
    m = S / np.float64(n)
    if mode == hv.LINEAR:
        Q = tau[0] * u[0]
        for k in range(1, n):
            Q = Q + tau[k] * u[k]
        b = Q / (np.float64(n * (n * n - 1)) / np.float64(12.0))
    else:
        b = np.zeros(rows.shape[1])
    a = []
    for k in range(n):
        ak = u[k] - m
        if mode == hv.LINEAR:
            ak = ak - b * tau[k]
        a.append(ak)
    C0 = a[0] * a[0]
    for k in range(1, n):
        C0 = C0 + a[k] * a[k]
    return a, m, b, C0 / np.float64(n)


def ordinates(a, c2):
    """I [J][N]: I_j of the residuals a (n arrays of [N]) by Goertzel's recurrence, j = 1 .. J at [j - 1]."""
    n = len(a)
    c = np.asarray(c2, dtype=np.float64)[:, None]
    s1 = np.zeros((len(c2), len(a[0])))
    s2 = np.zeros_like(s1)
    for k in range(n):
        s0 = (a[k][None, :] + c * s1) - s2
        s2 = s1
        s1 = s0
    return ((s1 * s1 + s2 * s2) - (c * s1) * s2) / np.float64(n)


def band_powers(I, edges):
    """[P_b]: the ordinates edges[b] <= j < edges[b + 1] summed in ascending j, over their count."""
    out = []
    for e0, e1 in zip(edges[:-1], edges[1:]):
        e0, e1 = int(e0), int(e1)
        acc = I[e0 - 1]
        for j in range(e0 + 1, e1):
            acc = acc + I[j - 1]
        out.append(acc / np.float64(e1 - e0))
    return out


def check_edges(n, edges):
    edges = [int(e) for e in edges]
    J = (n - 1) // 2
    assert 2 <= len(edges) <= 9 and edges[0] >= 1 and edges[-1] <= J + 1 and all(x < y for x, y in zip(edges, edges[1:])), (n, edges)
    return edges


def spectrum(rows, detrend, edges):
    """{"mean", "slope", "variance": [N], "power": [one [N] per band]} of ``rows`` [R][N]; NaN everywhere for a member with a
    non-finite row."""
    rows = np.asarray(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        a, m, b, var = residuals(rows, detrend)
        edges = check_edges(len(a), edges)
        power = band_powers(ordinates(a, coefficients(len(a))), edges)
    bad = ~np.isfinite(rows).all(axis=0)
    nan = lambda v: np.where(bad, np.nan, v)
    return {"mean": nan(m), "slope": nan(b), "variance": nan(var), "power": [nan(p) for p in power]}


def loglik_spectrum(power, record, counts, add=None, dtype=np.float64):
    """[N]: (add or 0.0) + sum_b counts[b] (ln P_b - 2 ln(P_b + record[b])) in order b, -inf where a P_b is non-finite or <= 0 or add is
    not finite.  In ``dtype``: float64 states the operations, np.longdouble (from the logarithms on) is the reference of the GPU
    test's bound."""
    power = [np.asarray(p, dtype=np.float64) for p in power]
    n = len(power[0])
    base = np.zeros(n) if add is None else np.asarray(add, dtype=np.float64)
    bad = ~np.isfinite(base)
    with np.errstate(all="ignore"):
        partial = np.zeros(n, dtype=dtype)
        for P, I, m in zip(power, record, counts):
            bad = bad | ~(np.isfinite(P) & (P > 0.0))
            Pd = P.astype(dtype)
            t = (P + np.float64(I)).astype(dtype)             # one float64 addition, as the definition states it
            partial = partial + dtype(int(m)) * (np.log(Pd) - dtype(2.0) * np.log(t))
        total = base.astype(dtype) + partial
    return np.where(bad, dtype(-np.inf), total)


def loglik_spectrum_magnitude(power, record, counts, add=None):
    """[N] longdouble: |add_i| + sum_b m_b (|ln P_b| + 2 |ln t_b|), what the GPU test's bound scales with (NaN where not defined)."""
    n = len(power[0])
    with np.errstate(all="ignore"):
        mag = np.zeros(n, dtype=LD) if add is None else np.abs(np.asarray(add, dtype=np.float64).astype(LD))
        for P, I, m in zip(power, record, counts):
            Pd = np.asarray(P, dtype=np.float64).astype(LD)
            t = (np.asarray(P, dtype=np.float64) + np.float64(I)).astype(LD)
            mag = mag + LD(int(m)) * (np.abs(np.log(Pd)) + LD(2.0) * np.abs(np.log(t)))
    return mag


# ---- references of the CPU tests ------------------------------------------------------------------------------------------------------

def ld_pi():
    return LD(4.0) * np.arctan(LD(1.0))


def dft_ordinates_ld(a):
    """I [J][N] in np.longdouble by the direct DFT of the residuals a [n][N]: |sum_k a_k exp(-2 pi i j k / n)|^2 / n, the angle of each
    term reduced in integers (j k mod n) before it meets pi."""
    a = np.asarray(a, dtype=np.float64).astype(LD)
    n = a.shape[0]
    J = (n - 1) // 2
    ang = LD(2.0) * ld_pi() * np.arange(n).astype(LD) / LD(n)
    cos_t, sin_t = np.cos(ang), np.sin(ang)
    k = np.arange(n, dtype=np.int64)
    out = np.empty((J, a.shape[1]), dtype=LD)
    for j0 in range(1, J + 1, 256):
        j = np.arange(j0, min(j0 + 256, J + 1), dtype=np.int64)
        r = (j[:, None] * k[None, :]) % n
        re = cos_t[r] @ a
        im = sin_t[r] @ a
        out[j0 - 1:j0 - 1 + len(j)] = (re * re + im * im) / LD(n)
    return out


def ar1(n, phi, rng, members=1, sd=1.0):
    """[n][members]: stationary AR(1) series of standard deviation ``sd``."""
    e = rng.standard_normal((n, members)) * np.sqrt(1.0 - phi * phi) * sd
    x = np.empty((n, members))
    x[0] = rng.standard_normal(members) * sd
    for k in range(1, n):
        x[k] = phi * x[k - 1] + e[k]
    return x
