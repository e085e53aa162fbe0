"""The per-member co-spectra of two variables in frequency bands (rscm_amd/csrc/cross_spectrum.hip; the definition stated in
include/rscm_gpu.h under rscm_ens_member_cross_spectrum) restated in numpy over two ``[R][N]`` blocks of rows: row loops, every
operation one float64 operation rounded on its own, sums left to right from their first term.  The working series and residuals are
those of tests/host_covariability.py (and so of tests/host_variability.py); the tables 2 cos(2 pi j / n) and sin(2 pi j / n) come from
the library's accessors, as the definition demands of every restatement; tests/test_cross_spectrum_cpu.py holds the sine table to a
high-precision sine.  The GPU tests compare the device against this bit for bit, the CPU tests
``rscm_amd.variability.series_cross_spectrum``.  Also the reference of the CPU tests: a direct cross-DFT in np.longdouble.  No
product code."""
import ctypes as C

import numpy as np

from tests import host_covariability as hc
from tests import host_spectrum as hs
from tests.host_variability import MODES

LD = np.longdouble
MAX_BANDS = 3
MAX_TERMS = hs.MAX_TERMS
MEANS = ("Pxx", "Pyy", "K", "Q")


def sines(n):
    """[J] float64: the library's table g_j, the double nearest sin(2 pi j / n), j = 1 .. J = (n - 1) // 2."""
    from rscm_amd import _lib
    out = np.empty((n - 1) // 2, dtype=np.float64)
    _lib.check(_lib.load().rscm_gpu_spectrum_sines(int(n), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def pair_residuals(rows_x, rows_y, detrend_x, detrend_y):
    """(a, c): the residuals of both working series, lists of n arrays [N], with host_covariability's operations."""
    mx, my = MODES[detrend_x], MODES[detrend_y]
    rows_x, rows_y = np.asarray(rows_x, dtype=np.float64), np.asarray(rows_y, dtype=np.float64)
    assert rows_x.ndim == 2 and rows_x.shape == rows_y.shape
    u, v = hc.pair_series(rows_x, mx, my), hc.pair_series(rows_y, my, mx)
    n = len(u)
    assert len(v) == n
    if n < 3 or n > MAX_TERMS:
        raise ValueError(f"{n} terms: 3 to {MAX_TERMS} are needed")
    return hc.residuals(u, mx), hc.residuals(v, my)


def _fma(p, q, acc):
    """p * q + acc with one rounding, elementwise (the exact product in Python fractions)."""
    from fractions import Fraction
    p, q, acc = np.broadcast_arrays(p, q, acc)
    out = np.empty(acc.shape)
    for i in np.ndindex(acc.shape):
        out[i] = float(Fraction(float(p[i])) * Fraction(float(q[i])) + Fraction(float(acc[i])))
    return out


def states(a, c2):
    """(s1, s2) [F][N] each: Goertzel's recurrence over the residuals a (n arrays of [N]) for the coefficients c2 [F]."""
    cf = np.asarray(c2, dtype=np.float64)[:, None]
    s1 = np.zeros((len(c2), len(a[0])))
    s2 = np.zeros_like(s1)
    for k in range(len(a)):
        s0 = (a[k][None, :] + cf * s1) - s2
        s2 = s1
        s1 = s0
    return s1, s2


def ordinates(s1, s2, t1, t2, c2, g, n, fused=False):
    """(Ixx, Iyy, K, Q) [F][N] each from the final states of the two recurrences.  ``fused``: the cross expressions as a compiler
    that contracts a*b + c would form them -- not the definition: what the comparison must be able to tell apart from it."""
    cf, gf, dn = np.asarray(c2, dtype=np.float64)[:, None], np.asarray(g, dtype=np.float64)[:, None], np.float64(n)
    h = cf * np.float64(0.5)
    Ixx = ((s1 * s1 + s2 * s2) - (cf * s1) * s2) / dn
    Iyy = ((t1 * t1 + t2 * t2) - (cf * t1) * t2) / dn
    if fused:
        K = _fma(-h, _fma(s1, t2, s2 * t1), _fma(s1, t1, s2 * t2)) / dn
        Q = (gf * _fma(s2, t1, -(s1 * t2))) / dn
    else:
        K = ((s1 * t1 + s2 * t2) - h * (s1 * t2 + s2 * t1)) / dn
        Q = (gf * (s2 * t1 - s1 * t2)) / dn
    return Ixx, Iyy, K, Q


def check_edges(n, edges):
    edges = [int(e) for e in edges]
    J = (n - 1) // 2
    assert 2 <= len(edges) <= MAX_BANDS + 1 and edges[0] >= 1 and edges[-1] <= J + 1 and all(x < y for x, y in zip(edges, edges[1:])), (n, edges)
    return edges


def cross_spectrum(rows_x, rows_y, detrend_x, detrend_y, edges, fused=False):
    """{"var_x", "var_y": [N]; "coherence2", "gain", "gain_quad": one [N] per band; "Pxx", "Pyy", "K", "Q": the band means, one [N]
    per band} of the rows [R][N] of two variables; NaN everywhere for a member with a non-finite value in a row of either."""
    rows_x, rows_y = np.asarray(rows_x, dtype=np.float64), np.asarray(rows_y, dtype=np.float64)
    with np.errstate(all="ignore"):
        a, c = pair_residuals(rows_x, rows_y, detrend_x, detrend_y)
        n = len(a)
        edges = check_edges(n, edges)
        lo, hi = edges[0], edges[-1]
        c2, g = hs.coefficients(n)[lo - 1:hi - 1], sines(n)[lo - 1:hi - 1]
        Cxx, Cyy = hc.lagged(a, a, 0), hc.lagged(c, c, 0)
        s1, s2 = states(a, c2)
        t1, t2 = states(c, c2)
        I = ordinates(s1, s2, t1, t2, c2, g, n, fused)
        dn = np.float64(n)
        out = {"var_x": Cxx / dn, "var_y": Cyy / dn, "coherence2": [], "gain": [], "gain_quad": [], "Pxx": [], "Pyy": [], "K": [], "Q": []}
        for e0, e1 in zip(edges[:-1], edges[1:]):
            mean = []
            for o in I:
                acc = o[e0 - lo]
                for j in range(e0 + 1, e1):
                    acc = acc + o[j - lo]
                mean.append(acc / np.float64(e1 - e0))
            Pxx, Pyy, K, Q = mean
            D = np.sqrt(Pxx) * np.sqrt(Pyy)
            kc, qc = K / D, Q / D
            out["coherence2"].append(kc * kc + qc * qc)
            out["gain"].append(K / Pxx)
            out["gain_quad"].append(Q / Pxx)
            for k, val in zip(MEANS, mean):
                out[k].append(val)
    bad = ~(np.isfinite(rows_x).all(axis=0) & np.isfinite(rows_y).all(axis=0))
    return {k: [np.where(bad, np.nan, w) for w in val] if isinstance(val, list) else np.where(bad, np.nan, val) for k, val in out.items()}


def flat(d):
    """The vectors of a result in the order of the C boundary's output: var_x, var_y, then per band coh2, gain, gain_quad."""
    out = [d["var_x"], d["var_y"]]
    for b in range(len(d["coherence2"])):
        out += [d["coherence2"][b], d["gain"][b], d["gain_quad"][b]]
    return out


# ---- reference of the CPU tests -------------------------------------------------------------------------------------------------------

def cross_dft_ld(a, c):
    """(Ixx, Iyy, K, Q) [J][N] each in np.longdouble by the direct DFTs X_a, X_c of the residuals a, c [n][N], X = sum_k x_k
    exp(-2 pi i j k / n): |X_a|^2 / n, |X_c|^2 / n and the real and imaginary parts of X_a conj(X_c) / n; the angle of each term
    reduced in integers (j k mod n) before it meets pi, as host_spectrum.dft_ordinates_ld does."""
    a, c = np.asarray(a, dtype=np.float64).astype(LD), np.asarray(c, dtype=np.float64).astype(LD)
    n = a.shape[0]
    J = (n - 1) // 2
    ang = LD(2.0) * hs.ld_pi() * np.arange(n).astype(LD) / LD(n)
    cos_t, sin_t = np.cos(ang), np.sin(ang)
    k = np.arange(n, dtype=np.int64)
    out = [np.empty((J, a.shape[1]), dtype=LD) for _ in range(4)]
    for j0 in range(1, J + 1, 256):
        j = np.arange(j0, min(j0 + 256, J + 1), dtype=np.int64)
        r = (j[:, None] * k[None, :]) % n
        ct, st = cos_t[r], sin_t[r]
        ra, ia, rc, ic = ct @ a, -(st @ a), ct @ c, -(st @ c)            # X = re + i im
        sl = slice(j0 - 1, j0 - 1 + len(j))
        out[0][sl] = (ra * ra + ia * ia) / LD(n)
        out[1][sl] = (rc * rc + ic * ic) / LD(n)
        out[2][sl] = (ra * rc + ia * ic) / LD(n)
        out[3][sl] = (ia * rc - ra * ic) / LD(n)
    return out
