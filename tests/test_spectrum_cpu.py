"""CPU tier of the per-member band powers and the spectral likelihood (include/rscm_gpu.h: rscm_ens_member_spectrum,
rscm_gpu_spectrum_coefficients, rscm_ens_loglik_spectrum_device): the coefficient table against a high-precision cosine, the
restatement (tests/host_spectrum.py) and the product's ``rscm_amd.variability.series_spectrum`` against each other and against a
direct DFT in np.longdouble, and the definitions' properties.  No GPU: the accessor is host code of the built library."""
import os
import re

import numpy as np
import pytest

from rscm_amd import variability as rv
from tests import host_math as hm
from tests import host_spectrum as hs
from tests import host_variability as hv
from tests.helpers import same_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
DETREND = ("mean", "linear", "difference")


# ---- the coefficient table ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tables():
    """{n: the library's c2 table} for every n the call accepts."""
    return {n: hs.coefficients(n) for n in range(3, hs.MAX_TERMS + 1)}


def _two_cos_ld(n, j):
    """2 cos(2 pi j / n) in longdouble for int64 arrays n, j (0 < 2 j < n).  The angle is folded in integers to [0, pi / 4] first --
    cos(pi - x) = -cos x, cos x = sin(pi / 2 - x) -- because an argument that has met pi loses, next to pi / 2, more bits than a
    double has to spare."""
    p, q = 2 * j, n
    neg = 2 * p > q
    p = np.where(neg, q - p, p)                      # angle pi p / q in (0, pi / 2]
    low = 4 * p <= q
    pi = hs.ld_pi()
    v = np.where(low, np.cos(pi * p.astype(LD) / q.astype(LD)), np.sin(pi * (q - 2 * p).astype(LD) / (2 * q).astype(LD)))
    return LD(2.0) * np.where(neg, -v, v)


def test_coefficients_within_one_ulp(tables):
    """Every c2_j of every n in 3..4096 is within 1 ulp of 2 cos(2 pi j / n): a stated condition of the table.  The bulk reference is
    the folded longdouble cosine; mpmath at 50 digits, which folds nothing, pins it (host_math.PIN) on a seeded sample and on the
    frequency next to n / 4 of every n, where an unfolded cosine would be worst."""
    n = np.concatenate([np.full((k - 1) // 2, k, dtype=np.int64) for k in tables])
    j = np.concatenate([np.arange(1, (k - 1) // 2 + 1, dtype=np.int64) for k in tables])
    got = np.concatenate([tables[k] for k in tables])
    assert got.size == n.size == sum((k - 1) // 2 for k in range(3, hs.MAX_TERMS + 1))
    near = np.flatnonzero((np.abs(4 * j - n) <= 3) & (4 * j != n))
    idx = np.union1d(hm.sample_indices(n.size, hm.MP_SAMPLE), near)
    mp = hm._mp()
    true_mp = np.array([hm.mp_to_ld(2 * mp.cos(2 * mp.pi * int(jj) / int(nn))) for nn, jj in zip(n[idx], j[idx])], dtype=LD)
    assert hm.ulp_error(got[idx], true_mp).max() <= 1.0
    if hm.LONGDOUBLE_OK:
        true = _two_cos_ld(n, j)
        assert hm.ulp_error(true[idx].astype(np.float64), true_mp).max() <= 0.5 + hm.PIN       # the bulk reference itself, pinned
        err = hm.ulp_error(got, true)
        print("c2 max ulp error:", float(err.max()))
        assert err.max() <= 1.0


def test_coefficients_exact_zero_and_refusals(tables):
    for n in range(4, hs.MAX_TERMS + 1, 4):
        c = tables[n][n // 4 - 1]
        assert c == 0.0 and not np.signbit(c), n
    assert all(len(tables[n]) == (n - 1) // 2 for n in tables)
    assert tables[3][0] == -1.0 or abs(tables[3][0] + 1.0) <= 2.0 ** -52          # 2 cos(2 pi / 3) = -1
    assert tables[6][0] == 1.0 or abs(tables[6][0] - 1.0) <= 2.0 ** -52           # 2 cos(pi / 3) = 1
    from rscm_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096)
    for n in (2, 0, -1, hs.MAX_TERMS + 1):
        assert lib.rscm_gpu_spectrum_coefficients(n, _lib.dptr(buf)) == 1
    assert lib.rscm_gpu_spectrum_coefficients(8, None) == 1
    assert same_values(rv.spectrum_coefficients(170), tables[170])
    with pytest.raises(_lib.RscmGpuError):
        rv.spectrum_coefficients(2)


# ---- the restatement against the long-double DFT -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4, 5, 47, 170, 750, 1024, 4096])
def test_series_spectrum_against_the_longdouble_dft(n):
    """Band powers of AR(1) series (phi = 0.9, five seeds as five columns), by series_spectrum, against a direct DFT in
    np.longdouble of the same residuals: relative deviation at most 1e-8.  A band of m ordinates has a sampling error of
    1 / sqrt(m), at least 1e-2 here; 1e-8 sits six orders below it, and the recurrence's own rounding (7e-11 at n = 4096, where it is
    largest, 2e-11 at n = 1024) stays well inside."""
    assert hm.LONGDOUBLE_OK, "the reference needs an np.longdouble wider than float64"
    x = np.concatenate([hs.ar1(n + 1, 0.9, np.random.default_rng(1000 * n + seed)) for seed in range(5)], axis=1)
    worst = 0.0
    for detrend in DETREND:
        rows = x if detrend == "difference" else x[:n]
        got = rv.series_spectrum(rows, detrend)
        want = hs.spectrum(rows, detrend, got["edges"])
        for k in hs.FIRST:
            assert same_values(got[k], want[k]), (detrend, k)
        assert len(got["power"]) == len(want["power"]) == len(got["edges"]) - 1
        assert all(same_values(p, w) for p, w in zip(got["power"], want["power"])), detrend
        a = np.stack(hs.residuals(rows, detrend)[0])
        I = hs.dft_ordinates_ld(a)
        for b, (e0, e1) in enumerate(zip(got["edges"][:-1], got["edges"][1:])):
            ref = I[e0 - 1:e1 - 1].sum(axis=0) / LD(int(e1 - e0))
            dev = np.abs(got["power"][b].astype(LD) - ref) / ref
            worst = max(worst, float(dev.max()))
    print(f"n = {n}: largest relative deviation of a band power from the longdouble DFT {worst:.3e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("n", [5, 47, 171, 751])
def test_parseval(n):
    """For odd n the ordinates j = 1 .. J are all of the spectrum but the mean: (2 / n) sum_j I_j = variance, to 1e-12 relative."""
    x = hs.ar1(n, 0.9, np.random.default_rng(n), 4)
    for detrend in ("mean", "linear"):
        J = (n - 1) // 2
        r = rv.series_spectrum(x, detrend, edges=[1, J + 1])
        total = r["power"][0] * J * 2.0 / n
        assert np.abs(total - r["variance"]).max() <= 1e-12 * r["variance"].max(), (detrend, total, r["variance"])


# ---- definitions and failure values ----------------------------------------------------------------------------------------------------

def test_band_edges():
    for n in list(range(3, 200)) + [750, 1024, 4095, 4096]:
        J = (n - 1) // 2
        for bands in (1, 2, 3, 8):
            e = rv.band_edges(n, bands)
            assert e.dtype == np.int32 and len(e) == min(bands, J) + 1
            assert e[0] == 1 and e[-1] == J + 1 and (np.diff(e) >= 1).all()
            hs.check_edges(n, e)
    e = rv.band_edges(170, 8)
    assert (np.diff(np.diff(e)) >= 0).all()                         # geometric: the bands widen towards high frequencies
    assert rv.band_edges(4096, 8).tolist() == [1, 2, 6, 17, 45, 117, 304, 789, 2048]       # floor(2048 ** (b / 8)), ascending
    assert rv.band_edges(19, 8).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 10]                   # J = 9: made ascending from the left
    assert rv.band_edges(513, 8).tolist() == [1, 2, 4, 8, 16, 32, 64, 128, 257]            # J + 1 = 257 > 2 ** 8: exact powers stay
    for bad in ((2, 8), (170, 0)):
        with pytest.raises(ValueError):
            rv.band_edges(*bad)
    x = hs.ar1(40, 0.5, np.random.default_rng(3))[:, 0]
    for edges in ([1], [0, 3], [1, 3, 3], [3, 2], [1, 21], list(range(1, 11))):
        with pytest.raises(ValueError):
            rv.series_spectrum(x, "mean", edges=edges)
    for rows in (x[:2], np.zeros(4098)):
        with pytest.raises(ValueError):
            rv.series_spectrum(rows, "mean")
    assert len(rv.series_spectrum(np.tile(x, 103)[:4097], "difference")["power"]) == 8       # 4096 terms: the cap itself


def test_failure_values():
    rng = np.random.default_rng(5)
    x = hs.ar1(60, 0.7, rng, 6)
    x[7, 1], x[0, 2], x[59, 3] = np.nan, np.inf, -np.inf
    x[:, 4] = 1.25                                                   # a constant series
    x[:, 5] = 0.5 * np.arange(60)                                    # constant increments
    for detrend in DETREND:
        r = rv.series_spectrum(x, detrend)
        vecs = [r[k] for k in hs.FIRST] + r["power"]
        for col in (1, 2, 3):
            assert all(np.isnan(v[col]) for v in vecs), (detrend, col)
        assert all(np.isfinite(v[0]) for v in vecs)
        assert r["variance"][4] == 0.0 and all(p[4] == 0.0 for p in r["power"])
        ll = hs.loglik_spectrum(r["power"], [1.0] * len(r["power"]), r["counts"])
        assert np.isneginf(ll[[1, 2, 3, 4]]).all() and np.isfinite(ll[0])
        if detrend == "difference":
            assert r["variance"][5] == 0.0 and all(p[5] == 0.0 for p in r["power"]) and np.isneginf(ll[5])
        one = rv.series_spectrum(x[:, 0], detrend)                    # a single series: floats
        assert isinstance(one["variance"], float) and one["variance"] == r["variance"][0]
        assert one["power"] == [float(p[0]) for p in r["power"]]
    ll = hs.loglik_spectrum([np.array([1.0, 2.0])], [1.5], [3], add=np.array([-np.inf, np.nan]))
    assert np.isneginf(ll).all()


@pytest.mark.parametrize("detrend", DETREND)
def test_first_three_are_series_variability(detrend):
    x = hs.ar1(171, 0.8, np.random.default_rng(11), 7) + 0.01 * np.arange(171)[:, None]
    s, v = rv.series_spectrum(x, detrend), rv.series_variability(x, detrend)
    w = hv.variability(x, detrend)
    for k in hs.FIRST:
        assert same_values(s[k], v[k]) and same_values(s[k], w[k]), k


def test_header_abi_minor():
    text = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define RSCM_GPU_ABI_MINOR (\d+)", text).group(1)) >= 17
    from rscm_amd import _lib
    assert _lib.load().rscm_gpu_abi_minor() >= 17


# ---- the likelihood --------------------------------------------------------------------------------------------------------------------

def test_likelihood_is_maximal_at_the_record_and_recovers_phi():
    """ll_b = m (ln P - 2 ln(P + I)) peaks at P = I.  And a record with phi = 0.6 (n = 170) scores members of equal variance with
    phi in {0, 0.3, 0.6, 0.9}, 200 realisations each: the mean log-likelihood is largest for 0.6."""
    P = np.linspace(0.2, 5.0, 481)
    for m in (1, 4, 37):
        ll = hs.loglik_spectrum([P], [1.7], [m])
        assert abs(P[np.argmax(ll)] - 1.7) <= 0.01
    n, members = 170, 200
    rng = np.random.default_rng(20260)
    record = rv.series_spectrum(hs.ar1(n, 0.6, rng)[:, 0], "mean")
    mean_ll = {}
    for phi in (0.0, 0.3, 0.6, 0.9):
        r = rv.series_spectrum(hs.ar1(n, phi, rng, members), "mean", edges=record["edges"])
        ll = hs.loglik_spectrum(r["power"], record["power"], record["counts"])
        assert np.isfinite(ll).all()
        mean_ll[phi] = float(ll.mean())
    print("mean log-likelihood by phi:", {k: round(v, 3) for k, v in mean_ll.items()})
    assert max(mean_ll, key=mean_ll.get) == 0.6
