"""CPU tier of the per-member co-spectra of two variables (include/rscm_gpu.h: rscm_ens_member_cross_spectrum,
rscm_gpu_spectrum_sines): the sine table against a high-precision sine; ``rscm_amd.variability.series_cross_spectrum`` (what a user
derives a record's targets with) against the numpy restatement of tests/host_cross_spectrum.py value for value (+0 equal to -0,
NaN to NaN); the band means against a direct cross-DFT in np.longdouble; the equalities the definition implies; the sign
convention; data that tells a fused multiply-add from the definition; and the C boundary's text.  No GPU: the accessors are host
code of the built library."""
import itertools
import os
import re

import numpy as np
import pytest

from rscm_amd import variability as rv
from tests import host_covariability as hc
from tests import host_cross_spectrum as hx
from tests import host_math as hm
from tests import host_spectrum as hs
from tests.helpers import same_values
from tests.test_gpu_cross_spectrum import F           # the kernel's tile (kXSpecF of csrc/cross_spectrum.hip)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
DETREND = ("mean", "linear", "difference")
PAIRS = list(itertools.product(DETREND, DETREND))
# the working series' lengths: the limits; J = (n - 1) // 2 one below the tile, at it, one and two into the second tile; one into the third
TERMS = [3, 4, 5, 8, 9] + list(range(2 * F - 1, 2 * F + 5)) + [4 * F + 3, 4 * F + 4]
# What test_band_means_against_the_longdouble_cross_dft holds every band mean to, in units of sqrt(Pxx_b Pyy_b): the scale
# tests/test_spectrum_cpu.py uses for band powers.  Measured worst over that test's cases: 9.7e-10 (n = 4096; 1.2e-11 at n = 750).
DEVIATION = 1e-8


def _rows(n, dx, dy):
    return n + (1 if "difference" in (dx, dy) else 0)


def _pair(R, N, seed, phi=0.9):
    """AR(1) pairs [R][N]: y = 0.5 x shifted by one row + independent noise."""
    rng = np.random.default_rng(seed)
    x = hs.ar1(R, phi, rng, N)
    y = 0.5 * np.vstack([x[:1], x[:-1]]) + 0.3 * rng.standard_normal((R, N))
    return x, y


def _edge_lists(n):
    """Edge lists for a working series of n terms: the defaults of 1, 2 and 3 bands, and lists that skip low and high frequencies."""
    J = (n - 1) // 2
    out = [rv.band_edges(n, b) for b in (1, 2, 3)]
    if J >= 3:
        out += [[2, J], [2, 3, J + 1], [1, 2, J]]
    if J >= F + 2:
        out += [[F - 1, F + 2], [3, F, F + 1, J], [F + 1, J + 1]]       # across two tiles; a band that ends with a tile; the second tile alone
    return out


# ---- the sine table -------------------------------------------------------------------------------------------------------------------

def _sin_ld(n, j):
    """sin(2 pi j / n) in longdouble for int64 arrays n, j (0 < 2 j < n), the angle folded in integers to [0, pi / 4] first."""
    p, q = 2 * j, n
    p = np.where(2 * p > q, q - p, p)                # angle pi p / q in (0, pi / 2]
    low = 4 * p <= q
    pi = hs.ld_pi()
    return np.where(low, np.sin(pi * p.astype(LD) / q.astype(LD)), np.cos(pi * (q - 2 * p).astype(LD) / (2 * q).astype(LD)))


def test_sines_within_one_ulp_and_refusals():
    """g_j of a sample of n in 3..4096 (every n up to 64, the limits, multiples of four and their neighbours, seeded others) is within
    1 ulp of sin(2 pi j / n) and > 0; the bulk reference is the folded longdouble sine, which mpmath at 50 digits pins on a sample."""
    rng = np.random.default_rng(21)
    sizes = sorted(set(range(3, 65)) | {170, 171, 750, 751, 1023, 1024, 1025, 4092, 4095, 4096} | set(int(v) for v in rng.integers(65, 4097, 60)))
    tables = {k: hx.sines(k) for k in sizes}
    assert all(len(tables[k]) == (k - 1) // 2 for k in sizes)
    n = np.concatenate([np.full((k - 1) // 2, k, dtype=np.int64) for k in sizes])
    j = np.concatenate([np.arange(1, (k - 1) // 2 + 1, dtype=np.int64) for k in sizes])
    got = np.concatenate([tables[k] for k in sizes])
    assert (got > 0.0).all() and (got <= 1.0).all()                  # j < n / 2: +0.0 is never needed
    for k in (4, 8, 1024, 4096):
        assert tables[k][k // 4 - 1] == 1.0
    idx = np.union1d(hm.sample_indices(n.size, 1024), np.flatnonzero(np.abs(4 * j - n) <= 3))
    mp = hm._mp()
    true_mp = np.array([hm.mp_to_ld(mp.sin(2 * mp.pi * int(jj) / int(nn))) for nn, jj in zip(n[idx], j[idx])], dtype=LD)
    assert hm.ulp_error(got[idx], true_mp).max() <= 1.0
    if hm.LONGDOUBLE_OK:
        true = _sin_ld(n, j)
        assert hm.ulp_error(true[idx].astype(np.float64), true_mp).max() <= 0.5 + hm.PIN       # the bulk reference itself, pinned
        err = hm.ulp_error(got, true)
        print("sine table max ulp error:", float(err.max()))
        assert err.max() <= 1.0
    from rscm_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096)
    for bad in (2, 0, -1, hs.MAX_TERMS + 1):
        assert lib.rscm_gpu_spectrum_sines(bad, _lib.dptr(buf)) == 1
    assert lib.rscm_gpu_spectrum_sines(8, None) == 1
    assert same_values(rv.spectrum_sines(170), tables[170])
    with pytest.raises(_lib.RscmGpuError):
        rv.spectrum_sines(2)
    with pytest.raises(_lib.RscmGpuError):
        rv.spectrum_sines(4097)


# ---- the host estimator against the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dx,dy", PAIRS)
def test_series_cross_spectrum_equals_the_restatement(dx, dy):
    N = 11
    for n in TERMS:
        x, y = _pair(_rows(n, dx, dy), N, seed=n)
        x[1, 4] = np.nan
        y[0, 9] = -np.inf
        x[:, 7] = 1.25                       # a constant x
        y[:, 8] = -0.5                       # a constant y
        for edges in _edge_lists(n):
            got, want = rv.series_cross_spectrum(x, y, dx, dy, edges), hx.cross_spectrum(x, y, dx, dy, edges)
            B = len(edges) - 1
            assert set(got) == {"var_x", "var_y", "coherence2", "gain", "gain_quad", "edges", "counts"}
            assert len(got["coherence2"]) == len(got["gain"]) == len(got["gain_quad"]) == B
            assert list(got["edges"]) == [int(e) for e in edges] and list(got["counts"]) == list(np.diff(np.asarray(edges, dtype=np.int64)))
            for g, w in zip(hx.flat(got), hx.flat(want)):
                assert g.shape == (N,) and same_values(g, w), (dx, dy, n, list(edges))
            for i in (4, 9):
                assert all(np.isnan(g[i]) for g in hx.flat(got))
            assert got["var_x"][7] == 0.0 and got["var_y"][8] == 0.0
            assert all(np.isnan(g[7]) for g in hx.flat(got)[2:])                                  # a constant x: 0 / 0 everywhere
            assert all(np.isnan(g[8]) for g in got["coherence2"])                                 # a constant y: 0 / 0 in the coherence,
            assert all(g[8] == 0.0 for g in got["gain"] + got["gain_quad"])                       # ... and no gain
            assert all(np.isfinite(g[:4]).all() for g in hx.flat(got))
        default = rv.series_cross_spectrum(x, y, dx, dy)
        assert list(default["edges"]) == list(rv.band_edges(n, 3))
        one = rv.series_cross_spectrum(x[:, 2], y[:, 2], dx, dy)                                  # [R]: floats, the same bits
        for g, w in zip(hx.flat(one), hx.flat(default)):
            assert isinstance(g, float) and same_values(np.float64(g), w[2])


# ---- the band means against the long-double cross-DFT ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 47, 170, 750, 4096])
def test_band_means_against_the_longdouble_cross_dft(n):
    """Pxx_b, Pyy_b, K_b, Q_b of AR(1) pairs (phi = 0.9, y = 0.5 x delayed by one row + independent noise; three seeds as columns)
    against the direct cross-DFT in np.longdouble of the same residuals: deviation over sqrt(Pxx_b Pyy_b) at most 1e-8, the scale
    tests/test_spectrum_cpu.py holds band powers to.  The cross terms share the recurrences' states with the powers, so the same
    bound was expected to hold, and it does: the measured worst is 9.7e-10 at n = 4096 (1.2e-11 at 750, 2.0e-12 at 170)."""
    assert hm.LONGDOUBLE_OK, "the reference needs an np.longdouble wider than float64"
    worst = 0.0
    for dx, dy in (("linear", "linear"), ("mean", "difference")):
        x, y = _pair(_rows(n, dx, dy), 3, seed=1000 * n)
        edges = rv.band_edges(n, 3)
        want = hx.cross_spectrum(x, y, dx, dy, edges)
        a, c = hx.pair_residuals(x, y, dx, dy)
        ref = hx.cross_dft_ld(np.stack(a), np.stack(c))
        for b, (e0, e1) in enumerate(zip(edges[:-1], edges[1:])):
            r = [o[e0 - 1:e1 - 1].sum(axis=0) / LD(int(e1 - e0)) for o in ref]
            scale = np.sqrt(r[0] * r[1])
            for k, name in enumerate(hx.MEANS):
                worst = max(worst, float((np.abs(want[name][b].astype(LD) - r[k]) / scale).max()))
    print(f"n = {n}: largest deviation of a band mean from the longdouble cross-DFT over sqrt(Pxx Pyy): {worst:.3e}")
    assert worst <= DEVIATION


# ---- the equalities of the definition -------------------------------------------------------------------------------------------------

def _neg_bits(a, b):
    """b is -a bit for bit (NaN against NaN)."""
    return same_values(a, -np.asarray(b)) and same_values(np.signbit(a) | np.isnan(a), ~np.signbit(b) | np.isnan(b))


@pytest.mark.parametrize("dx,dy", PAIRS)
def test_equalities(dx, dy):
    """var_x, var_y are covariability's; the exchange keeps coh2 and negates the quadrature; x against x and against 2 x."""
    for f in (rv.series_cross_spectrum, hx.cross_spectrum):
        for n in (5, 2 * F + 3, 170):
            x, y = _pair(_rows(n, dx, dy), 32, seed=300 + n)
            edges = rv.band_edges(n, 3)
            s, t = f(x, y, dx, dy, edges), f(y, x, dy, dx, edges)
            cov = hc.covariability(x, y, dx, dy, 0)
            assert same_values(s["var_x"], cov["var_x"]) and same_values(s["var_y"], cov["var_y"])
            assert same_values(s["var_x"], t["var_y"]) and same_values(s["var_y"], t["var_x"])
            for b in range(len(edges) - 1):
                assert same_values(s["coherence2"][b], t["coherence2"][b])
                assert np.isfinite(s["coherence2"][b]).all()
            if f is hx.cross_spectrum:
                for b in range(len(edges) - 1):
                    assert same_values(s["K"][b], t["K"][b]) and _neg_bits(s["Q"][b], t["Q"][b]) and same_values(s["Pxx"][b], t["Pyy"][b])
                    assert (s["Q"][b] != 0.0).any()
            same, twice = f(x, x, dx, dx, edges), f(x, 2.0 * x, dx, dx, edges)
            for b in range(len(edges) - 1):
                assert (same["gain_quad"][b] == 0.0).all() and (twice["gain_quad"][b] == 0.0).all()
                assert same_values(twice["coherence2"][b], same["coherence2"][b])
                assert same_values(twice["gain"][b], 2.0 * same["gain"][b])
                assert np.abs(same["gain"][b] - 1.0).max() <= 6 * DEVIATION and np.abs(same["coherence2"][b] - 1.0).max() <= 6 * DEVIATION
            assert same_values(twice["var_y"], 4.0 * same["var_x"])


def test_coherence_is_bounded():
    """coh2_b <= 1 up to rounding.  Exactly, K_b^2 + Q_b^2 <= Pxx_b Pyy_b (Cauchy-Schwarz over the band's ordinates).  With
    d = DEVIATION: the computed K_b and Q_b are within d D of their exact values, D = sqrt(Pxx_b Pyy_b) (the cross-DFT test above),
    and the computed Pxx_b, Pyy_b within d of their own size (tests/test_spectrum_cpu.py: Ixx is the spectrum's expression), so the
    computed D^2 is at least (1 - d)^2 of the exact one and, with k^2 + q^2 <= 1 for the exact ratios,
        coh2 <= ((|k| + d)^2 + (|q| + d)^2) / (1 - d)^2 <= (1 + 2 sqrt(2) d + 2 d^2) / (1 - d)^2 < 1 + 5 d;
    the two square roots, three divisions, two products and the sum that follow add less than 8 x 2^-53.  Asserted: 1 + 6 d.  Wild
    scales per member, every mode pair, wide and narrow bands."""
    rng = np.random.default_rng(3)
    for n in (9, 2 * F + 4, 120):
        scale = 10.0 ** rng.integers(-8, 8, 500)[None, :]
        for dx, dy in PAIRS:
            R = _rows(n, dx, dy)
            x = rng.normal(0.0, 1.0, (R, 500)) * scale
            y = (0.9 * x + 0.5 * rng.normal(0.0, 1.0, (R, 500)) * scale) * 2.0
            for edges in (rv.band_edges(n, 3), [1, (n - 1) // 2 + 1]):
                s = rv.series_cross_spectrum(x, y, dx, dy, edges)
                worst = max(float(np.max(c)) for c in s["coherence2"])
                assert worst <= 1.0 + 6 * DEVIATION, (dx, dy, n, worst)
                assert min(float(np.min(c)) for c in s["coherence2"]) >= 0.0


# ---- the sign convention --------------------------------------------------------------------------------------------------------------

def test_a_delayed_copy_has_positive_quadrature():
    """y a one-term delay of x: x leads, so gain_quad > 0 in every band; the exchange gives the negated bits.  The delay is circular
    (y_0 = x_{n-1}), so that X_c = e^{-iw} X_a holds at every frequency of the grid and the mean residuals are the same delay: the
    quadrature spectrum is |X_a|^2 sin w > 0, and no end effect competes with sin w in the lowest band, where it is 0.03."""
    rng = np.random.default_rng(8)
    x = hs.ar1(200, 0.5, rng, 16)
    y = np.roll(x, 1, axis=0)                                        # y_k = x_{k-1}
    for f in (rv.series_cross_spectrum, hx.cross_spectrum):
        for bands in (1, 2, 3):
            edges = rv.band_edges(200, bands)
            s, t = f(x, y, "mean", "mean", edges), f(y, x, "mean", "mean", edges)
            for b in range(bands):
                assert (s["gain_quad"][b] > 0.0).all() and (t["gain_quad"][b] < 0.0).all()
                if f is hx.cross_spectrum:
                    assert _neg_bits(s["Q"][b], t["Q"][b])


def test_a_sinusoid_pair_with_a_known_phase():
    """x = cos(w k), y = 2 cos(w k - 0.7) at w = 2 pi 10 / 96 (y lags: x leads), under weak independent noise: the band that holds
    frequency 10 has coherence ~ 1, gain 2 cos 0.7 and quadrature gain 2 sin 0.7; the noise bands have little coherence."""
    n, j0, amp, lag = 96, 10, 2.0, 0.7
    rng = np.random.default_rng(12)
    k = np.arange(n)[:, None]
    w = 2.0 * np.pi * j0 / n
    x = np.cos(w * k) + 1e-3 * rng.standard_normal((n, 8))
    y = amp * np.cos(w * k - lag) + 1e-3 * rng.standard_normal((n, 8))
    edges = [1, 8, 16, 48]
    for f in (rv.series_cross_spectrum, hx.cross_spectrum):
        s = f(x, y, "mean", "mean", edges)
        assert (s["coherence2"][1] > 0.9999).all()
        assert np.abs(s["gain"][1] - amp * np.cos(lag)).max() < 1e-2 and np.abs(s["gain_quad"][1] - amp * np.sin(lag)).max() < 1e-2
        assert (s["coherence2"][0] < 0.9).all() and (s["coherence2"][2] < 0.5).all()


# ---- failure values, refusals ---------------------------------------------------------------------------------------------------------

def test_failure_values_and_refused_arguments():
    x, y = _pair(60, 6, seed=5)
    x[7, 1], y[0, 2], y[59, 3] = np.nan, np.inf, -np.inf
    x[:, 4] = 3.0
    s = rv.series_cross_spectrum(x, y, "linear", "mean")
    for i in (1, 2, 3):
        assert all(np.isnan(g[i]) for g in hx.flat(s))
    assert s["var_x"][4] == 0.0 and np.isfinite(s["var_y"][4]) and all(np.isnan(g[4]) for g in hx.flat(s)[2:])
    assert all(np.isfinite(g[[0, 5]]).all() for g in hx.flat(s))
    for bad in ([1], [1, 1], [2, 1], [0, 3], [1, 31], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            rv.series_cross_spectrum(x, y, "mean", "mean", bad)
    with pytest.raises(ValueError):
        rv.series_cross_spectrum(x, y, "quadratic", "mean")
    with pytest.raises(ValueError):
        rv.series_cross_spectrum(x, y[:-1], "mean", "mean")
    with pytest.raises(ValueError):
        rv.series_cross_spectrum(x[:2], y[:2], "mean", "mean")
    with pytest.raises(ValueError):
        rv.series_cross_spectrum(x[:3], y[:3], "mean", "difference")
    with pytest.raises(ValueError):
        rv.series_cross_spectrum(np.zeros((4098, 1)), np.zeros((4098, 1)), "difference", "mean")


# ---- sensitivity to contraction -------------------------------------------------------------------------------------------------------

def test_a_fused_multiply_add_gives_other_bits():
    """Random full-mantissa doubles over nine terms (J = 4, one band): forming K and Q with fused multiply-adds changes the bits of
    more than a quarter of 1024 members in gain, gain_quad and coherence2 each (measured: 750, 380 and 690), so the bit-for-bit
    comparison on the device can tell whether the kernel fuses."""
    rng = np.random.default_rng(20261020)
    x, y = rng.random((9, 1024)) - 0.5, rng.random((9, 1024)) - 0.5
    plain, fused = hx.cross_spectrum(x, y, "mean", "mean", [1, 5]), hx.cross_spectrum(x, y, "mean", "mean", [1, 5], fused=True)
    differ = {k: int((plain[k][0] != fused[k][0]).sum()) for k in ("gain", "gain_quad", "coherence2")}
    print("members whose bits differ under fused multiply-adds, of 1024:", differ)
    assert all(v > 256 for v in differ.values())
    got = rv.series_cross_spectrum(x, y, "mean", "mean", [1, 5])
    assert all(same_values(g, w) for g, w in zip(hx.flat(got), hx.flat(plain)))


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------

def test_header_library_and_binding():
    text = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", text).group(1)) >= 21
    assert int(re.search(r"#define\s+RSCM_XSPEC_MAX_BANDS\s+(\d+)", text).group(1)) == 3 == hx.MAX_BANDS
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"RSCM_API\s+int\s+rscm_ens_member_cross_spectrum\s*\(\s*rscm_ens\*\s*h,\s*int32_t\s+var_x,\s*int32_t\s+var_y,\s*int32_t\s+t_begin,"
                     r"\s*int32_t\s+t_end,\s*int32_t\s+t_stride,\s*int32_t\s+mode_x,\s*int32_t\s+mode_y,\s*int32_t\s+n_bands,"
                     r"\s*const\s+int32_t\*\s*edges,\s*int32_t\s+slot,\s*void\*\*\s*out_dev\)", code)
    assert re.search(r"RSCM_API\s+int\s+rscm_gpu_spectrum_sines\s*\(\s*int32_t\s+n,\s*double\*\s*out\s*\)", code)
    import rscm_amd
    from rscm_amd import _lib
    from rscm_amd.core import GraphModel
    assert len(_lib.SIGNATURES["rscm_ens_member_cross_spectrum"][1]) == 12 and len(_lib.SIGNATURES["rscm_gpu_spectrum_sines"][1]) == 2
    assert _lib.XSPEC_MAX_BANDS == 3 == rv.XSPEC_MAX_BANDS
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 21 and hasattr(lib, "rscm_ens_member_cross_spectrum") and hasattr(lib, "rscm_gpu_spectrum_sines")
    assert callable(rscm_amd.Ensemble.cross_spectrum) and callable(GraphModel.cross_spectrum)
