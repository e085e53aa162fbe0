"""CPU tier of the covariability of two variables: ``rscm_amd.variability.series_covariability`` (what a user derives a record's
targets with) against the numpy restatement of tests/host_covariability.py value for value (+0 equal to -0, NaN to NaN) over the
nine mode pairs; the equalities the definition implies; the edges of the definition; data that tells a fused multiply-add from the
definition; and the C boundary's text (rscm_ens_member_covariability)."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import host_covariability as hc
from tests import host_variability as hv
from tests.helpers import same_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETREND = ("mean", "linear", "difference")
PAIRS = list(itertools.product(DETREND, DETREND))
LAGS = (0, 1, 2, 3)


def _sc():
    from rscm_amd.variability import series_covariability
    return series_covariability


def _rows(R, N, seed):
    """Two related random walks [R][N]: y responds to x with a delay of one row, plus noise of its own."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0.02, 0.15, (R, N)), axis=0) + rng.normal(0.0, 3.0, N)[None, :]
    y = 0.7 * np.vstack([x[:1], x[:-1]]) + np.cumsum(rng.normal(0.0, 0.05, (R, N)), axis=0)
    return x, y


def _terms(R, dx, dy):
    return R - (1 if "difference" in (dx, dy) else 0)


@pytest.mark.parametrize("dx,dy", PAIRS)
def test_series_covariability_equals_the_restatement(dx, dy):
    sc = _sc()
    for R in (3, 4, 5, 6, 7, 9, 40, 171):
        x, y = _rows(R, 23, seed=R)
        x[1, 4] = np.nan
        y[0, 9] = -np.inf
        x[:, 11] = 1.25                      # a constant x
        y[:, 12] = -0.5                      # a constant y
        for lags in LAGS:
            if _terms(R, dx, dy) < 3 + lags:                         # the refused shapes raise, in both
                with pytest.raises(ValueError):
                    sc(x, y, dx, dy, lags)
                with pytest.raises(ValueError):
                    hc.covariability(x, y, dx, dy, lags)
                continue
            got, want = sc(x, y, dx, dy, lags), hc.covariability(x, y, dx, dy, lags)
            assert set(got) == set(hc.NAMES) | {"lead", "lag"} and len(got["lead"]) == len(got["lag"]) == lags
            for g, w in zip(hc.flat(got), hc.flat(want)):
                assert g.shape == (23,) and same_values(g, w), (dx, dy, R, lags)
            for i in (4, 9):
                assert all(np.isnan(g[i]) for g in hc.flat(got))
            assert got["var_x"][11] == 0.0 and np.isnan(got["corr"][11]) and np.isnan(got["slope"][11]) and all(np.isnan(g[11]) for g in got["lead"] + got["lag"])
            assert got["var_y"][12] == 0.0 and np.isnan(got["corr"][12]) and all(np.isnan(g[12]) for g in got["lead"] + got["lag"])
            assert all(np.isfinite(g[:4]).all() for g in hc.flat(got))
            one = sc(x[:, 2], y[:, 2], dx, dy, lags)                 # [R]: floats, the same bits
            for g, w in zip(hc.flat(one), hc.flat(want)):
                assert isinstance(g, float) and same_values(np.float64(g), w[2])


@pytest.mark.parametrize("dx,dy", PAIRS)
def test_exchange_and_variance_equalities(dx, dy):
    """Exchanging the variables exchanges var_x with var_y and r_{+l} with r_{-l} and keeps cov and corr, value for value; with no mode
    mixed var_x is the variance of the variability statistics."""
    for f in (_sc(), hc.covariability):
        for R in (4, 7, 40, 171):
            x, y = _rows(R, 64, seed=100 + R)
            lags = min(3, _terms(R, dx, dy) - 3)
            s, t = f(x, y, dx, dy, lags), f(y, x, dy, dx, lags)
            assert same_values(s["var_x"], t["var_y"]) and same_values(s["var_y"], t["var_x"])
            assert same_values(s["cov"], t["cov"]) and same_values(s["corr"], t["corr"])
            for l in range(lags):
                assert same_values(s["lead"][l], t["lag"][l]) and same_values(s["lag"][l], t["lead"][l])
            if (dx == "difference") == (dy == "difference"):
                assert same_values(s["var_x"], hv.variability(x, dx)["variance"]) and same_values(s["var_y"], hv.variability(y, dy)["variance"])
            same = f(x, x, dx, dx, lags)                             # a variable against itself
            ok = np.isfinite(same["corr"])
            assert ok.all() and np.abs(same["corr"] - 1.0).max() <= 4 * 2.0 ** -52 and np.abs(same["slope"] - 1.0).max() <= 4 * 2.0 ** -52
            for l in range(lags):
                assert same_values(same["lead"][l], same["lag"][l])


def test_correlations_are_bounded():
    """|corr| and every lag are <= 1 up to rounding (Cauchy-Schwarz: 2 n roundings of relative size 2^-53 in each of three sums)."""
    rng = np.random.default_rng(3)
    sc = _sc()
    for R in (7, 40):
        wild_x = rng.normal(0.0, 1.0, (R, 4000)) * 10.0 ** rng.integers(-8, 8, 4000)[None, :]
        wild_y = 0.9 * wild_x + rng.normal(0.0, 1.0, (R, 4000)) * 10.0 ** rng.integers(-12, 4, 4000)[None, :]
        for dx, dy in PAIRS:
            s = sc(wild_x, wild_y, dx, dy, 3)
            for g in [s["corr"]] + s["lead"] + s["lag"]:
                assert np.nanmax(np.abs(g)) <= 1.0 + 8 * R * 2.0 ** -53, (dx, dy, R)


def test_a_fused_multiply_add_gives_other_bits():
    """Random full-mantissa doubles over nine terms: a contraction of the product sums into fused multiply-adds changes the bits of
    many members, so the bit-for-bit comparison on the device can tell whether the kernel fuses."""
    rng = np.random.default_rng(20261020)
    x, y = rng.random((9, 4096)) - 0.5, rng.random((9, 4096)) - 0.5
    plain, fused = hc.covariability(x, y, "mean", "mean", 1), hc.covariability(x, y, "mean", "mean", 1, fused=True)
    differ = {k: int((plain[k] != fused[k]).sum()) for k in ("var_x", "cov")}
    differ["lead"] = int((plain["lead"][0] != fused["lead"][0]).sum())
    print("members whose bits differ under fused multiply-adds, of 4096:", differ)
    assert all(v > 0 for v in differ.values())
    got = _sc()(x, y, "mean", "mean", 1)
    assert all(same_values(g, w) for g, w in zip(hc.flat(got), hc.flat(plain)))


def test_midpoint_pairing():
    """A differenced y next to a linear x: x at the midpoints, exactly; heat uptake that is a multiple of the temperature at the
    midpoints comes back with that multiple as the slope."""
    k = np.arange(12, dtype=np.float64)
    x = (0.25 * k * k)[:, None]                              # midpoints 0.25 (k^2 + k + 0.5), exact in binary
    mid = (x[:-1] + x[1:]) * 0.5
    y = np.vstack([np.zeros((1, 1)), np.cumsum(4.0 * mid, axis=0)])      # y_{k+1} - y_k = 4 mid_k, exactly
    for f in (_sc(), hc.covariability):
        s = f(x, y, "mean", "difference", 2)
        assert s["slope"][0] == 4.0 and abs(s["corr"][0] - 1.0) <= 2.0 ** -51
        assert same_values(s["var_x"], hv.variability(mid, "mean")["variance"])
        t = f(y, x, "difference", "mean", 2)
        assert t["var_y"][0] == s["var_x"][0] and t["slope"][0] == 0.25


def test_refused_arguments():
    sc = _sc()
    x, y = _rows(12, 3, seed=1)
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            sc(x, y, "mean", "mean", bad)
        with pytest.raises(ValueError):
            hc.covariability(x, y, "mean", "mean", bad)
    with pytest.raises(ValueError):
        sc(x, y, "quadratic", "mean")
    with pytest.raises(ValueError):
        sc(x, y, "mean", "cubic")
    with pytest.raises(ValueError):
        sc(x, y[:-1], "mean", "mean")
    with pytest.raises(ValueError):
        sc(np.zeros((3, 3, 3)), np.zeros((3, 3, 3)))
    for dx, dy, R, lags in (("mean", "linear", 2, 0), ("mean", "difference", 3, 0), ("linear", "linear", 5, 3), ("difference", "difference", 6, 3)):
        with pytest.raises(ValueError):
            sc(x[:R], y[:R], dx, dy, lags)


def test_header_library_and_binding():
    text = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", text).group(1)) >= 20        # (19 changed no entry point; this is 20)
    assert int(re.search(r"#define\s+RSCM_COV_MAX_LAGS\s+(\d+)", text).group(1)) == 3 == hc.MAX_LAGS
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"RSCM_API\s+int\s+rscm_ens_member_covariability\s*\(\s*rscm_ens\*\s*h,\s*int32_t\s+var_x,\s*int32_t\s+var_y,\s*int32_t\s+t_begin,"
                     r"\s*int32_t\s+t_end,\s*int32_t\s+t_stride,\s*int32_t\s+mode_x,\s*int32_t\s+mode_y,\s*int32_t\s+n_lags,\s*int32_t\s+slot,"
                     r"\s*void\*\*\s*out_dev\)", code)
    import rscm_amd
    from rscm_amd import _lib
    from rscm_amd.core import GraphModel
    assert "rscm_ens_member_covariability" in _lib.SIGNATURES and len(_lib.SIGNATURES["rscm_ens_member_covariability"][1]) == 11
    assert _lib.COV_MAX_LAGS == 3
    lib = _lib.load()
    assert lib.rscm_gpu_abi_minor() >= 20 and hasattr(lib, "rscm_ens_member_covariability")
    assert callable(rscm_amd.Ensemble.covariability) and callable(GraphModel.covariability)
