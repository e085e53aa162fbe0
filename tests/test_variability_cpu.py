"""CPU tier of the variability statistics: ``rscm_amd.variability.series_variability`` (what a user derives a record's targets
with) against the numpy restatement of tests/host_variability.py value for value (+0 equal to -0, NaN to NaN); the estimator
against the known moments of AR(1) noise; the edges of the definition; and the C boundary's text (ABI minor 16)."""
import os
import re

import numpy as np
import pytest

from tests import host_variability as hv
from tests.helpers import same_values
from tests.host_forcing_noise_red import red_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETREND = ("mean", "linear", "difference")


def _sv():
    from rscm_amd.variability import series_variability
    return series_variability


def _rows(R, N, seed=7):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(0.02, 0.15, (R, N)), axis=0) + rng.normal(0.0, 3.0, N)[None, :]


@pytest.mark.parametrize("detrend", DETREND)
@pytest.mark.parametrize("R", [3, 4, 9, 171])
def test_series_variability_equals_the_restatement(detrend, R):
    sv = _sv()
    if detrend == "difference" and R == 3:
        with pytest.raises(ValueError):
            sv(_rows(R, 5), detrend)
        with pytest.raises(ValueError):
            hv.variability(_rows(R, 5), detrend)
        return
    rows = _rows(R, 37, seed=R)
    rows[1, 4] = np.nan
    rows[0, 9] = np.inf
    rows[:, 11] = 1.25
    got, want = sv(rows, detrend), hv.variability(rows, detrend)
    assert set(got) == set(hv.NAMES)
    for k in hv.NAMES:
        assert got[k].shape == (37,) and same_values(got[k], want[k]), (k, detrend, R)
    for i in (0, 4, 9, 11):                                       # [R]: floats, the same bits
        one = sv(rows[:, i], detrend)
        for k in hv.NAMES:
            assert isinstance(one[k], float) and same_values(np.float64(one[k]), want[k][i]), (k, i)


@pytest.mark.parametrize("phi", [0.0, 0.6, 0.9])
def test_estimator_on_ar1_noise(phi):
    """64 members of 2048 terms of AR(1) noise with sd 0.5: the moments the statistics claim to measure."""
    n_members, n = 64, 2048
    x = np.asarray(red_noise(20260327, np.arange(n_members, dtype=np.uint64), n, 0.5, phi), dtype=np.float64)
    rows = x if x.shape == (n, n_members) else x.T
    assert rows.shape == (n, n_members)
    for detrend in ("mean", "linear"):
        s = hv.variability(rows, detrend)
        r1, var = s["r1"].mean(), s["variance"].mean()
        se_r1 = np.sqrt((1 - phi * phi) / (n_members * n))
        se_var = 0.25 * np.sqrt(2 * (1 + phi * phi) / ((1 - phi * phi) * n_members * n))
        print(f"{detrend} phi={phi}: r1 off by {(r1 - (phi - (1 + 3 * phi) / n)) / se_r1:+.2f} s.e., variance by {(var - 0.25) / se_var:+.2f} s.e.")
        assert abs(r1 - (phi - (1 + 3 * phi) / n)) <= 5 * se_r1, (detrend, phi, r1)
        assert abs(var - 0.25) <= 5 * se_var, (detrend, phi, var)
    s = hv.variability(rows, "difference")
    r1, var = s["r1"].mean(), s["variance"].mean()
    print(f"difference phi={phi}: r1 off by {r1 + (1 - phi) / 2:+.4f}, variance by {var / (2 * 0.25 * (1 - phi)) - 1:+.2%}")
    assert abs(r1 - (-(1 - phi) / 2)) <= 0.015, (phi, r1)
    assert abs(var - 2 * 0.25 * (1 - phi)) <= 0.03 * 2 * 0.25 * (1 - phi), (phi, var)


def test_edges():
    sv = _sv()
    rng = np.random.default_rng(3)
    rows = rng.normal(0.0, 1.0, (12, 6))
    rows[:, 0] = -2.5                       # a constant member
    rows[7, 2] = np.nan
    rows[3, 4] = -np.inf
    for detrend in DETREND:
        for f in (sv, hv.variability):
            s = f(rows, detrend)
            assert s["variance"][0] == 0.0 and s["sd"][0] == 0.0 and np.isnan(s["r1"][0])
            for i in (2, 4):
                assert all(np.isnan(s[k][i]) for k in hv.NAMES)
            for i in (1, 3, 5):
                assert all(np.isfinite(s[k][i]) for k in hv.NAMES)
    line = 3.0 + 0.25 * np.arange(40, dtype=np.float64)
    for f in (lambda x, d: sv(x, d), lambda x, d: {k: v[0] for k, v in hv.variability(x[:, None], d).items()}):
        s = f(line, "linear")
        assert s["slope"] == 0.25 and s["variance"] < 1e-28
        s = f(line, "difference")
        assert s["mean"] == 0.25 and s["variance"] == 0.0 and s["slope"] == 0.0
    wild = rng.normal(0.0, 1.0, (9, 4000)) * 10.0 ** rng.integers(-8, 8, 4000)[None, :]
    for detrend in DETREND:
        assert np.nanmax(np.abs(sv(wild, detrend)["r1"])) <= 1.0 + 1e-12
    for detrend, R in (("mean", 2), ("linear", 2), ("difference", 3)):
        with pytest.raises(ValueError):
            sv(rows[:R], detrend)
    with pytest.raises(ValueError):
        sv(rows, "quadratic")
    with pytest.raises(ValueError):
        sv(np.zeros((3, 3, 3)), "mean")


def test_loglik_vectors_restatement():
    v = [np.array([1.0, np.nan, 2.0, 0.5]), np.array([0.0, 1.0, np.inf, 0.25])]
    got = hv.loglik_vectors(v, [1.5, 0.5], [0.5, 0.25])
    assert got[0] == -0.5 * ((0.5 * 0.5) / 0.25) + -0.5 * ((0.5 * 0.5) / 0.0625) and np.isneginf(got[1]) and np.isneginf(got[2])
    add = np.array([-1.0, 0.0, 0.0, -np.inf])
    got2 = hv.loglik_vectors(v, [1.5, 0.5], [0.5, 0.25], add)
    assert got2[0] == -1.0 + got[0] and np.isneginf(got2[3])


def test_header_declares_the_boundary():
    text = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", text).group(1)) >= 16
    for name, value in (("RSCM_VAR_MEAN", 0), ("RSCM_VAR_LINEAR", 1), ("RSCM_VAR_DIFFERENCE", 2)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1)) == value
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"RSCM_API\s+int\s+rscm_ens_member_variability\s*\(\s*rscm_ens\*\s*h,\s*int32_t\s+var_id,\s*int32_t\s+t_begin,\s*int32_t\s+t_end,"
                     r"\s*int32_t\s+t_stride,\s*int32_t\s+mode,\s*int32_t\s+slot,\s*void\*\*\s*out_dev\)", code)
    assert re.search(r"RSCM_API\s+int\s+rscm_ens_loglik_vectors_device\s*\(\s*rscm_ens\*\s*h,\s*int32_t\s+n_vec,\s*const\s+double\*\s*const\*\s*vec_dev,"
                     r"\s*const\s+double\*\s*value,\s*const\s+double\*\s*sigma,\s*const\s+double\*\s*add_dev,\s*void\*\*\s*out_dev\)", code)
    from rscm_amd import _lib
    assert (_lib.VAR_MEAN, _lib.VAR_LINEAR, _lib.VAR_DIFFERENCE) == (0, 1, 2)
    assert {"rscm_ens_member_variability", "rscm_ens_loglik_vectors_device"} <= set(_lib.SIGNATURES)
