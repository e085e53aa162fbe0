"""CPU tier: reference periods on calibration targets (target.rs:63-145 of the reference, whose likelihood declares the field and never
reads it) -- the target surface, and the host ``GaussianLikelihood.ln_likelihood`` against the numpy restatement of the definition
(tests/host_likelihood.py; DESIGN.md section 7, "Reference periods")."""
import math

import numpy as np
import pytest

from rscm_amd import calibrate as cal
from tests import host_likelihood as hl
from tests.host_indicators import anomaly, baseline

TIMES = np.arange(1750.0, 1951.0)


def _series(rng, n, scale=1.0):
    """[T][N] smooth warming curves that do not start at their reference-period mean."""
    t = (TIMES - 1750.0)[:, None]
    return scale * (rng.uniform(0.5, 2.0, n)[None, :] * (1.0 - np.exp(-t / rng.uniform(30.0, 200.0, n)[None, :]))
                    + 0.05 * rng.standard_normal((len(TIMES), n)))


def _output(x, i):
    return {float(t): float(v) for t, v in zip(TIMES, x[:, i])}


def _rows(start, end):
    r = [n for n, t in enumerate(TIMES) if start <= t <= end]
    return (r[0], r[-1] + 1)


# ---- surface (target.rs:320-324, tests/test_calibration_python_api.py:210-228 of the reference) ----------------------------------
def test_reference_period_surface():
    vt = cal.VariableTarget("Surface Temperature")
    assert vt.reference_period is None
    assert vt.with_reference_period(1850, 1900) is vt
    assert vt.reference_period == (1850.0, 1900.0)
    assert vt.add_relative(2020, 1.0, 0.05) is vt
    assert vt.observations[-1].uncertainty == 0.05 and vt.observations[-1].value == 1.0
    assert vt.add_relative(2021, -2.0, 0.1).observations[-1].uncertainty == 0.2
    with pytest.raises(ValueError, match="must be positive"):
        vt.add_relative(2022, 0.0, 0.1)
    with pytest.raises(ValueError):
        vt.with_reference_period(1900, 1850)

    target = cal.Target()
    assert target.add_observation_relative("temp", 2000, 100, 0.1) is target
    assert target.get_variable("temp").observations[0].uncertainty == 10.0
    target.add_observation("temp", 2010, 1.0, 0.1)
    assert target.set_reference_period("temp", 1850, 1900) is target            # on a target that already has observations
    assert target.get_variable("temp").reference_period == (1850.0, 1900.0)
    assert len(target.get_variable("temp").observations) == 2
    assert target.set_reference_period("other", 1961, 1990).get_variable("other").reference_period == (1961.0, 1990.0)  # creates it
    assert target.variable_names() == ["temp", "other"]
    assert cal.Target().add_observation("x", 1.0, 1.0, 1.0).get_variable("x").reference_period is None


# ---- known answer --------------------------------------------------------------------------------------------------------------
def test_anomalies_of_the_series_itself_score_zero():
    rng = np.random.default_rng(3)
    x = _series(rng, 1)
    r0, r1 = _rows(1850.0, 1900.0)
    b = baseline(x[r0:r1])
    assert b[0] != 0.0
    obs_t = [1800.0, 1850.0, 1875.0, 1900.0, 1901.0, 1950.0]
    sigma = 0.25
    with_p, without = cal.Target(), cal.Target()
    shifted = cal.Target()
    for t in obs_t:
        a = float(anomaly(x[[int(t - 1750)]], b)[0, 0])
        with_p.add_observation("T", t, a, sigma)
        without.add_observation("T", t, a, sigma)
        shifted.add_observation("T", t, a + sigma, sigma)
    with_p.set_reference_period("T", 1850, 1900)
    shifted.set_reference_period("T", 1850, 1900)
    lik = cal.GaussianLikelihood()
    out = {"T": _output(x, 0)}
    assert lik.ln_likelihood(out, with_p) == 0.0
    assert lik.ln_likelihood(out, without) < 0.0
    # every residual is (a + sigma) - a: one sigma up to the rounding of that sum and difference
    assert lik.ln_likelihood(out, shifted) == pytest.approx(-0.5 * len(obs_t), rel=1e-12)


def test_one_sigma_shift_is_exact_on_binary_values():
    """values on a binary grid: every operation of the definition is exact, so the shifted result is -0.5 * n_obs to the bit"""
    x = (np.arange(len(TIMES)) * 0.125)[:, None]
    r0, r1 = _rows(1850.0, 1881.0)   # 32 rows: the mean of a grid of eighths over 32 rows is exact
    b = baseline(x[r0:r1])
    target = cal.Target().set_reference_period("T", 1850, 1881)
    obs_t = [1760.0, 1850.0, 1881.0, 1940.0]
    for t in obs_t:
        target.add_observation("T", t, float(x[int(t - 1750), 0] - b[0]) + 0.5, 0.5)
    assert cal.GaussianLikelihood().ln_likelihood({"T": _output(x, 0)}, target) == -0.5 * len(obs_t)


# ---- host likelihood == numpy restatement, bit for bit -------------------------------------------------------------------------
def _problem(period_on_second=False):
    obs_t = [1790.0, 1849.0, 1850.0, 1870.0, 1900.0, 1901.0, 1930.0, 1950.0]   # before, inside and after 1850-1900
    rng = np.random.default_rng(11)
    target = cal.Target()
    for t in obs_t:
        target.add_observation("Ts", t, rng.normal(0.3, 0.3), rng.uniform(0.05, 0.4))
    for t in obs_t[::2]:
        target.add_observation("Td", t, rng.normal(0.1, 0.1), rng.uniform(0.05, 0.4))
    target.set_reference_period("Ts", 1850, 1900)
    reference = {"Ts": _rows(1850.0, 1900.0)}
    if period_on_second:
        target.set_reference_period("Td", 1800, 1820)
        reference["Td"] = _rows(1800.0, 1820.0)
    ov, ot, val, sig = [], [], [], []
    for name, vt in target.variables():
        for o in vt.observations:
            ov.append(name), ot.append(int(o.time - 1750)), val.append(o.value), sig.append(o.uncertainty)
    return target, reference, (ov, ot, val, sig)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("both", [False, True])
def test_host_likelihood_equals_numpy_restatement(normalize, both):
    n = 300
    rng = np.random.default_rng(5)
    series = {"Ts": _series(rng, n), "Td": _series(rng, n, 0.3)}
    target, reference, (ov, ot, val, sig) = _problem(both)
    want = hl.loglik(series, ov, ot, val, sig, normalize, reference)
    lik = cal.GaussianLikelihood(normalize)
    got = np.array([lik.ln_likelihood({v: _output(x, i) for v, x in series.items()}, target) for i in range(n)])
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the period matters: without it the numbers differ
    assert not np.array_equal(want, hl.loglik(series, ov, ot, val, sig, normalize, None))
    assert hl.LN_2PI == math.log(2.0 * math.pi)


def test_failed_members_and_missing_periods():
    n = 40
    rng = np.random.default_rng(6)
    series = {"Ts": _series(rng, n), "Td": _series(rng, n, 0.3)}
    series["Ts"][120, 7] = np.nan       # inside the period, not observed
    series["Ts"][130, 9] = np.inf
    target, reference, (ov, ot, val, sig) = _problem()
    want = hl.loglik(series, ov, ot, val, sig, False, reference)
    assert want[7] == -np.inf and want[9] == -np.inf and np.isfinite(np.delete(want, [7, 9])).all()
    lik = cal.GaussianLikelihood()
    for i in (7, 9):
        with pytest.raises(ValueError, match="non-finite"):
            lik.ln_likelihood({v: _output(x, i) for v, x in series.items()}, target)

    # through a runner: a failed member is -inf and the batch goes on (sampler/ensemble.rs:163-172)
    runner = cal.ModelRunner(model_factory=lambda p: {v: _output(x, int(p["i"])) for v, x in series.items()}, param_names=["i"],
                             output_variables=["Ts", "Td"])
    got = runner.log_likelihood_batch([[float(i)] for i in range(n)], target, lik)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))

    # a period with no row on the axis: KeyError on the host form (like a missing observation time), -inf through the runner
    nowhere = cal.Target().add_observation("Ts", 1900.0, 0.5, 0.1).set_reference_period("Ts", 1600, 1700)
    with pytest.raises(KeyError):
        lik.ln_likelihood({"Ts": _output(series["Ts"], 0)}, nowhere)
    assert (runner.log_likelihood_batch([[0.0], [1.0]], nowhere, lik) == -np.inf).all()
    assert (hl.loglik(series, ["Ts"], [150], [0.5], [0.1], False, {"Ts": (100, 151)}, computed=120) == -np.inf).all()


def test_a_nan_the_output_leaves_out_is_averaged_over():
    """ModelRunner.run drops NaN values from its output (extract_outputs): the host form then averages over the rows it holds"""
    rng = np.random.default_rng(8)
    x = _series(rng, 1)
    out = _output(x, 0)
    del out[1860.0]
    r0, r1 = _rows(1850.0, 1900.0)
    rows = [r for r in range(r0, r1) if TIMES[r] != 1860.0]
    b = baseline(x[rows])
    target = cal.Target().add_observation("T", 1950.0, float(x[200, 0] - b[0]), 0.1).set_reference_period("T", 1850, 1900)
    assert cal.GaussianLikelihood().ln_likelihood({"T": out}, target) == 0.0
