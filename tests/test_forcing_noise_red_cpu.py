"""Host-only tier of the red (AR(1)) forcing noise of a two-layer ensemble (include/rscm_gpu.h, rscm_ens_set_forcing_noise_ar1): the
statistics of the numpy restatement (tests/host_forcing_noise_red.py) -- lag-one autocorrelation, variance, the stationary start --
its independence of how an ensemble is split into handles, the refusals of the Python front end that need no device, and the
header's text.  The GPU tier (tests/test_gpu_forcing_noise_red.py) pins the device to this restatement bit for bit.

The bounds are five standard errors of the estimators under the AR(1) model with normal innovations, over n independent members:
the least-squares lag-one coefficient sum(e_t e_t+1) / sum(e_t^2) over n x 64 pairs has variance (1 - phi^2) / (n 64); the mean of
e^2 over n x 65 values relative variance 2 (1 + phi^2) / ((1 - phi^2) n 65) (the squares are correlated with phi^2 per lag); the
mean of e^2 over the n values of one index relative variance 2 / n."""
import math
import os
import re

import numpy as np
import pytest

from tests import host_forcing_noise as hn
from tests import host_forcing_noise_red as hr
from tests.helpers import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N, T, SIGMA = 20260327, 512, 65, 0.5
PHIS = (0.7, -0.5, 0.95)


@pytest.fixture(scope="module")
def series():
    """phi -> e [512][65] at seed 20260327, sigma 0.5."""
    return {phi: hr.red_noise(SEED, np.arange(N), T, SIGMA, phi) for phi in PHIS}


@pytest.mark.parametrize("phi", PHIS)
def test_lag_one_autocorrelation_is_phi(series, phi):
    e = series[phi]
    r = (e[:, :-1] * e[:, 1:]).sum() / (e[:, :-1] ** 2).sum()
    se = math.sqrt((1.0 - phi * phi) / (N * (T - 1)))
    print(f"phi {phi}: lag-one coefficient {r:.5f}, {abs(r - phi) / se:.2f} standard errors off")
    assert abs(r - phi) <= 5.0 * se


@pytest.mark.parametrize("phi", PHIS)
def test_variance_is_sigma_squared(series, phi):
    e = series[phi]
    rel = (e ** 2).mean() / SIGMA ** 2 - 1.0
    se = math.sqrt(2.0 * (1.0 + phi * phi) / ((1.0 - phi * phi) * N * T))
    print(f"phi {phi}: variance / sigma^2 - 1 = {rel:+.5f}, {abs(rel) / se:.2f} standard errors")
    assert abs(rel) <= 5.0 * se


@pytest.mark.parametrize("phi", PHIS)
def test_start_is_stationary(series, phi):
    """Var e_0 = Var e_64 = sigma^2: e_0 = sigma z_0, not z_0 scaled by the innovation's s_e, and no spin-up transient."""
    e = series[phi]
    se = math.sqrt(2.0 / N)
    for t in (0, T - 1):
        rel = (e[:, t] ** 2).mean() / SIGMA ** 2 - 1.0
        print(f"phi {phi}, index {t}: variance / sigma^2 - 1 = {rel:+.4f}, {abs(rel) / se:.2f} standard errors")
        assert abs(rel) <= 5.0 * se
    assert_bit_equal(e[:, 0], np.float64(SIGMA) * hn.noise(SEED, np.arange(N), 0), "e_0 = sigma z_0")


def test_definition_step_by_step():
    """The vectorised restatement against the definition in bare Python floats, one member."""
    phi, g = 0.7, 12345
    z = hn.noise(SEED, np.uint64(g), np.arange(T))
    c = math.sqrt(1.0 - phi * phi)
    s_e = SIGMA * c
    e = [SIGMA * float(z[0])]
    for t in range(1, T):
        e.append((phi * e[-1]) + (s_e * float(z[t])))
    assert_bit_equal(hr.red_noise(SEED, [g], T, SIGMA, phi)[0], np.array(e), "member 12345")


def test_noise_does_not_depend_on_how_the_ensemble_is_split():
    F = np.zeros((7, 20))
    a, b = 40, 5
    whole = hr.noisy_forcing_red(np.zeros((a + 7, 20)), SIGMA, 0.7, SEED)
    part = hr.noisy_forcing_red(F, SIGMA, 0.7, SEED, member_offset=a)
    assert_bit_equal(part[b], whole[a + b], "offset a, member b against offset 0, member a + b")
    big = (1 << 33) + 5
    assert_bit_equal(hr.noisy_forcing_red(F, SIGMA, -0.5, SEED, member_offset=big)[3], hr.red_noise(SEED, [big + 3], 20, SIGMA, -0.5)[0],
                     "an offset beyond 2^32")


def test_phi_zero_is_the_white_restatement():
    F = np.full((5, 12), -0.0)
    assert_bit_equal(hr.noisy_forcing_red(F, 0.0, 0.0, SEED, 3), hn.noisy_forcing(F, 0.0, SEED, 3), "sigma = 0: signed zeros")
    assert_bit_equal(hr.red_noise(SEED, np.arange(5), 12, SIGMA, 0.0), np.float64(SIGMA) * hn.noise(SEED, np.arange(5)[:, None], np.arange(12)[None, :]),
                     "phi = 0: sigma z")


def test_builder_refuses_a_phi_outside_the_open_interval():
    from rscm_amd import core
    from rscm_amd.two_layer import TwoLayerBuilder
    fixed = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    axis = core.TimeAxis.from_values(np.arange(1750.0, 1791.0))

    def builder():
        return core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(fixed).build())

    for phi in (1.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="phi"):
            builder().with_forcing_noise(0.1, 1, phi=phi)
    b = builder().with_forcing_noise(0.1, 1, phi=0.7)
    assert b._noise == (0.1, 1) and b._noise_phi == 0.7
    assert builder().with_forcing_noise(0.1, 1)._noise_phi == 0.0


def test_header_states_minor_14_and_declares_the_prototypes():
    text = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", text).group(1)) >= 14
    flat = " ".join(text.split())
    assert "int rscm_ens_set_forcing_noise_ar1(rscm_ens* h, uint64_t seed, double sigma, double phi, int64_t member_offset);" in flat
    assert "int rscm_ens_forcing_noise_ar1(const rscm_ens* h, double* phi, int32_t* cached_index);" in flat
    from rscm_amd import _lib
    for name in ("rscm_ens_set_forcing_noise_ar1", "rscm_ens_forcing_noise_ar1"):
        assert name in _lib.SIGNATURES
