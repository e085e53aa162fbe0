"""Host-only tier of the seeded forcing noise of a two-layer ensemble (include/rscm_gpu.h, rscm_ens_set_forcing_noise): the numpy
restatement of the deviate (tests/host_forcing_noise.py) against scipy, CPython's statistics module and a bare Python loop, on
random draws and on chosen integers that put every branch in play; the stream's independence properties; its moments; the header's
tag; and the refusals of the Python front end that need no device.  The GPU tier (tests/test_gpu_forcing_noise.py) pins the
device to this restatement bit for bit."""
import math
import os
import re
import statistics

import numpy as np
import pytest

from tests import host_forcing_noise as hn
from tests.helpers import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
FIXED = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
ERF = "Effective Radiative Forcing"


@pytest.fixture(scope="module")
def draws():
    """k, u, z of 4096 members x 64 indices at seed 7 (262 144 draws)."""
    k = hn.k52(SEED, np.arange(4096)[:, None], np.arange(64)[None, :])
    return k, hn.uniform_from_k(k), hn.noise(SEED, np.arange(4096)[:, None], np.arange(64)[None, :])


def test_logarithm_is_within_one_ulp():
    """ln_small against math.log (correctly rounded to within an ulp itself) on 2e5 arguments log-uniform over [2^-53, 0.075] and
    on the interval's ends: within 1 ulp (measured: 1.0)."""
    rng = np.random.default_rng(0)
    p = np.exp(rng.uniform(math.log(2.0 ** -53), math.log(0.075), 200_000))
    p = np.concatenate([p, [2.0 ** -53, 0.075, 0.0625, 2.0 ** -20 * 1.4142135623730951, 2.0 ** -20 * 1.4142135623730954]])
    got = hn.ln_small(p)
    ref = np.array([math.log(x) for x in p])
    err = np.abs(got - ref) / np.spacing(np.abs(ref))
    print(f"ln_small: max {err.max():.2f} ulp")
    assert err.max() <= 1.0


def test_restatement_against_scipy(draws):
    """z against scipy.special.ndtri(u) on the 262 144 draws and the chosen integers: relative 4e-15 (the 1-ulp logarithm, whose
    error the square root halves, plus two polynomials and a rounded division; 18 ulp of margin).  Measured: 1.1e-15 on the
    draws (1.03e-15), 3.1e-16 on the chosen integers."""
    from scipy.special import ndtri
    k, u, z = draws
    for what, kk, zz in (("draws", k.ravel(), z.ravel()), ("chosen", hn.chosen_k(), hn.normal_from_k(hn.chosen_k()))):
        ref = ndtri(hn.uniform_from_k(kk))
        err = np.abs(zz - ref) / np.abs(ref)
        print(f"{what}: max relative deviation from ndtri {err.max():.3e}")
        assert err.max() <= 4e-15


def test_central_branch_is_the_stdlib_function_bit_for_bit(draws):
    k, u, z = draws
    central = np.abs(u - 0.5) <= 0.425
    assert 0.84 < central.mean() < 0.86
    nd = statistics.NormalDist()
    uu, zz = u[central][:50_000], z[central][:50_000]
    want = np.array([nd.inv_cdf(float(x)) for x in uu])
    assert_bit_equal(zz, want, "central branch against statistics.NormalDist().inv_cdf")


def test_chosen_integers_put_every_branch_in_play():
    ks = hn.chosen_k()
    top = (1 << 52) - 1
    z = hn.normal_from_k(ks)
    by_k = dict(zip(ks.tolist(), z.tolist()))
    assert by_k[0] == -by_k[top] and abs(by_k[0] + 8.2095) < 1e-4                 # the ends: |z| is bounded
    assert by_k[1 << 51] == -by_k[(1 << 51) - 1] and 0.0 < by_k[1 << 51] < 3e-16    # next to u = 1/2: q = +-2^-53
    u = hn.uniform_from_k(ks)
    q = u - 0.5
    central = np.abs(q) <= 0.425
    r = np.sqrt(-hn.ln_small(np.where(q < 0.0, u, 1.0 - u)))
    far = ~central & (r > 5.0)
    near = ~central & (r <= 5.0)
    for sign in (-1.0, 1.0):
        s = np.sign(q) == sign
        assert (central & s).sum() >= 3 and (near & s).sum() >= 4 and (far & s).sum() >= 3
    # each boundary is met from both sides by neighbouring integers
    sk = np.sort(ks)
    for mask in (central, far):
        m = mask[np.argsort(ks)]
        flips = np.flatnonzero(m[1:] != m[:-1])
        assert len(flips) == 2 and all(sk[i + 1] - sk[i] == 1 for i in flips)
    # antisymmetry: k and 2^52 - 1 - k give u and 1 - u
    assert_bit_equal(hn.normal_from_k(np.uint64(top) - ks), -z, "z(1 - u) == -z(u)")
    # monotone in k across every branch boundary
    assert (np.diff(z[np.argsort(ks)]) > 0).all()
    # continuity across |q| = 0.425 and r = 5: neighbours differ by less than 1e-9 relative
    for i in np.flatnonzero((central[np.argsort(ks)][1:] != central[np.argsort(ks)][:-1])):
        a, b = z[np.argsort(ks)][i], z[np.argsort(ks)][i + 1]
        assert abs(a - b) < 1e-9 * abs(a)


def test_vectorised_restatement_equals_a_bare_loop(draws):
    k, u, z = draws
    pick = np.concatenate([k.ravel()[:3000], hn.chosen_k()])
    want = np.array([hn.normal_from_k_loop(x) for x in pick])
    assert_bit_equal(hn.normal_from_k(pick), want, "numpy against the Python loop")


def test_stream_arguments_each_change_the_draw():
    g, t = np.arange(64)[:, None], np.arange(40)[None, :]
    base = hn.k52(SEED, g, t)
    # the two indices of one Philox block differ, and no two indices of a member share an integer
    assert (base[:, 0::2] != base[:, 1::2]).all()
    assert all(np.unique(row).size == row.size for row in base)
    for what, other in (("seed", hn.k52(SEED + 1, g, t)), ("high word of the seed", hn.k52(SEED + (1 << 32), g, t)),
                        ("member", hn.k52(SEED, g + 1, t)), ("high word of the member", hn.k52(SEED, g + (1 << 32), t)),
                        ("tag", hn.k52(SEED, g, t, tag=hn.NOISE_STREAM_TAG + 1))):
        assert (other != base).all(), what
    # z is a function of (seed, g, t) alone: evaluated one element at a time it is the broadcast result
    z = hn.noise(SEED, g, t)
    assert z[5, 9] == hn.noise(SEED, 5, 9)[()] and z[63, 39] == hn.noise(SEED, np.array([63]), np.array([39]))[0]
    F = np.zeros((4, 10))
    assert_bit_equal(hn.noisy_forcing(F, 0.1, SEED, member_offset=60), 0.0 + 0.1 * z[60:64, :10], "noisy_forcing offsets the member id")


def test_moments(draws):
    """4096 members x 64 indices at seed 7, each within 4 standard errors of a standard normal white field (n = 262 144:
    1/sqrt(n) = 0.00195, so 0.0078 for the mean and the two correlations and 4 sqrt(2/n) = 0.011 for the variance).
    Measured: mean 0.0003, variance - 1 0.0040, lag-1 over t 0.0039, neighbouring members 0.0009."""
    z = draws[2]
    mean, var = z.mean(), z.var()
    lag1 = np.mean(z[:, 1:] * z[:, :-1])
    nb = np.mean(z[1:] * z[:-1])
    print(f"mean {mean:.4f}  variance - 1 {var - 1.0:.4f}  lag-1 {lag1:.4f}  neighbouring members {nb:.4f}")
    assert abs(mean) <= 0.0078
    assert abs(var - 1.0) <= 0.011
    assert abs(lag1) <= 0.0078
    assert abs(nb) <= 0.0078


def test_header_declares_the_tag_and_it_is_its_own():
    text = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    m = re.search(r"#define\s+RSCM_NOISE_STREAM_TAG\s+(0x[0-9A-Fa-f]+)u?", text)
    assert m, "include/rscm_gpu.h does not define RSCM_NOISE_STREAM_TAG"
    tag = int(m.group(1), 16)
    resample = int(re.search(r"#define\s+RSCM_RESAMPLE_STREAM_TAG\s+(0x[0-9A-Fa-f]+)u?", text).group(1), 16)
    from tests import host_resample, host_sampler
    assert tag == hn.NOISE_STREAM_TAG and 0 < tag < 1 << 32
    assert tag not in (host_sampler.STREAM_PROPOSE, host_sampler.STREAM_ACCEPT, 0x5EED, 0xA5A5, resample, host_resample.STREAM_TAG)
    from rscm_amd import _lib
    assert _lib.NOISE_STREAM_TAG == tag
    minor = int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", text).group(1))
    assert minor >= 13
    for name in ("rscm_ens_set_forcing_noise", "rscm_ens_clear_forcing_noise", "rscm_ens_forcing_noise", "rscm_ens_forcing_noise_rows",
                 "rscm_gpu_selftest_normal"):
        assert name in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------- the front end, no device
def _two_layer(core, axis):
    from rscm_amd.two_layer import TwoLayerBuilder
    t = axis.values()
    return (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(FIXED).build())
            .with_exogenous_variable(ERF, core.Timeseries(0.03 * (np.asarray(t) - 1750.0), axis, "W/m^2", core.InterpolationStrategy.Linear))
            .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))


def test_builder_refuses_what_noise_is_no_option_of():
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    from rscm_amd.components import CarbonCycleBuilder, CO2ERFBuilder
    from rscm_amd.two_layer import TwoLayerBuilder
    axis = core.TimeAxis.from_values(np.arange(1750.0, 1791.0))
    for sigma, seed in ((-0.1, 1), (math.nan, 1), (math.inf, 1), (0.1, -1), (0.1, 1 << 64)):
        with pytest.raises(ValueError, match="with_forcing_noise"):
            _two_layer(core, axis).with_forcing_noise(sigma, seed)
    b = _two_layer(core, axis).with_forcing_noise(0.1, (1 << 64) - 1)
    assert b._noise == (0.1, (1 << 64) - 1)
    # every refusal below comes before any device call
    with pytest.raises(ValueError, match="series_window"):
        b.build(n_members=2, series_window=8)
    with pytest.raises(ValueError, match="store_series"):
        b.build(n_members=2, store_series=False)
    with pytest.raises(ValueError, match="forcing noise"):
        cal.ModelRunner(b, ["lambda0"], ["Surface Temperature"])
    schema = core.VariableSchema()
    schema.add_variable("Effective Radiative Forcing|CO2", "W/m^2")
    schema.add_aggregate(ERF, "W/m^2", "Sum", ["Effective Radiative Forcing|CO2"])
    graph = (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
             .with_rust_component(CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.02)).build())
             .with_rust_component(CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=278.0)).build())
             .with_rust_component(TwoLayerBuilder.from_parameters(FIXED).build())
             .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0, "Atmospheric Concentration|CO2": 278.0,
                                   "Cumulative Land Uptake": 0.0, "Cumulative Emissions|CO2": 0.0})
             .with_forcing_noise(0.1, 3))
    with pytest.raises(ValueError, match="GraphModel"):
        graph.build(n_members=2)

    class _Runner:   # what DeviceEnsembleSampler looks at before anything else
        param_names = ["lambda0"]
        _builder = b

    params = cal.ParameterSet()
    params.add("lambda0", cal.Uniform(0.8, 1.5))
    with pytest.raises(ValueError, match="forcing noise"):
        cal.DeviceEnsembleSampler(params, _Runner(), cal.GaussianLikelihood(), cal.Target())
