"""Host-only tier of the per-member forcing noise of a two-layer ensemble (include/rscm_gpu.h, rscm_ens_set_forcing_noise_members):
the numpy restatement (tests/host_forcing_noise_members.py) against the red and white restatements it generalises, what the formula
gives for rows nobody validated, the header's text, the bindings, and the part of the Python front end that needs no device.  The
GPU tier (tests/test_gpu_forcing_noise_members.py) pins the device to this restatement bit for bit."""
import math
import os
import re

import numpy as np
import pytest

from tests import host_forcing_noise as hn
from tests import host_forcing_noise_members as hmem
from tests import host_forcing_noise_red as hr
from tests.helpers import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N, T, SIGMA = 20260327, 64, 33, 0.5
FIXED = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
ERF = "Effective Radiative Forcing"


def _z(g, n_times=T):
    return hn.noise(SEED, np.asarray(g, dtype=np.uint64)[:, None], np.arange(n_times, dtype=np.uint64)[None, :])


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("phi", [0.7, -0.5, 0.95])
def test_equal_rows_give_the_red_restatement_bit_for_bit(phi):
    g = np.arange(N) + 40
    e = hmem.member_noise(SEED, g, T, np.full(N, SIGMA), np.full(N, phi))
    assert_bit_equal(e, hr.red_noise(SEED, g, T, SIGMA, phi), f"all rows equal, phi = {phi}")
    # ... and a member's series depends on its own two numbers only
    sig = np.linspace(0.1, 0.9, N)
    ph = np.linspace(-0.9, 0.9, N)
    mixed = hmem.member_noise(SEED, g, T, sig, ph)
    for i in (0, 17, N - 1):
        assert ph[i] != 0.0
        assert_bit_equal(mixed[i], hr.red_noise(SEED, [g[i]], T, sig[i], ph[i])[0], f"member {i} on its own")


def test_phi_zero_members_have_the_white_values():
    """(0 * e) + (sigma z): the white VALUES; where sigma z is a zero its sign may differ from the white setting's, nothing else."""
    g = np.arange(N)
    sig = np.where(np.arange(N) % 5 == 0, 0.0, np.linspace(0.1, 0.9, N))
    e = hmem.member_noise(SEED, g, T, sig, np.zeros(N))
    white = sig[:, None] * _z(g)
    assert np.array_equal(e, white)   # == : -0.0 equals +0.0
    differs = e.view(np.uint64) != white.view(np.uint64)
    assert not differs[white != 0.0].any()
    assert (e[differs] == 0.0).all()
    # negative zero as phi is a zero like any other
    assert np.array_equal(hmem.member_noise(SEED, g, T, sig, np.full(N, -0.0)), white)


def test_definition_step_by_step():
    """The vectorised restatement against the definition in bare Python floats, two members with different rows."""
    for g, sigma, phi in ((12345, 0.3, 0.8), ((1 << 33) + 7, 1.7, -0.25)):
        z = hn.noise(SEED, np.uint64(g), np.arange(T))
        s = sigma * math.sqrt(1.0 - phi * phi)
        e = [sigma * float(z[0])]
        for t in range(1, T):
            e.append((phi * e[-1]) + (s * float(z[t])))
        assert_bit_equal(hmem.member_noise(SEED, [g], T, [sigma], [phi])[0], np.array(e), f"member {g}")


def test_noise_does_not_depend_on_how_the_ensemble_is_split():
    sig, ph = np.linspace(0.1, 0.9, 47), np.linspace(-0.8, 0.8, 47)
    whole = hmem.noisy_forcing_members(np.zeros((47, 20)), sig, ph, SEED)
    part = hmem.noisy_forcing_members(np.zeros((7, 20)), sig[40:], ph[40:], SEED, member_offset=40)
    assert_bit_equal(part, whole[40:], "offset 40 with the matching row slices against offset 0")


def test_special_rows_give_what_the_formula_gives():
    g = np.arange(8)
    z = _z(g)
    sig = np.array([math.nan, math.inf, 0.4, 0.4, -0.4, 0.4, 0.4, 0.4])
    phi = np.array([0.5, 0.5, 1.0, 1.5, 0.6, -1.0, math.nan, math.inf])
    e = hmem.member_noise(SEED, g, T, sig, phi)
    assert np.isnan(e[0]).all(), "NaN sigma: NaN at every index"
    assert not np.isfinite(e[1]).any() and np.isnan(e[1]).any(), "Inf sigma: Inf, then NaN where the signs meet"
    assert_bit_equal(e[2], np.full(T, 0.4 * z[2, 0]), "phi = 1: s = 0 and a constant e_0")
    assert e[3, 0] == 0.4 * z[3, 0] and np.isnan(e[3, 1:]).all(), "phi = 1.5: the square root of a negative number"
    assert_bit_equal(e[4], -hr.red_noise(SEED, [4], T, 0.4, 0.6)[0], "a negative sigma mirrors the noise")
    assert_bit_equal(e[5], 0.4 * z[5, 0] * (-1.0) ** np.arange(T), "phi = -1: alternating")
    for i in (6, 7):
        assert e[i, 0] == 0.4 * z[i, 0] and np.isnan(e[i, 1:]).all(), "NaN or Inf phi"
    # every such member ends with NaN forcing, and none of them touches another: the ordinary members of a larger set keep their bits
    assert np.isnan(hmem.noisy_forcing_members(np.ones((8, T)), sig, phi, SEED)[[0, 1, 3, 6, 7], -1]).all()
    both = hmem.member_noise(SEED, np.arange(16), T, np.r_[sig, np.full(8, 0.4)], np.r_[phi, np.full(8, 0.6)])
    assert_bit_equal(both[8:], hr.red_noise(SEED, np.arange(8, 16), T, 0.4, 0.6), "the ordinary members beside them")


# ---------------------------------------------------------------------------------------------- header and bindings
def test_header_states_minor_15_the_flag_and_the_prototypes():
    text = open(os.path.join(ROOT, "include", "rscm_gpu.h")).read()
    assert int(re.search(r"#define\s+RSCM_GPU_ABI_MINOR\s+(\d+)", text).group(1)) >= 15
    assert re.search(r"#define\s+RSCM_FLAG_NOISE_PARAMS\s+4u", text)
    flat = " ".join(text.split())
    assert "#define RSCM_TL_P_NOISE_SIGMA(K) (RSCM_TL_P_COEFF0 + (K))" in flat
    assert "#define RSCM_TL_P_NOISE_PHI(K) (RSCM_TL_P_COEFF0 + (K) + 1)" in flat
    assert "int rscm_ens_set_forcing_noise_members(rscm_ens* h, uint64_t seed, int64_t member_offset);" in flat
    assert "int rscm_ens_forcing_noise_members(const rscm_ens* h, int32_t* per_member, int32_t* sigma_row, int32_t* phi_row);" in flat
    # the header says what differs from the white setting and lists what drops the cache
    assert "sign of a zero" in flat
    for name in ("rscm_ens_set_params", "rscm_ens_set_params_aos", "rscm_ens_sample_lhs", "rscm_ens_gather_members", "rscm_ens_params_devptr"):
        assert name in flat[flat.index("THE CACHE."):flat.index("int rscm_ens_set_forcing_noise_members(")]
    import ctypes as C

    from rscm_amd import _lib
    assert _lib.FLAG_NOISE_PARAMS == 4 and _lib.TL_P_COEFF0 == 6
    assert _lib.SIGNATURES["rscm_ens_set_forcing_noise_members"] == (C.c_int, [C.c_void_p, C.c_uint64, C.c_int64])
    res, args = _lib.SIGNATURES["rscm_ens_forcing_noise_members"]
    assert res is C.c_int and len(args) == 4 and args[1:] == [C.POINTER(C.c_int32)] * 3


# ---------------------------------------------------------------------------------------------- the front end, no device
def _two_layer(core, axis):
    from rscm_amd.two_layer import TwoLayerBuilder
    return (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(FIXED).build())
            .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))


def _erf(core, axis, scale=0.03):
    t = np.asarray(axis.values())
    return core.Timeseries(scale * (t - 1750.0), axis, "W/m^2", core.InterpolationStrategy.Linear)


def test_builder_appends_the_two_parameters_after_the_scales():
    from rscm_amd import core
    axis = core.TimeAxis.from_values(np.arange(1750.0, 1791.0))
    b = _two_layer(core, axis).with_exogenous_variable(ERF, _erf(core, axis)).with_forcing_noise_parameters(9, sigma=0.3, phi=0.6)
    assert b._noise == (0.3, 9) and b._noise_phi == 0.6 and b._noise_params
    plan = b.forcing_noise_plan()
    assert plan["per_member"] and plan["seed"] == 9
    assert plan["param_order"] == tuple(core.TL_PARAM_ORDER) + ("forcing_noise|sigma", "forcing_noise|phi")
    assert_bit_equal(plan["base_params"], np.array([FIXED[k] for k in core.TL_PARAM_ORDER] + [0.3, 0.6]), "base values")
    # the defaults, and a mix builder: after the forcing_scale|* names
    m = (_two_layer(core, axis).with_forcing_components(ERF, {"ghg": _erf(core, axis), "aerosol": _erf(core, axis, -0.01)}, {"aerosol": 0.8})
         .with_forcing_noise_parameters(11))
    plan = m.forcing_noise_plan()
    assert plan["param_order"] == tuple(core.TL_PARAM_ORDER) + ("forcing_scale|ghg", "forcing_scale|aerosol", "forcing_noise|sigma", "forcing_noise|phi")
    assert_bit_equal(plan["base_params"], np.array([FIXED[k] for k in core.TL_PARAM_ORDER] + [1.0, 0.8, 0.0, 0.0]), "mix base values")
    assert m.forcing_mix_plan()["param_order"] == plan["param_order"]
    # the handle-wide call after it takes the two names away again, and a builder without noise has no plan
    assert b.with_forcing_noise(0.3, 9, phi=0.6).forcing_noise_plan()["param_order"] == tuple(core.TL_PARAM_ORDER)
    assert not b._noise_params
    assert _two_layer(core, axis).forcing_noise_plan() is None


def test_builder_validates_the_base_values_and_keeps_the_refusals():
    from rscm_amd import calibrate as cal
    from rscm_amd import core
    axis = core.TimeAxis.from_values(np.arange(1750.0, 1791.0))

    def builder():
        return _two_layer(core, axis).with_exogenous_variable(ERF, _erf(core, axis))

    for kw in (dict(sigma=-0.1), dict(sigma=math.nan), dict(sigma=math.inf)):
        with pytest.raises(ValueError, match="sigma"):
            builder().with_forcing_noise_parameters(1, **kw)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            builder().with_forcing_noise_parameters(seed)
    for phi in (1.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="phi"):
            builder().with_forcing_noise_parameters(1, phi=phi)
    b = builder().with_forcing_noise_parameters((1 << 64) - 1, sigma=0.2, phi=-0.4)
    # every refusal below comes before any device call
    with pytest.raises(ValueError, match="series_window"):
        b.build(n_members=2, series_window=8)
    with pytest.raises(ValueError, match="store_series"):
        b.build(n_members=2, store_series=False)
    with pytest.raises(ValueError, match="store_series"):
        b.forcing_noise_plan(store_series=False)
    with pytest.raises(ValueError, match="forcing noise"):
        cal.ModelRunner(b, ["lambda0"], ["Surface Temperature"])

    class _Runner:   # what DeviceEnsembleSampler looks at before anything else
        param_names = ["lambda0"]
        _builder = b

    params = cal.ParameterSet()
    params.add("lambda0", cal.Uniform(0.8, 1.5))
    with pytest.raises(ValueError, match="forcing noise"):
        cal.DeviceEnsembleSampler(params, _Runner(), cal.GaussianLikelihood(), cal.Target())
