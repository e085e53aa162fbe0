"""Host-only parts of the two-layer mix ensemble (per-member forcing as a scaled sum of shared components), no device:
ModelBuilder.with_forcing_components -- the parameter order and base parameters it gives the model, the model shapes it refuses,
its TOML round trip -- and the host restatement of the forcing (tests/host_forcing_mix.py) against hand-computed cases."""
from fractions import Fraction

import numpy as np
import pytest

from tests import host_forcing_mix as hm
from tests.helpers import bits, same_values

FIXED = dict(lambda0=1.1, a=0.05, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
ERF = "Effective Radiative Forcing"


def _parts():
    from rscm_amd import core
    t = np.arange(1750.0, 1791.0)
    axis = core.TimeAxis.from_values(t)
    lin = core.InterpolationStrategy.Linear
    comps = {"ghg": core.Timeseries(0.03 * (t - 1750.0), axis, "W/m^2", lin),
             "aerosol": core.Timeseries(-0.01 * (t - 1750.0), axis, "W/m^2", lin),
             "solar": core.Timeseries(0.1 * np.sin(2.0 * np.pi * (t - 1750.0) / 11.0), axis, "W/m^2", lin)}
    return core, axis, t, comps


def _two_layer(core, axis):
    from rscm_amd.two_layer import TwoLayerBuilder
    return (core.ModelBuilder().with_time_axis(axis).with_rust_component(TwoLayerBuilder.from_parameters(FIXED).build())
            .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))


def test_param_order_and_base_params():
    core, axis, t, comps = _parts()
    b = _two_layer(core, axis)
    assert b.forcing_mix_plan() is None
    b.with_forcing_components(ERF, comps, scales={"aerosol": 0.8})
    plan = b.forcing_mix_plan()
    assert plan["names"] == ("ghg", "aerosol", "solar")
    assert plan["param_order"] == (core.TL_PARAM_ORDER + ("forcing_scale|ghg", "forcing_scale|aerosol", "forcing_scale|solar"))
    assert plan["base_params"].tolist() == [FIXED[k] for k in core.TL_PARAM_ORDER] + [1.0, 0.8, 1.0]
    assert plan["block"].shape == (3, len(t))
    for k, name in enumerate(plan["names"]):
        assert np.array_equal(plan["block"][k], comps[name].values())


def test_argument_checks():
    core, axis, t, comps = _parts()
    b = _two_layer(core, axis)
    with pytest.raises(ValueError, match="1 to 8"):
        b.with_forcing_components(ERF, {})
    with pytest.raises(ValueError, match="1 to 8"):
        b.with_forcing_components(ERF, {f"c{k}": comps["ghg"] for k in range(9)})
    with pytest.raises(ValueError, match="unknown component"):
        b.with_forcing_components(ERF, comps, scales={"volcanic": 1.0})
    with pytest.raises(TypeError):
        b.with_forcing_components(ERF, {"ghg": np.zeros(len(t))})


def test_unsupported_model_shapes_are_refused():
    core, axis, t, comps = _parts()
    from rscm_amd.components import CarbonCycleBuilder, CO2ERFBuilder
    from rscm_amd.two_layer import TwoLayerBuilder
    # another variable than the forcing the TwoLayer reads
    b = _two_layer(core, axis).with_forcing_components("Emissions|CO2|Anthropogenic", comps)
    with pytest.raises(ValueError, match="Weighted aggregate"):
        b.forcing_mix_plan()
    # the variable given twice
    b = (_two_layer(core, axis).with_forcing_components(ERF, comps)
         .with_exogenous_variable(ERF, comps["ghg"]))
    with pytest.raises(ValueError, match="also supplied"):
        b.forcing_mix_plan()
    # a graph of several components: the forcing is no exogenous series there
    schema = core.VariableSchema()
    schema.add_variable("Effective Radiative Forcing|CO2", "W/m^2")
    schema.add_aggregate(ERF, "W/m^2", "Sum", ["Effective Radiative Forcing|CO2"])
    b = (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
         .with_rust_component(CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.02)).build())
         .with_rust_component(CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=278.0)).build())
         .with_rust_component(TwoLayerBuilder.from_parameters(FIXED).build())
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0, "Atmospheric Concentration|CO2": 278.0,
                               "Cumulative Land Uptake": 0.0, "Cumulative Emissions|CO2": 0.0})
         .with_forcing_components(ERF, comps))
    with pytest.raises(ValueError, match="Weighted aggregate"):
        b.forcing_mix_plan()
    with pytest.raises(ValueError, match="Weighted aggregate"):
        b.build(n_members=2)   # refused before any device call


def test_toml_round_trip_of_the_description():
    core, axis, t, comps = _parts()
    from rscm_amd import serialise
    comps["solar"] = core.Timeseries(np.where(np.arange(len(t)) == 5, np.nan, comps["solar"].values()), axis, "W/m^2",
                                     core.InterpolationStrategy.Linear)
    b = _two_layer(core, axis).with_forcing_components(ERF, comps, scales={"ghg": 1.25, "solar": -0.0})
    text = serialise.dumps(serialise.describe_builder(b))
    assert "forcing_components" in text
    b2 = serialise.builder_from(serialise.loads(text))
    p1, p2 = b.forcing_mix_plan(), b2.forcing_mix_plan()
    assert p1["names"] == p2["names"] and p1["param_order"] == p2["param_order"]
    assert np.array_equal(bits(p1["base_params"]), bits(p2["base_params"]))   # -0.0 keeps its sign
    assert same_values(p1["block"], p2["block"]) and np.isnan(p2["block"][2, 5])
    # a description without components reads back without them
    plain = serialise.builder_from(serialise.loads(serialise.dumps(serialise.describe_builder(_two_layer(core, axis)))))
    assert plain.forcing_mix_plan() is None


def test_restated_forcing_against_hand_computed_cases():
    # K = 2.  Hand values: 1.1*1.1 = 1.2100000000000002, 0.3*-4.0 = -1.2, sum 0.010000000000000231 (fusing the first product
    # would give 0.01000000000000024); 0.1*0.3 = 0.03, 0.7*0.9 = 0.63, sum 0.66 (fusing the second: 0.6599999999999999)
    S = np.array([[1.1, 0.1], [0.3, 0.7]])            # [K][T]
    c = np.array([[1.1, 0.3], [-4.0, 0.9]])           # [K][N]
    want = np.array([[1.1 * 1.1 + 0.3 * -4.0, 0.1 * 1.1 + 0.7 * -4.0], [1.1 * 0.3 + 0.3 * 0.9, 0.1 * 0.3 + 0.7 * 0.9]])
    assert want[0, 0] == 0.010000000000000231 and want[1, 1] == 0.66
    for f in (hm.mix_forcing, hm.mix_forcing_loop):
        assert np.array_equal(bits(f(S, c)), bits(want))
    # ... each operation correctly rounded on its own: exact rational arithmetic, rounded after every product and sum
    def rounded(i, n):
        p0 = float(Fraction(float(S[0, n])) * Fraction(float(c[0, i])))
        p1 = float(Fraction(float(S[1, n])) * Fraction(float(c[1, i])))
        return float(Fraction(p0) + Fraction(p1))
    assert all(rounded(i, n) == want[i, n] for i in range(2) for n in range(2))
    # the order of summation: ((1e16 + 1) - 1e16) = 0, any other order gives 1
    S3 = np.array([[1e16], [1.0], [-1e16]])
    assert hm.mix_forcing(S3, np.ones((3, 1)))[0, 0] == 0.0 and hm.mix_forcing_loop(S3, np.ones((3, 1)))[0, 0] == 0.0
    # K = 1 is one product: -0.0 survives, nothing is added to it
    assert np.signbit(hm.mix_forcing(np.array([[0.0]]), np.array([[-1.0]]))[0, 0])
    # scenarios: member i takes the rows of scenario scen[i]; NaN and Inf propagate, nothing is skipped
    S2 = np.stack([S, 2.0 * S])
    got = hm.mix_forcing(S2, c, scen=[1, 0])
    assert np.array_equal(bits(got[0]), bits(hm.mix_forcing(2.0 * S, c[:, :1])[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    Sn = S.copy()
    Sn[1, 0] = np.nan
    assert np.isnan(hm.mix_forcing(Sn, c)[:, 0]).all() and not np.isnan(hm.mix_forcing(Sn, c)[:, 1]).any()
    assert np.isnan(hm.mix_forcing(S, np.array([[np.inf], [-np.inf]]))).all()
    assert np.array_equal(hm.mix_forcing_loop(S2, c, scen=[1, 0]), got)
