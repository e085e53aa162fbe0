"""GPU tier (-m gpu): linked inputs (rscm_ens_link_input) -- component graphs assembled from
ensembles whose inputs are other ensembles' device-resident series, stepped in graph order like
Model::step (crates/rscm-core/src/model/runtime.rs:368-527).

Parity bars:
  * CarbonCycle -> CO2ERF -> Sum -> TwoLayer assembled from four linked ensembles and stepped in
    lock-step: BIT-EXACT against the fused RSCM_KIND_COUPLED kernel (same arithmetic, same device
    math library), which tests/test_gpu_parity.py holds against the CPU oracle.
  * a linked row that carries the same numbers as a scenario-table row gives the same bits as
    the table (two-layer, CH4 chemistry, CO2 budget, ocean carbon, ClimateUDEB), and to the last-place
    error of sqrt / log / pow (1e-13 relative) for GhgForcing, whose table rows are built with
    the host's libm.
  * aggregate kind: exact against numpy restatements of compute_aggregate (schema.rs:760-802).
"""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_support import ra  # noqa: F401
from tests.helpers import assert_bit_equal, axis_values, coupled_params, emissions_syn, f_syn, magicc_chain, two_layer_params
from tests.host_lockstep import read_at_steps, relative_error

pytestmark = pytest.mark.gpu


class Stream:
    def __init__(self):
        from rscm_amd import _lib as L
        self.L, self.h = L, C.c_void_p()
        L.check(L.load().rscm_gpu_stream_create(0, C.byref(self.h)))

    def close(self):
        self.L.check(self.L.load().rscm_gpu_stream_destroy(0, self.h))


def _bounds(t):
    return np.append(t, t[-1] + (t[-1] - t[-2]))


def _coupled_graph(ra, t, P, E, stream):
    """The notebook's graph (registration order CarbonCycle, CO2ERF, TwoLayer + Sum aggregate)."""
    N, b = P.shape[1], _bounds(t)
    cc = ra.Ensemble(ra.KIND_CARBON_CYCLE, N, b)
    ce = ra.Ensemble(ra.KIND_CO2_ERF, N, b)
    ag = ra.Ensemble(ra.KIND_AGGREGATE, N, b)
    tl = ra.Ensemble(ra.KIND_TWO_LAYER, N, b)
    for e in (cc, ce, ag, tl):
        e.set_stream(stream.h.value)
    cc.set_params(P[[6, 7, 8]])
    ce.set_params(P[[9, 7]])
    ag.set_params(np.zeros((9, N)))  # Sum
    tl.set_params(P[:6])
    cc.set_forcing(np.stack([E, np.full(len(t), np.nan)]))
    for var, v in (("Atmospheric Concentration|CO2", 278.0), ("Cumulative Land Uptake", 0.0),
                   ("Cumulative Emissions|CO2", 0.0)):
        cc.set_initial(var, v)
    tl.set_initial("Surface Temperature", 0.0)
    tl.set_initial("Deep Ocean Temperature", 0.0)
    # CarbonCycle is registered before TwoLayer: it sees Ts as Exogenous (index n, lagged feedback)
    cc.link_input("Surface Temperature", tl, "Surface Temperature", ra.SRC_EXOGENOUS)
    ce.link_input(0, cc, "Atmospheric Concentration|CO2", ra.SRC_UPSTREAM)
    ag.link_input(0, ce, "Effective Radiative Forcing|CO2", ra.SRC_UPSTREAM)
    tl.link_input(0, ag, "aggregate", ra.SRC_UPSTREAM)
    return cc, ce, ag, tl


@pytest.mark.parametrize("mode", [0, 1])
def test_linked_graph_reproduces_fused_coupled_chain(ra, mode):
    """Either arithmetic: RSCM_MODE_FAST changes CarbonCycle and TwoLayer, in the fused kind and as linked components alike."""
    t = axis_values(1750, 2100)
    N = 3000
    P = coupled_params(N)
    E = emissions_syn(t)
    with ra.Ensemble(ra.KIND_COUPLED, N, _bounds(t)) as f:
        f.set_mode(mode)
        f.set_params(P)
        f.set_forcing(E)
        for var, v in (("Atmospheric Concentration|CO2", 278.0), ("Cumulative Land Uptake", 0.0),
                       ("Cumulative Emissions|CO2", 0.0), ("Surface Temperature", 0.0),
                       ("Deep Ocean Temperature", 0.0)):
            f.set_initial(var, v)
        f.run()
        want = {k: f.get_series(k) for k in f.var_ids if f.var_ids[k] > 0}
        want_status = f.status()
    s = Stream()
    cc, ce, ag, tl = _coupled_graph(ra, t, P, E, s)
    try:
        for e in (cc, ce, ag, tl):
            e.set_mode(mode)
        for n in range(len(t) - 1):  # Model::step: every component once, in graph order
            for e in (cc, ce, ag, tl):
                e.run(n + 1, sync=False)
        tl.sync()
        got = {"Surface Temperature": tl.get_series("Surface Temperature"),
               "Deep Ocean Temperature": tl.get_series("Deep Ocean Temperature"),
               "Atmospheric Concentration|CO2": cc.get_series(1), "Cumulative Land Uptake": cc.get_series(2),
               "Cumulative Emissions|CO2": cc.get_series(3),
               "Effective Radiative Forcing|CO2": ce.get_series(1), "Effective Radiative Forcing": ag.get_series(1)}
        assert set(got) == set(want)
        for k in want:
            assert_bit_equal(got[k], want[k], k)
        assert np.array_equal((cc.status() | tl.status()) != 0, want_status != 0)
        # a producer cannot go while a consumer still reads it
        with pytest.raises(Exception, match="linked input"):
            ag.close()
        # stepping out of graph order is caught: the aggregate has not produced index n+1 yet
        for e in (cc, ce, ag, tl):
            e.rewind()
        cc.run(1)
        ce.run(1)
        with pytest.raises(Exception, match="only been stepped"):
            tl.run(1)
    finally:
        # consumers first; the feedback edge CarbonCycle <- TwoLayer is cut by hand
        cc.unlink_input("Surface Temperature")
        for e in (tl, ag, ce, cc):
            e.close()
        s.close()


def test_linked_row_equals_table_row(ra):
    """Feed-forward: a producer run over the whole axis, then the consumer.  The linked row holds
    the numbers the table held, so the consumer's results carry the same bits."""
    t = axis_values(1750, 2050)
    N, b = 2000, _bounds(t)
    s = Stream()
    rng = np.random.default_rng(5)
    # producer: an aggregate that just passes one exogenous series through, shifted to index n+1
    F = f_syn(t)
    src = ra.Ensemble(ra.KIND_AGGREGATE, N, b)
    src.set_stream(s.h.value)
    src.set_params(np.zeros((9, N)))
    blk = np.full((8, len(t)), np.nan)
    blk[0] = F
    src.set_forcing(blk)
    src.run()
    out = src.get_series("aggregate")
    assert np.isnan(out[0]).all() and np.array_equal(out[1:], np.broadcast_to(F[1:, None], (len(t) - 1, N)))
    P = two_layer_params(N)
    res = {}
    for mode in ("table", "linked"):
        for src_kind in (ra.SRC_EXOGENOUS, ra.SRC_UPSTREAM):
            with ra.Ensemble(ra.KIND_TWO_LAYER, N, b) as e:
                e.set_stream(s.h.value)
                e.set_params(P)
                e.set_initial(1, 0.0)
                e.set_initial(2, 0.0)
                if mode == "table":
                    # the producer's series: NaN at index 0, F afterwards
                    e.set_forcing(np.concatenate([[np.nan], F[1:]]), None, src_kind)
                else:
                    e.link_input(0, src, "aggregate", src_kind)
                e.run()
                res[mode, src_kind] = e.get_series(1)
    for k in (ra.SRC_EXOGENOUS, ra.SRC_UPSTREAM):
        assert_bit_equal(res["linked", k], res["table", k], f"two-layer source {k}")
    assert np.isnan(res["linked", ra.SRC_EXOGENOUS][1:]).all()      # F[0] = NaN poisons the exogenous reading
    assert np.isfinite(res["linked", ra.SRC_UPSTREAM][1:, :10]).all()
    src.close()
    s.close()
    del rng


@pytest.mark.parametrize("kind_name", ["ch4", "co2_budget", "ocean", "udeb", "ghg_olbl", "ghg_ipcctar"])
def test_linked_inputs_of_magicc_kinds(ra, kind_name):
    """One input row per kind is produced on the device (an aggregate passing a per-member series
    through) and linked; the same numbers in the scenario table give the reference result."""
    from rscm_amd import _lib as L
    from rscm_amd import magicc
    t = axis_values(1850, 1950)
    T, N, b = len(t), 512, _bounds(t)
    s = Stream()
    yrs = t - t[0]
    if kind_name == "ch4":
        kind, comp = ra.KIND_CH4_CHEMISTRY, magicc.CH4ChemistryBuilder.from_parameters({}).build()
        block = np.stack([300.0 + 2.0 * yrs, 0.01 * yrs, 40.0 + 0.1 * yrs, 500.0 + yrs, 100.0 + 0.5 * yrs])
        row, init = 1, {"Atmospheric Concentration|CH4": 800.0}
    elif kind_name == "co2_budget":
        kind, comp = ra.KIND_CO2_BUDGET, magicc.CO2BudgetBuilder.from_parameters({}).build()
        block = np.stack([0.05 * yrs, 1.0 + 0.0 * yrs, 0.01 * yrs, 0.02 * yrs])
        row, init = 2, {"Atmospheric Concentration|CO2": 280.0}
    elif kind_name == "ocean":
        kind, comp = ra.KIND_OCEAN_CARBON, magicc.OceanCarbonBuilder.from_parameters({}).build()
        block = np.stack([280.0 + 0.8 * yrs, 0.005 * yrs])
        row, init = 0, {"Ocean Surface pCO2": 280.0, "Cumulative Ocean Uptake": 0.0}
    elif kind_name == "udeb":
        kind, comp = ra.KIND_UDEB, magicc.ClimateUDEBBuilder.from_parameters({}).build()
        block = (3.0 * (1.0 - np.exp(-yrs / 40.0)))[None]
        row, init = 0, {}
    else:
        method = "Olbl" if kind_name == "ghg_olbl" else "Ipcctar"
        kind, comp = ra.KIND_GHG_FORCING, magicc.GhgForcingBuilder.from_parameters({"method": method}).build()
        block = np.stack([278.0 + 1.5 * yrs, 722.0 + 9.0 * yrs, 270.0 + 0.5 * yrs])
        row, init = 1, {}
    params = np.repeat(np.asarray(comp.param_vector(), dtype=np.float64)[:, None], N, axis=1)
    # the linked row varies per member; scenario s of the table run is member s
    scale = 1.0 + 0.05 * np.arange(N) / N
    per_member = block[row][None, :] * scale[:, None]            # [N][T]
    prod = ra.Ensemble(ra.KIND_AGGREGATE, N, b)
    prod.set_stream(s.h.value)
    prod.set_params(np.zeros((9, N)))
    # the pass-through writes index n+1 from index n+1 of its table: give it one scenario per member
    blk = np.full((N, 8, T), np.nan)
    blk[:, 0, :] = per_member
    prod.set_forcing(blk, np.arange(N, dtype=np.int32))
    prod.set_state("aggregate", 0, per_member[:, 0])               # index 0 is nobody's output
    prod.run()
    assert np.array_equal(prod.get_series("aggregate"), per_member.T)

    def run(linked):
        with ra.Ensemble(kind, N, b) as e:
            e.set_stream(s.h.value)
            e.set_params(params)
            for name, v in init.items():
                e.set_initial(name, v)
            if kind == ra.KIND_UDEB:
                for vname, vid in e.var_ids.items():
                    if 1 <= vid <= 4:
                        e.set_initial(vid, 0.0)
            if linked:
                if block.shape[0] > 1:
                    e.set_forcing(block[None] if e.input_rows else block)
                e.link_input(row, prod, "aggregate", ra.SRC_EXOGENOUS)
            else:
                full = np.repeat(block[None], N, axis=0)
                full[:, row, :] = per_member
                e.set_forcing(full if e.input_rows else full[:, 0, :], np.arange(N, dtype=np.int32))
            e.run()
            return {name: e.get_series(vid) for name, vid in e.var_ids.items() if vid > 0}, e.status()

    want, st_w = run(False)
    got, st_g = run(True)
    assert np.array_equal(st_w, st_g)
    for name in want:
        if kind == ra.KIND_GHG_FORCING:
            assert np.allclose(got[name], want[name], rtol=1e-13, atol=1e-15, equal_nan=True), name
        else:
            assert_bit_equal(got[name], want[name], f"{kind_name} {name}")
    assert np.isfinite(got[next(iter(got))][1:]).all()
    del L
    prod.close()
    s.close()


def test_aggregate_operations(ra):
    t = axis_values(2000, 2010)
    T, N, b = len(t), 300, _bounds(t)
    rng = np.random.default_rng(9)
    rows = rng.normal(size=(8, T))
    rows[5:] = np.nan          # three unused contributors
    rows[2, 4] = np.nan        # a hole in a used one
    rows[:5, 7] = np.nan       # a year where every contributor is NaN
    w = rng.uniform(0.5, 2.0, size=(8, N))
    for op, name in enumerate(("Sum", "Mean", "Weighted")):
        with ra.Ensemble(ra.KIND_AGGREGATE, N, b) as e:
            e.set_params(np.concatenate([np.full((1, N), float(op)), w]))
            e.set_forcing(rows)
            e.run()
            got = e.get_series("aggregate")
        want = np.full((T, N), np.nan)
        for n in range(1, T):
            acc, cnt = np.zeros(N), 0
            for k in range(8):
                v = rows[k, n]
                if not np.isnan(v):
                    acc = acc + (v * w[k] if name == "Weighted" else v)
                    cnt += 1
            if cnt:
                want[n] = acc / float(cnt) if name == "Mean" else acc
        assert_bit_equal(got, want, name)


def test_link_argument_errors(ra):
    t = axis_values(2000, 2010)
    b = _bounds(t)
    with ra.Ensemble(ra.KIND_TWO_LAYER, 8, b) as a, ra.Ensemble(ra.KIND_TWO_LAYER, 9, b) as c, \
            ra.Ensemble(ra.KIND_TWO_LAYER, 8, b) as d, ra.Ensemble(ra.KIND_COUPLED, 8, b) as f:
        with pytest.raises(Exception, match="same members"):
            a.link_input(0, c, 1)
        with pytest.raises(Exception, match="itself"):
            a.link_input(0, a, 1)
        with pytest.raises(Exception, match="no stored series"):
            a.link_input(0, d, 0)
        with pytest.raises(Exception, match="out of range"):
            a.link_input(1, d, 1)
        with pytest.raises(Exception, match="cannot be linked"):
            f.link_input(0, d, 1)
        a.link_input(0, d, 1)
        a.set_params(two_layer_params(8))
        a.set_initial(1, 0.0)
        a.set_initial(2, 0.0)
        with pytest.raises(Exception, match="another stream"):
            a.run()
        a.unlink_input(0)
        with pytest.raises(Exception, match="not set"):
            a.run()


def test_graph_model_vs_generic_stepper_every_registration_order(ra):
    """ModelBuilder.build() on graphs without a fused kernel: one linked ensemble per component,
    stepped in the reference's breadth-first order.  Oracle: oracle/reference_model.py (the generic
    stepper restated from runtime.rs / builder.rs), every registration order of the notebook's three
    components, two aggregates with an exogenous contributor.  exp/log come from the device math
    library: 1e-11 relative, NaN pattern exact."""
    import itertools
    import rscm_amd.core as core
    from oracle import reference_model as rm
    from rscm_amd.components import CarbonCycleBuilder, CO2ERFBuilder
    from rscm_amd.two_layer import TwoLayerBuilder
    t = np.arange(1750.0, 1901.0)
    tl = dict(lambda0=1.1, a=0.02, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    make = {"CarbonCycle": lambda: CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.1)).build(),
            "CO2ERF": lambda: CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=278.0)).build(),
            "TwoLayer": lambda: TwoLayerBuilder.from_parameters(tl).build()}
    ref = {"CarbonCycle": lambda: rm.CarbonCycle(25.0, 278.0, 0.1), "CO2ERF": lambda: rm.CO2ERF(3.7, 278.0),
           "TwoLayer": lambda: rm.TwoLayer(*[tl[k] for k in core.TL_PARAM_ORDER])}
    init = {"Cumulative Land Uptake": 0.0, "Cumulative Emissions|CO2": 0.0, "Atmospheric Concentration|CO2": 278.0,
            "Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}
    agg = [("Effective Radiative Forcing", "Sum", ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other"]),
           ("Diagnostic", "Mean", ["Surface Temperature", "Deep Ocean Temperature"])]
    emis, other = emissions_syn(t) + 2.0, 0.3 * np.sin(t / 7.0)
    ran, refused = [], []
    for perm in itertools.permutations(make):
        schema = core.VariableSchema()
        for n in list(init) + ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other", "Emissions|CO2|Anthropogenic"]:
            schema.add_variable(n, "")
        for name, op, contributors in agg:
            schema.add_aggregate(name, "", op, contributors)
        axis = core.TimeAxis.from_values(t)
        b = core.ModelBuilder().with_time_axis(axis).with_schema(schema)
        for k in perm:
            b.with_rust_component(make[k]())
        b.with_initial_values(init)
        b.with_exogenous_variable("Emissions|CO2|Anthropogenic", core.Timeseries(emis, axis, "", core.InterpolationStrategy.Linear))
        b.with_exogenous_variable("Effective Radiative Forcing|Other", core.Timeseries(other, axis, "", core.InterpolationStrategy.Linear))
        try:
            model = b.build(n_members=3)
        except NotImplementedError as e:
            refused.append((perm, str(e)))
            continue
        assert isinstance(model, core.GraphModel)
        m = rm.ModelBuilder(axis=rm.TimeAxis.from_values(t), components=[ref[k]() for k in perm], aggregates=agg,
                            initial_values=init, schema_variables=["Effective Radiative Forcing|Other"],
                            exogenous={"Emissions|CO2|Anthropogenic": rm.ExoSeries(list(emis), rm.TimeAxis.from_values(t)),
                                       "Effective Radiative Forcing|Other": rm.ExoSeries(list(other), rm.TimeAxis.from_values(t))}).build()
        # half the axis step by step, the rest in one go
        for _ in range(40):
            model.step()
        model.run()
        m.run()
        assert model.finished()
        got = model.timeseries(member=2)
        for name, want in m.data.items():
            g, w = got.get_timeseries_by_name(name).values(), np.array(want)
            assert (np.isnan(g) == np.isnan(w)).all(), (perm, name)
            ok = ~np.isnan(w)
            assert (np.abs(g[ok] - w[ok]) <= 1e-11 * np.maximum(1.0, np.abs(w[ok]))).all(), (perm, name)
        ran.append(perm)
        model.close()
    # the notebook's order is among those that run; whatever is refused is refused for a stated reason
    assert ("CarbonCycle", "CO2ERF", "TwoLayer") in ran and len(ran) >= 3, (ran, refused)
    for perm, why in refused:
        assert "not reachable" in why, (perm, why)


@pytest.mark.parametrize("aerosol_first", [True, False])
def test_graph_model_magicc_lite_chain_with_feedback(ra, aerosol_first):
    """CH4Chemistry -> GhgForcing <- N2OChemistry, AerosolIndirect, Sum of four forcings -> TwoLayer,
    with the surface temperature fed back (lagged: TwoLayer is registered last) into the methane
    lifetime.  Oracle: the generic stepper with the C oracles' single-step functions as components
    (oracle/reference_model.py).  Device pow/log/exp: 1e-11 relative; NaN pattern exact.

    The reference steps components in petgraph's breadth-first order, which is not a topological
    one: with AerosolIndirect registered after the chemistry, the aggregate (two edges from the
    root) runs before GhgForcing (also two edges, but visited later) and finds NaN where the three
    greenhouse-gas forcings of the step will be -- its Sum then holds the aerosol term only.
    Registered first, the order is topological.  Both cases must come out as the stepper has them."""
    import rscm_amd.core as core
    from oracle import cbind
    from oracle import reference_model as rm
    from rscm_amd import magicc
    from rscm_amd.two_layer import TwoLayerBuilder
    t = np.arange(1850.0, 1951.0)
    yrs = t - t[0]
    tl = dict(lambda0=1.2, a=0.0, efficacy=1.1, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    exo = {"Emissions|CH4": 250.0 + 3.0 * yrs, "Emissions|NOx": 30.0 + 0.2 * yrs, "Emissions|CO": 400.0 + 2.0 * yrs,
           "Emissions|NMVOC": 80.0 + 0.5 * yrs, "Emissions|N2O": 8.0 + 0.05 * yrs,
           "Atmospheric Concentration|CO2": 285.0 + 0.3 * yrs + 0.004 * yrs ** 2,
           "Emissions|SOx": 5.0 + 0.6 * yrs, "Emissions|OC": 12.0 + 0.1 * yrs}
    init = {"Atmospheric Concentration|CH4": 800.0, "Atmospheric Concentration|N2O": 273.0,
            "Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}
    contributors = ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|CH4", "Effective Radiative Forcing|N2O",
                    "Effective Radiative Forcing|Aerosol|Indirect"]
    comps = [magicc.CH4ChemistryBuilder.from_parameters({"include_temp_feedback": True}).build(),
             magicc.N2OChemistryBuilder.from_parameters({"strat_delay": 3}).build(),
             magicc.GhgForcingBuilder.from_parameters({"method": "Olbl"}).build(),
             magicc.AerosolIndirectBuilder.from_parameters({}).build(),
             TwoLayerBuilder.from_parameters(tl).build()]
    ref_of = {"CH4Chemistry": rm.CH4Chemistry, "N2OChemistry": rm.N2OChemistry, "GhgForcing": rm.GhgForcing,
              "AerosolIndirect": rm.AerosolIndirect}
    if aerosol_first:
        comps = [comps[3]] + comps[:3] + comps[4:]
    schema = core.VariableSchema()
    for n in list(exo) + list(init) + contributors + ["Lifetime|CH4", "Lifetime|N2O"]:
        schema.add_variable(n, "")
    schema.add_aggregate("Effective Radiative Forcing", "W/m^2", "Sum", contributors)
    axis = core.TimeAxis.from_values(t)
    b = core.ModelBuilder().with_time_axis(axis).with_schema(schema).with_initial_values(init)
    for c in comps:
        b.with_rust_component(c)
    for name, vals in exo.items():
        b.with_exogenous_variable(name, core.Timeseries(vals, axis, "", core.InterpolationStrategy.Linear))
    model = b.build()
    assert isinstance(model, core.GraphModel) and not model._feed_forward
    assert model.variable_sources()[("Surface Temperature", "CH4Chemistry")] == "Exogenous"      # lagged feedback
    assert model.variable_sources()[("Atmospheric Concentration|CH4", "GhgForcing")] == "UpstreamOutput"
    model.run()
    got = model.timeseries()
    ref = rm.ModelBuilder(
        axis=rm.TimeAxis.from_values(t),
        components=[ref_of[c.type_name](c.param_vector()) for c in comps[:4]] + [rm.TwoLayer(*[tl[k] for k in core.TL_PARAM_ORDER])],
        aggregates=[("Effective Radiative Forcing", "Sum", contributors)], initial_values=init,
        exogenous={k: rm.ExoSeries(list(v), rm.TimeAxis.from_values(t)) for k, v in exo.items()}).build()
    ref.run()
    assert [n for n in model._order] == [ref.order_nodes[i].type_name for i in ref._bfs() if ref.order_nodes[i] is not None]
    for name, want in ref.data.items():
        g, w = got.get_timeseries_by_name(name).values(), np.array(want)
        assert (np.isnan(g) == np.isnan(w)).all(), name
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= 1e-11 * np.maximum(1.0, np.abs(w[ok]))).all(), (name, np.abs(g[ok] - w[ok]).max())
    ts = got.get_timeseries_by_name("Surface Temperature").values()
    erf = got.get_timeseries_by_name("Effective Radiative Forcing").values()
    aer = got.get_timeseries_by_name("Effective Radiative Forcing|Aerosol|Indirect").values()
    order = list(model._order)
    assert got.get_timeseries_by_name("Atmospheric Concentration|CH4").values()[-1] > 900.0
    if aerosol_first:
        assert order.index("GhgForcing") < order.index("Aggregator:Effective Radiative Forcing")
        assert ts[-1] > 0.2 and (erf[1:] > aer[1:]).all()
    else:
        assert order.index("GhgForcing") > order.index("Aggregator:Effective Radiative Forcing")
        assert np.array_equal(erf[1:], 0.0 + aer[1:]) and ts[-1] < 0.0
    # the temperature feedback is live: without it the methane path differs
    k_ch4 = [c.type_name for c in comps].index("CH4Chemistry")
    comps[k_ch4] = magicc.CH4ChemistryBuilder.from_parameters({"include_temp_feedback": False}).build()
    b2 = core.ModelBuilder().with_time_axis(axis).with_schema(schema).with_initial_values(init)
    for c in comps:
        b2.with_rust_component(c)
    for name, vals in exo.items():
        b2.with_exogenous_variable(name, core.Timeseries(vals, axis, "", core.InterpolationStrategy.Linear))
    m2 = b2.build()
    m2.run()
    ch4_b = m2.timeseries().get_timeseries_by_name("Atmospheric Concentration|CH4").values()
    diff = np.abs(ch4_b - got.get_timeseries_by_name("Atmospheric Concentration|CH4").values())[-1]
    # the feedback acts on warming only (delta_t = max(T, 0)): under cooling it is tau0 / (tau0 / tau + 0), tau to rounding
    # -- the kernel carries 1/tau and forms fma(tau0, 1/tau, 0) * (1/tau0): one rounding per factor, i.e. a
    # relative difference of a few ulp in the lifetime, which the contractive recurrence does not amplify:
    # bounded here by 16 ulp of the concentration (measured on an MI355X: 1 ulp)
    print(f"CH4 no-warming feedback difference: {diff:.3e} ({diff / np.spacing(ch4_b[-1]):.1f} ulp)")
    assert diff > 1e-3 if aerosol_first else diff <= 16 * np.spacing(ch4_b[-1])
    m2.close()
    model.close()
    del cbind


@pytest.mark.parametrize("execution_order", ["reference", "topological"])
def test_full_emissions_driven_magicc_graph_closed_loop(ra, execution_order):
    """The reference's emissions-driven MAGICC model (tests/regression/test_ghg_forcing.py:399-563:
    the ten rscm-magicc components in its registration order, FourBox surface temperature read as a
    scalar, FourBox aerosol forcing stored as a scalar, Sum of eight forcings) on synthetic
    emissions, as ten linked ensembles plus two grid transforms and the aggregate.

    Closed-loop check: every component's outputs are recomputed by its CPU oracle from the inputs
    that component saw -- the device's own series, picked by the reference's rules restated here
    (exogenous and lagged reads at index n, upstream reads at n+1 -- NaN if the producer runs later
    in the execution order; ClimateUDEB at n and n+1; aggregates at n+1 with NaN skipped; FourBox
    -> scalar = sum of value * 0.25) -- and must agree with what the device stored.  Tolerances are
    those of the single-component GPU tests."""
    import rscm_amd.core as core
    from oracle import cbind as orc
    from rscm_amd import _lib as L
    from rscm_amd import magicc as B
    t = np.arange(1750.0, 1831.0)
    T, yrs, b = len(t), t - 1750.0, _bounds(t)
    exo = {"Emissions|CO2|Fossil": 0.08 * yrs, "Emissions|CO2|Land Use": 0.5 + 0.0 * yrs, "Emissions|CH4": 200.0 + 2.0 * yrs,
           "Emissions|N2O": 7.0 + 0.05 * yrs, "Emissions|NOx": 10.0 + 0.2 * yrs, "Emissions|CO": 300.0 + 2.0 * yrs,
           "Emissions|NMVOC": 60.0 + 0.5 * yrs, "Emissions|SOx": 2.0 + 0.1 * yrs, "Emissions|BC": 2.5 + 0.02 * yrs,
           "Emissions|OC": 10.0 + 0.1 * yrs, "EESC": 1400.0 + 3.0 * yrs}
    init = {"Atmospheric Concentration|CO2": 278.0, "Atmospheric Concentration|CH4": 722.0, "Atmospheric Concentration|N2O": 270.0,
            "Surface Temperature": 0.0, "Ocean Surface pCO2": 278.0, "Cumulative Ocean Uptake": 0.0,
            "Carbon Pool|Plant": 884.86, "Carbon Pool|Detritus": 92.77, "Carbon Pool|Soil": 1681.53, "Carbon Pool|Humus": 836.0,
            "Effective Radiative Forcing": 0.0}  # ClimateUDEB reads the aggregate at_start of step 0
    contributors = ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|CH4", "Effective Radiative Forcing|N2O",
                    "Effective Radiative Forcing|O3|Stratospheric", "Effective Radiative Forcing|O3|Tropospheric",
                    "Effective Radiative Forcing|O3|Temperature Feedback", "Effective Radiative Forcing|Aerosol|Direct",
                    "Effective Radiative Forcing|Aerosol|Indirect"]
    schema = core.VariableSchema()
    scalars = list(exo) + [k for k in init if k not in ("Surface Temperature", "Effective Radiative Forcing")] + contributors + [
        "Heat Uptake", "Ocean Heat Content", "Sea Surface Temperature", "Carbon Flux|Terrestrial", "Carbon Flux|Ocean",
        "Emissions|CO2|Net", "Airborne Fraction|CO2", "Lifetime|CH4", "Lifetime|N2O"]
    for n in scalars:
        schema.add_variable(n, "")
    schema.add_variable("Surface Temperature", "K", core.GridType.FourBox)
    schema.add_aggregate("Effective Radiative Forcing", "W/m^2", "Sum", contributors)
    comps = [B.CH4ChemistryBuilder.from_parameters({}).build(), B.N2OChemistryBuilder.from_parameters({}).build(),
             B.GhgForcingBuilder.from_parameters({"method": "Ipcctar"}).build(), B.OzoneForcingBuilder.from_parameters({}).build(),
             B.AerosolDirectBuilder.from_parameters({}).build(), B.AerosolIndirectBuilder.from_parameters({}).build(),
             B.ClimateUDEBBuilder.from_parameters({}).build(), B.TerrestrialCarbonBuilder.from_parameters({}).build(),
             B.OceanCarbonBuilder.from_parameters({}).build(), B.CO2BudgetBuilder.from_parameters({}).build()]
    by_name = {c.type_name: c for c in comps}
    axis = core.TimeAxis.from_values(t)
    bld = core.ModelBuilder().with_time_axis(axis).with_schema(schema).with_initial_values(init)
    for c in comps:
        bld.with_rust_component(c)
    for name, vals in exo.items():
        bld.with_exogenous_variable(name, core.Timeseries(vals, axis, "", core.InterpolationStrategy.Linear))
    model = bld.build(execution_order=execution_order)
    order = list(model._order)
    pos = {n: k for k, n in enumerate(order)}
    if execution_order == "reference":  # hand-derived from the edges of builder.rs and petgraph's Bfs
        assert [n for n in order if not n.startswith("Transform:")] == [
            "AerosolIndirect", "AerosolDirect", "N2OChemistry", "CH4Chemistry", "Aggregator:Effective Radiative Forcing",
            "GhgForcing", "OzoneForcing", "ClimateUDEB", "OceanCarbon", "TerrestrialCarbon", "CO2Budget"]
    else:
        assert pos["GhgForcing"] < pos["Aggregator:Effective Radiative Forcing"] > pos["OzoneForcing"]
    model.run()
    coll = model.timeseries()
    S = {n: coll.get_timeseries_by_name(n).values() for n in coll.names() if coll.get_timeseries_by_name(n) is not None}
    boxes = coll.get_fourbox_timeseries_by_name("Surface Temperature").values()  # [T][4]
    ad = model.ensembles["AerosolDirect"]
    ad_boxes = np.stack([ad.get_series(v)[:, 0] for v in range(1, 5)], axis=1)
    assert "Effective Radiative Forcing|Aerosol|Direct" in S and S["Effective Radiative Forcing|Aerosol|Direct"].shape == (T,)

    def scalar_of(bx):
        s = np.zeros(len(bx))
        for k in range(4):
            s = s + bx[:, k] * 0.25
        return s

    S["Surface Temperature"] = scalar_of(boxes)
    assert_bit_equal(S["Effective Radiative Forcing|Aerosol|Direct"][1:], scalar_of(ad_boxes)[1:], "write transform of the aerosol forcing")
    producer = {}
    for c in comps:
        for name, _, kind in c.definitions:
            if kind in ("Output", "State"):
                producer[name] = c.type_name
    producer["Effective Radiative Forcing"] = "Aggregator:Effective Radiative Forcing"
    sources = model.variable_sources()

    def seen(name, consumer, force_end=False):
        """What `consumer` read of `name` at every step n (length T, last entry unused)."""
        if name not in producer:
            return np.asarray(exo[name], dtype=np.float64).copy()
        # a producer that runs later has not written index n+1 yet: NaN
        return read_at_steps(np.asarray(S[name], dtype=np.float64), force_end or sources.get((name, consumer)) == "UpstreamOutput",
                             pos[producer[name]] < pos[consumer])

    def check(name, got, want, tol):
        err = relative_error(got, want, name)
        assert err <= tol, (name, err)

    def P(c):
        return np.asarray(by_name[c].param_vector(), dtype=np.float64)

    def block(c, rows):
        return np.stack([seen(r, c) for r in rows])

    # chemistry
    conc, life = orc.chem_run(orc.CHEM_CH4, b, P("CH4Chemistry"), block("CH4Chemistry", L.CH4_INPUTS), 722.0)
    check("CH4", S["Atmospheric Concentration|CH4"], conc[:, 0], 1e-12)
    check("Lifetime|CH4", S["Lifetime|CH4"], life[:, 0], 1e-12)
    conc, life = orc.chem_run(orc.CHEM_N2O, b, P("N2OChemistry"), block("N2OChemistry", L.N2O_INPUTS), 270.0)
    check("N2O", S["Atmospheric Concentration|N2O"], conc[:, 0], 1e-12)
    # forcings
    g = orc.ghg_run(T, P("GhgForcing"), block("GhgForcing", L.GH_INPUTS))
    for key, name in zip(orc.GHG_VARS, ("Effective Radiative Forcing|CO2", "Effective Radiative Forcing|CH4", "Effective Radiative Forcing|N2O")):
        check(name, S[name], g[key][:, 0], 1e-12)
    o = orc.pointwise_run(orc.PW_OZONE, T, P("OzoneForcing"), block("OzoneForcing", L.OZ_INPUTS))
    for k, name in enumerate(contributors[3:6]):
        check(name, S[name], o[k, :, 0], 1e-12)
    o = orc.pointwise_run(orc.PW_AEROSOL_DIRECT, T, P("AerosolDirect"), block("AerosolDirect", L.AD_INPUTS))
    check("aerosol direct boxes", ad_boxes, o[:, :, 0].T, 1e-12)
    o = orc.pointwise_run(orc.PW_AEROSOL_INDIRECT, T, P("AerosolIndirect"), block("AerosolIndirect", L.AI_INPUTS))
    check(contributors[7], S[contributors[7]], o[0, :, 0], 1e-12)
    # the aggregate: contributors at n+1, NaN skipped, all-NaN -> NaN; index 0 is the initial value
    agg = np.full(T, np.nan)
    agg[0] = 0.0
    rows = [seen(c, "Aggregator:Effective Radiative Forcing", force_end=True) for c in contributors]
    for n in range(T - 1):
        acc, cnt = 0.0, 0
        for r in rows:
            if not np.isnan(r[n]):
                acc, cnt = acc + r[n], cnt + 1
        agg[n + 1] = acc if cnt else np.nan
    assert_bit_equal(S["Effective Radiative Forcing"], agg, "Sum of eight forcings")
    seen_by_agg = [c for c, r in zip(contributors, rows) if not np.isnan(r[:-1]).all()]
    if execution_order == "reference":
        # petgraph's order runs the aggregate before GhgForcing and OzoneForcing: it holds the aerosol terms only
        assert seen_by_agg == contributors[6:]
    else:
        assert seen_by_agg == contributors
    # climate: at_start / at_end of the aggregate
    u, st = orc.udeb_run(b, P("ClimateUDEB"), S["Effective Radiative Forcing"])
    assert st[0] == 0
    for k, key in enumerate(("st0", "st1", "st2", "st3")):
        check(f"Surface Temperature box {k}", boxes[:, k], u[key][:, 0], 1e-9)
    check("Sea Surface Temperature", S["Sea Surface Temperature"], u["sst"][:, 0], 1e-9)
    check("Heat Uptake", S["Heat Uptake"], u["heat_uptake"][:, 0], 1e-9)
    # carbon cycle
    tc = orc.carbon_run(orc.CARBON_TERRESTRIAL, b, P("TerrestrialCarbon"), block("TerrestrialCarbon", L.TC_INPUTS),
                        [884.86, 92.77, 1681.53, 836.0])
    for k, name in enumerate(("Carbon Pool|Plant", "Carbon Pool|Detritus", "Carbon Pool|Soil", "Carbon Pool|Humus", "Carbon Flux|Terrestrial")):
        check(name, S[name], tc[k, :, 0], 1e-12)
    oc = orc.ocean_run(b, P("OceanCarbon"), block("OceanCarbon", L.OC_INPUTS), 278.0, 0.0)
    for k, name in enumerate(("Ocean Surface pCO2", "Cumulative Ocean Uptake", "Carbon Flux|Ocean")):
        check(name, S[name], oc[k, :, 0], 1e-9)
    cb = orc.carbon_run(orc.CARBON_BUDGET, b, P("CO2Budget"), block("CO2Budget", L.CB_INPUTS), [278.0])
    for k, name in enumerate(("Atmospheric Concentration|CO2", "Emissions|CO2|Net", "Airborne Fraction|CO2")):
        check(name, S[name], cb[k, :, 0], 1e-12)
    # the chain is alive: concentrations respond to emissions, the ocean takes carbon up
    assert S["Atmospheric Concentration|CO2"][-1] > 285.0 and S["Atmospheric Concentration|CH4"][-1] > 900.0
    assert S["Cumulative Ocean Uptake"][-1] > 0.0
    if execution_order == "topological":
        assert S["Effective Radiative Forcing"][-1] > S["Effective Radiative Forcing|Aerosol|Indirect"][-1] + 0.3
        assert boxes[-1].mean() > 0.05
    # a second run of the same model object is a fresh run: what the aggregate read as NaN the first
    # time (rows its producers had not written yet) must not be found filled in by the first run
    model.rewind()
    model.run()
    again = model.timeseries()
    for name in ("Effective Radiative Forcing", "Atmospheric Concentration|CO2", "Sea Surface Temperature"):
        assert_bit_equal(again.get_timeseries_by_name(name).values(), coll.get_timeseries_by_name(name).values(), f"rerun {name}")
    model.close()


def _closed_loop_member(model, exo, init, contributors, b, member, series=None):
    """The closed-loop check of test_full_emissions_driven_magicc_graph_closed_loop for one member of
    an ensemble of chains (topological or reference order alike): every component's outputs
    recomputed by its CPU oracle, with that member's parameters, from the inputs the component saw on
    the device.  `series(name)` -> [T] overrides how a stored series of the member is fetched."""
    from oracle import cbind as orc
    from rscm_amd import _lib as L
    T = len(b) - 1
    order = list(model._order)
    pos = {n: k for k, n in enumerate(order)}
    get = series or (lambda name: model.get_series(name, m_begin=member, m_end=member + 1)[:, 0])
    names = [n for n in model._var_home if n != "Surface Temperature"]
    S = {n: get(n) for n in names}
    ud = model.ensembles["ClimateUDEB"]
    boxes = np.stack([ud.get_series(v, m_begin=member, m_end=member + 1)[:, 0] for v in range(1, 5)], axis=1)
    ad = model.ensembles["AerosolDirect"]
    ad_boxes = np.stack([ad.get_series(v, m_begin=member, m_end=member + 1)[:, 0] for v in range(1, 5)], axis=1)

    def scalar_of(bx):
        s = np.zeros(len(bx))
        for k in range(4):
            s = s + bx[:, k] * 0.25
        return s

    S["Surface Temperature"] = scalar_of(boxes)
    assert_bit_equal(S["Effective Radiative Forcing|Aerosol|Direct"][1:], scalar_of(ad_boxes)[1:], "write transform of the aerosol forcing")
    producer = {}
    for c in model._chain_components:
        for name, _, kind in c.definitions:
            if kind in ("Output", "State"):
                producer[name] = c.type_name
    producer["Effective Radiative Forcing"] = "Aggregator:Effective Radiative Forcing"
    sources = model.variable_sources()

    def seen(name, consumer, force_end=False):
        if name not in producer:
            return np.asarray(exo[name], dtype=np.float64).copy()
        return read_at_steps(np.asarray(S[name], dtype=np.float64), force_end or sources.get((name, consumer)) == "UpstreamOutput",
                             pos[producer[name]] < pos[consumer])

    worst = {}

    def check(name, got, want, tol):
        worst[name] = err = relative_error(got, want, f"{name} (member {member})")
        assert err <= tol, (name, member, err)

    def P(c):
        return np.ascontiguousarray(model.ensembles[c].get_params()[:, member])

    def block(c, rows):
        return np.stack([seen(r, c) for r in rows])

    conc, life = orc.chem_run(orc.CHEM_CH4, b, P("CH4Chemistry"), block("CH4Chemistry", L.CH4_INPUTS), init["Atmospheric Concentration|CH4"])
    check("CH4", S["Atmospheric Concentration|CH4"], conc[:, 0], 1e-12)
    check("Lifetime|CH4", S["Lifetime|CH4"], life[:, 0], 1e-12)
    conc, life = orc.chem_run(orc.CHEM_N2O, b, P("N2OChemistry"), block("N2OChemistry", L.N2O_INPUTS), init["Atmospheric Concentration|N2O"])
    check("N2O", S["Atmospheric Concentration|N2O"], conc[:, 0], 1e-12)
    g = orc.ghg_run(T, P("GhgForcing"), block("GhgForcing", L.GH_INPUTS))
    for key, name in zip(orc.GHG_VARS, contributors[:3]):
        check(name, S[name], g[key][:, 0], 1e-12)
    o = orc.pointwise_run(orc.PW_OZONE, T, P("OzoneForcing"), block("OzoneForcing", L.OZ_INPUTS))
    for k, name in enumerate(contributors[3:6]):
        check(name, S[name], o[k, :, 0], 1e-12)
    o = orc.pointwise_run(orc.PW_AEROSOL_DIRECT, T, P("AerosolDirect"), block("AerosolDirect", L.AD_INPUTS))
    check("aerosol direct boxes", ad_boxes, o[:, :, 0].T, 1e-12)
    o = orc.pointwise_run(orc.PW_AEROSOL_INDIRECT, T, P("AerosolIndirect"), block("AerosolIndirect", L.AI_INPUTS))
    check(contributors[7], S[contributors[7]], o[0, :, 0], 1e-12)
    agg = np.full(T, np.nan)
    agg[0] = init["Effective Radiative Forcing"]
    rows = [seen(c, "Aggregator:Effective Radiative Forcing", force_end=True) for c in contributors]
    for n in range(T - 1):
        acc, cnt = 0.0, 0
        for r in rows:
            if not np.isnan(r[n]):
                acc, cnt = acc + r[n], cnt + 1
        agg[n + 1] = acc if cnt else np.nan
    assert_bit_equal(S["Effective Radiative Forcing"], agg, "Sum of eight forcings")
    u, st = orc.udeb_run(b, P("ClimateUDEB"), S["Effective Radiative Forcing"])
    assert st[0] == 0
    for k, key in enumerate(("st0", "st1", "st2", "st3")):
        check(f"Surface Temperature box {k}", boxes[:, k], u[key][:, 0], 1e-9)
    check("Sea Surface Temperature", S["Sea Surface Temperature"], u["sst"][:, 0], 1e-9)
    check("Heat Uptake", S["Heat Uptake"], u["heat_uptake"][:, 0], 1e-9)
    tc = orc.carbon_run(orc.CARBON_TERRESTRIAL, b, P("TerrestrialCarbon"), block("TerrestrialCarbon", L.TC_INPUTS),
                        [init[k] for k in ("Carbon Pool|Plant", "Carbon Pool|Detritus", "Carbon Pool|Soil", "Carbon Pool|Humus")])
    for k, name in enumerate(("Carbon Pool|Plant", "Carbon Pool|Detritus", "Carbon Pool|Soil", "Carbon Pool|Humus", "Carbon Flux|Terrestrial")):
        check(name, S[name], tc[k, :, 0], 1e-12)
    oc = orc.ocean_run(b, P("OceanCarbon"), block("OceanCarbon", L.OC_INPUTS), init["Ocean Surface pCO2"], init["Cumulative Ocean Uptake"])
    for k, name in enumerate(("Ocean Surface pCO2", "Cumulative Ocean Uptake", "Carbon Flux|Ocean")):
        check(name, S[name], oc[k, :, 0], 1e-9)
    cb = orc.carbon_run(orc.CARBON_BUDGET, b, P("CO2Budget"), block("CO2Budget", L.CB_INPUTS), [init["Atmospheric Concentration|CO2"]])
    for k, name in enumerate(("Atmospheric Concentration|CO2", "Emissions|CO2|Net", "Airborne Fraction|CO2")):
        check(name, S[name], cb[k, :, 0], 1e-12)
    return S, worst


def test_magicc_graph_on_a_monthly_axis_closed_loop(ra):
    """BASELINE.json configs[3] shape: the emissions-driven MAGICC graph on a MONTHLY model axis
    (288 steps of 1/12 year from 1750; ClimateUDEB and OceanCarbon still take their 12 sub-steps per
    model step, as the reference does whatever the step length: climate/udeb/mod.rs:399-656,
    carbon/ocean.rs:151-190), 10 240 members that differ in ECS, ocean diffusivity and the
    fertilisation factor.  Members spread over the ensemble (first and last lane of a wavefront, the
    last member) pass the closed-loop check against all ten component oracles at the single-component
    tolerances; the other members are compared through ensemble-level properties."""
    mod = magicc_chain()
    years, spy, N = 24, 12, 10_240
    t, exo, init, contributors = mod.chain_inputs(years, spy)
    b = np.append(t, t[-1] + (t[-1] - t[-2]))
    model = mod.build_chain(N, years, "topological", steps_per_year=spy)
    assert len(t) == 289 and np.allclose(np.diff(t), 1.0 / 12.0)
    model.run()
    ud_status = model.ensembles["ClimateUDEB"].status()
    assert not ud_status.any()
    worst = {}
    for member in (0, 63, 64, 5000, N - 1):
        S, w = _closed_loop_member(model, exo, init, contributors, b, member)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert S["Atmospheric Concentration|CO2"][-1] > 278.0 and S["Cumulative Ocean Uptake"][-1] > 0.0
    print("monthly axis, worst relative deviation per variable:", {k: f"{v:.1e}" for k, v in worst.items() if v > 0})
    # members with equal parameters agree bit for bit wherever they sit; different ECS gives different warming
    ud = model.ensembles["ClimateUDEB"]
    P = ud.get_params()
    sst_end = model.get_series("Sea Surface Temperature", t_begin=len(t) - 1)[0]
    assert np.isfinite(sst_end).all() and np.unique(sst_end).size > N // 2
    model.rewind()
    P[:, 1::2] = P[:, 0::2]
    ud.set_params(P)
    tc = model.ensembles["TerrestrialCarbon"]
    Q = tc.get_params()
    Q[:, 1::2] = Q[:, 0::2]
    tc.set_params(Q)
    model.run()
    for name in ("Sea Surface Temperature", "Atmospheric Concentration|CO2", "Carbon Flux|Ocean", "Effective Radiative Forcing"):
        row = model.get_series(name, t_begin=len(t) - 1)[0]
        assert_bit_equal(row[1::2], row[0::2], f"paired members: {name}")
    model.close()


def test_calibrating_a_linked_graph(ra):
    """rscm-calibrate over a graph without a fused kernel: ModelRunner batches the members through
    the linked ensembles, the Gaussian log-likelihood is reduced on the device per owning ensemble.
    Checks: run_batch of a graph == the same members run one by one; log-likelihoods == the host
    formula on the extracted series (likelihood.rs:167-250); the stretch-move sampler recovers the
    parameters that generated the pseudo-observations (ECS-like lambda0 of TwoLayer and the CO2
    fertilisation-like conc_pi-free tau of CarbonCycle, two different components)."""
    import rscm_amd.calibrate as cal
    import rscm_amd.core as core
    from rscm_amd.components import CarbonCycleBuilder, CO2ERFBuilder
    from rscm_amd.two_layer import TwoLayerBuilder
    t = np.arange(1750.0, 1901.0)
    axis = core.TimeAxis.from_values(t)
    tl = dict(lambda0=1.1, a=0.0, efficacy=1.2, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    schema = core.VariableSchema()
    names = ["Emissions|CO2|Anthropogenic", "Surface Temperature", "Deep Ocean Temperature", "Atmospheric Concentration|CO2",
             "Cumulative Land Uptake", "Cumulative Emissions|CO2", "Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other"]
    for n in names:
        schema.add_variable(n, "")
    schema.add_aggregate("Effective Radiative Forcing", "W/m^2", "Sum", ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other"])

    def builder():
        return (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
                .with_rust_component(CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.05)).build())
                .with_rust_component(CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=278.0)).build())
                .with_rust_component(TwoLayerBuilder.from_parameters(tl).build())
                .with_exogenous_variable("Emissions|CO2|Anthropogenic", core.Timeseries(emissions_syn(t) + 1.0, axis, "", core.InterpolationStrategy.Linear))
                .with_exogenous_variable("Effective Radiative Forcing|Other", core.Timeseries(0.2 * np.sin(t / 9.0), axis, "", core.InterpolationStrategy.Linear))
                .with_initial_values({"Cumulative Land Uptake": 0.0, "Cumulative Emissions|CO2": 0.0, "Atmospheric Concentration|CO2": 278.0,
                                      "Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))

    pnames = ["TwoLayer.lambda0", "tau"]   # qualified, and bare where unique
    outputs = ["Surface Temperature", "Atmospheric Concentration|CO2"]
    runner = cal.ModelRunner(builder(), pnames, outputs)
    assert runner._graph
    with pytest.raises(ValueError, match="ambiguous"):
        cal.ModelRunner(builder(), ["conc_pi"], outputs)   # CarbonCycle and CO2ERF both have one
    truth = [1.25, 30.0]
    sets = np.array([truth, [0.9, 20.0], [1.4, 38.0]])
    batch = runner.run_batch(sets)
    for k, ps in enumerate(sets):
        one = runner.run(list(ps))
        for v in outputs:
            assert one[v] == batch[k][v]
    assert len(batch[0]["Surface Temperature"]) == len(t) and batch[0]["Atmospheric Concentration|CO2"][1900.0] > 300.0
    target = cal.Target()
    obs_years = np.arange(1800.0, 1901.0, 10.0)
    for v, sigma in (("Surface Temperature", 0.005), ("Atmospheric Concentration|CO2", 0.1)):
        for y in obs_years:
            target.add_observation(v, float(y), batch[0][v][float(y)], sigma)
    lik = cal.GaussianLikelihood()
    ll = runner.log_likelihood_batch(sets, target, lik)
    want = [sum(-0.5 * ((batch[0][v][float(y)] - batch[k][v][float(y)]) / s) ** 2
                for v, s in (("Surface Temperature", 0.005), ("Atmospheric Concentration|CO2", 0.1)) for y in obs_years) for k in range(3)]
    assert ll[0] == 0.0 and np.allclose(ll, want, rtol=1e-10, atol=1e-12)
    params = cal.ParameterSet().add("TwoLayer.lambda0", cal.Uniform(0.8, 1.6)).add("tau", cal.Uniform(15.0, 45.0))
    sampler = cal.EnsembleSampler(params, runner, lik, target)
    chain = sampler.run(400, cal.WalkerInit.from_prior(), n_walkers=64, rng=np.random.default_rng(3))
    flat = chain.flat_samples(discard=300)
    med = np.median(flat, axis=0)
    assert abs(med[0] - truth[0]) < 0.02 and abs(med[1] - truth[1]) < 1.0, med
    # the device sampler over the graph as the evaluator (rscm_sampler_create_graph): the proposal kernel writes lambda0 into
    # TwoLayer's parameter block and tau into CarbonCycle's, the graph is stepped to the last observed index, the likelihood
    # kernel reads Ts and CO2 where their owners store them -- no host round trip per sweep
    dev = cal.DeviceEnsembleSampler(params, runner, lik, target)
    rng = np.random.default_rng(0)
    pos = params.sample_random(128, rng)
    pos[7, 1] = 50.0   # outside Uniform(15, 45)
    want = sampler.log_posterior_batch(pos)
    one = dev.run(1, cal.WalkerInit.explicit(pos), n_walkers=128, seed=5)
    got_pos, got_lp = one.flat_samples(), one.flat_log_probs()
    same = (got_pos == pos).all(axis=1)
    assert same.any() and (~same).any() and want[7] == -np.inf
    # walkers that did not move keep their initial score; accepted proposals carry their own: both are the host's
    # numbers (the per-owner partial sums are added in the target's order on both sides)
    assert np.allclose(got_lp[same], want[same], rtol=1e-12, atol=1e-9) and got_lp[7] == -np.inf
    moved = sampler.log_posterior_batch(got_pos[~same])
    assert np.allclose(got_lp[~same], moved, rtol=1e-12, atol=1e-9) and np.isfinite(got_lp[~same]).all()
    big = dev.run(150, cal.WalkerInit.from_prior(), n_walkers=4096, seed=11)
    x = big.flat_samples(discard=120)
    dmed = np.median(x, axis=0)
    assert abs(dmed[0] - truth[0]) < 0.02 and abs(dmed[1] - truth[1]) < 1.0, dmed
    hstd, dstd = flat.std(axis=0), x.std(axis=0)
    assert np.all(np.abs(dmed - med) < 3.0 * hstd), (dmed, med)          # the host sampler's posterior ...
    assert np.all(dstd < 3.0 * hstd) and np.all(dstd > hstd / 3.0), (dstd, hstd)   # ... location and spread
    assert 0.15 < dev.acceptance_rate() < 0.9 and (dev.n_proposed == 150).all()
    runner.close()


def test_halocarbon_eesc_feeds_ozone(ra):
    """HalocarbonChemistry -> (EESC) -> OzoneForcing: a 41-input producer whose output is linked
    into a consumer.  The producer's series equal those of the same component run alone; the ozone
    forcing equals the CPU oracle evaluated on the EESC it read (UpstreamOutput: index n+1)."""
    import rscm_amd.core as core
    from oracle import cbind as orc
    from rscm_amd import _lib as L
    from rscm_amd import magicc as B
    t = np.arange(1950.0, 2011.0)
    T, yrs = len(t), t - 1950.0
    axis = core.TimeAxis.from_values(t)
    emis = {f"Emissions|{s}": np.zeros(T) for s in L.HC_SPECIES}
    emis["Emissions|CFC-11"] = 50.0 + 8.0 * yrs
    emis["Emissions|CFC-12"] = 80.0 + 10.0 * yrs
    emis["Emissions|Halon-1211"] = 0.2 * yrs
    other = {"Atmospheric Concentration|CH4": 1100.0 + 10.0 * yrs, "Emissions|NOx": 20.0 + 0.3 * yrs, "Emissions|CO": 500.0 + 3.0 * yrs,
             "Emissions|NMVOC": 100.0 + yrs, "Surface Temperature": 0.01 * yrs}
    init = {f"Atmospheric Concentration|{s}": 0.0 for s in L.HC_SPECIES}
    init["Atmospheric Concentration|CFC-11"] = 5.0

    def builder(with_ozone):
        b = core.ModelBuilder().with_time_axis(axis).with_initial_values(init)
        b.with_rust_component(B.HalocarbonChemistryBuilder.from_parameters({}).build())
        if with_ozone:
            b.with_rust_component(B.OzoneForcingBuilder.from_parameters({"eesc_reference": 100.0}).build())
        for name, vals in {**emis, **(other if with_ozone else {})}.items():
            b.with_exogenous_variable(name, core.Timeseries(vals, axis, "", core.InterpolationStrategy.Linear))
        return b

    alone = builder(False).build()
    alone.run()
    eesc_alone = alone.timeseries().get_timeseries_by_name("EESC").values()
    alone.close()
    model = builder(True).build()
    assert isinstance(model, core.GraphModel) and model._feed_forward
    assert model.variable_sources()[("EESC", "OzoneForcing")] == "UpstreamOutput"
    model.run()
    got = model.timeseries()
    eesc = got.get_timeseries_by_name("EESC").values()
    assert_bit_equal(eesc, eesc_alone, "EESC")
    assert eesc[-1] > 500.0
    seen = np.full(T, np.nan)
    seen[:-1] = eesc[1:]
    block = np.stack([seen] + [other[k] for k in L.OZ_INPUTS[1:]])
    P = np.asarray(B.OzoneForcingBuilder.from_parameters({"eesc_reference": 100.0}).build().param_vector())
    want = orc.pointwise_run(orc.PW_OZONE, T, P, block)
    for k, name in enumerate(("Effective Radiative Forcing|O3|Stratospheric", "Effective Radiative Forcing|O3|Tropospheric",
                              "Effective Radiative Forcing|O3|Temperature Feedback")):
        g, w = got.get_timeseries_by_name(name).values(), want[k, :, 0]
        assert (np.isnan(g) == np.isnan(w)).all() and np.allclose(g[1:], w[1:], rtol=1e-12, atol=1e-15), name
    assert got.get_timeseries_by_name("Effective Radiative Forcing|O3|Stratospheric").values()[-1] < -0.01
    model.close()


def test_link_bookkeeping_and_lockstep_errors(ra):
    """Relinking a row moves the reference from the old producer to the new one; destroying a
    consumer releases its producers; rscm_ens_run_lockstep refuses handles that stand at different
    time indices or run on different streams; clear_series makes rows after index 0 NaN again."""
    from rscm_amd.ensemble import run_lockstep
    t = axis_values(2000, 2010)
    b = _bounds(t)
    s = Stream()
    P = two_layer_params(8)

    def two_layer():
        e = ra.Ensemble(ra.KIND_TWO_LAYER, 8, b)
        e.set_stream(s.h.value)
        e.set_params(P)
        e.set_initial(1, 0.0)
        e.set_initial(2, 0.0)
        return e

    p1, p2, c = two_layer(), two_layer(), two_layer()
    p1.set_forcing(f_syn(t))
    p2.set_forcing(2.0 * f_syn(t))
    c.link_input(0, p1, 1)
    c.link_input(0, p2, 1)          # relink: p1 is free again
    p1.close()
    with pytest.raises(Exception, match="linked input"):
        p2.close()
    p2.run()
    c.run()
    want = c.get_series(1)
    with ra.Ensemble(ra.KIND_TWO_LAYER, 8, b) as ref:   # the same numbers through the table: Ts of p2, member 0 .. 7 as scenarios
        ref.set_params(P)
        ref.set_initial(1, 0.0)
        ref.set_initial(2, 0.0)
        ref.set_forcing(p2.get_series(1).T.copy(), np.arange(8, dtype=np.int32))
        ref.run()
        assert_bit_equal(want, ref.get_series(1), "linked to the second producer")
    # lock-step preconditions
    p2.rewind()
    with pytest.raises(Exception, match="time index"):
        run_lockstep((p2, c))
    c.rewind()
    other = ra.Ensemble(ra.KIND_TWO_LAYER, 8, b)     # keeps its own stream
    other.set_params(P)
    with pytest.raises(Exception, match="another stream"):
        run_lockstep((p2, other))
    other.close()
    run_lockstep((p2, c), 4)
    assert p2.time_index == 4 and c.time_index == 4
    run_lockstep((p2, c))
    assert_bit_equal(c.get_series(1), want, "lock-step in two legs")
    c.clear_series()
    cleared = c.get_series(1, 0, len(t))
    assert c.time_index == 0 and (cleared[0] == 0.0).all()
    c.close()                        # releases p2
    p2.close()
    s.close()


def test_carbon_cycle_and_co2_erf_kinds_on_their_own(ra):
    """RSCM_KIND_CARBON_CYCLE / RSCM_KIND_CO2_ERF with table inputs (no links) against the generic
    stepper: CarbonCycle with exogenous emissions and temperature, two RK4 step sizes, scenario map;
    CO2ERF at the reference's known-answer points (co2_erf.rs:94-114: 0 at C0, erf_2xco2 at 2 C0)."""
    from oracle import reference_model as rm
    t = np.arange(1750.0, 1851.0)
    T, b = len(t), _bounds(t)
    E = np.stack([emissions_syn(t) + 0.5, 3.0 + 0.0 * t])
    Temp = np.stack([0.01 * (t - 1750.0), 1.0 + 0.0 * t])
    N = 6
    rng = np.random.default_rng(4)
    P = np.stack([rng.uniform(15.0, 40.0, N), np.full(N, 278.0), rng.uniform(0.0, 0.1, N)])
    scen = (np.arange(N) % 2).astype(np.int32)
    for h in (0.1, 0.25):
        with ra.Ensemble(ra.KIND_CARBON_CYCLE, N, b) as e:
            e.set_params(P)
            e.set_step_size(1, h)
            e.set_forcing(np.stack([np.stack([E[s], Temp[s]]) for s in range(2)]), scen)
            for var, v in ((1, 280.0), (2, 0.0), (3, 0.0)):
                e.set_initial(var, v)
            e.run(40)
            e.run()
            got = [e.get_series(v) for v in (1, 2, 3)]
            assert not e.status().any()
        for i in range(N):
            s = int(scen[i])
            m = rm.ModelBuilder(axis=rm.TimeAxis.from_values(t), components=[rm.CarbonCycle(P[0, i], P[1, i], P[2, i], step=h)],
                                initial_values={"Atmospheric Concentration|CO2": 280.0, "Cumulative Land Uptake": 0.0,
                                                "Cumulative Emissions|CO2": 0.0},
                                exogenous={"Emissions|CO2|Anthropogenic": rm.ExoSeries(list(E[s]), rm.TimeAxis.from_values(t)),
                                           "Surface Temperature": rm.ExoSeries(list(Temp[s]), rm.TimeAxis.from_values(t))}).build()
            m.run()
            for k, name in enumerate(("Atmospheric Concentration|CO2", "Cumulative Land Uptake", "Cumulative Emissions|CO2")):
                w = np.array(m.data[name])
                assert np.allclose(got[k][:, i], w, rtol=1e-12, atol=0.0), (h, i, name)
            assert_bit_equal(got[2][:, i], np.array(m.data["Cumulative Emissions|CO2"]), "cumulative emissions involve no exp")
    with pytest.raises(Exception, match="does not land"):
        with ra.Ensemble(ra.KIND_CARBON_CYCLE, N, b) as e:
            e.set_params(P)
            e.set_step_size(1, 0.3)   # ceil(1/0.3) = 4 steps of 0.3 overshoot the year by 0.2
            e.set_forcing(np.stack([E[0], Temp[0]]))
            for var in (1, 2, 3):
                e.set_initial(var, 0.0)
            e.run()
    conc = np.array([278.0, 556.0, 417.0, 0.0])
    with ra.Ensemble(ra.KIND_CO2_ERF, 3, _bounds(np.array([0.0, 1.0, 2.0, 3.0]))) as e:
        e.set_params(np.array([[3.7, 4.0, 3.7], [278.0, 278.0, 300.0]]))
        e.set_forcing(conc)  # C at indices 0, 1, 2 is read by steps 0, 1, 2 (exogenous: index n)
        e.run()
        got = e.get_series(1)
    assert np.isnan(got[0]).all()
    assert got[1, 0] == 0.0 and abs(got[2, 0] - 3.7) < 1e-15 and abs(got[2, 1] - 4.0) < 1e-15
    want = rm.CO2ERF(3.7, 300.0).calculate_erf(417.0)
    assert abs(got[3, 2] - want) < 1e-15


def test_graph_checkpoint_resumes_the_full_chain_bit_identically(ra, tmp_path):
    """Checkpoint / resume (Model::checkpoint / from_checkpoint, runtime.rs:270-282) of the
    emissions-driven MAGICC graph: time index, the current row of every stored variable, the rows the
    chemistry looks back at (N2O: strat_delay + 1), and the internal component states -- ClimateUDEB's
    ocean columns and temperature history, OceanCarbon's flux history.  A fresh model object restored
    at step 33 (odd: inside a split ocean tile) continues to the same bits."""
    mod = magicc_chain()
    years, N = 70, 96
    a = mod.build_chain(N, years, "topological")
    a.run()
    names = ["Atmospheric Concentration|CO2", "Atmospheric Concentration|CH4", "Atmospheric Concentration|N2O", "Sea Surface Temperature",
             "Cumulative Ocean Uptake", "Carbon Pool|Soil", "Effective Radiative Forcing", "Effective Radiative Forcing|O3|Tropospheric"]
    want = {n: a.get_series(n) for n in names}
    a.close()
    b1 = mod.build_chain(N, years, "topological")
    for _ in range(33):
        b1.step()
    ck = b1.checkpoint()
    b1.close()
    assert ck["time_index"] == 33 and ck["ensembles"]["OceanCarbon"]["internal"].size == 33 * 12 * N
    assert ck["ensembles"]["N2OChemistry"]["history"]["Atmospheric Concentration|N2O"].shape[0] >= 2
    import rscm_amd.core as core
    core.save_checkpoint(tmp_path / "chain.npz", ck)   # through a file: plain arrays, nothing pickled
    ck = core.load_checkpoint(tmp_path / "chain.npz")
    b2 = mod.build_chain(N, years, "topological")
    b2.restore(ck)
    assert b2.time_index == 33
    b2.step()
    b2.run()
    for n in names:
        assert_bit_equal(b2.get_series(n)[33:], want[n][33:], f"resumed {n}")
    assert np.isfinite(want["Sea Surface Temperature"][1:]).all()
    with pytest.raises(ValueError, match="does not match"):
        other = mod.build_chain(N, years, "reference")
        try:
            other.restore(ck)
        finally:
            other.close()
    b2.close()


def test_graph_rollback_into_the_same_model_in_reference_order(ra):
    """Roll an already finished model back to an earlier checkpoint of itself, in the reference's
    breadth-first order (where the forcing aggregate runs before some of its producers and must find
    NaN at n+1): the rows the first pass wrote beyond the checkpoint must not be seen by the second.
    The continuation carries the bits of the uninterrupted run."""
    mod = magicc_chain()
    years, N = 40, 64
    m = mod.build_chain(N, years, "reference")
    assert m._reads_unwritten
    names = ["Effective Radiative Forcing", "Atmospheric Concentration|CO2", "Atmospheric Concentration|CH4", "Sea Surface Temperature",
             "Carbon Flux|Ocean", "Effective Radiative Forcing|CO2"]
    for _ in range(17):
        m.step()
    ck = m.checkpoint()
    m.run()
    want = {n: m.get_series(n) for n in names}
    m.restore(ck)          # the same model object, all rows up to the end already written once
    assert m.time_index == 17
    erf, _ = m.variable_home("Effective Radiative Forcing")
    assert np.isnan(erf.get_series(1, 18, 19)).all()
    m.step()
    m.run()
    for n in names:
        assert_bit_equal(m.get_series(n), want[n], f"rolled back {n}")
    m.close()


@pytest.mark.parametrize("seed", range(8))
def test_graph_model_random_registration_orders(ra, seed):
    """The five-component chain of test_graph_model_magicc_lite_chain_with_feedback registered in a
    random order, with a random aggregate operation and N2O delay: whatever petgraph's breadth-first
    order and the registration-order classification make of it (lagged reads, reads of rows not
    written yet), the linked ensembles must reproduce the generic stepper variable by variable.
    Orders that leave components unreachable from the root are refused."""
    import rscm_amd.core as core
    from oracle import reference_model as rm
    from rscm_amd import magicc
    from rscm_amd.two_layer import TwoLayerBuilder
    rng = np.random.default_rng(700 + seed)
    t = np.arange(1850.0, 1911.0)
    yrs = t - t[0]
    tl = dict(lambda0=1.2, a=0.0, efficacy=1.1, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)
    exo = {"Emissions|CH4": 250.0 + 3.0 * yrs, "Emissions|NOx": 30.0 + 0.2 * yrs, "Emissions|CO": 400.0 + 2.0 * yrs,
           "Emissions|NMVOC": 80.0 + 0.5 * yrs, "Emissions|N2O": 8.0 + 0.05 * yrs,
           "Atmospheric Concentration|CO2": 285.0 + 0.3 * yrs + 0.004 * yrs ** 2,
           "Emissions|SOx": 5.0 + 0.6 * yrs, "Emissions|OC": 12.0 + 0.1 * yrs}
    init = {"Atmospheric Concentration|CH4": 800.0, "Atmospheric Concentration|N2O": 273.0,
            "Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}
    contributors = ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|CH4", "Effective Radiative Forcing|N2O",
                    "Effective Radiative Forcing|Aerosol|Indirect"]
    op = str(rng.choice(["Sum", "Mean"]))
    delay = int(rng.integers(1, 5))
    comps = [magicc.CH4ChemistryBuilder.from_parameters({"include_temp_feedback": True}).build(),
             magicc.N2OChemistryBuilder.from_parameters({"strat_delay": delay}).build(),
             magicc.GhgForcingBuilder.from_parameters({"method": str(rng.choice(["Olbl", "Ipcctar"]))}).build(),
             magicc.AerosolIndirectBuilder.from_parameters({}).build(),
             TwoLayerBuilder.from_parameters(tl).build()]
    perm = rng.permutation(5)
    comps = [comps[k] for k in perm]
    ref_of = {"CH4Chemistry": rm.CH4Chemistry, "N2OChemistry": rm.N2OChemistry, "GhgForcing": rm.GhgForcing,
              "AerosolIndirect": rm.AerosolIndirect}
    schema = core.VariableSchema()
    for n in list(exo) + list(init) + contributors + ["Lifetime|CH4", "Lifetime|N2O"]:
        schema.add_variable(n, "")
    schema.add_aggregate("Effective Radiative Forcing", "W/m^2", op, contributors)
    axis = core.TimeAxis.from_values(t)
    b = core.ModelBuilder().with_time_axis(axis).with_schema(schema).with_initial_values(init)
    for c in comps:
        b.with_rust_component(c)
    for name, vals in exo.items():
        b.with_exogenous_variable(name, core.Timeseries(vals, axis, "", core.InterpolationStrategy.Linear))
    ref = rm.ModelBuilder(
        axis=rm.TimeAxis.from_values(t),
        components=[rm.TwoLayer(*[tl[k] for k in core.TL_PARAM_ORDER]) if c.type_name == "TwoLayer" else ref_of[c.type_name](c.param_vector())
                    for c in comps],
        aggregates=[("Effective Radiative Forcing", op, contributors)], initial_values=init,
        exogenous={k: rm.ExoSeries(list(v), rm.TimeAxis.from_values(t)) for k, v in exo.items()}).build()
    ref_order = [ref.order_nodes[i].type_name for i in ref._bfs() if ref.order_nodes[i] is not None]
    names = [c.type_name for c in comps]
    if len(ref_order) < 6:
        with pytest.raises(NotImplementedError, match="not reachable"):
            b.build()
        return
    model = b.build()
    assert list(model._order) == ref_order, (names, model._order, ref_order)
    model.run()
    ref.run()
    got = model.timeseries()
    for name, want in ref.data.items():
        g, w = got.get_timeseries_by_name(name).values(), np.array(want)
        assert (np.isnan(g) == np.isnan(w)).all(), (names, op, name)
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= 1e-11 * np.maximum(1.0, np.abs(w[ok]))).all(), (names, op, name)
    model.close()


def test_ssp245_emissions_driven_against_magicc7(ra):
    """The reference's own emissions-driven regression scenario (tests/regression/test_ghg_forcing.py::
    test_03_emissions_driven: SSP245 emissions 1750-2100 from MAGICC7's output file, committed as
    tests/golden/magicc7_emissions_driven.json by make_emissions_goldens.py; xfail upstream) through
    the ten-component graph on the GPU, wired and initialised as that test does.

    Upstream compares concentrations at rtol 5e-2 and expects to fail.  Stepped in the reference's
    breadth-first order the total forcing holds the aerosol terms only (the aggregate runs before
    GhgForcing and OzoneForcing) and the model cools; stepped in topological order, with the initial
    value of the aggregate that ClimateUDEB's at_start() needs, the chain lands on MAGICC7: CO2 within
    the upstream tolerance over the whole run, forcing and warming in 2100 within 2 % and 0.2 K.  CH4
    and N2O keep the deviations the upstream issues (#108-#110: simplified chemistry) describe."""
    import json
    import os
    import rscm_amd.core as core
    from rscm_amd import magicc as B
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "magicc7_emissions_driven.json")))
    V = {k: np.array(v) for k, v in g["variables"].items()}
    t = np.array(g["years"], dtype=float)
    assert t[0] == 1750.0 and t[-1] == 2100.0 and g["config"]["core_climatesensitivity"] == 3.0

    def sectors(base):  # _extract_emissions of the upstream test: MAGICC's two sectors summed
        return V[f"{base}|MAGICC Fossil and Industrial"] + V[f"{base}|MAGICC AFOLU"]

    exo = {"Emissions|CO2|Fossil": V["Emissions|CO2"], "Emissions|CO2|Land Use": 0.0 * t, "Emissions|CH4": V["Emissions|CH4"],
           "Emissions|N2O": V["Emissions|N2O"], "Emissions|NOx": sectors("Emissions|NOx"), "Emissions|CO": sectors("Emissions|CO"),
           "Emissions|NMVOC": sectors("Emissions|NMVOC"), "Emissions|SOx": sectors("Emissions|SOx"),
           "Emissions|BC": sectors("Emissions|BC"), "Emissions|OC": sectors("Emissions|OC"), "EESC": 0.0 * t}
    co2_0, ch4_0, n2o_0 = (float(V[f"Atmospheric Concentrations|{s}"][0]) for s in ("CO2", "CH4", "N2O"))
    init = {"Atmospheric Concentration|CO2": co2_0, "Atmospheric Concentration|CH4": ch4_0, "Atmospheric Concentration|N2O": n2o_0,
            "Surface Temperature": 0.0, "Ocean Surface pCO2": co2_0, "Cumulative Ocean Uptake": 0.0,
            "Carbon Pool|Plant": 884.86, "Carbon Pool|Detritus": 92.77, "Carbon Pool|Soil": 1681.53, "Carbon Pool|Humus": 836.0}
    contributors = ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|CH4", "Effective Radiative Forcing|N2O",
                    "Effective Radiative Forcing|O3|Stratospheric", "Effective Radiative Forcing|O3|Tropospheric",
                    "Effective Radiative Forcing|O3|Temperature Feedback", "Effective Radiative Forcing|Aerosol|Direct",
                    "Effective Radiative Forcing|Aerosol|Indirect"]

    def run(order, erf0):
        schema = core.VariableSchema()
        for n in list(exo) + [k for k in init if k != "Surface Temperature"] + contributors + [
                "Heat Uptake", "Ocean Heat Content", "Sea Surface Temperature", "Carbon Flux|Terrestrial", "Carbon Flux|Ocean",
                "Emissions|CO2|Net", "Airborne Fraction|CO2", "Lifetime|CH4", "Lifetime|N2O"]:
            schema.add_variable(n, "")
        schema.add_variable("Surface Temperature", "K", core.GridType.FourBox)
        schema.add_aggregate("Effective Radiative Forcing", "W/m^2", "Sum", contributors)
        comps = [B.CH4ChemistryBuilder.from_parameters({"ch4_pi": ch4_0}).build(), B.N2OChemistryBuilder.from_parameters({"n2o_pi": n2o_0}).build(),
                 B.GhgForcingBuilder.from_parameters({"method": "Ipcctar", "delq2xco2": 3.71, "co2_pi": co2_0, "ch4_pi": ch4_0,
                                                      "n2o_pi": n2o_0}).build(),
                 B.OzoneForcingBuilder.from_parameters({}).build(), B.AerosolDirectBuilder.from_parameters({}).build(),
                 B.AerosolIndirectBuilder.from_parameters({}).build(),
                 B.ClimateUDEBBuilder.from_parameters({"ecs": 3.0, "rf_2xco2": 3.71}).build(),
                 B.TerrestrialCarbonBuilder.from_parameters({}).build(), B.OceanCarbonBuilder.from_parameters({}).build(),
                 B.CO2BudgetBuilder.from_parameters({}).build()]
        axis = core.TimeAxis.from_values(t)
        iv = dict(init)
        if erf0:
            iv["Effective Radiative Forcing"] = 0.0
        b = core.ModelBuilder().with_time_axis(axis).with_schema(schema).with_initial_values(iv)
        for c in comps:
            b.with_rust_component(c)
        for name, vals in exo.items():
            b.with_exogenous_variable(name, core.Timeseries(vals, axis, "", core.InterpolationStrategy.Linear))
        m = b.build(execution_order=order)
        m.run()
        ts = m.timeseries()
        out = {n: ts.get_timeseries_by_name(n).values() for n in ("Atmospheric Concentration|CO2", "Atmospheric Concentration|CH4",
                                                                "Atmospheric Concentration|N2O", "Effective Radiative Forcing")}
        out["T"] = ts.get_fourbox_timeseries_by_name("Surface Temperature").values().mean(axis=1)
        m.close()
        return out

    def max_rel(ours, magicc):  # the upstream comparison: our index n+1 against MAGICC7's year n
        a, e = ours[1:], magicc[:-1]
        return float(np.max(np.abs(a - e) / np.abs(e)))

    as_upstream = run("reference", False)
    assert as_upstream["Effective Radiative Forcing"][-1] < 0.0          # aerosols only: negative total forcing in 2100
    assert max_rel(as_upstream["Atmospheric Concentration|CO2"], V["Atmospheric Concentrations|CO2"]) > 0.05   # upstream's xfail
    fixed = run("topological", True)
    assert max_rel(fixed["Atmospheric Concentration|CO2"], V["Atmospheric Concentrations|CO2"]) < 0.05          # upstream's tolerance
    assert max_rel(fixed["Atmospheric Concentration|N2O"], V["Atmospheric Concentrations|N2O"]) < 0.08
    assert max_rel(fixed["Atmospheric Concentration|CH4"], V["Atmospheric Concentrations|CH4"]) < 0.20
    assert abs(fixed["Effective Radiative Forcing"][-1] / V["Effective Radiative Forcing"][-2] - 1.0) < 0.03
    assert abs(fixed["T"][-1] - V["Surface Temperature"][-2]) < 0.25
    assert np.isfinite(fixed["T"]).all()


def test_python_components_in_a_gpu_graph(ra):
    """Components written in Python (rscm_amd.component, the reference's rscm.component surface) inside
    a graph of GPU components: their solve() runs on the host between the launches, their outputs
    live in device series the GPU components link to.

    1. the reference's own example (tests/test_typed_python_component.py::test_typed_component_in_model):
       280 + 10 * 0.5 = 285 ppm and 5 GtC after one step; the history window example runs.
    2. CO2ERF rewritten in Python between the GPU CarbonCycle and the GPU TwoLayer, plus a Python
       diagnostic that reads the GPU temperature: the same series as the all-GPU graph (host log vs
       device log: 1e-12), same execution order, lagged temperature feedback intact, three members."""
    import math
    import rscm_amd.core as core
    from rscm_amd.component import Component, Input, Output, PythonComponent, State
    from rscm_amd.components import CarbonCycleBuilder, CO2ERFBuilder
    from rscm_amd.two_layer import TwoLayerBuilder

    class SimpleCarbonCycle(Component, register=False):
        emissions = Input("Emissions|CO2", unit="GtCO2")
        concentration = State("Atmospheric Concentration|CO2", unit="ppm")
        uptake = Output("Carbon Uptake", unit="GtC")

        def __init__(self, sensitivity):
            self.sensitivity = sensitivity

        def solve(self, t_current, t_next, inputs):
            e = inputs.emissions.at_start()
            return self.Outputs(concentration=inputs.concentration.at_start() + e * self.sensitivity, uptake=e * 0.5)

    axis3 = core.TimeAxis.from_values(np.array([2020.0, 2021.0, 2022.0]))
    model = (core.ModelBuilder().with_py_component(PythonComponent.build(SimpleCarbonCycle(0.5))).with_time_axis(axis3)
             .with_exogenous_variable("Emissions|CO2", core.Timeseries(np.array([10.0, 10.0, 10.0]), axis3, "GtCO2", core.InterpolationStrategy.Previous))
             .with_initial_values({"Atmospheric Concentration|CO2": 280.0}).build())
    model.step()
    coll = model.timeseries()
    assert abs(coll.get_timeseries_by_name("Atmospheric Concentration|CO2").at(1) - 285.0) < 1e-3
    assert abs(coll.get_timeseries_by_name("Carbon Uptake").at(1) - 5.0) < 1e-3
    model.run()
    assert model.finished() and coll.get_timeseries_by_name("Atmospheric Concentration|CO2").at(0) == 280.0
    assert model.timeseries().get_timeseries_by_name("Atmospheric Concentration|CO2").at(2) == 290.0
    model.close()

    class Delta(Component, register=False):
        temperature = Input("Temperature", unit="K")
        output = Output("Output", unit="")

        def solve(self, t_current, t_next, inputs):
            try:
                return self.Outputs(output=inputs.temperature.at_start() - inputs.temperature.previous)
            except ValueError:
                return self.Outputs(output=0.0)

    axis4 = core.TimeAxis.from_values(np.array([2020.0, 2021.0, 2022.0, 2023.0]))
    m = (core.ModelBuilder().with_py_component(PythonComponent.build(Delta())).with_time_axis(axis4)
         .with_exogenous_variable("Temperature", core.Timeseries(np.array([288.0, 289.0, 290.5, 291.0]), axis4, "K", core.InterpolationStrategy.Previous))
         .build())
    m.run()
    out = m.timeseries().get_timeseries_by_name("Output").values()
    assert np.isnan(out[0]) and list(out[1:]) == [0.0, 1.0, 1.5]
    m.close()

    class PyCO2ERF(Component, register=False):
        conc = Input("Atmospheric Concentration|CO2", unit="ppm")
        erf = Output("Effective Radiative Forcing|CO2", unit="W/m^2")

        def solve(self, t_current, t_next, inputs):
            c = inputs.conc.get()   # UpstreamOutput: the concentration CarbonCycle has just written
            return self.Outputs(erf=3.7 / math.log(2.0) * math.log(1.0 + (c - 278.0) / 278.0))

    class Anomaly(Component, register=False):
        ts = Input("Surface Temperature", unit="K")
        td = Input("Deep Ocean Temperature", unit="K")
        gap = Output("Surface minus Deep", unit="K")

        def solve(self, t_current, t_next, inputs):
            return self.Outputs(gap=inputs.ts.get() - inputs.td.get())

    t = np.arange(1750.0, 1801.0)
    axis = core.TimeAxis.from_values(t)
    tl = dict(lambda0=1.1, a=0.0, efficacy=1.3, eta=0.7, heat_capacity_surface=8.0, heat_capacity_deep=100.0)

    def graph(python_erf):
        schema = core.VariableSchema()
        for n in ("Emissions|CO2|Anthropogenic", "Surface Temperature", "Deep Ocean Temperature", "Atmospheric Concentration|CO2",
                  "Cumulative Land Uptake", "Cumulative Emissions|CO2", "Effective Radiative Forcing|CO2", "Surface minus Deep"):
            schema.add_variable(n, "")
        schema.add_aggregate("Effective Radiative Forcing", "", "Sum", ["Effective Radiative Forcing|CO2"])
        b = (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
             .with_rust_component(CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.1)).build()))
        if python_erf:
            b.with_py_component(PythonComponent.build(PyCO2ERF()))
        else:
            b.with_rust_component(CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=278.0)).build())
        b.with_rust_component(TwoLayerBuilder.from_parameters(tl).build())
        if python_erf:
            b.with_py_component(PythonComponent.build(Anomaly()))
        b.with_exogenous_variable("Emissions|CO2|Anthropogenic", core.Timeseries(emissions_syn(t) + 2.0, axis, "", core.InterpolationStrategy.Linear))
        b.with_initial_values({"Cumulative Land Uptake": 0.0, "Cumulative Emissions|CO2": 0.0, "Atmospheric Concentration|CO2": 278.0,
                               "Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0})
        return b.build(n_members=3)

    gpu, mixed = graph(False), graph(True)
    assert isinstance(gpu, core.Model) and isinstance(mixed, core.GraphModel)   # all-GPU: the fused coupled kernel
    assert list(mixed._order) == ["CarbonCycle", "PyCO2ERF", "Aggregator:Effective Radiative Forcing", "TwoLayer", "Anomaly"]
    assert mixed.variable_sources()[("Atmospheric Concentration|CO2", "PyCO2ERF")] == "UpstreamOutput"
    gpu.run()
    mixed.run()
    for name in ("Surface Temperature", "Atmospheric Concentration|CO2", "Effective Radiative Forcing|CO2", "Effective Radiative Forcing"):
        g, w = mixed.get_series(name), gpu.ensemble.get_series(name)
        assert (np.isnan(g) == np.isnan(w)).all(), name
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= 1e-12 * np.maximum(1.0, np.abs(w[ok]))).all(), name
    gap = mixed.get_series("Surface minus Deep")
    assert np.isnan(gap[0]).all() and np.array_equal(gap[1:], mixed.get_series("Surface Temperature")[1:] - mixed.get_series("Deep Ocean Temperature")[1:])
    assert mixed.get_series("Surface Temperature")[-1, 0] > 0.05
    with pytest.raises(NotImplementedError, match="Python components"):
        mixed.checkpoint()
    gpu.close()
    mixed.close()


def test_chain_members_are_independent(ra):
    """Every member of an ensemble run of the ten-component graph equals the one-member model with that
    member's parameters, bit for bit (no cross-member coupling anywhere in the linked kernels)."""
    from rscm_amd import _lib as L
    mod = magicc_chain()
    years, N = 40, 5
    big = mod.build_chain(N, years, "topological")
    P_ud = big.ensembles["ClimateUDEB"].get_params()
    P_tc = big.ensembles["TerrestrialCarbon"].get_params()
    assert len(set(P_ud[L.UD_PARAM_NAMES.index("ecs")])) == N      # the members really differ
    big.run()
    names = ["Atmospheric Concentration|CO2", "Atmospheric Concentration|CH4", "Sea Surface Temperature", "Cumulative Ocean Uptake",
             "Carbon Pool|Humus", "Effective Radiative Forcing"]
    want = {n: big.get_series(n) for n in names}
    big.close()
    for k in range(N):
        one = mod.build_chain(1, years, "topological")
        one.ensembles["ClimateUDEB"].set_params(P_ud[:, k:k + 1].copy())
        one.ensembles["TerrestrialCarbon"].set_params(P_tc[:, k:k + 1].copy())
        one.run()
        for n in names:
            assert_bit_equal(one.get_series(n)[:, 0], want[n][:, k], f"member {k} {n}")
        one.close()


def test_chain_full_size_properties(ra):
    """BASELINE configs[3] size (1e5 members; 150 years to keep the test short): a second run of the
    same model object gives the same bits (launch order, split ocean tiles and the cleared series are
    deterministic), and the first 777 members equal a 777-member ensemble with their parameters (the
    result of a member does not depend on the ensemble it sits in, its block or its lane)."""
    mod = magicc_chain()
    years, N, n_small = 150, 100_000, 777
    big = mod.build_chain(N, years, "topological")
    big.run()
    names = ["Atmospheric Concentration|CO2", "Sea Surface Temperature", "Cumulative Ocean Uptake", "Effective Radiative Forcing"]
    first = {n: big.get_series(n, t_begin=years - 1, m_end=2048) for n in names}
    head = {n: big.get_series(n, m_end=n_small) for n in names}
    assert big.ensembles["CO2Budget"].summary(1, years)["count"] == N
    big.rewind()
    big.run()
    for n in names:
        assert_bit_equal(big.get_series(n, t_begin=years - 1, m_end=2048), first[n], f"rerun {n}")
    P_ud = big.ensembles["ClimateUDEB"].get_params()[:, :n_small].copy()
    P_tc = big.ensembles["TerrestrialCarbon"].get_params()[:, :n_small].copy()
    big.close()
    small = mod.build_chain(n_small, years, "topological")
    small.ensembles["ClimateUDEB"].set_params(P_ud)
    small.ensembles["TerrestrialCarbon"].set_params(P_tc)
    small.run()
    for n in names:
        assert_bit_equal(small.get_series(n), head[n], f"sub-ensemble {n}")
    small.close()


def test_graph_models_release_what_they_allocate(ra):
    """Build / run / close cycles of the thirteen-ensemble graph (handles, linked references, the
    shared stream, split-tile scratch, internal states) do not eat device memory: after the
    runtime's own pools (code objects, queue scratch -- a one-off few hundred MB) have settled over
    the first cycles, 24 more cycles leave the free memory where it was.  A leak of one ensemble's
    buffers per cycle would show as > 300 MB here."""
    from rscm_amd import _lib as L
    mod = magicc_chain()

    def cycle(k):
        m = mod.build_chain(20_000, 20, "topological" if k % 2 else "reference")
        m.run()
        if k % 3 == 0:
            m.rewind()
            m.run()
        m.close()

    for k in range(12):
        cycle(k)
    free0, _ = L.mem_info(0)
    for k in range(24):
        cycle(k)
    free1, _ = L.mem_info(0)
    print(f"free-memory change over 24 build/run/close cycles: {(free0 - free1) / 2**20:.1f} MiB")
    # one cycle allocates ~0.6 GB (20 000 members x 13 ensembles); a leak of any one ensemble's series
    # per cycle would be > 24 x 3 MB x (its variables).  Measured on an MI355X after the 12 warm-up
    # cycles: 0.0 MiB; the bound leaves room for a few of the runtime's 2 MiB granules either way.
    assert abs(free0 - free1) <= 8 << 20, (free0, free1)
