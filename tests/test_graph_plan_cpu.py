"""CPU tier: what ``ModelBuilder.build()`` asks of the library on the graph path, and the plan it is read off.

``tests/golden/graph_build_transcripts.json`` holds, per graph below, the transcript ``tests/host_graph_recorder.py`` took of the
commit BEFORE the builder was split into a host plan (``rscm_amd/graph_plan.py``) and its realisation -- every ensemble created
with its arguments, every parameter row, link, table and initial value, in call order -- and the ``GraphModel`` attributes that
tests and ``serialise`` read; of each call and each attribute it keeps a digest, and a failing test prints the call.  ``build()``
has to reproduce both exactly.  The plan-level tests below assert decisions that could only fail on a GPU before: aggregate stages,
the transform's position, the links that run ahead of their producer; and that every refusal is raised before a stream or an
ensemble exists.  ``python -m tests.test_graph_plan_cpu`` rewrites the golden file."""
import hashlib
import json
import math
import os
import re

import numpy as np
import pytest

from rscm_amd import _lib as L
from rscm_amd import core
from rscm_amd import magicc as B
from rscm_amd.component import Component, Input, Output, PythonComponent, State
from rscm_amd.components import CarbonCycleBuilder, CO2ERFBuilder, FourBoxOceanHeatUptakeBuilder
from rscm_amd.two_layer import TwoLayerBuilder
from tests import host_graph_recorder as hr
from tests.helpers import magicc_chain
from tests.test_host_frontend import P_TL, _coupled_builder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_build_transcripts.json")
N = 3
LINEAR = core.InterpolationStrategy.Linear
INIT = {"Cumulative Land Uptake": 0.0, "Cumulative Emissions|CO2": 0.0, "Atmospheric Concentration|CO2": 278.0,
        "Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}
TL_A = dict(lambda0=0.9, a=0.02, efficacy=1.1, eta=0.6, heat_capacity_surface=7.0, heat_capacity_deep=90.0)
ERF = "Effective Radiative Forcing"


# ------------------------------------------------------------------------------------ the graphs
def coupled(emissions_unit="GtC / yr", conc_pi=285.0):
    """tests/test_host_frontend.py::_coupled_builder; ``conc_pi`` of CO2ERF differs from CarbonCycle's, so build() takes the graph
    path.  The emissions come on an axis of their own (resampled at build); ``emissions_unit=None``: nobody supplies them."""
    b = _coupled_builder().with_initial_values(INIT)
    b._components[1] = CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=conc_pi)).build()
    if emissions_unit is not None:
        years = np.array([1750.0, 1753.0, 1758.0, 1765.0])
        b.with_exogenous_variable("Emissions|CO2|Anthropogenic",
                                  core.Timeseries([0.0, 0.5, 3.0, 7.0], core.TimeAxis.from_values(years), emissions_unit, LINEAR))
    return b


def two_of_a_type(at):
    """A second TwoLayer registered second (``at=1``) or last (``at=4``): the one that runs last stands."""
    b = coupled(conc_pi=278.0)
    b._components.insert(at, TwoLayerBuilder.from_parameters(TL_A).build())
    return b


TWO_AGGREGATES = [(ERF, "Sum", ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other"]),
                  ("Diagnostic", "Mean", ["Surface Temperature", "Deep Ocean Temperature"])]


def reader_between_two_of_a_type():
    """CarbonCycle, CO2ERF, CarbonCycle, CarbonCycle: the first CarbonCycle runs first, CO2ERF reads its concentration at the end of
    the step, and only then does the CarbonCycle that stands override it."""
    return permuted_coupled(("CarbonCycle", "CO2ERF", "CarbonCycle", "CarbonCycle"), TWO_AGGREGATES[:1])


def permuted_coupled(perm, aggregates):
    """The graph of tests/test_gpu_links.py::test_graph_model_vs_generic_stepper_every_registration_order."""
    make = {"CarbonCycle": lambda: CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.1)).build(),
            "CO2ERF": lambda: CO2ERFBuilder.from_parameters(dict(erf_2xco2=3.7, conc_pi=278.0)).build(),
            "TwoLayer": lambda: TwoLayerBuilder.from_parameters(P_TL).build()}
    t = np.arange(1750.0, 1759.0)
    axis = core.TimeAxis.from_values(t)
    schema = core.VariableSchema()
    for n in list(INIT) + ["Effective Radiative Forcing|CO2", "Effective Radiative Forcing|Other", "Emissions|CO2|Anthropogenic"]:
        schema.add_variable(n, "")
    for name, op, contributors in aggregates:
        schema.add_aggregate(name, "", op, contributors)
    b = core.ModelBuilder().with_time_axis(axis).with_schema(schema).with_initial_values(INIT)
    for k in perm:
        b.with_rust_component(make[k]())
    b.with_exogenous_variable("Emissions|CO2|Anthropogenic", core.Timeseries(2.0 + 0.1 * (t - 1750.0), axis, "", LINEAR))
    b.with_exogenous_variable("Effective Radiative Forcing|Other", core.Timeseries(0.3 - 0.05 * (t - 1754.0) ** 2, axis, "", LINEAR))
    return b


def udeb_write_transform():
    """ClimateUDEB's FourBox surface temperature read by CarbonCycle as a scalar and stored as a scalar by the schema; one scalar
    initial value for the four regions; area weights that are not the default."""
    t = np.arange(1850.0, 1859.0)
    axis = core.TimeAxis.from_values(t)
    schema = core.VariableSchema()
    for n in ("Emissions|CO2|Anthropogenic", "Surface Temperature", "Atmospheric Concentration|CO2", "Cumulative Land Uptake",
              "Cumulative Emissions|CO2", ERF, "Heat Uptake", "Ocean Heat Content", "Sea Surface Temperature"):
        schema.add_variable(n, "")
    return (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
            .with_grid_weights(core.GridType.FourBox, [0.3, 0.2, 0.4, 0.1])
            .with_rust_component(B.ClimateUDEBBuilder.from_parameters({}).build())
            .with_rust_component(CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.1)).build())
            .with_exogenous_variable(ERF, core.Timeseries(0.1 * (t - 1850.0), axis, "", LINEAR))
            .with_exogenous_variable("Emissions|CO2|Anthropogenic", core.Timeseries(2.0 + 0.0 * t, axis, "", LINEAR))
            .with_initial_values({"Surface Temperature": 0.7, "Atmospheric Concentration|CO2": 278.0, "Cumulative Land Uptake": 0.0,
                                  "Cumulative Emissions|CO2": 0.0}))


def fourbox_aggregate(operation, grid=None):
    """tests/test_gpu_frontend.py::test_fourbox_aggregate_per_region_and_its_scalar_view, with an initial value for the aggregate."""
    grid = grid or core.GridType.FourBox
    t = np.arange(1850.0, 1863.0)
    axis = core.TimeAxis.from_values(t)
    yr = t - 1850.0
    direct, uptake = "Effective Radiative Forcing|Aerosol|Direct", "Heat Uptake|Ocean"
    exo = {"Emissions|SOx": 2.0 + 1.5 * yr, "Emissions|BC": 2.5 + 0.1 * yr, "Emissions|OC": 10.0 + 0.3 * yr, "Emissions|NOx": 10.0 + 0.5 * yr,
           "Effective Radiative Forcing|Aggregated": 0.5 + 0.04 * yr - 0.01 * (yr - 6.0) ** 2}   # (arithmetic only: the tables are compared by hash)
    schema = core.VariableSchema()
    for n in list(exo) + ["Surface Temperature", "Deep Ocean Temperature"]:
        schema.add_variable(n, "")
    schema.add_variable(direct, "", grid)
    schema.add_variable(uptake, "", grid)
    schema.add_aggregate(ERF, "", operation, [direct, uptake], [1.0, -0.5] if operation == "Weighted" else None, grid_type=grid)
    ratios = dict(northern_ocean_ratio=1.1, northern_land_ratio=0.8, southern_ocean_ratio=1.2, southern_land_ratio=0.9)
    b = (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
         .with_grid_weights(core.GridType.FourBox, [0.3, 0.2, 0.4, 0.1])
         .with_rust_component(B.AerosolDirectBuilder.from_parameters({}).build())
         .with_rust_component(FourBoxOceanHeatUptakeBuilder.from_parameters(ratios).build())
         .with_rust_component(TwoLayerBuilder.from_parameters(P_TL).build())
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0, ERF: 0.7}))
    for n, v in exo.items():
        b.with_exogenous_variable(n, core.Timeseries(v, axis, "", LINEAR))
    return b


def wide_aggregate(operation, count):
    """tests/test_gpu_frontend.py::test_aggregate_of_more_than_eight_contributors with ``count`` contributors."""
    t = np.arange(1850.0, 1856.0)
    axis = core.TimeAxis.from_values(t)
    names = [f"Effective Radiative Forcing|Part{k}" for k in range(count)]
    schema = core.VariableSchema()
    for n in names + ["Surface Temperature", "Deep Ocean Temperature"]:
        schema.add_variable(n, "")
    schema.add_aggregate(ERF, "W/m^2", operation, names, [0.5 + 0.25 * k for k in range(count)] if operation == "Weighted" else None)
    b = (core.ModelBuilder().with_time_axis(axis).with_schema(schema).with_rust_component(TwoLayerBuilder.from_parameters(P_TL).build())
         .with_initial_values({"Surface Temperature": 0.0, "Deep Ocean Temperature": 0.0}))
    for k, n in enumerate(names):
        b.with_exogenous_variable(n, core.Timeseries(0.1 * k + 0.01 * (t - 1850.0), axis, "W/m^2", core.InterpolationStrategy.Previous))
    return b


class SimpleCarbonCycle(Component, register=False):
    emissions = Input("Emissions|CO2", unit="GtCO2")
    concentration = State("Atmospheric Concentration|CO2", unit="ppm")
    uptake = Output("Carbon Uptake", unit="GtC")

    def __init__(self, sensitivity):
        self.sensitivity = sensitivity

    def solve(self, t_current, t_next, inputs):
        e = inputs.emissions.at_start()
        return self.Outputs(concentration=inputs.concentration.at_start() + e * self.sensitivity, uptake=e * 0.5)


class PyCO2ERF(Component, register=False):
    conc = Input("Atmospheric Concentration|CO2", unit="ppm")
    erf = Output("Effective Radiative Forcing|CO2", unit="W/m^2")

    def solve(self, t_current, t_next, inputs):
        return self.Outputs(erf=3.7 / math.log(2.0) * math.log(1.0 + (inputs.conc.get() - 278.0) / 278.0))


class Anomaly(Component, register=False):
    ts = Input("Surface Temperature", unit="K")
    td = Input("Deep Ocean Temperature", unit="K")
    gap = Output("Surface minus Deep", unit="K")

    def solve(self, t_current, t_next, inputs):
        return self.Outputs(gap=inputs.ts.get() - inputs.td.get())


def python_graph():
    """The mixed graph of tests/test_gpu_links.py::test_python_components_in_a_gpu_graph: CO2ERF and a diagnostic written in Python
    between the GPU CarbonCycle and TwoLayer."""
    t = np.arange(1750.0, 1760.0)
    axis = core.TimeAxis.from_values(t)
    schema = core.VariableSchema()
    for n in ("Emissions|CO2|Anthropogenic", "Surface Temperature", "Deep Ocean Temperature", "Atmospheric Concentration|CO2",
              "Cumulative Land Uptake", "Cumulative Emissions|CO2", "Effective Radiative Forcing|CO2", "Surface minus Deep"):
        schema.add_variable(n, "")
    schema.add_aggregate(ERF, "", "Sum", ["Effective Radiative Forcing|CO2"])
    return (core.ModelBuilder().with_time_axis(axis).with_schema(schema)
            .with_rust_component(CarbonCycleBuilder.from_parameters(dict(tau=25.0, conc_pi=278.0, alpha_temperature=0.1)).build())
            .with_py_component(PythonComponent.build(PyCO2ERF()))
            .with_rust_component(TwoLayerBuilder.from_parameters(P_TL).build())
            .with_py_component(PythonComponent.build(Anomaly()))
            .with_exogenous_variable("Emissions|CO2|Anthropogenic", core.Timeseries(2.0 + 0.3 * (t - 1750.0), axis, "", LINEAR))
            .with_initial_values(INIT))


def python_alone(copies=1):
    axis = core.TimeAxis.from_values(np.array([2020.0, 2021.0, 2022.0]))
    b = core.ModelBuilder().with_time_axis(axis)
    for _ in range(copies):
        b.with_py_component(PythonComponent.build(SimpleCarbonCycle(0.5)))
    return (b.with_exogenous_variable("Emissions|CO2", core.Timeseries(np.array([10.0, 10.0, 10.0]), axis, "GtCO2", core.InterpolationStrategy.Previous))
            .with_initial_values({"Atmospheric Concentration|CO2": 280.0}))


def chain(order, **kw):
    """scripts/bench_magicc_chain.py::build_chain on 12 years: ten components, one aggregate of eight, a write transform."""
    return lambda n: magicc_chain().build_chain(n, 12, order, **kw)


CHAIN_OUTPUTS = ["Surface Temperature", "Atmospheric Concentration|CO2", "Carbon Pool|Soil"]

# name -> (n_members -> GraphModel)
CASES = {
    "coupled, reference order": lambda n: coupled().build(n_members=n),
    "coupled, topological order": lambda n: coupled().build(n_members=n, execution_order="topological"),
    "coupled, emissions not supplied": lambda n: coupled(emissions_unit=None).build(n_members=n),
    "two aggregates, CarbonCycle registered last": lambda n: permuted_coupled(("CO2ERF", "TwoLayer", "CarbonCycle"), TWO_AGGREGATES).build(n_members=n),
    "second TwoLayer registered second": lambda n: two_of_a_type(1).build(n_members=n),
    "second TwoLayer registered last": lambda n: two_of_a_type(4).build(n_members=n),
    "ClimateUDEB write transform, reference order": lambda n: udeb_write_transform().build(n_members=n),
    "ClimateUDEB write transform, topological order": lambda n: udeb_write_transform().build(n_members=n, execution_order="topological"),
    "FourBox aggregate, Sum": lambda n: fourbox_aggregate("Sum").build(n_members=n, execution_order="topological"),
    "FourBox aggregate, Weighted": lambda n: fourbox_aggregate("Weighted").build(n_members=n, execution_order="topological"),
    "FourBox aggregate, Mean": lambda n: fourbox_aggregate("Mean").build(n_members=n),
    **{f"{op} of {k}": (lambda n, op=op, k=k: wide_aggregate(op, k).build(n_members=n))
       for op, k in (("Sum", 8), ("Sum", 9), ("Sum", 15), ("Sum", 16), ("Weighted", 9), ("Mean", 8), ("Mean", 9), ("Mean", 16))},
    "Python components in a GPU graph": lambda n: python_graph().build(n_members=n),
    "one Python component": lambda n: python_alone().build(n_members=n),
    "chain, reference order": chain("reference"),
    "chain, topological order": chain("topological"),
    "chain, windowed, every output": chain("topological", series_window=8, output_stride=10),
    "chain, windowed, three outputs": chain("topological", series_window=8, output_stride=10, outputs=CHAIN_OUTPUTS),
    "chain, windowed, reference order, three outputs": chain("reference", series_window=8, output_stride=10, outputs=CHAIN_OUTPUTS),
    "chain, window as long as the axis": chain("topological", series_window=13, output_stride=10),
}


def record(case, n=N):
    """(transcript of the build, snapshot of the model): the model is closed inside the recording, after both were taken."""
    with hr.recording() as rec:
        model = CASES[case](n)
        assert isinstance(model, core.GraphModel), case
        out = (list(rec.log), hr.snapshot(model))
        model.close()
    return out


def digest(x):
    """What the golden file keeps of one call or one attribute: 32 bits of the SHA-256 of its JSON text."""
    return hashlib.sha256(json.dumps(x, separators=(",", ":")).encode()).hexdigest()[:8]


def digests(transcript, model):
    """The digest of every call in order, and of every attribute of the model in the order of their names."""
    return {"calls": " ".join(digest(call) for call in transcript), "model": " ".join(digest(model[name]) for name in sorted(model))}


def rewrite_golden():
    """Called by hand only, and only from the commit whose build is the yardstick."""
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(case)}: {json.dumps(digests(*record(case)))}" for case in CASES) + "\n}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_covers_the_cases(golden):
    assert sorted(golden) == sorted(CASES)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "two_layer_golden.npz"))


@pytest.mark.parametrize("case", list(CASES))
def test_build_asks_the_library_what_it_asked_before(golden, case):
    """Call for call, in order: the ensembles created and their arguments, streams, parameter rows, step sizes, links and their
    source flags, switched-off order checks, tables, initial values; then the attributes of the model, dict and list order included."""
    transcript, model = record(case)
    got, want = digests(transcript, model), golden[case]
    for k, (got_call, want_call) in enumerate(zip(got["calls"].split(), want["calls"].split())):
        assert got_call == want_call, f"{case}: call {k} is {transcript[k]}"
    assert len(got["calls"]) == len(want["calls"])
    for name, got_value, want_value in zip(sorted(model), got["model"].split(), want["model"].split()):
        assert got_value == want_value, f"{case}: GraphModel.{name} is {model[name]}"
    assert len(got["model"]) == len(want["model"])


# ------------------------------------------------------------------------------------ the plan itself
def plan_of(builder, endogenous=None, **kw):
    resolved, sources, exo_names, aggregates = builder._resolve()
    return builder._plan_graph(resolved if endogenous is None else endogenous, sources, exo_names, aggregates, **kw)


def chain_builder(order):
    """The builder ``build_chain`` makes (it keeps it to itself: taken from a model built under the recorder)."""
    with hr.recording():
        model = chain(order)(N)
        model.close()
    return model._builder


def part(k):
    return f"Effective Radiative Forcing|Part{k}"


AGG, PARTIAL = f"Aggregator:{ERF}", f"{ERF}#partial"
OPS = L.AG_OPERATIONS
# (operation, contributors) -> the stages in execution order: (key, operation code, input rows, weights of those rows); a carried
# partial has weight 1 whatever the operation (only Weighted reads it)
STAGES = {
    ("Sum", 8): [(AGG, OPS["Sum"], [part(k) for k in range(8)], [])],
    ("Sum", 9): [(AGG + "#0", OPS["Sum"], [part(k) for k in range(8)], []),
                 (AGG, OPS["Sum"], [PARTIAL + "0", part(8)], [1.0])],
    ("Sum", 15): [(AGG + "#0", OPS["Sum"], [part(k) for k in range(8)], []),
                  (AGG, OPS["Sum"], [PARTIAL + "0"] + [part(k) for k in range(8, 15)], [1.0])],
    ("Sum", 16): [(AGG + "#0", OPS["Sum"], [part(k) for k in range(8)], []),
                  (AGG + "#1", OPS["Sum"], [PARTIAL + "0"] + [part(k) for k in range(8, 15)], [1.0]),
                  (AGG, OPS["Sum"], [PARTIAL + "1", part(15)], [1.0])],
    ("Weighted", 9): [(AGG + "#0", OPS["Weighted"], [part(k) for k in range(8)], [0.5 + 0.25 * k for k in range(8)]),
                      (AGG, OPS["Weighted"], [PARTIAL + "0", part(8)], [1.0, 2.5])],   # the partial enters with weight 1
    ("Mean", 8): [(AGG, OPS["Mean"], [part(k) for k in range(8)], [])],
    ("Mean", 9): [(AGG + "#0", OPS["Sum"], [part(k) for k in range(8)], []),
                  (AGG + "#1", OPS["Sum"], [PARTIAL + "0", part(8)], [1.0]),
                  (AGG + "#count0", OPS["Count"], [part(k) for k in range(8)], []),
                  (AGG + "#count1", OPS["CountCarry"], [PARTIAL + "count0", part(8)], [1.0]),
                  (AGG, OPS["Quotient"], [PARTIAL + "1", PARTIAL + "count1"], [])],
}


@pytest.mark.parametrize("operation,count", list(STAGES))
def test_aggregate_stages_at_their_edges(operation, count):
    """An aggregate ensemble takes eight contributors: the first stage takes 8, every later one its predecessor's partial and 7
    more; the stages run next to one another, the aggregate itself last, ahead of its reader; each contributor is an exogenous row
    of its stage's table and each partial a link to the stage before."""
    plan = plan_of(wide_aggregate(operation, count))
    want = STAGES[(operation, count)]
    assert plan.stages == {ERF: [(key, rows) for key, _, rows, _ in want]}
    assert plan.order == [key for key, _, _, _ in want] + ["TwoLayer"]
    for key, op, rows, weights in want:
        assert plan.node(key).params == [op] + weights + [0.0] * (L.AG_NINPUTS - len(weights)), key
        assert plan.var_home[ERF if key == AGG else key.replace("Aggregator:", "").replace("#", "#partial")] == (key, 1)
        consumer = next(c for c in plan.consumers if c.key == key)
        assert [(k.row, k.producer, k.var, k.source, k.before_producer) for k in consumer.links] == [
            (row, plan.var_home[name][0], 1, L.SRC_UPSTREAM, False) for row, name in enumerate(rows) if "#partial" in name]
        supplied = [row for row, name in enumerate(rows) if "#partial" not in name]
        if not supplied:   # the quotient of the two chains reads links only: no table
            assert consumer.table is None
            continue
        assert consumer.table.shape == (L.AG_NINPUTS, 6)
        assert [row for row in range(L.AG_NINPUTS) if not np.isnan(consumer.table[row]).all()] == supplied
    assert plan.feed_forward and not plan.reads_unwritten


def test_fourbox_aggregate_plan():
    """Four per-region aggregates over the contributors' regions, then the scalar view under the aggregate's name; one scalar initial
    value goes to the four regions and, summed over the area weights left to right, to the view."""
    plan = plan_of(fourbox_aggregate("Weighted"), execution_order="topological")
    mine = [f"{AGG}|box{b}" for b in range(4)] + [f"Transform:{ERF}"]
    at = plan.order.index(mine[0])
    assert plan.order[at:at + 5] == mine and plan.order[at + 5] == "TwoLayer"
    assert plan.stages[ERF][-1] == (f"Transform:{ERF}", [f"{ERF}|box{b}" for b in range(4)])
    assert plan.fourbox_aggregates == {ERF: [(f"{AGG}|box{b}", 1) for b in range(4)]}
    for b in range(4):
        assert plan.node(f"{AGG}|box{b}").params == [OPS["Weighted"], 1.0, -0.5] + [0.0] * 6
        assert plan.var_home[f"Effective Radiative Forcing|Aerosol|Direct|box{b}"] == ("AerosolDirect", 1 + b)
        assert plan.var_home[f"Heat Uptake|Ocean|box{b}"] == ("FourBoxOceanHeatUptake", 1 + b)
    assert plan.node(f"Transform:{ERF}").params == [OPS["Weighted"], 0.3, 0.2, 0.4, 0.1, 0.0, 0.0, 0.0, 0.0]
    view = (((0.0 + 0.7 * 0.3) + 0.7 * 0.2) + 0.7 * 0.4) + 0.7 * 0.1
    assert plan.initial[-5:] == [(f"{AGG}|box{b}", 1, 0.7) for b in range(4)] + [(f"Transform:{ERF}", 1, view)]
    assert plan.var_home[ERF] == (f"Transform:{ERF}", 1)


def test_write_transform_position():
    """The scalar of ClimateUDEB's FourBox temperature runs right after ClimateUDEB in the reference's order.  In the topological
    order OceanCarbon -- a kernel of its own that does not read the temperature -- follows ClimateUDEB, and the transform moves behind
    it, next to TerrestrialCarbon, which reads it and shares a fused launch with it."""
    name = "Transform:Surface Temperature"
    reference, topological = (plan_of(chain_builder(o), execution_order=o) for o in ("reference", "topological"))
    at = reference.order.index("ClimateUDEB")
    assert reference.order[at + 1] == name
    at = topological.order.index("ClimateUDEB")
    assert topological.order[at + 1:at + 4] == ["OceanCarbon", name, "TerrestrialCarbon"]
    assert "OceanCarbon" in core.OWN_KERNEL_TYPES and "TerrestrialCarbon" not in core.OWN_KERNEL_TYPES
    for plan in (reference, topological):
        assert plan.var_home["Surface Temperature"] == (name, 1) and plan.fourbox["Surface Temperature"] == ("ClimateUDEB", 1, False)
        assert [(k.row, k.producer, k.var, k.source) for k in plan.node(name).links] == [(b, "ClimateUDEB", 1 + b, L.SRC_UPSTREAM) for b in range(4)]
    small = plan_of(udeb_write_transform())
    assert small.fourbox["Surface Temperature"] == ("ClimateUDEB", 1, True)   # the schema stores the scalar
    view = (((0.0 + 0.7 * 0.3) + 0.7 * 0.2) + 0.7 * 0.4) + 0.7 * 0.1
    assert small.initial[-5:] == [("ClimateUDEB", v, 0.7) for v in (1, 2, 3, 4)] + [(name, 1, view)]


@pytest.mark.parametrize("order,unwritten", [("reference", True), ("topological", False)])
def test_consumers_that_run_ahead_of_their_producer(order, unwritten):
    """A link is flagged exactly where its producer comes later in the final order; the link order check is switched off for those
    links and no other; a flagged link that reads the end of the step makes the graph one that reads unwritten rows -- the
    breadth-first order of the chain has such links, the topological order only lagged feedbacks."""
    plan = plan_of(chain_builder(order), execution_order=order)
    at = {key: k for k, key in enumerate(plan.order)}
    flagged = [(k.consumer, k.row) for k in plan.links if k.before_producer]
    assert flagged == [(k.consumer, k.row) for k in plan.links if at[k.producer] > at[k.consumer]] and flagged
    assert plan.reads_unwritten == unwritten == any(k.before_producer and k.source == L.SRC_UPSTREAM for k in plan.links)
    assert not plan.feed_forward
    calls, model = json.loads(json.dumps(record(f"chain, {order} order")))   # (the recorded build: the test above)
    created = [key for key, _ in model["ensembles"]]
    off = [(created[c[1]["ensemble"]], calls[k - 1][2]) for k, c in enumerate(calls) if c[0] == "rscm_ens_set_link_order_check"]
    assert off == flagged and all(calls[k - 1][0] == "link_input" and c[2] == 0 for k, c in enumerate(calls) if c[0] == "rscm_ens_set_link_order_check")


def test_an_input_nobody_supplies_is_a_nan_row():
    plan = plan_of(coupled(emissions_unit=None))
    cc = next(c for c in plan.consumers if c.key == "CarbonCycle")
    assert cc.table.shape == (2, 11) and np.isnan(cc.table).all() and np.isnan(plan.exogenous["Emissions|CO2|Anthropogenic"]).all()
    assert [(k.row, k.producer, k.source, k.before_producer) for k in cc.links] == [(1, "TwoLayer", L.SRC_EXOGENOUS, True)]
    assert not plan.reads_unwritten and not plan.feed_forward   # a lagged feedback: the value of the step before


def test_windowed_storage():
    """A windowed graph keeps ``series_window`` rows everywhere and every ``output_stride``-th row of the wanted outputs: a FourBox
    variable by its four regions and its scalar, nothing of an ensemble none of whose variables is wanted."""
    builder = chain_builder("topological")
    plan = plan_of(builder, execution_order="topological", series_window=8, output_stride=10, outputs=CHAIN_OUTPUTS)
    assert plan.windowed and plan.output_stride == 10 and all(n.window_rows == 8 for n in plan.nodes)
    kept = {n.key: (n.output_stride, n.output_vars) for n in plan.nodes}
    assert kept["ClimateUDEB"] == (10, [1, 2, 3, 4]) and kept["Transform:Surface Temperature"] == (10, None)
    assert kept["TerrestrialCarbon"] == (10, [L.TC_VARS["Carbon Pool|Soil"]]) and kept["CO2Budget"] == (10, [L.CB_VARS["Atmospheric Concentration|CO2"]])
    assert kept["OceanCarbon"] == (0, []) and kept[AGG] == (0, None) and kept["Transform:Effective Radiative Forcing|Aerosol|Direct"] == (0, None)
    every = plan_of(builder, execution_order="topological", series_window=8, output_stride=10)
    assert all((n.window_rows, n.output_stride, n.output_vars) == (8, 10, None) for n in every.nodes)
    whole = plan_of(builder, execution_order="topological", series_window=13, output_stride=10)   # 13 points: not windowed after all
    assert not whole.windowed and whole.output_stride == 1 and all(n.window_rows is None and n.output_vars is None for n in whole.nodes)


def test_python_components_plan():
    """A Python component gets one storage ensemble per output, keyed "<Type>:<output>" and never launched; it runs where its type
    name stands in the order, and the plan holds its series once, not per member."""
    plan = plan_of(python_graph())
    assert plan.order == ["CarbonCycle", "PyCO2ERF", AGG, "TwoLayer", "Anomaly"]
    assert [(n.key, n.host_owner) for n in plan.nodes if n.host_owner] == [("PyCO2ERF:Effective Radiative Forcing|CO2", "PyCO2ERF"),
                                                                          ("Anomaly:Surface minus Deep", "Anomaly")]
    assert list(plan.hosts) == ["PyCO2ERF", "Anomaly"] and not plan.feed_forward
    assert plan.hosts["PyCO2ERF"].device_reads == {"Atmospheric Concentration|CO2": ("CarbonCycle", 1)}
    assert plan.hosts["PyCO2ERF"].sources == {"Atmospheric Concentration|CO2": "UpstreamOutput"}
    series = plan.hosts["Anomaly"].series["Surface Temperature"]
    assert series.shape == (10,) and series[0] == 0.0 and np.isnan(series[1:]).all()


def _without_member_counts(x):
    if isinstance(x, dict):
        return {k: "N" if k == "members" else _without_member_counts(v) for k, v in x.items()}
    if isinstance(x, list) and len(x) == 2 and x[0] in ("members", "n_members"):
        return [x[0], "N"]
    return [_without_member_counts(v) for v in x] if isinstance(x, list) else x


def test_one_plan_realised_at_two_sizes(golden):
    """A plan does not depend on the member count: realised for 3 and for 5 members it gives transcripts and models that differ in
    ``n_members`` and the member extent of the arrays alone; the one for 3 is the recorded build."""
    builder = coupled()
    plan = plan_of(builder)
    taken = {}
    for n in (3, 5):
        with hr.recording() as rec:
            model = builder._realise(plan, n)
            taken[n] = json.loads(json.dumps((list(rec.log), hr.snapshot(model))))
            model.close()
    assert digests(*taken[3]) == golden["coupled, reference order"]
    assert taken[3] != taken[5] and _without_member_counts(taken[3]) == _without_member_counts(taken[5])


def test_planning_needs_no_library():
    """The planner imports numpy and the tables of ``_lib`` and nothing that could reach a device; planning the chain leaves the
    library handle as it found it."""
    import ast
    from rscm_amd import graph_plan
    with open(graph_plan.__file__) as f:
        tree = ast.parse(f.read())
    imported = {(n.module or "") if isinstance(n, ast.ImportFrom) else a.name for n in ast.walk(tree)
                if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names}
    assert imported == {"__future__", "dataclasses", "typing", "numpy", ""}   # "": from . import _lib
    assert [a.name for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and not n.module for a in n.names] == ["_lib"]
    assert not any(isinstance(n, ast.Attribute) and n.attr == "load" for n in ast.walk(tree))
    builder = chain_builder("topological")
    before = L._LIB
    plan_of(builder, execution_order="topological")
    assert L._LIB is before


# ------------------------------------------------------------------------------------ refusals
class Foreign(core.Component):
    type_name = "Foreign"
    definitions = [("x", "", "Input"), ("y", "", "Output")]


def _foreign():
    return core.ModelBuilder().with_time_axis(core.TimeAxis.from_values([0.0, 1.0, 2.0])).with_rust_component(Foreign({})).build()


def _mismatched_fourbox_aggregate():
    b = fourbox_aggregate("Sum")
    b._schema.add_variable("Regional Forcing|Other", "", core.GridType.FourBox)   # FourBox in the schema, but nobody's FourBox output
    b._schema.aggregates[ERF].contributors.append("Regional Forcing|Other")
    return b.build()


def _homeless(builder, name):
    """``name`` made endogenous without a home: what a FourBox variable was to a scalar reader before the read transform.  No
    builder reaches the refusal any more (every endogenous variable gets a home); the planner keeps it."""
    endogenous = dict(builder._resolve()[0])
    endogenous[name] = "Elsewhere"
    return plan_of(builder, endogenous=endogenous)


REFUSALS = {
    "no GPU kernel": (_foreign, NotImplementedError, "component Foreign has no GPU kernel; supported: "),
    "two Python components of one type": (lambda: python_alone(2).build(), NotImplementedError,
                                          "two Python components of the same type in one graph: SimpleCarbonCycle"),
    "bad execution_order": (lambda: coupled().build(execution_order="bfs"), ValueError, "execution_order must be 'reference' or 'topological'"),
    "not reachable from the root": (lambda: permuted_coupled(("TwoLayer", "CarbonCycle", "CO2ERF"), TWO_AGGREGATES).build(), NotImplementedError,
                                    "components not reachable from the graph root: ['TwoLayer', 'CarbonCycle', 'CO2ERF', "),
    "reads before override": (lambda: reader_between_two_of_a_type().build(), NotImplementedError,
                              "CO2ERF reads ['Atmospheric Concentration|CO2'] of CarbonCycle#1 within the step, before CarbonCycle overrides them"),
    "Hemispheric aggregate": (lambda: fourbox_aggregate("Sum", core.GridType.Hemispheric).build(), NotImplementedError,
                              "aggregate 'Effective Radiative Forcing': no component of this package produces a Hemispheric variable"),
    "Grid type mismatch": (_mismatched_fourbox_aggregate, ValueError,
                           "Grid type mismatch: contributor 'Regional Forcing|Other' of the FourBox aggregate 'Effective Radiative Forcing' is not a FourBox variable"),
    "FourBox variable, device reader": (lambda: _homeless(coupled(), "Emissions|CO2|Anthropogenic"), NotImplementedError,
                                        "'Emissions|CO2|Anthropogenic' is a FourBox variable: it cannot feed the scalar input of CarbonCycle"),
    "FourBox variable, host reader": (lambda: _homeless(python_alone(), "Emissions|CO2"), NotImplementedError,
                                      "'Emissions|CO2' is a FourBox variable: it cannot feed the scalar input of SimpleCarbonCycle"),
    "unit conversion": (lambda: coupled(emissions_unit="MtC / yr").build(), NotImplementedError,
                        "unit conversion is not available on the GPU path: 'Emissions|CO2|Anthropogenic' is supplied in 'MtC / yr', expected ['GtC/yr']"),
}


@pytest.mark.parametrize("refusal", list(REFUSALS))
def test_every_refusal_comes_before_anything_exists(refusal):
    """Type and message as they were; and the recorder has seen no stream and no ensemble when it is raised (before the plan, those
    raised while wiring -- grid type, FourBox reader, units -- left a stream and ensembles to close)."""
    attempt, error, message = REFUSALS[refusal]
    with hr.recording() as rec:
        with pytest.raises(error, match="^" + re.escape(message)):
            attempt()
        assert rec.log == [] and rec.ensembles == []


if __name__ == "__main__":
    rewrite_golden()
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(CASES)} graphs")
