"""The host plan of a component graph: which linked ensembles ``ModelBuilder.build()`` creates for a graph the fused kernels do not
cover, in which order they are stepped, and what is linked, tabulated and initialised -- decided before anything exists on a device.

``plan_graph`` turns a builder's registered components and schema aggregates into a ``GraphPlan`` of plain records;
``ModelBuilder._realise`` (``rscm_amd/core.py``) creates the stream and the ensembles from it.  Nothing here loads the library,
constructs an ``Ensemble`` or depends on the member count: parameters are vectors, host series are ``[T]``.  Every refusal of a
graph is raised here, so none of them leaves a stream or an ensemble behind."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Set, Tuple

import numpy as np

from . import _lib as L

NAN = float("nan")

SUPPORTED = ("any graph of the built-in components with scalar links (one linked ensemble per component, "
             "stepped in the reference's graph order); fused single-launch kernels for: "
             "[ClimateUDEB] with exogenous 'Effective Radiative Forcing'",
             "[GhgForcing] | [OzoneForcing] | [AerosolDirect] | [AerosolIndirect] | [CH4Chemistry] | "
             "[N2OChemistry] | [CO2Budget] | [TerrestrialCarbon] | [OceanCarbon] | [HalocarbonChemistry] | "
             "[FourBoxOceanHeatUptake] | [OceanSurfacePartialPressure] with their inputs as "
             "exogenous series",
             "[TwoLayer] with exogenous or upstream 'Effective Radiative Forcing'",
             "[CarbonCycle, CO2ERF, TwoLayer] + Sum aggregate 'Effective Radiative Forcing' "
             "over ['Effective Radiative Forcing|CO2'] (registration order as listed)")

# single-component graphs whose inputs are all exogenous rows of the input block
STATELESS_KINDS = {"GhgForcing": L.KIND_GHG_FORCING, "OzoneForcing": L.KIND_OZONE_FORCING,
                   "AerosolDirect": L.KIND_AEROSOL_DIRECT, "AerosolIndirect": L.KIND_AEROSOL_INDIRECT,
                   "CH4Chemistry": L.KIND_CH4_CHEMISTRY, "N2OChemistry": L.KIND_N2O_CHEMISTRY,
                   "CO2Budget": L.KIND_CO2_BUDGET, "TerrestrialCarbon": L.KIND_TERRESTRIAL_CARBON,
                   "OceanCarbon": L.KIND_OCEAN_CARBON, "HalocarbonChemistry": L.KIND_HALOCARBON,
                   "FourBoxOceanHeatUptake": L.KIND_FOURBOX_OHU, "OceanSurfacePartialPressure": L.KIND_OSPP}

# components whose step is a kernel of their own (csrc/kinds.hpp, `fusable`); the others share fused launches
OWN_KERNEL_TYPES = ("ClimateUDEB", "OceanCarbon", "HalocarbonChemistry")

# type name -> ensemble kind, for graphs assembled from linked ensembles
COMPONENT_KINDS = {"TwoLayer": L.KIND_TWO_LAYER, "ClimateUDEB": L.KIND_UDEB, "CarbonCycle": L.KIND_CARBON_CYCLE,
                   "CO2ERF": L.KIND_CO2_ERF, **STATELESS_KINDS}


def is_host_component(comp) -> bool:
    """A component written in Python (``rscm_amd.component.PythonComponent``): stepped on the host, no kernel."""
    return bool(getattr(comp, "is_python", False))


def component_param_names(comp) -> Tuple[str, ...]:
    return tuple(L.PARAM_NAMES[COMPONENT_KINDS[comp.type_name]])


def component_params(comp) -> List[float]:
    if hasattr(comp, "param_vector"):
        return list(comp.param_vector())
    return [comp.parameters[k] for k in component_param_names(comp)]


# ------------------------------------------------------------------------------------ records
@dataclass
class GraphNode:
    """A node of the reference's graph while the plan is made.  ``name`` is what ``_graph_order`` calls it; ``key`` what the
    survivor of its type is called from then on (the key of its ensemble, its entry in the order)."""
    type_name: str             # component type, or the aggregate's name
    index: int = 0             # "<type>#<index>" for all but the last registered component of a type (0: the last)
    is_aggregate: bool = False
    survivor: bool = True      # of several components of one type, the one that runs last

    @property
    def name(self) -> str:
        if self.is_aggregate:
            return f"Aggregator:{self.type_name}"
        return f"{self.type_name}#{self.index}" if self.index else self.type_name

    @property
    def key(self) -> str:
        return self.name if self.is_aggregate else self.type_name


class LinkSpec(NamedTuple):
    """Input row ``row`` of ``consumer`` reads variable ``var`` of ``producer``.  ``before_producer``: the consumer runs ahead of
    the producer (lagged feedback, or a breadth-first order that is not a topological one: it then reads NaN at n+1 like in the
    reference), so the library's link order check is switched off for it."""
    consumer: str
    row: int
    producer: str
    var: int
    source: int
    before_producer: bool = False


@dataclass
class NodeSpec:
    """One ensemble to create.  ``links`` are made as soon as it exists (the four regions of a write transform)."""
    key: str
    kind: int
    params: List[float]                            # one value per row
    step_size: Optional[Tuple[int, float]] = None  # (component id, step)
    window_rows: Optional[int] = None
    output_stride: int = 0
    output_vars: Optional[List[int]] = None
    host_owner: Optional[str] = None               # the Python component whose output this ensemble only stores (never launched)
    links: Tuple[LinkSpec, ...] = ()


class ConsumerSpec(NamedTuple):
    """The inputs of one ensemble: its links, then its exogenous table (None if no row needed one)."""
    key: str
    links: List[LinkSpec]
    table: Optional[np.ndarray]


@dataclass
class HostSpec:
    """A Python component: where each input comes from and its host series ``[T]``."""
    comp: object
    sources: Dict[str, str] = field(default_factory=dict)
    device_reads: Dict[str, Tuple[str, int]] = field(default_factory=dict)
    series: Dict[str, np.ndarray] = field(default_factory=dict)


@dataclass
class GraphPlan:
    order: List[str]                       # execution order, transforms and partial stages inserted
    sources: Dict[Tuple[str, str], str]
    execution_order: str
    windowed: bool
    output_stride: int
    nodes: List[NodeSpec] = field(default_factory=list)           # in creation order
    consumers: List[ConsumerSpec] = field(default_factory=list)   # in wiring order
    initial: List[Tuple[str, int, float]] = field(default_factory=list)   # (key, variable id, value), in writing order
    var_home: Dict[str, Tuple[str, int]] = field(default_factory=dict)
    stages: Dict[str, List[Tuple[str, List[str]]]] = field(default_factory=dict)   # aggregate -> (stage key, its input rows)
    fourbox: Dict[str, Tuple[str, int, bool]] = field(default_factory=dict)
    fourbox_aggregates: Dict[str, List[Tuple[str, int]]] = field(default_factory=dict)
    param_home: Dict[str, Tuple[str, int]] = field(default_factory=dict)
    base_params: Dict[str, np.ndarray] = field(default_factory=dict)
    hosts: Dict[str, HostSpec] = field(default_factory=dict)
    exogenous: Dict[str, np.ndarray] = field(default_factory=dict)

    @property
    def links(self) -> List[LinkSpec]:
        """Every link in the order it is made."""
        return [k for n in self.nodes for k in n.links] + [k for c in self.consumers for k in c.links]

    @property
    def feed_forward(self) -> bool:
        """No edge points backwards: every producer can finish before its consumers start."""
        return not self.hosts and not any(k.before_producer for k in self.links)

    @property
    def reads_unwritten(self) -> bool:
        """Some component reads index n+1 of a producer that runs after it."""
        return any(k.before_producer and k.source == L.SRC_UPSTREAM for k in self.links)

    def node(self, key: str) -> NodeSpec:
        return next(n for n in self.nodes if n.key == key)


class Storage(NamedTuple):
    """What a windowed graph keeps: ``series_window`` rows of every series and every ``output_stride``-th row of the wanted
    outputs (``wanted`` None: all variables)."""
    windowed: bool
    series_window: Optional[int]
    output_stride: int
    wanted: Optional[Set[str]]

    def wants(self, name: str) -> bool:
        return self.wanted is None or name in self.wanted

    def of_component(self, kind: int) -> Dict[str, object]:
        if not self.windowed:
            return {}
        ids = L.KIND_TABLE[kind][0]
        keep = None
        if self.wanted is not None:
            fb = L.FOURBOX_VARS.get(kind)
            keep = [v for n, v in ids.items() if v > 0 and (n in self.wanted or (fb and fb[0] in self.wanted and fb[1] <= v < fb[1] + 4))]
        return {"window_rows": self.series_window, "output_stride": self.output_stride if keep is None or keep else 0, "output_vars": keep}

    def of_stage(self, wanted: bool) -> Dict[str, object]:
        return {"window_rows": self.series_window if self.windowed else None, "output_stride": self.output_stride if wanted else 0}


# ------------------------------------------------------------------------------------ survivors
def component_nodes(components) -> List[GraphNode]:
    """One node per registered component.  The reference accepts several components that provide the same variables
    (builder.rs:531-559: the later one becomes the owner, with an edge from the earlier one); each of them writes index n+1 of the
    same series every step, so what stands is the write of whichever runs LAST in the execution order (runtime.rs:504-527).  For
    components of one built-in type -- same variables, same states -- the others' work is never seen: they keep their nodes (the
    edges shape the breadth-first order) but get no ensemble (``survivors``)."""
    last = {c.type_name: k for k, c in enumerate(components)}
    seen: Dict[str, int] = {}
    out = []
    for k, c in enumerate(components):
        if last[c.type_name] != k:
            seen[c.type_name] = seen.get(c.type_name, 0) + 1
        out.append(GraphNode(c.type_name, 0 if last[c.type_name] == k else seen[c.type_name]))
    return out


def check_components(components, nodes: List[GraphNode]) -> None:
    for c, node in zip(components, nodes):
        if c.type_name not in COMPONENT_KINDS and not is_host_component(c):
            raise NotImplementedError(f"component {c.type_name} has no GPU kernel; supported: " + "; ".join(SUPPORTED))
        if node.index and is_host_component(c):
            # host components of one class may declare different variables: they would all be live
            raise NotImplementedError(f"two Python components of the same type in one graph: {c.type_name}")


def _provides(comp) -> Set[str]:
    return {name for name, _, kind in comp.definitions if kind in ("Output", "State")}


def survivors(components, nodes: List[GraphNode], order_names: List[str], aggregates, sources):
    """Of several components of one type the one that runs last stands: the others take part in the ordering only.  Returns the
    order as ensemble keys, the surviving components and the source table with the survivor under its plain type name."""
    by_name = {n.name: (n, c) for n, c in zip(nodes, components)}
    by_name.update({n.name: (n, None) for n in (GraphNode(a, is_aggregate=True) for a in aggregates)})
    missing = [name for name in by_name if name not in order_names]
    if missing:
        raise NotImplementedError(f"components not reachable from the graph root: {missing}")
    order = [by_name[name][0] for name in order_names]
    runs_last: Dict[str, GraphNode] = {}
    for n in order:
        if not n.is_aggregate:
            runs_last[n.type_name] = n
    for at, n in enumerate(order):
        if n.is_aggregate or runs_last[n.type_name] is n:
            continue
        n.survivor = False
        # an overridden component's values ARE seen by whoever reads index n+1 between it and the survivor
        provided = _provides(by_name[n.name][1])
        for reader in order[at + 1:order.index(runs_last[n.type_name])]:
            if reader.is_aggregate:
                reads = set(aggregates[reader.type_name].contributors)
            else:
                reads = {name for name, _, kind in by_name[reader.name][1].definitions
                         if kind == "Input" and sources.get((name, reader.name)) == "UpstreamOutput"}
            if provided & reads:
                raise NotImplementedError(f"{reader.name} reads {sorted(provided & reads)} of {n.name} within the step, before "
                                          f"{runs_last[n.type_name].name} overrides them")
    for n, c in zip(nodes, components):
        if n.survivor and n.index:
            sources = dict(sources)
            for name, _, kind in c.definitions:
                if kind in ("Input", "State"):
                    sources[(name, c.type_name)] = sources[(name, n.name)]
    return [n.key for n in order if n.survivor], [c for n, c in zip(nodes, components) if n.survivor], sources


# ------------------------------------------------------------------------------------ component nodes
def transform_node(storage: Storage, name: str, weights: Sequence[float]) -> NodeSpec:
    """A FourBox variable is four scalar series.  Whoever wants it as a scalar gets sum(value * weight) over the boxes, formed by a
    Weighted aggregate ensemble ``"Transform:<name>"`` that runs after its producer, index by index."""
    return NodeSpec(f"Transform:{name}", L.KIND_AGGREGATE, [L.AG_OPERATIONS["Weighted"]] + list(weights) + [0.0] * 4,
                    **storage.of_stage(storage.wants(name)))


def scalar_view(x0: float, weights: Sequence[float]) -> float:
    """The scalar view of a FourBox variable whose four regions hold ``x0``, summed like aggregate_global."""
    s0 = 0.0
    for wk in weights:
        s0 = s0 + x0 * wk
    return s0


def plan_host_storage(plan: GraphPlan, comp) -> None:
    """A host component's outputs live in one device series each (an aggregate-kind ensemble used as storage, never launched), so
    that GPU components can link to them."""
    for name in comp.output_names():
        key = f"{comp.type_name}:{name}"
        plan.nodes.append(NodeSpec(key, L.KIND_AGGREGATE, [0.0] * (1 + L.AG_NINPUTS), host_owner=comp.type_name))
        plan.var_home[name] = (key, 1)


def plan_component(plan: GraphPlan, builder, storage: Storage, comp, by_type) -> None:
    key, kind = comp.type_name, COMPONENT_KINDS[comp.type_name]
    base = component_params(comp)
    step = (L.COMP_CARBON_CYCLE, comp.step_size) if key == "CarbonCycle" else None
    plan.nodes.append(NodeSpec(key, kind, base, step, **storage.of_component(kind)))
    plan.base_params[key] = np.array(base, dtype=np.float64)
    for row, pname in enumerate(component_param_names(comp)):
        plan.param_home[f"{key}.{pname}"] = (key, row)
        # a bare name addresses the parameter only if no other component has one of that name
        plan.param_home[pname] = (key, row) if pname not in plan.param_home else ("", -1)
    fb = L.FOURBOX_VARS.get(kind)
    for name in comp.output_names():
        if fb and name == fb[0]:
            plan_write_transform(plan, builder, storage, comp, name, fb[1], by_type)
        else:
            plan.var_home[name] = (key, L.KIND_TABLE[kind][0][name])


def plan_write_transform(plan: GraphPlan, builder, storage: Storage, comp, name: str, first: int, by_type) -> None:
    """The scalar of a component's FourBox output: what the collection stores where the schema says Scalar (write transform,
    runtime.rs:452-470) and what a reader that declares a scalar input gets (read transform, state/aggregating.rs:162-176).  It
    runs right after the producer -- or, in the topological order, after the own-kernel components that follow the producer and
    do not read the variable: the transform then shares their successors' launch."""
    node = transform_node(storage, name, builder._fourbox_weights())
    node.links = tuple(LinkSpec(node.key, k, comp.type_name, first + k, L.SRC_UPSTREAM) for k in range(4))
    plan.nodes.append(node)
    at = plan.order.index(comp.type_name) + 1
    if plan.execution_order == "topological":
        while (at < len(plan.order) and plan.order[at] in OWN_KERNEL_TYPES and plan.order[at] in by_type
               and name not in by_type[plan.order[at]].input_names()):
            at += 1
    plan.order.insert(at, node.key)
    plan.var_home[name] = (node.key, 1)
    plan.fourbox[name] = (comp.type_name, first, builder._stored_as_scalar(name))


# ------------------------------------------------------------------------------------ aggregate stages
# An aggregate ensemble takes eight contributors.  More are folded left to right through partial-sum stages -- stage k adds up to
# seven further contributors to the partial of stage k-1 -- which keeps compute_aggregate's order of additions (schema.rs:760-802:
# one running sum over the contributors in declaration order, NaN skipped, all-NaN -> NaN), so the result carries the same bits.
# Weighted: the partial enters the next stage with weight 1.  A Mean of more than eight is that Sum chain, a second chain that
# counts the non-NaN contributors, and a last stage that divides the one by the other (sum / n as f64, NaN for n = 0).
def add_stage(plan: GraphPlan, storage: Storage, agg: str, key: str, op: str, rows: List[str], weights: List[float], out_var: str,
              final: bool) -> None:
    w = list(weights) + [0.0] * (L.AG_NINPUTS - len(weights))
    plan.nodes.append(NodeSpec(key, L.KIND_AGGREGATE, [L.AG_OPERATIONS[op]] + w, **storage.of_stage(final and storage.wants(agg))))
    plan.var_home[out_var] = (key, 1)
    plan.stages[agg].append((key, rows))


def chain_stages(plan: GraphPlan, storage: Storage, agg: str, op: str, carry_op: str, contributors: List[str], wts: List[float],
                 tag: str, final: bool) -> str:
    """Stages over ``contributors``; returns the variable the last one writes."""
    k, n_stage, out_var = 0, 0, ""
    while True:
        first = n_stage == 0
        take = L.AG_NINPUTS if first else L.AG_NINPUTS - 1
        last = len(contributors) - k <= take
        chunk = contributors[k:k + take]
        wchunk = wts[k:k + take] if wts else []
        k += len(chunk)
        is_final = final and last
        key = f"Aggregator:{agg}" if is_final else f"Aggregator:{agg}#{tag}{n_stage}"
        rows = chunk if first else [out_var] + chunk
        wrow = wchunk if first else [1.0] + wchunk
        out_var = agg if is_final else f"{agg}#partial{tag}{n_stage}"
        add_stage(plan, storage, agg, key, op if first else carry_op, rows, wrow, out_var, is_final)
        n_stage += 1
        if last:
            return out_var


def scalar_aggregate(plan: GraphPlan, storage: Storage, agg: str, op: str, contributors: List[str], weights) -> None:
    plan.stages[agg] = []
    if op == "Mean" and len(contributors) > L.AG_NINPUTS:
        total = chain_stages(plan, storage, agg, "Sum", "Sum", contributors, [], "", False)
        count = chain_stages(plan, storage, agg, "Count", "CountCarry", contributors, [], "count", False)
        add_stage(plan, storage, agg, f"Aggregator:{agg}", "Quotient", [total, count], [], agg, True)
    else:
        chain_stages(plan, storage, agg, op, op, contributors, list(weights or []), "", True)


def fourbox_aggregate(plan: GraphPlan, builder, storage: Storage, agg: str, op: str, contributors: List[str], weights) -> None:
    """AggregatorComponent::solve for a FourBox aggregate (schema.rs:902-923): compute_aggregate per region over the contributors'
    values of that region.  A FourBox variable is four scalar series here, so the aggregate is four scalar aggregates
    "<name>|box<k>" (k = 0..3: the reference's region order) over box k of every contributor, plus the scalar view of the result
    -- what a component that declares the variable as a scalar input reads -- under the aggregate's name."""
    stages: List[Tuple[str, List[str]]] = []
    homes = []
    for b in range(4):
        rows_b = []
        for c in contributors:
            cb = f"{c}|box{b}"
            if cb not in plan.var_home:
                if c not in plan.fourbox:
                    raise ValueError(f"Grid type mismatch: contributor {c!r} of the FourBox aggregate {agg!r} is not a FourBox variable")
                owner_c, first_c, _ = plan.fourbox[c]
                plan.var_home[cb] = (owner_c, first_c + b)
            rows_b.append(cb)
        scalar_aggregate(plan, storage, f"{agg}|box{b}", op, rows_b, weights)
        stages += plan.stages.pop(f"{agg}|box{b}")
        homes.append(plan.var_home[f"{agg}|box{b}"])
    node = transform_node(storage, agg, builder._fourbox_weights())
    plan.nodes.append(node)
    plan.var_home[agg] = (node.key, 1)
    plan.stages[agg] = stages + [(node.key, [f"{agg}|box{b}" for b in range(4)])]
    plan.fourbox_aggregates[agg] = homes
    at = plan.order.index(f"Aggregator:{agg}")
    plan.order[at:at + 1] = [key for key, _ in plan.stages[agg]]


def plan_aggregate(plan: GraphPlan, builder, storage: Storage, agg: str, definition) -> None:
    contributors = list(definition.contributors)
    if definition.grid_type.name == "Hemispheric":
        raise NotImplementedError(f"aggregate {agg!r}: no component of this package produces a Hemispheric variable")
    if definition.grid_type.name == "FourBox":
        fourbox_aggregate(plan, builder, storage, agg, definition.operation_type, contributors, definition.weights)
        return
    scalar_aggregate(plan, storage, agg, definition.operation_type, contributors, definition.weights)
    at = plan.order.index(f"Aggregator:{agg}")
    plan.order[at:at] = [key for key, _ in plan.stages[agg][:-1]]   # the partial stages run right before the aggregate itself


# ------------------------------------------------------------------------------------ links and tables
def wire_consumer(plan: GraphPlan, builder, key: str, rows: List[str], read_end: bool, endogenous, exo_names,
                  runs_at: Dict[str, int]) -> ConsumerSpec:
    """Each input row of ``key``: a link to the variable's home, or a row of the exogenous table (never supplied: a NaN series,
    builder.rs:772-780)."""
    input_rows = L.KIND_TABLE[plan.node(key).kind][2]
    table = np.full((len(input_rows) if input_rows else 1, len(builder._axis)), NAN)
    links, use_table = [], False
    for k, name in enumerate(rows):
        if name in plan.var_home:
            producer, vid = plan.var_home[name]
            src = L.SRC_UPSTREAM if read_end or plan.sources.get((name, key)) == "UpstreamOutput" else L.SRC_EXOGENOUS
            links.append(LinkSpec(key, k, producer, vid, src, runs_at[producer] > runs_at[key]))
            continue
        if name in endogenous:
            raise NotImplementedError(f"{name!r} is a FourBox variable: it cannot feed the scalar input of {key}")
        vals = builder._exogenous_on_axis(name, exo_names + list(rows))
        use_table = True
        if vals is not None:
            table[k] = vals
        plan.exogenous[name] = table[k].copy()
    return ConsumerSpec(key, links, (table if input_rows else table[0]) if use_table else None)


def host_reads(plan: GraphPlan, builder, comp, endogenous, exo_names) -> HostSpec:
    """The series a Python component reads: a device variable (refreshed row by row while the model runs) or an exogenous one."""
    host = HostSpec(comp)
    for name in comp.input_names():
        host.sources[name] = plan.sources.get((name, comp.type_name), "Exogenous")
        series = np.full(len(builder._axis), NAN)
        if name in plan.var_home:
            host.device_reads[name] = plan.var_home[name]
            if name in builder._initial:
                series[0] = builder._initial[name]
        else:
            if name in endogenous:
                raise NotImplementedError(f"{name!r} is a FourBox variable: it cannot feed the scalar input of {comp.type_name}")
            vals = builder._exogenous_on_axis(name, exo_names + [name])
            if vals is not None:
                series[:] = vals
            plan.exogenous[name] = series.copy()
        host.series[name] = series
    return host


def plan_inputs(plan: GraphPlan, builder, components, aggregates, endogenous, exo_names) -> None:
    position = {key: k for k, key in enumerate(plan.order)}
    runs_at = {n.key: position[n.host_owner or n.key] for n in plan.nodes}   # a host component's storage runs where it does
    for comp in components:
        if is_host_component(comp):
            plan.hosts[comp.type_name] = host_reads(plan, builder, comp, endogenous, exo_names)
            continue
        kind = COMPONENT_KINDS[comp.type_name]
        var_ids, _, input_rows = L.KIND_TABLE[kind]
        rows = list(input_rows or [n for n, v in var_ids.items() if v == 0])
        plan.consumers.append(wire_consumer(plan, builder, comp.type_name, rows, kind == L.KIND_UDEB, endogenous, exo_names, runs_at))
    for agg in aggregates:
        for key, rows in plan.stages[agg]:
            plan.consumers.append(wire_consumer(plan, builder, key, rows, True, endogenous, exo_names, runs_at))


# ------------------------------------------------------------------------------------ initial values
def plan_initial_values(plan: GraphPlan, initial: Dict[str, float], weights: Sequence[float]) -> None:
    """A FourBox state or aggregate initialised with one scalar sets all four regions (builder.rs:797-804) and the scalar view."""
    for name, (key, vid) in plan.var_home.items():
        if name in initial:
            plan.initial.append((key, vid, initial[name]))
    regions = list(plan.fourbox_aggregates.items())
    for node in plan.nodes:
        if node.kind in L.FOURBOX_VARS:
            name, first = L.FOURBOX_VARS[node.kind]
            regions.append((name, [(node.key, v) for v in range(first, first + 4)]))
    for name, homes in regions:
        if name in initial:
            plan.initial += [(key, vid, initial[name]) for key, vid in homes]
            plan.initial.append((f"Transform:{name}", 1, scalar_view(initial[name], weights)))


# ------------------------------------------------------------------------------------ the plan
def plan_graph(builder, endogenous, sources, exo_names, aggregates, execution_order: str = "reference",
               series_window: Optional[int] = None, output_stride: int = 0, outputs: Optional[Sequence[str]] = None) -> GraphPlan:
    nodes = component_nodes(builder._components)
    check_components(builder._components, nodes)
    if execution_order not in ("reference", "topological"):
        raise ValueError("execution_order must be 'reference' or 'topological'")
    order_names = builder._graph_order(aggregates, topological=execution_order == "topological")
    order, components, sources = survivors(builder._components, nodes, order_names, aggregates, sources)
    windowed = series_window is not None and series_window < len(builder._axis)
    storage = Storage(windowed, series_window, output_stride, None if outputs is None else set(outputs))
    plan = GraphPlan(order, sources, execution_order, windowed, int(output_stride) if windowed else 1)
    by_type = {c.type_name: c for c in components}
    for comp in components:
        if is_host_component(comp):
            plan_host_storage(plan, comp)
        else:
            plan_component(plan, builder, storage, comp, by_type)
    plan.param_home = {k: v for k, v in plan.param_home.items() if v[1] >= 0}
    for agg, definition in aggregates.items():
        plan_aggregate(plan, builder, storage, agg, definition)
    plan_inputs(plan, builder, components, aggregates, endogenous, exo_names)
    plan_initial_values(plan, builder._initial, builder._fourbox_weights())
    return plan
