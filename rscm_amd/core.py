"""Host-side mirror of the reference's Python model-description surface for the hot path.

Same names, argument meaning and error behaviour as ``rscm._lib.core``
(python/rscm/_lib/core/__init__.pyi:19-175,322-463,563-628; implementations under
crates/rscm-core/src/python/), so a script that builds a two-layer or coupled model keeps working:

    model = (ModelBuilder().with_time_axis(axis).with_rust_component(two_layer)
             .with_exogenous_variable("Effective Radiative Forcing", erf)
             .with_initial_values({...}).build())
    model.run(); model.timeseries().get_timeseries_by_name("Surface Temperature").values()

``build()`` resolves the component graph exactly as the reference does
(crates/rscm-core/src/model/builder.rs:418-860: registration-order variable sources, schema
aggregates, missing-initial-value check, exogenous resampling onto the model axis) and maps the
result onto one of the fused HIP kernels.  Graphs outside the supported set raise
``NotImplementedError`` -- there is no generic CPU interpreter and no CPU fallback.

Everything numeric that happens per time step runs on the GPU; the only host arithmetic here is
the build-time resampling of exogenous series (cold path, crates/rscm-core/src/timeseries.rs:586-609).
"""
from __future__ import annotations

import ctypes as C
import enum
import math
from bisect import bisect_left
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from . import graph_plan
from .ensemble import Ensemble, run_lockstep
from .graph_plan import COMPONENT_KINDS, OWN_KERNEL_TYPES, STATELESS_KINDS, SUPPORTED, is_host_component  # noqa: F401

NAN = float("nan")


# ------------------------------------------------------------------------------------ time axis
class TimeAxis:
    """crates/rscm-core/src/timeseries.rs:45-212.  ``bounds`` has ``len()+1`` entries; value ``i``
    is the start of step ``i``."""

    def __init__(self, bounds: np.ndarray):
        b = np.ascontiguousarray(bounds, dtype=np.float64)
        if b.ndim != 1 or not np.all(b[1:] > b[:-1]):
            raise ValueError("time axis must be strictly increasing")  # assert!(is_monotonic)
        self._bounds = b

    @staticmethod
    def from_values(values) -> "TimeAxis":
        v = np.asarray(values, dtype=np.float64)
        if len(v) < 2:
            raise ValueError("from_values needs at least 2 values")
        step = v[-1] - v[-2]
        return TimeAxis(np.concatenate([v, [v[-1] + step]]))

    @staticmethod
    def from_bounds(bounds) -> "TimeAxis":
        b = np.asarray(bounds, dtype=np.float64)
        if len(b) < 2:
            raise ValueError("from_bounds needs at least 2 bounds")
        return TimeAxis(b)

    def values(self) -> np.ndarray:
        return self._bounds[:-1].copy()

    def bounds(self) -> np.ndarray:
        return self._bounds.copy()

    def __len__(self) -> int:
        return len(self._bounds) - 1

    def at(self, index: int) -> Optional[float]:
        return float(self._bounds[index]) if 0 <= index < len(self) else None

    def at_bounds(self, index: int) -> Optional[Tuple[float, float]]:
        if 0 <= index < len(self):
            return float(self._bounds[index]), float(self._bounds[index + 1])
        return None

    def contains(self, value: float) -> bool:
        return bool(np.any(self._bounds[:-1] == value))

    def index_of(self, value: float) -> Optional[int]:
        hit = np.nonzero(np.abs(self._bounds[:-1] - value) < 1e-10)[0]  # timeseries.rs:204-211
        return int(hit[0]) if len(hit) else None


class InterpolationStrategy(enum.Enum):
    Linear = enum.auto()
    Next = enum.auto()
    Previous = enum.auto()


class VariableType(enum.Enum):
    Exogenous = enum.auto()
    Endogenous = enum.auto()


# ------------------------------------------------------------------------------------ interpolation
def _find_segment(target: float, tb: np.ndarray, extrapolate: bool) -> Tuple[str, int]:
    """crates/rscm-core/src/interpolate/strategies/mod.rs:24-81."""
    idx = bisect_left(tb, target)
    fwd = idx == len(tb)
    back = (not fwd) and idx == 0
    if not fwd and math.isclose(tb[idx], target, rel_tol=1e-9, abs_tol=0.0):  # is_close! defaults
        return "OnBoundary", idx
    if (fwd or back) and not extrapolate:
        where = "start of" if back else "end of"
        edge = tb[0] if back else tb[-1]
        raise RuntimeError(f"Extrapolation is not allowed. Target={target} is before the "
                           f"{where} the interpolation range={edge}")
    if back:
        return "ExtrapolateBackward", 0
    if fwd:
        return "ExtrapolateForward", len(tb)
    return "InSegment", idx


def interpolate(strategy: InterpolationStrategy, time: np.ndarray, y: np.ndarray, t: float,
                extrapolate: bool = True) -> float:
    """One query of Interp1d (strategies/linear_spline.rs:33-96, previous.rs:58-80,
    next.rs:56-80).  ``time`` is what the caller hands over: ``interpolate_into`` and ``at_time``
    pass the len(y) time VALUES, so the Linear strategy's "trim the last bound" drops the last
    value and a query there goes through the forward-extrapolation formula."""
    n = len(y)
    if strategy is InterpolationStrategy.Linear:
        kind, idx = _find_segment(t, time[: len(time) - 1], extrapolate)
        idx = min(idx, n - 1)
        if kind == "OnBoundary":
            return float(y[idx])
        if kind == "ExtrapolateBackward":
            t1, y1, t2, y2 = time[0], y[0], time[1], y[1]
        elif kind == "ExtrapolateForward":
            if n < 2:
                raise RuntimeError("linear extrapolation needs two points")
            t1, y1, t2, y2 = time[n - 2], y[n - 2], time[n - 1], y[n - 1]
        else:
            t1, y1, t2, y2 = time[idx - 1], y[idx - 1], time[idx], y[idx]
        m = (y2 - y1) / (t2 - t1)
        return float(m * (t - t1) + y1)
    kind, idx = _find_segment(t, time, extrapolate)
    if strategy is InterpolationStrategy.Previous:
        if kind == "OnBoundary":
            return float(y[idx])
        if kind == "ExtrapolateBackward":
            return float(y[0])
        if kind == "ExtrapolateForward":
            return float(y[n - 1])
        return float(y[idx - 1])
    idx = min(idx, n - 1)  # Next
    if kind in ("OnBoundary", "InSegment"):
        return float(y[idx])
    return float(y[0] if kind == "ExtrapolateBackward" else y[n - 1])


# ------------------------------------------------------------------------------------ timeseries
class Timeseries:
    """Scalar timeseries (python/rscm/_lib/core/__init__.pyi:37-93).  Python-built strategies
    extrapolate (crates/rscm-core/src/python/timeseries.rs:62-74)."""

    def __init__(self, values, time_axis: TimeAxis, units: str,
                 interpolation_strategy: InterpolationStrategy):
        v = np.array(values, dtype=np.float64).reshape(-1)
        if len(v) != len(time_axis):
            raise ValueError(f"values ({len(v)}) and time axis ({len(time_axis)}) differ in length")
        self._values = v
        self._axis = time_axis
        self._units = units
        self._strategy = interpolation_strategy
        self._latest = len(v) - 1 if len(v) and not np.isnan(v[-1]) else self._last_valid(v)

    @staticmethod
    def _last_valid(v: np.ndarray) -> int:
        ok = np.nonzero(~np.isnan(v))[0]
        return int(ok[-1]) if len(ok) else 0

    @staticmethod
    def from_values(values, time) -> "Timeseries":
        axis = time if isinstance(time, TimeAxis) else TimeAxis.from_values(time)
        return Timeseries(values, axis, "", InterpolationStrategy.Linear)

    def with_interpolation_strategy(self, interpolation_strategy) -> "Timeseries":
        self._strategy = interpolation_strategy
        return self

    def __len__(self) -> int:
        return len(self._values)

    def set(self, time_index: int, value: float) -> None:
        self._values[time_index] = value
        self._latest = max(self._latest, time_index)

    def values(self) -> np.ndarray:
        return self._values.copy()

    @property
    def latest(self) -> int:
        return self._latest

    @property
    def units(self) -> str:
        return self._units

    @property
    def time_axis(self) -> TimeAxis:
        return self._axis

    @property
    def interpolation_strategy(self) -> InterpolationStrategy:
        return self._strategy

    def latest_value(self) -> Optional[float]:
        return float(self._values[self._latest]) if len(self._values) else None

    def at(self, time_index: int) -> Optional[float]:
        return float(self._values[time_index]) if 0 <= time_index < len(self) else None

    def at_time(self, time: float) -> float:
        return interpolate(self._strategy, self._axis.values(), self._values, float(time), True)

    def interpolate_into(self, new_axis: TimeAxis) -> "Timeseries":
        """crates/rscm-core/src/timeseries.rs:586-609."""
        tv = self._axis.values()
        out = np.array([interpolate(self._strategy, tv, self._values, float(t), True)
                        for t in new_axis.values()])
        return Timeseries(out, new_axis, self._units, self._strategy)


class FourBoxTimeseries:
    """FourBox grid timeseries: values (n_times, 4) in the order NorthernOcean, NorthernLand,
    SouthernOcean, SouthernLand (python/rscm/_lib/core/__init__.pyi:95-106)."""

    def __init__(self, values, time_axis: TimeAxis, units: str = ""):
        v = np.array(values, dtype=np.float64)
        if v.shape != (len(time_axis), 4):
            raise ValueError(f"FourBox values must be ({len(time_axis)}, 4), got {v.shape}")
        self._values, self._axis, self._units = v, time_axis, units

    def __len__(self) -> int:
        return len(self._values)

    def values(self) -> np.ndarray:
        return self._values.copy()

    @property
    def units(self) -> str:
        return self._units

    @property
    def time_axis(self) -> TimeAxis:
        return self._axis

    @property
    def latest(self) -> int:
        ok = np.nonzero(~np.isnan(self._values[:, 0]))[0]
        return int(ok[-1]) if len(ok) else 0


class GridType(enum.Enum):
    Scalar = enum.auto()
    FourBox = enum.auto()
    Hemispheric = enum.auto()


class TimeseriesCollection:
    """python/rscm/_lib/core/__init__.pyi:119-190; kept sorted by name like the reference's
    ``Vec<TimeseriesItem>`` (crates/rscm-core/src/timeseries_collection.rs:318-321)."""

    def __init__(self) -> None:
        self._items: Dict[str, Tuple[Timeseries, VariableType]] = {}
        self._fourbox: Dict[str, FourBoxTimeseries] = {}

    def add_fourbox_timeseries(self, name: str, timeseries: FourBoxTimeseries) -> None:
        self._fourbox[name] = timeseries

    def get_fourbox_timeseries_by_name(self, name: str) -> Optional[FourBoxTimeseries]:
        return self._fourbox.get(name)

    def add_timeseries(self, name: str, timeseries: Timeseries,
                       variable_type: VariableType = VariableType.Exogenous) -> None:
        if name in self._items:
            raise ValueError(f"timeseries {name!r} already exists")
        self._items[name] = (timeseries, variable_type)

    def get_timeseries_by_name(self, name: str) -> Optional[Timeseries]:
        item = self._items.get(name)
        if item is None:
            return None
        ts = item[0]
        return Timeseries(ts.values(), ts.time_axis, ts.units, ts.interpolation_strategy)

    def variable_type(self, name: str) -> Optional[VariableType]:
        item = self._items.get(name)
        return item[1] if item else None

    def names(self) -> List[str]:
        return sorted(list(self._items) + list(self._fourbox))

    def timeseries(self) -> List[Timeseries]:
        return [self.get_timeseries_by_name(n) for n in sorted(self._items)]

    def __contains__(self, name: str) -> bool:
        return name in self._items


# ------------------------------------------------------------------------------------ schema
class SchemaVariableDefinition:
    """python/rscm/_lib/core/__init__.pyi: one declared variable (name, unit, grid type)."""

    def __init__(self, name: str, unit: str, grid_type: "GridType"):
        self.name, self.unit, self.grid_type = name, unit, grid_type

    def __repr__(self) -> str:
        return f"SchemaVariableDefinition({self.name!r}, {self.unit!r}, {self.grid_type.name})"


class AggregateDefinition:
    """One aggregate of the schema.  Unpacks as ``(unit, operation_type, contributors, weights)``."""

    def __init__(self, name: str, unit: str, operation_type: str, contributors: List[str], weights: Optional[List[float]],
                 grid_type: "GridType"):
        self.name, self.unit, self.operation_type = name, unit, operation_type
        self.contributors, self.weights, self.grid_type = contributors, weights, grid_type

    def __iter__(self):
        return iter((self.unit, self.operation_type, self.contributors, self.weights))

    def __getitem__(self, k):
        return (self.unit, self.operation_type, self.contributors, self.weights)[k]


class VariableSchema:
    """python/rscm/_lib/core/__init__.pyi:322-404; validation as crates/rscm-core/src/schema.rs
    (undefined contributors, unit / grid type / weight-count mismatches, circular aggregates)."""

    def __init__(self) -> None:
        self.variables: Dict[str, SchemaVariableDefinition] = {}
        self.aggregates: Dict[str, AggregateDefinition] = {}

    @property
    def grid_types(self) -> Dict[str, "GridType"]:
        return {n: v.grid_type for n, v in self.variables.items()}

    def add_variable(self, name: str, unit: str, grid_type=None) -> "VariableSchema":
        self.variables[name] = SchemaVariableDefinition(name, unit, grid_type or GridType.Scalar)
        return self

    def add_aggregate(self, name: str, unit: str, operation: str, contributors: Sequence[str],
                      weights: Optional[Sequence[float]] = None, grid_type=None) -> "VariableSchema":
        if operation not in ("Sum", "Mean", "Weighted"):
            raise ValueError(f"Unknown operation {operation!r}: expected 'Sum', 'Mean' or 'Weighted'")
        if operation == "Weighted" and weights is None:
            raise ValueError("weights must be provided for the 'Weighted' operation")
        self.aggregates[name] = AggregateDefinition(name, unit, operation, list(contributors),
                                                    list(weights) if weights is not None else None, grid_type or GridType.Scalar)
        return self

    def contains(self, name: str) -> bool:
        return name in self.variables or name in self.aggregates

    def get_grid_type(self, name: str) -> Optional["GridType"]:
        if name in self.variables:
            return self.variables[name].grid_type
        return self.aggregates[name].grid_type if name in self.aggregates else None

    def validate(self) -> None:
        def norm(u: str) -> str:
            return "".join(str(u).split())
        for name, agg in self.aggregates.items():
            for c in agg.contributors:
                if not self.contains(c):
                    raise ValueError(f"Undefined contributor: aggregate {name!r}: contributor {c!r} is not in the schema")
                unit = self.variables[c].unit if c in self.variables else self.aggregates[c].unit
                if unit and agg.unit and norm(unit) != norm(agg.unit):
                    raise ValueError(f"Unit mismatch: contributor {c!r} has unit {unit!r}, aggregate {name!r} has {agg.unit!r}")
                if self.get_grid_type(c) != agg.grid_type:
                    raise ValueError(f"Grid type mismatch: contributor {c!r} is {self.get_grid_type(c).name}, "
                                     f"aggregate {name!r} is {agg.grid_type.name}")
            if agg.operation_type == "Weighted" and len(agg.weights or []) != len(agg.contributors):
                raise ValueError(f"Weight count mismatch: aggregate {name!r} has {len(agg.contributors)} contributors "
                                 f"and {len(agg.weights or [])} weights")
        state: Dict[str, int] = {}

        def visit(n: str) -> None:
            if state.get(n) == 1:
                raise ValueError(f"Circular dependency among the aggregates at {n!r}")
            if state.get(n) == 2 or n not in self.aggregates:
                return
            state[n] = 1
            for c in self.aggregates[n].contributors:
                visit(c)
            state[n] = 2

        for n in self.aggregates:
            visit(n)


# ------------------------------------------------------------------------------------ components
class Component:
    """A built Rust component as the reference's ``ModelBuilder.with_rust_component`` sees it:
    a type name, parameters, and its requirement definitions in macro order (inputs, outputs,
    states; crates/rscm-macros/src/lib.rs:645-651)."""

    type_name = "Component"
    definitions: List[Tuple[str, str, str]] = []  # (name, unit, "Input"|"Output"|"State")

    def __init__(self, parameters: Dict[str, float]):
        self.parameters = dict(parameters)

    def input_names(self) -> List[str]:
        return [n for n, _, k in self.definitions if k in ("Input", "State")]

    def output_names(self) -> List[str]:
        return [n for n, _, k in self.definitions if k in ("Output", "State")]


class ComponentBuilder:
    component_cls = Component
    required: Tuple[str, ...] = ()

    def __init__(self, parameters: Dict[str, float]):
        self._parameters = dict(parameters)

    @classmethod
    def from_parameters(cls, parameters: Dict[str, float]):
        missing = [k for k in cls.required if k not in parameters]
        if missing:  # pythonize/serde: "missing field `x`" (crates/rscm-core/src/python/component.rs:19-48)
            raise ValueError(f"missing field `{missing[0]}`")
        return cls({k: float(parameters[k]) for k in cls.required})

    def build(self):
        return self.component_cls(self._parameters)


# ------------------------------------------------------------------------------------ builder
TL_PARAM_ORDER = L.TL_PARAM_NAMES
CP_PARAM_ORDER = L.CP_PARAM_NAMES


class ModelBuilder:
    """python/rscm/_lib/core/__init__.pyi:405-463 -> crates/rscm-core/src/model/builder.rs."""

    def __init__(self) -> None:
        self._axis: Optional[TimeAxis] = None
        self._components: List[Component] = []
        self._initial: Dict[str, float] = {}
        self._exogenous = TimeseriesCollection()
        self._schema: Optional[VariableSchema] = None
        self._device = 0
        self._grid_weights: Dict["GridType", List[float]] = {}
        self._mix: Optional[Tuple[str, Dict[str, Timeseries], Dict[str, float]]] = None   # with_forcing_components
        self._noise: Optional[Tuple[float, int]] = None   # with_forcing_noise: (sigma, seed)
        self._noise_phi = 0.0                             # ... and its phi (0: white)
        self._noise_params = False                        # with_forcing_noise_parameters: sigma and phi are parameter rows
        self._diagnostics: List[Tuple[str, Dict[str, Optional[str]], Dict[str, float]]] = []   # with_diagnostic
        self._energy_budgets: List[Tuple[str, str, float]] = []   # with_energy_budget: (quantity, name, scale)
        self._running_means: List[Tuple[str, str, int, str, int]] = []   # with_running_mean: (name, source, window, align, step)

    def with_time_axis(self, time_axis: TimeAxis) -> "ModelBuilder":
        self._axis = time_axis
        return self

    def with_rust_component(self, component: Component) -> "ModelBuilder":
        self._components.append(component)
        return self

    with_component = with_rust_component

    def with_py_component(self, component) -> "ModelBuilder":
        """A component written in Python (``rscm_amd.component.PythonComponent.build(obj)``).  It cannot
        be part of a kernel: its ``solve`` runs on the host between the launches of the graph's linked
        ensembles, once per member and step (``GraphModel``)."""
        from .component import PythonComponent
        if not isinstance(component, PythonComponent):
            raise NotImplementedError("with_py_component takes PythonComponent.build(<rscm_amd.component.Component instance>)")
        self._components.append(component)
        return self

    def with_initial_values(self, initial_values: Dict[str, float]) -> "ModelBuilder":
        self._initial.update({k: float(v) for k, v in initial_values.items()})
        return self

    def with_exogenous_variable(self, name: str, timeseries: Timeseries) -> "ModelBuilder":
        self._exogenous.add_timeseries(name, timeseries, VariableType.Exogenous)
        return self

    def with_forcing_components(self, variable: str, components: Dict[str, Timeseries],
                                scales: Optional[Dict[str, float]] = None) -> "ModelBuilder":
        """Extension: supply the exogenous ``variable`` as a sum of named component series, each scaled PER MEMBER -- what a
        factory closure that scales exogenous series does in the reference's ``ModelRunner``, kept on the device.  For the model
        that is one ``TwoLayer`` reading ``variable`` as its forcing, ``build()`` makes a mix ensemble
        (``Ensemble(..., forcing_components=names)``): member i is forced by ``((S_0 c_0 + S_1 c_1) + ...)``, every product and
        sum rounded on its own, NaN and Inf propagating (an exogenous series formed per member, not the schema's Weighted
        aggregate, which skips NaN contributors).  The coefficients are model parameters named ``"forcing_scale|<name>"``
        after the component's own in ``Model.param_order``; ``scales`` gives their base values (default 1.0)."""
        names = [str(n) for n in components]
        if not 1 <= len(names) <= L.TL_MAX_COMPONENTS:
            raise ValueError(f"with_forcing_components takes 1 to {L.TL_MAX_COMPONENTS} components, got {len(names)}")
        for n, ts in components.items():
            if not isinstance(ts, Timeseries):
                raise TypeError(f"component {n!r} must be a Timeseries")
        unknown = [n for n in (scales or {}) if n not in components]
        if unknown:
            raise ValueError(f"scales given for unknown component(s) {unknown}; components: {names}")
        self._mix = (str(variable), {str(n): ts for n, ts in components.items()},
                     {n: float((scales or {}).get(n, 1.0)) for n in names})
        return self

    def with_diagnostic(self, name: str, weights: Dict[str, Optional[str]], scales: Optional[Dict[str, float]] = None) -> "ModelBuilder":
        """Extension: a diagnostic variable ``name`` of the built model -- per member ``sum_k scale_k p_k x_k`` over the entries
        ``{variable: parameter name or None}`` of ``weights`` in their order, ``x_k`` the variable's row and ``p_k`` the member's
        own value of the parameter (``None``: no parameter, the scale alone; ``scales`` default 1.0).  ``build()`` defines it on
        the model's ensemble, the parameter resolved through ``Model.param_order`` (``"forcing_scale|*"`` and ``"forcing_noise|*"``
        included), or in a graph on the variables' home (``GraphModel.define_diagnostic``).  Its rows are formed on request:
        ``compute_diagnostic`` after ``run()`` (``Ensemble.define_diagnostic``)."""
        if not weights or len(weights) > L.DIAG_MAX_TERMS:
            raise ValueError(f"with_diagnostic takes 1 to {L.DIAG_MAX_TERMS} variables, got {len(weights)}")
        unknown = [v for v in (scales or {}) if v not in weights]
        if unknown:
            raise ValueError(f"scales given for unknown variable(s) {unknown}; variables: {list(weights)}")
        if any(name == n for n, _, _ in self._diagnostics):
            raise ValueError(f"diagnostic {name!r} is defined already")
        self._diagnostics.append((str(name), {str(v): (None if p is None else str(p)) for v, p in weights.items()},
                                  {str(v): float((scales or {}).get(v, 1.0)) for v in weights}))
        return self

    def with_energy_budget(self, quantity: str, name: Optional[str] = None, scale: float = 1.0) -> "ModelBuilder":
        """Extension: a term of the two-layer energy budget as a diagnostic variable of the built model --
        ``"forcing" | "response" | "deep_uptake" | "imbalance"`` (``Ensemble.define_energy_budget``; ``name`` defaults to the
        quantity's own).  ``build()`` defines it on the model's two-layer ensemble, or in a graph on its one two-layer ensemble
        (``GraphModel.define_energy_budget``: with a linked forcing the two forcing-free quantities only)."""
        if quantity not in L.BUDGET_QUANTITIES:
            raise ValueError(f"unknown energy-budget quantity {quantity!r}; one of {sorted(L.BUDGET_QUANTITIES)}")
        name = L.BUDGET_DEFAULT_NAMES[quantity] if name is None else str(name)
        if any(name == n for n, _, _ in self._diagnostics) or any(name == n for _, n, _ in self._energy_budgets):
            raise ValueError(f"diagnostic {name!r} is defined already")
        self._energy_budgets.append((str(quantity), name, float(scale)))
        return self

    def with_running_mean(self, name: str, source: str, window: int = 20, align: str = "centre", step: int = 1) -> "ModelBuilder":
        """Extension: a diagnostic variable ``name`` of the built model, the running mean of ``source`` -- a variable of the model
        or a diagnostic of ``with_diagnostic`` / ``with_energy_budget`` -- over ``window`` rows ``step`` time indices apart
        (``Ensemble.define_running_mean``).  ``build()`` defines it after the other diagnostics, on the model's ensemble or in a
        graph on the source's home (``GraphModel.define_running_mean``)."""
        from .variability import running_mean_back
        running_mean_back(window, align)
        if int(step) < 1:
            raise ValueError(f"step must be at least 1, got {step}")
        taken = [n for n, _, _ in self._diagnostics] + [n for _, n, _ in self._energy_budgets] + [n for n, *_ in self._running_means]
        if name in taken:
            raise ValueError(f"diagnostic {name!r} is defined already")
        self._running_means.append((str(name), str(source), int(window), str(align), int(step)))
        return self

    def _define_diagnostics(self, model):
        """What ``build()`` does with ``with_diagnostic``, ``with_energy_budget`` and ``with_running_mean``: on the ensemble of a
        ``Model`` or the homes of a ``GraphModel``."""
        for quantity, name, scale in self._energy_budgets:
            (model if isinstance(model, GraphModel) else model.ensemble).define_energy_budget(quantity, name, scale)
        for name, weights, scales in self._diagnostics:
            if isinstance(model, GraphModel):
                model.define_diagnostic(name, [(v, p, scales[v]) for v, p in weights.items()])
                continue
            terms = []
            for v, p in weights.items():
                if p is not None and p not in model.param_order:
                    raise ValueError(f"diagnostic {name!r}: {p!r} is no parameter of this model; parameters: {list(model.param_order)}")
                terms.append((v, None if p is None else model.param_order.index(p), scales[v]))
            if any(v not in model.ensemble.var_ids for v, _, _ in terms):
                raise ValueError(f"diagnostic {name!r}: variables {[v for v, _, _ in terms]}; this model has {sorted(model.ensemble.var_ids)}")
            model.ensemble.define_diagnostic(name, terms)
        for name, source, window, align, step in self._running_means:   # last: their sources may be the diagnostics above
            (model if isinstance(model, GraphModel) else model.ensemble).define_running_mean(name, source, window, align, step)
        return model

    def with_forcing_noise(self, sigma: float, seed: int, phi: float = 0.0) -> "ModelBuilder":
        """Extension: internal variability.  Where ``build()`` returns the single two-layer ensemble (one ``TwoLayer`` reading
        its exogenous forcing, with or without ``with_forcing_components``), member i is forced by ``F + sigma * z(seed, i, t)``:
        seeded white noise in the heat flux into the upper layer, a pure function of (seed, member, index on the forcing axis)
        (``Ensemble.set_forcing_noise``).  Any other build -- a graph of linked ensembles, ``series_window``, a likelihood-only
        model -- raises ``ValueError``; so do ``ModelRunner`` and ``DeviceEnsembleSampler`` on such a builder: the likelihood of
        one noise realisation per walker is not a target the stretch move samples.  Run the model, score the stored series
        (``Ensemble.loglik``), weight, resample and branch instead.  ``phi != 0`` (``|phi| < 1``) makes the noise red: AR(1) with
        lag-one correlation ``phi`` per index of the forcing axis and variance ``sigma**2`` at every index."""
        sigma, seed, phi = float(sigma), int(seed), float(phi)
        if not (sigma >= 0.0 and math.isfinite(sigma)):
            raise ValueError(f"with_forcing_noise: sigma must be finite and not negative, got {sigma}")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"with_forcing_noise: seed must fit 64 unsigned bits, got {seed}")
        if not (math.isfinite(phi) and abs(phi) < 1.0):
            raise ValueError(f"with_forcing_noise: phi must be finite with |phi| < 1, got {phi}")
        self._noise = (sigma, seed)
        self._noise_phi = phi
        self._noise_params = False
        return self

    NOISE_PARAM_NAMES = ("forcing_noise|sigma", "forcing_noise|phi")

    def with_forcing_noise_parameters(self, seed: int, sigma: float = 0.0, phi: float = 0.0) -> "ModelBuilder":
        """Extension: internal variability whose amplitude and persistence are PARAMETERS.  As ``with_forcing_noise``, but the
        two-layer ensemble is made with ``noise_params=True`` and ``"forcing_noise|sigma"`` and ``"forcing_noise|phi"`` are
        appended to ``Model.param_order`` and ``base_params`` (after any ``forcing_scale|*``), with ``sigma`` and ``phi`` as their
        base values: every member is forced with its own ``sigma_i`` and ``phi_i`` (``Ensemble.set_forcing_noise_members``), so
        ``sample_lhs`` bounds, ``set_params`` and the posterior take the two like any parameter.  The base values are validated
        as ``with_forcing_noise`` validates its own; values set later are data (``Ensemble.set_forcing_noise_members``).  The
        refusals of ``with_forcing_noise`` apply unchanged, ``ModelRunner`` and ``DeviceEnsembleSampler`` included."""
        self.with_forcing_noise(sigma, seed, phi)
        self._noise_params = True
        return self

    def _with_noise_params(self, param_order, base_params):
        """``param_order`` and ``base_params`` with the two noise parameters appended where ``with_forcing_noise_parameters`` asked."""
        if not self._noise_params:
            return tuple(param_order), np.array(base_params, dtype=np.float64)
        return (tuple(param_order) + self.NOISE_PARAM_NAMES,
                np.append(np.array(base_params, dtype=np.float64), [self._noise[0], self._noise_phi]))

    def _set_noise(self, ens: Ensemble) -> None:
        if self._noise is None:
            return
        if self._noise_params:
            ens.set_forcing_noise_members(self._noise[1])
        else:
            ens.set_forcing_noise(*self._noise, phi=self._noise_phi)

    def forcing_noise_plan(self, store_series: bool = True, series_window=None) -> Optional[Dict[str, object]]:
        """What ``build()`` makes of ``with_forcing_noise*`` (None without it), formed on the host: ``per_member``, ``seed`` and the
        ``param_order`` and ``base_params`` of the model.  Raises ``ValueError`` where ``build()`` would."""
        if self._noise is None:
            return None
        self._check_forcing_noise(store_series, series_window)
        mix = self.forcing_mix_plan()
        if mix is not None:
            order, base = mix["param_order"], mix["base_params"]
        else:
            order, base = self._with_noise_params(TL_PARAM_ORDER, [self._components[0].parameters[k] for k in TL_PARAM_ORDER])
        return {"per_member": self._noise_params, "seed": self._noise[1], "param_order": order, "base_params": base}

    def _check_forcing_noise(self, store_series: bool, series_window) -> None:
        """Raises ``ValueError`` unless ``build()`` with these arguments yields the single two-layer (or mix) ensemble with
        stored series, the one shape forcing noise is an option of.  Needs no device."""
        why = None
        types = [c.type_name for c in self._components]
        if series_window is not None:
            why = "series_window builds a graph of windowed ensembles"
        elif any(is_host_component(c) for c in self._components) or types != ["TwoLayer"]:
            why = f"this model (components {types}) builds a GraphModel or another kind"
        elif self._mix is None and self._resolve()[3]:
            why = "a schema aggregate in front of the TwoLayer builds a GraphModel"
        elif not store_series:
            why = "a likelihood-only model (store_series=False) keeps no series to add the noise's effect to"
        if why:
            raise ValueError(f"with_forcing_noise: {why}; forcing noise is an option of the single two-layer ensemble "
                             "(one TwoLayer reading its exogenous forcing, whole series stored)")

    def forcing_mix_plan(self) -> Optional[Dict[str, object]]:
        """What ``build()`` makes of ``with_forcing_components`` (None without it), formed on the host: ``names``, the
        ``param_order`` and ``base_params`` of the model and the ``[K][T]`` component block on the model's axis.  Raises
        ``ValueError`` for a model shape the mix ensemble does not cover."""
        if self._mix is None:
            return None
        variable, components, scales = self._mix
        endogenous, sources, exo_names, aggregates = self._resolve()
        types = [c.type_name for c in self._components]
        erf = "Effective Radiative Forcing"
        hint = ("per-member forcing components are available for the model that is one TwoLayer reading the variable as its "
                "exogenous forcing; for any other graph put a Weighted aggregate (VariableSchema.add_aggregate) in front of the consumer")
        if any(is_host_component(c) for c in self._components) or types != ["TwoLayer"] or aggregates:
            raise ValueError(f"with_forcing_components: this model has components {types}"
                             f"{' and schema aggregates' if aggregates else ''}; {hint}")
        if variable != erf or variable not in exo_names:
            raise ValueError(f"with_forcing_components: {variable!r} is not the exogenous forcing the TwoLayer reads ({erf!r}); {hint}")
        if variable in self._exogenous:
            raise ValueError(f"with_forcing_components: {variable!r} is also supplied with with_exogenous_variable; give one of the two")
        rows = []
        for name, ts in components.items():
            self._check_units(variable, ts.units)
            rows.append(ts.interpolate_into(self._axis).values())
        names = tuple(components)
        base = [self._components[0].parameters[k] for k in TL_PARAM_ORDER] + [scales[n] for n in names]
        order, base = self._with_noise_params(TL_PARAM_ORDER + tuple(f"forcing_scale|{n}" for n in names), base)
        return {"names": names, "param_order": order, "base_params": base, "block": np.stack(rows)}

    def _build_mix(self, n_members: int, store_series: bool) -> "Model":
        plan = self.forcing_mix_plan()
        endogenous, sources, _, _ = self._resolve()
        ens = Ensemble(L.KIND_TWO_LAYER, n_members, self._axis.bounds(), device=self._device, store_series=store_series,
                       forcing_components=plan["names"], noise_params=self._noise_params)
        ens.set_step_size(L.COMP_TWO_LAYER, 0.1)
        ens.set_params(np.repeat(plan["base_params"][:, None], n_members, axis=1))
        ens.set_forcing(plan["block"][None], None, L.SRC_EXOGENOUS)
        for name, vid in ens.var_ids.items():
            if vid > 0 and name in self._initial:
                ens.set_initial(vid, self._initial[name])
        self._set_noise(ens)
        model = Model(ens, self._axis, sources, endogenous, plan["block"], dict(self._initial), plan["param_order"], plan["base_params"])
        model._builder = self
        return self._define_diagnostics(model)

    def with_exogenous_collection(self, collection: TimeseriesCollection) -> "ModelBuilder":
        for name in collection.names():
            self._exogenous.add_timeseries(name, collection.get_timeseries_by_name(name),
                                           VariableType.Exogenous)
        return self

    def with_schema(self, schema: VariableSchema) -> "ModelBuilder":
        self._schema = schema
        return self

    def with_grid_weights(self, grid_type: "GridType", weights: Sequence[float]) -> "ModelBuilder":
        """builder.rs:56-103: area weights used wherever a FourBox variable is aggregated to a scalar
        (default 0.25 each, FourBoxGrid::magicc_standard)."""
        w = [float(x) for x in weights]
        if grid_type != GridType.FourBox:
            raise NotImplementedError("only FourBox weights are used on the device path")
        if len(w) != 4:
            raise ValueError(f"Weights length {len(w)} does not match FourBox grid size 4")
        if abs(sum(w) - 1.0) >= 1e-6:
            raise ValueError(f"Weights must sum to 1.0, got {sum(w)}")
        self._grid_weights[grid_type] = w
        return self

    def with_device(self, device: int) -> "ModelBuilder":
        """Extension: which GPU the model lives on."""
        self._device = device
        return self

    # -- graph resolution (builder.rs:448-560) ----------------------------------------------
    def _resolve(self):
        if self._axis is None:
            raise ValueError("no time axis")
        endogenous: Dict[str, str] = {}
        sources: Dict[Tuple[str, str], str] = {}
        exo_names: List[str] = []
        kinds: Dict[str, str] = {}
        aggregates = self._schema.aggregates if self._schema else {}
        if self._schema:
            self._schema.validate()
        for comp, node_name in zip(self._components, self._node_names()):
            for name, _, kind in comp.definitions:
                if kind not in ("Input", "State"):
                    continue
                if kind == "State":
                    src = "OwnState"
                elif name in endogenous or name in aggregates:
                    src = "UpstreamOutput"
                else:
                    src = "Exogenous"
                sources[(name, comp.type_name)] = src
                sources[(name, node_name)] = src  # "<type>#k" for all but the last component of a type
                kinds.setdefault(name, kind)
                if name not in endogenous and name not in aggregates and name not in exo_names:
                    exo_names.append(name)
            for name, _, kind in comp.definitions:
                if kind in ("Output", "State"):
                    if kind == "State" or name not in kinds:
                        kinds[name] = kind
                    endogenous[name] = comp.type_name
        for name in aggregates:
            endogenous[name] = f"Aggregator:{name}"
            kinds[name] = "Output"
        for name, kind in kinds.items():  # builder.rs:704-717
            if kind == "State" and name not in self._initial:
                raise ValueError(f"Missing initial value for state variable '{name}' "
                                 f"(component {endogenous.get(name, 'unknown')})")
        return endogenous, sources, exo_names, aggregates

    def _exogenous_on_axis(self, name: str, exo_names: List[str]) -> Optional[np.ndarray]:
        if name in exo_names and name in self._exogenous:
            ts = self._exogenous.get_timeseries_by_name(name)
            self._check_units(name, ts.units)
            return ts.interpolate_into(self._axis).values()
        return None

    def _check_units(self, name: str, supplied: str) -> None:
        """The reference converts between compatible units when a series, the schema and a component
        disagree (builder.rs:141-338).  There is no units registry on this path -- every factor is
        1.0 -- so a disagreement that is more than spelling is refused instead of computed wrongly."""
        def norm(u: str) -> str:
            return "".join(str(u).split()).replace("**", "^")
        wanted = {norm(u) for c in self._components for n, u, k in c.definitions if n == name and k in ("Input", "State") and u}
        if self._schema and name in self._schema.variables and self._schema.variables[name].unit:
            wanted.add(norm(self._schema.variables[name].unit))
        if supplied and wanted and norm(supplied) not in wanted:
            raise NotImplementedError(f"unit conversion is not available on the GPU path: {name!r} is supplied in "
                                      f"{supplied!r}, expected {sorted(wanted)}")

    def _node_names(self) -> List[str]:
        """One graph-node name per component: its type name, except that all but the LAST registered
        component of a type are "<type>#<k>" (``graph_plan.component_nodes``, which says why; which of them
        gets an ensemble is decided by ``graph_plan.survivors``)."""
        return [node.name for node in graph_plan.component_nodes(self._components)]

    def _graph_order(self, aggregates, topological: bool = False) -> List[str]:
        """Execution order of the reference: nodes in registration order (root, components,
        aggregates), edges as ModelBuilder::build adds them, petgraph Bfs from the root (neighbours
        come out most-recently-added edge first).  builder.rs:448-701, runtime.rs:504-527.

        ``topological`` (an extension) orders the same nodes so that every edge points forwards:
        the order in which no component reads a value of the current step before it has been
        produced.  Every such order gives the same values; among the nodes that are ready the next
        one is of the class of the previous one if possible -- components that share a fused
        launch (csrc/lockstep.cpp) against those with a kernel of their own (ClimateUDEB,
        OceanCarbon, HalocarbonChemistry, host components) -- so that a step takes as few launches
        as the edges allow; within a class the breadth-first position decides."""
        names = ["<root>"]
        edges: Dict[int, List[int]] = {}
        endogenous: Dict[str, int] = {}
        pending: List[Tuple[int, str]] = []
        node_names = self._node_names()

        def add_edge(a: int, b: int) -> None:
            edges.setdefault(a, []).append(b)

        for comp, node_name in zip(self._components, node_names):
            node = len(names)
            names.append(node_name)
            has_dep = False
            for name, _, kind in comp.definitions:
                if kind not in ("Input", "State"):
                    continue
                if name in endogenous:
                    add_edge(endogenous[name], node)
                    has_dep = True
                elif name in aggregates:
                    pending.append((node, name))
                    has_dep = True
            if not has_dep:
                add_edge(0, node)
            for name, _, kind in comp.definitions:
                if kind in ("Output", "State"):
                    if name in endogenous:
                        add_edge(endogenous[name], node)
                    endogenous[name] = node
        for agg, (_, _, contributors, _) in aggregates.items():
            node = len(names)
            names.append(f"Aggregator:{agg}")
            has_dep = False
            for c in contributors:
                if c in endogenous:
                    add_edge(endogenous[c], node)
                    has_dep = True
            if not has_dep:
                add_edge(0, node)
            endogenous[agg] = node
        for node, name in pending:
            if name in endogenous:
                add_edge(endogenous[name], node)
        seen, order, queue = {0}, [], [0]
        while queue:
            n = queue.pop(0)
            if n:
                order.append(names[n])
            for m in reversed(edges.get(n, [])):
                if m not in seen:
                    seen.add(m)
                    queue.append(m)
        if not topological:
            return order
        rank = {name: k for k, name in enumerate(order)}
        for name in names[1:]:
            rank.setdefault(name, len(rank))
        indeg = {n: 0 for n in range(1, len(names))}
        for a, targets in edges.items():
            for b in set(targets):
                if a:
                    indeg[b] += 1
        own_kernel = {0: False}
        for k, comp in enumerate(self._components, start=1):
            own_kernel[k] = comp.type_name in OWN_KERNEL_TYPES or is_host_component(comp)
        ready = sorted((n for n, d in indeg.items() if d == 0), key=lambda n: rank[names[n]])
        topo: List[str] = []
        last = False
        while ready:
            ready.sort(key=lambda k: (own_kernel.get(k, False) != last, rank[names[k]]))
            n = ready.pop(0)
            last = own_kernel.get(n, False)
            topo.append(names[n])
            for m in set(edges.get(n, [])):
                indeg[m] -= 1
                if indeg[m] == 0:
                    ready.append(m)
        if len(topo) != len(names) - 1:
            raise ValueError("the component graph has a cycle")
        return topo

    def _fourbox_weights(self) -> List[float]:
        return self._grid_weights.get(GridType.FourBox, [0.25, 0.25, 0.25, 0.25])

    def _stored_as_scalar(self, name: str) -> bool:
        return self._schema is not None and self._schema.grid_types.get(name) == GridType.Scalar

    def _plan_graph(self, endogenous, sources, exo_names, aggregates, execution_order: str = "reference",
                    series_window: Optional[int] = None, output_stride: int = 0,
                    outputs: Optional[Sequence[str]] = None) -> graph_plan.GraphPlan:
        """Every decision about a graph of linked ensembles, and every refusal, on the host (``rscm_amd/graph_plan.py``)."""
        return graph_plan.plan_graph(self, endogenous, sources, exo_names, aggregates, execution_order, series_window, output_stride, outputs)

    def _realise(self, plan: graph_plan.GraphPlan, n_members: int) -> "GraphModel":
        """The stream and the ensembles of ``plan``, the library calls in the order the plan lists them."""
        bounds = self._axis.bounds()
        stream = C.c_void_p()
        L.check(L.load().rscm_gpu_stream_create(self._device, C.byref(stream)))
        model = GraphModel(self._axis, list(plan.order), {}, dict(plan.var_home), [], dict(plan.exogenous), plan.sources, stream,
                           self._device, plan.feed_forward)
        model._builder = self
        model._execution_order = plan.execution_order
        model._windowed, model._output_stride = plan.windowed, plan.output_stride
        model._reads_unwritten = plan.reads_unwritten
        model._fourbox, model._fourbox_aggregates = dict(plan.fourbox), dict(plan.fourbox_aggregates)
        model.param_home, model.base_params = dict(plan.param_home), dict(plan.base_params)
        for name, host in plan.hosts.items():
            node = model._host_nodes[name] = _HostNode(host.comp)
            node.sources, node.device_reads = dict(host.sources), dict(host.device_reads)
            node.series = {v: np.repeat(s[:, None], n_members, axis=1) for v, s in host.series.items()}

        def link(spec: graph_plan.LinkSpec) -> None:
            ens = model.ensembles[spec.consumer]
            ens.link_input(spec.row, model.ensembles[spec.producer], spec.var, spec.source)
            model._links.append((spec.consumer, spec.row))
            if spec.before_producer:
                L.check(L.load().rscm_ens_set_link_order_check(ens._h, 0))

        try:
            for spec in plan.nodes:
                ens = Ensemble(spec.kind, n_members, bounds, device=self._device, window_rows=spec.window_rows,
                               output_stride=spec.output_stride, output_vars=spec.output_vars)
                model.ensembles[spec.key] = ens
                ens.set_stream(stream.value)
                ens.set_params(np.repeat(np.array(spec.params, dtype=np.float64)[:, None], n_members, axis=1))
                if spec.step_size is not None:
                    ens.set_step_size(*spec.step_size)
                for made_with_it in spec.links:
                    link(made_with_it)
            for consumer in plan.consumers:
                for spec in consumer.links:
                    link(spec)
                if consumer.table is not None:
                    model.ensembles[consumer.key].set_forcing(consumer.table)
            for key, vid, value in plan.initial:
                model.ensembles[key].set_initial(vid, value)
        except Exception:
            model.close()
            raise
        return model

    def build(self, n_members: int = 1, store_series: bool = True, execution_order: str = "reference",
              series_window: Optional[int] = None, output_stride: int = 0,
              outputs: Optional[Sequence[str]] = None) -> "Model":
        """``execution_order`` (graphs without a fused kernel only): "reference" steps the components
        in the reference's breadth-first order, which can run a component before the producer of a
        value it reads at the end of the step (it then reads NaN, which an aggregate skips);
        "topological" is the order in which that cannot happen.

        ``series_window`` (an extension, for long axes and large ensembles): run the model as a graph of
        linked ensembles that keep only a sliding window of that many rows of every series -- what a
        step and its consumers read -- plus every ``output_stride``-th row of ``outputs`` (variable
        names; None: every variable).  The reference holds whole collections, one member at a time
        (model/builder.rs:735-830); 1e5 members x 9001 monthly points x 36 series do not fit a GPU that
        way.  ``get_series(name, t_stride=output_stride)`` reads the kept rows."""
        if self._noise is not None:
            self._check_forcing_noise(store_series, series_window)
        endogenous, sources, exo_names, aggregates = self._resolve()
        if self._mix is not None:
            if series_window is not None:
                raise ValueError("with_forcing_components: a mix ensemble has no windowed storage (series_window)")
            return self._build_mix(n_members, store_series)
        hosted = any(is_host_component(c) for c in self._components)
        if series_window is not None and hosted:
            raise NotImplementedError("Python components read whole host series: no series_window for such graphs")
        fused = None if series_window is not None or hosted else self._fused_shape(sources, exo_names, aggregates)
        if fused is None:
            # any other graph: one ensemble per component, linked on the device (output_stride and outputs belong to series_window)
            window = (series_window, output_stride, outputs) if series_window is not None else (None, 0, None)
            plan = self._plan_graph(endogenous, sources, exo_names, aggregates, execution_order, *window)
            return self._define_diagnostics(self._realise(plan, n_members))
        kind, forcing, params, step_sizes = fused
        if not store_series and kind != L.KIND_TWO_LAYER:
            store_series = True  # likelihood-only handles exist for the two-layer kind
        noise_params = self._noise is not None and self._noise_params   # (_check_forcing_noise: this is the two-layer ensemble)
        if noise_params:
            _, params = self._with_noise_params((), params)
        ens = Ensemble(kind, n_members, self._axis.bounds(), device=self._device,
                       store_series=store_series, noise_params=noise_params)
        for comp_id, step in step_sizes.items():
            ens.set_step_size(comp_id, step)
        ens.set_params(np.repeat(np.array(params, dtype=np.float64)[:, None], n_members, axis=1))
        ens.set_forcing(forcing, None, L.SRC_EXOGENOUS)
        self._set_noise(ens)
        for name, vid in ens.var_ids.items():
            if vid > 0 and name in self._initial:
                ens.set_initial(vid, self._initial[name])
            elif vid > 0 and "|" in name and name.split("|")[0] in self._initial and kind == L.KIND_UDEB:
                # a FourBox state initialised with one scalar sets all four regions (builder.rs:797-804)
                ens.set_initial(vid, self._initial[name.split("|")[0]])
        param_order = tuple(L.PARAM_NAMES[kind]) + (self.NOISE_PARAM_NAMES if noise_params else ())
        model = Model(ens, self._axis, sources, endogenous, forcing, dict(self._initial), param_order,
                      np.array(params, dtype=np.float64))
        model._builder = self
        return self._define_diagnostics(model)

    def _exogenous_or_nan(self, name: str, exo_names: List[str]) -> np.ndarray:
        """The exogenous series on the axis; never supplied: a NaN series (builder.rs:772-780), and run() then yields NaN."""
        vals = self._exogenous_on_axis(name, exo_names)
        return np.full(len(self._axis), NAN) if vals is None else vals

    def _fused_shape(self, sources, exo_names, aggregates):
        """``(kind, forcing, parameters, step sizes)`` of the single ensemble where the model is one of the four shapes a fused
        kernel covers; None for any other graph."""
        types = [c.type_name for c in self._components]
        erf = "Effective Radiative Forcing"
        if types == ["TwoLayer"] and not aggregates:
            params = [self._components[0].parameters[k] for k in TL_PARAM_ORDER]
            return L.KIND_TWO_LAYER, self._exogenous_or_nan(erf, exo_names), params, {L.COMP_TWO_LAYER: 0.1}
        if (types == ["CarbonCycle", "CO2ERF", "TwoLayer"] and list(aggregates) == [erf]
                and aggregates[erf][1] == "Sum"
                and aggregates[erf][2] == ["Effective Radiative Forcing|CO2"]
                # the fused coupled kernel carries ONE conc_pi row; two different pre-industrial
                # concentrations run as the same graph of linked ensembles (one launch as well: all light)
                and self._components[0].parameters["conc_pi"] == self._components[1].parameters["conc_pi"]):
            cc, ce, tl = self._components
            assert sources[("Surface Temperature", "CarbonCycle")] == "Exogenous"
            assert sources[(erf, "TwoLayer")] == "UpstreamOutput"
            params = ([tl.parameters[k] for k in TL_PARAM_ORDER] +
                      [cc.parameters["tau"], cc.parameters["conc_pi"],
                       cc.parameters["alpha_temperature"], ce.parameters["erf_2xco2"]])
            return (L.KIND_COUPLED, self._exogenous_or_nan("Emissions|CO2|Anthropogenic", exo_names), params,
                    {L.COMP_TWO_LAYER: 0.1, L.COMP_CARBON_CYCLE: cc.step_size})
        if types == ["ClimateUDEB"] and not aggregates:
            return L.KIND_UDEB, self._exogenous_or_nan(erf, exo_names), self._components[0].param_vector(), {}
        if len(types) == 1 and types[0] in STATELESS_KINDS and not aggregates:
            kind = STATELESS_KINDS[types[0]]
            forcing = np.stack([self._exogenous_or_nan(name, exo_names) for name in L.KIND_TABLE[kind][2]])
            return kind, forcing, self._components[0].param_vector(), {}
        return None


def save_checkpoint(path, ck: Dict[str, object]) -> None:
    """A checkpoint (of an ``Ensemble`` or a ``GraphModel``) as one ``.npz`` of plain arrays: nested
    keys joined with ``/``; nothing is pickled, so loading executes nothing from the file."""
    flat: Dict[str, np.ndarray] = {}

    def walk(prefix: str, value) -> None:
        if isinstance(value, dict):
            flat[prefix + "/__dict__"] = np.array(len(value))
            for k, v in value.items():
                if "/" in str(k):
                    raise ValueError(f"key {k!r} contains '/'")
                walk(f"{prefix}/{k}", v)
        elif value is None:
            flat[prefix + "/__none__"] = np.array(0)
        elif isinstance(value, (list, tuple)) and all(isinstance(x, str) for x in value):
            flat[prefix + "/__strings__"] = np.array(list(value), dtype=np.str_)
        else:
            flat[prefix] = np.asarray(value)

    walk("", ck)
    np.savez(path, **{k.lstrip("/").replace("|", "__BAR__"): v for k, v in flat.items()})


def load_checkpoint(path) -> Dict[str, object]:
    out: Dict[str, object] = {}
    with np.load(path, allow_pickle=False) as z:
        for raw in z.files:
            parts = raw.replace("__BAR__", "|").split("/")
            node = out
            leaf = parts[-1]
            if leaf in ("__dict__", "__none__", "__strings__"):
                parts, marker = parts[:-1], leaf
            else:
                marker = None
            for p_ in parts[:-1]:
                node = node.setdefault(p_, {})
            if not parts:
                continue
            if marker == "__dict__":
                node.setdefault(parts[-1], {})
            elif marker == "__none__":
                node[parts[-1]] = None
            elif marker == "__strings__":
                node[parts[-1]] = [str(x) for x in z[raw]]
            else:
                v = z[raw]
                node[parts[-1]] = v.item() if v.ndim == 0 else v
    return out


_component_param_names = graph_plan.component_param_names
_component_params = graph_plan.component_params


class _HostNode:
    """A Python component inside a GraphModel: the series it reads (host copies, refreshed row by
    row from the device), where those come from, and the source classification of each."""

    def __init__(self, comp):
        self.comp = comp
        self.series: Dict[str, np.ndarray] = {}
        self.device_reads: Dict[str, Tuple[str, int]] = {}
        self.sources: Dict[str, str] = {}


class GraphModel:
    """A component graph the fused kernels do not cover, run as one ensemble per component (and per
    schema aggregate) whose inputs are linked on the device (``rscm_ens_link_input``) and which are
    stepped in the reference's order: petgraph BFS from the root over the edges
    ``ModelBuilder::build`` adds (builder.rs:487-560, runtime.rs:368-497).  Same surface as ``Model``.

    ``ensembles`` maps a component's type name (``"Aggregator:<name>"`` for aggregates) to its
    ``Ensemble``, e.g. to give the members different parameters before ``run()``."""

    def __init__(self, axis: TimeAxis, order: List[str], ensembles: Dict[str, Ensemble], var_home, links,
                 exogenous: Dict[str, np.ndarray], sources, stream, device: int, feed_forward: bool):
        self._axis = axis
        self._order = order
        self.ensembles = ensembles
        self._var_home = var_home          # variable name -> (owner, variable id)
        self._diagnostics: Dict[str, Tuple[str, int]] = {}   # diagnostic name -> (owner, id): define_diagnostic
        self._links = links                # (consumer, row) pairs, for teardown
        self._exogenous = exogenous
        self._sources = sources
        self._stream = stream
        self._device = device
        self._feed_forward = feed_forward
        self._host_nodes: Dict[str, "_HostNode"] = {}  # Python components, stepped on the host
        self._reads_unwritten = False  # some component reads index n+1 of a producer that runs after it
        self._fourbox: Dict[str, Tuple[str, int, bool]] = {}  # FourBox variable -> (producer, first id, stored as scalar)
        self._fourbox_aggregates: Dict[str, List[Tuple[str, int]]] = {}  # FourBox aggregate -> (ensemble, id) of each region
        self._windowed = False      # ensembles keep a sliding window of rows + strided outputs (build(series_window=...))
        self._output_stride = 1
        self.time_index = 0
        # component parameters: "Type.name" -> (owner, row); bare names too where they are unique
        self.param_home: Dict[str, Tuple[str, int]] = {}
        self.base_params: Dict[str, np.ndarray] = {}

    @property
    def n_members(self) -> int:
        return next(iter(self.ensembles.values())).n_members

    def set_mode(self, mode: int) -> None:
        """Arithmetic mode of every ensemble of the graph (``MODE_FAST``: fused multiply-adds in
        the two-layer RK4 and the OceanCarbon convolution; the other kinds compute the same either way)."""
        for ens in self.ensembles.values():
            ens.set_mode(mode)

    def rewind(self) -> None:
        """Back to a fresh model.  Where a component runs ahead of a producer it reads at n+1, the
        rows of the previous run must not be found there: they are cleared to NaN."""
        for ens in self.ensembles.values():
            if self._reads_unwritten:
                ens.clear_series()
            else:
                ens.rewind()
        self.time_index = 0

    _builder: Optional["ModelBuilder"] = None
    _execution_order = "reference"

    def to_toml(self) -> str:
        from . import serialise
        return serialise.dumps(serialise.describe(self._builder, self))

    from_toml = staticmethod(lambda text: Model.from_toml(text))

    def as_dot(self) -> str:
        from . import serialise
        return serialise.as_dot(self._builder)

    def debug_info(self, format: str = "plain") -> str:
        """Execution order, variable flow and source classification (Model::debug_info)."""
        from . import serialise
        return serialise.debug_info(self._builder, self, format)

    def checkpoint(self) -> Dict[str, object]:
        """Everything needed to continue from the current step in another model object built from
        the same builder: per ensemble the current row of every stored variable (linked consumers
        read outputs as well as states), the rows the chemistry looks back at, the internal
        component states (runtime.rs:270-282)."""
        if self._host_nodes:
            raise NotImplementedError("checkpoints of graphs with Python components are not available")
        for ens in self.ensembles.values():
            ens.sync()
        return {"time_index": self.time_index, "order": list(self._order),
                "ensembles": {name: ens.checkpoint(all_variables=True) for name, ens in self.ensembles.items()}}

    def restore(self, ck: Dict[str, object]) -> None:
        if ck["order"] != list(self._order) or set(ck["ensembles"]) != set(self.ensembles):
            raise ValueError("checkpoint does not match this graph")
        # In the reference's execution order a component can read index n+1 of a producer that runs
        # after it and must find NaN there, as in the collection the checkpoint was taken from: rows
        # this (already advanced) model wrote beyond the checkpoint must not survive the roll-back.
        for name, ens in self.ensembles.items():
            ens.restore(ck["ensembles"][name], clear_later_rows=self._reads_unwritten)
        self.time_index = int(ck["time_index"])

    def variable_home(self, name: str) -> Tuple[Ensemble, int]:
        """The ensemble and variable id that hold the scalar series of ``name``."""
        if name in self._diagnostics:
            owner, vid = self._diagnostics[name]
            return self.ensembles[owner], vid
        if name not in self._var_home:
            raise KeyError(f"Model output missing variable: {name}")
        owner, vid = self._var_home[name]
        return self.ensembles[owner], vid

    def define_diagnostic(self, name: str, terms) -> int:
        """``Ensemble.define_diagnostic`` on the home ensemble the terms' variables share: ``terms`` is a sequence of
        ``(variable name, parameter or None[, scale])``, the parameter a row of that ensemble or a name of ``param_home``
        (``"Type.name"``, or the bare name where it is unique) that lives there.  ``variable_home(name)`` then resolves the
        diagnostic, so ``quantile_rows``, ``indicators``, ``variability``, ``spectrum``, ``covariability``, ``cross_spectrum``, ``set_baseline`` and ``get_series`` take it
        by name.  Variables of two ensembles: ``ValueError`` (a diagnostic does not cross handles)."""
        if name in self._diagnostics or name in self._var_home:
            raise ValueError(f"variable name {name!r} is taken")
        terms = [tuple(t) for t in terms]
        if not terms:
            raise ValueError("a diagnostic needs at least one term")
        for t in terms:
            if t[0] in self._diagnostics:
                raise ValueError(f"term {t!r}: a diagnostic combines stored variables, not diagnostics")
            if t[0] not in self._var_home:
                raise KeyError(f"Model output missing variable: {t[0]}")
        homes = [self._var_home[t[0]] for t in terms]
        owners = sorted({o for o, _ in homes})
        if len(owners) != 1:
            raise ValueError(f"diagnostic {name!r}: its variables live in the ensembles {owners}; all terms must share one home")
        resolved = []
        for t, (_, vid) in zip(terms, homes):
            row = t[1]
            if isinstance(row, str):
                if row not in self.param_home or self.param_home[row][0] != owners[0]:
                    raise ValueError(f"diagnostic {name!r}: parameter {row!r} is no parameter of {owners[0]!r}, the variables' home")
                row = self.param_home[row][1]
            resolved.append((vid, row) + tuple(t[2:3]))
        vid = self.ensembles[owners[0]].define_diagnostic(name, resolved)
        self._diagnostics[name] = (owners[0], vid)
        return vid

    def define_energy_budget(self, quantity: str, name: Optional[str] = None, scale: float = 1.0) -> int:
        """``Ensemble.define_energy_budget`` on the graph's one two-layer ensemble (``ValueError`` for none or for several).  Where
        that ensemble's forcing is linked -- it usually is in a graph -- only ``"response"`` and ``"deep_uptake"`` are
        available: the library refuses ``"forcing"`` and ``"imbalance"`` there."""
        if quantity not in L.BUDGET_QUANTITIES:
            raise ValueError(f"unknown energy-budget quantity {quantity!r}; one of {sorted(L.BUDGET_QUANTITIES)}")
        name = L.BUDGET_DEFAULT_NAMES[quantity] if name is None else name
        if name in self._diagnostics or name in self._var_home:
            raise ValueError(f"variable name {name!r} is taken")
        owners = [o for o, ens in self.ensembles.items() if ens.kind == L.KIND_TWO_LAYER]
        if len(owners) != 1:
            raise ValueError(f"define_energy_budget needs exactly one two-layer ensemble in the graph, found {len(owners)}: {owners}")
        vid = self.ensembles[owners[0]].define_energy_budget(quantity, name, scale)
        self._diagnostics[name] = (owners[0], vid)
        return vid

    def define_running_mean(self, name: str, source: str, window: int = 20, align: str = "centre", step: int = 1) -> int:
        """``Ensemble.define_running_mean`` on the home ensemble of ``source``, a variable of the graph or a diagnostic defined on
        it before.  ``variable_home(name)`` then resolves it like any diagnostic."""
        if name in self._diagnostics or name in self._var_home:
            raise ValueError(f"variable name {name!r} is taken")
        ens, src = self.variable_home(source)
        owner = next(o for o, e in self.ensembles.items() if e is ens)
        vid = ens.define_running_mean(name, src, window, align, step)
        self._diagnostics[name] = (owner, vid)
        return vid

    def compute_diagnostic(self, name: str, t_begin: Optional[int] = None, t_end: Optional[int] = None, t_stride: int = 1) -> None:
        """``Ensemble.compute_diagnostic`` of ``name`` on its home ensemble (``t_begin=None``: row 0, ``t_end=None``: up to and
        including the model's current step; for a running mean the first and one past the last row with a full window at or
        below it)."""
        if name not in self._diagnostics:
            raise KeyError(f"no diagnostic named {name!r}")
        for ens in self.ensembles.values():
            ens.sync()
        ens, vid = self.variable_home(name)
        if ens.diagnostics_running_mean(vid) is not None:
            lo, hi = ens.running_mean_range(vid, time_index=self.time_index)
            t_begin, t_end = (lo if t_begin is None else t_begin), (hi if t_end is None else t_end)
        ens.compute_diagnostic(vid, 0 if t_begin is None else t_begin, self.time_index + 1 if t_end is None else t_end, t_stride)

    def get_series(self, name: str, **kw) -> np.ndarray:
        ens, vid = self.variable_home(name)
        return ens.get_series(vid, **kw)

    def quantile_rows(self, name: str, q, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1,
                      weighted: bool = False, anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """Ensemble quantiles of ``name`` (``numpy.nanquantile``, linear) over the rows ``t_begin, t_begin + t_stride, ...
        < t_end``, reduced on the device wherever the rows are resident (a windowed graph's window or output store included):
        ``Ensemble.quantile_rows`` of the variable's home.  ``weighted``: with the member weights (``set_member_weights`` /
        ``set_weights_from_loglik``), ``method="inverted_cdf"``; the result then has ``"weight"`` in place of ``"count"``.
        ``anomaly``: of each member's anomaly against the baseline ``set_baseline`` gave the variable's home.  ``grouped``: per
        member group (``set_member_groups``), group-major as ``Ensemble.quantile_rows`` returns it."""
        ens, vid = self.variable_home(name)
        kw = {"grouped": True} if grouped else {}
        return ens.quantile_rows(vid, q, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly, **kw)

    def set_baseline(self, name: str, t_begin: int, t_end: int, t_stride: int = 1) -> None:
        """Each member's mean of ``name`` over the rows ``t_begin, t_begin + t_stride, ... < t_end`` as the baseline of the
        variable's home ensemble (``Ensemble.set_baseline``; one baseline per ensemble, so variables sharing a home share it)."""
        ens, vid = self.variable_home(name)
        ens.set_baseline(vid, t_begin, t_end, t_stride)

    def set_baseline_values(self, name: str, b) -> None:
        self.variable_home(name)[0].set_baseline_values(b)

    def baseline(self, name: str) -> np.ndarray:
        return self.variable_home(name)[0].baseline()

    def clear_baseline(self, name: str) -> None:
        self.variable_home(name)[0].clear_baseline()

    def indicators(self, name: str, t_begin: int, t_end: int, t_stride: int = 1, thresholds=(), anomaly: bool = False,
                   slot: int = 0) -> Dict[str, object]:
        """``Ensemble.indicators`` of ``name`` on its home ensemble: device vectors ``mean``, ``peak``, ``peak_time``,
        ``crossing``, which ``quantile_vectors`` and ``exceedance`` read."""
        ens, vid = self.variable_home(name)
        return ens.indicators(vid, t_begin, t_end, t_stride, thresholds, anomaly, slot)

    def variability(self, name: str, t_begin: int, t_end: int, t_stride: int = 1, detrend: str = "linear", slot: int = 0) -> Dict[str, object]:
        """``Ensemble.variability`` of ``name`` on its home ensemble: device vectors ``mean``, ``slope``, ``variance``, ``sd``,
        ``r1``, which ``quantile_vectors``, ``exceedance`` and ``Ensemble.loglik_vectors`` read."""
        ens, vid = self.variable_home(name)
        return ens.variability(vid, t_begin, t_end, t_stride, detrend, slot)

    def covariability(self, name_x: str, name_y: str, t_begin: int, t_end: int, t_stride: int = 1, detrend_x: str = "linear",
                      detrend_y: str = "linear", lags: int = 0, slot: int = 0) -> Dict[str, object]:
        """``Ensemble.covariability`` of ``name_x`` and ``name_y`` on the home ensemble the two share: device vectors ``var_x``,
        ``var_y``, ``cov``, ``corr``, ``slope`` and the lists ``lead`` and ``lag``.  Variables of two ensembles: ``ValueError`` (the
        statistic does not cross handles)."""
        (ens_x, vid_x), (ens_y, vid_y) = self.variable_home(name_x), self.variable_home(name_y)
        if ens_x is not ens_y:
            raise ValueError(f"covariability: {name_x!r} and {name_y!r} live in different ensembles; both variables must share one home")
        return ens_x.covariability(vid_x, vid_y, t_begin, t_end, t_stride, detrend_x, detrend_y, lags, slot)

    def cross_spectrum(self, name_x: str, name_y: str, t_begin: int, t_end: int, t_stride: int = 1, detrend_x: str = "linear",
                       detrend_y: str = "linear", bands=3, slot: int = 0) -> Dict[str, object]:
        """``Ensemble.cross_spectrum`` of ``name_x`` and ``name_y`` on the home ensemble the two share: device vectors ``var_x``,
        ``var_y`` and per band ``coherence2``, ``gain``, ``gain_quad``, with the bands' ``edges`` and ``counts``.  Variables of two
        ensembles: ``ValueError`` (the statistic does not cross handles)."""
        (ens_x, vid_x), (ens_y, vid_y) = self.variable_home(name_x), self.variable_home(name_y)
        if ens_x is not ens_y:
            raise ValueError(f"cross_spectrum: {name_x!r} and {name_y!r} live in different ensembles; both variables must share one home")
        return ens_x.cross_spectrum(vid_x, vid_y, t_begin, t_end, t_stride, detrend_x, detrend_y, bands, slot)

    def spectrum(self, name: str, t_begin: int, t_end: int, t_stride: int = 1, detrend: str = "difference", bands=8,
                 slot: int = 0) -> Dict[str, object]:
        """``Ensemble.spectrum`` of ``name`` on its home ensemble: device vectors ``mean``, ``slope``, ``variance`` and the band
        powers ``power``, with the bands' ``edges`` and ``counts``; ``Ensemble.loglik_spectrum`` and ``quantile_vectors`` read them."""
        ens, vid = self.variable_home(name)
        return ens.spectrum(vid, t_begin, t_end, t_stride, detrend, bands, slot)

    def quantile_vectors(self, vectors, q, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``Ensemble.quantile_vectors`` on the ensemble that owns the vectors (every ensemble of the graph shares the member
        index and, after ``set_member_weights`` / ``set_weights_from_loglik`` / ``set_member_groups``, the weights and groups)."""
        vs = list(vectors)
        kw = {"grouped": True} if grouped else {}
        return vs[0].owner.quantile_vectors(vs, q, weighted=weighted, **kw)

    def moments(self, vectors, weighted: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``Ensemble.moments`` (exact weighted means, covariances and correlations across members) on the ensemble that owns the
        vectors; the vectors of several ensembles of the graph go together, as for ``quantile_vectors``."""
        vs = list(vectors)
        kw = {"grouped": True} if grouped else {}
        return vs[0].owner.moments(vs, weighted=weighted, **kw)

    def moment_rows(self, name: str, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, vectors=(), weighted: bool = False,
                    anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``Ensemble.moment_rows`` (the exact weighted mean and spread of ``name`` at every row, and its covariance with per-member
        vectors) on the variable's home ensemble.  The vectors must belong to that ensemble: ``ValueError`` otherwise (the rows are
        read where they live, and the statistic does not cross handles)."""
        ens, vid = self.variable_home(name)
        vs = list(vectors)
        for v in vs:
            if getattr(v, "owner", None) is not ens:
                raise ValueError(f"moment_rows: a vector does not belong to the home ensemble of {name!r}; take it from that ensemble")
        kw = {"grouped": True} if grouped else {}
        return ens.moment_rows(vid, t_begin, t_end, t_stride, vs, weighted=weighted, anomaly=anomaly, **kw)

    def exceedance_rows(self, name: str, thresholds, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                        anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``Ensemble.exceedance_rows`` (the exceedance of ``[K]`` or ``[rows][K]`` thresholds at every row of ``name``) on the
        variable's home ensemble."""
        ens, vid = self.variable_home(name)
        kw = {"grouped": True} if grouped else {}
        return ens.exceedance_rows(vid, thresholds, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly, **kw)

    def histogram_rows(self, name: str, edges, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                       anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``Ensemble.histogram_rows`` (the members in each bin between ``edges`` at every row of ``name``) on the variable's home
        ensemble."""
        ens, vid = self.variable_home(name)
        kw = {"grouped": True} if grouped else {}
        return ens.histogram_rows(vid, edges, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly, **kw)

    def rank_rows(self, name: str, record, t_begin: int = 0, t_end: Optional[int] = None, t_stride: int = 1, weighted: bool = False,
                  anomaly: bool = False, grouped: bool = False) -> Dict[str, np.ndarray]:
        """``Ensemble.rank_rows`` (where the record ``[rows]`` lies inside the plume of ``name`` at every row) on the variable's
        home ensemble."""
        ens, vid = self.variable_home(name)
        kw = {"grouped": True} if grouped else {}
        return ens.rank_rows(vid, record, t_begin, t_end, t_stride, weighted=weighted, anomaly=anomaly, **kw)

    def exceedance(self, vector, thresholds, weighted: bool = False, grouped: bool = False) -> Dict[str, object]:
        """``Ensemble.exceedance`` on the ensemble that owns the vector."""
        kw = {"grouped": True} if grouped else {}
        return vector.owner.exceedance(vector, thresholds, weighted=weighted, **kw)

    def set_member_groups(self, groups, n_groups: Optional[int] = None) -> None:
        """Member groups (``[N]`` int32, -1 or ``0 <= id < n_groups``) for the ``grouped=True`` statistics, set on every device
        ensemble of the graph: they all share the member index.  ``branch`` leaves a destination's groups alone."""
        for ens in self.ensembles.values():
            ens.set_member_groups(groups, n_groups)

    def clear_member_groups(self) -> None:
        for ens in self.ensembles.values():
            ens.clear_member_groups()

    def set_member_weights(self, w) -> None:
        """Integer member weights (``[N]`` int64 >= 0) for ``quantile_rows(..., weighted=True)``, set on every ensemble of the
        graph: they all share the member index."""
        for ens in self.ensembles.values():
            ens.set_member_weights(w)

    def set_weights_from_loglik(self, ll, bits: Optional[int] = None, ll_max: Optional[float] = None):
        """Member weights from a per-member log-likelihood ``ll`` (``[N]``, computed by the caller) on every ensemble of the
        graph, as ``Ensemble.set_weights_from_loglik``.  A member that failed in any ensemble of the graph gets weight 0
        everywhere, so that every variable's plume reads one member set.  Returns the ``(ll_max, bits)`` used."""
        from .ensemble import DeviceVector, default_weight_bits
        x = ll.to_host() if isinstance(ll, DeviceVector) else np.array(ll, dtype=np.float64)
        if x.shape != (self.n_members,):
            raise ValueError(f"log-likelihood: need {self.n_members} values, got shape {x.shape}")
        for ens in self.ensembles.values():
            x[ens.status() != 0] = -np.inf
        if ll_max is None:
            fin = x[np.isfinite(x)]
            ll_max = float(fin.max()) if fin.size else -np.inf
        if bits is None:
            bits = default_weight_bits(self.n_members)
        for ens in self.ensembles.values():
            ens.set_weights_from_loglik(x, bits, ll_max)
        return float(ll_max), int(bits)

    def resample(self, n_draws: int, seed: int = 0, offset: Optional[int] = None):
        """``Ensemble.resample`` with the member weights ``set_member_weights`` / ``set_weights_from_loglik`` put on every
        ensemble of the graph (they all share the member index): the ancestors as an int64 device vector."""
        return next(iter(self.ensembles.values())).resample(n_draws, seed, offset)

    def branch(self, dst_model: "GraphModel", ancestors, dst_offset: int = 0) -> None:
        """``Ensemble.branch`` handle by handle: the same ancestors applied to every ensemble of the graph, so that member ``j``
        of ``dst_model`` (built from the same builder, any member count, full or windowed storage) continues member
        ``ancestors[j]`` of this model from the current step.  ``dst_model`` keeps its own exogenous series."""
        if self._host_nodes or dst_model._host_nodes:
            raise NotImplementedError("branching graphs with Python components is not available")
        if list(dst_model._order) != list(self._order) or set(dst_model.ensembles) != set(self.ensembles):
            raise ValueError("the destination is not a model of this graph")
        for ens in self.ensembles.values():
            ens.sync()
        for name, ens in self.ensembles.items():
            ens.branch(dst_model.ensembles[name], ancestors, dst_offset)
        dst_model.time_index = self.time_index

    def set_member_params(self, names: Sequence[str], values) -> None:
        """``values[N][len(names)]``: per-member values of the named component parameters; every
        other parameter keeps the value its component was built with."""
        v = np.asarray(values, dtype=np.float64)
        if v.ndim != 2 or v.shape != (self.n_members, len(names)):
            raise ValueError(f"Expected {len(names)} parameters for {self.n_members} members, got {v.shape}")
        per_owner: Dict[str, np.ndarray] = {}
        for k, name in enumerate(names):
            owner, row = self.param_home[name]
            if owner not in per_owner:
                per_owner[owner] = np.repeat(self.base_params[owner][:, None], self.n_members, axis=1)
            per_owner[owner][row] = v[:, k]
        for owner, full in per_owner.items():
            self.ensembles[owner].set_params(full)

    def variable_sources(self) -> Dict[Tuple[str, str], str]:
        return dict(self._sources)

    def current_time(self) -> float:
        return self._axis.at(self.time_index)

    def current_time_bounds(self) -> Tuple[float, float]:
        return self._axis.at_bounds(self.time_index)

    def _sync(self) -> None:
        next(iter(self.ensembles.values())).sync()  # one stream for all

    def _host_step(self, name: str, n: int) -> None:
        """One step of a Python component: the rows it may read come back from the device, ``solve`` runs
        per member, the new rows go into the component's storage series on the device."""
        node = self._host_nodes[name]
        T = len(self._axis)
        for var, (owner, vid) in node.device_reads.items():
            hi = min(n + 2, T)
            node.series[var][n:hi] = self.ensembles[owner].get_series(vid, n, hi)
        t0, t1 = self._axis.at_bounds(n)
        outs = {v: np.full(self.n_members, NAN) for v in node.comp.output_names()}
        for m in range(self.n_members):
            for var, value in node.comp.solve_member(t0, t1, node.series, m, n, node.sources).items():
                if var not in outs:
                    raise KeyError(f"{name}.solve returned {var!r}, which it does not declare as an output")
                outs[var][m] = value
        for var, row in outs.items():
            store = self.ensembles[f"{name}:{var}"]
            store.set_state(1, n + 1, row)
            store.set_time_index(n + 1)

    def step(self) -> None:
        if not self.time_index < len(self._axis) - 1:
            raise RuntimeError("assertion failed: self.time_index < self.time_axis.len() - 1")
        if self._host_nodes:
            for name in self._order:
                if name in self._host_nodes:
                    self._host_step(name, self.time_index)
                else:
                    self.ensembles[name].run(self.time_index + 1, sync=False)
        else:  # one native call: consecutive light components share a launch (rscm_ens_run_lockstep)
            run_lockstep([self.ensembles[name] for name in self._order], self.time_index + 1, sync=False)
        self.time_index += 1
        self._sync()

    def run(self) -> None:
        last = len(self._axis) - 1
        if self._host_nodes:  # Python components: the host takes part in every step
            while self.time_index < last:
                self.step()
            return
        if self._feed_forward and not self._windowed:  # no edge points backwards: every producer can finish before its consumers start
            for name in self._order:
                self.ensembles[name].run(last, sync=False)
        else:
            run_lockstep([self.ensembles[name] for name in self._order], last, sync=False)
        self.time_index = last
        self._sync()

    def finished(self) -> bool:
        return self.time_index == len(self._axis) - 1

    def timeseries(self, member: int = 0) -> TimeseriesCollection:
        if self._windowed:
            raise NotImplementedError("a windowed model keeps every output_stride-th row only: read them with "
                                      "get_series(name, t_stride=output_stride)")
        coll = TimeseriesCollection()
        for name, vals in self._exogenous.items():
            coll.add_timeseries(name, Timeseries(vals, self._axis, "", InterpolationStrategy.Linear), VariableType.Exogenous)
        skip = set()
        for name, (owner, first, stored_scalar) in self._fourbox.items():
            if stored_scalar:
                continue  # the collection holds the aggregated scalar (write transform)
            ens = self.ensembles[owner]
            boxes = np.stack([ens.get_series(v, m_begin=member, m_end=member + 1)[:, 0] for v in range(first, first + 4)], axis=1)
            coll.add_fourbox_timeseries(name, FourBoxTimeseries(boxes, self._axis, "K" if ens.kind == L.KIND_UDEB else "W/m^2"))
            skip.add(name)
        for name, homes in self._fourbox_aggregates.items():
            boxes = np.stack([self.ensembles[o].get_series(v, m_begin=member, m_end=member + 1)[:, 0] for o, v in homes], axis=1)
            coll.add_fourbox_timeseries(name, FourBoxTimeseries(boxes, self._axis, ""))
            skip.add(name)
        for name, (owner, vid) in self._var_home.items():
            if name in skip or "#partial" in name or "|box" in name:  # partial sums and the per-region series of FourBox variables are internal
                continue
            vals = self.ensembles[owner].get_series(vid, m_begin=member, m_end=member + 1)[:, 0]
            coll.add_timeseries(name, Timeseries(vals, self._axis, "", InterpolationStrategy.Linear), VariableType.Endogenous)
        return coll

    def close(self) -> None:
        for consumer, row in self._links:
            if self.ensembles[consumer]._h:
                self.ensembles[consumer].unlink_input(row)
        self._links = []
        for ens in self.ensembles.values():
            ens.close()
        if self._stream is not None:
            L.check(L.load().rscm_gpu_stream_destroy(self._device, self._stream))
            self._stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """python/rscm/_lib/core/__init__.pyi:563-628 over one device-resident ensemble.  With
    ``n_members == 1`` it behaves like the reference's ``Model``; with more it is the batch the
    calibration front drives (all members share the graph, axis, forcing and initial values and
    differ in parameters)."""

    def __init__(self, ens: Ensemble, axis: TimeAxis, sources, endogenous, forcing, initial,
                 param_order, base_params):
        self.ensemble = ens
        self._axis = axis
        self._sources = sources
        self._endogenous = endogenous
        self._forcing = forcing
        self._initial = initial
        self.param_order = tuple(param_order)
        self.base_params = base_params

    _builder: Optional["ModelBuilder"] = None

    @property
    def n_members(self) -> int:
        return self.ensemble.n_members

    @property
    def time_index(self) -> int:
        return self.ensemble.time_index

    def checkpoint(self) -> Dict[str, object]:
        return self.ensemble.checkpoint()

    def restore(self, ck: Dict[str, object]) -> None:
        self.ensemble.restore(ck)

    def to_toml(self) -> str:
        """Model::to_toml (runtime.rs:270-300): description + state as TOML text (rscm_amd/serialise.py)."""
        from . import serialise
        return serialise.dumps(serialise.describe(self._builder, self))

    @staticmethod
    def from_toml(text: str):
        """Model::from_toml: the model a ``to_toml`` text describes, at the step it was taken at."""
        from . import serialise
        return serialise.rebuild(serialise.loads(text))

    def as_dot(self) -> str:
        from . import serialise
        return serialise.as_dot(self._builder)

    def debug_info(self, format: str = "plain") -> str:
        """Execution order, variable flow and source classification (Model::debug_info)."""
        from . import serialise
        return serialise.debug_info(self._builder, self, format)

    def variable_sources(self) -> Dict[Tuple[str, str], str]:
        return dict(self._sources)

    def current_time(self) -> float:
        return self._axis.at(self.ensemble.time_index)

    def current_time_bounds(self) -> Tuple[float, float]:
        return self._axis.at_bounds(self.ensemble.time_index)

    def step(self) -> None:
        if not self.ensemble.time_index < len(self._axis) - 1:
            raise RuntimeError("assertion failed: self.time_index < self.time_axis.len() - 1")
        self.ensemble.step()

    def run(self) -> None:
        self.ensemble.run()

    def finished(self) -> bool:
        return self.ensemble.finished()

    def timeseries(self, member: int = 0) -> TimeseriesCollection:
        coll = TimeseriesCollection()
        input_name = [n for n, v in self.ensemble.var_ids.items() if v == 0][0]
        fourbox = L.FOURBOX_VARS.get(self.ensemble.kind)
        fb_ids = ()
        if fourbox:  # a FourBox variable is stored as four scalar series
            fb_ids = tuple(range(fourbox[1], fourbox[1] + 4))
            boxes = np.stack([self.ensemble.get_series(v, m_begin=member, m_end=member + 1)[:, 0]
                              for v in fb_ids], axis=1)
            unit = "K" if self.ensemble.kind == L.KIND_UDEB else "W/m^2"
            coll.add_fourbox_timeseries(fourbox[0], FourBoxTimeseries(boxes, self._axis, unit))
        for name, vid in self.ensemble.var_ids.items():
            if vid in fb_ids or vid >= self.ensemble.n_vars:   # (a diagnostic is no series of the collection: its rows are computed on request)
                continue
            if vid == 0 and self.ensemble.input_rows:
                for k, input_row in enumerate(self.ensemble.input_rows):  # the input block's series
                    coll.add_timeseries(input_row, Timeseries(self._forcing[k], self._axis, "",
                                                              InterpolationStrategy.Linear), VariableType.Exogenous)
                continue
            if vid == 0:
                vals, vt = self._forcing, VariableType.Exogenous
            else:
                vals = self.ensemble.get_series(vid, m_begin=member, m_end=member + 1)[:, 0]
                vt = VariableType.Endogenous
            coll.add_timeseries(name, Timeseries(vals, self._axis, "", InterpolationStrategy.Linear), vt)
        del input_name
        return coll

    def close(self) -> None:
        self.ensemble.close()
