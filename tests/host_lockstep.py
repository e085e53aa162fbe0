"""Host side of the lock-step scheduler tests (csrc/lockstep.cpp, csrc/group.hip): a typed catalogue of the
component kinds, a seeded generator of linked graphs, a restatement of the launch plan rscm_ens_run_lockstep
makes for a call, plan_split's tie relation, and a closed-loop reference that recomputes every handle's
series from what it read of its producers with the CPU oracles (oracle/cbind.py).  Pure numpy + oracles:
the device side lives in tests/test_gpu_lockstep_graphs.py."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from rscm_amd import _lib as L

# ------------------------------------------------------------------------------------------------ constants of the scheduler
MAX_GROUP_OPS = 16      # kMaxGroupOps: a fused segment has at most this many ops
GROUP_TABLE_OPS = 12    # kGroupTableOps: op lists up to this length travel by value; also the limit of a merged launch
N_MODES = 7             # rscm_gpu_set_lockstep_fusion(0..6)
CACHE_SLOT_BUDGET = 20  # kCacheSlotBudget: LDS slots of a multi-step launch
# the member counts of the fuzz: the split kernel takes 64 members per workgroup, the others 256
MEMBER_COUNTS = (1, 63, 64, 65, 203, 257)

# ------------------------------------------------------------------------------------------------ value classes
# Exogenous series per value class (yrs = 0, 1, ...): what an unlinked input row of that class reads, and the
# values that keep every formula in its domain.
EXO = {
    "co2_emis": lambda y: 2.0 + 0.1 * y,
    "co2_conc": lambda y: 280.0 + 1.0 * y,
    "ch4_conc": lambda y: 722.0 + 5.0 * y,
    "n2o_conc": lambda y: 270.0 + 0.5 * y,
    "ch4_emis": lambda y: 200.0 + 2.0 * y,
    "n2o_emis": lambda y: 7.0 + 0.05 * y,
    "nox": lambda y: 10.0 + 0.2 * y,
    "co": lambda y: 300.0 + 2.0 * y,
    "nmvoc": lambda y: 60.0 + 0.5 * y,
    "sox": lambda y: 2.0 + 0.1 * y,
    "bc": lambda y: 2.5 + 0.02 * y,
    "oc": lambda y: 10.0 + 0.1 * y,
    "eesc": lambda y: 1400.0 + 3.0 * y,
    "temp": lambda y: 0.01 * y,
    "dic": lambda y: 0.2 * y,
    "erf": lambda y: 4.0 * (1.0 - np.exp(-(y + 1.0) / 60.0)),
    "cflux": lambda y: 1.5 + 0.02 * y,
    "heat": lambda y: 0.5 + 0.01 * y,
    "cstock": lambda y: 1000.0 + 1.0 * y,
}
# classes an aggregate may combine (Sum / Weighted of concentrations or temperatures would leave the domain of what reads them)
AGG_CLASSES = ("erf", "temp", "co2_conc", "cflux", "heat", "cstock")
MEAN_ONLY = ("temp", "co2_conc")
OPS = {"Sum": 0.0, "Mean": 1.0, "Weighted": 2.0}

HALO_EMIS = {"CFC-11": lambda y: 50.0 + 8.0 * y, "CFC-12": lambda y: 80.0 + 10.0 * y, "Halon-1211": lambda y: 0.2 * y}


@dataclass(frozen=True)
class KindInfo:
    name: str
    inputs: Tuple[str, ...]        # value class per input row (None: exogenous only, e.g. the halocarbon emissions)
    outputs: Dict[int, str]        # stored variable id -> value class
    init: Dict[int, float]         # row 0 of every stored variable
    light: bool                    # the kind's `fusable` in csrc/kinds.hpp (GhgForcing: only with linked inputs)
    perturb: Tuple[int, ...] = ()  # parameter rows drawn per member (x U(0.9, 1.1))
    tol: float = 1e-12             # relative tolerance of the closed-loop check (those of the single-component GPU tests)


def _fourbox(cls, first=1):
    return {first + k: cls for k in range(4)}


CATALOGUE = {
    L.KIND_TWO_LAYER: KindInfo("TwoLayer", ("erf",), {1: "temp", 2: "temp"}, {1: 0.0, 2: 0.0}, True, tol=1e-9),
    L.KIND_CARBON_CYCLE: KindInfo("CarbonCycle", ("co2_emis", "temp"), {1: "co2_conc", 2: "cstock", 3: "cstock"},
                                  {1: 278.0, 2: 0.0, 3: 0.0}, True, tol=1e-9),
    L.KIND_CO2_ERF: KindInfo("CO2ERF", ("co2_conc",), {1: "erf"}, {1: 0.0}, True, (0,)),
    L.KIND_AGGREGATE: KindInfo("Aggregate", (), {1: None}, {1: 0.0}, True),
    L.KIND_OZONE_FORCING: KindInfo("OzoneForcing", ("eesc", "ch4_conc", "nox", "co", "nmvoc", "temp"), {1: "erf", 2: "erf", 3: "erf"},
                                   {1: 0.0, 2: 0.0, 3: 0.0}, True, (1, 3)),
    L.KIND_AEROSOL_DIRECT: KindInfo("AerosolDirect", ("sox", "bc", "oc", "nox"), _fourbox("erf"), {k: 0.0 for k in range(1, 5)}, True, (0, 1)),
    L.KIND_AEROSOL_INDIRECT: KindInfo("AerosolIndirect", ("sox", "oc"), {1: "erf"}, {1: 0.0}, True, (0, 1)),
    L.KIND_CH4_CHEMISTRY: KindInfo("CH4Chemistry", ("ch4_emis", "temp", "nox", "co", "nmvoc"), {1: "ch4_conc", 2: "lifetime"},
                                   {1: 722.0, 2: 9.0}, True, (1, 2)),
    L.KIND_N2O_CHEMISTRY: KindInfo("N2OChemistry", ("n2o_emis",), {1: "n2o_conc", 2: "lifetime"}, {1: 270.0, 2: 120.0}, True, (1, 2)),
    L.KIND_CO2_BUDGET: KindInfo("CO2Budget", ("co2_emis", "co2_emis", "cflux", "cflux"), {1: "co2_conc", 2: "co2_net", 3: "fraction"},
                                {1: 278.0, 2: 0.0, 3: 0.0}, True, (0,)),
    L.KIND_TERRESTRIAL_CARBON: KindInfo("TerrestrialCarbon", ("co2_conc", "temp", "co2_emis"), {**_fourbox("cstock"), 5: "cflux"},
                                        {1: 884.86, 2: 92.77, 3: 1681.53, 4: 836.0, 5: 0.0}, True, (0, 2)),
    L.KIND_FOURBOX_OHU: KindInfo("FourBoxOHU", ("erf",), _fourbox("heat"), {k: 0.0 for k in range(1, 5)}, True, (0,)),
    L.KIND_OSPP: KindInfo("OSPP", ("temp", "dic"), {1: "pco2"}, {1: 278.0}, True, (1,)),
    L.KIND_GHG_FORCING: KindInfo("GhgForcing", ("co2_conc", "ch4_conc", "n2o_conc"), {1: "erf", 2: "erf", 3: "erf"},
                                 {1: 0.0, 2: 0.0, 3: 0.0}, True, (4, 5)),
    L.KIND_OCEAN_CARBON: KindInfo("OceanCarbon", ("co2_conc", "temp"), {1: "pco2", 2: "cstock", 3: "cflux"}, {1: 278.0, 2: 0.0, 3: 0.0},
                                  False, (5,), tol=1e-9),
    L.KIND_HALOCARBON: KindInfo("HalocarbonChemistry", (None,) * 41, {**{k: "halo_conc" for k in range(1, 42)}, 42: "erf", 43: "erf",
                                                                       44: "erf", 45: "eesc"},
                                {**{k: 0.0 for k in range(1, 46)}, 2: 5.0}, False),
    L.KIND_UDEB: KindInfo("ClimateUDEB", ("erf",), {**_fourbox("temp"), 5: "heat", 6: "ohc", 7: "temp"}, {k: 0.0 for k in range(1, 8)},
                          False, (3, 10), tol=1e-9),
}
LIGHT_KINDS = tuple(k for k, v in CATALOGUE.items() if v.light)
# group_kind_is_small (csrc/group.hip): a launch of these only may keep LDS slots
SMALL_KINDS = (L.KIND_TWO_LAYER, L.KIND_AEROSOL_INDIRECT, L.KIND_FOURBOX_OHU, L.KIND_OSPP, L.KIND_CO2_ERF, L.KIND_AGGREGATE,
               L.KIND_CO2_BUDGET, L.KIND_CARBON_CYCLE)
# group_seq_available: SeqCoupled and SeqForced have a kernel of their own (group_seq_kernel)
OWN_SEQUENCES = ((L.KIND_CARBON_CYCLE, L.KIND_CO2_ERF, L.KIND_AGGREGATE, L.KIND_TWO_LAYER), (L.KIND_AGGREGATE, L.KIND_TWO_LAYER))
HEAVY_KINDS = (L.KIND_GHG_FORCING, L.KIND_HALOCARBON, L.KIND_OCEAN_CARBON, L.KIND_UDEB)   # (GhgForcing on its table path)
# plan_split's op_cost, for nothing but choosing hand-built graphs the cut accepts
OP_COST = {L.KIND_TWO_LAYER: 12, L.KIND_CH4_CHEMISTRY: 6, L.KIND_N2O_CHEMISTRY: 5, L.KIND_CARBON_CYCLE: 4, L.KIND_GHG_FORCING: 4,
           L.KIND_TERRESTRIAL_CARBON: 4, L.KIND_OZONE_FORCING: 2, L.KIND_AEROSOL_DIRECT: 2}


def default_params(kind: int, n: int, rng: Optional[np.random.Generator], ghg_method: float = 1.0, op: float = 0.0) -> np.ndarray:
    """[P][n]: the oracle's defaults, with the catalogue's rows perturbed per member when rng is given."""
    from oracle import cbind as orc
    if kind in (L.KIND_OZONE_FORCING, L.KIND_AEROSOL_DIRECT, L.KIND_AEROSOL_INDIRECT, L.KIND_FOURBOX_OHU, L.KIND_OSPP):
        p = orc.pointwise_default_params(kind)
    elif kind in (L.KIND_CH4_CHEMISTRY, L.KIND_N2O_CHEMISTRY):
        p = orc.chem_default_params(kind)
    elif kind in (L.KIND_CO2_BUDGET, L.KIND_TERRESTRIAL_CARBON):
        p = orc.carbon_default_params(kind)
    elif kind == L.KIND_GHG_FORCING:
        p = orc.ghg_default_params(method=ghg_method)
    elif kind == L.KIND_OCEAN_CARBON:
        p = orc.ocean_default_params("3D-GFDL")
    elif kind == L.KIND_HALOCARBON:
        p = orc.halo_default_params()
    elif kind == L.KIND_UDEB:
        p = orc.udeb_default_params()
    elif kind == L.KIND_TWO_LAYER:
        p = np.array([1.2, 0.05, 1.4, 0.7, 8.0, 100.0])
    elif kind == L.KIND_CARBON_CYCLE:
        p = np.array([25.0, 278.0, 0.05])
    elif kind == L.KIND_CO2_ERF:
        p = np.array([3.71, 278.0])
    elif kind == L.KIND_AGGREGATE:
        p = np.concatenate([[op], np.linspace(0.4, 1.1, 8)])
    else:
        raise KeyError(kind)
    P = np.repeat(np.asarray(p, dtype=np.float64).reshape(-1, 1), n, axis=1)
    if rng is not None:
        rows = CATALOGUE[kind].perturb
        if kind == L.KIND_TWO_LAYER:
            rows = tuple(range(6))
        elif kind == L.KIND_CARBON_CYCLE:
            rows = (0, 2)
        elif kind == L.KIND_AGGREGATE:
            rows = tuple(range(1, 9))
        for j in rows:
            P[j] = P[j] * rng.uniform(0.9, 1.1, n)
    return P


# ------------------------------------------------------------------------------------------------ graphs
@dataclass
class Link:
    src: int        # position of the producer in the execution order
    var: int        # its stored variable
    upstream: bool  # SRC_UPSTREAM (row n + 1) rather than SRC_EXOGENOUS (row n)


@dataclass
class Node:
    kind: int
    params: np.ndarray                                   # [P][N]
    links: Dict[int, Link] = field(default_factory=dict)  # input row -> link; every other used row is exogenous
    n_rows: int = 0                                      # input rows in use (aggregates: contributors; the rest stay NaN)
    agg_class: Optional[str] = None                      # the aggregate's value class

    @property
    def info(self) -> KindInfo:
        return CATALOGUE[self.kind]

    def row_class(self, row: int) -> Optional[str]:
        return self.agg_class if self.kind == L.KIND_AGGREGATE else self.info.inputs[row]

    def out_class(self, var: int) -> Optional[str]:
        return self.agg_class if self.kind == L.KIND_AGGREGATE else self.info.outputs[var]

    @property
    def init(self) -> Dict[int, float]:
        """Row 0 of every stored variable (an aggregate starts from its class's exogenous value)."""
        return {1: float(EXO[self.agg_class](0.0))} if self.kind == L.KIND_AGGREGATE else dict(self.info.init)

    @property
    def light(self) -> bool:
        """can_fuse() of csrc/ens.hpp."""
        return self.info.light and (self.kind != L.KIND_GHG_FORCING or len(self.links) > 0)

    @property
    def keep_rows(self) -> int:
        """rscm_ens::keep_rows(): the look-back of the chemistry plus one, at least two."""
        lookback = 0
        if self.kind == L.KIND_CH4_CHEMISTRY:
            lookback = 1
        elif self.kind == L.KIND_N2O_CHEMISTRY:
            lookback = int(min(max(1.0, float(self.params[4].max())), 1e6)) + 1
        return max(lookback + 1, 2)

    def reads_end(self, row: int) -> bool:
        """Whether input row `row` reads the end of the step (row n + 1) -- aggregates always."""
        return self.kind == L.KIND_AGGREGATE or self.links[row].upstream


@dataclass
class Graph:
    nodes: List[Node]
    T: int      # time points; the steps are [0, T - 1)
    N: int

    @property
    def steps(self) -> int:
        return self.T - 1


def exogenous_block(node: Node, T: int) -> np.ndarray:
    """[n_inputs][T] of what the node's table holds: the class's series on every unlinked row in use, NaN elsewhere."""
    y = np.arange(T, dtype=np.float64)
    n_in = 41 if node.kind == L.KIND_HALOCARBON else (8 if node.kind == L.KIND_AGGREGATE else len(node.info.inputs))
    out = np.full((n_in, T), np.nan)
    if node.kind == L.KIND_HALOCARBON:
        out[:] = 0.0
        for s, f in HALO_EMIS.items():
            out[L.HC_SPECIES.index(s)] = f(y)
        return out
    for r in range(node.n_rows):
        if r not in node.links:
            out[r] = EXO[node.row_class(r)](y) * (1.0 + 0.01 * r)
    return out


def generate(seed: int, N: int = 8, T: int = 17, max_handles: int = 30) -> Graph:
    """A linked graph drawn from `seed`: 3 to max_handles handles in execution order, heavy (non-fusable) handles placed so the order
    falls into 1 to 5 segments, every input row either exogenous or linked to a handle of the same value class (earlier or later in
    the order, read at n or n + 1), Sum / Mean / Weighted aggregates with 1 to 8 contributors."""
    rng = np.random.default_rng([seed, 0x10C5])
    while True:
        if rng.random() < 0.3:   # light kinds the group kernel keeps in LDS only: a whole-graph launch with cache slots
            n = int(rng.integers(3, 13))
            kinds = [L.KIND_AGGREGATE if rng.random() < 0.25 else int(rng.choice([k for k in SMALL_KINDS if k != L.KIND_AGGREGATE]))
                     for _ in range(n)]
            table_ghg = set()
        else:
            n = int(rng.integers(3, max_handles + 1))
            n_heavy = int(rng.integers(0, 5)) if n >= 4 else 0
            kinds = []
            for _ in range(n):
                if rng.random() < 0.25:
                    kinds.append(L.KIND_AGGREGATE)
                else:
                    kinds.append(int(rng.choice([k for k in LIGHT_KINDS if k != L.KIND_AGGREGATE])))
            for pos in rng.choice(n, size=n_heavy, replace=False):
                kinds[int(pos)] = int(rng.choice(HEAVY_KINDS))
            # (a GhgForcing handle on its table path keeps no links)
            table_ghg = set(int(p) for p in np.flatnonzero([k == L.KIND_GHG_FORCING for k in kinds]) if rng.random() < 0.4)
        graph = link_graph(kinds, rng, N=N, T=T, table_ghg=table_ghg)
        # (counted on the handles as linked: a GhgForcing left without a co2 producer to link is not fusable)
        if 1 <= len(segments([nd.light for nd in graph.nodes])) <= 5:
            return graph


def fuzz_graph(seed: int) -> Tuple[Graph, List[int]]:
    """The graph of fuzz seed `seed` (tests/test_gpu_lockstep_graphs.py): its member count drawn from MEMBER_COUNTS, and the
    points at which the cut runs end a call (pieces of one and two steps first)."""
    rng = np.random.default_rng([seed, 7])
    N = int(rng.choice(MEMBER_COUNTS))
    graph = generate(seed, N=N)
    cuts = sorted({1, 3} | {int(x) for x in rng.integers(4, graph.steps, size=2)})
    return graph, cuts


def link_graph(kinds, rng: np.random.Generator, N: int = 8, T: int = 17, table_ghg=frozenset()) -> Graph:
    """Handles of `kinds` in this order with parameters, aggregate classes and links drawn from `rng` (generate's rules);
    the GhgForcing handles at the positions `table_ghg` stay on their table path."""
    nodes: List[Node] = []
    for pos, k in enumerate(kinds):
        method = float(rng.integers(0, 2)) if k == L.KIND_GHG_FORCING else 1.0
        op = float(rng.choice(list(OPS.values())))
        node = Node(k, default_params(k, N, rng if rng.random() < 0.8 else None, ghg_method=method, op=op))
        node.n_rows = 41 if k == L.KIND_HALOCARBON else len(node.info.inputs)
        if k == L.KIND_AGGREGATE:
            node.n_rows = int(rng.integers(1, 9))
        nodes.append(node)
    # value classes of the aggregates: one some handle of the graph produces, where there is one
    producers: Dict[str, List[Tuple[int, int]]] = {}

    def out_classes():
        producers.clear()
        for q, nd in enumerate(nodes):
            if nd.kind == L.KIND_AGGREGATE and nd.agg_class is None:
                continue
            for v, c in nd.info.outputs.items() if nd.kind != L.KIND_AGGREGATE else ((1, nd.agg_class),):
                if c is not None:
                    producers.setdefault(c, []).append((q, v))

    out_classes()
    for nd in nodes:
        if nd.kind == L.KIND_AGGREGATE:
            have = [c for c in AGG_CLASSES if c in producers]
            nd.agg_class = str(rng.choice(have or list(AGG_CLASSES)))
            if nd.agg_class in MEAN_ONLY:
                nd.params[0] = OPS["Mean"]
    out_classes()
    for i, nd in enumerate(nodes):
        if nd.kind == L.KIND_HALOCARBON or i in table_ghg:
            continue
        for r in range(nd.n_rows):
            cands = [(q, v) for q, v in producers.get(nd.row_class(r), []) if q != i and (nd.kind != L.KIND_UDEB or q < i)]
            if not cands or rng.random() < 0.35:
                continue
            q, v = cands[int(rng.integers(len(cands)))]
            upstream = bool(rng.random() < 0.5) if q < i else False   # a later producer's row n + 1 is not written yet: read at n
            nd.links[r] = Link(q, v, upstream)
        if nd.kind == L.KIND_AGGREGATE and all(nd.links[r].src > i for r in range(nd.n_rows) if r in nd.links) \
                and all(r in nd.links for r in range(nd.n_rows)):
            del nd.links[int(rng.integers(nd.n_rows))]   # one contributor the aggregate can see at the end of the step
        if nd.kind == L.KIND_GHG_FORCING and not nd.links:
            cands = [(q, v) for q, v in producers.get("co2_conc", []) if q != i]
            if cands:
                q, v = cands[int(rng.integers(len(cands)))]
                nd.links[0] = Link(q, v, q < i and bool(rng.random() < 0.5))
    return Graph(nodes, T, N)


def hand_graph(kinds, links=(), N=203, T=13, uniform=False, seed=0, agg=None) -> Graph:
    """A graph of `kinds` in this order; links: (consumer, row, producer, var, upstream); agg: position -> (class, n_rows, op).
    `uniform`: the oracle's default parameters for every member (no row varies)."""
    rng = np.random.default_rng(seed)
    nodes = []
    for k in kinds:
        nd = Node(k, default_params(k, N, None if uniform else rng))
        nd.n_rows = 41 if k == L.KIND_HALOCARBON else len(nd.info.inputs)
        nodes.append(nd)
    for pos, (cls, n_rows, op) in (agg or {}).items():
        nodes[pos].agg_class, nodes[pos].n_rows = cls, n_rows
        nodes[pos].params[0] = OPS[op]
    for i, r, q, v, up in links:
        assert nodes[i].row_class(r) == nodes[q].out_class(v), (i, r, q, v)
        nodes[i].links[r] = Link(q, v, up)
    return Graph(nodes, T, N)


def slot_budget_graph(uniform: bool) -> Graph:
    """Eight small light kinds with 22 series and 31 parameter rows against the 20-slot budget: the series of the first seven
    handles take 18 slots, the last FourBox gets none; of the parameter rows only CO2ERF's fit (uniform=False).  The first two
    handles read row n of later producers that hold slots (link_warm)."""
    kinds = (L.KIND_FOURBOX_OHU, L.KIND_CARBON_CYCLE, L.KIND_CO2_ERF, L.KIND_FOURBOX_OHU, L.KIND_AGGREGATE, L.KIND_TWO_LAYER,
             L.KIND_CO2_BUDGET, L.KIND_FOURBOX_OHU)
    links = ((0, 0, 4, 1, False),   # the aggregate, later, at n: warm
             (1, 1, 5, 1, False),   # the two-layer temperature, later, at n: warm
             (2, 0, 1, 1, True),    # an earlier producer at n + 1: from its slot
             (3, 0, 2, 1, False),   # an earlier producer at n: from HBM (its slot already holds n + 1)
             (4, 0, 2, 1, True), (5, 0, 4, 1, True), (7, 0, 4, 1, True))
    return hand_graph(kinds, links, N=257, T=15, uniform=uniform, agg={4: ("erf", 2, "Sum")})


# ------------------------------------------------------------------------------------------------ the plan rscm_ens_run_lockstep makes
def segments(light: List[bool], fuse: bool = True) -> List[Tuple[int, int]]:
    """(first, count) per segment: consecutive fusable handles, at most MAX_GROUP_OPS of them; every other handle on its own."""
    out, k = [], 0
    while k < len(light):
        c = 1
        if fuse and light[k]:
            while k + c < len(light) and c < MAX_GROUP_OPS and light[k + c]:
                c += 1
        out.append((k, c))
        k += c
    return out


def fuse_flags(mode: int) -> Dict[str, bool]:
    """rscm_gpu_set_lockstep_fusion."""
    return dict(fuse=mode != 0, cache=mode == 1 or mode >= 3, by_value=mode != 3, split=mode != 4, merge=mode != 5,
                own_cut=mode not in (5, 6))


def merge_eligible(graph: Graph, segs: List[Tuple[int, int]]) -> bool:
    """The merged schedule's conditions bar the mode and the step count: at least three segments, F and L fusable, F + L <= 12,
    and no op of F reads the end of its step from a handle outside F."""
    if len(segs) < 3:
        return False
    F, Lst = segs[0], segs[-1]
    nodes = graph.nodes
    if not (nodes[F[0]].light and nodes[Lst[0]].light and F[1] + Lst[1] <= GROUP_TABLE_OPS):
        return False
    inside = range(F[0], F[0] + F[1])
    for k in inside:
        for r, l in nodes[k].links.items():
            if nodes[k].reads_end(r) and l.src not in inside:
                return False
    return True


def predict(graph: Graph, mode: int, step_begin: int, step_end: int, windows: Optional[List[Optional[int]]] = None) -> Dict[str, int]:
    """What rscm_gpu_lockstep_stats (launches, component_steps) and rscm_gpu_lockstep_merged_launches report for one call of
    rscm_ens_run_lockstep over [step_begin, step_end) in fusion mode `mode`; windows[k]: the window rows of handle k (None: full)."""
    f = fuse_flags(mode)
    n = len(graph.nodes)
    steps = step_end - step_begin
    segs = segments([nd.light for nd in graph.nodes], f["fuse"])
    out = dict(launches=0, component_steps=n * steps, merged=0)
    if steps <= 0:
        out["component_steps"] = 0
        return out
    if len(segs) == 1 and segs[0][1] > 1:
        chunk = steps
        for k, nd in enumerate(graph.nodes):
            if windows and windows[k] is not None:
                chunk = min(chunk, max(1, windows[k] - nd.keep_rows))
        out["launches"] = -(-steps // chunk)
        return out
    any_fused = any(c > 1 for _, c in segs)
    if f["fuse"] and f["merge"] and f["by_value"] and any_fused and steps >= 2 and merge_eligible(graph, segs):
        out["launches"] = steps * (len(segs) - 1) + 1
        out["merged"] = steps - 1
    else:
        out["launches"] = steps * len(segs)
    return out


def whole_graph_chunk(graph: Graph, windows: Optional[List[Optional[int]]]) -> Optional[int]:
    """Steps per launch of a graph that is one fused segment (None if it is not)."""
    segs = segments([nd.light for nd in graph.nodes])
    if not (len(segs) == 1 and segs[0][1] > 1):
        return None
    chunk = graph.steps
    for k, nd in enumerate(graph.nodes):
        if windows and windows[k] is not None:
            chunk = min(chunk, max(1, windows[k] - nd.keep_rows))
    return chunk


@dataclass
class CachePlan:
    """What fused_segment and assign_cache_slots decide for a multi-step whole-graph launch."""
    own_kernel: bool                  # group_seq_kernel (parameters in registers: no parameter slots)
    slots: int                        # LDS slots in use (0: none, the op interpreter reads everything from HBM)
    series_slot: List[int]            # per op: first series slot or -1
    param_slot: List[int]             # per op: first parameter slot or -1
    link_slot: Dict[Tuple[int, int], int]   # (op, input row) -> slot the link is served from
    warm: List[Tuple[int, int]]       # the links served from a later producer's slot (link_warm: not at a launch's first step)


def cache_plan(graph: Graph, mode: int = 1) -> Optional[CachePlan]:
    """The LDS slots of the graph's multi-step launches (None when the graph is not one fused segment); assign_cache_slots restated."""
    f = fuse_flags(mode)
    nodes = graph.nodes
    if not f["fuse"] or whole_graph_chunk(graph, None) is None:
        return None
    kinds = tuple(nd.kind for nd in nodes)
    all_small = all(k in SMALL_KINDS for k in kinds)
    if not (all_small and f["cache"]):
        return CachePlan(False, 0, [-1] * len(nodes), [-1] * len(nodes), {}, [])
    own = f["by_value"] and len(nodes) <= GROUP_TABLE_OPS and kinds in OWN_SEQUENCES
    series, params, nxt = [], [], 0
    for nd in nodes:
        n_series = max(L.KIND_TABLE[nd.kind][0].values())
        if n_series > 0 and nxt + n_series <= CACHE_SLOT_BUDGET:
            series.append(nxt)
            nxt += n_series
        else:
            series.append(-1)
    for nd in nodes:
        P = nd.params.shape[0]
        varies = bool((nd.params != nd.params[:, :1]).any())
        if not own and nd.kind != L.KIND_AGGREGATE and varies and P <= 16 and nxt + P <= CACHE_SLOT_BUDGET:
            params.append(nxt)
            nxt += P
        else:
            params.append(-1)
    link_slot, warm = {}, []
    for k, nd in enumerate(nodes):
        for r, l in sorted(nd.links.items()):
            at = l.src
            if series[at] < 0:
                continue
            reads_end = nd.reads_end(r)
            if (not reads_end) if at < k else reads_end:
                continue   # the slot holds the other row at that point of the step
            link_slot[(k, r)] = series[at] + l.var - 1
            if at >= k:
                warm.append((k, r))
    if nxt <= 0:
        own = False
    return CachePlan(own, nxt, series, params, link_slot, warm)


def ties(graph: Graph, idx: List[int], off: List[int]) -> np.ndarray:
    """plan_split's tie relation over the ops (handle idx[k] at step offset off[k]): op k reads row off[k] + (1 if it reads the end
    of its step else 0) of producer q, which writes row off[q] + 1; the two are tied when that is the same row."""
    m = len(idx)
    tie = np.zeros((m, m), dtype=bool)
    for k in range(m):
        nd = graph.nodes[idx[k]]
        for r, l in nd.links.items():
            row = off[k] + (1 if nd.reads_end(r) else 0)
            for q in range(m):
                if q != k and idx[q] == l.src and row == off[q] + 1:
                    tie[k, q] = tie[q, k] = True
    return tie


# ------------------------------------------------------------------------------------------------ closed-loop reference
def read_at_steps(src: np.ndarray, reads_end: bool, producer_first: bool) -> np.ndarray:
    """What a consumer read of the stored series `src` ([T] or [T][M]) at every step n (the last entry is unused): row n + 1 if it
    reads the end of its step -- NaN where the producer comes later in the execution order and has not written that row yet --
    else row n.  (The reading rule of the closed-loop checks here and in tests/test_gpu_links.py.)"""
    out = np.full_like(src, np.nan)
    if reads_end:
        if producer_first:
            out[:-1] = src[1:]
    else:
        out[:-1] = src[:-1]
    return out


def relative_error(got: np.ndarray, want: np.ndarray, what: str) -> float:
    """The worst deviation of `got` from `want` relative to max(1, |want|); the NaN patterns must be the same."""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if (nan_g != nan_w).any():
        where = tuple(np.argwhere(nan_g != nan_w)[0])
        raise AssertionError(f"{what}: NaN pattern differs ({nan_g.sum()} vs {nan_w.sum()} NaN) first at {where}: "
                             f"stored {got[where]!r}, recomputed {want[where]!r}")
    ok = ~nan_w
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    return float(err.max()) if err.size else 0.0


def seen_row(graph: Graph, i: int, r: int, S: Dict[Tuple[int, int], np.ndarray]) -> np.ndarray:
    """[T][M]: what input row r of handle i read at every step n (read_at_steps; an exogenous row: the table's series).
    ClimateUDEB reads rows n and n + 1 of its input itself: it gets the producer's series as it stands."""
    nd = graph.nodes[i]
    M = next(iter(S.values())).shape[1]
    if r not in nd.links:
        x = exogenous_block(nd, graph.T)[r]
        if nd.kind == L.KIND_AGGREGATE:   # (its table rows too are read at the end of the step)
            x = np.append(x[1:], np.nan)
        return np.repeat(x[:, None], M, axis=1)
    l = nd.links[r]
    src = S[(l.src, l.var)]
    if nd.kind == L.KIND_UDEB:
        assert l.src < i
        return src.copy()
    return read_at_steps(src, nd.reads_end(r), l.src < i)


def recompute(graph: Graph, i: int, S: Dict[Tuple[int, int], np.ndarray], members: np.ndarray) -> Dict[int, np.ndarray]:
    """Handle i's stored series ([T][M] per variable) recomputed by its CPU oracle from the rows it read (`S`: every handle's
    series, [T][M] over the checked members) and its parameters; row 0 is the initial value."""
    from oracle import cbind as orc
    nd = graph.nodes[i]
    T = graph.T
    M = len(members)
    P = np.ascontiguousarray(nd.params[:, members])
    b = np.arange(T + 1, dtype=np.float64)
    scen = np.arange(M, dtype=np.int32)
    n_in = 41 if nd.kind == L.KIND_HALOCARBON else (8 if nd.kind == L.KIND_AGGREGATE else len(nd.info.inputs))
    rows = [seen_row(graph, i, r, S) if r < nd.n_rows else np.full((T, M), np.nan) for r in range(n_in)]
    block = np.ascontiguousarray(np.stack(rows, axis=1).transpose(2, 1, 0))   # [M][rows][T]: one scenario per member
    k = nd.kind
    init = nd.init
    out: Dict[int, np.ndarray] = {}
    if k in (L.KIND_OZONE_FORCING, L.KIND_AEROSOL_DIRECT, L.KIND_AEROSOL_INDIRECT, L.KIND_FOURBOX_OHU, L.KIND_OSPP):
        o = orc.pointwise_run(k, T, P, block, scen=scen)
        out = {v + 1: o[v] for v in range(o.shape[0])}
    elif k in (L.KIND_CH4_CHEMISTRY, L.KIND_N2O_CHEMISTRY):
        conc, life = orc.chem_run(k, b, P, block, init[1], scen=scen)
        out = {1: conc, 2: life}
    elif k in (L.KIND_CO2_BUDGET, L.KIND_TERRESTRIAL_CARBON):
        ns = 1 if k == L.KIND_CO2_BUDGET else 4
        o = orc.carbon_run(k, b, P, block, [init[v] for v in range(1, ns + 1)], scen=scen)
        out = {v + 1: o[v] for v in range(o.shape[0])}
    elif k == L.KIND_GHG_FORCING:
        g = orc.ghg_run(T, P, block, scen=scen)
        out = {v + 1: g[key] for v, key in enumerate(orc.GHG_VARS)}
    elif k == L.KIND_OCEAN_CARBON:
        o = orc.ocean_run(b, P, block, init[1], init[2], scen=scen)
        out = {v + 1: o[v] for v in range(3)}
    elif k == L.KIND_HALOCARBON:
        o = orc.halo_run(b, P, block, [init[v] for v in range(1, 42)], scen=scen)
        out = {v + 1: o[v] for v in range(o.shape[0])}
    elif k == L.KIND_UDEB:
        u, _ = orc.udeb_run(b, P, block[:, 0, :], scen=scen)
        out = {v + 1: u[key] for v, key in enumerate(("st0", "st1", "st2", "st3", "heat_uptake", "ohc", "sst"))}
    elif k == L.KIND_TWO_LAYER:
        ts, td = orc.two_layer_run(b, P, block[:, 0, :], init[1], init[2], scen=scen)
        out = {1: ts, 2: td}
    elif k == L.KIND_CARBON_CYCLE:
        y = np.full((3, T, M), np.nan)
        for m in range(M):
            st = np.array([init[1], init[2], init[3]])
            y[:, 0, m] = st
            for n in range(T - 1):
                st = orc.carbon_cycle_solve(P[:, m], block[m, 0, n], block[m, 1, n], b[n], b[n + 1], 0.1, st)
                y[:, n + 1, m] = st
        out = {1: y[0], 2: y[1], 3: y[2]}
    elif k == L.KIND_CO2_ERF:
        e = np.full((T, M), np.nan)
        for m in range(M):
            for n in range(T - 1):
                e[n + 1, m] = orc.co2_erf(P[0, m], P[1, m], block[m, 0, n])
        out = {1: e}
    elif k == L.KIND_AGGREGATE:
        a = np.full((T, M), np.nan)
        op = P[0, 0]
        for n in range(T - 1):
            acc, cnt = np.zeros(M), np.zeros(M)
            for r in range(nd.n_rows):
                v = block[:, r, n]
                ok = ~np.isnan(v)
                acc = np.where(ok, acc + (v * P[1 + r] if op == OPS["Weighted"] else v), acc)
                cnt += ok
            a[n + 1] = np.where(cnt > 0, acc / np.maximum(cnt, 1.0) if op == OPS["Mean"] else acc, np.nan)
        out = {1: a}
    for v, x in out.items():
        x[0] = init[v]
    return {v: out[v] for v in nd.info.outputs}


def host_run(graph: Graph, members: np.ndarray) -> Dict[Tuple[int, int], np.ndarray]:
    """The graph stepped on the host, handle by handle in execution order, each handle's row n + 1 from the oracles
    (recompute over the rows written so far: a row depends on nothing after it)."""
    M = len(members)
    S = {}
    for i, nd in enumerate(graph.nodes):
        for v in nd.info.outputs:
            S[(i, v)] = np.full((graph.T, M), np.nan)
            S[(i, v)][0] = nd.init[v]
    for n in range(graph.steps):
        for i in range(len(graph.nodes)):
            got = recompute(graph, i, S, members)
            for v, x in got.items():
                S[(i, v)][n + 1] = x[n + 1]
    return S


def closed_loop_errors(graph: Graph, S: Dict[Tuple[int, int], np.ndarray], members: np.ndarray) -> Dict[Tuple[int, int], float]:
    """Per series: the worst relative deviation of the stored rows from the recomputed ones.  The NaN pattern must be exact."""
    worst = {}
    for i, nd in enumerate(graph.nodes):
        want = recompute(graph, i, S, members)
        for v, w in want.items():
            worst[(i, v)] = relative_error(S[(i, v)], w, f"handle {i} ({nd.info.name}) variable {v} (row, member)")
    return worst


def check_closed_loop(graph: Graph, S: Dict[Tuple[int, int], np.ndarray], members: np.ndarray) -> None:
    for (i, v), e in closed_loop_errors(graph, S, members).items():
        nd = graph.nodes[i]
        assert e <= nd.info.tol, f"handle {i} ({nd.info.name}) variable {v}: relative deviation {e:.3e} > {nd.info.tol:g}"
