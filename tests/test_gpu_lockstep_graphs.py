"""The lock-step scheduler (csrc/lockstep.cpp rscm_ens_run_lockstep, csrc/group.hip) on graphs built for each of its paths and
on seeded random graphs (tests/host_lockstep.py): segments of every length, whole-graph launches with LDS slots, by-value and
device tables, the two-wavefront cut, the merged schedule and its refusals.  For every graph the launch counters equal the
host restatement of the plan, every fusion mode carries the bits of the unfused run (mode 0) -- with full storage, minimal
windows and strided output, in one call and in pieces -- and the first members pass a closed-loop check against the CPU
oracles."""
import ctypes as C

import numpy as np
import pytest

from tests import host_lockstep as H
from tests.gpu_support import ra  # noqa: F401
from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

FUZZ_SEEDS = range(32)


@pytest.fixture(autouse=True)
def _fusion_back_on():
    yield
    from rscm_amd import _lib as L
    L.check(L.load().rscm_gpu_set_lockstep_fusion(1))


@pytest.fixture(scope="module")
def stream(ra):
    from rscm_amd import _lib as L
    s = C.c_void_p()
    L.check(L.load().rscm_gpu_stream_create(0, C.byref(s)))
    yield s.value
    L.check(L.load().rscm_gpu_stream_destroy(0, s))


def _counters():
    """(launches, component_steps, merged, split) since the last call; resets them."""
    from rscm_amd import _lib as L
    lib = L.load()
    a, b, m, s = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    L.check(lib.rscm_gpu_lockstep_stats(C.byref(a), C.byref(b)))
    L.check(lib.rscm_gpu_lockstep_merged_launches(C.byref(m)))
    L.check(lib.rscm_gpu_lockstep_split_launches(C.byref(s)))
    return a.value, b.value, m.value, s.value


def _layout():
    from rscm_amd import _lib as L
    out = (C.c_int32 * (3 + 2 * H.GROUP_TABLE_OPS))()
    L.check(L.load().rscm_gpu_lockstep_last_layout(out))
    return list(out)


class Built:
    """The graph as linked ensembles on one stream; `window`: None (full storage), "min" (2 x keep_rows rows and every row
    output) or (rows, stride)."""

    def __init__(self, ra, graph, stream, window=None):
        self.graph = graph
        T = graph.T
        b = np.arange(T + 1, dtype=np.float64)
        self.stride = 1
        self.ens, self.windows = [], []
        try:
            for nd in graph.nodes:
                if window is None:
                    e = ra.Ensemble(nd.kind, graph.N, b)
                elif window == "min":
                    e = ra.Ensemble(nd.kind, graph.N, b, window_rows=2 * nd.keep_rows, output_stride=1)
                else:
                    e = ra.Ensemble(nd.kind, graph.N, b, window_rows=max(window[0], 2 * nd.keep_rows), output_stride=window[1])
                    self.stride = window[1]
                self.ens.append(e)
                self.windows.append(e.window_rows)
                e.set_stream(stream)
                e.set_params(nd.params)
                blk = H.exogenous_block(nd, T)
                e.set_forcing(blk[0] if e.input_rows is None else blk)
                for v, x in nd.init.items():
                    e.set_initial(v, x)
            from rscm_amd import _lib as L
            for i, nd in enumerate(graph.nodes):
                for r, l in nd.links.items():
                    self.ens[i].link_input(r, self.ens[l.src], l.var, L.SRC_UPSTREAM if l.upstream else L.SRC_EXOGENOUS)
                L.check(L.load().rscm_ens_set_link_order_check(self.ens[i]._h, 0))
        except Exception:
            self.close()
            raise

    def run(self, mode, cuts=()):
        """Steps the whole axis in fusion mode `mode`, in calls ending at `cuts` and at the end; returns the counters summed over the
        calls and the prediction of the host restatement."""
        from rscm_amd import _lib as L
        from rscm_amd.ensemble import run_lockstep
        L.check(L.load().rscm_gpu_set_lockstep_fusion(mode))
        _counters()
        want = dict(launches=0, component_steps=0, merged=0)
        begin = 0
        for stop in list(cuts) + [self.graph.steps]:
            run_lockstep(self.ens, stop)
            for k, v in H.predict(self.graph, mode, begin, stop, self.windows).items():
                want[k] += v
            begin = stop
        launches, steps, merged, split = _counters()
        return dict(launches=launches, component_steps=steps, merged=merged), want, split

    def series(self):
        return {(i, v): e.get_series(v, t_stride=self.stride) for i, (e, nd) in enumerate(zip(self.ens, self.graph.nodes))
                for v in nd.info.outputs}

    def close(self):
        for i, nd in enumerate(self.graph.nodes):
            if i < len(self.ens):
                for r in nd.links:
                    try:
                        self.ens[i].unlink_input(r)
                    except Exception:
                        pass
        for e in self.ens:
            e.close()


def exercise(ra, graph, stream, modes=range(H.N_MODES), windows=(None, "min", (7, 3)), cuts=(), closed_loop=True):
    """Runs `graph` in every mode and storage; asserts the counters and the bits against mode 0 of full storage.  Returns what the
    mode 1 runs reached: merged and split launches (the device's counters); multi-step launches with LDS slots, links served warm
    from a later producer's slot, parameter slots (the restatement of assign_cache_slots for those launches); a device table."""
    reached = dict(merged=0, split=0, cached=0, warm=0, params=0)
    cp = H.cache_plan(graph, 1)
    ref = None
    for window in windows:
        for mode in modes:
            for pieces in ((), tuple(cuts)) if cuts and window is None else ((),):
                g = Built(ra, graph, stream, window)
                try:
                    got, want, split = g.run(mode, pieces)
                    what = f"mode {mode} window {window} cuts {pieces}"
                    assert got == want, f"{what}: counters {got} != predicted {want}"
                    if mode == 1:
                        reached["merged"] += got["merged"]
                        reached["split"] += split
                        if H.whole_graph_chunk(graph, g.windows) not in (None, 1) and cp.slots > 0:
                            reached["cached"] += 1
                            reached["warm"] += len(cp.warm)
                            reached["params"] += sum(p >= 0 for p in cp.param_slot)
                    if mode == 4:
                        assert split == 0, what
                    S = g.series()
                    if ref is None:
                        assert window is None and mode == 0 and not pieces
                        ref = S
                        continue
                    for key, x in S.items():
                        assert_bit_equal(x, ref[key][::g.stride], f"{what}: handle {key[0]} ({graph.nodes[key[0]].info.name}) var {key[1]}")
                    if closed_loop and mode == 1 and window is None and not pieces:
                        members = np.arange(min(8, graph.N))
                        H.check_closed_loop(graph, {k: np.ascontiguousarray(x[:, members]) for k, x in S.items()}, members)
                finally:
                    g.close()
    reached["table"] = int(any(c > H.GROUP_TABLE_OPS for _, c in H.segments([nd.light for nd in graph.nodes])))
    return reached


# ------------------------------------------------------------------------------------------------ hand-built graphs
hand = H.hand_graph
K = H.L
# (a) [CO2ERF TwoLayer] OceanCarbon [CO2Budget Aggregate]: merged, and the merged launch has no cut -- F reads L's row n (tied at
# step offsets 1 and 0), each segment is a chain
GRAPH_A = dict(kinds=(K.KIND_CO2_ERF, K.KIND_TWO_LAYER, K.KIND_OCEAN_CARBON, K.KIND_CO2_BUDGET, K.KIND_AGGREGATE),
               links=((0, 0, 3, 1, False), (1, 0, 0, 1, True), (4, 0, 3, 1, True), (2, 0, 3, 1, False)),
               agg={4: ("co2_conc", 2, "Mean")})


def test_merged_launch_that_plan_split_refuses(ra, stream):
    """ADVICE (a): the merged launch goes through the plain group kernel with step_off = 1 for F's ops."""
    g = hand(**GRAPH_A)
    idx, off = [3, 4, 0, 1], [0, 0, 1, 1]
    t = H.ties(g, idx, off)
    assert t[0, 1] and t[2, 0] and t[3, 2]   # one connected set: plan_split has nothing to cut
    b = Built(ra, g, stream)
    try:
        got, want, split = b.run(1)
        assert got == want and got["merged"] == g.steps - 1 > 0 and split == 0, (got, want, split)
    finally:
        b.close()
    exercise(ra, g, stream, cuts=(1, 3))


def test_no_merge_on_a_read_ahead_link_into_F(ra, stream):
    """ADVICE (b): an aggregate of F reads the end of its step from L: the window of L's handle would have to move first."""
    g = hand(kinds=(K.KIND_CO2_ERF, K.KIND_AGGREGATE, K.KIND_OCEAN_CARBON, K.KIND_CO2_BUDGET, K.KIND_AGGREGATE),
             links=((0, 0, 3, 1, False), (1, 0, 3, 1, True), (4, 0, 3, 1, True)),
             agg={1: ("co2_conc", 2, "Mean"), 4: ("co2_conc", 2, "Mean")})
    segs = H.segments([nd.light for nd in g.nodes])
    assert len(segs) == 3 and not H.merge_eligible(g, segs)
    b = Built(ra, g, stream)
    try:
        got, want, _ = b.run(1)
        assert got == want and got["merged"] == 0 and got["launches"] == 3 * g.steps, (got, want)
    finally:
        b.close()
    exercise(ra, g, stream, cuts=(2,))


@pytest.mark.parametrize("shape", ["F1", "L1"])
def test_merged_launch_with_a_single_handle_segment(ra, stream, shape):
    """ADVICE (c): F (or L) is one handle: its prologue (epilogue) runs through run_range, inside the merged launch it runs through
    the fused body."""
    light3 = (K.KIND_AEROSOL_INDIRECT, K.KIND_CO2_ERF, K.KIND_AGGREGATE)
    if shape == "F1":   # [TwoLayer] OceanCarbon [AerosolIndirect CO2ERF Aggregate], the aggregate feeding the two-layer model
        g = hand(kinds=(K.KIND_TWO_LAYER, K.KIND_OCEAN_CARBON) + light3,
                 links=((0, 0, 4, 1, False), (1, 1, 0, 1, False), (4, 0, 2, 1, True), (4, 1, 3, 1, True)), agg={4: ("erf", 2, "Sum")})
    else:               # [AerosolIndirect CO2ERF Aggregate] OceanCarbon [TwoLayer]
        g = hand(kinds=light3 + (K.KIND_OCEAN_CARBON, K.KIND_TWO_LAYER),
                 links=((2, 0, 0, 1, True), (2, 1, 1, 1, True), (4, 0, 2, 1, True), (3, 1, 4, 1, False)),
                 agg={2: ("erf", 2, "Weighted")})
    segs = H.segments([nd.light for nd in g.nodes])
    assert min(segs[0][1], segs[-1][1]) == 1 and H.merge_eligible(g, segs)
    b = Built(ra, g, stream)
    try:
        got, want, _ = b.run(1)
        assert got == want and got["merged"] == g.steps - 1 > 0, (got, want)
    finally:
        b.close()
    exercise(ra, g, stream, cuts=(1, 2, 4))


INDEPENDENT = (K.KIND_CH4_CHEMISTRY, K.KIND_N2O_CHEMISTRY, K.KIND_TERRESTRIAL_CARBON, K.KIND_CARBON_CYCLE, K.KIND_OZONE_FORCING,
               K.KIND_AEROSOL_DIRECT, K.KIND_AEROSOL_INDIRECT, K.KIND_FOURBOX_OHU, K.KIND_OSPP, K.KIND_CO2_BUDGET, K.KIND_CO2_ERF,
               K.KIND_TWO_LAYER)


@pytest.mark.parametrize("n_ops", [9, 10, 12])
def test_split_launch_of_nine_to_twelve_ops(ra, stream, n_ops):
    """ADVICE (d): a one-step segment of 9-12 ops (by value since kGroupTableOps = 12) cut over two wavefronts.  Distinct kinds, so the
    recorded layout names its ops: two non-empty sets with no tie between them, each in graph order, then the tail."""
    kinds = INDEPENDENT[:n_ops - 1] + (K.KIND_AGGREGATE,)
    # a few ties: the aggregate (the tail's candidate) reads three ops at the end of the step, the budget reads the terrestrial flux
    links = [(n_ops - 1, 0, 4, 1, True), (n_ops - 1, 1, 5, 1, True), (n_ops - 1, 2, 6, 1, True)]
    if n_ops >= 11:
        links.append((9, 2, 2, 5, True))
    g = hand(kinds=kinds + (K.KIND_OCEAN_CARBON,), links=links, agg={n_ops - 1: ("erf", 3, "Sum")})
    b = Built(ra, g, stream)
    try:
        got, want, split = b.run(1)
        assert got == want and split == g.steps, (got, want, split)
        lay = _layout()
        total, n1, n2 = lay[:3]
        assert total == n_ops and n1 > 0 and n2 > 0 and n1 + n2 <= n_ops, lay[:3]
        ops = [lay[3 + 2 * k] for k in range(total)]
        assert all(lay[4 + 2 * k] & 0xFF == 0 for k in range(total))
        pos = [kinds.index(kd) for kd in ops]
        first, second = pos[:n1], pos[n1:n1 + n2]
        assert first == sorted(first) and second == sorted(second) and pos[n1 + n2:] == sorted(pos[n1 + n2:])
        t = H.ties(g, list(range(n_ops)), [0] * n_ops)
        assert not t[np.ix_(first, second)].any(), (first, second)
    finally:
        b.close()
    exercise(ra, g, stream, windows=(None, "min"), cuts=(1,))


@pytest.mark.parametrize("n_light", [13, 16, 17, 21])
def test_long_segments(ra, stream, n_light):
    """Segments of 13-16 ops (device table) and longer ones, cut at 16, in front of a heavy handle and as the whole graph."""
    rng = np.random.default_rng(n_light)
    pool = [k for k in H.LIGHT_KINDS if k != K.KIND_GHG_FORCING]
    kinds = tuple(int(rng.choice(pool)) for _ in range(n_light))
    for tail in ((K.KIND_UDEB,), ()):
        g = H.link_graph(kinds + tail, rng, N=65, T=11)
        segs = H.segments([nd.light for nd in g.nodes])
        assert segs[0][1] == min(n_light, H.MAX_GROUP_OPS)
        exercise(ra, g, stream, windows=(None, "min"), cuts=(1, 3))


@pytest.mark.parametrize("uniform", [False, True])
def test_whole_light_graph_over_the_slot_budget(ra, stream, uniform):
    """A graph of small light kinds runs many steps per launch with LDS slots (tests/host_lockstep.py slot_budget_graph): the series
    and parameter rows overflow the 20-slot budget, consumers ahead of their producers read row n from the slot the producer left in
    the previous step (link_warm: from HBM at a launch's first, cold step, which minimal windows make recur every two steps).
    `uniform`: every parameter row is the same over the members, so no op gets a parameter slot."""
    g = H.slot_budget_graph(uniform)
    cp = H.cache_plan(g)
    assert cp.slots > 0 and not cp.own_kernel and -1 in cp.series_slot
    assert set(cp.warm) >= {(0, 0), (1, 1)}
    assert (sum(p >= 0 for p in cp.param_slot) == 0) == uniform
    reached = exercise(ra, g, stream, cuts=(1, 2, 5))
    assert reached["cached"] >= 2 and reached["warm"] > 0


@pytest.mark.parametrize("order", ["coupled", "forced", "permuted"])
def test_sequences_with_a_kernel_of_their_own(ra, stream, order):
    """SeqCoupled (CarbonCycle CO2ERF Aggregate TwoLayer) and SeqForced (Aggregate TwoLayer) go through group_seq_kernel (series in LDS
    slots, parameters in registers); the same kinds in an order that matches no sequence through the interpreter, with parameter
    slots.  Same bits as the unfused run either way."""
    if order == "coupled":
        g = hand(kinds=(K.KIND_CARBON_CYCLE, K.KIND_CO2_ERF, K.KIND_AGGREGATE, K.KIND_TWO_LAYER),
                 links=((0, 1, 3, 1, False), (1, 0, 0, 1, True), (2, 0, 1, 1, True), (3, 0, 2, 1, True)), agg={2: ("erf", 2, "Sum")})
    elif order == "forced":
        g = hand(kinds=(K.KIND_AGGREGATE, K.KIND_TWO_LAYER), links=((1, 0, 0, 1, True),), agg={0: ("erf", 3, "Weighted")})
    else:
        g = hand(kinds=(K.KIND_CO2_ERF, K.KIND_CARBON_CYCLE, K.KIND_TWO_LAYER, K.KIND_AGGREGATE),
                 links=((0, 0, 1, 1, False), (1, 1, 2, 1, False), (3, 0, 0, 1, True), (2, 0, 3, 1, False)), agg={3: ("erf", 2, "Mean")})
    cp = H.cache_plan(g)
    assert cp.slots > 0 and cp.own_kernel == (order != "permuted")
    assert any(p >= 0 for p in cp.param_slot) == (order == "permuted")
    exercise(ra, g, stream, cuts=(1, 2, 6))


# ------------------------------------------------------------------------------------------------ fuzz
def test_generated_graphs(ra, stream):
    """Seeded graphs (tests/host_lockstep.py fuzz_graph): every fusion mode, three storages, one call and calls cut at random points,
    members in {1, 63, 64, 65, 203, 257}; the paths reached over the seed set are counted and must stay reached."""
    totals = dict(merged=0, split=0, cached=0, warm=0, params=0, table=0)
    for seed in FUZZ_SEEDS:
        graph, cuts = H.fuzz_graph(seed)
        reached = exercise(ra, graph, stream, cuts=cuts)
        for k in totals:
            totals[k] += int(reached[k] > 0)
    print("graphs that reached each path:", totals)
    assert totals["merged"] >= 3 and totals["split"] >= 10 and totals["table"] >= 4, totals
    assert totals["cached"] >= 8 and totals["warm"] >= 5 and totals["params"] >= 4, totals
