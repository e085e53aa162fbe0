"""The host side of the lock-step scheduler tests (tests/host_lockstep.py): the graph generator, the restatement of the launch plan
on hand-derived cases, and the closed-loop reference run on the host with the oracles alone."""
import numpy as np
import pytest

from tests import host_lockstep as H

K = H.L


def _graph(spec, N=4, T=11, links=()):
    """spec: a string of L (light: CO2ERF) and H (heavy: OceanCarbon) handles."""
    kinds = [K.KIND_CO2_ERF if c == "L" else K.KIND_OCEAN_CARBON for c in spec]
    nodes = []
    for k in kinds:
        nd = H.Node(k, H.default_params(k, N, None))
        nd.n_rows = len(nd.info.inputs)
        nodes.append(nd)
    for i, r, q, v, up in links:
        nodes[i].links[r] = H.Link(q, v, up)
    return H.Graph(nodes, T, N)


FUZZ_SEEDS = range(32)   # those of tests/test_gpu_lockstep_graphs.py


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_generator_is_deterministic_and_typed(seed):
    (a, cuts), (b, cuts_b) = H.fuzz_graph(seed), H.fuzz_graph(seed)
    assert cuts == cuts_b and cuts[:2] == [1, 3] and cuts[-1] < a.steps and a.N in H.MEMBER_COUNTS
    assert [nd.kind for nd in a.nodes] == [nd.kind for nd in b.nodes]
    assert [{r: vars(l) for r, l in nd.links.items()} for nd in a.nodes] == [{r: vars(l) for r, l in nd.links.items()} for nd in b.nodes]
    for x, y in zip(a.nodes, b.nodes):
        assert np.array_equal(x.params, y.params)
    assert 3 <= len(a.nodes) <= 30
    assert 1 <= len(H.segments([nd.light for nd in a.nodes])) <= 5
    for i, nd in enumerate(a.nodes):
        if nd.kind == K.KIND_AGGREGATE:
            assert 1 <= nd.n_rows <= 8 and nd.params[0, 0] in H.OPS.values()
        exo = H.exogenous_block(nd, a.T)
        for r in range(nd.n_rows):
            if r in nd.links:
                l = nd.links[r]
                assert l.src != i and a.nodes[l.src].out_class(l.var) == nd.row_class(r), (i, r)
                assert np.isnan(exo[r]).all()
                if l.src > i:   # a later producer is read at n (an aggregate reads the end of its step: NaN, skipped)
                    assert not l.upstream and nd.kind != K.KIND_UDEB
            else:
                assert np.isfinite(exo[r]).all()


def test_fuzz_graphs_stay_finite_and_reach_the_paths():
    """The host run of every fuzz graph (each handle's row n + 1 from the oracles, in execution order) leaves >= 90 % of the stored
    entries finite -- a graph of NaNs could not pass the device comparison vacuously -- and passes its own closed-loop check.  The
    seed set reaches the plans the device test counts."""
    reach = dict(merge=0, table=0, cached=0, warm=0, params=0)
    for seed in FUZZ_SEEDS:
        g, _ = H.fuzz_graph(seed)
        members = np.arange(min(2, g.N))
        S = H.host_run(g, members)
        finite = sum(int(np.isfinite(x).sum()) for x in S.values()) / sum(x.size for x in S.values())
        assert finite >= 0.9, (seed, finite)
        H.check_closed_loop(g, S, members)
        segs = H.segments([nd.light for nd in g.nodes])
        reach["merge"] += H.merge_eligible(g, segs) and any(c > 1 for _, c in segs)
        reach["table"] += any(c > H.GROUP_TABLE_OPS for _, c in segs)
        cp = H.cache_plan(g)
        if cp and cp.slots > 0 and H.whole_graph_chunk(g, None) > 1:
            reach["cached"] += 1
            reach["warm"] += bool(cp.warm)
            reach["params"] += any(p >= 0 for p in cp.param_slot)
    assert reach["merge"] >= 3 and reach["table"] >= 4 and reach["cached"] >= 8 and reach["warm"] >= 5 and reach["params"] >= 4, reach


def test_cache_slots_of_the_slot_budget_graph():
    """assign_cache_slots restated on tests/test_gpu_lockstep_graphs.py's graph: series slots in order while the budget lasts, then
    parameter slots for the ops with a varying row, links served from a slot only where it holds the row they read."""
    for uniform in (False, True):
        cp = H.cache_plan(H.slot_budget_graph(uniform))
        assert not cp.own_kernel
        assert cp.series_slot == [0, 4, 7, 8, 12, 13, 15, -1]
        assert cp.param_slot == ([-1] * 8 if uniform else [-1, -1, 18, -1, -1, -1, -1, -1])
        assert cp.slots == (18 if uniform else 20)
        assert cp.link_slot == {(0, 0): 12, (1, 1): 13, (2, 0): 4, (4, 0): 7, (5, 0): 12, (7, 0): 12}   # (3, 0) reads HBM
        assert cp.warm == [(0, 0), (1, 1)]
    # not a single fused segment, or a kind that is not small: no slots
    assert H.cache_plan(_graph("LHL")) is None
    g = H.slot_budget_graph(False)
    g.nodes[6].kind = K.KIND_TERRESTRIAL_CARBON
    assert H.cache_plan(g).slots == 0
    assert H.cache_plan(H.slot_budget_graph(False), mode=2).slots == 0   # (mode 2: no slots)


def test_sequences_with_a_kernel_of_their_own_keep_no_parameter_slots():
    g = H.hand_graph((K.KIND_CARBON_CYCLE, K.KIND_CO2_ERF, K.KIND_AGGREGATE, K.KIND_TWO_LAYER), agg={2: ("erf", 2, "Sum")})
    cp = H.cache_plan(g)
    assert cp.own_kernel and cp.slots == 3 + 1 + 1 + 2 and cp.param_slot == [-1] * 4
    assert not H.cache_plan(g, mode=3).own_kernel   # the device table: no kernel of its own
    g = H.hand_graph((K.KIND_CO2_ERF, K.KIND_CARBON_CYCLE, K.KIND_TWO_LAYER, K.KIND_AGGREGATE), agg={3: ("erf", 2, "Sum")})
    cp = H.cache_plan(g)
    assert not cp.own_kernel and cp.param_slot == [7, 9, 12, -1]


def test_closed_loop_reference_catches_a_wrong_row():
    g = H.generate(1, N=3, T=9, max_handles=10)
    members = np.arange(3)
    S = H.host_run(g, members)
    key = next(k for k, x in S.items() if np.isfinite(x[5]).all() and g.nodes[k[0]].kind != K.KIND_HALOCARBON)
    S[key][5, 1] *= 1.0 + 1e-6
    with pytest.raises(AssertionError):
        H.check_closed_loop(g, S, members)
    S[key][5, 1] = np.nan
    with pytest.raises(AssertionError, match="NaN pattern"):
        H.check_closed_loop(g, S, members)


def test_plan_two_light_heavy_two_light():
    g = _graph("LLHLL")
    assert H.segments([nd.light for nd in g.nodes]) == [(0, 2), (2, 1), (3, 2)]
    steps = g.steps
    for mode in (1, 2, 4, 6):
        assert H.predict(g, mode, 0, steps) == dict(launches=2 * steps + 1, component_steps=5 * steps, merged=steps - 1)
    for mode in (3, 5):   # device table / round 5's plan: no merging
        assert H.predict(g, mode, 0, steps) == dict(launches=3 * steps, component_steps=5 * steps, merged=0)
    assert H.predict(g, 0, 0, steps) == dict(launches=5 * steps, component_steps=5 * steps, merged=0)
    # one step per call: nothing to merge; two steps: prologue, one merged launch, epilogue
    assert H.predict(g, 1, 3, 4) == dict(launches=3, component_steps=5, merged=0)
    assert H.predict(g, 1, 3, 5) == dict(launches=5, component_steps=10, merged=1)


def test_plan_one_light_heavy_three_light():
    g = _graph("LHLLL")
    steps = g.steps
    assert H.predict(g, 1, 0, steps) == dict(launches=2 * steps + 1, component_steps=5 * steps, merged=steps - 1)
    # a read-ahead link into F (row n + 1 of a handle outside F) refuses the merge
    g = _graph("LHLLL", links=((0, 0, 2, 1, True),))
    g.nodes[2].kind = K.KIND_CO2_BUDGET
    assert not H.merge_eligible(g, H.segments([nd.light for nd in g.nodes]))
    assert H.predict(g, 1, 0, steps)["merged"] == 0
    # the same link read at n is no read-ahead
    g.nodes[0].links[0].upstream = False
    assert H.predict(g, 1, 0, steps)["merged"] == steps - 1
    # one light handle on each side and no segment of two: no fused launch at all, hence no plan and no merge
    assert H.predict(_graph("LHLHL"), 1, 0, steps) == dict(launches=5 * steps, component_steps=5 * steps, merged=0)


@pytest.mark.parametrize("f,l,merged", [(6, 6, True), (7, 6, False), (5, 7, True), (1, 11, True), (1, 12, False)])
def test_plan_merge_limit_of_twelve_ops(f, l, merged):
    g = _graph("L" * f + "H" + "L" * l)
    assert (H.predict(g, 1, 0, g.steps)["merged"] > 0) == merged


def test_plan_segment_of_seventeen_ops():
    g = _graph("L" * 17)
    assert H.segments([nd.light for nd in g.nodes]) == [(0, 16), (16, 1)]
    # two segments: neither a whole-graph launch nor a merged schedule
    assert H.predict(g, 1, 0, g.steps) == dict(launches=2 * g.steps, component_steps=17 * g.steps, merged=0)
    g = _graph("L" * 16)
    assert H.predict(g, 1, 0, g.steps) == dict(launches=1, component_steps=16 * g.steps, merged=0)
    assert H.predict(g, 0, 0, g.steps)["launches"] == 16 * g.steps


def test_plan_whole_graph_chunks():
    g = _graph("LLL", T=21)
    steps = g.steps
    assert H.predict(g, 1, 0, steps, [4, None, 9])["launches"] == -(-steps // 2)   # min(4 - 2, 9 - 2)
    assert H.predict(g, 2, 0, steps, [None, 9, None])["launches"] == -(-steps // 7)
    g.nodes[1].kind = K.KIND_N2O_CHEMISTRY   # keeps three rows (a stratospheric delay of one step)
    g.nodes[1].params = H.default_params(K.KIND_N2O_CHEMISTRY, 4, None)
    assert g.nodes[1].keep_rows == 3
    assert H.predict(g, 1, 0, steps, [None, 6, None])["launches"] == -(-steps // 3)
    assert H.predict(g, 1, 5, 8, [None, 6, None])["launches"] == 1


def test_magicc_chain_counts_in_topological_order():
    """[8 light] ClimateUDEB OceanCarbon [3 light] (scripts/bench_magicc_chain.py, topological order): 3 * steps + 1 launches and
    steps - 1 merged launches (tests/test_gpu_group.py asserts the same on the device)."""
    kinds = [K.KIND_CH4_CHEMISTRY] * 8 + [K.KIND_UDEB, K.KIND_OCEAN_CARBON] + [K.KIND_CO2_BUDGET] * 3
    nodes = []
    for k in kinds:
        nd = H.Node(k, H.default_params(k, 2, None))
        nd.n_rows = len(nd.info.inputs)
        nodes.append(nd)
    g = H.Graph(nodes, 31, 2)
    assert H.predict(g, 1, 0, 30) == dict(launches=3 * 30 + 1, component_steps=13 * 30, merged=29)
    assert H.predict(g, 5, 0, 30)["launches"] == 4 * 30
    assert H.predict(g, 1, 0, 7)["merged"] + H.predict(g, 1, 7, 30)["merged"] == 30 - 2


def test_tie_relation():
    """plan_split's ties: a read at n + 1 of a producer at the same step offset, a read at n of a producer one offset behind; an
    aggregate always reads the end of its step."""
    g = _graph("LLL", links=((1, 0, 0, 1, True), (2, 0, 0, 1, False)))
    t = H.ties(g, [0, 1, 2], [0, 0, 0])
    assert t[0, 1] and t[1, 0] and not t[0, 2] and not t[1, 2]
    t = H.ties(g, [0, 2], [0, 1])   # handle 2 one step ahead reads handle 0's row n + 1 = what 0 writes at offset 0
    assert t[0, 1]
    t = H.ties(g, [0, 1], [0, 1])   # handle 1 reads row n + 2 of handle 0: not written in this launch
    assert not t.any()
