"""GPU tier: member groups on the handle, the grouped select (RSCM_SELECT_GROUPED: csrc/select.hip's kG instantiations) and the
grouped exceedance (csrc/indicators.hip).  For every row and group the result must be exactly what the ungrouped call returns
for an ensemble of that group's members: the oracles are numpy on the subsets -- np.nanquantile(x[:, group == g], q, axis=1), and
with weights method="inverted_cdf" -- and the numpy restatement tests/host_gselect.py, both bit for bit, counts and weights
included.  The data carry no negative zeros except where a test says so (the select orders -0.0 before +0.0, numpy keeps member
order).  Shapes are the smallest at which the kernels can go wrong: member counts around the wavefront, the pair chunk and the
workgroup split, group x target counts below, at and above the 16 LDS histograms of one launch."""
import warnings

import numpy as np
import pytest

from tests import host_resample as hr
from tests.gpu_support import ra  # noqa: F401
from tests.gpu_support import refusal_code
from tests.helpers import f_syn, magicc_chain, same_bits, two_layer_params
from tests.host_gselect import exceedance_grouped, sharded_gquantiles

pytestmark = pytest.mark.gpu

T = np.arange(1750, 1762, dtype=np.float64)            # 12 time points
BOUNDS = np.append(T, T[-1] + 1.0)
STEPS = 10                                             # row 11 lies beyond the time index
SIZES = [1, 2, 3, 63, 64, 65, 511, 513, 4097, 8195]
QS = {1: [0.5], 3: [0.05, 0.5, 0.95], 8: [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0, 1e-12], 9: [0.0, 0.05, 0.17, 0.33, 0.5, 0.67, 0.83, 0.95, 1.0]}
# (n_groups, quantiles, group vector): groups x targets = 2 .. 1152 unweighted, 1 .. 576 weighted; (1, 8) is exactly one launch's 16
COMBOS = [(1, 1, "random"), (1, 8, "interleaved"), (2, 3, "blocks"), (3, 3, "interleaved"), (3, 9, "single"), (5, 3, "empty"),
          (5, 1, "allnan"), (17, 1, "random"), (17, 9, "interleaved"), (64, 3, "blocks"), (64, 9, "random")]
RESTATED = {(2, 3, "blocks"), (3, 3, "interleaved")}    # also against tests/host_gselect.py (slow in Python)


def _two_layer(ra, n, P=None, steps=STEPS, bounds=BOUNDS, forcing=None):
    e = ra.Ensemble(ra.KIND_TWO_LAYER, n, bounds)
    e.set_params(two_layer_params(n) if P is None else P)
    e.set_forcing(f_syn(bounds[:-1]) if forcing is None else forcing)
    e.set_initial(1, 0.0)
    e.set_initial(2, 0.0)
    e.run(steps)
    return e


def _spoil(e, rng, n):
    """NaN members of both signs, +-inf, ties and a row of rounded values (no negative zeros)."""
    for r, frac in ((3, 0.3), (6, 0.6)):
        x = e.get_series(1, r, r + 1)[0]
        x[rng.random(n) < frac] = np.nan if r == 3 else -np.float64(np.nan)
        x[rng.random(n) < 0.05] = rng.choice([np.inf, -np.inf, 0.0, 1.5])
        e.set_state(1, r, x)
    e.set_state(1, 8, np.round(rng.standard_normal(n), 1) + 0.0)


def _groups(kind, rng, n, G):
    if kind == "blocks":
        return (np.arange(n) * G // n).astype(np.int32)
    if kind == "interleaved":
        return (np.arange(n) % G).astype(np.int32)
    if kind == "empty":                                   # the last group has no member
        return rng.integers(-1, max(G - 1, 0), n).astype(np.int32)
    if kind == "single":                                  # the last group has one member
        g = rng.integers(-1, max(G - 1, 0), n).astype(np.int32)
        g[n // 2] = G - 1
        return g
    return rng.integers(-1, G, n).astype(np.int32)        # "random", "allnan"


def _nanq(x, q, w=None):
    """[rows][len(q)] of numpy on one subset; rows without (weighted: positive-weight) members NaN; and the counts / weights."""
    ok = ~np.isnan(x)
    cnt = ok.sum(axis=1) if w is None else (ok * w[None, :]).sum(axis=1)
    out = np.full((x.shape[0], len(q)), np.nan)
    live = cnt > 0
    if live.any():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            if w is None:
                out[live] = np.nanquantile(x[live], q, axis=1).T
            else:
                out[live] = np.nanquantile(x[live], q, axis=1, weights=np.broadcast_to(w, x[live].shape), method="inverted_cdf").T
    return out, cnt


def _want(x, group, G, q, w=None):
    res = [_nanq(x[:, group == g], q, None if w is None else w[group == g]) for g in range(G)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


MODES = [(False, False), (True, False), (False, True), (True, True)]    # (weighted, anomaly)


@pytest.mark.parametrize("n", SIZES)
def test_grouped_select_equals_numpy_on_the_subsets(ra, n):
    rng = np.random.default_rng(4000 + n)
    with _two_layer(ra, n) as e:
        _spoil(e, rng, n)
        w = rng.integers(0, 1 << 30, n, dtype=np.int64)
        w[rng.random(n) < 0.2] = 0
        b = rng.standard_normal(n)
        b[rng.random(n) < 0.05] = np.nan
        e.set_member_weights(w)
        e.set_baseline_values(b)
        for G, nq, kind in COMBOS:
            q, group = QS[nq], _groups(kind, rng, n, G)
            if kind == "allnan":                            # every member of group 0 is NaN in row 4
                x = e.get_series(1, 4, 5)[0]
                x[group == 0] = np.nan
                e.set_state(1, 4, x)
            e.set_member_groups(group, G)
            assert np.array_equal(e.member_groups(), group) and e.n_groups == G
            ser = e.get_series(1, 0, STEPS + 1)
            for weighted, anomaly in MODES:
                got = e.quantile_rows(1, q, weighted=weighted, anomaly=anomaly, grouped=True)
                key = "weight" if weighted else "count"
                assert got["quantiles"].shape == (G, len(T), len(q)) and got[key].shape == (G, len(T))
                x = ser - b[None, :] if anomaly else ser
                want, cnt = _want(x, group, G, q, w if weighted else None)
                what = (n, G, nq, kind, weighted, anomaly)
                assert np.array_equal(got[key][:, :STEPS + 1], cnt), what
                assert same_bits(got["quantiles"][:, :STEPS + 1], want), what
                assert (got[key][:, STEPS + 1:] == 0).all() and np.isnan(got["quantiles"][:, STEPS + 1:]).all(), what
                if (G, nq, kind) in RESTATED:
                    host = sharded_gquantiles([x], [group], G, q, [w] if weighted else None)[0]
                    assert np.array_equal(host[key], cnt) and same_bits(host["quantiles"], want), what
            strided = e.quantile_rows(1, q, 1, 9, 3, grouped=True)
            assert same_bits(strided["quantiles"], _want(ser[1:9:3], group, G, q)[0]), (n, G, nq, kind)


@pytest.mark.parametrize("n", [3, 65, 4097])
def test_one_group_of_all_members_is_the_ungrouped_call(ra, n):
    """Bit for bit, the sign of zeros included (a row of +-0.0)."""
    rng = np.random.default_rng(n)
    with _two_layer(ra, n) as e:
        _spoil(e, rng, n)
        e.set_state(1, 5, rng.choice([-0.0, 0.0], n))
        e.set_member_weights(rng.integers(0, 1 << 20, n, dtype=np.int64))
        e.set_baseline_values(rng.standard_normal(n))
        e.set_member_groups(np.zeros(n, dtype=np.int32), 1)
        for weighted, anomaly in MODES:
            a = e.quantile_rows(1, QS[9], weighted=weighted, anomaly=anomaly, grouped=True)
            p = e.quantile_rows(1, QS[9], weighted=weighted, anomaly=anomaly)
            key = "weight" if weighted else "count"
            assert np.array_equal(a["quantiles"][0].view(np.uint64), p["quantiles"].view(np.uint64)), (weighted, anomaly)
            assert np.array_equal(a[key][0], p[key])
        z = e.quantile_rows(1, [0.0, 1.0], 5, 6, grouped=True)["quantiles"][0, 0]
        if n > 3:
            assert np.signbit(z[0]) and not np.signbit(z[1])


def test_three_contiguous_blocks_equal_three_handles(ra):
    n, sizes = 1201, [513, 65, 623]
    P = two_layer_params(n)
    rng = np.random.default_rng(9)
    w = rng.integers(1, 1 << 30, n, dtype=np.int64)
    group = np.repeat(np.arange(3, dtype=np.int32), sizes)
    with _two_layer(ra, n, P) as e:
        e.set_member_groups(group)                          # n_groups defaults to max + 1
        e.set_member_weights(w)
        assert e.n_groups == 3
        for weighted in (False, True):
            got = e.quantile_rows(1, QS[3], weighted=weighted, grouped=True)
            key = "weight" if weighted else "count"
            for g in range(3):
                with _two_layer(ra, sizes[g], np.ascontiguousarray(P[:, group == g])) as part:
                    part.set_member_weights(w[group == g])
                    one = part.quantile_rows(1, QS[3], weighted=weighted)
                    assert np.array_equal(got["quantiles"][g].view(np.uint64), one["quantiles"].view(np.uint64)), (weighted, g)
                    assert np.array_equal(got[key][g], one[key])


@pytest.mark.parametrize("n", [65, 4097])
def test_grouped_vectors_and_exceedance(ra, n):
    rng = np.random.default_rng(77 + n)
    G = 5
    with _two_layer(ra, n) as e:
        x = e.get_series(1, 7, 8)[0]
        x[rng.random(n) < 0.1] = np.nan                     # members with NaN indicators
        e.set_state(1, 7, x)
        group = _groups("random", rng, n, G)
        w = rng.integers(0, 1 << 40, n, dtype=np.int64)
        e.set_member_groups(group, G)
        e.set_member_weights(w)
        thr = [0.05, 0.2, 0.4]
        ind = e.indicators(1, 1, STEPS + 1, thresholds=thr)
        vecs = [ind["peak"], ind["mean"], e.params_vector(0), e.params_vector(5)]
        host = np.stack([v.to_host() for v in vecs])
        for weighted in (False, True):
            got = e.quantile_vectors(vecs, QS[3], weighted=weighted, grouped=True)
            want, cnt = _want(host, group, G, QS[3], w if weighted else None)
            assert same_bits(got["quantiles"], want) and np.array_equal(got["weight" if weighted else "count"], cnt)
            with e.select_vectors(vecs, QS[3], weighted=weighted, grouped=True) as s:
                while s.next_pass() is not None:
                    s.commit()
                staged = s.result()
            assert same_bits(staged["quantiles"], want)
            exc = e.exceedance(ind["peak"], thr, weighted=weighted, grouped=True)
            hits, total = exceedance_grouped(host[0], group, G, thr, w if weighted else None)
            assert np.array_equal(exc["hits"], hits) and np.array_equal(exc["total"], total)
            assert exc["hits"].dtype == np.int64 and exc["probability"].shape == (G, 3)
            live = total > 0
            assert np.array_equal(exc["probability"][live], hits[live] / total[live, None].astype(np.float64))
            flat = e.exceedance(ind["peak"], thr, weighted=weighted)          # the ungrouped call is unchanged
            keep = group >= 0
            assert flat["total"] - exc["total"].sum() == (w if weighted else np.ones(n, dtype=np.int64))[~keep & ~np.isnan(host[0])].sum()


def test_grouped_exceedance_over_more_members_than_one_grid(ra):
    """300 001 members: every thread of the 1024 workgroups takes a second member, of another group when they interleave."""
    n, G = 300_001, 64
    rng = np.random.default_rng(5)
    with _two_layer(ra, n, steps=1) as e:
        v = e.params_vector(4)
        host = v.to_host()
        w = rng.integers(0, 1 << 33, n, dtype=np.int64)
        e.set_member_weights(w)
        thr = np.quantile(host, [0.1, 0.5, 0.9, 0.99, 0.0, 1.0, 0.3, 0.7])      # eight thresholds
        for kind in ("interleaved", "blocks", "random"):
            group = _groups(kind, rng, n, G)
            e.set_member_groups(group, G)
            for weighted in (False, True):
                exc = e.exceedance(v, thr, weighted=weighted, grouped=True)
                ww = w if weighted else np.ones(n, dtype=np.int64)
                keep = group >= 0
                hits = np.stack([np.bincount(group[keep & (host >= t)], ww[keep & (host >= t)], G) for t in thr], axis=1)
                assert np.array_equal(exc["hits"], hits) and np.array_equal(exc["total"], np.bincount(group[group >= 0], ww[group >= 0], G))


def _staged_sum(sels):
    try:
        sizes = []
        while True:
            bufs = [s.next_pass() for s in sels]
            if bufs[0] is None:
                break
            sizes.append(bufs[0].n)
            total = np.sum([b.to_host() for b in bufs], axis=0)
            for s in sels:
                s.commit(total)
        return [s.result() for s in sels], sizes
    finally:
        for s in sels:
            s.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_two_handles_summing_their_histograms_equal_the_whole(ra, weighted):
    n, cut, G = 1037, 1000, 3
    P = two_layer_params(n)
    rng = np.random.default_rng(31)
    group = np.sort(rng.integers(0, G, n)).astype(np.int32)          # the handle of 37 holds members of the last group only
    group[::11] = -1
    w = rng.integers(0, 1 << 30, n, dtype=np.int64)
    with _two_layer(ra, n, P) as whole, _two_layer(ra, cut, np.ascontiguousarray(P[:, :cut])) as a, \
            _two_layer(ra, n - cut, np.ascontiguousarray(P[:, cut:])) as b:
        for h, sl in ((whole, slice(None)), (a, slice(0, cut)), (b, slice(cut, None))):
            h.set_member_groups(group[sl], G)
            h.set_member_weights(w[sl])
        want = whole.quantile_rows(1, QS[3], weighted=weighted, grouped=True)
        res, sizes = _staged_sum([h.select(1, QS[3], weighted=weighted, grouped=True) for h in (a, b)])
        n_t = 3 if weighted else 6
        assert sizes == [(STEPS + 1) * G * 256] + [(STEPS + 1) * G * n_t * 256] * 7
        for r in res:
            assert np.array_equal(r["quantiles"].view(np.uint64), want["quantiles"].view(np.uint64))
            key = "weight" if weighted else "count"
            assert np.array_equal(r[key], want[key])


def test_windowed_strided_graph_gives_the_full_storage_numbers(ra):
    """GraphModel.set_member_groups / quantile_rows(grouped=True) on a windowed graph that keeps every 12th row equal numpy on
    get_series(t_stride=12) of the group's members, and the same graph on full storage."""
    mod = magicc_chain()
    n, G = 1001, 3
    group = (np.arange(n) % (G + 1) - 1).astype(np.int32)
    names = ["Surface Temperature", "Atmospheric Concentration|CO2"]
    res = {}
    for kw in (dict(series_window=16, output_stride=12), {}):
        model = mod.build_chain(n, 6, "topological", steps_per_year=12, **kw)
        try:
            model.set_member_groups(group, G)
            model.run()
            for name in names:
                got = model.quantile_rows(name, QS[3], t_stride=12, grouped=True)
                ser = model.get_series(name, t_stride=12)
                want, cnt = _want(ser, group, G, QS[3])
                assert same_bits(got["quantiles"], want) and np.array_equal(got["count"], cnt), (name, kw)
                res[(name, bool(kw))] = got["quantiles"]
            peak = model.indicators("Surface Temperature", 0, model.time_index + 1, 12, thresholds=[0.5])["peak"]
            exc = model.exceedance(peak, [0.5], grouped=True)
            hits, total = exceedance_grouped(peak.to_host(), group, G, [0.5])
            assert np.array_equal(exc["hits"], hits) and np.array_equal(exc["total"], total)
            assert same_bits(model.quantile_vectors([peak], QS[3], grouped=True)["quantiles"], _want(peak.to_host()[None, :], group, G, QS[3])[0])
        finally:
            model.close()
    for name in names:
        assert np.array_equal(res[(name, True)].view(np.uint64), res[(name, False)].view(np.uint64))


def test_posterior_sets_the_scenarios_as_groups(ra):
    rng = np.random.default_rng(7)
    N, M, S, K = 500, 201, 3, 4
    w = rng.integers(0, 1 << 33, size=N, dtype=np.int64)
    w[rng.random(N) < 0.5] = 0
    base = f_syn(T)
    scenarios = np.stack([base, np.where(np.arange(len(T)) > K, 2.0 * base, base), np.where(np.arange(len(T)) > K, 0.0, base)])
    with _two_layer(ra, N, steps=K) as src:
        src.set_member_weights(w)
        dst, scen = src.posterior(lambda n: ra.Ensemble(ra.KIND_TWO_LAYER, n, BOUNDS), M, seed=21, scenarios=S)
        with dst:
            assert np.array_equal(scen, np.repeat(np.arange(S), M)) and np.array_equal(dst.member_groups(), scen) and dst.n_groups == S
            dst.set_forcing(scenarios, scen)
            dst.run()
            got = dst.quantile_rows(1, QS[3], grouped=True)
            ser = dst.get_series(1)
            for s in range(S):
                want, cnt = _nanq(ser[:, s * M:(s + 1) * M], QS[3])
                assert same_bits(got["quantiles"][s], want) and np.array_equal(got["count"][s], cnt)
            assert not same_bits(got["quantiles"][0, -1], got["quantiles"][1, -1])
            # a branch leaves the groups set beforehand on the destination alone
            dst.rewind()
            assert np.array_equal(dst.member_groups(), scen)
        with ra.Ensemble(ra.KIND_TWO_LAYER, M, BOUNDS) as other:
            mine = (np.arange(M) % 2).astype(np.int32)
            other.set_member_groups(mine, 2)
            src.branch(other, hr.ancestors(w, M, hr.offset(21, int(w.sum())))[2])
            assert np.array_equal(other.member_groups(), mine) and other.n_groups == 2
            other.set_forcing(base)
            other.run()
            assert np.array_equal(other.member_groups(), mine)
            got = other.quantile_rows(1, QS[3], K, None, grouped=True)
            assert same_bits(got["quantiles"], _want(other.get_series(1, K), mine, 2, QS[3])[0])
            other.clear_member_groups()
            assert other.n_groups == 0


def test_refusals(ra):
    from rscm_amd import RscmGpuError
    from rscm_amd import _lib as L
    n = 101

    def refused(code, fn, *a, **kw):
        with pytest.raises(RscmGpuError) as err:
            fn(*a, **kw)
        assert err.value.code == code, err.value

    with _two_layer(ra, n) as e:
        peak = e.indicators(1, 1, 5)["peak"]
        refused(L.ERR_STATE, e.quantile_rows, 1, [0.5], grouped=True)                   # grouped without groups
        refused(L.ERR_STATE, e.select, 1, [0.5], grouped=True)
        refused(L.ERR_STATE, e.quantile_vectors, [peak], [0.5], grouped=True)
        refused(L.ERR_STATE, e.exceedance, peak, [0.5], grouped=True)
        refused(L.ERR_STATE, e.member_groups)
        good = (np.arange(n) % 3).astype(np.int32)
        e.set_member_groups(good, 3)
        for bad_id in (3, -2):                                                          # an id of n_groups or of -2
            bad = good.copy()
            bad[n - 1] = bad_id
            refused(L.ERR_INVALID, e.set_member_groups, bad, 3)
            assert np.array_equal(e.member_groups(), good) and e.n_groups == 3         # the previous groups are kept
        for G in (0, 65):
            refused(L.ERR_INVALID, e.set_member_groups, np.zeros(n, dtype=np.int32), G)
        assert e.n_groups == 3
        e.set_member_groups(e.member_groups_device(), 64)                               # from device memory; 64 groups are allowed
        assert np.array_equal(e.member_groups(), good) and e.n_groups == 64
        e.set_member_groups(good, 3)
        with e.select(1, [0.5], grouped=True):                                          # set or clear with a select in flight
            refused(L.ERR_STATE, e.set_member_groups, good, 3)
            refused(L.ERR_STATE, e.clear_member_groups)
        e.set_member_groups(good, 3)
        q, out, cnt = np.array([0.5]), np.empty((len(T), 3, 1)), np.empty((len(T), 3))
        rc = e._lib.rscm_ens_quantile_rows_ex(e._h, 1, 0, len(T), 1, 1, L.dptr(q), 8, L.dptr(out), L.dptr(cnt))     # flag value 8
        assert rc == L.ERR_INVALID
        arr, _n = e._vectors([peak])
        rc = e._lib.rscm_ens_quantile_vectors(e._h, 1, arr, 1, L.dptr(q), L.SELECT_GROUPED | L.SELECT_ANOMALY, L.dptr(out), L.dptr(cnt))
        assert rc == L.ERR_INVALID                                                      # anomaly on vectors, with grouped too
        refused(L.ERR_STATE, e.quantile_rows, 1, [0.5], weighted=True, grouped=True)    # weighted without weights
        e.clear_member_groups()
        refused(L.ERR_STATE, e.quantile_rows, 1, [0.5], grouped=True)
        assert e.quantile_rows(1, [0.5])["quantiles"].shape == (len(T), 1)              # the ungrouped call never needed them


def test_a_group_weight_past_2_53_is_refused_on_both_handles(ra):
    """Each handle's weights sum to less than 2^53 and so does every group on its own handle; group 1 of the two together does not."""
    with _two_layer(ra, 101, steps=5) as a, _two_layer(ra, 101, steps=5) as b:
        for h in (a, b):
            w = np.ones(101, dtype=np.int64)
            w[7] = (1 << 52) + 5
            g = np.zeros(101, dtype=np.int32)
            g[7] = 1
            h.set_member_weights(w)
            h.set_member_groups(g, 2)
            assert (h.quantile_rows(1, [0.5], 0, 6, weighted=True, grouped=True)["weight"][1] == (1 << 52) + 5).all()
        sels = [h.select(1, [0.5], 0, 6, weighted=True, grouped=True) for h in (a, b)]
        try:
            total = np.sum([s.next_pass().to_host() for s in sels], axis=0)
            for s in sels:
                assert refusal_code(s.commit, total) == 1
        finally:
            for s in sels:
                s.close()
