"""CPU tier: the numpy restatement of the grouped radix select (tests/host_gselect.py) against numpy on the group subsets --
np.nanquantile(x[:, group == g], q, axis=1), bit for bit -- over shards, with a group absent from a shard, and in the weighted form
against nanquantile(..., weights=, method="inverted_cdf").

The data carry no negative zeros: the select orders -0.0 before +0.0 where numpy keeps member order, the documented signed-zero
case.  (np.round leaves -0.0 behind; a rounded row has + 0.0 added to it.)"""
import warnings

import numpy as np
import pytest

from tests.helpers import same_bits
from tests.host_gselect import HostGSelect, exceedance_grouped, sharded_gquantiles
from tests.host_select import HostSelect

Q = [0.0, 0.05, 0.5, 0.95, 1.0, 1e-12]
SIZES = [1, 2, 3, 65, 4099]


def _rows(rng, n):
    """[5][n] without negative zeros: clustered, rounded with ties, NaNs of both signs, all NaN, +-inf."""
    rows = np.stack([1.2 + 1e-3 * rng.standard_normal(n),
                     np.round(rng.standard_normal(n), 1) + 0.0,
                     np.where(rng.random(n) < 0.3, np.nan, np.where(rng.random(n) < 0.3, -np.float64(np.nan), rng.standard_normal(n))),
                     np.full(n, np.nan),
                     rng.choice([-np.inf, np.inf, 0.0, 1.0, 5e-324], n)])
    assert not (np.signbit(rows) & (rows == 0)).any()
    return rows


def _groups(rng, n, G):
    """Random ids with -1 among them; the last group stays empty when there is more than one."""
    return rng.integers(-1, max(G - 1, 1), n)


def _nanq(x, q=Q):
    if x.shape[1] == 0:
        return np.full((x.shape[0], len(q)), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(x, q, axis=1).T


def _want(rows, group, G):
    return (np.stack([_nanq(rows[:, group == g]) for g in range(G)]),
            np.stack([(~np.isnan(rows[:, group == g])).sum(axis=1) for g in range(G)]))


@pytest.mark.parametrize("n", SIZES)
def test_subset_through_host_select_is_numpy_once_rounding_leaves_no_negative_zero(n):
    rng = np.random.default_rng(100 + n)
    rows = _rows(rng, n)
    s = HostSelect(rows, Q)
    while s.next_pass() is not None:
        s.commit()
    assert same_bits(s.result()["quantiles"], _nanq(rows))
    raw = np.round(rng.standard_normal((1, 4099)) * 0.04, 1)       # about a third of its zeros are -0.0 without the + 0.0
    assert (np.signbit(raw) & (raw == 0)).any() and not (np.signbit(raw + 0.0) & (raw == 0)).any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("G", [1, 3, 17, 64])
def test_grouped_restatement_equals_numpy_on_the_subsets(n, G):
    rng = np.random.default_rng(1000 * G + n)
    rows, group = _rows(rng, n), _groups(rng, n, G)
    res = sharded_gquantiles([rows], [group], G, Q)[0]
    want, count = _want(rows, group, G)
    assert res["quantiles"].shape == (G, rows.shape[0], len(Q))
    assert same_bits(res["quantiles"], want) and np.array_equal(res["count"], count)
    if G > 1:
        assert (res["count"][G - 1] == 0).all() and np.isnan(res["quantiles"][G - 1]).all()   # the empty group


def test_buffer_layouts():
    rng = np.random.default_rng(3)
    rows, group = _rows(rng, 65), _groups(rng, 65, 5)
    s = HostGSelect(rows, group, 5, Q)
    h = s.next_pass()
    assert h.dtype == np.int64 and h.size == 5 * 5 * 256
    assert np.array_equal(h.reshape(5, 5, 256).sum(axis=2).T, _want(rows, group, 5)[1])
    s.commit()
    assert s.next_pass().size == 5 * 5 * 2 * len(Q) * 256


@pytest.mark.parametrize("n", [3, 65, 4099])
@pytest.mark.parametrize("weighted", [False, True])
def test_sharded_composition_with_a_group_absent_from_a_shard(n, weighted):
    rng = np.random.default_rng(7 * n + weighted)
    G = 4
    rows = _rows(rng, n)
    group = np.sort(rng.integers(0, G - 1, n))          # contiguous blocks: the first shard holds no member of the later groups
    group[rng.random(n) < 0.1] = -1
    w = rng.integers(0, 1 << 30, n, dtype=np.int64) if weighted else None
    whole = sharded_gquantiles([rows], [group], G, Q, None if w is None else [w])[0]
    for _ in range(4):
        cuts = np.sort(rng.integers(0, n + 1, 2))
        idx = np.split(np.arange(n), cuts)
        parts = sharded_gquantiles([rows[:, i] for i in idx], [group[i] for i in idx], G, Q, None if w is None else [w[i] for i in idx])
        for p in parts:
            for k in whole:
                assert same_bits(p[k], whole[k]) if k == "quantiles" else np.array_equal(p[k], whole[k])
    if not weighted:
        assert same_bits(whole["quantiles"], _want(rows, group, G)[0])


@pytest.mark.parametrize("n", [2, 65, 4099])
def test_weighted_form_equals_numpy_inverted_cdf(n):
    rng = np.random.default_rng(50 + n)
    G = 3
    rows, group = _rows(rng, n), _groups(rng, n, G + 1)
    w = rng.integers(0, 1 << 30, n, dtype=np.int64)
    res = sharded_gquantiles([rows], [group], G, Q, [w])[0]
    for g in range(G):
        sub, ws = rows[:, group == g], w[group == g]
        W = ((~np.isnan(sub)) * ws[None, :]).sum(axis=1)
        assert np.array_equal(res["weight"][g], W)
        want = np.full((rows.shape[0], len(Q)), np.nan)
        live = W > 0
        if live.any():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want[live] = np.nanquantile(sub[live], Q, axis=1, weights=np.broadcast_to(ws, sub[live].shape), method="inverted_cdf").T
        assert same_bits(res["quantiles"][g], want)


def test_group_weight_past_2_53_is_refused_at_the_first_commit():
    rows = np.arange(4.0).reshape(1, 4)
    a = HostGSelect(rows, [0, 0, 1, 1], 2, [0.5], w=[1 << 52, 1 << 51, 1, 1])
    b = HostGSelect(rows, [0, 1, 1, 1], 2, [0.5], w=[1 << 52, 1, 1, 1])
    total = a.next_pass() + b.next_pass()
    for s in (a, b):
        with pytest.raises(ValueError, match="2\\^53"):
            s.commit(total)


def test_bad_groups_and_exceedance():
    with pytest.raises(ValueError):
        HostGSelect(np.zeros((1, 2)), [0, 2], 2, [0.5])
    with pytest.raises(ValueError):
        HostGSelect(np.zeros((1, 2)), [0, -2], 2, [0.5])
    with pytest.raises(ValueError):
        HostGSelect(np.zeros((1, 2)), [0, 0], 65, [0.5])
    v = np.array([1.0, np.nan, 2.0, 3.0, 0.5])
    hits, total = exceedance_grouped(v, [0, 0, 1, 1, -1], 3, [1.0, 2.5], w=[1 << 52, 5, 1 << 52, 1 << 52, 9])
    assert hits.tolist() == [[1 << 52, 0], [1 << 53, 1 << 52], [0, 0]] and total.tolist() == [1 << 52, 1 << 53, 0]
