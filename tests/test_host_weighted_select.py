"""CPU tier: the weighted radix select of csrc/select.hip, restated in numpy (tests/host_wselect.py), against
numpy.nanquantile(row, q, weights=w, method="inverted_cdf") -- on rows with NaNs, +-inf, ties and zero weights, weights near the
2^53 bound, and shards of one member set split unevenly -- and the C* search against a brute-force minimum."""
import warnings

import numpy as np
import pytest

from tests.helpers import same_values
from tests.host_wselect import HostWSelect, sharded_wquantiles, weight_target

Q = [0.0, 1.0, 0.5, 1e-12, 0.05, 0.95, 0.17, 0.83, 1.0 - 1e-12, 1.0 / 3.0]


def _np_weighted(row, w, q):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.array([np.nanquantile(row, qq, weights=w, method="inverted_cdf") for qq in q])


def _unsign(x):
    """Zeros without their sign (the key order puts -0.0 first; numpy keeps member order), every other bit kept."""
    return np.where(np.asarray(x) == 0, 0.0, x)


def _rows(rng, n):
    neg_nan = -np.float64(np.nan)
    return np.stack([
        1.2 + 1e-3 * rng.standard_normal(n),
        rng.choice([-1.0, 0.0, -0.0, 2.5, 2.5, 7.0], n),
        np.where(rng.random(n) < 0.1, np.nan, rng.standard_normal(n)),
        np.where(rng.random(n) < 0.1, neg_nan, rng.integers(-5, 5, n).astype(np.float64)),
        rng.choice([-np.inf, np.inf, 5e-324, -5e-324, 1e-310, np.nan, 1.0, -1.0], n),
        rng.standard_normal(n) * 1e300,
    ])


def _weights(rng, n, kind):
    if kind == "small":
        w = rng.integers(0, 5, n)
    elif kind == "zeros30":
        w = np.where(rng.random(n) < 0.3, 0, rng.integers(1, 1 << 40, n))
    elif kind == "lead_trail_zero":
        w = rng.integers(1, 100, n)
        w[: n // 4] = 0
        w[-(n // 4):] = 0
    elif kind == "near_bound":                     # the row weights sum to at most 2^53
        w = rng.integers(0, (1 << 53) // n, n)
    else:
        raise ValueError(kind)
    return w.astype(np.int64)


def _check(rows, w, res):
    for r, row in enumerate(rows):
        ok = ~np.isnan(row)
        W = int(w[ok].sum())
        assert res["weight"][r] == W
        got = res["quantiles"][r]
        if W == 0:
            assert np.isnan(got).all()
            continue
        want = _np_weighted(row, w, Q)
        assert np.array_equal(_unsign(got).view(np.uint64), _unsign(want).view(np.uint64)), (r, got, want)
        assert not np.isnan(got).any()


@pytest.mark.parametrize("kind", ["small", "zeros30", "lead_trail_zero", "near_bound"])
@pytest.mark.parametrize("seed", [1, 2])
def test_weighted_select_equals_numpy(kind, seed):
    rng = np.random.default_rng(seed * 10 + len(kind))
    n = 257
    rows, w = _rows(rng, n), _weights(rng, n, kind)
    res = sharded_wquantiles([rows], [w], Q)[0]
    _check(rows, w, res)


def test_zero_weight_rows_and_members():
    rows = np.array([[1.0, 2.0, 3.0, np.nan], [np.nan] * 4, [5.0, 4.0, 3.0, 2.0]])
    w = np.array([0, 0, 0, 7], dtype=np.int64)           # the only weighted member is NaN in row 0
    res = sharded_wquantiles([rows], [w], Q)[0]
    assert res["weight"].tolist() == [0, 0, 7]
    assert np.isnan(res["quantiles"][:2]).all()
    assert (res["quantiles"][2] == 2.0).all()            # a zero-weight member is never returned


def test_unit_and_constant_weights_equal_unweighted_inverted_cdf():
    rng = np.random.default_rng(3)
    rows = _rows(rng, 101)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = np.nanquantile(rows, Q, axis=1, method="inverted_cdf").T
    for k in (1, 7, 1 << 40):
        got = sharded_wquantiles([rows], [np.full(101, k, dtype=np.int64)], Q)[0]["quantiles"]
        assert same_values(_unsign(got), _unsign(want))


@pytest.mark.parametrize("split", [2, 3, 5])
def test_uneven_shards_give_the_same_bits(split):
    rng = np.random.default_rng(40 + split)
    n = 311
    rows, w = _rows(rng, n), _weights(rng, n, "zeros30")
    whole = sharded_wquantiles([rows], [w], Q)[0]
    cuts = np.sort(rng.choice(np.arange(1, n), split - 1, replace=False))
    if split >= 3:
        cuts[0] = 1                                       # a one-member shard
    parts = sharded_wquantiles(np.split(rows, cuts, axis=1), np.split(w, cuts), Q)
    for p in parts:
        assert np.array_equal(p["weight"], whole["weight"])
        assert np.array_equal(p["quantiles"].view(np.uint64), whole["quantiles"].view(np.uint64))
    _check(rows, w, whole)


def test_weight_target_is_the_brute_force_minimum():
    grid = np.unique(np.concatenate([np.linspace(0.0, 1.0, 2001), [1e-300, 1e-16, 1.0 - 1e-16, 0.1, 0.2, 0.3, 0.7]]))
    for W in range(1, 65):
        fracs = np.arange(1, W + 1, dtype=np.float64) / float(W)    # IEEE division, C = 1 .. W
        for q in grid:
            want = int(np.argmax(fracs >= q)) + 1
            assert weight_target(float(q), W) == want, (q, W)
        for C in range(1, W + 1):                                   # the fractions themselves, and their neighbours
            f = float(C) / float(W)
            for q in (f, np.nextafter(f, 0.0), np.nextafter(f, 2.0)):
                if q <= 1.0:
                    assert weight_target(float(q), W) == int(np.argmax(fracs >= q)) + 1


def test_weight_sum_beyond_2_53_is_refused():
    """A handle's weights may sum to 2^53 at most (refused when it takes them); shards that each hold less can still sum to more,
    which the first commit reports."""
    rows = np.array([[1.0, 2.0]])
    with pytest.raises(ValueError):
        HostWSelect(rows, np.array([1 << 52, (1 << 52) + 1]), [0.5])
    HostWSelect(rows, np.array([1 << 52, 1 << 52]), [0.5])                  # exactly 2^53
    with pytest.raises(ValueError):
        HostWSelect(rows, np.array([1, -1]), [0.5])
    shards = [HostWSelect(rows[:, :1], np.array([(1 << 52) + 1]), [0.5]), HostWSelect(rows[:, 1:], np.array([1 << 52]), [0.5])]
    total = np.sum([x.next_pass() for x in shards], axis=0)
    for x in shards:
        with pytest.raises(ValueError):
            x.commit(total)


def test_weights_that_would_wrap_64_bit_bins_are_refused():
    """Weights whose sum wraps in 64 bits (two near 2^63 and a small one on members in one bin) are refused, not summed to a
    small wrong W."""
    rows = np.array([[1.0, 1.0 + 2**-40, 1.0 + 2**-39]])
    with pytest.raises(ValueError):
        HostWSelect(rows, np.array([2**63 - 1, 2**63 - 1, 3]), [0.5])
    with pytest.raises(ValueError):                                          # bins of 2^11 members of 2^53 each
        HostWSelect(np.ones((1, 2048)), np.full(2048, 1 << 53), [0.5])
