"""CPU tier: the staged radix select of csrc/select.hip, restated in numpy (tests/host_select.py), against numpy.nanquantile on
shards of one member set split 1 to 5 ways -- the algorithm pinned before the GPU runs it."""
import numpy as np
import pytest

from tests.helpers import same_values
from tests.host_select import HostSelect, key_value, order_keys, sharded_quantiles

Q = [0.0, 1.0, 0.5, 1e-12, 0.05, 0.95, 0.17, 0.83]


def _adversarial_rows(rng, n):
    """[rows][n]: clustered values, ties, +-inf, +-0, denormals, NaNs of both signs, an all-NaN row and rows with one member."""
    neg_nan = -np.float64(np.nan)
    rows = [
        1.2 + 1e-3 * rng.standard_normal(n),                          # a plume row: every key shares its top digits
        rng.choice([-1.0, 0.0, 2.5, 2.5, 7.0], n),                    # ties
        np.where(rng.random(n) < 0.2, np.nan, rng.standard_normal(n)),
        np.where(rng.random(n) < 0.2, neg_nan, rng.standard_normal(n)),
        rng.choice([-np.inf, np.inf, -0.0, 0.0, 5e-324, -5e-324, 1e-310, np.nan, neg_nan], n),
        np.full(n, np.nan),                                           # every member NaN
        np.where(np.arange(n) == n // 2, 3.0, np.nan),                # one member that is not NaN
        rng.choice([-0.0, 0.0], n),
        rng.standard_normal(n) * 1e300,
    ]
    return np.stack(rows)


def _nanq(rows, q):
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning) if np.isnan(rows).all(axis=1).any() else _nullctx():
        return np.nanquantile(rows, q, axis=1).T


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_key_map_orders_like_the_radix_sort():
    x = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf])
    k, ok = order_keys(x)
    assert ok.all() and (np.diff(k.astype(object)) > 0).all()          # strictly increasing: -0.0 before +0.0
    for v, kk in zip(x, k):
        assert np.float64(key_value(kk)).view(np.uint64) == v.view(np.uint64)
    assert not order_keys(np.array([np.nan, -np.float64(np.nan)]))[1].any()


@pytest.mark.parametrize("split", [1, 2, 3, 5])
def test_sharded_select_equals_nanquantile(split):
    rng = np.random.default_rng(100 + split)
    n = 397
    rows = _adversarial_rows(rng, n)
    cuts = np.sort(rng.choice(np.arange(1, n), split - 1, replace=False)) if split > 1 else []
    shards = np.split(rows, cuts, axis=1)
    if split >= 3:   # one shard with a single member, one whose members are all NaN
        shards[0] = rows[:, :1]
        shards[1] = np.full((rows.shape[0], 7), np.nan)
        rows = np.concatenate(shards, axis=1)
    res = sharded_quantiles(shards, Q)
    want = _nanq(rows, Q)
    for r in res:                                                      # every shard ends with the same numbers
        assert same_values(r["quantiles"], want)
        assert np.array_equal(r["count"], (~np.isnan(rows)).sum(axis=1))
        assert np.array_equal(r["quantiles"].view(np.uint64), res[0]["quantiles"].view(np.uint64))


def test_split_does_not_change_a_bit():
    """The key order decides between -0.0 and +0.0 where numpy's partition may not: the split must not."""
    rng = np.random.default_rng(7)
    rows = _adversarial_rows(rng, 200)
    whole = sharded_quantiles([rows], Q)[0]["quantiles"]
    for split in (2, 4, 5):
        cuts = np.sort(rng.choice(np.arange(1, 200), split - 1, replace=False))
        got = sharded_quantiles(np.split(rows, cuts, axis=1), Q)[0]["quantiles"]
        assert np.array_equal(got.view(np.uint64), whole.view(np.uint64))


def test_minus_zero_orders_before_plus_zero():
    r = sharded_quantiles([np.array([[0.0, -0.0, 0.0]])], [0.0, 0.5, 1.0])[0]["quantiles"][0]
    assert np.signbit(r[0]) and not np.signbit(r[1]) and not np.signbit(r[2])


def test_no_rows_and_bad_quantiles():
    s = HostSelect(np.empty((0, 5)), [0.5])
    assert s.next_pass() is None
    with pytest.raises(ValueError):
        HostSelect(np.zeros((1, 3)), [1.5])
