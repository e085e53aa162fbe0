"""CPU tier of tests/host_reduce.py: the generators and the bound that tests/test_gpu_reduction_edges.py holds the device to are
proved here, without a GPU -- an exactly summable row has one sum in every order, the bound derived from the kernels' addition tree
holds for a restatement of that tree, and it does not hold for a restatement that loses the members beyond one grid."""
import math

import numpy as np
import pytest

from tests import host_reduce as hd

SIZES = [1, 63, 64, 65, 255, 256, 257, 262_143, 262_144, 262_145, 262_144 + 257, 600_001]


def _bits(x: float) -> int:
    return int(np.float64(x).view(np.uint64))


def test_block_count_and_depth_follow_the_launch_shape():
    assert [hd.summary_blocks(n) for n in (1, 256, 257, 262_144, 262_145, 600_001)] == [1, 1, 2, 1024, 1024, 1024]
    # one block: one serial term and one partial; the cap: four partials per thread of the final kernel; beyond it: more strides
    assert hd.additions_depth(1) == hd.additions_depth(256) == (1 + 9) + (1 + 9)
    assert hd.additions_depth(257) == (1 + 9) + (1 + 9) and hd.additions_depth(256 * 257) == (1 + 9) + (2 + 9)
    assert hd.additions_depth(262_144) == (1 + 9) + (4 + 9)
    assert hd.additions_depth(262_145) == hd.additions_depth(2 * 262_144) == (2 + 9) + (4 + 9)
    assert hd.additions_depth(600_001) == (3 + 9) + (4 + 9)


@pytest.mark.parametrize("n", [1, 65, 257, 262_145, 600_001, 1 << 21])
def test_an_exactly_summable_row_has_one_sum_in_every_order(n):
    rng = np.random.default_rng(n)
    x = hd.exact_row(rng, n)
    k = x * 2.0 ** 20
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() < 2 ** 20
    want = math.fsum(x)
    assert want == int(k.astype(np.int64).sum()) / 2 ** 20          # the integer sum, exactly
    for _ in range(3):
        p = rng.permutation(x)
        assert _bits(float(np.add.reduce(p))) == _bits(want)         # numpy's blocked pairwise order
        assert _bits(float(np.cumsum(p)[-1])) == _bits(want)         # strictly left to right
        assert _bits(hd.pairwise_sum(p)) == _bits(want)
    assert _bits(hd.pairwise_sum(x)) == _bits(want)
    if n < 1 << 21:
        assert _bits(hd.device_tree_sum(x)) == _bits(want)            # the kernels' own tree


@pytest.mark.parametrize("n", SIZES)
def test_the_derived_bound_holds_for_the_kernels_tree(n):
    rng = np.random.default_rng(1000 + n)
    x = hd.ill_conditioned_row(rng, n)
    assert x.size == n and np.isfinite(x).all()
    cnt, want, mn, mx = hd.summary(x)
    mag = math.fsum(np.abs(x))
    assert cnt == n and (mn, mx) == (x.min(), x.max())
    assert abs(want) < 4.0                                           # the remainder is the exact sum ...
    if n >= 3:
        assert mag >= 2e300 and abs(want) < 1e-299 * mag             # ... and tiny next to the magnitudes
    bound = hd.sum_bound(x)
    assert bound == hd.additions_depth(n) * hd.U * mag / (1.0 - hd.additions_depth(n) * hd.U)
    got = hd.device_tree_sum(x)
    print(n, "D", hd.additions_depth(n), "error", abs(got - want), "bound", bound)
    assert abs(got - want) <= bound
    e = hd.exact_row(rng, n)
    assert _bits(hd.device_tree_sum(e)) == _bits(math.fsum(e))       # the same tree on an exact row: fsum's bits at every size


@pytest.mark.parametrize("n", [262_145, 262_144 + 257, 600_001])
def test_a_tree_that_drops_the_second_stride_is_outside_the_bound(n):
    rng = np.random.default_rng(2000 + n)
    x = hd.ill_conditioned_row(rng, n)
    want, bound = math.fsum(x), hd.sum_bound(x)
    assert abs(hd.device_tree_sum(x) - want) <= bound
    lost = hd.device_tree_sum(x, passes=1)
    assert abs(lost - want) > 1e9 * bound                             # off by the last member's partner, 1e300
    e = hd.exact_row(rng, n)
    assert _bits(hd.device_tree_sum(e)) == _bits(math.fsum(e)) != _bits(hd.device_tree_sum(e, passes=1))


def test_non_finite_members_are_skipped_by_the_reference_and_the_tree():
    rng = np.random.default_rng(5)
    x = hd.exact_row(rng, 300_001)
    keep = x.copy()
    x[hd.ONE_GRID:] = np.resize([np.nan, np.inf, -np.inf], x.size - hd.ONE_GRID)
    x[256:512] = np.nan
    keep[hd.ONE_GRID:] = 0.0
    keep[256:512] = 0.0
    cnt, s, mn, mx = hd.summary(x)
    assert cnt == hd.ONE_GRID - 256 and _bits(s) == _bits(math.fsum(keep)) == _bits(hd.device_tree_sum(x))
    assert (mn, mx) == (np.nanmin(np.where(np.isfinite(x), x, np.nan)), np.nanmax(np.where(np.isfinite(x), x, np.nan)))
    assert hd.summary(np.full(65, np.nan)) == (0, 0.0, math.inf, -math.inf)
    assert hd.summary([np.inf, -np.inf, np.nan]) == (0, 0.0, math.inf, -math.inf)


def test_likelihood_references():
    ll = np.array([1.0, 7.0, np.inf, np.nan, -np.inf, 3.0, 2.0])
    status = np.array([0, 1, 0, 0, 0, 0, 0], dtype=np.uint8)
    assert hd.loglik_ok(ll, status).tolist() == [True, False, False, False, False, True, True]
    assert hd.loglik_max(ll, status) == 3.0
    assert hd.loglik_max(ll, np.ones(7, dtype=np.uint8)) == -math.inf
    w = hd.weights_from_loglik(ll, status, 3.0, 10)
    assert w.tolist() == [float(np.rint(math.exp(-2.0) * 1024)), 0.0, 0.0, 0.0, 0.0, 1024.0, float(np.rint(math.exp(-1.0) * 1024))]
    assert hd.weights_from_loglik(ll, status, 2.0, 4)[5] == 16.0     # above the given max: clamped to 2^bits
